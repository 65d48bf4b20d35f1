// The row collapse (row_collapse.hip) as pure computations on sizes: whether a collapse runs at all, the route its sort takes, the
// layout of the `info` block, the element count of every temporary buffer, the radix sort's bit range, the merge rounds and the
// grid and block of every launch of the chain, in launch order — for the group matrices and the EM problems alike.  Plain C++17,
// no HIP types, no getenv: a CPU test reaches every decision (tests/cpp/collapse_plan_check.cpp).
#ifndef RPVG_COLLAPSE_PLAN_HPP
#define RPVG_COLLAPSE_PLAN_HPP

#include "segment_sort_plan.hpp"

#include <algorithm>
#include <cstdint>

namespace rpvg_collapse {

// the fields of the sort key (collapseSortKey, common.hpp; row_collapse.hip asserts that these restate them)
constexpr int kKeyLargestBits = 20;
constexpr int kKeyMatrixShift = 44;
constexpr uint32_t kMaxMatrices = 1u << 20;        // the matrix field; the EM problems need one index more, for their unused row slots
constexpr uint64_t kMaxTotalRows = 0x7fffffffull;  // rows and sorted positions are 32-bit, and the library sorts count in int
constexpr int kCsrCellHashBits = 8;  // of the sort key's low field, for the rows of EM problems (CsrArrays)

constexpr uint32_t kSortThreads = 256;  // (1 024 in rounds 2-3: sixteen waves' worth of registers to find on one CU before the kernel could even see that it has no big list)
constexpr uint32_t kBetweenThreads = 256;
constexpr uint32_t kBetweenRows = 2 * kBetweenThreads;  // rows of a matrix per work item of step b
constexpr uint64_t kPairTableBytes = 16ull << 20;
constexpr uint32_t kSmallSortThreads = rpvg_sort::kSmallSortWaves * rpvg_sort::kWaveLanes;
constexpr uint32_t kChunkSortThreads = rpvg_sort::kChunkWaves * rpvg_sort::kWaveLanes;
constexpr uint32_t kMergeThreads = 128;
constexpr uint32_t kPairCapacityMax = 0x20000000u;

// ---- the info block -----------------------------------------------------------------------------------------------------------
// [counters | zeroed words | active bytes | list sizes], 32-bit words.  The first kInfoWords are what the callers read back:
enum : uint32_t { kInfoMatrices = 0, kInfoRowsReplaced = 1, kInfoWholeMatrices = 2, kInfoActiveRows = 3, kInfoPairsEquivalent = 4, kInfoPairsApart = 5, kInfoWords = 6 };

// Word offsets of the regions, in their order.  One memset clears [0, zeroed_words); the list sizes behind are written by the
// list kernel.
struct InfoLayout {
    static constexpr uint64_t info = 0;  // [kInfoWords], whatever the sizes
    uint64_t pair_bytes = 0;      // [2] the pair tables' byte counter: 8 bytes, on an 8-byte boundary
    uint64_t mat_flag = 0;        // [M]
    uint64_t replay_list = 0;     // [M + 1] the matrices with a list, then their number
    uint64_t marked_bits = 0;     // [mark_words] a bit per row
    uint64_t marked_count = 0;    // the five counters: the marked list,
    uint64_t pair_counts = 0;     //   [2] the forward and the around pair lists,
    uint64_t between_count = 0;   //   the between items,
    uint64_t row_item_count = 0;  //   the row items
    uint64_t active = 0;          // [active_words] a byte per row
    uint64_t mat_list = 0;        // [M] list sizes
    uint64_t mark_words = 0, active_words = 0;
    uint64_t zeroed_words = 0, total_words = 0;
};

inline InfoLayout infoLayout(const uint32_t M, const uint64_t total_rows) {
    InfoLayout l;
    l.mark_words = (total_rows + 31) / 32;
    l.active_words = (total_rows + 3) / 4;
    l.pair_bytes = InfoLayout::info + kInfoWords;
    l.mat_flag = l.pair_bytes + 2;
    l.replay_list = l.mat_flag + M;
    l.marked_bits = l.replay_list + M + 1;
    l.marked_count = l.marked_bits + l.mark_words;
    l.pair_counts = l.marked_count + 1;
    l.between_count = l.pair_counts + 2;
    l.row_item_count = l.between_count + 1;
    l.active = l.row_item_count + 1;
    l.mat_list = l.active + l.active_words;
    l.zeroed_words = l.mat_list;
    l.total_words = l.mat_list + M;
    return l;
}

// ---- the hand-written segment sort (stage 0) ----------------------------------------------------------------------------------
struct Launch {
    uint32_t grid = 0, block = 0;  // grid 0: not launched on this route
};
inline bool operator==(const Launch & a, const Launch & b) { return a.grid == b.grid && a.block == b.block; }

// The launches of the segment sort: the small kernel over all segments; for the segments beyond it — a few dozen per batch —
// the chunks of their list, the merge rounds and their positions.  The host does not know every segment's rows (the EM
// problems' kept rows are counted on the device): it launches the rounds the largest segment its bound allows would need, and a
// round in which no segment has work is a dispatch and nothing else.  With no such segment possible, nothing.
struct SegmentSortPlan {
    uint32_t chunk_capacity = 0;  // (segment, chunk) entries of the chunk list
    uint32_t merge_rounds = 0;
    Launch small_sort, chunk_sort, merge_round, merged_positions;  // merge_round: launched merge_rounds times
};

inline uint32_t segmentSortChunkCapacity(const uint64_t total_rows, const uint32_t M) {
    return static_cast<uint32_t>(std::min<uint64_t>(total_rows / rpvg_sort::kChunkRows + M + 1, 0x7fffffffull));
}

inline SegmentSortPlan planSegmentSort(const uint32_t M, const uint64_t total_rows, const uint64_t max_segment_rows, const uint32_t small_grid) {
    SegmentSortPlan s;
    s.chunk_capacity = segmentSortChunkCapacity(total_rows, M);
    const uint32_t pairs = (M + rpvg_sort::kSmallSortWaves - 1) / rpvg_sort::kSmallSortWaves;
    s.small_sort = Launch{std::max<uint32_t>(1, std::min<uint32_t>(pairs, 16 * small_grid)), kSmallSortThreads};
    if (max_segment_rows <= rpvg_sort::kSmallSortRows) return s;
    s.chunk_sort = Launch{4 * small_grid, kChunkSortThreads};
    s.merge_rounds = rpvg_sort::mergeRoundsOf(max_segment_rows);
    if (s.merge_rounds > 0) s.merge_round = Launch{8 * small_grid, kMergeThreads};
    s.merged_positions = Launch{4 * small_grid, 256};
    return s;
}

// ---- the plan of a collapse ---------------------------------------------------------------------------------------------------
struct CollapseShape {
    uint32_t M = 0;                 // matrices; EM problems: the bound of their number
    uint64_t total_rows = 0;        // row slots
    uint64_t max_segment_rows = 0;  // a bound of the rows of the longest segment: 0 = unknown
    int hash_bits = 0;              // of the row view: 0 (group matrices) or kCsrCellHashBits (EM problems)
    bool caller_keys = false;       // group matrices: the build wrote the keys; EM problems: the sort computes them
    uint32_t num_items_bound = 0;   // EM problems: the work items of the fill
    uint32_t cus = 0;
};

// the experiment switches of the collapse (docs/design/knobs.md; all off in the shipped library)
struct CollapseKnobs {
    bool library_sort_matrices = false, library_sort_problems = false;  // RPVG_HIP_COLLAPSE_LIBRARY_SORT = 1 | matrices | problems
    uint32_t small_grid = 256;   // RPVG_HIP_COLLAPSE_GRID
    bool no_lds_tables = false;  // RPVG_HIP_COLLAPSE_NO_LDS_TABLES
    bool debug = false;          // RPVG_HIP_EM_COLLAPSE_DEBUG
};

enum Verdict { kRun = 0, kNothingToDo = 1, kTooLarge = 2 };
// The sort of the rows, segment by segment, on (projection[, hash]):
//   HandSort          the segment sort in registers (segment_sort_plan.hpp), for segments of fewer than 2^20 rows
//   LibraryGlobal     group matrices beyond that: ONE stable radix sort of the whole array on the projection and as many matrix bits as
//                     there are matrices
//   LibrarySegmented  EM problems beyond that: the keys kernel, then the library's segmented radix sort, a segment per problem
enum Route { HandSort = 0, LibraryGlobal = 1, LibrarySegmented = 2 };

// element counts of the temporary buffers (0: not needed on this route)
struct BufferCounts {
    uint64_t sorted_key = 0, sorted_row = 0;
    uint64_t order = 0, head = 0, pair_column = 0, pair_bound = 0, pair_pattern = 0, marked_list = 0, pairs = 0, between_items = 0, row_items = 0,
             list_index = 0, pair_base = 0, pair_table = 0;
    uint64_t bytes = 0;    // same_prev, close, barrier: total_rows each
    uint64_t stretch = 0;  // stretch starts by position, their running maximum, stretch ends, positions by row: total_rows each
    uint64_t words = 0, chunks = 0, chunk_count = 0;       // HandSort: each of the two word buffers, the chunk list, its counter
    uint64_t keys = 0, rows = 0, segments = 0;             // LibrarySegmented: what the keys kernel writes (segments: begins [M], ends [M])
    uint64_t pattern = 0;                                  // EM problems: the zero pattern of every row slot
};

struct CollapsePlan {
    Verdict verdict = kNothingToDo;
    uint32_t M = 0;           // of the shape
    uint64_t total_rows = 0;
    Route route = HandSort;
    InfoLayout info;
    BufferCounts counts;
    uint32_t pair_capacity = 0;
    int matrix_bits = 0, begin_bit = 0, end_bit = 0;  // the library sorts' bit range
    SegmentSortPlan segment_sort;                     // HandSort
    // The launches in their order.  The kernels over pairs, lists and matrices with a list draw their (few) items from device-side
    // counts with grid-stride loops: a workgroup per CU or two, not thousands that find nothing (a workgroup costs the dispatcher
    // ~40 ns whatever it does: 4 096 of them were most of a 60 us kernel).
    Launch keys;          // LibrarySegmented
    Launch unused_slots;  // HandSort on EM problems (then segment_sort's launches)
    Launch same_prev;     // the library routes (the hand sort writes what it writes itself)
    Launch stretch_end, forward_pairs, mark_pairs, around_pairs, active_pairs;
    Launch list, pair_table, rank, list_sort, between, runs;
    Launch adjust_sums, rewrite;  // the held-back stage of the group matrices
};

inline CollapsePlan planCollapse(const CollapseShape & s, const CollapseKnobs & knobs) {
    CollapsePlan p;
    const uint32_t M = s.M;
    const uint64_t T = s.total_rows;
    p.M = M;
    p.total_rows = T;
    if (M == 0 || T == 0) return p;
    p.verdict = (T > kMaxTotalRows || (s.caller_keys ? M : M + 1) >= kMaxMatrices) ? kTooLarge : kRun;
    if (p.verdict != kRun) return p;
    const bool library_sort = s.caller_keys ? knobs.library_sort_matrices : knobs.library_sort_problems;
    p.route = !library_sort && s.max_segment_rows > 0 && s.max_segment_rows <= rpvg_sort::kMaxSegmentRows ? HandSort
              : s.caller_keys ? LibraryGlobal : LibrarySegmented;
    p.info = infoLayout(M, T);
    p.pair_capacity = static_cast<uint32_t>(std::min<uint64_t>(4 * T + 4096, kPairCapacityMax));

    BufferCounts & c = p.counts;
    c.sorted_key = c.sorted_row = T;
    c.order = 2 * T;
    c.head = T;
    c.pair_column = T;
    c.pair_bound = 2 * T;
    c.pair_pattern = T;
    c.marked_list = T;
    c.pairs = 2 * static_cast<uint64_t>(p.pair_capacity);
    c.between_items = 2 * (T / kBetweenRows + M);
    c.row_items = 2 * T;
    c.list_index = T;
    c.pair_base = M;
    c.pair_table = kPairTableBytes;
    c.bytes = 3 * T;
    c.stretch = 4 * T;
    c.pattern = s.caller_keys ? 0 : T;

    // (+ 1: the index unused row slots of the EM problems carry)
    p.matrix_bits = 1;
    while ((1u << p.matrix_bits) < M + 1) ++p.matrix_bits;
    p.begin_bit = kKeyLargestBits - s.hash_bits;
    p.end_bit = p.route == LibrarySegmented ? kKeyMatrixShift : kKeyMatrixShift + p.matrix_bits;

    const uint32_t small_grid = knobs.small_grid;
    const uint32_t row_blocks = static_cast<uint32_t>((T + 255) / 256);
    if (p.route == HandSort) {
        p.segment_sort = planSegmentSort(M, T, s.max_segment_rows, small_grid);
        c.words = T;
        c.chunks = 2 * static_cast<uint64_t>(p.segment_sort.chunk_capacity);
        c.chunk_count = 1;
        if (s.hash_bits) p.unused_slots = Launch{std::max<uint32_t>(1, std::min<uint32_t>(s.num_items_bound, 8 * small_grid)), 256};
    } else {
        if (p.route == LibrarySegmented) {
            c.keys = c.rows = T;
            c.segments = 2 * static_cast<uint64_t>(M);
            p.keys = Launch{std::max<uint32_t>(1, std::min<uint32_t>(s.num_items_bound, s.cus * 8)), 256};
        }
        p.same_prev = Launch{row_blocks, 256};
    }
    p.stretch_end = p.forward_pairs = Launch{row_blocks, 256};
    p.mark_pairs = Launch{small_grid, 64};
    p.around_pairs = Launch{256, 64};
    p.active_pairs = Launch{small_grid, 64};
    p.list = Launch{std::min<uint32_t>(M, small_grid), 256};
    p.pair_table = Launch{small_grid, 64};
    p.rank = Launch{small_grid, 256};
    p.list_sort = Launch{std::min<uint32_t>(M, 32), kSortThreads};
    p.between = Launch{2 * small_grid, kBetweenThreads};
    p.runs = Launch{small_grid, 256};
    p.adjust_sums = Launch{4 * small_grid, 256};
    p.rewrite = Launch{small_grid, 256};
    return p;
}

}  // namespace rpvg_collapse

#endif
