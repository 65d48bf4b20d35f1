// The plan of the row collapse (rpvg_amd/csrc/collapse_plan.hpp) against the arithmetic the launch code carried before it had a
// plan, written out here literally: refusals, route, the info block, the buffer counts, the radix sort's bits, the merge rounds and
// every launch — over a grid of shapes and at the edges of every formula.  Plain C++17; built with -fsanitize=address,undefined.
// Prints "ok".
#include "collapse_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace rpvg_collapse;

static CollapseShape matrices(const uint32_t M, const uint64_t total_rows, const uint64_t longest) {
    CollapseShape s;
    s.M = M;
    s.total_rows = total_rows;
    s.max_segment_rows = longest;
    s.hash_bits = 0;
    s.caller_keys = true;
    return s;
}
static CollapseShape problems(const uint32_t P, const uint64_t total_rows, const uint64_t longest, const uint32_t items = 1000, const uint32_t cus = 256) {
    CollapseShape s;
    s.M = P;
    s.total_rows = total_rows;
    s.max_segment_rows = longest;
    s.hash_bits = kCsrCellHashBits;
    s.caller_keys = false;
    s.num_items_bound = items;
    s.cus = cus;
    return s;
}

static void requireLaunch(const Launch got, const uint32_t grid, const uint32_t block) {
    REQUIRE(got.grid == grid);
    REQUIRE(got.block == (grid ? block : 0u));
}

// the info block: regions disjoint, in the documented order, adding up to the total
static void checkInfoShape(const InfoLayout & l, const uint32_t M) {
    struct Region {
        uint64_t begin, words;
    };
    const Region regions[] = {{InfoLayout::info, kInfoWords}, {l.pair_bytes, 2},   {l.mat_flag, M},      {l.replay_list, uint64_t(M) + 1},
                              {l.marked_bits, l.mark_words},  {l.marked_count, 1}, {l.pair_counts, 2},   {l.between_count, 1},
                              {l.row_item_count, 1},          {l.active, l.active_words}, {l.mat_list, M}};
    uint64_t at = 0;
    for (const Region & r : regions) {
        REQUIRE(r.begin == at);  // starts where the one before ends: disjoint, ordered, no gap
        at += r.words;
    }
    REQUIRE(at == l.total_words);
    REQUIRE(l.pair_bytes * sizeof(uint32_t) % 8 == 0);  // the 8-byte counter
    REQUIRE(l.zeroed_words == l.mat_list);              // the zeroed prefix ends where the list sizes begin
}

// what the launch code computed, formula for formula
static void checkAgainstFormulas(const CollapseShape & s, const CollapseKnobs & knobs) {
    const CollapsePlan p = planCollapse(s, knobs);
    const uint32_t M = s.M;
    const uint64_t total_rows = s.total_rows;
    if (M == 0 || total_rows == 0) {
        REQUIRE(p.verdict == kNothingToDo);
        return;
    }
    if (total_rows > 0x7fffffffull || (s.caller_keys ? M >= (1u << 20) : M + 1 >= (1u << 20))) {
        REQUIRE(p.verdict == kTooLarge);
        return;
    }
    REQUIRE(p.verdict == kRun && p.M == M && p.total_rows == total_rows);
    const bool library_sort = s.caller_keys ? knobs.library_sort_matrices : knobs.library_sort_problems;
    const bool hand = !library_sort && s.max_segment_rows <= (1ull << 20) - 1 && s.max_segment_rows > 0;  // (0: unknown)
    REQUIRE(p.route == (hand ? HandSort : s.caller_keys ? LibraryGlobal : LibrarySegmented));

    const uint64_t mark_words = (total_rows + 31) / 32;
    const uint64_t num_words = 2 + 2 * static_cast<uint64_t>(M) + 1 + mark_words + 5;
    const uint64_t active_words = (total_rows + 3) / 4;
    const InfoLayout & l = p.info;
    REQUIRE(l.mark_words == mark_words && l.active_words == active_words);
    REQUIRE(l.total_words == 6 + num_words + active_words + M);
    REQUIRE(l.zeroed_words == 6 + num_words + active_words);
    REQUIRE(InfoLayout::info == 0 && l.pair_bytes == 6 && l.mat_flag == l.pair_bytes + 2 && l.replay_list == l.mat_flag + M);
    REQUIRE(l.marked_bits == l.replay_list + M + 1 && l.marked_count == l.marked_bits + mark_words && l.pair_counts == l.marked_count + 1);
    REQUIRE(l.between_count == l.pair_counts + 2 && l.row_item_count == l.between_count + 1);
    REQUIRE(l.active == l.pair_bytes + num_words && l.mat_list == l.pair_bytes + num_words + active_words);
    REQUIRE(l.marked_count == 6 + 2 + 2 * static_cast<uint64_t>(M) + 1 + mark_words);  // (as the EM solve's dump read it)
    checkInfoShape(l, M);

    const uint32_t pair_capacity = static_cast<uint32_t>(std::min<uint64_t>(4 * total_rows + 4096, 0x20000000ull));
    REQUIRE(p.pair_capacity == pair_capacity);
    const BufferCounts & c = p.counts;
    REQUIRE(c.sorted_key == total_rows && c.sorted_row == total_rows);
    REQUIRE(c.order == 2 * total_rows && c.head == total_rows && c.pair_column == total_rows && c.pair_bound == 2 * total_rows);
    REQUIRE(c.pair_pattern == total_rows && c.marked_list == total_rows && c.pairs == 2 * static_cast<uint64_t>(pair_capacity));
    REQUIRE(c.between_items == 2 * (total_rows / 512 + M) && c.row_items == 2 * total_rows && c.list_index == total_rows);
    REQUIRE(c.pair_base == M && c.pair_table == (16ull << 20) && c.bytes == 3 * total_rows && c.stretch == 4 * total_rows);
    REQUIRE(c.pattern == (s.caller_keys ? 0 : total_rows));
    const uint32_t chunk_capacity = static_cast<uint32_t>(std::min<uint64_t>(total_rows / 2048 + M + 1, 0x7fffffffull));
    REQUIRE(segmentSortChunkCapacity(total_rows, M) == chunk_capacity);
    if (hand) {
        REQUIRE(c.words == total_rows && c.chunks == 2 * static_cast<uint64_t>(chunk_capacity) && c.chunk_count == 1);
        REQUIRE(c.keys == 0 && c.rows == 0 && c.segments == 0);
        REQUIRE(p.segment_sort.chunk_capacity == chunk_capacity);
    } else {
        REQUIRE(c.words == 0 && c.chunks == 0 && c.chunk_count == 0);
        REQUIRE(c.keys == (s.caller_keys ? 0 : total_rows) && c.rows == c.keys && c.segments == (s.caller_keys ? 0 : 2 * static_cast<uint64_t>(M)));
    }

    int matrix_bits = 1;
    while ((1u << matrix_bits) < M + 1) ++matrix_bits;
    const bool segmented = !hand && !s.caller_keys;
    REQUIRE(p.matrix_bits == matrix_bits && p.begin_bit == 20 - s.hash_bits && p.end_bit == (segmented ? 44 : 44 + matrix_bits));

    const uint32_t small_grid = knobs.small_grid;
    const uint32_t row_blocks = static_cast<uint32_t>((total_rows + 255) / 256);
    if (hand) {
        requireLaunch(p.keys, 0, 0);
        requireLaunch(p.same_prev, 0, 0);
        requireLaunch(p.unused_slots, s.hash_bits ? std::max<uint32_t>(1, std::min<uint32_t>(s.num_items_bound, 8 * small_grid)) : 0, 256);
        const uint32_t pairs = (M + 2 - 1) / 2;
        requireLaunch(p.segment_sort.small_sort, std::max<uint32_t>(1, std::min<uint32_t>(pairs, 16 * small_grid)), 128);
        const bool chunked = s.max_segment_rows > 1024;
        const uint32_t merge_rounds = chunked ? rpvg_sort::mergeRoundsOf(s.max_segment_rows) : 0;
        REQUIRE(p.segment_sort.merge_rounds == merge_rounds);
        requireLaunch(p.segment_sort.chunk_sort, chunked ? 4 * small_grid : 0, 256);
        requireLaunch(p.segment_sort.merge_round, merge_rounds ? 8 * small_grid : 0, 128);
        requireLaunch(p.segment_sort.merged_positions, chunked ? 4 * small_grid : 0, 256);
    } else {
        requireLaunch(p.keys, segmented ? std::max<uint32_t>(1, std::min<uint32_t>(s.num_items_bound, s.cus * 8)) : 0, 256);
        requireLaunch(p.unused_slots, 0, 0);
        requireLaunch(p.same_prev, row_blocks, 256);
        requireLaunch(p.segment_sort.small_sort, 0, 0);
    }
    requireLaunch(p.stretch_end, row_blocks, 256);
    requireLaunch(p.forward_pairs, row_blocks, 256);
    requireLaunch(p.mark_pairs, small_grid, 64);
    requireLaunch(p.around_pairs, 256, 64);
    requireLaunch(p.active_pairs, small_grid, 64);
    requireLaunch(p.list, std::min<uint32_t>(M, small_grid), 256);
    requireLaunch(p.pair_table, small_grid, 64);
    requireLaunch(p.rank, small_grid, 256);
    requireLaunch(p.list_sort, std::min<uint32_t>(M, 32), 256);
    requireLaunch(p.between, 2 * small_grid, 256);
    requireLaunch(p.runs, small_grid, 256);
    requireLaunch(p.adjust_sums, small_grid * 4, 256);
    requireLaunch(p.rewrite, small_grid, 256);
}

static void checkBothViews(const uint32_t M, const uint64_t total_rows, const uint64_t longest, const CollapseKnobs & knobs) {
    checkAgainstFormulas(matrices(M, total_rows, longest), knobs);
    checkAgainstFormulas(problems(M, total_rows, longest), knobs);
    checkAgainstFormulas(problems(M, total_rows, longest, 0, 1), knobs);          // (no items: a grid of 1 all the same)
    checkAgainstFormulas(problems(M, total_rows, longest, 1u << 20, 304), knobs);  // (more items than either grid holds)
}

int main() {
    const uint64_t kMaxSegment = rpvg_sort::kMaxSegmentRows;
    REQUIRE(kMaxSegment == (1ull << 20) - 1);
    const uint64_t cap_rows = (0x20000000ull - 4096) / 4;  // 4 rows + 4096 == the cap of the pair list
    std::vector<uint32_t> Ms = {0, 1, 2, 3, 4, 31, 32, 33, 255, 256, 257, 511, 512, 513, (1u << 20) - 3, (1u << 20) - 2, (1u << 20) - 1, 1u << 20};
    for (int k = 1; k < 20; ++k) {  // matrix bits of M + 1
        Ms.push_back((1u << k) - 1);
        Ms.push_back(1u << k);
    }
    const std::vector<uint64_t> rows = {0, 1, 3, 4, 5, 31, 32, 33, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 1000003, cap_rows - 1, cap_rows, cap_rows + 1,
                                        0x7ffffffeull, 0x7fffffffull, 0x80000000ull};
    const std::vector<uint64_t> longest = {0, 1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8193, kMaxSegment - 1, kMaxSegment, kMaxSegment + 1, 1ull << 31};
    std::vector<CollapseKnobs> knobs(6);
    knobs[1].library_sort_matrices = true;  // the library knob for one view and not the other
    knobs[2].library_sort_problems = true;
    knobs[3].library_sort_matrices = knobs[3].library_sort_problems = true;
    knobs[4].small_grid = 1;
    knobs[5].small_grid = 1024;
    knobs[5].debug = knobs[5].no_lds_tables = true;
    for (const uint32_t M : Ms) {
        for (const uint64_t T : rows) {
            for (const uint64_t R : longest) {
                for (const CollapseKnobs & k : knobs) checkBothViews(M, T, R, k);
            }
        }
    }

    // ---- the edges, one by one -----------------------------------------------------------------------------------------------------
    const CollapseKnobs none;
    // active words (a byte per row) and mark words (a bit per row)
    const uint64_t active_at[][2] = {{1, 1}, {3, 1}, {4, 1}, {5, 2}}, mark_at[][2] = {{31, 1}, {32, 1}, {33, 2}};
    for (const auto & e : active_at) REQUIRE(planCollapse(matrices(1, e[0], e[0]), none).info.active_words == e[1]);
    for (const auto & e : mark_at) REQUIRE(planCollapse(matrices(1, e[0], e[0]), none).info.mark_words == e[1]);
    // matrix bits: as many as M + 1 values need, one at least
    const uint32_t bits_at[][2] = {{1, 1}, {2, 2}, {3, 2}, {4, 3}, {7, 3}, {8, 4}, {(1u << 19) - 1, 19}, {1u << 19, 20}, {(1u << 20) - 1, 20}};
    for (const auto & e : bits_at) {
        const CollapsePlan p = planCollapse(matrices(e[0], 100, 0), none);  // (bound unknown: the global sort, which uses them)
        REQUIRE(p.route == LibraryGlobal && p.matrix_bits == static_cast<int>(e[1]) && p.begin_bit == 20 && p.end_bit == 44 + static_cast<int>(e[1]));
    }
    REQUIRE(planCollapse(problems(5, 100, 0), none).begin_bit == 20 - kCsrCellHashBits && planCollapse(problems(5, 100, 0), none).end_bit == 44);
    // the pair list's cap
    REQUIRE(planCollapse(matrices(1, cap_rows - 1, 1), none).pair_capacity == 0x20000000u - 4);
    REQUIRE(planCollapse(matrices(1, cap_rows, 1), none).pair_capacity == 0x20000000u);
    REQUIRE(planCollapse(matrices(1, cap_rows + 1, 1), none).pair_capacity == 0x20000000u);
    // the longest segment: the small sort only, then the chunks with 0, 1, 2 rounds
    const uint64_t rounds_at[][3] = {{1024, 0, 0}, {1025, 1, 0}, {2048, 1, 0}, {2049, 1, 1}, {4096, 1, 1}, {4097, 1, 2}};
    for (const auto & e : rounds_at) {
        const SegmentSortPlan s = planCollapse(problems(10, 100000, e[0]), none).segment_sort;
        REQUIRE((s.chunk_sort.grid != 0) == (e[1] != 0) && (s.merged_positions.grid != 0) == (e[1] != 0));
        REQUIRE(s.merge_rounds == e[2] && (s.merge_round.grid != 0) == (e[2] != 0));
        REQUIRE(s.small_sort.grid == 5 && s.small_sort.block == 128);
        const SegmentSortPlan alone = planSegmentSort(10, 100000, e[0], 256);  // (the sort's own entry point: the same launches)
        REQUIRE(alone.chunk_capacity == s.chunk_capacity && alone.merge_rounds == s.merge_rounds && alone.small_sort == s.small_sort &&
                alone.chunk_sort == s.chunk_sort && alone.merge_round == s.merge_round && alone.merged_positions == s.merged_positions);
    }
    // the route
    REQUIRE(planCollapse(matrices(3, 1ull << 22, kMaxSegment - 1), none).route == HandSort);
    REQUIRE(planCollapse(matrices(3, 1ull << 22, kMaxSegment), none).route == HandSort);
    REQUIRE(planCollapse(matrices(3, 1ull << 22, kMaxSegment + 1), none).route == LibraryGlobal);
    REQUIRE(planCollapse(problems(3, 1ull << 22, kMaxSegment), none).route == HandSort);
    REQUIRE(planCollapse(problems(3, 1ull << 22, kMaxSegment + 1), none).route == LibrarySegmented);
    REQUIRE(planCollapse(problems(3, 1ull << 22, 0), none).route == LibrarySegmented);  // bound unknown
    REQUIRE(planCollapse(matrices(3, 100, 50), knobs[1]).route == LibraryGlobal && planCollapse(problems(3, 100, 50), knobs[1]).route == HandSort);
    REQUIRE(planCollapse(matrices(3, 100, 50), knobs[2]).route == HandSort && planCollapse(problems(3, 100, 50), knobs[2]).route == LibrarySegmented);
    REQUIRE(planCollapse(matrices(3, 100, 50), knobs[3]).route == LibraryGlobal && planCollapse(problems(3, 100, 50), knobs[3]).route == LibrarySegmented);
    // the refusals, at the limit and one below
    REQUIRE(planCollapse(matrices(1, 0x7fffffffull, 1), none).verdict == kRun && planCollapse(matrices(1, 0x80000000ull, 1), none).verdict == kTooLarge);
    REQUIRE(planCollapse(matrices((1u << 20) - 1, 10, 1), none).verdict == kRun && planCollapse(matrices(1u << 20, 10, 1), none).verdict == kTooLarge);
    REQUIRE(planCollapse(problems((1u << 20) - 2, 10, 1), none).verdict == kRun && planCollapse(problems((1u << 20) - 1, 10, 1), none).verdict == kTooLarge);
    REQUIRE(planCollapse(matrices(0, 10, 1), none).verdict == kNothingToDo && planCollapse(matrices(1, 0, 1), none).verdict == kNothingToDo);
    REQUIRE(planCollapse(problems(0, 1ull << 40, 1), none).verdict == kNothingToDo);  // (nothing to do comes first)
    REQUIRE(planCollapse(matrices(1, 1, 1), none).verdict == kRun && planCollapse(problems(1, 1, 1), none).verdict == kRun);
    std::printf("ok\n");
    return 0;
}
