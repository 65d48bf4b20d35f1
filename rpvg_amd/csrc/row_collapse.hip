// readCollapseProbabilityMatrix (src/path_estimator.cpp:197-259, comparator :13-31) replayed on the group matrices
// (callers src/path_abundance_estimator.cpp:380,443) on the GPU (gfx950).
//
// The reference sorts the rows of the normalised matrix (group columns, then the noise column, then the read
// count; every comparison tolerant, Utils::doubleCompare) and merges every row that lies within prob_precision of
// the head of its run — in all columns, absolutely — into that head: the head keeps its values, the counts add up.
// The consumers of a group matrix are sums over rows of count * log(noise + columns), so "merged into the head" is
// "takes the values of the head" with the row's own count: the rows stay where they are (their class order,
// LogProduct, is untouched) and only values move.
//
// Such rows are not rare: a read whose worst candidate path falls below prob_precision moves that mass into its noise
// probability (src/read_path_probabilities.cpp:181-215), the caller's sort compares the noise first
// (:283-322) and so does not bring it next to the row without that candidate, and the two meet again here.  But they
// are few (427 of the 3.28 M rows of the configs[2] workload), so nothing below sorts a whole matrix unless it must:
//   1. close pairs.  Every row carries a projection key (the sum of its values with fixed weights in [0, 2), written
//      by the build kernels as (matrix, fixed-point key): collapseSortKey, common.hpp).  Rows within prob_precision of
//      each other in all columns have keys within 2 (G + 1) prob_precision, so one radix sort over all matrices and
//      a forward window scan find every close pair.  A close pair that is equal up to rounding (<= 1e-13 relative) moves
//      nothing worth moving; a pair that is not marks both rows, and a second window scan adds the rows close to a
//      marked row: the ACTIVE rows.  A run of the reference that changes a value consists of active rows only, and an
//      inactive row is close to no active one.
//   2. replay, for the matrices with active rows:
//      a. (one workgroup per matrix) the active rows are sorted with the reference's comparator, bitonic network in LDS;
//      b. (the rows of those matrices, spread over many workgroups) an inactive row that the order places between two
//         neighbours of that list ends the run there, as it would in the reference (it is compared with the head,
//         fails, and becomes the head) — such a row has the zeros of both neighbours up to the first column in which
//         they differ, and lies between them in that column;
//      c. (one workgroup per matrix) the reference's compare-with-the-head rule, and the values of the head (group
//         columns, noise, row maximum) are copied over its run.
//      A matrix whose windows are too crowded to look through, or with more active rows than the LDS list holds,
//      takes the same code with every row active (the whole matrix sorted; no rows left to lie in between).
// The tolerant comparison is not a strict weak order; where it is inconsistent the reference's own result is
// whatever std::sort makes of it.

#include "collapse_plan.hpp"
#include "common.hpp"

#include <hipcub/hipcub.hpp>

#include <cfloat>

using namespace rpvg_hip_detail;

namespace {

using namespace rpvg_collapse;
static_assert(kKeyLargestBits == kCollapseLargestBits && kKeyMatrixShift == kCollapseMatrixShift && kMaxMatrices == kCollapseMaxMatrices,
              "collapse_plan.hpp restates these");

constexpr int kKeyFractionBits = kCollapseKeyFractionBits;
constexpr uint32_t kMaxWindowCompares = 256;   // a row with more candidates than this sends its matrix to the full sort
enum : uint8_t { kRowListed = 1, kRowStoodFor = 2 };
constexpr double kEquivalentRelative = 1e-13;  // close rows that differ by no more than this are interchangeable
// (8 192 in rounds 2-3: 96 KB of static LDS and 1 024 threads, a whole CU per workgroup — on a batch without a single big list
// the kernel still waited 0.2-0.4 ms for CUs the other lane's kernels held, on the collapse's critical path)
constexpr uint32_t kListLdsRows = 2048;        // row lists up to this size live (and are sorted) in LDS
constexpr uint32_t kPairChunk = 256;           // neighbour pairs staged in LDS at a time
constexpr uint32_t kWholeMatrixBit = 0x80000000u;  // mat_list: every row of the matrix is listed
constexpr uint32_t kBigListBit = 0x40000000u;      // mat_list: sorted by the bitonic kernel, compared in depth (no pair table)
constexpr uint32_t kListSizeMask = 0x3FFFFFFFu;
constexpr uint32_t kPairwiseRows = 1024;           // lists up to this size get a table of all their pairs
constexpr uint8_t kPairLess = 1, kPairClose = 2;
constexpr uint32_t kLdsTableRows = 128;            // pair tables of lists up to this size are read from LDS (16 KB)

enum : uint32_t { kFlagNone = 0, kFlagActiveRows = 1, kFlagWholeMatrix = 2 };

__device__ __forceinline__ bool tolerantEqual(const double a, const double b) {  // Utils::doubleCompare, src/utils.hpp:87-93
    return a == b || fabs(a - b) < fabs(fmin(a, b)) * (DBL_EPSILON * 100);
}

struct MatrixView {
    const double * values;     // column-major R x G
    const double * noise;
    const double * count;
    const uint64_t * pattern;  // bit c: column c (< 64) of the row is not zero
    uint64_t R;
    uint32_t G;
    // column G = noise.  (One load behind a selected address: a load on either side of a branch would wait for the
    // previous one, and the comparisons below live on having their loads in flight together.)
    __device__ __forceinline__ double at(const uint32_t column, const uint32_t row) const {
        const double * address = column < G ? values + (static_cast<uint64_t>(column) * R + row) : noise + row;
        return __builtin_nontemporal_load(address);
    }
    __device__ __forceinline__ uint64_t patternOf(const uint32_t row) const { return pattern[row]; }
    __device__ __forceinline__ double countOf(const uint32_t row) const { return count[row]; }
};

// The rows of one EM problem (em_sparse.hip: the compacted CSR of a cluster restricted to a path subset): the same
// interface over sparse rows.  A row holds a handful of entries, in no particular column order: at() walks them.
struct CsrView {
    const uint32_t * off;      // [R + 1] entry range of every row, relative to `col` / `val`
    const uint32_t * col;
    const double * val;
    const double * noise;
    const double * count;
    const uint64_t * pattern;
    uint64_t R;
    uint32_t G;
    __device__ __forceinline__ double at(const uint32_t column, const uint32_t row) const {
        if (column >= G) return noise[row];
        double value = 0.0;
        for (uint32_t e = off[row]; e < off[row + 1]; ++e) {
            if (col[e] == column) value = val[e];
        }
        return value;
    }
    __device__ __forceinline__ uint64_t patternOf(const uint32_t row) const { return pattern[row]; }
    __device__ __forceinline__ double countOf(const uint32_t row) const { return count[row]; }
};

// Rows that are compared in depth agree in most columns, and a column costs two strided loads.  The comparisons below
// walk the columns in the reference's order but (1) skip the columns in which both rows are zero — equal for every
// purpose here — by their zero patterns, and (2) fetch kBatch columns of both rows before they look at any of them,
// so that the loads are in flight together.
constexpr uint32_t kBatch = 8;

template <typename View, typename Decide>  // decide(x, y) -> true: stop
__device__ __forceinline__ void forEachColumnPair(const View & mv, const uint32_t a, const uint32_t b, uint64_t live, Decide decide) {
    uint32_t next_wide = 64;  // columns from 64 on carry no pattern: all of them
    bool noise_done = false;
    while (true) {
        uint32_t column[kBatch];
        uint32_t filled = 0;
        while (filled < kBatch && live) {
            column[filled++] = static_cast<uint32_t>(__ffsll(static_cast<long long>(live)) - 1);
            live &= live - 1;
        }
        while (filled < kBatch && next_wide < mv.G) column[filled++] = next_wide++;
        if (filled < kBatch && !noise_done) {
            column[filled++] = mv.G;
            noise_done = true;
        }
        if (filled == 0) return;
        double x[kBatch], y[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t c = column[k < filled ? k : 0];
            x[k] = mv.at(c, a);
            y[k] = mv.at(c, b);
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            if (k < filled && decide(x[k], y[k])) return;
        }
    }
}

// probabilityCountRowSorter (src/path_estimator.cpp:13-31) on rows a, b of one matrix
template <typename View>
__device__ bool rowLess(const View & mv, const uint32_t a, const uint32_t b, const uint64_t pattern_a, const uint64_t pattern_b) {
    int result = -1;
    forEachColumnPair(mv, a, b, pattern_a | pattern_b, [&](const double x, const double y) {
        if (tolerantEqual(x, y)) return false;
        result = x < y ? 1 : 0;
        return true;
    });
    if (result >= 0) return result != 0;
    const double x = mv.countOf(a), y = mv.countOf(b);
    if (!tolerantEqual(x, y)) return x < y;
    return false;
}

template <typename View>
__device__ __forceinline__ bool rowLess(const View & mv, const uint32_t a, const uint32_t b) {
    return rowLess(mv, a, b, mv.patternOf(a), mv.patternOf(b));
}

// every column (noise included) within `precision` of each other, absolutely (src/path_estimator.cpp:232-239);
// *equivalent: additionally equal up to rounding in every column
template <typename View>
__device__ __forceinline__ bool rowsClose(const View & mv, const uint32_t a, const uint32_t b, const double precision, bool * equivalent) {
    bool eq = true, close = true;
    forEachColumnPair(mv, a, b, mv.patternOf(a) | mv.patternOf(b), [&](const double x, const double y) {
        // (both flags updated on every path: a store to whichever flag a branch picked kept them in scratch memory)
        const double d = fabs(x - y);
        const bool apart = d >= precision;
        close = close && !apart;
        eq = eq && !(d > kEquivalentRelative * fmin(fabs(x), fabs(y)));
        return apart;
    });
    if (close && equivalent) *equivalent = eq;
    return close;
}

// The rows of an EM problem are cluster rows cut down to the problem's columns: thousands of them agree up to the rounding of
// their last normalisation, not bit for bit.  A "cell" is a value's multiple of 2^-44 (5.7e-14, five orders below the
// precision of the collapse): rows with the same cells in every column stand for each other in the search for close rows.
constexpr double kCellsPerUnit = 0x1p44;
constexpr double kCellWidth = 0x1p-44;
__device__ __forceinline__ int64_t cellOf(const double v) { return static_cast<int64_t>(v * kCellsPerUnit); }

template <typename View>
__device__ bool rowsSameCells(const View & mv, const uint32_t a, const uint32_t b) {
    bool same = true;
    forEachColumnPair(mv, a, b, mv.patternOf(a) | mv.patternOf(b), [&](const double x, const double y) {
        if (cellOf(x) == cellOf(y)) return false;
        same = false;
        return true;
    });
    return same;
}

// (rows of a problem nearly always list their entries in the same column order: the entry lists are compared as they are, the
// column walk only decides when the lists differ in shape)
__device__ bool rowsSameCells(const CsrView & mv, const uint32_t a, const uint32_t b) {
    const uint32_t a0 = mv.off[a], a1 = mv.off[a + 1], b0 = mv.off[b];
    if (cellOf(mv.noise[a]) != cellOf(mv.noise[b])) return false;
    bool same_shape = a1 - a0 == mv.off[b + 1] - b0;
    for (uint32_t k = 0; same_shape && k < a1 - a0; ++k) same_shape = mv.col[a0 + k] == mv.col[b0 + k];
    if (same_shape) {
        for (uint32_t k = 0; k < a1 - a0; ++k) {
            if (cellOf(mv.val[a0 + k]) != cellOf(mv.val[b0 + k])) return false;
        }
        return true;
    }
    return rowsSameCells<CsrView>(mv, a, b);
}

template <typename View>
__device__ bool rowsIdentical(const View & mv, const uint32_t a, const uint32_t b) {
    bool same = true;
    forEachColumnPair(mv, a, b, mv.patternOf(a) | mv.patternOf(b), [&](const double x, const double y) {
        if (x == y) return false;
        same = false;
        return true;
    });
    return same;
}

struct MatrixArrays {
    const uint64_t * mat_val_off;
    const uint64_t * mat_row_off;
    const uint64_t * mat_rows;
    const uint32_t * mat_cols;
    double * values;
    double * row_noise;
    const double * row_count;
    const uint64_t * zero_pattern;
    typedef MatrixView View;
    static constexpr int kHashBits = 0;  // stretches: bit for bit equal rows
    __device__ __forceinline__ uint64_t rowOffset(const uint32_t m) const { return mat_row_off[m]; }
    __device__ __forceinline__ uint64_t numRows(const uint32_t m) const { return mat_rows[m]; }
    __device__ __forceinline__ uint32_t numCols(const uint32_t m) const { return mat_cols[m]; }
    __device__ __forceinline__ MatrixView view(const uint32_t m) const {
        MatrixView mv;
        mv.values = values + mat_val_off[m];
        mv.noise = row_noise + mat_row_off[m];
        mv.count = row_count + mat_row_off[m];
        mv.pattern = zero_pattern + mat_row_off[m];
        mv.R = mat_rows[m];
        mv.G = mat_cols[m];
        return mv;
    }
};

// the EM problems of a solve as "matrices": problem p's rows sit at row_base[p] (the layout by the bound: there are unused
// row slots between the problems, whose sort keys carry a matrix index no problem has)
struct CsrArrays {
    EmProblemsView problems;       // (as filled: without the merged counts, which this collapse writes)
    const uint64_t * zero_pattern; // [rows]
    double * merged_count;         // [rows] read counts after the merges (written for the problems with a replay)
    uint32_t * problem_merged;     // [P] 1: rows of the problem were merged
    uint32_t * merged_problems;    // [0]: their number
    typedef CsrView View;
    static constexpr int kHashBits = kCsrCellHashBits;  // stretches: rows of equal cells (rowsSameCells), kept together by a hash of them in the key
    __device__ __forceinline__ uint64_t rowOffset(const uint32_t p) const { return problems.row_base[p]; }
    __device__ __forceinline__ uint64_t numRows(const uint32_t p) const { return problems.kept_rows[p]; }
    __device__ __forceinline__ uint32_t numCols(const uint32_t p) const { return problems.paths(p); }
    __device__ __forceinline__ CsrView view(const uint32_t p) const {
        CsrView mv;
        const EmProblemRows csr = problems.rows(p);
        mv.off = csr.off;
        mv.col = csr.col;
        mv.val = csr.val;
        mv.noise = csr.noise;
        mv.count = csr.count;
        mv.pattern = zero_pattern + problems.row_base[p];
        mv.R = csr.rows;
        mv.G = numCols(p);
        return mv;
    }
};

template <typename Arrays>
__device__ __forceinline__ typename Arrays::View viewOf(const uint32_t m, const Arrays & g) { return g.view(m); }

// ---- sort key fields (collapseSortKey, common.hpp) -------------------------------------------------------------
__device__ __forceinline__ uint32_t keyMatrix(const uint64_t key) { return static_cast<uint32_t>(key >> kCollapseMatrixShift); }
// HASH bits at the top of the low field belong to the sorted part (EM problems: a hash of the row's cells)
template <int HASH>
__device__ __forceinline__ uint64_t keySorted(const uint64_t key) { return key >> (kCollapseLargestBits - HASH); }  // (matrix, projection[, hash])
__device__ __forceinline__ uint64_t keyProjection(const uint64_t key) { return key >> kCollapseLargestBits; }  // (matrix, projection)
template <int HASH>
__device__ __forceinline__ int64_t keyLargest(const uint64_t key) { return static_cast<int64_t>(key & ((1ull << (kCollapseLargestBits - HASH)) - 1)); }

// |key_a - key_b| <= sum_c w_c |a_c - b_c| < 2 (G + 1) precision for close rows; + rounding of the keys, + 2 quanta
__device__ __forceinline__ uint64_t windowQuanta(const uint32_t G, const double precision) {
    const double window = 2.0001 * (G + 1) * precision + 1e-12;
    return static_cast<uint64_t>(window * static_cast<double>(1ull << kKeyFractionBits)) + 2;
}

// the largest values of close rows lie within the precision of each other: steps of the key's low field apart
// (the field wraps: half its range or more means "no filter")
template <int HASH>
__device__ __forceinline__ int64_t largestSteps(const double precision) {
    const double steps = precision * static_cast<double>(1ull << kCollapseLargestFractionBits) + (HASH ? 2.0 : 1.0);  // (rows of equal cells: up to a step from their first)
    return steps >= static_cast<double>(1ull << (kCollapseLargestBits - HASH - 1)) ? (1ll << (kCollapseLargestBits - HASH)) : static_cast<int64_t>(steps);
}

// `other` (at or behind `key` in the sorted order) can be close to `key`'s row
template <int HASH>
__device__ __forceinline__ bool inWindow(const uint64_t key, const uint64_t other, const uint64_t window_q, const int64_t largest_steps, bool * beyond) {
    *beyond = keyMatrix(other) != keyMatrix(key) || keyProjection(other) - keyProjection(key) > window_q;
    if (*beyond) return false;
    constexpr int bits = kCollapseLargestBits - HASH;
    int64_t d = (keyLargest<HASH>(other) - keyLargest<HASH>(key)) & ((1ll << bits) - 1);  // modulo the field
    if (d >= (1ll << (bits - 1))) d -= 1ll << bits;
    return d <= largest_steps && -d <= largest_steps;
}

// ---- stage 1: close pairs ---------------------------------------------------------------------------------------

template <typename Arrays>
struct PairScanArgs {
    uint32_t num_matrices;   // sort keys with a matrix index from here on belong to unused row slots (EM problems)
    uint64_t total_rows;
    double precision;
    const uint64_t * sort_key;   // sorted (matrix, key, largest value)
    const uint32_t * sort_row;   // position of the row in the row arrays (mat_row_off[m] + row)
    Arrays g;
    uint8_t * same_prev;     // [total rows] by sorted position
    uint32_t * stretch_first; // [total rows] by sorted position: first position of the stretch of bit-for-bit equal rows it lies in
    uint32_t * stretch_end;   // [total rows] at the first position of a stretch: one past its last
    uint32_t * position_of;   // [total rows] by row: its sorted position (EM problems)
    uint32_t * marked_bits;  // [total rows / 32] by row: has a close partner that is not its equal up to rounding
    uint32_t * marked_list;  // [total rows] sorted positions of the marked rows
    uint32_t * marked_count;
    uint32_t * pairs;        // [2 x pair_capacity] candidate pairs (sorted positions) of the scan that runs
    uint32_t * pair_count;   // its number of pairs
    uint32_t pair_capacity;
    uint8_t * active;        // [total rows] by row: kRowListed: marked, or close to a marked row; kRowStoodFor (EM problems): the first row of its stretch is
    uint32_t * mat_flag;     // [M]
    uint32_t * info;
    bool count_pairs;        // measuring aid: info[] counts the candidate pairs that were equal up to rounding / not close
};

// The window scans only collect candidate pairs; the comparisons, each a few dependent rounds of strided loads, then
// run one per thread, all at once (a thread that walked its window and compared as it went spent ~1 us per step:
// 0.2-0.4 ms for the longest windows of the batch).
template <typename Arrays>
__device__ __forceinline__ bool appendPair(const PairScanArgs<Arrays> & a, const uint64_t p, const uint64_t q) {
    const uint32_t slot = atomicAdd(a.pair_count, 1u);
    if (slot >= a.pair_capacity) return false;
    a.pairs[2 * static_cast<uint64_t>(slot)] = static_cast<uint32_t>(p);
    a.pairs[2 * static_cast<uint64_t>(slot) + 1] = static_cast<uint32_t>(q);
    return true;
}

// same_prev[p] = the row at sorted position p is bit for bit the row at p - 1 (same matrix)
template <typename Arrays>
__global__ void collapseSamePrevKernel(const PairScanArgs<Arrays> a) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= a.total_rows) return;
    uint8_t same = 0;
    constexpr int HASH = Arrays::kHashBits;
    // equal keys (with a hash: equal sorted parts — the largest values of rows of equal cells can lie a step apart):
    // nearly always the same values twice; the comparison leaves at the first difference
    if (p > 0 && (HASH ? keySorted<HASH>(a.sort_key[p]) == keySorted<HASH>(a.sort_key[p - 1]) : a.sort_key[p] == a.sort_key[p - 1]) &&
        keyMatrix(a.sort_key[p]) < a.num_matrices) {
        const uint32_t m = keyMatrix(a.sort_key[p]);
        const typename Arrays::View mv = viewOf(m, a.g);
        const uint64_t r0 = a.g.rowOffset(m);
        const uint32_t row = static_cast<uint32_t>(a.sort_row[p] - r0), before = static_cast<uint32_t>(a.sort_row[p - 1] - r0);
        same = (HASH ? rowsSameCells(mv, row, before) : rowsIdentical(mv, row, before)) ? 1 : 0;
    }
    a.same_prev[p] = same;
    if (HASH) a.position_of[a.sort_row[p]] = static_cast<uint32_t>(p);
    a.stretch_first[p] = same ? 0u : static_cast<uint32_t>(p);  // (the running maximum of these is the stretch's first position)
}

// stretch_end[] of every stretch, written by its last position
template <typename Arrays>
__global__ void collapseStretchEndKernel(const PairScanArgs<Arrays> a) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p >= a.total_rows) return;
    if (p + 1 == a.total_rows || !a.same_prev[p + 1]) a.stretch_end[a.stretch_first[p]] = static_cast<uint32_t>(p + 1);
}

// The first row of every stretch of equal rows lists the stretches after it whose keys lie within the window (a window too
// crowded to list sends the matrix to the full sort).  The scans step from stretch to stretch: the rows of an EM problem are
// cluster rows cut down to a few columns, thousands of them bit for bit the same, and a scan that walked over every copy
// took 3 ms on the problems of one batch.
template <typename Arrays>
__global__ void collapseForwardPairsKernel(const PairScanArgs<Arrays> a) {
    const uint64_t p = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (p + 1 >= a.total_rows || a.same_prev[p]) return;
    const uint64_t first = a.stretch_end[p];
    if (first >= a.total_rows) return;
    const uint64_t key = a.sort_key[p];
    const uint64_t next = a.sort_key[first];
    const uint32_t m = keyMatrix(key);
    if (keyMatrix(next) != m || m >= a.num_matrices) return;
    const uint64_t window_q = windowQuanta(a.g.numCols(m), a.precision);
    if (keyProjection(next) - keyProjection(key) > window_q) return;  // nearly every row leaves here
    constexpr int HASH = Arrays::kHashBits;
    const int64_t largest_steps = largestSteps<HASH>(a.precision);
    uint32_t listed = 0;
    for (uint64_t q = first; q < a.total_rows; q = a.stretch_end[q]) {
        const uint64_t other = a.sort_key[q];
        bool beyond;
        if (!inWindow<HASH>(key, other, window_q, largest_steps, &beyond)) {
            if (beyond) break;
            continue;
        }
        if (++listed > kMaxWindowCompares || !appendPair(a, p, q)) {
            atomicMax(&a.mat_flag[m], static_cast<uint32_t>(kFlagWholeMatrix));
            break;
        }
    }
}

// marks the row at sorted position p; the first marker puts it on the list
template <typename Arrays>
__device__ __forceinline__ void markRow(const PairScanArgs<Arrays> & a, const uint64_t p) {
    const uint32_t row = a.sort_row[p];
    const uint32_t bit = 1u << (row & 31);
    if ((atomicOr(&a.marked_bits[row >> 5], bit) & bit) == 0) a.marked_list[atomicAdd(a.marked_count, 1u)] = static_cast<uint32_t>(p);
}

template <typename Arrays>
__device__ __forceinline__ bool isMarked(const PairScanArgs<Arrays> & a, const uint32_t row) { return (a.marked_bits[row >> 5] >> (row & 31)) & 1u; }

// what a candidate pair of first rows has to pass for their stretches to count as close: the rows of a stretch lie within a
// cell of its first row (bit for bit equal rows: no margin)
template <typename Arrays>
__device__ __forceinline__ double pairPrecision(const double precision) { return Arrays::kHashBits ? precision + 2 * kCellWidth : precision; }

// the wave walks the stretches that start at the sorted positions its lanes hold in `first` (lanes with `wanted`):
// visit(position) for every row of them
template <typename Arrays, typename Visit>
__device__ __forceinline__ void forEachRowOfStretches(const PairScanArgs<Arrays> & a, const bool wanted, const uint32_t first, Visit visit) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t todo = __ballot(wanted); todo; todo &= todo - 1) {
        const int source = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t begin = __shfl(first, source), end = a.stretch_end[begin];
        for (uint32_t s = begin + lane; s < end; s += 64) visit(s);
    }
}

// first position of the stretch that sorted position s lies in
template <typename Arrays>
__device__ __forceinline__ uint32_t p0(const PairScanArgs<Arrays> & a, const uint32_t s) { return a.stretch_first[s]; }

// both stretches of a close pair that is not equal up to rounding are marked (blocks of one wave)
template <typename Arrays>
__global__ void collapseMarkPairsKernel(const PairScanArgs<Arrays> a) {
    const uint32_t count = min(*a.pair_count, a.pair_capacity);
    // (lane l of block b takes pair b + l * blocks: a short list spreads over the waves, each of which walks the stretches of its pairs)
    for (uint32_t base = 0; base < count; base += gridDim.x * blockDim.x) {
        const uint32_t item = base + threadIdx.x * gridDim.x + blockIdx.x;
        uint32_t p = 0, q = 0;
        bool mark = false;
        if (item < count) {
            p = a.pairs[2 * static_cast<uint64_t>(item)];
            q = a.pairs[2 * static_cast<uint64_t>(item) + 1];
            const uint32_t m = keyMatrix(a.sort_key[p]);
            const typename Arrays::View mv = viewOf(m, a.g);
            const uint64_t r0 = a.g.rowOffset(m);
            bool equivalent = true;
            const bool close = rowsClose(mv, static_cast<uint32_t>(a.sort_row[p] - r0), static_cast<uint32_t>(a.sort_row[q] - r0), pairPrecision<Arrays>(a.precision), &equivalent);
            if (a.count_pairs) atomicAdd(&a.info[close ? kInfoPairsEquivalent : kInfoPairsApart], close && !equivalent ? 0u : 1u);
            mark = close && !equivalent;
            if (mark) atomicMax(&a.mat_flag[m], static_cast<uint32_t>(kFlagActiveRows));
        }
        if (Arrays::kHashBits) {
            // EM problems: the first row of a stretch goes through the replay for all of it (finishRuns); the others only must
            // not count as rows that part neighbours of the lists
            if (mark) {
                markRow(a, p);
                markRow(a, q);
            }
            forEachRowOfStretches(a, mark, p, [&](const uint32_t s) { if (s != p0(a, s)) a.active[a.sort_row[s]] = kRowStoodFor; });
            forEachRowOfStretches(a, mark, q, [&](const uint32_t s) { if (s != p0(a, s)) a.active[a.sort_row[s]] = kRowStoodFor; });
        } else {
            forEachRowOfStretches(a, mark, p, [&](const uint32_t s) { markRow(a, s); });
            forEachRowOfStretches(a, mark, q, [&](const uint32_t s) { markRow(a, s); });
        }
    }
}

// active = marked, or close to a marked row: the first row of every marked stretch (they are few: a list) lists its
// window, both ways, stretch by stretch
template <typename Arrays>
__global__ void collapseAroundPairsKernel(const PairScanArgs<Arrays> a) {
    const uint32_t count = *a.marked_count;
    for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < count; item += gridDim.x * blockDim.x) {
        const uint64_t p = a.marked_list[item];
        a.active[a.sort_row[p]] = kRowListed;
        if (a.same_prev[p]) continue;  // a copy: the first row of its stretch lists for it
        const uint64_t key = a.sort_key[p];
        const uint32_t m = keyMatrix(key);
        const uint64_t window_q = windowQuanta(a.g.numCols(m), a.precision);
        constexpr int HASH = Arrays::kHashBits;
        const int64_t largest_steps = largestSteps<HASH>(a.precision);
        uint32_t listed = 0;
        bool crowded = false;
        for (uint64_t q = a.stretch_end[p]; q < a.total_rows && !crowded; q = a.stretch_end[q]) {
            bool beyond;
            const bool candidate = inWindow<HASH>(key, a.sort_key[q], window_q, largest_steps, &beyond);
            if (beyond) break;
            if (!candidate || isMarked(a, a.sort_row[q])) continue;
            if (++listed > kMaxWindowCompares || !appendPair(a, p, q)) crowded = true;
        }
        for (uint64_t below = p; below > 0 && !crowded;) {
            const uint64_t q = a.stretch_first[below - 1];
            below = q;
            bool beyond;
            const bool candidate = inWindow<HASH>(a.sort_key[q], key, window_q, largest_steps, &beyond);
            if (beyond) break;
            if (!candidate || isMarked(a, a.sort_row[q])) continue;
            if (++listed > kMaxWindowCompares || !appendPair(a, p, q)) crowded = true;
        }
        if (crowded) atomicMax(&a.mat_flag[m], static_cast<uint32_t>(kFlagWholeMatrix));
    }
}

template <typename Arrays>
__global__ void collapseActivePairsKernel(const PairScanArgs<Arrays> a) {  // (blocks of one wave)
    const uint32_t count = min(*a.pair_count, a.pair_capacity);
    for (uint32_t base = 0; base < count; base += gridDim.x * blockDim.x) {
        const uint32_t item = base + threadIdx.x * gridDim.x + blockIdx.x;
        uint32_t q = 0;
        bool close = false;
        if (item < count) {
            const uint32_t p = a.pairs[2 * static_cast<uint64_t>(item)];
            q = a.pairs[2 * static_cast<uint64_t>(item) + 1];
            const uint32_t m = keyMatrix(a.sort_key[p]);
            const typename Arrays::View mv = viewOf(m, a.g);
            const uint64_t r0 = a.g.rowOffset(m);
            close = rowsClose(mv, static_cast<uint32_t>(a.sort_row[p] - r0), static_cast<uint32_t>(a.sort_row[q] - r0), pairPrecision<Arrays>(a.precision), nullptr);
        }
        // q is the first row of its stretch: the rows it stands for are active with it (several writers, one value)
        forEachRowOfStretches(a, close, q, [&](const uint32_t s) { a.active[a.sort_row[s]] = Arrays::kHashBits && s != p0(a, s) ? kRowStoodFor : kRowListed; });
    }
}

// ---- stage 2: replay ------------------------------------------------------------------------------------------

constexpr uint32_t kNoRow = 0xFFFFFFFFu;

template <typename Arrays>
struct ReplayArgs {
    uint32_t num_matrices;
    double precision;
    Arrays g;
    const uint32_t * mat_flag;
    const uint8_t * active;      // [total rows] by row
    const uint32_t * sort_row;   // (EM problems: the stretches behind the rows of the lists)
    const uint32_t * position_of;
    const uint32_t * stretch_end;
    double * rowmax;
    uint32_t * mat_fast;
    uint32_t * mat_mid;
    uint32_t * mat_list;         // [M] size of the matrix's list (| kWholeMatrixBit: every row), 0: nothing to replay
    uint32_t * replay_list;      // [M] the matrices with a list, [M]: their number
    uint32_t * between_items;    // [2 x (total rows / kBetweenRows + M)] (matrix, slice of its rows) of step b
    uint32_t * between_count;
    uint32_t * row_items;        // [2 x total rows] (matrix, list index) of the rows of the lists with a pair table
    uint32_t * row_item_count;
    uint64_t * pair_base;        // [M] offset of the matrix's n x n pair table
    unsigned long long * pair_bytes;  // bytes of pair tables handed out
    uint8_t * pair_table;        // [kPairTableBytes] entry i * n + j: kPairLess (row i sorts before row j), kPairClose
    uint32_t * list_index;       // [total rows] index in the unsorted list (= in the pair table) of every sorted position
    uint32_t * order;            // [2 * total rows] list of matrix m at 2 * mat_row_off[m], sorted
    uint32_t * head_of;          // [total rows] list position of the run head of every list position
    uint8_t * close;             // [total rows] list position p is close to p - 1 and nothing lies between them
    uint8_t * barrier;           // [total rows] an inactive row lies between list positions p - 1 and p
    uint32_t * pair_column;      // [total rows] column that orders list positions p - 1 and p (kNoRow: not looked at)
    double * pair_lo;            // [total rows] their values in it, smaller
    double * pair_hi;            //              and larger
    uint64_t * pair_pattern;     // [total rows] zero pattern they share before that column
    uint32_t * info;
    bool debug;                  // RPVG_HIP_EM_COLLAPSE_DEBUG: slow workgroups of the runs kernel report where their time went
    bool no_lds_tables;          // RPVG_HIP_COLLAPSE_NO_LDS_TABLES (A/B): pair tables read from global memory as in round 3
    // group matrices whose diploid search ran on the values as built (rpvg_hip_groups::held_back_runs): its sums, to be adjusted
    // for every row the runs rewrite; part_pair == NULL: nobody has read the matrices yet
    SearchParts sums;
    uint32_t * rewritten_count;  // [M] rows of the matrix's list that take the values of a head (listRewrittenRows)
    bool walk_only;              // collapseRunsKernel stops behind the runs (collapseAdjustSumsKernel and collapseRewriteKernel follow)
};

// a1. every pair of rows of a small list, one thread each: order and closeness in one pass over the columns.  (A
// workgroup that sorts its list with a comparison network goes through dozens of dependent rounds of strided loads;
// here every comparison of the batch is in flight at once, and ranks and runs are then read off the table.)
// row i of matrix m's pair table; the calling threads stride its columns (thread `first` of `stride`)
template <typename Arrays>
__device__ __forceinline__ void pairTableRow(const ReplayArgs<Arrays> & a, const uint32_t m, const uint32_t i, const uint32_t first, const uint32_t stride) {
    const uint32_t n = a.mat_list[m] & kListSizeMask;
    const typename Arrays::View mv = viewOf(m, a.g);
    const uint32_t * list = a.order + 2 * a.g.rowOffset(m);
    uint8_t * table = a.pair_table + a.pair_base[m] + static_cast<uint64_t>(i) * n;
    const uint32_t row_i = list[i];
    const uint64_t pattern_i = mv.patternOf(row_i);
    for (uint32_t j = first; j < n; j += stride) {
        const uint32_t row_j = list[j];
        int less = -1;
        bool close = true;
        forEachColumnPair(mv, row_i, row_j, pattern_i | mv.patternOf(row_j), [&](const double x, const double y) {
            if (less < 0 && !tolerantEqual(x, y)) less = x < y ? 1 : 0;
            if (fabs(x - y) >= a.precision) close = false;
            return less >= 0 && !close;
        });
        if (less < 0) {
            const double x = mv.countOf(row_i), y = mv.countOf(row_j);
            less = (!tolerantEqual(x, y) && x < y) ? 1 : 0;
        }
        table[j] = (less ? kPairLess : 0) | (close ? kPairClose : 0);
    }
}

template <typename Arrays>
__global__ __launch_bounds__(64) void collapsePairTableKernel(const ReplayArgs<Arrays> a) {
    const uint32_t num_items = *a.row_item_count;
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
        pairTableRow(a, a.row_items[2 * static_cast<uint64_t>(item)], a.row_items[2 * static_cast<uint64_t>(item) + 1], threadIdx.x, blockDim.x);
    }
}

// a2. small lists sorted by rank: the number of rows that sort before a row (equal rows in list order).  Where the
// tolerant comparison is inconsistent the ranks may collide; such a list is sorted by the comparison network instead.
// the list of matrix m (a small one: it has a pair table) sorted by rank, and the column that orders every pair of neighbours
template <typename Arrays>
__device__ void rankList(const ReplayArgs<Arrays> & a, const uint32_t m) {
    __shared__ uint32_t lds_row[kPairwiseRows], lds_slot[kPairwiseRows];
    __shared__ uint8_t lds_table[kLdsTableRows * kLdsTableRows];
    __shared__ uint32_t collision;
    const uint32_t encoded = a.mat_list[m];
    if (encoded & kBigListBit) return;
    const uint32_t n = encoded;
    const uint64_t r0 = a.g.rowOffset(m);
    uint32_t * list = a.order + 2 * r0;
    uint32_t * list_index = a.list_index + r0;
    const uint8_t * table = a.pair_table + a.pair_base[m];
    __syncthreads();
    if (threadIdx.x == 0) collision = 0;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        lds_row[i] = list[i];
        lds_slot[i] = kNoRow;
    }
    __syncthreads();
    // (the table of a short list — nearly every list — moves to LDS first: a rank is 2 n dependent byte loads, and from global
    // memory the 100-row list of a batch made this kernel 0.1-0.2 ms of the collapse's critical path)
    const bool table_in_lds = n <= kLdsTableRows && !a.no_lds_tables;
    if (table_in_lds) {
        for (uint32_t k = threadIdx.x; k < n * n; k += blockDim.x) lds_table[k] = table[k];
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        uint32_t rank = 0;
        if (table_in_lds) {
            for (uint32_t j = 0; j < n; ++j) {
                const bool before = (lds_table[j * n + i] & kPairLess) != 0;
                const bool after = (lds_table[i * n + j] & kPairLess) != 0;
                rank += (before || (!after && j < i)) ? 1u : 0u;
            }
        } else {
            for (uint32_t j = 0; j < n; ++j) {
                const bool before = (table[static_cast<uint64_t>(j) * n + i] & kPairLess) != 0;
                const bool after = (table[static_cast<uint64_t>(i) * n + j] & kPairLess) != 0;
                rank += (before || (!after && j < i)) ? 1u : 0u;
            }
        }
        if (rank >= n || atomicExch(&lds_slot[rank], i) != kNoRow) collision = 1;
    }
    __syncthreads();
    if (collision) {  // (never seen; kept correct rather than fast) insertion sort with the comparator itself
        if (threadIdx.x == 0) {
            const typename Arrays::View mv = viewOf(m, a.g);
            for (uint32_t i = 0; i < n; ++i) lds_slot[i] = i;
            for (uint32_t i = 1; i < n; ++i) {
                const uint32_t moving = lds_slot[i];
                uint32_t k = i;
                while (k > 0 && rowLess(mv, lds_row[moving], lds_row[lds_slot[k - 1]])) {
                    lds_slot[k] = lds_slot[k - 1];
                    --k;
                }
                lds_slot[k] = moving;
            }
        }
        __syncthreads();
    }
    for (uint32_t p = threadIdx.x; p < n; p += blockDim.x) {
        list[p] = lds_row[lds_slot[p]];
        list_index[p] = lds_slot[p];
        a.barrier[r0 + p] = 0;
    }
    __syncthreads();
    // the column that orders every pair of neighbours, and the interval between them in it (collapseSortKernel)
    const typename Arrays::View mv = viewOf(m, a.g);
    for (uint32_t p = 1 + threadIdx.x; p < n; p += blockDim.x) {
        const uint32_t x = lds_row[lds_slot[p - 1]], y = lds_row[lds_slot[p]];
        uint32_t d = kNoRow;
        bool can_join = true;
        // (forEachColumnPair visits the columns in order but skips those in which both rows are zero: the column
        // index is recovered from the patterns)
        const uint64_t live = mv.patternOf(x) | mv.patternOf(y);
        uint64_t remaining = live;
        uint32_t wide = 64;
        forEachColumnPair(mv, x, y, live, [&](const double vx, const double vy) {
            uint32_t column;
            if (remaining) {
                column = static_cast<uint32_t>(__ffsll(static_cast<long long>(remaining)) - 1);
                remaining &= remaining - 1;
            } else if (wide < mv.G) {
                column = wide++;
            } else {
                column = mv.G;
            }
            if (fabs(vx - vy) >= 2 * a.precision) can_join = false;
            if (d == kNoRow && !tolerantEqual(vx, vy)) d = column;
            return !can_join;
        });
        const bool look = can_join && d != kNoRow;
        a.pair_column[r0 + p] = look ? d : kNoRow;
        if (look) {
            const double vx = mv.at(d, x), vy = mv.at(d, y);
            a.pair_lo[r0 + p] = fmin(vx, vy);
            a.pair_hi[r0 + p] = fmax(vx, vy);
            a.pair_pattern[r0 + p] = mv.patternOf(x) & (d >= 64 ? ~0ull : (1ull << d) - 1ull);
        }
    }
}

template <typename Arrays>
__global__ __launch_bounds__(256) void collapseRankKernel(const ReplayArgs<Arrays> a) {
    const uint32_t num_items = a.replay_list[a.num_matrices];
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) rankList(a, a.replay_list[item]);
}

// a3. big lists (more than kPairwiseRows rows, whole matrices): sorted with the reference's comparator in a
// comparison network, and for every pair of neighbours the column that orders them
template <typename Arrays>
__global__ __launch_bounds__(kSortThreads) void collapseSortKernel(const ReplayArgs<Arrays> a) {
    __shared__ uint32_t lds_list[kListLdsRows];
    __shared__ uint64_t lds_pattern[kListLdsRows];  // zero pattern of the row at each list position (LDS lists)
    // over the matrices with a list (a workgroup of this kernel takes a CU's worth of LDS: one per matrix of the batch, each
    // only to find that its matrix has no big list, took 0.35-0.8 ms next to the other lane's kernels)
    const uint32_t num_items = a.replay_list[a.num_matrices];
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
    __syncthreads();  // the lists of the matrix before are done with
    const uint32_t m = a.replay_list[item];
    const uint32_t encoded = a.mat_list[m];
    if (!(encoded & kBigListBit)) continue;  // a small list (pair table, collapseRankKernel)
    const bool whole = (encoded & kWholeMatrixBit) != 0;
    const uint64_t n = encoded & kListSizeMask;
    const typename Arrays::View mv = viewOf(m, a.g);
    const uint64_t r0 = a.g.rowOffset(m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, num_waves = blockDim.x >> 6;
    uint64_t padded = 1;
    while (padded < n) padded <<= 1;
    uint32_t * global_order = a.order + 2 * r0;
    uint32_t * order = padded <= kListLdsRows ? lds_list : global_order;
    for (uint64_t i = threadIdx.x; i < padded; i += blockDim.x) order[i] = i < n ? (whole ? static_cast<uint32_t>(i) : global_order[i]) : kNoRow;
    __syncthreads();
    const bool in_lds = order == lds_list;
    if (in_lds) {
        for (uint64_t i = threadIdx.x; i < padded; i += blockDim.x) lds_pattern[i] = order[i] == kNoRow ? 0ull : mv.patternOf(order[i]);
    }
    __syncthreads();
    // bitonic network with the reference's comparator; kNoRow sorts behind every row
    for (uint64_t k = 2; k <= padded; k <<= 1) {
        for (uint64_t j = k >> 1; j > 0; j >>= 1) {
            for (uint64_t t = threadIdx.x; t < (padded >> 1); t += blockDim.x) {
                const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j of i is clear
                const uint64_t l = i | j;
                const uint32_t x = order[i], y = order[l];
                const bool ascending = (i & k) == 0;
                bool swap;
                if (x == kNoRow || y == kNoRow) {
                    swap = ascending ? (x == kNoRow && y != kNoRow) : (y == kNoRow && x != kNoRow);
                } else {
                    const uint64_t px = in_lds ? lds_pattern[i] : mv.patternOf(x), py = in_lds ? lds_pattern[l] : mv.patternOf(y);
                    swap = ascending ? rowLess(mv, y, x, py, px) : rowLess(mv, x, y, px, py);
                }
                if (swap) {
                    order[i] = y;
                    order[l] = x;
                    if (in_lds) {
                        const uint64_t px = lds_pattern[i];
                        lds_pattern[i] = lds_pattern[l];
                        lds_pattern[l] = px;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (order != global_order) {
        for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) global_order[i] = order[i];
    }
    uint8_t * barrier = a.barrier + r0;
    for (uint64_t p = threadIdx.x; p < n; p += blockDim.x) barrier[p] = 0;
    if (whole) continue;
    // One wave per pair of neighbours: d, the first column in which they differ, and the interval between them in it.
    // A row x with a <= x <= b in the reference's order equals both up to rounding before column d and lies between
    // them in column d.  A row that joins a run is within prob_precision of a head its predecessor is within
    // prob_precision of (or the predecessor is that head): only neighbours that close can be parted by a row.
    uint32_t * pair_column = a.pair_column + r0;
    for (uint64_t p = 1 + wave; p < n; p += num_waves) {
        const uint32_t x = order[p - 1], y = order[p];
        uint32_t d = mv.G + 1;
        bool can_join = true;
        for (uint32_t c0 = 0; c0 <= mv.G; c0 += 64) {
            const uint32_t c = c0 + lane;
            const double vx = c <= mv.G ? mv.at(c, x) : 0.0, vy = c <= mv.G ? mv.at(c, y) : 0.0;
            if (__ballot(fabs(vx - vy) >= 2 * a.precision)) can_join = false;
            const unsigned long long differs = __ballot(c <= mv.G && !tolerantEqual(vx, vy));
            if (differs && d > mv.G) d = c0 + static_cast<uint32_t>(__ffsll(static_cast<long long>(differs)) - 1);
        }
        if (lane == 0) {
            const bool look = can_join && d <= mv.G;  // (equal in every column: whatever lies between them is their equal, too)
            pair_column[p] = look ? d : kNoRow;
            if (look) {
                const double vx = mv.at(d, x), vy = mv.at(d, y);
                a.pair_lo[r0 + p] = fmin(vx, vy);
                a.pair_hi[r0 + p] = fmax(vx, vy);
                a.pair_pattern[r0 + p] = mv.patternOf(x) & (d >= 64 ? ~0ull : (1ull << d) - 1ull);
            }
        }
    }
    }
}

// b. inactive rows between neighbours of the lists: work item = (matrix with a list, slice of its rows)
// the rows [slice * kBetweenRows, ...) of matrix m against the neighbour pairs of its list
template <typename Arrays>
__device__ void betweenSlice(const ReplayArgs<Arrays> & a, const uint32_t m, const uint32_t slice) {
    __shared__ uint32_t lds_column[kPairChunk];
    __shared__ double lds_lo[kPairChunk], lds_hi[kPairChunk];
    __shared__ uint64_t lds_pattern[kPairChunk], lds_before[kPairChunk];
    const uint64_t n = a.mat_list[m] & kListSizeMask;  // (not a whole matrix: those have no items)
    const typename Arrays::View mv = viewOf(m, a.g);
    const uint64_t r0 = a.g.rowOffset(m);
    const uint8_t * active = a.active + r0;
    const uint32_t * order = a.order + 2 * r0;
    for (uint64_t p0 = 1; p0 < n; p0 += kPairChunk) {
        const uint32_t chunk = static_cast<uint32_t>(min(static_cast<uint64_t>(kPairChunk), n - p0));
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < chunk; k += blockDim.x) {
            const uint32_t d = a.pair_column[r0 + p0 + k];
            lds_column[k] = d;
            if (d != kNoRow) {
                lds_lo[k] = a.pair_lo[r0 + p0 + k];
                lds_hi[k] = a.pair_hi[r0 + p0 + k];
                lds_pattern[k] = a.pair_pattern[r0 + p0 + k];
                lds_before[k] = d >= 64 ? ~0ull : (1ull << d) - 1ull;
            }
        }
        __syncthreads();
        const uint64_t x_end = min(mv.R, (slice + 1ull) * kBetweenRows);
        for (uint64_t x = slice * static_cast<uint64_t>(kBetweenRows) + threadIdx.x; x < x_end; x += blockDim.x) {
            if (active[x]) continue;
            const uint64_t pattern_x = mv.patternOf(x);
            uint32_t loaded_column = kNoRow;
            double vx = 0.0;
            for (uint32_t k = 0; k < chunk; ++k) {
                const uint32_t d = lds_column[k];
                if (d == kNoRow || (pattern_x & lds_before[k]) != lds_pattern[k]) continue;
                if (d != loaded_column) {
                    vx = mv.at(d, static_cast<uint32_t>(x));
                    loaded_column = d;
                }
                const double lo = lds_lo[k], hi = lds_hi[k];
                if (!((vx >= lo || tolerantEqual(vx, lo)) && (vx <= hi || tolerantEqual(vx, hi)))) continue;
                const uint64_t p = p0 + k;
                if (!rowLess(mv, static_cast<uint32_t>(x), order[p - 1]) && !rowLess(mv, order[p], static_cast<uint32_t>(x))) a.barrier[r0 + p] = 1;
            }
        }
    }
}

template <typename Arrays>
__global__ __launch_bounds__(kBetweenThreads) void collapseBetweenKernel(const ReplayArgs<Arrays> a) {
    const uint32_t num_items = *a.between_count;
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
        betweenSlice(a, a.between_items[2 * static_cast<uint64_t>(item)], a.between_items[2 * static_cast<uint64_t>(item) + 1]);
    }
}

// The diploid search has summed count * log(noise + (u_a + u_b) / 2) over the rows AS BUILT (pairTile2Kernel: per chunk of rows,
// pair of columns a <= b, and column; rpvg_hip_groups::held_back_runs).  A row that takes the values of its head contributes the
// head's term with its own count: the difference, count * log(after / before), goes to the sums of the row's chunk.  Work item =
// (matrix with a list, slice of its G x G table of cells): the rewritten rows are staged in LDS some at a time (old and new
// values: the global loads of a batch of rows in flight together), a thread owns its cells throughout — every sum has one
// writer and the order of its additions is the list's: the result does not depend on how threads run — and keeps a cell's
// difference in a register while the rows stay in one chunk (most matrices have one).  The rows are few (some hundred per
// configs[2] batch) but a matrix may hold most of them: on one workgroup, cell by cell from global memory with two logarithms
// each, they were 1.5 ms behind the search.
constexpr uint32_t kAdjustSlices = 16;

__device__ void adjustSearchSums(const ReplayArgs<MatrixArrays> & a, const uint32_t m, const uint32_t slice) {
    const uint64_t n = a.mat_list[m] & kListSizeMask;
    const MatrixView mv = viewOf(m, a.g);
    const uint64_t R = mv.R;
    const uint64_t r0 = a.g.rowOffset(m);
    const uint32_t * order = a.order + 2 * r0;
    const uint32_t * head_of = a.head_of + r0;
    const double * M = a.g.values + a.g.mat_val_off[m];
    const double * nz = a.g.row_noise + r0;
    const uint32_t G = mv.G;
    constexpr uint32_t kStageDoubles = 4096;
    constexpr uint32_t kStageRows = 32;
    __shared__ double stage[kStageDoubles];                      // [row of the batch][old | new][column]
    __shared__ double stage_noise[2 * kStageRows], stage_count[kStageRows];
    __shared__ uint32_t stage_chunk[kStageRows];
    const uint32_t rows_per_stage = G <= kStageDoubles / 2 ? min(kStageRows, kStageDoubles / (2 * G)) : 0u;
    double * pairs = a.sums.part_pair + a.sums.pair_part_off[m];
    double * singles = a.sums.part_marginal + a.sums.col_part_off[m];
    const double * cnt = a.g.row_count + r0;
    // count * log(after / before): after / before - 1 is tiny for rows within prob_precision of each other unless the values
    // themselves are — the series then, the logarithm otherwise
    auto difference = [](const double c, const double before, const double after) {
        if (before == after) return 0.0;
        const double x = (after - before) / before;
        if (fabs(x) < 1e-4) return c * (x * (1.0 - x * (0.5 - x * (1.0 / 3.0 - 0.25 * x))));
        return c * log1p(x);
    };
    // the list positions whose rows are rewritten, in list order (the walk of the runs listed them: runsOfMatrix)
    const uint32_t * rewritten = a.pair_column + r0;
    const uint32_t num_rewritten = a.rewritten_count[m];
    (void) n;
    for (uint32_t i0 = 0; rows_per_stage && i0 < num_rewritten; i0 += rows_per_stage) {
        const uint32_t rows = min(rows_per_stage, num_rewritten - i0);
        __syncthreads();  // (the batch before is done with the LDS)
        if (threadIdx.x < rows) {
            const uint64_t q = rewritten[i0 + threadIdx.x];
            const uint32_t dst = order[q], src = order[head_of[q]];
            stage_chunk[threadIdx.x] = dst / a.sums.chunk_rows;
            stage_noise[2 * threadIdx.x] = nz[dst];
            stage_noise[2 * threadIdx.x + 1] = nz[src];
            stage_count[threadIdx.x] = cnt[dst];
        }
        __syncthreads();
        for (uint32_t idx = threadIdx.x; idx < rows * G; idx += blockDim.x) {
            const uint32_t row = idx / G, c = idx % G;
            const uint64_t q = rewritten[i0 + row];
            stage[(2 * row) * G + c] = M[static_cast<uint64_t>(c) * R + order[q]];
            stage[(2 * row + 1) * G + c] = M[static_cast<uint64_t>(c) * R + order[head_of[q]]];
        }
        __syncthreads();
        for (uint64_t cell = static_cast<uint64_t>(slice) * blockDim.x + threadIdx.x; cell < static_cast<uint64_t>(G) * G; cell += static_cast<uint64_t>(kAdjustSlices) * blockDim.x) {
            const uint32_t x = static_cast<uint32_t>(cell / G), y = static_cast<uint32_t>(cell % G);
            if (x > y) continue;
            double sum = 0.0, single_sum = 0.0;
            uint32_t sum_chunk = kNoRow;
            auto flush = [&]() {
                if (sum_chunk == kNoRow) return;
                if (sum != 0.0) pairs[static_cast<uint64_t>(sum_chunk) * G * G + cell] += sum;
                if (x == y && single_sum != 0.0) singles[static_cast<uint64_t>(sum_chunk) * G + x] += single_sum;
                sum = 0.0;
                single_sum = 0.0;
            };
            for (uint32_t row = 0; row < rows; ++row) {
                const uint32_t chunk = stage_chunk[row];
                if (chunk != sum_chunk) {
                    flush();
                    sum_chunk = chunk;
                }
                const double * before_row = stage + (2 * row) * G, * after_row = before_row + G;
                const double old_noise = stage_noise[2 * row], new_noise = stage_noise[2 * row + 1], c = stage_count[row];
                // (the search's own arithmetic: 2 x = (u_a + 2 noise) + u_b)
                sum += difference(c, 0.5 * (fma(2.0, old_noise, before_row[x]) + before_row[y]), 0.5 * (fma(2.0, new_noise, after_row[x]) + after_row[y]));
                if (x == y) single_sum += difference(c, before_row[x] + old_noise, after_row[x] + new_noise);
            }
            flush();
        }
    }
}

// the list positions of matrix m whose rows take the values of their head, in list order, into the scratch of a stage that is
// done (pair_column), and their number
__device__ void listRewrittenRows(const ReplayArgs<MatrixArrays> & a, const uint32_t m, const uint64_t n, const uint32_t * head_of) {
    __shared__ uint32_t rewritten_total, wave_rewritten[4];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t * rewritten = a.pair_column + a.g.rowOffset(m);
    if (threadIdx.x == 0) rewritten_total = 0;
    __syncthreads();
    for (uint64_t q0 = 0; q0 < n; q0 += blockDim.x) {
        const uint64_t q = q0 + threadIdx.x;
        const bool mine = q < n && head_of[q] != q;
        const unsigned long long ballot = __ballot(mine);
        if (lane == 0) wave_rewritten[threadIdx.x >> 6] = __popcll(ballot);
        __syncthreads();
        uint32_t at = rewritten_total + __popcll(ballot & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) at += wave_rewritten[w];
        if (mine) rewritten[at] = static_cast<uint32_t>(q);
        __syncthreads();
        if (threadIdx.x == 0) rewritten_total += wave_rewritten[0] + wave_rewritten[1] + wave_rewritten[2] + wave_rewritten[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.rewritten_count[m] = rewritten_total;
}
__device__ void listRewrittenRows(const ReplayArgs<CsrArrays> &, const uint32_t, const uint64_t, const uint32_t *) {}

// What a run does to its rows.  Group matrices: the rows of a run take the values of its head — the consumers are sums over
// rows of count * log(noise + columns), so "merged into the head" is "takes the values of the head" with the row's own
// count; a wave per row, its lanes over the columns.
__device__ __forceinline__ void finishRuns(const ReplayArgs<MatrixArrays> & a, const uint32_t m, const uint64_t n, const uint32_t * order,
                                           const uint32_t * head_of, uint32_t * demote, const bool whole) {
    (void) whole;
    const int lane = threadIdx.x & 63;
    const MatrixView mv = viewOf(m, a.g);
    const uint64_t R = mv.R;
    const uint64_t r0 = a.g.rowOffset(m);
    double * M = a.g.values + a.g.mat_val_off[m];
    double * nz = a.g.row_noise + r0;
    double * rm = a.rowmax + r0;
    const uint32_t fast_mid_end = a.mat_mid[m];
    uint32_t replaced = 0;
    for (uint64_t q = threadIdx.x >> 6; q < n; q += blockDim.x >> 6) {
        const uint32_t h = head_of[q];
        if (h == q) continue;
        const uint32_t dst = order[q], src = order[h];
        // a copy of its head (the rows of a stretch join their runs together) takes its head's values and keeps its own: only
        // the rows whose values CHANGE count as replaced
        bool changed = nz[dst] != nz[src];
        // (a column is a cache line of its own, in either row: eight loads in flight per lane — one at a time, a merged row of a
        // 2 000-column matrix took a wave 60 us)
        for (uint32_t c0 = lane; c0 < mv.G; c0 += 64 * 8) {
            double v[8], old[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t c = c0 + 64 * k;
                v[k] = c < mv.G ? __builtin_nontemporal_load(&M[static_cast<uint64_t>(c) * R + src]) : 0.0;
                old[k] = c < mv.G ? __builtin_nontemporal_load(&M[static_cast<uint64_t>(c) * R + dst]) : 0.0;
            }
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                const uint32_t c = c0 + 64 * k;
                changed = changed || old[k] != v[k];
                if (c < mv.G) M[static_cast<uint64_t>(c) * R + dst] = v[k];
            }
        }
        changed = __any(changed) != 0;  // (a wave per row: uniform)
        if (lane == 0) {
            const double noise = nz[src];
            nz[dst] = noise;
            rm[dst] = rm[src];
            if (changed) ++replaced;
            // a product-path row (LogProduct, common.hpp) needs noise >= kProductMinNoise: if the head's is below,
            // the whole matrix takes the logarithm path
            if (dst < fast_mid_end && !(noise >= kProductMinNoise)) *demote = 1;
        }
    }
    if (replaced) atomicAdd(&a.info[kInfoRowsReplaced], replaced);
    __syncthreads();
    if (threadIdx.x == 0 && *demote) {
        a.mat_fast[m] = 0;
        a.mat_mid[m] = 0;
    }
}

// EM problems (src/path_abundance_estimator.cpp:266,668 -> src/path_estimator.cpp:219-259): the head keeps its values and
// the counts of its run add up — in CSR terms a merged row's count moves to its run head (read counts are integers: the
// sums are exact in any order).  A row of the list stands for its stretch (rows of equal cells: all of them join the run
// with it); in a whole-matrix list every row is there itself.  The counts after the merges go to a second array (the
// first EM pass may still be reading the original ones); the problem is flagged for the second pass.
__device__ __forceinline__ void finishRuns(const ReplayArgs<CsrArrays> & a, const uint32_t p, const uint64_t n, const uint32_t * order,
                                           const uint32_t * head_of, uint32_t * demote, const bool whole) {
    (void) demote;
    __shared__ uint32_t any_merge, members_total;
    const uint64_t r0 = a.g.rowOffset(p);
    const uint64_t R = a.g.numRows(p);
    double * merged = a.g.merged_count + r0;
    const double * count = a.g.problems.rows(p).count;
    uint8_t * joined = a.barrier + r0;  // (free again: the runs are known) by list position: 1 = a head that rows joined
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, num_waves = blockDim.x >> 6;
    if (threadIdx.x == 0) any_merge = 0, members_total = 0;
    for (uint64_t r = threadIdx.x; r < R; r += blockDim.x) merged[r] = count[r];
    for (uint64_t q = threadIdx.x; q < n; q += blockDim.x) joined[q] = 0;
    __syncthreads();
    for (uint64_t q = threadIdx.x; q < n; q += blockDim.x) {
        if (head_of[q] != q) joined[head_of[q]] = 1, any_merge = 1;  // (several writers, one value)
    }
    __syncthreads();
    if (any_merge) {  // (uniform)
        // the rows of the runs with more than a head, stretch by stretch (a wave each): first their counts go...
        auto forStretchOf = [&](const uint64_t q, auto visit) {  // visit(row of the problem)
            if (whole) {
                if (lane == 0) visit(order[q]);
                return;
            }
            const uint32_t first = a.position_of[r0 + order[q]], end = a.stretch_end[first];
            for (uint32_t s = first + lane; s < end; s += 64) visit(static_cast<uint32_t>(a.sort_row[s] - r0));
        };
        for (uint64_t q = wave; q < n; q += num_waves) {
            if (head_of[q] == q && !joined[q]) continue;
            forStretchOf(q, [&](const uint32_t row) { merged[row] = 0.0; });
        }
        __syncthreads();
        // ... then they arrive at the head
        for (uint64_t q = wave; q < n; q += num_waves) {
            const uint32_t h = head_of[q];
            if (h == q && !joined[q]) continue;
            double sum = 0.0;
            uint32_t rows = 0;
            forStretchOf(q, [&](const uint32_t row) { sum += count[row]; ++rows; });
            for (int step = 32; step; step >>= 1) {
                sum += __shfl_xor(sum, step);
                rows += __shfl_xor(rows, step);
            }
            if (lane == 0) {
                atomicAdd(&merged[order[h]], sum);
                atomicAdd(&members_total, h == q ? rows - 1 : rows);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            a.g.problem_merged[p] = 1;
            atomicAdd(a.g.merged_problems, 1u);
            atomicAdd(&a.info[kInfoRowsReplaced], members_total);
        }
    }
    __syncthreads();
}

// c. runs and values of matrix m (the workgroup's)
template <typename Arrays>
__device__ void runsOfMatrix(const ReplayArgs<Arrays> & a, const uint32_t m) {
    __shared__ uint32_t demote;
    __shared__ uint32_t walk_at, run_end;
    const uint32_t encoded = a.mat_list[m];
    const uint64_t n = encoded & kListSizeMask;
    const bool tabled = !(encoded & kBigListBit);
    const typename Arrays::View mv = viewOf(m, a.g);
    const uint64_t r0 = a.g.rowOffset(m);
    const uint32_t * order = a.order + 2 * r0;
    const uint32_t * list_index = a.list_index + r0;
    const uint8_t * table = a.pair_table + (tabled ? a.pair_base[m] : 0);
    uint32_t * head_of = a.head_of + r0;
    uint8_t * close = a.close + r0;
    const uint8_t * barrier = a.barrier + r0;
    // list positions p, q hold rows within prob_precision of each other: read off the pair table, or compared
    auto closeRows = [&](const uint64_t p, const uint64_t q) {
        if (tabled) return (table[static_cast<uint64_t>(list_index[p]) * n + list_index[q]] & kPairClose) != 0;
        return rowsClose(mv, order[p], order[q], a.precision, nullptr);
    };
    __syncthreads();
    const long long clock_begin = wall_clock64();
    if (threadIdx.x == 0) demote = 0;
    if (tabled && n <= kLdsTableRows && !a.no_lds_tables) {
        // A short list with a pair table — nearly every list: table, barriers and heads in LDS, and ONE thread walks the runs
        // (src/path_estimator.cpp:226-255: a row joins the run of the current head if nothing parts them and it is close to the
        // head, otherwise it becomes the head).  The walk below, a workgroup stepping from head to head through barriers and
        // global memory, took 0.1-0.3 ms for the 100-row list of a batch.
        __shared__ uint8_t lds_table[kLdsTableRows * kLdsTableRows];
        __shared__ uint8_t lds_barrier[kLdsTableRows];
        __shared__ uint32_t lds_index[kLdsTableRows], lds_head[kLdsTableRows];
        const uint32_t nn = static_cast<uint32_t>(n);
        for (uint32_t k = threadIdx.x; k < nn * nn; k += blockDim.x) lds_table[k] = table[k];
        for (uint32_t p = threadIdx.x; p < nn; p += blockDim.x) {
            lds_barrier[p] = barrier[p];
            lds_index[p] = list_index[p];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t h = 0;
            while (h < nn) {
                uint32_t q = h + 1;
                while (q < nn && !lds_barrier[q] && (lds_table[lds_index[h] * nn + lds_index[q]] & kPairClose) != 0) ++q;
                for (uint32_t r = h; r < q; ++r) lds_head[r] = h;
                h = q;
            }
        }
        __syncthreads();
        for (uint32_t p = threadIdx.x; p < nn; p += blockDim.x) head_of[p] = lds_head[p];
        __syncthreads();
        if (a.walk_only) listRewrittenRows(a, m, n, head_of);
        else finishRuns(a, m, n, order, head_of, &demote, (encoded & kWholeMatrixBit) != 0);
        return;
    }
    for (uint64_t p = threadIdx.x; p < n; p += blockDim.x) {
        head_of[p] = kNoRow;
        close[p] = (p > 0 && !barrier[p] && closeRows(p - 1, p)) ? 1 : 0;
    }
    __syncthreads();
    // Runs (src/path_estimator.cpp:226-255): a row joins the run of the current head if it is close to the head,
    // otherwise it becomes the head.  The workgroup walks from head to head: a head whose successor is not close to it
    // (nearly every one) is a run of its own and costs one flag; a head with followers has the whole workgroup look
    // for the end of its run, 256 candidates at a time.  (Round 2 had every list position find "where would the next
    // head be if I were one" on its own before one thread walked the heads: with n rows all close to each other —
    // an EM problem over 10^5 reads that differ in the ninth digit — that is n^2 / 2 comparisons for the one run.)
    if (threadIdx.x == 0) walk_at = 0;
    __syncthreads();
    while (walk_at < n) {  // (uniform: walk_at only changes between barriers)
        const uint64_t h = walk_at;
        if (h + 1 >= n || !close[h + 1]) {
            // a stretch of single-row runs, up to the next row with a close successor: the workgroup looks for it, 256
            // positions at a time (one thread stepping through a list of a few hundred single rows, a dependent load per
            // step, was most of this kernel's 0.23 ms on the group matrices)
            if (threadIdx.x == 0) run_end = static_cast<uint32_t>(n);
            __syncthreads();
            for (uint64_t q0 = h + 1; q0 < n && run_end == n; q0 += blockDim.x) {  // (uniform: run_end read behind the barrier below)
                const uint64_t q = q0 + threadIdx.x;
                if (q + 1 < n && close[q + 1]) atomicMin(&run_end, static_cast<uint32_t>(q));
                __syncthreads();
            }
            const uint64_t stretch_end = run_end;
            for (uint64_t q = h + threadIdx.x; q < stretch_end; q += blockDim.x) head_of[q] = static_cast<uint32_t>(q);
            __syncthreads();
            if (threadIdx.x == 0) walk_at = static_cast<uint32_t>(stretch_end);
            __syncthreads();
            continue;
        }
        if (threadIdx.x == 0) run_end = static_cast<uint32_t>(n);
        __syncthreads();
        for (uint64_t q0 = h + 2; q0 < n && run_end == n; q0 += blockDim.x) {  // (uniform: run_end read behind the barrier below)
            const uint64_t q = q0 + threadIdx.x;
            if (q < n && (barrier[q] != 0 || !closeRows(h, q))) atomicMin(&run_end, static_cast<uint32_t>(q));
            __syncthreads();
        }
        const uint64_t end = run_end;
        for (uint64_t q = h + threadIdx.x; q < end; q += blockDim.x) head_of[q] = static_cast<uint32_t>(h);
        __syncthreads();
        if (threadIdx.x == 0) walk_at = static_cast<uint32_t>(end);
        __syncthreads();
    }
    const long long clock_walked = wall_clock64();
    if (a.walk_only) listRewrittenRows(a, m, n, head_of);
    else finishRuns(a, m, n, order, head_of, &demote, (encoded & kWholeMatrixBit) != 0);
    if (a.debug && threadIdx.x == 0 && wall_clock64() - clock_begin > 2000) {
        printf("[runs] matrix %u rows %llu cols %u list %llu tabled %d: walk %lld finish %lld (10 ns)\n", m, static_cast<unsigned long long>(mv.R), mv.G,
               static_cast<unsigned long long>(n), tabled ? 1 : 0, clock_walked - clock_begin, wall_clock64() - clock_walked);
    }
}

// a0. the list of a matrix: its active rows (the replay then only touches those), or all of them.  Persistent workgroups, a
// grid-stride loop over the matrices: most have no flag and cost a load.
// (Round 4 tried the whole replay of a short list right here, twice — pair table, ranks, rows between neighbours, runs, one stage
// after the other behind workgroup barriers instead of six dependent launches; first a workgroup per matrix with the tables in
// global memory, then persistent workgroups with the tables in LDS: 12.5 against 11.5 and 11.4 against 10.3 ms per configs[2]
// batch.  The staged kernels spread a matrix's pairs and row slices over many workgroups; one workgroup walking the stages of
// its matrices in turn is the longer chain, and the batch waits for the longest.)
template <typename Arrays>
__global__ __launch_bounds__(256) void collapseListKernel(const ReplayArgs<Arrays> a) {
    __shared__ uint32_t list_size;
    for (uint32_t m = blockIdx.x; m < a.num_matrices; m += gridDim.x) {
        const uint32_t flag = a.mat_flag[m];
        if (flag == kFlagNone) {
            if (threadIdx.x == 0) a.mat_list[m] = 0;
            continue;
        }
        const uint64_t R = a.g.numRows(m);
        const uint64_t r0 = a.g.rowOffset(m);
        const uint8_t * active = a.active + r0;
        uint32_t * list = a.order + 2 * r0;
        __syncthreads();  // (the matrix before is done with the shared words)
        if (threadIdx.x == 0) list_size = 0;
        __syncthreads();
        if (flag != kFlagWholeMatrix) {
            // (eight flags per load where the alignment allows: the largest matrix of a batch has 10^5 rows, and a byte per thread
            // and step was 50 us of this kernel)
            const uint64_t head = min(R, static_cast<uint64_t>((8 - (reinterpret_cast<uintptr_t>(active) & 7)) & 7));
            for (uint64_t i = threadIdx.x; i < head; i += blockDim.x) {
                if (active[i] == kRowListed) list[atomicAdd(&list_size, 1u)] = static_cast<uint32_t>(i);
            }
            const uint64_t words = (R - head) / 8;
            const uint64_t * active_words = reinterpret_cast<const uint64_t *>(active + head);
            for (uint64_t w = threadIdx.x; w < words; w += blockDim.x) {
                uint64_t flags = active_words[w];
                for (uint32_t k = 0; flags; ++k, flags >>= 8) {
                    if ((flags & 0xFF) == kRowListed) list[atomicAdd(&list_size, 1u)] = static_cast<uint32_t>(head + 8 * w + k);
                }
            }
            for (uint64_t i = head + 8 * words + threadIdx.x; i < R; i += blockDim.x) {
                if (active[i] == kRowListed) list[atomicAdd(&list_size, 1u)] = static_cast<uint32_t>(i);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const bool whole = flag == kFlagWholeMatrix;
            const uint64_t n = whole ? R : list_size;
            if (n < 2) {
                a.mat_list[m] = 0;
            } else {
                uint32_t encoded = static_cast<uint32_t>(n);
                if (whole) encoded |= kWholeMatrixBit | kBigListBit;
                else if (n > kPairwiseRows) encoded |= kBigListBit;
                else {
                    const unsigned long long base = atomicAdd(a.pair_bytes, static_cast<unsigned long long>(n * n));
                    if (base + n * n > kPairTableBytes) encoded |= kBigListBit;
                    else {
                        a.pair_base[m] = base;
                        const uint32_t first = atomicAdd(a.row_item_count, static_cast<uint32_t>(n));
                        for (uint32_t i = 0; i < n; ++i) {
                            a.row_items[2 * static_cast<uint64_t>(first + i)] = m;
                            a.row_items[2 * static_cast<uint64_t>(first + i) + 1] = i;
                        }
                    }
                }
                a.mat_list[m] = encoded;
                a.replay_list[atomicAdd(&a.replay_list[a.num_matrices], 1u)] = m;
                if (!whole) {  // work items of step b: (matrix, slice of kBetweenRows rows)
                    const uint32_t slices = static_cast<uint32_t>((R + kBetweenRows - 1) / kBetweenRows);
                    const uint32_t first = atomicAdd(a.between_count, slices);
                    for (uint32_t k = 0; k < slices; ++k) {
                        a.between_items[2 * static_cast<uint64_t>(first + k)] = m;
                        a.between_items[2 * static_cast<uint64_t>(first + k) + 1] = k;
                    }
                }
                atomicAdd(&a.info[kInfoMatrices], 1u);
                atomicAdd(&a.info[kInfoActiveRows], static_cast<uint32_t>(n));
                if (whole) atomicAdd(&a.info[kInfoWholeMatrices], 1u);
            }
        }
    }
}

// work item = matrix with a list
template <typename Arrays>
__global__ __launch_bounds__(256) void collapseRunsKernel(const ReplayArgs<Arrays> a) {
    const uint32_t num_items = a.replay_list[a.num_matrices];
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) runsOfMatrix(a, a.replay_list[item]);
}

// behind a walk-only collapseRunsKernel: the search's sums ((matrix with a list, slice of its cells) per work item), ...
__global__ __launch_bounds__(256) void collapseAdjustSumsKernel(const ReplayArgs<MatrixArrays> a) {
    const uint32_t num_items = a.replay_list[a.num_matrices] * kAdjustSlices;
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
        const uint32_t m = a.replay_list[item / kAdjustSlices];
        if (a.rewritten_count[m] == 0) continue;  // (uniform)
        __syncthreads();
        adjustSearchSums(a, m, item % kAdjustSlices);
    }
}

// ... and the values of the heads over their runs
__global__ __launch_bounds__(256) void collapseRewriteKernel(const ReplayArgs<MatrixArrays> a) {
    __shared__ uint32_t demote;
    const uint32_t num_items = a.replay_list[a.num_matrices];
    for (uint32_t item = blockIdx.x; item < num_items; item += gridDim.x) {
        const uint32_t m = a.replay_list[item];
        const uint32_t encoded = a.mat_list[m];
        __syncthreads();
        if (threadIdx.x == 0) demote = 0;
        __syncthreads();
        finishRuns(a, m, encoded & kListSizeMask, a.order + 2 * a.g.rowOffset(m), a.head_of + a.g.rowOffset(m), &demote, (encoded & kWholeMatrixBit) != 0);
    }
}

}  // namespace

namespace {

// ---- stage 0: the rows of every matrix in the order of their sort keys — without a library sort ---------------------------
// What the window scans need: the rows of a matrix ordered by (projection[, hash of the cells]), rows of equal keys in row
// order.  The keys carry the matrix above the projection and the rows of a matrix are contiguous, so the order is one
// segment per matrix, and nearly every segment fits a few KB of LDS: a workgroup loads up to 1 024 rows as 64-bit words
// [projection 24 | hash H | row 20 | largest value 20 - H], sorts them with a bitonic network and — the usual case, the whole
// matrix in one go — writes the sorted keys and rows, every row's sorted position, "equal to its predecessor" and the
// stretch starts itself.  A larger matrix lists its chunks of 2 048 rows; they are sorted the same way into a buffer and
// merged pairwise, round by round (merge path: every thread finds its eight output words by a binary search on its
// diagonal) — the host launches ceil(log2(chunks)) rounds for the largest matrix there can be, a matrix takes part in
// the rounds it needs itself; a last kernel writes what the one-chunk matrices wrote in the sort.  (Rounds 2-3:
// hipcub::DeviceRadixSort over all rows of all matrices — five passes of three launches
// each, 0.31 ms of a lane's 1.2 ms of collapse standing alone — and DeviceSegmentedRadixSort for the EM problems, 0.5 ms in
// one kernel behind a host wait for its partition sizes, plus a kernel for the keys and one for "equal to its predecessor"
// that walked every row slot.  A first version of this one sorted chunks of 8 192 rows on 512 threads whatever the matrix —
// 0.28 ms for the 5 000 matrices of a configs[2] batch, two workgroups per CU — and ranked every element of a large matrix in
// every other chunk of it: chunks squared, 0.17-0.64 ms.)
// (The network itself: segment_sort_plan.hpp has the schedule — size classes, kind, partner and direction of every stage, the
// rounds a segment needs — and sortWordsInRegisters below runs it with the words in registers: a lane holds up to eight
// consecutive elements, stages inside a lane are register compare-exchanges, stages inside a wavefront lane exchanges, and only
// the stages across wavefronts go through LDS behind a barrier.  docs/design/kernels-collapse.md, "Segment sort in registers".)
constexpr uint32_t kMergeTile = 1024;                       // output words of a merge round per work item

template <int HASH>
__device__ __forceinline__ uint64_t packSortWord(const uint64_t key, const uint32_t row) {
    constexpr int low = kCollapseLargestBits - HASH;  // bits of the key that are not sorted on
    const uint64_t sorted = (key & ((1ull << kCollapseMatrixShift) - 1)) >> low;
    return (sorted << (rpvg_sort::kRowBits + low)) | (static_cast<uint64_t>(row) << low) | (key & ((1ull << low) - 1));
}
template <int HASH>
__device__ __forceinline__ uint32_t sortWordRow(const uint64_t word) { return static_cast<uint32_t>(word >> (kCollapseLargestBits - HASH)) & ((1u << rpvg_sort::kRowBits) - 1); }
template <int HASH>
__device__ __forceinline__ uint64_t sortWordKey(const uint64_t word, const uint32_t matrix) {
    constexpr int low = kCollapseLargestBits - HASH;
    return (static_cast<uint64_t>(matrix) << kCollapseMatrixShift) | ((word >> (rpvg_sort::kRowBits + low)) << low) | (word & ((1ull << low) - 1));
}
template <int HASH>
__device__ __forceinline__ bool sortWordsSameSortedPart(const uint64_t x, const uint64_t y) {
    constexpr int shift = rpvg_sort::kRowBits + kCollapseLargestBits - HASH;
    return HASH ? (x >> shift) == (y >> shift) : ((x >> shift) == (y >> shift) && ((x ^ y) & ((1ull << (kCollapseLargestBits - HASH)) - 1)) == 0);
}

// a column's share of the hash of a row's cells (summed: the entries of a row come in no particular order; an empty cell adds nothing)
__device__ __forceinline__ uint64_t cellHashTerm(const uint32_t column, const double value) {
    const uint64_t cell = static_cast<uint64_t>(cellOf(value));
    uint64_t x = (cell + 0x632BE59BD9B4E019ull * (column + 1)) * 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    return cell ? x * 0xC2B2AE3D27D4EB4Full : 0;
}

// the key of row i of matrix m: group matrices carry it (written by the build kernels), the rows of an EM problem get it here
// (projection of the normalised row, its largest value, a hash of its cells) together with their zero pattern
__device__ __forceinline__ uint64_t sortKeyOfRow(const MatrixArrays & g, const uint32_t m, const uint64_t r0, const uint32_t i, const uint64_t * key_in,
                                                 uint64_t * pattern_out) {
    (void) g; (void) m; (void) pattern_out;
    return key_in[r0 + i];
}
struct CsrRowKey {  // of row i of EM problem p: the one place that computes it (the segment sort, and csrCollapseKeysKernel of the library route)
    uint64_t key, pattern;
};
__device__ __forceinline__ CsrRowKey csrRowKey(const CsrView & mv, const uint32_t p, const uint32_t i) {
    const double noise = mv.noise[i];
    double projection = collapseWeight(mv.G) * noise, largest = 0.0;
    uint64_t cells = cellHashTerm(mv.G, noise), pattern = 0;
    for (uint32_t e = mv.off[i]; e < mv.off[i + 1]; ++e) {
        const uint32_t c = mv.col[e];
        const double v = mv.val[e];
        projection = fma(collapseWeight(c), v, projection);
        largest = fmax(largest, v);
        cells += cellHashTerm(c, v);
        if (c < 64 && v != 0.0) pattern |= 1ull << c;
    }
    // the top of the low field: a hash of the row's cells, sorted on (rows of equal cells end up next to each other)
    constexpr int low_bits = kCollapseLargestBits - kCsrCellHashBits;
    uint64_t k = collapseSortKey(p, projection, largest);
    k = (k & ~((1ull << kCollapseLargestBits) - 1)) | (((cells * 0x9E3779B97F4A7C15ull) >> (64 - kCsrCellHashBits)) << low_bits) | (k & ((1ull << low_bits) - 1));
    return CsrRowKey{k, pattern};
}
__device__ __forceinline__ uint64_t sortKeyOfRow(const CsrArrays & g, const uint32_t p, const uint64_t r0, const uint32_t i, const uint64_t * key_in,
                                                 uint64_t * pattern_out) {
    (void) key_in;
    const CsrRowKey row = csrRowKey(g.view(p), p, i);
    pattern_out[r0 + i] = row.pattern;
    return row.key;
}

// caller-supplied words instead of rows (rpvg_hip_segment_sort_words: the sort alone, for its test)
struct WordArrays {
    const uint64_t * words;
    const uint64_t * segment_off;
    uint64_t * out;
    __device__ __forceinline__ uint64_t rowOffset(const uint32_t s) const { return segment_off[s]; }
    __device__ __forceinline__ uint64_t numRows(const uint32_t s) const { return segment_off[s + 1] - segment_off[s]; }
};

template <typename Arrays>
struct SegmentSortArgs {
    Arrays g;
    uint32_t num_matrices;               // group matrices: their number; EM problems: the bound of their number
    const uint32_t * num_matrices_dev;   // EM problems on a device-built list: their number
    // EM problems: the work items of the fill (em_sparse.hip: segment_rows row slots of a problem) — collapseUnusedSlotsKernel
    uint32_t num_items_bound;
    const uint32_t * num_items_dev;
    const uint64_t * seg_first;
    const uint32_t * item_problem;
    uint32_t segment_rows;
    uint64_t total_rows;
    const uint64_t * key_in;             // group matrices: the keys of the build
    uint64_t * pattern_out;              // EM problems: zero pattern of every row slot
    uint64_t * sort_key;                 // sorted (matrix, key, largest value), by position
    uint32_t * sort_row;
    uint32_t * position_of;              // by row: its sorted position
    uint8_t * same_prev;
    uint32_t * stretch_start;
    uint64_t * words_a, * words_b;       // [total rows] each: buffers 0 and 1 of the merge rounds (segment_sort_plan.hpp); the chunk sort writes words_a
    uint32_t * chunks;                   // [2 x capacity] (matrix, chunk of rpvg_sort::kChunkRows rows) of the matrices beyond rpvg_sort::kSmallSortRows rows
    uint32_t * chunk_count;
    uint32_t chunk_capacity;
    uint32_t round;                      // of the merge
};

// the word row i of matrix m is sorted as
template <typename Arrays>
__device__ __forceinline__ uint64_t sortWordOfRow(const SegmentSortArgs<Arrays> & a, const uint32_t m, const uint64_t r0, const uint32_t i) {
    return packSortWord<Arrays::kHashBits>(sortKeyOfRow(a.g, m, r0, i, a.key_in, a.pattern_out), i);
}
__device__ __forceinline__ uint64_t sortWordOfRow(const SegmentSortArgs<WordArrays> & a, const uint32_t, const uint64_t r0, const uint32_t i) { return a.g.words[r0 + i]; }

template <typename Arrays>
__device__ __forceinline__ void writeSortedPosition(const SegmentSortArgs<Arrays> & a, const uint32_t m, const uint64_t r0, const uint64_t position, const uint64_t word,
                                                    const uint64_t word_before, const bool has_before) {
    constexpr int HASH = Arrays::kHashBits;
    const uint32_t row = sortWordRow<HASH>(word);
    uint8_t same = 0;
    if (has_before && sortWordsSameSortedPart<HASH>(word, word_before)) {
        const typename Arrays::View mv = viewOf(m, a.g);
        const uint32_t before = sortWordRow<HASH>(word_before);
        same = (HASH ? rowsSameCells(mv, row, before) : rowsIdentical(mv, row, before)) ? 1 : 0;
    }
    a.sort_key[position] = sortWordKey<HASH>(word, m);
    a.sort_row[position] = static_cast<uint32_t>(r0 + row);
    a.position_of[r0 + row] = static_cast<uint32_t>(position);
    a.same_prev[position] = same;
    a.stretch_start[position] = same ? 0u : static_cast<uint32_t>(position);
}
__device__ __forceinline__ void writeSortedPosition(const SegmentSortArgs<WordArrays> & a, const uint32_t, const uint64_t, const uint64_t position, const uint64_t word,
                                                    const uint64_t, const bool) {
    a.g.out[position] = word;
}

// ---- the network in registers --------------------------------------------------------------------------------------------------
// The word of lane ^ D.  D = 1, 2: DPP quad_perm (a modifier of a VALU move, nothing leaves the SIMD); D = 4, 8: ds_swizzle in
// bit mode (the LDS crossbar without an address register or memory: the instruction set has no DPP pattern that is an XOR by 4
// or 8).  D = 16, 32 take v_permlane16_swap / v_permlane32_swap in exchangeStage below.
template <uint32_t D>
__device__ __forceinline__ uint64_t wordOfLaneXor(const uint64_t x) {
    static_assert(D == 1 || D == 2 || D == 4 || D == 8, "lane distance");
    const int lo = static_cast<int>(static_cast<uint32_t>(x)), hi = static_cast<int>(static_cast<uint32_t>(x >> 32));
    int other_lo, other_hi;
    if constexpr (D == 1) {
        other_lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
        other_hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
    } else if constexpr (D == 2) {
        other_lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
        other_hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true);
    } else {
        constexpr int pattern = static_cast<int>((D << 10) | 0x1F);            // bit mode: and 0x1f, or 0, xor D
        other_lo = __builtin_amdgcn_ds_swizzle(lo, pattern);
        other_hi = __builtin_amdgcn_ds_swizzle(hi, pattern);
    }
    return (static_cast<uint64_t>(static_cast<uint32_t>(other_hi)) << 32) | static_cast<uint32_t>(other_lo);
}

// a stage between the lanes l and l ^ D of a wavefront: every word of the lane meets the same word of the other lane
template <int E, uint32_t D>
__device__ __forceinline__ void exchangeStage(uint64_t (&v)[E], const bool keep_smaller) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if constexpr (D == 16 || D == 32) {
            // Both operands are the lane's word: the swap (odd rows of 16 of the first <-> even rows of the second; upper half of
            // the first <-> lower half of the second) leaves, in BOTH lanes of a pair, the lower lane's word in the first and
            // the upper lane's in the second result.
            const uint32_t lo = static_cast<uint32_t>(v[e]), hi = static_cast<uint32_t>(v[e] >> 32);
            const auto l = D == 16 ? __builtin_amdgcn_permlane16_swap(lo, lo, false, false) : __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
            const auto h = D == 16 ? __builtin_amdgcn_permlane16_swap(hi, hi, false, false) : __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
            const uint64_t lower = (static_cast<uint64_t>(h[0]) << 32) | l[0], upper = (static_cast<uint64_t>(h[1]) << 32) | l[1];
            v[e] = ((lower < upper) == keep_smaller) ? lower : upper;
        } else {
            const uint64_t other = wordOfLaneXor<D>(v[e]);
            v[e] = ((other < v[e]) == keep_smaller) ? other : v[e];
        }
    }
}

// a stage across the wavefronts of the workgroup: thread t meets thread t ^ distance through LDS (word e of everybody side by
// side: no bank conflicts), two barriers
template <int E, int WAVES>
__device__ __forceinline__ void exchangeThroughLds(uint64_t (&v)[E], uint64_t * lds, const uint32_t t, const uint32_t distance, const bool keep_smaller) {
    constexpr uint32_t T = rpvg_sort::kWaveLanes * WAVES;
#pragma unroll
    for (int e = 0; e < E; ++e) lds[e * T + t] = v[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint64_t other = lds[e * T + (t ^ distance)];
        v[e] = ((other < v[e]) == keep_smaller) ? other : v[e];
    }
    __syncthreads();
}

// a stage inside the lane: words e and e | j
template <int E>
__device__ __forceinline__ void inLaneStage(uint64_t (&v)[E], const uint32_t t, const uint32_t k, const uint32_t j) {
#pragma unroll
    for (uint32_t e = 0; e < static_cast<uint32_t>(E); ++e) {
        if (e & j) continue;
        const bool ascending = rpvg_sort::ascendingAt(t * E + e, k);
        const uint64_t x = v[e], y = v[e | j];
        const bool swap = (x > y) == ascending;
        v[e] = swap ? y : x;
        v[e | j] = swap ? x : y;
    }
}

// ... all of them in one direction (k beyond the lane's words)
template <int E>
__device__ __forceinline__ void inLaneStageDirected(uint64_t (&v)[E], const bool ascending, const uint32_t j) {
#pragma unroll
    for (uint32_t e = 0; e < static_cast<uint32_t>(E); ++e) {
        if (e & j) continue;
        const uint64_t x = v[e], y = v[e | j];
        const bool swap = (x > y) == ascending;
        v[e] = swap ? y : x;
        v[e | j] = swap ? x : y;
    }
}

// Thread t of a group of WAVES wavefronts holds the elements t E .. t E + E - 1 of a bitonic network over 64 WAVES E words
// (segment_sort_plan.hpp); afterwards they ascend with the element index.  WAVES > 1: the group is the whole workgroup, `lds`
// holds 64 WAVES E words nobody else uses, and every thread of the workgroup calls.  The stages between lanes are a loop with
// one body per lane distance, not the unrolled network: thirteen instantiations of up to 66 stages each would not fit the
// instruction cache side by side.
template <int E, int WAVES>
__device__ __forceinline__ void sortWordsInRegisters(uint64_t (&v)[E], uint64_t * lds, const uint32_t t) {
    constexpr uint32_t N = rpvg_sort::kWaveLanes * WAVES * E;
    (void) lds;
#pragma unroll
    for (uint32_t k = 2; k <= static_cast<uint32_t>(E); k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) inLaneStage<E>(v, t, k, j);
    }
#pragma unroll 1
    for (uint32_t k = 2 * E; k <= N; k <<= 1) {
        const bool ascending = rpvg_sort::ascendingAt(t * E, k);  // (k > E: the same for every word of the lane)
#pragma unroll 1
        for (uint32_t j = k >> 1; j >= static_cast<uint32_t>(E); j >>= 1) {
            const uint32_t distance = rpvg_sort::laneDistance(j, E);
            const bool keep_smaller = ((t & distance) == 0) == ascending;  // rpvg_sort::keepsSmaller(t E + e, k, j)
            if (rpvg_sort::stageKind(j, E) == rpvg_sort::kAcrossWaves) {
                if constexpr (WAVES > 1) exchangeThroughLds<E, WAVES>(v, lds, t, distance, keep_smaller);
            } else {
                switch (distance) {
                    case 1: exchangeStage<E, 1>(v, keep_smaller); break;
                    case 2: exchangeStage<E, 2>(v, keep_smaller); break;
                    case 4: exchangeStage<E, 4>(v, keep_smaller); break;
                    case 8: exchangeStage<E, 8>(v, keep_smaller); break;
                    case 16: exchangeStage<E, 16>(v, keep_smaller); break;
                    default: exchangeStage<E, 32>(v, keep_smaller); break;
                }
            }
        }
#pragma unroll
        for (uint32_t j = static_cast<uint32_t>(E) >> 1; j > 0; j >>= 1) inLaneStageDirected<E>(v, ascending, j);
    }
}

// what one wavefront wrote to LDS is seen by its other lanes (the LDS runs a wavefront's accesses in order: nothing to wait for,
// the compiler must only keep the order); WAVES > 1: a workgroup barrier
template <int WAVES>
__device__ __forceinline__ void sortGroupSync() {
    if constexpr (WAVES > 1) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// The rows [c0, c0 + n) of matrix m, n <= 64 WAVES E, sorted by the calling group of WAVES wavefronts (thread t of it) into
// image[0 .. n).  A thread loads the rows t, t + 64 WAVES .. (coalesced; for the EM problems their keys are computed here, by
// the lane that owns the word) — which word starts in which element of the network does not matter to a sort — pads with
// ~0, runs the network and writes its E consecutive words of the result to the image, from which the caller's threads read
// them side by side together with their predecessors.  WAVES > 1: the whole workgroup calls, behind a barrier that
// separates it from the image's last readers.
template <typename Arrays, int E, int WAVES>
__device__ __forceinline__ void sortSegmentWords(const SegmentSortArgs<Arrays> & a, const uint32_t m, const uint64_t r0, const uint64_t c0, const uint32_t n,
                                                 uint64_t * image, const uint32_t t) {
    constexpr uint32_t T = rpvg_sort::kWaveLanes * WAVES;
    uint64_t v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = e * T + t;
        v[e] = i < n ? sortWordOfRow(a, m, r0, static_cast<uint32_t>(c0 + i)) : rpvg_sort::kPaddingWord;
    }
    sortWordsInRegisters<E, WAVES>(v, image, t);
#pragma unroll
    for (int e = 0; e < E; ++e) image[t * E + e] = v[e];
    sortGroupSync<WAVES>();
}

// ... with the size class chosen by n (uniform in the group)
template <typename Arrays, int WAVES>
__device__ __forceinline__ void sortSegmentOfGroup(const SegmentSortArgs<Arrays> & a, const uint32_t m, const uint64_t r0, const uint64_t c0, const uint32_t n,
                                                   uint64_t * image, const uint32_t t) {
    switch (rpvg_sort::classOfGroup(n, WAVES).words_per_lane) {
        case 1: sortSegmentWords<Arrays, 1, WAVES>(a, m, r0, c0, n, image, t); break;
        case 2: sortSegmentWords<Arrays, 2, WAVES>(a, m, r0, c0, n, image, t); break;
        case 4: sortSegmentWords<Arrays, 4, WAVES>(a, m, r0, c0, n, image, t); break;
        default: sortSegmentWords<Arrays, 8, WAVES>(a, m, r0, c0, n, image, t); break;
    }
}

// Matrices of up to rpvg_sort::kSmallSortRows rows — nearly all of a batch.  A workgroup of two wavefronts draws two matrices at a time
// with a grid-stride loop: a matrix of up to 512 rows is sorted by ONE wavefront in its half of the 8 KB of LDS, without a
// workgroup barrier, next to the other wavefront's; a matrix of 513 .. 1 024 rows then takes both.  Sixteen workgroups per CU.
// A larger matrix lists its chunks for the kernel below.  (amdgpu_waves_per_eu(4): left alone the compiler takes 138 VGPRs for
// the EM problems' instantiation, three wavefronts per SIMD — fewer than a launch of 3 800 problems puts on 1 024 SIMDs; 128 cost
// it no spill.  A floor of five spills.)
template <typename Arrays>
__global__ __launch_bounds__(kSmallSortThreads) __attribute__((amdgpu_waves_per_eu(4))) void collapseSmallSortKernel(const SegmentSortArgs<Arrays> a) {
    __shared__ uint64_t words[rpvg_sort::kSmallSortRows];
    const uint32_t M = a.num_matrices_dev ? min(*a.num_matrices_dev, a.num_matrices) : a.num_matrices;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / rpvg_sort::kWaveLanes), lane = threadIdx.x % rpvg_sort::kWaveLanes;
    for (uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * rpvg_sort::kSmallSortWaves; m0 < M; m0 += static_cast<uint64_t>(gridDim.x) * rpvg_sort::kSmallSortWaves) {
        if (m0 + wave < M) {  // this wavefront's matrix
            const uint32_t m = static_cast<uint32_t>(m0 + wave);
            const uint64_t R = a.g.numRows(m);
            if (R > rpvg_sort::kSmallSortRows) {
                if (lane == 0) {
                    const uint32_t chunks = static_cast<uint32_t>((R + rpvg_sort::kChunkRows - 1) / rpvg_sort::kChunkRows);
                    const uint32_t first = atomicAdd(a.chunk_count, chunks);
                    for (uint32_t c = 0; c < chunks && first + c < a.chunk_capacity; ++c) {
                        a.chunks[2 * static_cast<uint64_t>(first + c)] = m;
                        a.chunks[2 * static_cast<uint64_t>(first + c) + 1] = c;
                    }
                }
            } else if (R > 0 && R <= rpvg_sort::kOneWaveRows) {
                const uint64_t r0 = a.g.rowOffset(m);
                const uint32_t n = static_cast<uint32_t>(R);
                uint64_t * image = words + wave * rpvg_sort::kOneWaveRows;
                sortSegmentOfGroup<Arrays, 1>(a, m, r0, 0, n, image, lane);
                for (uint32_t i = lane; i < n; i += rpvg_sort::kWaveLanes) writeSortedPosition(a, m, r0, r0 + i, image[i], i ? image[i - 1] : 0ull, i != 0);
                sortGroupSync<1>();  // (the image is read before the wavefront's next matrix overwrites it)
            }
        }
        for (uint32_t w = 0; w < rpvg_sort::kSmallSortWaves && m0 + w < M; ++w) {  // the pair's matrices of both wavefronts (uniform)
            const uint32_t m = static_cast<uint32_t>(m0 + w);
            const uint64_t R = a.g.numRows(m);
            if (R <= rpvg_sort::kOneWaveRows || R > rpvg_sort::kSmallSortRows) continue;
            const uint64_t r0 = a.g.rowOffset(m);
            const uint32_t n = static_cast<uint32_t>(R);
            __syncthreads();  // (the halves are free)
            sortSegmentWords<Arrays, rpvg_sort::kMaxWordsPerLane, rpvg_sort::kSmallSortWaves>(a, m, r0, 0, n, words, threadIdx.x);
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) writeSortedPosition(a, m, r0, r0 + i, words[i], i ? words[i - 1] : 0ull, i != 0);
            __syncthreads();
        }
    }
}

// the chunks of the larger matrices: sorted runs of rpvg_sort::kChunkRows words in words_a (four wavefronts, eight words per lane; a
// matrix's short last chunk takes fewer words per lane)
template <typename Arrays>
__global__ __launch_bounds__(kChunkSortThreads) void collapseChunkSortKernel(const SegmentSortArgs<Arrays> a) {
    __shared__ uint64_t words[rpvg_sort::kChunkRows];
    const uint32_t count = min(*a.chunk_count, a.chunk_capacity);
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t m = a.chunks[2 * static_cast<uint64_t>(item)], chunk = a.chunks[2 * static_cast<uint64_t>(item) + 1];
        const uint64_t R = a.g.numRows(m), r0 = a.g.rowOffset(m);
        const uint64_t c0 = static_cast<uint64_t>(chunk) * rpvg_sort::kChunkRows;
        const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(rpvg_sort::kChunkRows), R - c0));
        __syncthreads();  // (the chunk before is done with the LDS)
        sortSegmentOfGroup<Arrays, rpvg_sort::kChunkWaves>(a, m, r0, c0, n, words, threadIdx.x);
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) a.words_a[r0 + c0 + i] = words[i];
    }
}

// One round of the merge: the sorted runs of length rpvg_sort::kChunkRows << round of every larger matrix, two by two.  Work item =
// kMergeTile output words of a matrix (two per chunk of the list); a thread finds where its eight outputs begin in the two
// runs by a binary search along its diagonal (merge path; the words are distinct: they carry the row) and merges them out.
// The host launches the rounds the largest matrix it allows would need; a matrix whose runs are complete (round >=
// mergeRoundsOf(rows)) touches no memory any more — its words stay in the buffer of its own last round, where
// collapseMergedPositionsKernel looks for them — and while it has rounds in front of it, a last run without a partner is
// copied (nB == 0 below), so that the runs of the next round all lie in one buffer.  (Leaving that run where it is and
// reading it from the buffer of ITS last round would make a round merge in place: three chunks — the third waits in
// buffer 0, which round 1 writes.)
template <typename Arrays>
__global__ __launch_bounds__(kMergeThreads) void collapseMergeRoundKernel(const SegmentSortArgs<Arrays> a) {
    constexpr uint32_t kPerThread = kMergeTile / kMergeThreads;
    constexpr uint32_t kTilesPerChunk = rpvg_sort::kChunkRows / kMergeTile;
    const uint32_t count = min(*a.chunk_count, a.chunk_capacity) * kTilesPerChunk;
    const uint64_t * __restrict__ source = rpvg_sort::sourceBuffer(a.round) ? a.words_b : a.words_a;
    uint64_t * __restrict__ target = rpvg_sort::targetBuffer(a.round) ? a.words_b : a.words_a;
    const uint64_t run = rpvg_sort::runLength(a.round);
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t m = a.chunks[2 * static_cast<uint64_t>(item / kTilesPerChunk)];
        const uint64_t R = a.g.numRows(m);
        if (!rpvg_sort::roundHasWork(R, a.round)) continue;
        const uint64_t r0 = a.g.rowOffset(m);
        const uint64_t out0 = static_cast<uint64_t>(a.chunks[2 * static_cast<uint64_t>(item / kTilesPerChunk) + 1]) * rpvg_sort::kChunkRows + (item % kTilesPerChunk) * kMergeTile;
        if (out0 >= R) continue;
        const uint64_t pair0 = out0 / (2 * run) * (2 * run);
        const uint64_t a1 = min(R, pair0 + run), b1 = min(R, pair0 + 2 * run);
        const uint64_t * A = source + r0 + pair0, * B = source + r0 + a1;
        const uint64_t nA = a1 - pair0, nB = b1 - a1;
        const uint64_t d = (out0 - pair0) + static_cast<uint64_t>(threadIdx.x) * kPerThread;  // this thread's diagonal
        if (d >= nA + nB) continue;
        // i = words of A among the first d of the merged sequence: the smallest i with A[i] > B[d - i - 1]
        uint64_t lo = d > nB ? d - nB : 0, hi = min(d, nA);
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (A[mid] < B[d - mid - 1]) lo = mid + 1;
            else hi = mid;
        }
        uint64_t i = lo, j = d - lo;
        uint64_t * out = target + r0 + pair0 + d;
        const uint32_t outputs = static_cast<uint32_t>(min(static_cast<uint64_t>(kPerThread), nA + nB - d));
        uint64_t x = i < nA ? A[i] : ~0ull, y = j < nB ? B[j] : ~0ull;
        for (uint32_t k = 0; k < outputs; ++k) {
            if (x < y) {
                out[k] = x;
                ++i;
                x = i < nA ? A[i] : ~0ull;
            } else {
                out[k] = y;
                ++j;
                y = j < nB ? B[j] : ~0ull;
            }
        }
    }
}

// the larger matrices' rows at their sorted positions (what the small kernel writes itself), each matrix read from the buffer in
// which its own last round left it
template <typename Arrays>
__global__ __launch_bounds__(256) void collapseMergedPositionsKernel(const SegmentSortArgs<Arrays> a) {
    const uint32_t count = min(*a.chunk_count, a.chunk_capacity);
    for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
        const uint32_t m = a.chunks[2 * static_cast<uint64_t>(item)], chunk = a.chunks[2 * static_cast<uint64_t>(item) + 1];
        const uint64_t R = a.g.numRows(m), r0 = a.g.rowOffset(m);
        const uint64_t * __restrict__ sorted = rpvg_sort::finalBuffer(R) ? a.words_b : a.words_a;
        const uint64_t c0 = static_cast<uint64_t>(chunk) * rpvg_sort::kChunkRows;
        const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(rpvg_sort::kChunkRows), R - c0));
        for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) {
            const uint64_t i = c0 + e;
            writeSortedPosition(a, m, r0, r0 + i, sorted[r0 + i], i ? sorted[r0 + i - 1] : 0ull, i != 0);
        }
    }
}

// EM problems: the row slots no problem's rows fill (the storage is laid out by a bound) get keys that sort behind every row
// and are close to nothing.  A workgroup per work item of the fill (em_sparse.hip: segment_rows slots of a problem): the
// unused slots of its own range, the last item of a problem up to the next problem's first slot; everybody shares the
// slots behind the last problem's items.
template <typename Arrays>
__global__ __launch_bounds__(256) void collapseUnusedSlotsKernel(const SegmentSortArgs<Arrays> a) {
    const uint32_t M = a.num_matrices_dev ? min(*a.num_matrices_dev, a.num_matrices) : a.num_matrices;
    const uint32_t items = a.num_items_dev ? min(*a.num_items_dev, a.num_items_bound) : a.num_items_bound;
    const uint64_t unused = collapseSortKey(a.num_matrices, 0.0, 0.0);
    auto fill = [&](const uint64_t r) {
        a.sort_key[r] = unused;
        a.sort_row[r] = static_cast<uint32_t>(r);
        a.position_of[r] = static_cast<uint32_t>(r);
        a.same_prev[r] = 0;
        a.stretch_start[r] = static_cast<uint32_t>(r);
        a.pattern_out[r] = 0;
    };
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t m = a.item_problem[item];
        if (m >= M) continue;
        const uint64_t s = item - a.seg_first[m];
        const bool last = item + 1 == a.seg_first[m + 1];
        const uint64_t r0 = a.g.rowOffset(m), R = a.g.numRows(m);
        const uint64_t lo = max(R, s * a.segment_rows);
        const uint64_t own = static_cast<uint64_t>(a.seg_first[m + 1] - a.seg_first[m]) * a.segment_rows;
        const uint64_t bound = min((m + 1 < M) ? a.g.rowOffset(m + 1) - r0 : own, a.total_rows - r0);
        const uint64_t hi = last ? bound : min(bound, (s + 1) * a.segment_rows);
        for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) fill(r0 + i);
    }
    const uint64_t tail = M == 0 ? 0 : min(a.total_rows, a.g.rowOffset(M - 1) + static_cast<uint64_t>(a.seg_first[M] - a.seg_first[M - 1]) * a.segment_rows);
    for (uint64_t r = tail + blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; r < a.total_rows; r += static_cast<uint64_t>(gridDim.x) * blockDim.x) fill(r);
}

// ---- the host side: a plan (collapse_plan.hpp) and the stages over it --------------------------------------------------------------
struct CollapseTemporaries {
    DeviceBuffer<uint32_t> rewritten_count;
    DeviceBuffer<uint64_t> key_out, pair_pattern;
    DeviceBuffer<uint32_t> row_out, order, head, pair_column, marked_list, pairs, between_items, row_items, list_index;
    DeviceBuffer<uint32_t> stretch;  // stretch starts by position, their running maximum, stretch ends, positions by row: total_rows each
    DeviceBuffer<uint64_t> pair_base;
    DeviceBuffer<uint8_t> pair_table;
    DeviceBuffer<double> pair_bound;
    DeviceBuffer<uint8_t> bytes;  // same_prev, close, barrier: total_rows each
    DeviceBuffer<unsigned char> sort_tmp;
    // EM problems only
    DeviceBuffer<uint64_t> csr_key, csr_pattern;
    DeviceBuffer<uint32_t> csr_row, csr_segments;
    // the hand-written segment sort (stage 0)
    DeviceBuffer<uint64_t> words_a, words_b;
    DeviceBuffer<uint32_t> chunks, chunk_count;
    // the slices of `stretch` and `bytes`
    uint32_t * stretchStart(const uint64_t) const { return stretch.ptr; }
    uint32_t * stretchFirst(const uint64_t T) const { return stretch.ptr + T; }
    uint32_t * stretchEnd(const uint64_t T) const { return stretch.ptr + 2 * T; }
    uint32_t * positionOf(const uint64_t T) const { return stretch.ptr + 3 * T; }
    uint8_t * samePrev() const { return bytes.ptr; }
    uint8_t * close(const uint64_t T) const { return bytes.ptr + T; }
    uint8_t * barrier(const uint64_t T) const { return bytes.ptr + 2 * T; }
};

// What is the caller's own.  Group matrices: the keys the build wrote, the outputs for the search, and where the held-back part
// of the runs goes (null: the runs are not held back).
struct MatrixCaller {
    const uint64_t * key;
    const uint32_t * row;
    double * rowmax;
    uint32_t * mat_fast, * mat_mid;
    std::function<hipError_t(hipStream_t, const SearchParts *)> * held_back_runs;
};
// EM problems: the work items of the fill
struct ProblemCaller {
    const CsrCollapseInput & in;
};

hipError_t queueStretchScan(const CollapseTemporaries & t, const uint64_t total_rows, void * scratch, size_t & bytes, hipStream_t st) {
    return hipcub::DeviceScan::InclusiveScan(scratch, bytes, t.stretchStart(total_rows), t.stretchFirst(total_rows), hipcub::Max(), static_cast<int>(total_rows), st);
}

// The keys carry the matrix above the projection and the rows of a matrix are contiguous: ONE (stable) radix sort of the whole array
// on the projection and as many matrix bits as there are matrices orders every matrix's rows by their projection.  (Round 2 sorted
// segment by segment, hipcub::DeviceSegmentedRadixSort: 0.33 ms per 1.6 M rows in 2 500 segments, the longest kernel of the
// collapse, and no better on the group matrices since.)
hipError_t queueLibrarySort(const MatrixCaller & caller, const CollapsePlan & plan, const CollapseTemporaries & t, void * scratch, size_t & bytes, hipStream_t st) {
    return hipcub::DeviceRadixSort::SortPairs(scratch, bytes, caller.key, t.key_out.ptr, caller.row, t.row_out.ptr, static_cast<int>(plan.total_rows),
                                              plan.begin_bit, plan.end_bit, st);
}
// The rows of a problem are sorted as a segment, behind csrCollapseKeysKernel: a handful of launches against the global sort's seven
// passes of three launches each (same box, configs[2] batch: 12.0-12.5 ms per step against 14.6).
// (hipcub's segmented sort partitions the segments by size and reads the partition sizes back — the lane's thread waits there for
// the fill; rocprim's unpartitioned configuration, one kernel and no wait, was 1 ms slower per lane all the same)
hipError_t queueLibrarySort(const ProblemCaller &, const CollapsePlan & plan, const CollapseTemporaries & t, void * scratch, size_t & bytes, hipStream_t st) {
    const uint32_t * segment_begin = t.csr_segments.ptr, * segment_end = segment_begin + plan.M;
    return hipcub::DeviceSegmentedRadixSort::SortPairs(scratch, bytes, t.csr_key.ptr, t.key_out.ptr, t.csr_row.ptr, t.row_out.ptr, static_cast<int>(plan.total_rows),
                                                       static_cast<int>(plan.M), segment_begin, segment_end, plan.begin_bit, plan.end_bit, st);
}

// every buffer of the plan's counts, and the library's scratch for the scan and (library routes) the sort
template <typename Caller>
hipError_t allocateCollapse(const CollapsePlan & plan, const Caller & caller, CollapseTemporaries & t, DeviceBuffer<uint32_t> & info, hipStream_t st) {
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    const BufferCounts & c = plan.counts;
    ok(info.alloc(plan.info.total_words));
    ok(t.key_out.alloc(c.sorted_key));
    ok(t.row_out.alloc(c.sorted_row));
    ok(t.order.alloc(c.order));
    ok(t.head.alloc(c.head));
    ok(t.pair_column.alloc(c.pair_column));
    ok(t.pair_bound.alloc(c.pair_bound));
    ok(t.pair_pattern.alloc(c.pair_pattern));
    ok(t.marked_list.alloc(c.marked_list));
    ok(t.pairs.alloc(c.pairs));
    ok(t.between_items.alloc(c.between_items));
    ok(t.row_items.alloc(c.row_items));
    ok(t.list_index.alloc(c.list_index));
    ok(t.pair_base.alloc(c.pair_base));
    ok(t.pair_table.alloc(c.pair_table));
    ok(t.bytes.alloc(c.bytes));
    ok(t.stretch.alloc(c.stretch));
    ok(t.words_a.alloc(c.words));
    ok(t.words_b.alloc(c.words));
    ok(t.chunks.alloc(c.chunks));
    ok(t.chunk_count.alloc(c.chunk_count));
    ok(t.csr_pattern.alloc(c.pattern));
    ok(t.csr_key.alloc(c.keys));
    ok(t.csr_row.alloc(c.rows));
    ok(t.csr_segments.alloc(c.segments));
    size_t sort_bytes = 0, scan_bytes = 0;
    if (e == hipSuccess && plan.route != HandSort) ok(queueLibrarySort(caller, plan, t, nullptr, sort_bytes, st));
    if (e == hipSuccess) ok(queueStretchScan(t, plan.total_rows, nullptr, scan_bytes, st));
    ok(t.sort_tmp.alloc(std::max(sort_bytes, scan_bytes)));
    return e;
}

template <typename Arrays>
void launchSegmentSort(SegmentSortArgs<Arrays> c, const SegmentSortPlan & s, hipStream_t st) {
    collapseSmallSortKernel<Arrays><<<dim3(s.small_sort.grid), dim3(s.small_sort.block), 0, st>>>(c);
    if (s.chunk_sort.grid == 0) return;
    collapseChunkSortKernel<Arrays><<<dim3(s.chunk_sort.grid), dim3(s.chunk_sort.block), 0, st>>>(c);
    for (uint32_t round = 0; round < s.merge_rounds; ++round) {
        c.round = round;
        collapseMergeRoundKernel<Arrays><<<dim3(s.merge_round.grid), dim3(s.merge_round.block), 0, st>>>(c);
    }
    collapseMergedPositionsKernel<Arrays><<<dim3(s.merged_positions.grid), dim3(s.merged_positions.block), 0, st>>>(c);
}

// ---- the argument structs, each from (view, plan, temporaries) ---------------------------------------------------------------------
template <typename Arrays>
SegmentSortArgs<Arrays> segmentSortArgs(const Arrays & arrays, const CollapsePlan & plan, const CollapseTemporaries & t) {
    const uint64_t T = plan.total_rows;
    SegmentSortArgs<Arrays> c{};
    c.g = arrays;
    c.num_matrices = plan.M;
    c.total_rows = T;
    c.sort_key = t.key_out.ptr;
    c.sort_row = t.row_out.ptr;
    c.position_of = t.positionOf(T);
    c.same_prev = t.samePrev();
    c.stretch_start = t.stretchStart(T);
    c.words_a = t.words_a.ptr;
    c.words_b = t.words_b.ptr;
    c.chunks = t.chunks.ptr;
    c.chunk_count = t.chunk_count.ptr;
    c.chunk_capacity = plan.segment_sort.chunk_capacity;
    return c;
}
// ... and where the rows' keys come from: the build's, or computed by the sort over the work items of the fill
void setKeySource(SegmentSortArgs<MatrixArrays> & c, const MatrixCaller & caller, const CollapseTemporaries &) { c.key_in = caller.key; }
void setKeySource(SegmentSortArgs<CsrArrays> & c, const ProblemCaller & caller, const CollapseTemporaries & t) {
    c.num_matrices_dev = caller.in.num_problems_dev;
    c.num_items_bound = caller.in.num_items_bound;
    c.num_items_dev = caller.in.num_items_dev;
    c.seg_first = caller.in.seg_first;
    c.item_problem = caller.in.item_problem;
    c.segment_rows = caller.in.segment_rows;
    c.pattern_out = t.csr_pattern.ptr;
}

template <typename Arrays>
PairScanArgs<Arrays> pairScanArgs(const Arrays & arrays, const CollapsePlan & plan, const CollapseKnobs & knobs, const double precision, const CollapseTemporaries & t,
                                  uint32_t * info) {
    const InfoLayout & l = plan.info;
    const uint64_t T = plan.total_rows;
    PairScanArgs<Arrays> a;
    a.num_matrices = plan.M;
    a.total_rows = T;
    a.precision = precision;
    a.sort_key = t.key_out.ptr;
    a.sort_row = t.row_out.ptr;
    a.g = arrays;
    a.same_prev = t.samePrev();
    a.stretch_first = t.stretchStart(T);  // (the kernel in front of the scan writes the starts; behind it: stretchFirst)
    a.stretch_end = t.stretchEnd(T);
    a.position_of = t.positionOf(T);
    a.marked_bits = info + l.marked_bits;
    a.marked_list = t.marked_list.ptr;
    a.marked_count = info + l.marked_count;
    a.pairs = t.pairs.ptr;
    a.pair_count = info + l.pair_counts;  // (the forward list; the around list: + 1)
    a.pair_capacity = plan.pair_capacity;
    a.active = reinterpret_cast<uint8_t *>(info + l.active);
    a.mat_flag = info + l.mat_flag;
    a.info = info + l.info;
    a.count_pairs = knobs.debug;
    return a;
}

// (no sums, nothing held back; the outputs for the search — rowmax, mat_fast, mat_mid — are the group matrices' own: setOutputs)
template <typename Arrays>
ReplayArgs<Arrays> replayArgs(const Arrays & arrays, const CollapsePlan & plan, const CollapseKnobs & knobs, const double precision, const CollapseTemporaries & t,
                              uint32_t * info) {
    const InfoLayout & l = plan.info;
    const uint64_t T = plan.total_rows;
    ReplayArgs<Arrays> r{};
    r.num_matrices = plan.M;
    r.precision = precision;
    r.g = arrays;
    r.mat_flag = info + l.mat_flag;
    r.active = reinterpret_cast<uint8_t *>(info + l.active);
    r.sort_row = t.row_out.ptr;
    r.position_of = t.positionOf(T);
    r.stretch_end = t.stretchEnd(T);
    r.mat_list = info + l.mat_list;
    r.replay_list = info + l.replay_list;
    r.between_items = t.between_items.ptr;
    r.between_count = info + l.between_count;
    r.row_items = t.row_items.ptr;
    r.row_item_count = info + l.row_item_count;
    r.pair_base = t.pair_base.ptr;
    r.pair_bytes = reinterpret_cast<unsigned long long *>(info + l.pair_bytes);
    r.pair_table = t.pair_table.ptr;
    r.list_index = t.list_index.ptr;
    r.order = t.order.ptr;
    r.head_of = t.head.ptr;
    r.close = t.close(T);
    r.barrier = t.barrier(T);
    r.pair_column = t.pair_column.ptr;
    r.pair_lo = t.pair_bound.ptr;
    r.pair_hi = t.pair_bound.ptr + T;
    r.pair_pattern = t.pair_pattern.ptr;
    r.info = info + l.info;
    r.debug = knobs.debug;
    r.no_lds_tables = knobs.no_lds_tables;
    return r;
}
void setOutputs(ReplayArgs<MatrixArrays> & r, const MatrixCaller & caller) {
    r.rowmax = caller.rowmax;
    r.mat_fast = caller.mat_fast;
    r.mat_mid = caller.mat_mid;
}
void setOutputs(ReplayArgs<CsrArrays> &, const ProblemCaller &) {}  // (the merged counts: CsrArrays)

// ---- the runs ------------------------------------------------------------------------------------------------------------------------
// What was held back behind a walk-only collapseRunsKernel, on the stream of whoever read the matrices: the search has read them as
// built (sums): its sums are adjusted, then the rows of the runs take their heads' values; nobody has (null): the rows only.
hipError_t launchHeldBackRuns(ReplayArgs<MatrixArrays> r, const SearchParts * sums, const Launch adjust_sums, const Launch rewrite, hipStream_t on) {
    if (sums) {
        r.sums = *sums;
        collapseAdjustSumsKernel<<<dim3(adjust_sums.grid), dim3(adjust_sums.block), 0, on>>>(r);
    }
    r.walk_only = false;
    collapseRewriteKernel<<<dim3(rewrite.grid), dim3(rewrite.block), 0, on>>>(r);
    return hipGetLastError();
}

hipError_t queueRuns(ReplayArgs<MatrixArrays> r, const CollapsePlan & plan, const MatrixCaller & caller, CollapseTemporaries & t, hipStream_t st) {
    if (caller.held_back_runs) {
        // The walk over the runs writes nothing a reader of the matrices sees (the heads of the list positions, the list of the
        // rows that will take their head's values): it runs here, on the collapse's stream, beside the search — one matrix of a
        // configs[2] batch walks for 0.8 ms, which stood behind the tile kernel on the search's stream (round 5) — and what is
        // held back is the adjustment of the search's sums and the rewrite of the rows.
        const hipError_t e = t.rewritten_count.alloc(plan.M);
        if (e != hipSuccess) return e;
        r.rewritten_count = t.rewritten_count.ptr;
        r.walk_only = true;
    }
    collapseRunsKernel<MatrixArrays><<<dim3(plan.runs.grid), dim3(plan.runs.block), 0, st>>>(r);
    if (caller.held_back_runs) {
        const Launch adjust_sums = plan.adjust_sums, rewrite = plan.rewrite;
        *caller.held_back_runs = [=](hipStream_t on, const SearchParts * sums) { return launchHeldBackRuns(r, sums, adjust_sums, rewrite, on); };
    }
    return hipSuccess;
}
hipError_t queueRuns(const ReplayArgs<CsrArrays> & r, const CollapsePlan & plan, const ProblemCaller &, CollapseTemporaries &, hipStream_t st) {
    collapseRunsKernel<CsrArrays><<<dim3(plan.runs.grid), dim3(plan.runs.block), 0, st>>>(r);
    return hipSuccess;
}

// sort key, slot and zero pattern of every row slot of the EM problems' storage: the slots of a problem's kept rows carry
// (problem, projection of the normalised row, its largest value); the others the index `num_problems`, which no problem
// has — they sort behind every row and are close to nothing
__global__ __launch_bounds__(256) void csrCollapseKeysKernel(const CsrArrays g, const uint32_t num_problems_bound, const uint32_t * __restrict__ num_problems_dev,
                                                           const uint32_t num_items_bound, const uint32_t * __restrict__ num_items_dev,
                                                           const uint64_t * __restrict__ seg_first, const uint32_t * __restrict__ item_problem,
                                                           const uint32_t segment_rows, const uint64_t total_rows, uint64_t * __restrict__ key,
                                                           uint32_t * __restrict__ row, uint64_t * __restrict__ pattern_out, uint32_t * __restrict__ segment_begin,
                                                           uint32_t * __restrict__ segment_end, uint64_t * __restrict__ sorted_key,
                                                           uint32_t * __restrict__ sorted_row) {
    // Work item = a problem's stretch of `segment_rows` row slots (the items of the fill, em_sparse.hip: a problem has at least
    // as many as its slots need); the last item of a problem also covers the unused slots up to the next problem's.
    // (segment_begin != NULL: the rows are sorted problem by problem, a segment each, and the unused slots — which no segment
    // covers — keep what is written here in the sorted arrays.)
    const uint32_t P = num_problems_dev ? *num_problems_dev : num_problems_bound;
    const uint32_t items = num_items_dev ? min(*num_items_dev, num_items_bound) : num_items_bound;
    const uint64_t unused = collapseSortKey(num_problems_bound, 0.0, 0.0);
    for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p = item_problem[item];
        if (p >= P) continue;
        const uint64_t s = item - seg_first[p];
        const bool last = item + 1 == seg_first[p + 1];
        const CsrView mv = g.view(p);
        const uint64_t r0 = g.rowOffset(p);
        const uint64_t slots = (p + 1 < P ? g.rowOffset(p + 1) : r0 + mv.R) - r0;
        if (s == 0 && threadIdx.x == 0 && segment_begin) {
            segment_begin[p] = static_cast<uint32_t>(r0);
            segment_end[p] = static_cast<uint32_t>(r0 + mv.R);
        }
        const uint64_t lo = s * segment_rows, hi = last ? slots : min(slots, (s + 1) * segment_rows);
        for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
            uint64_t k = unused, pattern = 0;
            if (i < mv.R) {
                const CsrRowKey own = csrRowKey(mv, p, static_cast<uint32_t>(i));
                k = own.key;
                pattern = own.pattern;
            }
            key[r0 + i] = k;
            row[r0 + i] = static_cast<uint32_t>(r0 + i);
            pattern_out[r0 + i] = pattern;
            if (segment_begin && i >= mv.R) {
                sorted_key[r0 + i] = unused;
                sorted_row[r0 + i] = static_cast<uint32_t>(r0 + i);
            }
        }
    }
    const uint64_t thread = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x, threads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    if (segment_begin) {  // the segments of the bound's problems that do not exist
        for (uint64_t p = P + thread; p < num_problems_bound; p += threads) segment_begin[p] = segment_end[p] = 0;
    }
    // the tail behind the last problem (everything, if there is no problem)
    const uint64_t from = P == 0 ? 0 : g.rowOffset(P - 1) + g.numRows(P - 1);
    for (uint64_t r = from + thread; r < total_rows; r += threads) {
        key[r] = unused;
        row[r] = static_cast<uint32_t>(r);
        pattern_out[r] = 0;
        if (segment_begin) {
            sorted_key[r] = unused;
            sorted_row[r] = static_cast<uint32_t>(r);
        }
    }
}

// The experiment switches of the collapse (docs/design/knobs.md; the names exist in an EXPERIMENTS=1 build only).  The grid once per
// process; the others per call: the tests take both ways of the sort in one process.
CollapseKnobs collapseKnobs() {
    static const uint32_t small_grid = RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_GRID") ? std::max(1, std::atoi(RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_GRID"))) : 256;
    CollapseKnobs k;
    k.small_grid = small_grid;
    // the library's radix sorts instead of the hand-written segment sort (A/B, and the only way to the library routes below 2^20 rows)
    const char * library = RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_LIBRARY_SORT");
    k.library_sort_matrices = library != nullptr && (std::strcmp(library, "1") == 0 || std::strcmp(library, "matrices") == 0);
    k.library_sort_problems = library != nullptr && (std::strcmp(library, "1") == 0 || std::strcmp(library, "problems") == 0);
    k.no_lds_tables = RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_NO_LDS_TABLES") != nullptr;
    k.debug = RPVG_EXPERIMENT_ENV("RPVG_HIP_EM_COLLAPSE_DEBUG") != nullptr;
    return k;
}

// ---- the sort, one function per route ------------------------------------------------------------------------------------------------
// HandSort: the segment sort in registers; for the EM problems behind the kernel that fills the row slots no problem uses
template <typename Arrays, typename Caller>
hipError_t queueHandSort(const Arrays & arrays, const CollapsePlan & plan, const Caller & caller, const CollapseTemporaries & t, hipStream_t st) {
    const hipError_t e = zeroAsync(t.chunk_count.ptr, sizeof(uint32_t), st);
    SegmentSortArgs<Arrays> c = segmentSortArgs(arrays, plan, t);
    setKeySource(c, caller, t);
    if (Arrays::kHashBits) collapseUnusedSlotsKernel<Arrays><<<dim3(plan.unused_slots.grid), dim3(plan.unused_slots.block), 0, st>>>(c);
    launchSegmentSort(c, plan.segment_sort, st);
    return e;
}
// LibraryGlobal / LibrarySegmented (queueLibrarySort of the caller), then "equal to its predecessor" for every sorted position
template <typename Arrays, typename Caller>
hipError_t queueLibrarySortAndSamePrev(const PairScanArgs<Arrays> & a, const CollapsePlan & plan, const Caller & caller, const CollapseTemporaries & t, hipStream_t st) {
    size_t bytes = t.sort_tmp.count;
    const hipError_t e = queueLibrarySort(caller, plan, t, t.sort_tmp.ptr, bytes, st);
    collapseSamePrevKernel<Arrays><<<dim3(plan.same_prev.grid), dim3(plan.same_prev.block), 0, st>>>(a);
    return e;
}

// The stages of a collapse, for group matrices and for EM problems alike, behind allocateCollapse (and, on the EM problems' library
// route, csrCollapseKeysKernel): `info` receives [counters | zeroed words | active bytes | list sizes] (InfoLayout).
template <typename Arrays, typename Caller>
hipError_t queueCollapseStages(const Arrays & arrays, const CollapsePlan & plan, const CollapseKnobs & knobs, const double precision, const Caller & caller,
                               CollapseTemporaries & t, uint32_t * info, hipEvent_t sorted, hipStream_t st) {
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    ok(zeroAsync(info, plan.info.zeroed_words * sizeof(uint32_t), st));
    PairScanArgs<Arrays> a = pairScanArgs(arrays, plan, knobs, precision, t, info);
    // the sort
    if (plan.route == HandSort) ok(queueHandSort(arrays, plan, caller, t, st));
    else ok(queueLibrarySortAndSamePrev(a, plan, caller, t, st));
    if (sorted) ok(hipEventRecord(sorted, st));
    // the pair scans
    size_t scan_bytes = t.sort_tmp.count;
    ok(queueStretchScan(t, plan.total_rows, t.sort_tmp.ptr, scan_bytes, st));
    a.stretch_first = t.stretchFirst(plan.total_rows);
    collapseStretchEndKernel<Arrays><<<dim3(plan.stretch_end.grid), dim3(plan.stretch_end.block), 0, st>>>(a);
    collapseForwardPairsKernel<Arrays><<<dim3(plan.forward_pairs.grid), dim3(plan.forward_pairs.block), 0, st>>>(a);
    collapseMarkPairsKernel<Arrays><<<dim3(plan.mark_pairs.grid), dim3(plan.mark_pairs.block), 0, st>>>(a);
    a.pair_count += 1;  // the list is free again
    collapseAroundPairsKernel<Arrays><<<dim3(plan.around_pairs.grid), dim3(plan.around_pairs.block), 0, st>>>(a);
    collapseActivePairsKernel<Arrays><<<dim3(plan.active_pairs.grid), dim3(plan.active_pairs.block), 0, st>>>(a);
    // the replay
    ReplayArgs<Arrays> r = replayArgs(arrays, plan, knobs, precision, t, info);
    setOutputs(r, caller);
    collapseListKernel<Arrays><<<dim3(plan.list.grid), dim3(plan.list.block), 0, st>>>(r);
    collapsePairTableKernel<Arrays><<<dim3(plan.pair_table.grid), dim3(plan.pair_table.block), 0, st>>>(r);
    collapseRankKernel<Arrays><<<dim3(plan.rank.grid), dim3(plan.rank.block), 0, st>>>(r);
    collapseSortKernel<Arrays><<<dim3(plan.list_sort.grid), dim3(plan.list_sort.block), 0, st>>>(r);
    collapseBetweenKernel<Arrays><<<dim3(plan.between.grid), dim3(plan.between.block), 0, st>>>(r);
    // the runs
    ok(queueRuns(r, plan, caller, t, st));
    ok(hipGetLastError());
    return e;
}

}  // namespace

// Queues the collapse of the matrices of `g` on `st` behind their build (rpvg_hip_groups_build).
hipError_t rpvg_hip_detail::queueRowCollapse(rpvg_hip_ctx * ctx, rpvg_hip_groups * g, const uint64_t total_rows, const double precision,
                                             hipStream_t st, const bool hold_back_runs) {
    CollapseShape shape;
    shape.M = g->num_matrices;
    shape.total_rows = total_rows;
    for (uint32_t m = 0; m < shape.M; ++m) shape.max_segment_rows = std::max<uint64_t>(shape.max_segment_rows, g->h_num_rows[m]);
    shape.hash_bits = MatrixArrays::kHashBits;
    shape.caller_keys = true;
    (void) ctx;  // (the CU count sizes the keys kernel of the EM problems only)
    const CollapseKnobs knobs = collapseKnobs();
    const CollapsePlan plan = planCollapse(shape, knobs);
    if (plan.verdict != kRun) return plan.verdict == kNothingToDo ? hipSuccess : hipErrorInvalidValue;
    std::shared_ptr<CollapseTemporaries> tmp = std::make_shared<CollapseTemporaries>();
    g->build_temporaries.emplace_back(tmp);
    const MatrixCaller caller{g->collapse_key.ptr, g->collapse_row.ptr, g->rowmax.ptr, g->mat_fast.ptr, g->mat_mid.ptr, hold_back_runs ? &g->held_back_runs : nullptr};
    const hipError_t e = allocateCollapse(plan, caller, *tmp, g->collapse_info, st);
    if (e != hipSuccess) return e;
    MatrixArrays arrays;
    arrays.mat_val_off = g->mat_val_off.ptr;
    arrays.mat_row_off = g->mat_row_off.ptr;
    arrays.mat_rows = g->mat_rows.ptr;
    arrays.mat_cols = g->mat_cols.ptr;
    arrays.values = g->values.ptr;
    arrays.row_noise = g->row_noise.ptr;
    arrays.row_count = g->row_count.ptr;
    arrays.zero_pattern = g->collapse_mask.ptr;
    return queueCollapseStages(arrays, plan, knobs, precision, caller, *tmp, g->collapse_info.ptr, nullptr, st);
}

// readCollapseProbabilityMatrix on the rows of every EM problem of a solve (src/path_abundance_estimator.cpp:266,668): queued
// on `st` behind the compaction of the problems' rows.  Afterwards work.problem_merged[p] != 0 marks the problems in which a
// run joined rows that were not equal up to rounding, merged_count holds their read counts after the merges (a merged
// row's count moved to its run head) and merged_problems[0] their number.
hipError_t rpvg_hip_detail::queueCsrCollapse(rpvg_hip_ctx * ctx, const CsrCollapseInput & in, const double precision, CsrCollapseWork & work, hipStream_t st,
                                             hipEvent_t sorted) {
    const uint32_t P = in.num_problems_bound;
    // The hand-written segment sort computes the keys itself; problems of 2^20 rows or more (by the bound) and the A/B knob take
    // the library sort behind csrCollapseKeysKernel.
    CollapseShape shape;
    shape.M = P;
    shape.total_rows = in.rows_capacity;
    shape.max_segment_rows = in.max_rows_bound;
    shape.hash_bits = CsrArrays::kHashBits;
    shape.caller_keys = false;
    shape.num_items_bound = in.num_items_bound;
    shape.cus = static_cast<uint32_t>(ctx->props.multiProcessorCount);
    const CollapseKnobs knobs = collapseKnobs();
    const CollapsePlan plan = planCollapse(shape, knobs);
    if (plan.verdict != kRun) return plan.verdict == kNothingToDo ? hipSuccess : hipErrorInvalidValue;
    std::shared_ptr<CollapseTemporaries> tmp = std::make_shared<CollapseTemporaries>();
    work.temporaries = tmp;
    const ProblemCaller caller{in};
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    ok(allocateCollapse(plan, caller, *tmp, work.info, st));
    ok(work.merged_count.alloc(plan.total_rows));
    ok(work.problem_merged.alloc(P + 1));  // [P]: the number of merged problems
    if (e != hipSuccess) return e;
    ok(zeroAsync(work.problem_merged.ptr, (P + 1) * sizeof(uint32_t), st));
    CsrArrays arrays;
    arrays.problems = in.problems;
    arrays.zero_pattern = tmp->csr_pattern.ptr;
    arrays.merged_count = work.merged_count.ptr;
    arrays.problem_merged = work.problem_merged.ptr;
    arrays.merged_problems = work.problem_merged.ptr + P;
    if (plan.route == LibrarySegmented) {
        uint32_t * segment_begin = tmp->csr_segments.ptr, * segment_end = segment_begin + P;
        csrCollapseKeysKernel<<<dim3(plan.keys.grid), dim3(plan.keys.block), 0, st>>>(arrays, P, in.num_problems_dev, in.num_items_bound, in.num_items_dev, in.seg_first,
                                                                                    in.item_problem, in.segment_rows, plan.total_rows, tmp->csr_key.ptr, tmp->csr_row.ptr,
                                                                                    tmp->csr_pattern.ptr, segment_begin, segment_end, tmp->key_out.ptr, tmp->row_out.ptr);
        ok(hipGetLastError());
        if (e != hipSuccess) return e;
    }
    return queueCollapseStages(arrays, plan, knobs, precision, caller, *tmp, work.info.ptr, sorted, st);
}

extern "C" int rpvg_hip_groups_collapse_info(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t * matrices_replayed,
                                             uint32_t * rows_replaced, uint32_t * matrices_sorted_whole, uint32_t * active_rows) {
    RPVG_REQUIRE(ctx && groups, "rpvg_hip_groups_collapse_info: NULL argument");
    uint32_t info[kInfoWords] = {0};
    if (groups->collapse_info.ptr) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        RPVG_HIP_CHECK(groups->waitCollapse(ctx->stream));
        RPVG_HIP_CHECK(hipMemcpyAsync(info, groups->collapse_info.ptr + InfoLayout::info, sizeof(info), hipMemcpyDeviceToHost, ctx->stream));
        RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    if (matrices_replayed) *matrices_replayed = info[kInfoMatrices];
    if (rows_replaced) *rows_replaced = info[kInfoRowsReplaced];
    if (matrices_sorted_whole) *matrices_sorted_whole = info[kInfoWholeMatrices];
    if (active_rows) *active_rows = info[kInfoActiveRows];
    return RPVG_HIP_OK;
}

// The segment sort of the collapse on caller-supplied words, for its test (include/rpvg_hip.h): the launches of
// launchSegmentSort — small kernel, chunk kernel, the rounds the longest segment needs, the read-back of every chunked segment
// from its own final buffer — with the words as they are in place of the rows' keys and `out` in place of the positions.
extern "C" int rpvg_hip_segment_sort_words(rpvg_hip_ctx * ctx, const uint64_t * words, const uint64_t * segment_off, uint32_t num_segments, uint64_t * out) {
    RPVG_REQUIRE(ctx && segment_off, "rpvg_hip_segment_sort_words: NULL argument");
    if (num_segments == 0) return RPVG_HIP_OK;
    uint64_t longest = 0;
    for (uint32_t s = 0; s < num_segments; ++s) {
        RPVG_REQUIRE(segment_off[s] <= segment_off[s + 1], "rpvg_hip_segment_sort_words: segment_off descends at segment %u", s);
        longest = std::max(longest, segment_off[s + 1] - segment_off[s]);
    }
    const uint64_t total = segment_off[num_segments];
    RPVG_REQUIRE(segment_off[0] == 0 && total <= 0x7fffffffull, "rpvg_hip_segment_sort_words: segment_off must start at 0 and end below 2^31");
    if (total == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(words && out, "rpvg_hip_segment_sort_words: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<uint64_t> d_words, d_off, d_out, words_a, words_b;
    DeviceBuffer<uint32_t> chunks, chunk_count;
    const SegmentSortPlan plan = planSegmentSort(num_segments, total, longest, CollapseKnobs().small_grid);
    RPVG_HIP_CHECK(d_words.upload(words, total, st));
    RPVG_HIP_CHECK(d_off.upload(segment_off, static_cast<size_t>(num_segments) + 1, st));
    RPVG_HIP_CHECK(d_out.alloc(total));
    RPVG_HIP_CHECK(words_a.alloc(total));
    RPVG_HIP_CHECK(words_b.alloc(total));
    RPVG_HIP_CHECK(chunks.alloc(2 * static_cast<size_t>(plan.chunk_capacity)));
    RPVG_HIP_CHECK(chunk_count.alloc(1));
    RPVG_HIP_CHECK(zeroAsync(chunk_count.ptr, sizeof(uint32_t), st));
    SegmentSortArgs<WordArrays> c{};
    c.g.words = d_words.ptr;
    c.g.segment_off = d_off.ptr;
    c.g.out = d_out.ptr;
    c.num_matrices = num_segments;
    c.total_rows = total;
    c.words_a = words_a.ptr;
    c.words_b = words_b.ptr;
    c.chunks = chunks.ptr;
    c.chunk_count = chunk_count.ptr;
    c.chunk_capacity = plan.chunk_capacity;
    launchSegmentSort(c, plan, st);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(d_out.download(out, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}
