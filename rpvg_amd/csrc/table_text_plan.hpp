// The rows of a result file as text (table_text.hip; interface include/rpvg_text.h): ONE shape of row for the Gibbs samples file and
// the two per-path estimates files, described by TextRows, and what a row is made of: cell by cell for the kernels (a wavefront
// along a row), row by row for one host thread (the comparison line of the harness).  Plain C++17 under the RPVG_PLAN_FN convention,
// so the kernels and the CPU check (tests/cpp/table_text_plan_check.cpp) walk the same code.
//
//   row r   =  name bytes  '\t' cluster_id[k]  [ '\t' second_u32[r] ]  ( '\t' fixed column )*  ( '\t' run[r * run_stride + s] ){run_length}  '\n'
//
// with k the cluster of row r (cluster_path_off).  The cells of a row are numbered behind the name: cell c is the tab and the text of
// its value, and the last cell carries the '\n'.  A row the filter drops has no bytes.
#ifndef RPVG_HIP_TABLE_TEXT_PLAN_HPP
#define RPVG_HIP_TABLE_TEXT_PLAN_HPP

#include <cstdint>

#include "number_text.hpp"
#include "table_kit.hpp"

namespace rpvg_table_text {

constexpr int kMaxFixedColumns = 4;
constexpr int kMaxCellBytes = 2 + rpvg_number_text::kMaxCellBytes;  // '\t', the value, '\n'
constexpr int kStepCells = 64;                                      // a wavefront's step: a cell (or a piece of the name) per lane
constexpr int kStageBytes = 4 + kStepCells * kMaxCellBytes;         // of LDS per wavefront: a step's text behind at most 3 bytes carried over

// a column of doubles: values[r], or with cluster_base values[cluster_base[k] + (r - cluster_path_off[k])]
struct DoubleColumn {
    const double * values;
    const uint64_t * cluster_base;  // [K] or NULL
};

struct TextRows {
    uint64_t num_rows;                 // P
    uint32_t num_clusters;             // K
    const uint64_t * name_off;         // [P+1]
    const char * name_bytes;
    const uint64_t * cluster_path_off; // [K+1]
    const uint32_t * cluster_id;       // [K]
    const uint32_t * second_u32;       // [P] or NULL: no such column
    uint32_t num_fixed;                // <= kMaxFixedColumns
    DoubleColumn fixed[kMaxFixedColumns];
    uint64_t run_length;               // N; 0: no run
    const double * run;
    uint64_t run_stride;
    const uint8_t * filter;            // [P] or NULL: every row
    int precision;
    const uint64_t * pow10;            // rpvg_number_text::buildPow10Table
};

// NULL, or what is wrong with the numbers of a descriptor (the pointers are the builder's)
RPVG_PLAN_FN const char * descriptorBad(const TextRows & t) {
    if (t.precision < rpvg_number_text::kMinPrecision || t.precision > rpvg_number_text::kMaxPrecision) return "precision outside 1 .. 17";
    if (t.num_fixed > static_cast<uint32_t>(kMaxFixedColumns)) return "too many fixed columns";
    if (t.run_length > 0 && t.run_stride < t.run_length) return "a run longer than its stride";
    if (t.num_clusters == 0 && t.num_rows != 0) return "rows without clusters";
    return nullptr;
}

RPVG_PLAN_FN uint64_t headCells(const TextRows & t) { return 1u + (t.second_u32 ? 1u : 0u) + t.num_fixed; }
RPVG_PLAN_FN uint64_t numCells(const TextRows & t) { return headCells(t) + t.run_length; }
RPVG_PLAN_FN bool printed(const TextRows & t, const uint64_t r) { return !t.filter || t.filter[r] != 0; }
RPVG_PLAN_FN uint64_t clusterOf(const TextRows & t, const uint64_t r) { return rpvg_hip_detail::lastAtMost(t.cluster_path_off, t.num_clusters, r); }
RPVG_PLAN_FN uint64_t nameBytes(const TextRows & t, const uint64_t r) { return t.name_off[r + 1] - t.name_off[r]; }

// the double of cell c >= 1 + (second_u32 ? 1 : 0) of row r of cluster k
RPVG_PLAN_FN double doubleOfCell(const TextRows & t, const uint64_t r, const uint64_t k, const uint64_t c) {
    const uint64_t first = 1u + (t.second_u32 ? 1u : 0u);
    if (c < first + t.num_fixed) {
        const DoubleColumn & column = t.fixed[c - first];
        return column.cluster_base ? column.values[column.cluster_base[k] + (r - t.cluster_path_off[k])] : column.values[r];
    }
    return t.run[r * t.run_stride + (c - first - t.num_fixed)];
}

// cell c of row r of cluster k, read and decomposed once: a lane measures it and stores it from the same value
struct Cell {
    rpvg_number_text::Decimal decimal;  // !is_u32
    uint32_t u32;
    bool is_u32;
    bool last;  // carries the '\n'
};

RPVG_PLAN_FN Cell cellOf(const TextRows & t, const uint64_t r, const uint64_t k, const uint64_t c) {
    Cell cell;
    cell.is_u32 = c == 0 || (c == 1 && t.second_u32);
    cell.u32 = 0;
    cell.last = c + 1 == numCells(t);
    if (cell.is_u32) {
        cell.u32 = c == 0 ? t.cluster_id[k] : t.second_u32[r];
        cell.decimal = rpvg_number_text::Decimal{0, 0, rpvg_number_text::kZero, false, false, false, false};
    } else {
        cell.decimal = rpvg_number_text::decompose(doubleOfCell(t, r, k, c), t.precision, t.pow10);
    }
    return cell;
}

// The bytes of a cell, the tab in front included: written to out (kStore) or counted; at most kMaxCellBytes.
template <bool kStore>
RPVG_PLAN_FN uint32_t cellText(const Cell & cell, const int precision, char * out) {
    uint32_t n = 1;
    if (kStore) out[0] = '\t';
    if (cell.is_u32) n += kStore ? rpvg_number_text::formatU32(cell.u32, out + 1) : rpvg_number_text::decimalDigits(cell.u32);
    else n += rpvg_number_text::textOf<kStore>(cell.decimal, precision, out + 1);
    if (cell.last) {
        if (kStore) out[n] = '\n';
        n += 1;
    }
    return n;
}

// rows of at most this many cells are measured by a lane each, wider ones by a wavefront each
constexpr uint64_t kNarrowCells = 8;
RPVG_PLAN_FN bool measuredByWavefront(const TextRows & t) { return numCells(t) > kNarrowCells; }

// the bytes of row r, one cell behind the other (a lane of the measure kernel for the rows of few cells; the host line)
RPVG_PLAN_FN uint64_t rowBytes(const TextRows & t, const uint64_t r, uint64_t * exact_cells) {
    if (!printed(t, r)) return 0;
    const uint64_t k = clusterOf(t, r), cells = numCells(t);
    uint64_t bytes = nameBytes(t, r);
    for (uint64_t c = 0; c < cells; ++c) {
        const Cell cell = cellOf(t, r, k, c);
        bytes += cellText<false>(cell, t.precision, nullptr);
        *exact_cells += cell.decimal.exact ? 1u : 0u;
    }
    return bytes;
}

// row r written to out (rowBytes(r) bytes) by one thread
RPVG_PLAN_FN uint64_t rowWrite(const TextRows & t, const uint64_t r, char * out) {
    if (!printed(t, r)) return 0;
    const uint64_t k = clusterOf(t, r), cells = numCells(t), name = nameBytes(t, r);
    for (uint64_t i = 0; i < name; ++i) out[i] = t.name_bytes[t.name_off[r] + i];
    uint64_t at = name;
    for (uint64_t c = 0; c < cells; ++c) at += cellText<true>(cellOf(t, r, k, c), t.precision, out + at);
    return at;
}

// ---- a wavefront's step -------------------------------------------------------------------------------------------------------
// The text of a row leaves the staging block of kStageBytes as aligned 4-byte words.  Byte i of the block stands for byte
// base + i of the text, base a multiple of 4; [lo, hi) of the block is filled.  flushPlan says what of it may leave now:
//   head bytes   [lo, head_end) one by one — the ragged start of the row (lo > 0 happens in a row's first step alone)
//   words        [first_word, end_word) as words
//   tail bytes   [tail_begin, hi) one by one — at the end of the row only; otherwise they stay, moved down by `advance`
// so that every byte of [row_off[r], row_off[r+1]) is stored exactly once and no byte outside it is touched.
struct FlushPlan {
    uint32_t head_end;               // head bytes [lo, head_end); head_end == lo: none
    uint32_t first_word, end_word;   // words [first_word, end_word)
    uint32_t tail_begin;             // the bytes [tail_begin, hi) behind them: stored one by one at the end of the row, carried otherwise
    uint32_t advance;                // carried: the base moves on by this (a multiple of 4) and the tail moves to [next_lo, next_hi)
    uint32_t next_lo, next_hi;
};

RPVG_PLAN_FN FlushPlan flushPlan(const uint32_t lo, const uint32_t hi) {
    FlushPlan p;
    const uint32_t whole = hi / 4u;  // words that end at or below hi
    if (lo > 0 && hi < 4u) {         // the row starts inside word 0 and has not reached its end: nothing is complete
        p.head_end = lo;
        p.first_word = p.end_word = 0;
        p.tail_begin = lo;
        p.advance = 0;
        p.next_lo = lo;
        p.next_hi = hi;
        return p;
    }
    p.head_end = lo > 0 ? 4u : 0u;
    p.first_word = lo > 0 ? 1u : 0u;
    p.end_word = whole;
    p.tail_begin = 4u * whole;
    p.advance = 4u * whole;
    p.next_lo = 0;
    p.next_hi = hi - 4u * whole;
    return p;
}

}  // namespace rpvg_table_text

#endif
