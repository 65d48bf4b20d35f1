// The --write-probs dump as text (rows_text.hip; interface include/rpvg_text.h): the file of ProbabilityClusterWriter::addCluster
// (src/threaded_output_writer.cpp:40-95), of which writeProbabilityClusters (rpvg_amd/host/io/cluster_io.cpp) is this project's copy,
// described by DumpRows.  The third shape of row beside TextRows (table_text_plan.hpp) and SetRows (set_text_plan.hpp): a ragged line
// of `prob:idx,idx,...` groups.  From table_text_plan.hpp this takes flushPlan and the staging constants; the digits are
// number_text.hpp's.  Plain C++17 under the RPVG_PLAN_FN convention, so the kernels, the host comparison line and the CPU check
// (tests/cpp/rows_text_plan_check.cpp) walk the same code.
//
// For cluster k with n_k > 0 paths and at least one row (any other cluster has no bytes):
//
//   marker line   "#\n"                     or, with rank keys,   "# " num_align_lists[k] " " cluster_index[k] "\n"
//   path line     name(p) "," path_length[p] "," path_effective_length[p]    for every path p, a ' ' between paths, then "\n"
//   row line      row_count[r] " " row_noise[r]  ( " " grp_prob[g] ":" idx "," idx ... ){groups of r}  "\n"
//
// The effective length is printed at kPathDigits = 8, row_noise and grp_prob at `digits`.  The text has L = 2 K + R LINES in file
// order: line 2 k + cluster_row_off[k] is the marker of cluster k, the next its path line, line 2 (k + 1) + r is row r of cluster k.
// The `rows` of the text's handle are these lines.
//
// CELLS.  The whole file is one flat sequence of cells in file order, C = 3 K + 3 P + 2 R + G + M of them:
//   cluster k    2 marker cells    "#" [" " lists]    and    [" " index] "\n"
//                3 cells a path    [" "] name    "," length    "," effective length          (the NAME cell is the only unbounded one)
//                1 end cell        "\n" of the path line
//   row r        count    " " noise    and for every group    " " prob ":"    and for every member    [","] idx
//                the last cell of a row carries its "\n"
// A cell of a cluster that is not printed has no bytes but keeps its place, so the first cell of cluster k and of row r have closed
// forms:   clusterCell(k) = 3 k + 3 cluster_path_off[k] + rowCell(cluster_row_off[k]),   rowCell(r) = 2 r + row_grp_off[r] +
// grp_idx_off[row_grp_off[r]]  (both strictly increasing), and row r of cluster k starts at 3 (k + 1) + 3 cluster_path_off[k + 1] +
// rowCell(r).  Every cell but a name is at most kMaxDumpCellBytes long.
//
// ROUTES and their limits.
//   lengths     a lane per cell: cell_len [C + 1] (64-bit), one exclusive sum over the CELLS gives cell_off, and the offset of a line
//               is the offset of its first cell (every line has a cell).  Hence C + 1 < 2^31 and L + 1 < 2^31.
//   the text    a wavefront takes 64 consecutive cells wherever the line ends fall (blockWalk): their bytes are one contiguous range
//               of the file.  It finds the cluster of its first cell by bisection over clusterCell and then walks uniformly: runs of
//               bounded cells (a lane a cell; a lane of a row run finds its row and group by bisection over rowCell and the row's
//               groups) and name cells (all lanes along the name, 64 bytes a pass).  A row of five cells fills five lanes, not a
//               wavefront; a row of thousands of indices and a path line of thousands of names are as many wavefronts as they need.
//               The staging block leaves when it is full and at the end of the 64 cells, the ragged first and last word byte by byte.
//   64 bounded cells are at most 63 * 26 + 27 = 1665 bytes (only the last cell of a row that ends in a group without members has
//   27, and a second one has a read count of at most 10 bytes before it): they fit the staging block behind a carried word.
#ifndef RPVG_HIP_ROWS_TEXT_PLAN_HPP
#define RPVG_HIP_ROWS_TEXT_PLAN_HPP

#include <cstdint>

#include <algorithm>
#include <cmath>

#include "table_text_plan.hpp"

namespace rpvg_rows_text {

using rpvg_hip_detail::lastAtMost;
using rpvg_table_text::kStageBytes;

constexpr int kPathDigits = 8;             // out_precision_digits (src/threaded_output_writer.cpp:6)
constexpr uint32_t kBlockCells = 64;       // a wavefront's cells
constexpr uint32_t kMaxDumpCellBytes = 27; // ' ' -1.2345678901234567e-308 ':' '\n'
constexpr uint64_t kMaxLines = 0x7ffffffeull, kMaxCells = 0x7ffffffeull;  // fewer than 2^31 - 1 of each
static_assert(kStageBytes % 4 == 0 && 3 + (kBlockCells - 1) * (kMaxDumpCellBytes - 1) + kMaxDumpCellBytes <= static_cast<uint32_t>(kStageBytes), "64 bounded cells fit the staging block behind a carried word");

// (host) the digits of row_noise and grp_prob, as the reference chooses them (src/threaded_output_writer.cpp:40)
inline uint32_t probPrecisionDigits(const double prob_precision) {
    return std::max(static_cast<uint32_t>(kPathDigits), static_cast<uint32_t>(std::ceil(-1 * std::log10(prob_precision))));
}
// NULL, or why a dump cannot be written at this prob_precision
inline const char * probPrecisionBad(const double prob_precision) {
    if (!(prob_precision > 0.0 && prob_precision < 1.0)) return "prob_precision outside (0, 1)";
    if (probPrecisionDigits(prob_precision) > static_cast<uint32_t>(rpvg_number_text::kMaxPrecision)) return "prob_precision asks for more than 17 digits";
    return nullptr;
}

struct DumpRows {
    uint32_t num_clusters;                 // K
    uint64_t num_rows, num_groups, num_entries, num_paths;  // R, G, M, P
    const uint64_t * cluster_row_off;      // [K+1]
    const uint64_t * cluster_path_off;     // [K+1]
    const uint32_t * row_count;            // [R]
    const double * row_noise;              // [R]
    const uint64_t * row_grp_off;          // [R+1]
    const double * grp_prob;               // [G]
    const uint64_t * grp_idx_off;          // [G+1]
    const uint32_t * path_idx;             // [M] cluster-local
    const uint64_t * name_off;             // [P+1]
    const char * name_bytes;
    const uint32_t * path_length;          // [P]
    const double * path_effective_length;  // [P]
    const uint64_t * num_align_lists;      // [K] or NULL: bare markers
    const uint64_t * cluster_index;        // [K] with num_align_lists
    int digits;                            // of row_noise and grp_prob
    const uint64_t * pow10;                // rpvg_number_text::buildPow10Table
    const uint64_t * cluster_cell;         // [K+1] clusterCell(k): blockWalk and lineCell only
    const uint64_t * row_cell;             // [R+1] rowCell(r):     blockWalk and lineCell only
};

RPVG_PLAN_FN uint64_t numLines(const DumpRows & t) { return 2ull * t.num_clusters + t.num_rows; }
RPVG_PLAN_FN uint64_t numCells(const DumpRows & t) { return 3ull * t.num_clusters + 3ull * t.num_paths + 2ull * t.num_rows + t.num_groups + t.num_entries; }

// NULL, or what is wrong with the numbers of a descriptor (the pointers are the builder's)
RPVG_PLAN_FN const char * descriptorBad(const DumpRows & t) {
    if (t.digits < kPathDigits || t.digits > rpvg_number_text::kMaxPrecision) return "digits outside 8 .. 17";
    if ((t.num_align_lists == nullptr) != (t.cluster_index == nullptr)) return "one rank-key array without the other";
    if (t.num_clusters == 0 && (t.num_rows != 0 || t.num_paths != 0)) return "rows or paths without clusters";
    if (numLines(t) > kMaxLines) return "2^31 - 1 lines or more";
    if (numCells(t) > kMaxCells) return "2^31 - 1 cells or more";
    return nullptr;
}

// the closed forms of the header (r in 0 .. R, k in 0 .. K)
RPVG_PLAN_FN uint64_t rowCell(const DumpRows & t, const uint64_t r) {
    const uint64_t g = t.row_grp_off[r];
    return 2ull * r + g + t.grp_idx_off[g];
}
RPVG_PLAN_FN uint64_t clusterCell(const DumpRows & t, const uint64_t k) { return 3ull * k + 3ull * t.cluster_path_off[k] + rowCell(t, t.cluster_row_off[k]); }

RPVG_PLAN_FN bool clusterPrinted(const DumpRows & t, const uint64_t k) {
    return t.cluster_path_off[k + 1] > t.cluster_path_off[k] && t.cluster_row_off[k + 1] > t.cluster_row_off[k];
}

// ---- a bounded cell ---------------------------------------------------------------------------------------------------------------
// [lead0 [lead1]] value [trail] ['\n'], read and decomposed once: a lane measures it and stores it from the same value
enum DumpCellKind { kCellNone = 0, kCellU32 = 1, kCellU64 = 2, kCellDouble = 3 };

struct DumpCell {
    rpvg_number_text::Decimal decimal;  // kCellDouble
    uint64_t integer;                   // kCellU32, kCellU64
    int kind, precision;
    char lead0, lead1, trail;           // 0: none
    bool newline;
};

// the bytes of a cell: written to out (kStore) or counted; at most kMaxDumpCellBytes
template <bool kStore>
RPVG_PLAN_FN uint32_t dumpCellText(const DumpCell & cell, char * out) {
    uint32_t n = 0;
    if (cell.lead0) {
        if (kStore) out[n] = cell.lead0;
        n += 1;
    }
    if (cell.lead1) {
        if (kStore) out[n] = cell.lead1;
        n += 1;
    }
    if (cell.kind == kCellU32) n += kStore ? rpvg_number_text::formatU32(static_cast<uint32_t>(cell.integer), out + n) : rpvg_number_text::decimalDigits(static_cast<uint32_t>(cell.integer));
    else if (cell.kind == kCellU64) n += kStore ? rpvg_number_text::formatU64(cell.integer, out + n) : rpvg_number_text::decimalDigits64(cell.integer);
    else if (cell.kind == kCellDouble) n += rpvg_number_text::textOf<kStore>(cell.decimal, cell.precision, out + n);
    if (cell.trail) {
        if (kStore) out[n] = cell.trail;
        n += 1;
    }
    if (cell.newline) {
        if (kStore) out[n] = '\n';
        n += 1;
    }
    return n;
}

// what a cell prints, before the one decompose of cellFrom
struct CellSource {
    int kind;
    uint64_t integer;
    double value;
    int precision;
    char lead0, lead1, trail;
    bool newline;
};

RPVG_PLAN_FN CellSource sourceOf(const int kind, const char lead0, const char lead1, const char trail, const bool newline) {
    return CellSource{kind, 0, 0.0, kPathDigits, lead0, lead1, trail, newline};
}

RPVG_PLAN_FN DumpCell cellFrom(const DumpRows & t, const CellSource & s) {
    DumpCell cell;
    cell.decimal = rpvg_number_text::Decimal{0, 0, rpvg_number_text::kZero, false, false, false, false};
    if (s.kind == kCellDouble) cell.decimal = rpvg_number_text::decompose(s.value, s.precision, t.pow10);
    cell.integer = s.integer;
    cell.kind = s.kind;
    cell.precision = s.precision;
    cell.lead0 = s.lead0;
    cell.lead1 = s.lead1;
    cell.trail = s.trail;
    cell.newline = s.newline;
    return cell;
}

// marker cell `which` (0, 1) of cluster k
RPVG_PLAN_FN CellSource markerSource(const DumpRows & t, const uint64_t k, const uint32_t which) {
    const bool ranked = t.num_align_lists != nullptr;
    CellSource s = which == 0 ? sourceOf(ranked ? kCellU64 : kCellNone, '#', ranked ? ' ' : 0, 0, false) : sourceOf(ranked ? kCellU64 : kCellNone, ranked ? ' ' : 0, 0, 0, true);
    if (ranked) s.integer = which == 0 ? t.num_align_lists[k] : t.cluster_index[k];
    return s;
}

// number cell `which` (1 the length, 2 the effective length) of path p
RPVG_PLAN_FN CellSource pathSource(const DumpRows & t, const uint64_t p, const uint32_t which) {
    CellSource s = sourceOf(which == 1 ? kCellU32 : kCellDouble, ',', 0, 0, false);
    if (which == 1) s.integer = t.path_length[p];
    else s.value = t.path_effective_length[p];
    return s;
}

// cell e of row r: 0 the count, 1 the noise, then a cell per group and per member
RPVG_PLAN_FN CellSource rowSource(const DumpRows & t, const uint64_t r, const uint64_t e, const bool last) {
    if (e == 0) {
        CellSource s = sourceOf(kCellU32, 0, 0, 0, false);
        s.integer = t.row_count[r];
        return s;
    }
    if (e == 1) {
        CellSource s = sourceOf(kCellDouble, ' ', 0, 0, last);
        s.value = t.row_noise[r];
        s.precision = t.digits;
        return s;
    }
    const uint64_t x = e - 2, g0 = t.row_grp_off[r], m0 = t.grp_idx_off[g0];
    uint64_t lo = g0, hi = t.row_grp_off[r + 1];  // the last group whose first cell (g - g0) + (grp_idx_off[g] - m0) is at most x
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((mid - g0) + (t.grp_idx_off[mid] - m0) <= x) lo = mid;
        else hi = mid;
    }
    const uint64_t first = (lo - g0) + (t.grp_idx_off[lo] - m0);
    if (x == first) {
        CellSource s = sourceOf(kCellDouble, ' ', 0, ':', last);
        s.value = t.grp_prob[lo];
        s.precision = t.digits;
        return s;
    }
    const uint64_t j = x - first - 1;
    CellSource s = sourceOf(kCellU32, j ? ',' : 0, 0, 0, last);
    s.integer = t.path_idx[t.grp_idx_off[lo] + j];
    return s;
}

// ---- a line of the text -----------------------------------------------------------------------------------------------------------
enum LineKind { kLineMarker = 0, kLinePaths = 1, kLineRow = 2 };
struct Line {
    uint64_t cluster, row;
    int kind;
};

// line j < L: the last cluster k with 2 k + cluster_row_off[k] <= j
RPVG_PLAN_FN Line lineOf(const DumpRows & t, const uint64_t j) {
    uint64_t lo = 0, hi = t.num_clusters;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (2ull * mid + t.cluster_row_off[mid] <= j) lo = mid;
        else hi = mid;
    }
    const uint64_t d = j - (2ull * lo + t.cluster_row_off[lo]);
    return Line{lo, d >= 2 ? t.cluster_row_off[lo] + d - 2 : 0, d == 0 ? kLineMarker : (d == 1 ? kLinePaths : kLineRow)};
}

// the first cell of line j <= L (cluster_cell and row_cell filled)
RPVG_PLAN_FN uint64_t lineCell(const DumpRows & t, const uint64_t j) {
    if (j >= numLines(t)) return numCells(t);
    const Line line = lineOf(t, j);
    const uint64_t base = t.cluster_cell[line.cluster];
    if (line.kind == kLineMarker) return base;
    if (line.kind == kLinePaths) return base + 2;
    const uint64_t paths = t.cluster_path_off[line.cluster + 1] - t.cluster_path_off[line.cluster];
    return base + 3 + 3 * paths + (t.row_cell[line.row] - t.row_cell[t.cluster_row_off[line.cluster]]);
}

// Line j by one thread, one cell behind the other: counted (kStore false) or written to out.  The host comparison line.
template <bool kStore>
RPVG_PLAN_FN uint64_t lineText(const DumpRows & t, const uint64_t j, char * out, uint64_t * exact_cells) {
    const Line line = lineOf(t, j);
    const uint64_t k = line.cluster;
    if (!clusterPrinted(t, k)) return 0;
    uint64_t at = 0;
    const auto put = [&](const CellSource & source) {
        const DumpCell cell = cellFrom(t, source);
        at += dumpCellText<kStore>(cell, kStore ? out + at : nullptr);
        if (exact_cells) *exact_cells += cell.decimal.exact ? 1u : 0u;
    };
    if (line.kind == kLineMarker) {
        put(markerSource(t, k, 0));
        put(markerSource(t, k, 1));
    } else if (line.kind == kLinePaths) {
        for (uint64_t p = t.cluster_path_off[k]; p < t.cluster_path_off[k + 1]; ++p) {
            if (p > t.cluster_path_off[k]) {
                if (kStore) out[at] = ' ';
                at += 1;
            }
            const uint64_t name = t.name_off[p + 1] - t.name_off[p];
            if (kStore) {
                for (uint64_t i = 0; i < name; ++i) out[at + i] = t.name_bytes[t.name_off[p] + i];
            }
            at += name;
            put(pathSource(t, p, 1));
            put(pathSource(t, p, 2));
        }
        put(sourceOf(kCellNone, 0, 0, 0, true));
    } else {
        const uint64_t r = line.row;
        const uint64_t cells = 2 + (t.row_grp_off[r + 1] - t.row_grp_off[r]) + (t.grp_idx_off[t.row_grp_off[r + 1]] - t.grp_idx_off[t.row_grp_off[r]]);
        for (uint64_t e = 0; e < cells; ++e) put(rowSource(t, r, e, e + 1 == cells));
    }
    return at;
}

RPVG_PLAN_FN uint64_t rowBytes(const DumpRows & t, const uint64_t line, uint64_t * exact_cells) { return lineText<false>(t, line, nullptr, exact_cells); }
RPVG_PLAN_FN uint64_t rowWrite(const DumpRows & t, const uint64_t line, char * out) { return lineText<true>(t, line, out, nullptr); }

// ---- a wavefront's walk along 64 consecutive cells (the measure and the write kernel) -------------------------------------------------
// how much of a name's remaining bytes fits the block now (0: flush first)
RPVG_PLAN_FN uint32_t pieceOf(const uint64_t remaining, const uint32_t hi) {
    const uint32_t room = static_cast<uint32_t>(kStageBytes) - hi;
    return remaining < room ? static_cast<uint32_t>(remaining) : room;
}

// where cell c lies in its cluster
struct ClusterCells {
    uint64_t cluster;
    uint64_t base, next;          // clusterCell(k), clusterCell(k + 1)
    uint64_t first_path, paths;
    uint64_t first_row_cell;      // rowCell(cluster_row_off[k])
    bool printed;
};

RPVG_PLAN_FN ClusterCells clusterCells(const DumpRows & t, const uint64_t k) {
    ClusterCells cc;
    cc.cluster = k;
    cc.base = t.cluster_cell[k];
    cc.next = t.cluster_cell[k + 1];
    cc.first_path = t.cluster_path_off[k];
    cc.paths = t.cluster_path_off[k + 1] - cc.first_path;
    cc.first_row_cell = t.row_cell[t.cluster_row_off[k]];
    cc.printed = clusterPrinted(t, k);
    return cc;
}

// the bounded cell c of the cluster (not a name cell)
RPVG_PLAN_FN CellSource boundedSource(const DumpRows & t, const ClusterCells & cc, const uint64_t c) {
    const uint64_t path_begin = cc.base + 2, end_cell = path_begin + 3 * cc.paths;
    if (c < path_begin) return markerSource(t, cc.cluster, static_cast<uint32_t>(c - cc.base));
    if (c < end_cell) return pathSource(t, cc.first_path + (c - path_begin) / 3, static_cast<uint32_t>((c - path_begin) % 3));
    if (c == end_cell) return sourceOf(kCellNone, 0, 0, 0, true);
    const uint64_t rc = cc.first_row_cell + (c - end_cell - 1);  // among the row cells of the whole file
    uint64_t lo = t.cluster_row_off[cc.cluster], hi = t.cluster_row_off[cc.cluster + 1];  // the last row whose first cell is at most rc
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (t.row_cell[mid] <= rc) lo = mid;
        else hi = mid;
    }
    return rowSource(t, lo, rc - t.row_cell[lo], rc + 1 == t.row_cell[lo + 1]);
}

// The cells [c0, min(C, c0 + 64)) by one wavefront; cell c0 + i is lane i's.  kStore false: w.length(c, bytes) for every cell and
// w.exact counted.  kStore true: the text of the cells through the staging block to its place (cell_off [C + 1]).  `w` is the
// wavefront: the kernel's runs the lane loop once (laneBegin() = the lane), the CPU check's runs it for the 64 lanes in turn;
// everything outside a lane loop is uniform.
template <bool kStore, typename Wave>
RPVG_PLAN_FN void blockWalk(const DumpRows & t, const uint64_t * cell_off, const uint64_t c0, Wave & w) {
    const uint64_t C = numCells(t);
    const uint64_t c1 = c0 + kBlockCells < C ? c0 + kBlockCells : C;
    if (kStore) {
        if (cell_off[c0] == cell_off[c1]) return;
        w.open(cell_off[c0]);
    }
    uint64_t k = lastAtMost(t.cluster_cell, t.num_clusters, c0);
    uint64_t c = c0;
    while (c < c1) {
        const ClusterCells cc = clusterCells(t, k);
        const uint64_t stop = c1 < cc.next ? c1 : cc.next;
        const uint64_t path_begin = cc.base + 2, end_cell = path_begin + 3 * cc.paths;
        while (c < stop) {
            if (!cc.printed) {  // no bytes
                if (!kStore) {
                    for (uint32_t lane = w.laneBegin(); lane < w.laneEnd(); ++lane) {
                        if (c0 + lane >= c && c0 + lane < stop) w.length(c0 + lane, 0);
                    }
                }
                c = stop;
            } else if (c >= path_begin && c < end_cell && (c - path_begin) % 3 == 0) {  // a name: all lanes along it
                const uint64_t j = (c - path_begin) / 3, at = t.name_off[cc.first_path + j];
                const uint64_t space = j ? 1 : 0, bytes = space + (t.name_off[cc.first_path + j + 1] - at);
                if (!kStore) {
                    for (uint32_t lane = w.laneBegin(); lane < w.laneEnd(); ++lane) {
                        if (c0 + lane == c) w.length(c, bytes);
                    }
                } else {
                    uint64_t done = 0;
                    while (done < bytes) {
                        const uint32_t piece = pieceOf(bytes - done, w.hi);
                        if (piece == 0) {  // the block is full
                            w.flush(false);
                            continue;
                        }
                        for (uint32_t lane = w.laneBegin(); lane < w.laneEnd(); ++lane) {
                            for (uint32_t i = lane; i < piece; i += kBlockCells) w.stage[w.hi + i] = (space && done + i == 0) ? ' ' : t.name_bytes[at + (done + i - space)];
                        }
                        w.hi += piece;
                        done += piece;
                    }
                }
                c += 1;
            } else {  // a run of bounded cells, a lane each: up to the next name, or the end of the cluster's share
                uint64_t run_end = stop;
                if (c < path_begin) run_end = path_begin;
                else if (c < end_cell) run_end = path_begin + 3 * ((c - path_begin) / 3 + 1);
                if (run_end > stop) run_end = stop;
                uint32_t bytes = 0;
                if (kStore) {
                    bytes = static_cast<uint32_t>(cell_off[run_end] - cell_off[c]);  // at most 1665: it fits an emptied block
                    if (w.hi + bytes > static_cast<uint32_t>(kStageBytes)) w.flush(false);
                }
                for (uint32_t lane = w.laneBegin(); lane < w.laneEnd(); ++lane) {
                    const uint64_t mine = c0 + lane;
                    if (mine >= c && mine < run_end) {
                        const DumpCell cell = cellFrom(t, boundedSource(t, cc, mine));
                        if (kStore) dumpCellText<true>(cell, w.stage + w.hi + (cell_off[mine] - cell_off[c]));
                        else {
                            w.length(mine, dumpCellText<false>(cell, nullptr));
                            w.exact += cell.decimal.exact ? 1u : 0u;
                        }
                    }
                }
                if (kStore) w.hi += bytes;
                c = run_end;
            }
        }
        k += 1;
    }
    if (kStore) w.flush(true);
}

}  // namespace rpvg_rows_text

#endif
