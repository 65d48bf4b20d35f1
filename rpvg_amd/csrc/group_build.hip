// The build of the group (haplotype / diplotype) matrices on the GPU (gfx950);
// loglik.hip contracts them.
//
// Takes over
//   constructGroupedProbabilityMatrix / constructProbabilityMatrix
//                                            src/path_estimator.cpp:55-77,115-154
//   addNoiseAndNormalizeProbabilityMatrix    src/path_estimator.cpp:156-166
//   rowwise().maxCoeff()                     src/path_estimator.cpp:414
//
// Layout: one column-major R_m x G_m matrix per requested (cluster, grouping),
// so that a wave walking the rows of one or two columns reads contiguous
// memory.  The rows of a matrix are its cluster's rows ordered by class (count
// 1 first: partitionRowsKernel), with counts and noise copied in that order.
// Host side: group_build_plan.hpp decides — refusals, the kernel of every
// matrix, the per-matrix arrays and item lists, every launch's shape —,
// buildGroups below uploads the plan and queues what it says, stage by stage.

#include "common.hpp"
#include "group_build_plan.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <type_traits>

using namespace rpvg_hip_detail;
using namespace rpvg_group_build;

static_assert(rpvg_group_build::kCollapseMaxMatrices == rpvg_hip_detail::kCollapseMaxMatrices && kStatusOk == RPVG_HIP_OK &&
              kStatusInvalid == RPVG_HIP_ERR_INVALID, "group_build_plan.hpp restates these");

namespace {

// Row order of every matrix: the rows of its cluster by class (rowClass, common.hpp) — count 1 first, then the mid
// counts ascending, then the rest — in cluster order within a class (stable, deterministic).  One workgroup per
// matrix: class histogram, then placement chunk by chunk with ballot ranks.
// (BLOCK threads per matrix: 1 024 — a matrix of 20 000 rows is 80 rounds of three barriers on 256 threads, 0.16 ms at the head of
// a lane's chain of kernels)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void partitionRowsKernel(
    const uint32_t num_matrices, const uint64_t * __restrict__ mat_row_off, const uint64_t * __restrict__ mat_row0,
    const uint64_t * __restrict__ mat_rows, const double * __restrict__ row_count, const double * __restrict__ row_noise,
    uint32_t * __restrict__ row_perm, double * __restrict__ count_out, double * __restrict__ noise_out,
    uint32_t * __restrict__ mat_fast, uint32_t * __restrict__ mat_mid, const uint32_t mid_min_rows) {
    __shared__ uint32_t class_base[kNumRowClasses];       // next free slot of every class
    __shared__ uint32_t wave_count[BLOCK / 64][kNumRowClasses];
    const uint32_t m = blockIdx.x;
    if (m >= num_matrices) return;
    const uint32_t R = static_cast<uint32_t>(mat_rows[m]);
    const double * cnt = row_count + mat_row0[m];
    const double * nz = row_noise + mat_row0[m];
    const uint64_t out0 = mat_row_off[m];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < kNumRowClasses) class_base[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < R; i += BLOCK) atomicAdd(&class_base[rowClass(cnt[i], nz[i], R >= mid_min_rows)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t running = 0;
        for (uint32_t c = 0; c < kNumRowClasses; ++c) {
            const uint32_t n = class_base[c];
            class_base[c] = running;
            running += n;
            if (c == 0) mat_fast[m] = running;
            if (c + 2 == kNumRowClasses) mat_mid[m] = running;
        }
    }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < R; c0 += BLOCK) {
        const uint32_t i = c0 + threadIdx.x;
        const bool in = i < R;
        const double c = in ? cnt[i] : 0.0, z = in ? nz[i] : 0.0;
        const uint32_t mine = in ? rowClass(c, z, R >= mid_min_rows) : kNumRowClasses;
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t k = 0; k < kNumRowClasses; ++k) {
            const unsigned long long ballot = __ballot(mine == k);
            if (mine == k) rank = __popcll(ballot & ((1ull << lane) - 1ull));
            if (lane == 0) wave_count[wave][k] = __popcll(ballot);
        }
        __syncthreads();
        if (in) {
            uint32_t dest = class_base[mine] + rank;
            for (int w = 0; w < wave; ++w) dest += wave_count[w][mine];
            row_perm[out0 + dest] = i;
            count_out[out0 + dest] = c;
            noise_out[out0 + dest] = z;
        }
        __syncthreads();
        if (threadIdx.x < kNumRowClasses) {
            uint32_t added = 0;
            for (int w = 0; w < BLOCK / 64; ++w) added += wave_count[w][threadIdx.x];
            class_base[threadIdx.x] += added;
        }
        __syncthreads();
    }
}

// one workgroup per (matrix, chunk of 256 rows), thread per row
__global__ __launch_bounds__(256) void groupsBuildKernel(
    const uint32_t num_items, const uint32_t * __restrict__ item_matrix, const uint32_t * __restrict__ item_chunk,
    const uint64_t * __restrict__ mat_val_off, const uint64_t * __restrict__ mat_row_off,
    const uint64_t * __restrict__ mat_row0, const uint64_t * __restrict__ mat_rows, const uint32_t * __restrict__ mat_cols,
    const uint64_t * __restrict__ mat_inc_off,   // [M] offset of the matrix's path->groups CSR offsets
    const uint64_t * __restrict__ path_grp_off,  // per matrix N_k+1 offsets (absolute into path_grp)
    const uint32_t * __restrict__ path_grp, const uint64_t * __restrict__ row_ent_off,
    const uint32_t * __restrict__ ent_path, const double * __restrict__ ent_prob, const double * __restrict__ row_noise,
    const uint32_t * __restrict__ row_perm, const int normalise, double * __restrict__ values, double * __restrict__ rowmax,
    uint64_t * __restrict__ collapse_key, uint32_t * __restrict__ collapse_row, uint64_t * __restrict__ collapse_mask) {  // null: no row collapse
    if (blockIdx.x >= num_items) return;
    const uint32_t m = item_matrix[blockIdx.x];
    const uint64_t R = mat_rows[m], r0 = mat_row0[m];
    const uint32_t G = mat_cols[m];
    double * M = values + mat_val_off[m];
    double * rm = rowmax + mat_row_off[m];
    const uint64_t * pgo = path_grp_off + mat_inc_off[m];
    const uint64_t i = static_cast<uint64_t>(item_chunk[blockIdx.x]) * 256 + threadIdx.x;
    if (i < R) {
        const uint64_t r = r0 + row_perm[mat_row_off[m] + i];  // matrix row i = this row of the cluster
        for (uint64_t e = row_ent_off[r]; e < row_ent_off[r + 1]; ++e) {
            const uint32_t p = ent_path[e];
            const double v = ent_prob[e];
            for (uint64_t x = pgo[p]; x < pgo[p + 1]; ++x) M[static_cast<uint64_t>(path_grp[x]) * R + i] += v;
        }
        double mx = 0.0;
        if (normalise) {
            double rowsum = 0.0;
            for (uint32_t g = 0; g < G; ++g) rowsum += M[static_cast<uint64_t>(g) * R + i];
            const double keep = 1 - row_noise[r];
            double key = collapseWeight(G) * row_noise[r];
            uint64_t pattern = 0;
            for (uint32_t g = 0; g < G; ++g) {
                double v = (M[static_cast<uint64_t>(g) * R + i] / rowsum) * keep;
                if (v != v) v = 0.0;  // 0/0 rows -> 0 (src/path_estimator.cpp:162)
                M[static_cast<uint64_t>(g) * R + i] = v;
                mx = (g == 0) ? v : fmax(mx, v);
                key = fma(collapseWeight(g), v, key);
                if (g < 64 && v != 0.0) pattern |= 1ull << g;
            }
            if (collapse_key) {
                collapse_key[mat_row_off[m] + i] = collapseSortKey(m, key, mx);
                collapse_row[mat_row_off[m] + i] = static_cast<uint32_t>(mat_row_off[m] + i);
                collapse_mask[mat_row_off[m] + i] = pattern;
            }
        } else {
            for (uint32_t g = 0; g < G; ++g) {
                const double v = M[static_cast<uint64_t>(g) * R + i];
                mx = (g == 0) ? v : fmax(mx, v);
            }
        }
        rm[i] = mx;
    }
}

// The same construction through an LDS tile (tileRows, group_build_plan.hpp): one workgroup per (matrix, tile of rows).  The rows of the tile are
// accumulated, normalised and scanned for their maximum in LDS by the thread that owns the row (same order of
// additions as groupsBuildKernel: the results are bit-identical), then the tile leaves in one coalesced write —
// one HBM write per matrix element instead of zero-fill + read-modify-writes + two normalisation passes.
__global__ __launch_bounds__(256) void groupsBuildTileKernel(
    const uint32_t num_items, const uint32_t * __restrict__ item_matrix, const uint32_t * __restrict__ item_chunk,
    const uint64_t * __restrict__ mat_val_off, const uint64_t * __restrict__ mat_row_off,
    const uint64_t * __restrict__ mat_row0, const uint64_t * __restrict__ mat_rows, const uint32_t * __restrict__ mat_cols,
    const uint64_t * __restrict__ mat_inc_off, const uint64_t * __restrict__ path_grp_off,
    const uint32_t * __restrict__ path_grp, const uint64_t * __restrict__ row_ent_off,
    const uint32_t * __restrict__ ent_path, const double * __restrict__ ent_prob, const double * __restrict__ row_noise,
    const uint32_t * __restrict__ row_perm, const int normalise, double * __restrict__ values, double * __restrict__ rowmax,
    uint64_t * __restrict__ collapse_key, uint32_t * __restrict__ collapse_row, uint64_t * __restrict__ collapse_mask) {  // null: no row collapse
    extern __shared__ double tile[];
    if (blockIdx.x >= num_items) return;
    const uint32_t m = item_matrix[blockIdx.x];
    const uint64_t R = mat_rows[m], r0 = mat_row0[m];
    const uint32_t G = mat_cols[m];
    const uint32_t Rc = tileRows(G);
    const uint64_t i0 = static_cast<uint64_t>(item_chunk[blockIdx.x]) * Rc;
    const uint32_t nrows = static_cast<uint32_t>(min(static_cast<uint64_t>(Rc), R - i0));
    const uint32_t Rs = Rc + 1;  // odd stride: a walk along a row of the tile (second loop below) meets every LDS bank
    const uint32_t cells = G * Rc;
    for (uint32_t idx = threadIdx.x; idx < G * Rs; idx += blockDim.x) tile[idx] = 0.0;
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < nrows) {
        const uint64_t r = r0 + row_perm[mat_row_off[m] + i0 + t];  // matrix row i0 + t = this row of the cluster
        const uint64_t * pgo = path_grp_off + mat_inc_off[m];
        // The row's entries hang on a chain of dependent loads (entry -> path -> its columns' offsets -> column): four
        // entries walk it side by side, the additions stay in entry order.
        const uint64_t e_end = row_ent_off[r + 1];
        for (uint64_t e = row_ent_off[r]; e < e_end; e += 4) {
            uint32_t p[4];
            double v[4];
            uint64_t x_begin[4], x_end[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = e + k < e_end;
                p[k] = in ? ent_path[e + k] : 0u;
                v[k] = in ? ent_prob[e + k] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = e + k < e_end;
                x_begin[k] = in ? pgo[p[k]] : 0;
                x_end[k] = in ? pgo[p[k] + 1] : 0;
            }
            // A path lies in as many columns as haplotype groups carry it — dozens for a common allele — and every column
            // index is a load of its own: the first kAhead of all four entries are fetched before anything is added (32
            // loads in flight), longer lists eight at a time.  The additions keep their order: entry after entry, column
            // after column.
            constexpr int kAhead = 8;
            uint32_t columns[4][kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
#pragma unroll
                for (int k = 0; k < 4; ++k) columns[k][j] = x_begin[k] + j < x_end[k] ? path_grp[x_begin[k] + j] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < kAhead; ++j) {
                    if (x_begin[k] + j < x_end[k]) tile[columns[k][j] * Rs + t] += v[k];
                }
                for (uint64_t x = x_begin[k] + kAhead; x < x_end[k]; x += kAhead) {
                    uint32_t more[kAhead];
#pragma unroll
                    for (int j = 0; j < kAhead; ++j) more[j] = x + j < x_end[k] ? path_grp[x + j] : 0u;
#pragma unroll
                    for (int j = 0; j < kAhead; ++j) {
                        if (x + j < x_end[k]) tile[more[j] * Rs + t] += v[k];
                    }
                }
            }
        }
    }
    // The rows' second half — row sum, normalisation, maximum, sort key, zero pattern — with as many lanes per row as the
    // workgroup has to spare (a tile of 64 columns is 64 rows: four lanes each, neighbours in a wave, every one a quarter of
    // the columns; the owner thread alone spent 8 of the tile's 23 us here, one division and three dependent chains per
    // column).  The row sum keeps its order (column after column, by the row's first lane); the key is a sum of the lanes'
    // partial keys in a fixed order.
    __syncthreads();
    uint32_t parts = 1;
    while (parts < 8 && 2 * parts * Rc <= blockDim.x) parts *= 2;
    const uint32_t row = threadIdx.x / parts, part = threadIdx.x % parts;
    if (row < Rc) {  // (whole groups of `parts` lanes: the shuffles below stay inside them)
        const bool valid = row < nrows;
        const uint64_t r = valid ? r0 + row_perm[mat_row_off[m] + i0 + row] : 0;
        double mx = 0.0;
        if (normalise) {
            double rowsum = 0.0;
            if (valid && part == 0) {
                for (uint32_t g = 0; g < G; ++g) rowsum += tile[g * Rs + row];
            }
            rowsum = __shfl(rowsum, static_cast<int>(threadIdx.x & 63u) - static_cast<int>(part));
            const double noise = valid ? row_noise[r] : 0.0;
            const double keep = 1 - noise;
            double key = part == 0 ? collapseWeight(G) * noise : 0.0;
            uint64_t pattern = 0;
            if (valid) {
                for (uint32_t g = part; g < G; g += parts) {
                    double v = (tile[g * Rs + row] / rowsum) * keep;
                    if (v != v) v = 0.0;  // 0/0 rows -> 0 (src/path_estimator.cpp:162)
                    tile[g * Rs + row] = v;
                    mx = fmax(mx, v);
                    key = fma(collapseWeight(g), v, key);
                    if (g < 64 && v != 0.0) pattern |= 1ull << g;
                }
            }
            for (uint32_t step = 1; step < parts; step *= 2) {
                mx = fmax(mx, __shfl_xor(mx, static_cast<int>(step)));
                key += __shfl_xor(key, static_cast<int>(step));
                pattern |= __shfl_xor(pattern, static_cast<int>(step));
            }
            if (valid && part == 0 && collapse_key) {
                collapse_key[mat_row_off[m] + i0 + row] = collapseSortKey(m, key, mx);
                collapse_row[mat_row_off[m] + i0 + row] = static_cast<uint32_t>(mat_row_off[m] + i0 + row);
                collapse_mask[mat_row_off[m] + i0 + row] = pattern;
            }
        } else {
            if (valid) {
                for (uint32_t g = part; g < G; g += parts) mx = fmax(mx, tile[g * Rs + row]);
            }
            for (uint32_t step = 1; step < parts; step *= 2) mx = fmax(mx, __shfl_xor(mx, static_cast<int>(step)));
        }
        if (valid && part == 0) rowmax[mat_row_off[m] + i0 + row] = mx;
    }
    __syncthreads();
    double * M = values + mat_val_off[m];
    const uint32_t shift = 31 - __clz(Rc);
    for (uint32_t idx = threadIdx.x; idx < cells; idx += blockDim.x) {
        const uint32_t g = idx >> shift, tt = idx & (Rc - 1);
        if (tt < nrows) M[static_cast<uint64_t>(g) * R + i0 + tt] = tile[g * Rs + tt];
    }
}

// ---- path -> groups incidence, inverted on the device ---------------------------------
// The caller gives, per matrix, the paths of every column (group).  The build kernel needs the
// opposite: the columns of every path.  One thread per column counts / scatters; the per-path lists
// come out in arbitrary column order, which does not matter (a row adds each of its entries to every
// column of the entry's path; the order of those columns does not change any sum).

__device__ __forceinline__ uint32_t matrixOfColumn(const uint64_t * __restrict__ group_off, const uint32_t num_matrices,
                                                   const uint64_t column) {
    uint32_t lo = 0, hi = num_matrices - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (group_off[mid] <= column) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void incidenceCountKernel(const uint32_t num_matrices, const uint64_t num_columns,
                                     const uint64_t * __restrict__ group_off, const uint64_t * __restrict__ group_path_off,
                                     const uint32_t * __restrict__ group_path, const uint64_t * __restrict__ inc_off,
                                     const uint64_t * __restrict__ num_paths, uint32_t * __restrict__ degree,
                                     uint32_t * __restrict__ error_flag) {
    const uint64_t column = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (column >= num_columns) return;
    const uint32_t m = matrixOfColumn(group_off, num_matrices, column);
    for (uint64_t x = group_path_off[column]; x < group_path_off[column + 1]; ++x) {
        const uint32_t p = group_path[x];
        if (p >= num_paths[m]) {
            *error_flag = 1;
            continue;
        }
        atomicAdd(&degree[inc_off[m] + p], 1u);
    }
}

__global__ void incidenceFillKernel(const uint32_t num_matrices, const uint64_t num_columns,
                                    const uint64_t * __restrict__ group_off, const uint64_t * __restrict__ group_path_off,
                                    const uint32_t * __restrict__ group_path, const uint64_t * __restrict__ inc_off,
                                    const uint64_t * __restrict__ num_paths, const uint64_t * __restrict__ path_grp_off,
                                    uint32_t * __restrict__ cursor, uint32_t * __restrict__ path_grp) {
    const uint64_t column = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (column >= num_columns) return;
    const uint32_t m = matrixOfColumn(group_off, num_matrices, column);
    const uint32_t local = static_cast<uint32_t>(column - group_off[m]);
    for (uint64_t x = group_path_off[column]; x < group_path_off[column + 1]; ++x) {
        const uint32_t p = group_path[x];
        if (p >= num_paths[m]) continue;
        const uint64_t slot = inc_off[m] + p;
        path_grp[path_grp_off[slot] + atomicAdd(&cursor[slot], 1u)] = local;
    }
}

// ---- the same matrices from the columns' path sets as bit masks (round 4) -----------------------------------------------
//
// groupsBuildTileKernel walks, for every entry of a row, a chain of dependent loads (entry -> path -> the path's list of
// columns -> column) and adds into an LDS tile that holds 64 rows of 64 columns: a wave of the workgroup's four works, four
// workgroups fit a CU, and 23 us per tile is what the chain takes (0.95 ms per configs[2] batch, a third of the HBM time of
// the 1.5 GB it writes).  The incidence the other way round needs no lists: a column IS a set of paths, and a cluster has tens
// of paths — one or a few 64-bit words per column.  A lane owns a row, a wave a quarter of (up to 64) columns: the lane loads
// its row's entries once and, for each of its columns, adds the probabilities of the entries whose path is in the column's
// set, entry after entry (the additions of groupsBuildKernel in the same order: bit-identical values).  No tile: the values
// stay in registers until they leave, 64 consecutive rows of a column per store.  Row sum, normalisation, largest value,
// sort key and zero pattern as before (the sum over the columns in ascending order, handed from wave to wave).

// one thread per column: the set of its paths
__global__ void columnMaskKernel(const uint32_t num_matrices, const uint64_t num_columns, const uint64_t * __restrict__ group_off,
                                 const uint64_t * __restrict__ group_path_off, const uint32_t * __restrict__ group_path,
                                 const uint64_t * __restrict__ num_paths, const uint64_t * __restrict__ mask_off, uint64_t * __restrict__ masks,
                                 uint32_t * __restrict__ error_flag) {
    const uint64_t column = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (column >= num_columns) return;
    const uint32_t m = matrixOfColumn(group_off, num_matrices, column);
    if (mask_off[m] == ~0ull) return;  // (a matrix of the other kernels)
    const uint32_t words = static_cast<uint32_t>((num_paths[m] + 63) / 64);
    uint64_t * const out = masks + mask_off[m] + (column - group_off[m]) * words;
    for (uint32_t k = 0; k < words; ++k) out[k] = 0;
    for (uint64_t x = group_path_off[column]; x < group_path_off[column + 1]; ++x) {
        const uint32_t p = group_path[x];
        if (p >= num_paths[m]) {
            *error_flag = 1;
            continue;
        }
        const uint64_t bit = 1ull << (p & 63u);
        if (out[p >> 6] & bit) *error_flag = 2;  // (the lists of the other kernels would add such a path twice)
        out[p >> 6] |= bit;
    }
}

struct MaskBuildArgs {
    uint32_t num_items;
    const uint32_t * item_matrix;
    const uint32_t * item_chunk;
    const uint64_t * mat_val_off;
    const uint64_t * mat_row_off;
    const uint64_t * mat_row0;
    const uint64_t * mat_rows;
    const uint32_t * mat_cols;
    const uint64_t * num_paths;
    const uint64_t * mask_off;
    const uint64_t * masks;
    const uint64_t * row_ent_off;
    const uint32_t * ent_path;
    const double * ent_prob;
    const double * row_noise;
    const uint32_t * row_perm;
    int normalise;
#ifdef RPVG_HIP_EXPERIMENTS
    int debug_no_long_rows;    // timing experiment (RPVG_HIP_BUILD_DEBUG=1): entries past the held ones are dropped
#endif
    double * values;
    double * rowmax;
    uint64_t * collapse_key;   // null: no row collapse
    uint32_t * collapse_row;
    uint64_t * collapse_mask;
};

// A wave per (matrix, 64 rows) item, a lane per row, and nothing shared between lanes: the lane walks the columns of its row
// twice — once for the row sum (column after column: the order of the other kernels), once more for the values, which it
// computes again rather than keeping them (a cell is a handful of bit tests and additions; a tile of 64 x 64 values in LDS was
// what limited a CU to four workgroups, and the kernel's time went with the workgroups a CU held: 0.97 ms with four, 1.31 with
// three, 2.35 with two — latency of its loads and of its short dependent loops, not bandwidth).  No LDS, no barrier; the set of
// a column is the same word for every lane (a scalar load).
constexpr int kMaskHeld = 8;   // entries of a row in registers (3.3 a row on the configs[2] batch), in two halves

__global__ __launch_bounds__(256) void groupsBuildMaskKernel(const MaskBuildArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (item >= a.num_items) return;
    const uint32_t m = a.item_matrix[item];
    const uint64_t R = a.mat_rows[m], r0 = a.mat_row0[m], row_off = a.mat_row_off[m];
    const uint32_t G = a.mat_cols[m];
    const uint32_t words = static_cast<uint32_t>((a.num_paths[m] + 63) / 64);
    const uint64_t * const sets = a.masks + a.mask_off[m];
    double * const M = a.values + a.mat_val_off[m];
    const uint64_t i = static_cast<uint64_t>(a.item_chunk[item]) * kMaskRows + lane;
    const bool valid = i < R;
    const uint64_t r = valid ? r0 + a.row_perm[row_off + i] : 0;
    const uint64_t e_begin = valid ? a.row_ent_off[r] : 0, e_end = valid ? a.row_ent_off[r + 1] : 0;
    const double noise = valid && a.normalise ? a.row_noise[r] : 0.0;
    uint32_t p[kMaskHeld];
    double v[kMaskHeld];
#pragma unroll
    for (int k = 0; k < kMaskHeld; ++k) {
        p[k] = 0u;
        v[k] = 0.0;  // (an entry past the row's last adds + 0.0: nothing)
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (e_begin + k < e_end) {
            p[k] = a.ent_path[e_begin + k];
            v[k] = a.ent_prob[e_begin + k];
        }
    }
    const bool second_half = __ballot(e_begin + 4 < e_end) != 0ull;  // (of the wave: the same for every lane)
    if (second_half) {
#pragma unroll
        for (int k = 4; k < kMaskHeld; ++k) {
            if (e_begin + k < e_end) {
                p[k] = a.ent_path[e_begin + k];
                v[k] = a.ent_prob[e_begin + k];
            }
        }
    }
#ifdef RPVG_HIP_EXPERIMENTS
    const bool longer = !a.debug_no_long_rows && __ballot(e_begin + kMaskHeld < e_end) != 0ull;
#else
    const bool longer = __ballot(e_begin + kMaskHeld < e_end) != 0ull;
#endif

    // the row's value in column c: the probabilities of its entries whose path is in the column's set, entry after entry
    auto cell = [&](const uint32_t c) {
        double sum = 0.0;
        if (words == 1) {
            const uint64_t set = sets[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) sum += ((set >> (p[k] & 63u)) & 1ull) ? v[k] : 0.0;
            if (second_half) {
#pragma unroll
                for (int k = 4; k < kMaskHeld; ++k) sum += ((set >> (p[k] & 63u)) & 1ull) ? v[k] : 0.0;
            }
            if (longer) {
                for (uint64_t e = e_begin + kMaskHeld; e < e_end; ++e) sum += ((set >> (a.ent_path[e] & 63u)) & 1ull) ? a.ent_prob[e] : 0.0;
            }
        } else {
            const uint64_t * const set = sets + static_cast<size_t>(c) * words;
#pragma unroll
            for (int k = 0; k < 4; ++k) sum += ((set[p[k] >> 6] >> (p[k] & 63u)) & 1ull) ? v[k] : 0.0;
            if (second_half) {
#pragma unroll
                for (int k = 4; k < kMaskHeld; ++k) sum += ((set[p[k] >> 6] >> (p[k] & 63u)) & 1ull) ? v[k] : 0.0;
            }
            if (longer) {
                for (uint64_t e = e_begin + kMaskHeld; e < e_end; ++e) {
                    const uint32_t path = a.ent_path[e];
                    sum += ((set[path >> 6] >> (path & 63u)) & 1ull) ? a.ent_prob[e] : 0.0;
                }
            }
        }
        return sum;
    };

    double rowsum = 0.0;
    if (a.normalise) {
#pragma unroll 4
        for (uint32_t c = 0; c < G; ++c) rowsum += cell(c);
    }
    const double keep = 1 - noise;
    double key = collapseWeight(G) * noise, mx = 0.0;
    uint64_t pattern = 0;
#pragma unroll 4
    for (uint32_t c = 0; c < G; ++c) {
        double value = cell(c);
        if (a.normalise) {
            value = (value / rowsum) * keep;
            if (value != value) value = 0.0;  // 0/0 rows -> 0 (src/path_estimator.cpp:162)
            key = fma(collapseWeight(c), value, key);
            if (c < 64 && value != 0.0) pattern |= 1ull << c;
        }
        mx = fmax(mx, value);
        if (valid) M[static_cast<uint64_t>(c) * R + i] = value;
    }
    if (valid) {
        a.rowmax[row_off + i] = mx;
        if (a.normalise && a.collapse_key) {
            a.collapse_key[row_off + i] = collapseSortKey(m, key, mx);
            a.collapse_row[row_off + i] = static_cast<uint32_t>(row_off + i);
            a.collapse_mask[row_off + i] = pattern;
        }
    }
}

// ---- every column one path of its own, values as they are (rpvg_hip_groups_build_single_paths without normalisation: the raw path
// posteriors of configs[4]) ------------------------------------------------------------------------------------------------------
// The general kernels ask, cell by cell, which entries of the row lie in the column's set: columns x entries bit tests per row, for
// matrices of up to thousands of columns (groupsBuildMaskKernel: 5.1 ms per lane of a configs[4] batch, a sixth of the batch's kernel
// time).  Here a cell is an entry or nothing: the lane zeroes its row column after column (the lanes of a wave write 64 neighbouring
// doubles of a column) and stores its entries where they belong — the same values, the same row maxima.  A wave per (matrix, 64 rows).
__global__ __launch_bounds__(256) void groupsBuildSinglePathKernel(const MaskBuildArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (item >= a.num_items) return;
    const uint32_t m = a.item_matrix[item];
    const uint64_t R = a.mat_rows[m], r0 = a.mat_row0[m], row_off = a.mat_row_off[m];
    const uint32_t G = a.mat_cols[m];
    double * const M = a.values + a.mat_val_off[m];
    const uint64_t i = static_cast<uint64_t>(a.item_chunk[item]) * kMaskRows + lane;
    if (i >= R) return;
    const uint64_t r = r0 + a.row_perm[row_off + i];
    for (uint32_t c = 0; c < G; ++c) M[static_cast<uint64_t>(c) * R + i] = 0.0;
    double mx = 0.0;
    for (uint64_t e = a.row_ent_off[r]; e < a.row_ent_off[r + 1]; ++e) {  // (behind the zeros of the same lane)
        const double value = a.ent_prob[e];
        M[static_cast<uint64_t>(a.ent_path[e]) * R + i] = value;
        mx = fmax(mx, value);
    }
    a.rowmax[row_off + i] = mx;
}

// ---- matrices of up to 64 columns: the columns of a path as ONE word (round 5) ---------------------------------------------
//
// With several batches in flight the GPU is busy throughout, and groupsBuildMaskKernel is a quarter of what its SIMDs issue per
// configs[2] batch: a cell costs a test of every held entry of the row against the column's set — twice, once for the row sum and
// once for the value —, four or eight entries whatever the row has, and a set is a load per cell.  The matrices of that batch
// have up to 64 columns (99 % of its cells), few enough for the incidence the other way round to be a word per PATH: the columns
// that contain it.  A lane (= a row) then takes its entries one after the other — as many as the wave's longest row has — and
// adds each entry's probability to the cells whose bit is set in the entry's word, all 64 cells in registers: a bit field
// extract, two ANDs and an addition per entry and cell (the additions of a cell are those of the other kernels in the same
// order: entry after entry; an entry outside the column adds + 0.0), no load after the entries', and the cells are still there
// when the row sum is known.
constexpr int kWordHeld = 4;   // entries loaded ahead of the loop (3.3 a row on the configs[2] batch; the wave's longest row: 4.4)

// one thread per column: its bit into the word of every path it contains (words zeroed before)
__global__ void pathColumnWordKernel(const uint32_t num_matrices, const uint64_t num_columns, const uint64_t * __restrict__ group_off,
                                     const uint64_t * __restrict__ group_path_off, const uint32_t * __restrict__ group_path,
                                     const uint64_t * __restrict__ num_paths, const uint64_t * __restrict__ word_off,
                                     unsigned long long * __restrict__ words, uint32_t * __restrict__ error_flag) {
    const uint64_t column = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (column >= num_columns) return;
    const uint32_t m = matrixOfColumn(group_off, num_matrices, column);
    if (word_off[m] == ~0ull) return;  // (a matrix of the other kernels)
    const unsigned long long bit = 1ull << (column - group_off[m]);
    for (uint64_t x = group_path_off[column]; x < group_path_off[column + 1]; ++x) {
        const uint32_t p = group_path[x];
        if (p >= num_paths[m]) {
            *error_flag = 1;
            continue;
        }
        if (atomicOr(&words[word_off[m] + p], bit) & bit) *error_flag = 2;  // (the lists of the other kernels would add such a path twice)
    }
}

// cells[c] += the entry's probability where bit c of its word is set
__device__ __forceinline__ void addEntryToCells(double (&cells)[kWordMaxColumns], const uint32_t blocks, const uint64_t word, const double prob) {
    const int lo = static_cast<int>(static_cast<uint32_t>(word)), hi = static_cast<int>(static_cast<uint32_t>(word >> 32));
    const int prob_lo = __double2loint(prob), prob_hi = __double2hiint(prob);
#pragma unroll
    for (uint32_t b = 0; b < kWordMaxColumns / 8; ++b) {
        if (b < blocks) {  // (of the wave; a column past the matrix's last has no bit anywhere)
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t c = 8 * b + j;
                const int all = __builtin_amdgcn_sbfe(c < 32 ? lo : hi, c & 31u, 1);  // 0 or ~0
                cells[c] += __hiloint2double(prob_hi & all, prob_lo & all);
            }
        }
    }
}

// A wave per (matrix, 64 rows) item, a lane per row, as groupsBuildMaskKernel; MaskBuildArgs with `masks` = the words of the
// paths and `mask_off` = the first word of a matrix.
__global__ __launch_bounds__(256) void groupsBuildWordKernel(const MaskBuildArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (item >= a.num_items) return;
    const uint32_t m = a.item_matrix[item];
    const uint64_t R = a.mat_rows[m], r0 = a.mat_row0[m], row_off = a.mat_row_off[m];
    const uint32_t G = a.mat_cols[m], blocks = (G + 7) / 8;
    const uint64_t * const words = a.masks + a.mask_off[m];
    double * const M = a.values + a.mat_val_off[m];
    const uint64_t i = static_cast<uint64_t>(a.item_chunk[item]) * kMaskRows + lane;
    const bool valid = i < R;
    const uint64_t r = valid ? r0 + a.row_perm[row_off + i] : 0;
    const uint64_t e_begin = valid ? a.row_ent_off[r] : 0, e_end = valid ? a.row_ent_off[r + 1] : 0;
    const double noise = valid && a.normalise ? a.row_noise[r] : 0.0;
    const uint32_t n = static_cast<uint32_t>(e_end - e_begin);
    uint32_t longest = n;
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
        const uint32_t other = __shfl_xor(longest, offset);
        longest = other > longest ? other : longest;
    }
    longest = __builtin_amdgcn_readfirstlane(longest);

    uint64_t word[kWordHeld];
    double prob[kWordHeld];
    bool tiny_entry = false;  // a non-zero entry below 2^-400 (or not a number): see the quotients below
#pragma unroll
    for (int k = 0; k < kWordHeld; ++k) {
        word[k] = 0;   // (an entry past the row's last: no column)
        prob[k] = 0.0;
        if (static_cast<uint32_t>(k) < n) {
            word[k] = words[a.ent_path[e_begin + k]];
            prob[k] = a.ent_prob[e_begin + k];
            tiny_entry |= !(prob[k] == 0.0 || prob[k] >= 0x1p-400);
        }
    }
    double cells[kWordMaxColumns];
#pragma unroll
    for (uint32_t c = 0; c < kWordMaxColumns; ++c) cells[c] = 0.0;
#pragma unroll
    for (int k = 0; k < kWordHeld; ++k) {
        if (static_cast<uint32_t>(k) < longest) addEntryToCells(cells, blocks, word[k], prob[k]);
    }
    for (uint32_t k = kWordHeld; k < longest; ++k) {
        uint64_t w = 0;
        double v = 0.0;
        if (k < n) {
            w = words[a.ent_path[e_begin + k]];
            v = a.ent_prob[e_begin + k];
            tiny_entry |= !(v == 0.0 || v >= 0x1p-400);
        }
        addEntryToCells(cells, blocks, w, v);
    }

    double rowsum = 0.0;
    if (a.normalise) {
#pragma unroll
        for (uint32_t b = 0; b < kWordMaxColumns / 8; ++b) {
            if (b < blocks) {
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) rowsum += cells[8 * b + j];  // (in column order; a column past the last adds + 0.0)
            }
        }
    }
    // The quotients cell / rowsum.  The division the compiler emits is eleven instructions a cell, six of them on the
    // denominator alone: its reciprocal (v_rcp_f64, two Newton steps) — once per row here —, then quotient = cell x reciprocal,
    // remainder = cell - rowsum x quotient, quotient + remainder x reciprocal: the hardware's own sequence, which differs from
    // this one by the scaling of operands near the ends of the exponent range (v_div_scale / v_div_fmas) and the special cases
    // of v_div_fixup.  Neither arises while the row sum lies in [2^-400, 2^400] and every non-zero cell is at least 2^-400 (a
    // cell is a sum of the row's non-negative entries: at least its smallest non-zero one, at most the row sum): such waves —
    // all of them, in practice — take the three instructions, the others the division.  0 / rowsum is 0 either way, and a row
    // sum of 0 (all cells 0) gives not-a-number, hence 0, either way.
    const double keep = 1 - noise;
    constexpr double kSmall = 0x1p-400, kLarge = 0x1p400;
    const bool plain = __ballot(valid && a.normalise && (!(rowsum == 0.0 || (rowsum >= kSmall && rowsum <= kLarge)) || tiny_entry)) == 0ull;
    double reciprocal = 0.0;
    if (plain) {
        reciprocal = __builtin_amdgcn_rcp(rowsum);
        reciprocal = fma(reciprocal, fma(-rowsum, reciprocal, 1.0), reciprocal);
        reciprocal = fma(reciprocal, fma(-rowsum, reciprocal, 1.0), reciprocal);
    }
    double key = collapseWeight(G) * noise, mx = 0.0;
    uint32_t pattern_lo = 0, pattern_hi = 0;
    double * out = M + i;
    // eight columns at a time: without a branch between them their quotients overlap
    auto columns = [&](const uint32_t b, auto all_eight, auto plain_division) {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t c = 8 * b + j;
            if (decltype(all_eight)::value || c < G) {
                double value = cells[c];
                if (a.normalise) {
                    if (decltype(plain_division)::value) {
                        const double quotient = value * reciprocal;
                        value = fma(fma(-rowsum, quotient, value), reciprocal, quotient);
                    } else {
                        value = value / rowsum;
                    }
                    value *= keep;
                    if (value != value) value = 0.0;  // 0/0 rows -> 0 (src/path_estimator.cpp:162)
                    key = fma(collapseWeight(c), value, key);
                    if (c < 32) pattern_lo |= value != 0.0 ? 1u << (c & 31u) : 0u;
                    else pattern_hi |= value != 0.0 ? 1u << (c & 31u) : 0u;
                }
                asm("v_max_f64 %0, %1, %2" : "=v"(mx) : "v"(mx), "v"(value));  // (no NaN here: fmax() would quiet both operands first)
                if (valid) out[static_cast<uint64_t>(j) * R] = value;
            }
        }
        out += 8 * R;
    };
#pragma unroll
    for (uint32_t b = 0; b < kWordMaxColumns / 8; ++b) {
        if (8 * b + 8 <= G) {
            if (plain) columns(b, std::true_type(), std::true_type()); else columns(b, std::true_type(), std::false_type());
        } else if (8 * b < G) {
            if (plain) columns(b, std::false_type(), std::true_type()); else columns(b, std::false_type(), std::false_type());
        }
    }
    if (valid) {
        a.rowmax[row_off + i] = mx;
        if (a.normalise && a.collapse_key) {
            a.collapse_key[row_off + i] = collapseSortKey(m, key, mx);
            a.collapse_row[row_off + i] = static_cast<uint32_t>(row_off + i);
            a.collapse_mask[row_off + i] = (static_cast<uint64_t>(pattern_hi) << 32) | pattern_lo;
        }
    }
}

// storage of the matrices groupsBuildKernel accumulates in global memory: one work item = 256 rows of one matrix
__global__ __launch_bounds__(256) void zeroWideMatricesKernel(const uint32_t * __restrict__ item_matrix, const uint32_t * __restrict__ item_chunk,
                                                              const uint64_t * __restrict__ mat_val_off, const uint64_t * __restrict__ mat_rows,
                                                              const uint32_t * __restrict__ mat_cols, double * __restrict__ values) {
    const uint32_t m = item_matrix[blockIdx.x];
    const uint64_t R = mat_rows[m];
    const uint64_t row = static_cast<uint64_t>(item_chunk[blockIdx.x]) * 256 + threadIdx.x;
    if (row >= R) return;
    double * M = values + mat_val_off[m];
    const uint32_t G = mat_cols[m];
    for (uint32_t g = 0; g < G; ++g) M[static_cast<uint64_t>(g) * R + row] = 0.0;
}

}  // namespace

// The haplotype columns of the batch (path_sources.hip: laid out by bounds, per cluster) for the clusters of a build, as the
// compact lists the build kernels take.  One workgroup per matrix.
__global__ __launch_bounds__(256) void gatherSourceColumnsKernel(const uint32_t num_matrices, const uint32_t * __restrict__ cluster,
                                                                 const uint64_t * __restrict__ cluster_src_off, const uint32_t * __restrict__ src_col_count,
                                                                 const uint32_t * __restrict__ src_col_end, const uint32_t * __restrict__ src_col_path,
                                                                 const uint64_t * __restrict__ group_off, const uint64_t * __restrict__ first_path,
                                                                 uint64_t * __restrict__ group_path_off, uint32_t * __restrict__ group_path,
                                                                 uint32_t * __restrict__ column_counts) {
    const uint32_t m = blockIdx.x;
    if (m >= num_matrices) return;
    const uint64_t slot0 = cluster_src_off[cluster[m]];
    const uint64_t g0 = group_off[m], p0 = first_path[m];
    const uint32_t G = static_cast<uint32_t>(group_off[m + 1] - g0), L = static_cast<uint32_t>(first_path[m + 1] - p0);
    if (threadIdx.x == 0 && m == 0) group_path_off[0] = 0;
    for (uint32_t c = threadIdx.x; c < G; c += 256) {
        group_path_off[g0 + c + 1] = p0 + src_col_end[slot0 + c];
        column_counts[g0 + c] = src_col_count[slot0 + c];
    }
    for (uint32_t x = threadIdx.x; x < L; x += 256) group_path[p0 + x] = src_col_path[slot0 + x];
}

// column c of a matrix = path c of its cluster, alone (rpvg_hip_groups_build_single_paths)
__global__ __launch_bounds__(256) void singlePathColumnsKernel(const uint32_t num_matrices, const uint64_t * __restrict__ group_off,
                                                               uint64_t * __restrict__ group_path_off, uint32_t * __restrict__ group_path) {
    const uint32_t m = blockIdx.x;
    if (m >= num_matrices) return;
    const uint64_t g0 = group_off[m];
    const uint32_t G = static_cast<uint32_t>(group_off[m + 1] - g0);
    if (threadIdx.x == 0 && m == 0) group_path_off[0] = 0;
    for (uint32_t c = threadIdx.x; c < G; c += 256) {
        group_path_off[g0 + c + 1] = g0 + c + 1;
        group_path[g0 + c] = c;
    }
}

// ---- the host side: the plan (group_build_plan.hpp), uploaded and queued stage by stage -------------------------------------------------
namespace {

struct ItemBuffers {
    DeviceBuffer<uint32_t> matrix, chunk;
};

// temporaries: owned by the matrices object (the kernels that use them may still be queued on return)
struct BuildTemporaries {
    DeviceBuffer<uint64_t> inc_off, path_grp_off, group_off, group_path_off, num_paths;
    DeviceBuffer<uint32_t> path_grp, group_path, degree, cursor, cluster;
    ItemBuffers list_items, tile_items, mask_items, word_items;
    DeviceBuffer<uint64_t> mask_off, masks, first_path, word_off, path_words;
    DeviceBuffer<uint32_t> column_counts;
    DeviceBuffer<unsigned char> scan_tmp;
};

// what the stages of one build share
struct BuildState {
    rpvg_hip_ctx * ctx;
    const rpvg_hip_batch * batch;
    const rpvg_hip_group_spec * spec;
    Columns kind;
    bool collapse;
    const GroupBuildPlan & plan;
    rpvg_hip_groups * g;
    BuildTemporaries & tmp;
    hipStream_t st;
    hipError_t e;           // the first error
    size_t scan_bytes = 0;  // temporary storage of the scan over the paths' degrees
    bool ok(const hipError_t r) {
        if (e == hipSuccess) e = r;
        return e == hipSuccess;
    }
};

// Which kernel builds a matrix may be switched: RPVG_HIP_BUILD_MASKS=1: no word kernel, =0: the list kernels for everything (the
// three produce the identical values: switches for the tests and for A/B timing — 0.84 (masks) against 1.05 ms (lists) per
// configs[2] batch standing alone, but 9.71 against 9.65 ms per batch in round 4's two-lane bench: the list kernels wait, and the
// other lane's kernels run meanwhile; with batches in flight the GPU has no such gaps).  RPVG_HIP_NO_DIRECT_BUILD=1: the general
// kernels for single-path columns as they are too (test_single_path_matrices_equal_… compares the direct kernel — the implied
// build — with the general ones — the same columns listed).  Read per call.
BuildKnobs readBuildKnobs() {
    BuildKnobs knobs;
    const char * masks_env = std::getenv("RPVG_HIP_BUILD_MASKS");
    knobs.masks = masks_env ? std::atoi(masks_env) != 0 : true;
    knobs.words = masks_env ? std::atoi(masks_env) >= 2 : true;
    knobs.direct = !std::getenv("RPVG_HIP_NO_DIRECT_BUILD");
    return knobs;
}

// one block, one copy for the host arrays (UploadPack); the zero-initialised counters ride behind them (one memset)
void uploadPlan(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    const uint32_t M = p.M;
    rpvg_hip_groups * g = s.g;
    BuildTemporaries & t = s.tmp;
    UploadPack & pack = g->uploads;
    const auto addItems = [&pack](ItemBuffers & to, const Items & from) {
        pack.add(to.matrix, from.matrix.data(), from.size());
        pack.add(to.chunk, from.chunk.data(), from.size());
    };
    pack.add(g->mat_val_off, p.val_off.data(), M);
    pack.add(g->mat_row_off, p.row_off.data(), M);
    pack.add(g->mat_row0, p.row0.data(), M);
    pack.add(g->mat_rows, p.rows.data(), M);
    pack.add(g->mat_cols, p.cols.data(), M);
    pack.add(t.inc_off, p.inc_off.data(), M);
    pack.add(t.num_paths, p.num_paths.data(), M);
    pack.add(t.group_off, s.spec->group_off, M + 1);
    if (s.kind == Columns::Sources) {
        pack.add(t.first_path, s.spec->group_path_off, M + 1);
    } else if (s.kind == Columns::Lists) {  // (single paths: the lists are written on the device)
        pack.add(t.group_path_off, s.spec->group_path_off, p.num_columns + 1);
        pack.add(t.group_path, s.spec->group_path, p.num_incidences);
    }
    if (!p.list_items.empty()) addItems(t.list_items, p.list_items);
    if (!p.tile_items.empty()) addItems(t.tile_items, p.tile_items);
    if (!p.mask_items.empty()) {
        addItems(t.mask_items, p.mask_items);
        pack.add(t.mask_off, p.mask_off.data(), M);
    }
    if (!p.word_items.empty()) {
        addItems(t.word_items, p.word_items);
        pack.add(t.word_off, p.word_off.data(), M);
        pack.addZero(t.path_words, p.word_total);
    }
    pack.add(t.cluster, s.spec->cluster, M);
    if (p.lists_needed) {
        pack.addZero(t.degree, p.inc_total);
        pack.addZero(t.cursor, p.inc_total);
    }
    pack.addZero(g->build_error_flag, 1);
    s.ok(pack.commit(s.st));
}

// the columns that are not the caller's stay on the device: gathered from the batch's, or written path by path
void queueDeviceColumns(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    rpvg_hip_groups * g = s.g;
    BuildTemporaries & t = s.tmp;
    if (s.kind != Columns::Lists) {
        s.ok(t.group_path_off.alloc(p.num_columns + 1));
        s.ok(t.group_path.alloc(p.num_incidences));
    }
    if (s.kind == Columns::Sources) {
        s.ok(t.column_counts.alloc(p.num_columns));
        if (s.e == hipSuccess) {
            gatherSourceColumnsKernel<<<dim3(p.gather_columns.grid), dim3(p.gather_columns.block), 0, s.st>>>(
                p.M, t.cluster.ptr, s.batch->cluster_src_off.ptr, s.batch->src_col_count.ptr, s.batch->src_col_end.ptr, s.batch->src_col_path.ptr,
                t.group_off.ptr, t.first_path.ptr, t.group_path_off.ptr, t.group_path.ptr, t.column_counts.ptr);
            s.ok(hipGetLastError());
        }
        g->d_column_counts = t.column_counts.ptr;
    }
    if (s.kind == Columns::SinglePaths && s.e == hipSuccess) {
        singlePathColumnsKernel<<<dim3(p.single_path_columns.grid), dim3(p.single_path_columns.block), 0, s.st>>>(
            p.M, t.group_off.ptr, t.group_path_off.ptr, t.group_path.ptr);
        s.ok(hipGetLastError());
    }
    g->d_group_off = t.group_off.ptr;
    g->d_group_path_off = t.group_path_off.ptr;
    g->d_group_path = t.group_path.ptr;
    g->d_cluster = t.cluster.ptr;
}

void allocate(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    rpvg_hip_groups * g = s.g;
    BuildTemporaries & t = s.tmp;
    s.ok(g->values.alloc(p.val_total + 2));
    s.ok(g->rowmax.alloc(p.row_total));
    s.ok(g->row_perm.alloc(p.row_total));
    s.ok(g->row_count.alloc(p.row_total + 2));
    s.ok(g->row_noise.alloc(p.row_total + 2));
    s.ok(g->mat_fast.alloc(p.M));
    s.ok(g->mat_mid.alloc(p.M));
    if (s.collapse) {
        s.ok(g->collapse_key.alloc(p.row_total));
        s.ok(g->collapse_row.alloc(p.row_total));
        s.ok(g->collapse_mask.alloc(p.row_total));
    }
    if (p.lists_needed) {
        s.ok(t.path_grp_off.alloc(p.inc_total));
        s.ok(t.path_grp.alloc(p.num_incidences));
        if (s.e == hipSuccess) {
            s.ok(hipcub::DeviceScan::ExclusiveSum(nullptr, s.scan_bytes, t.degree.ptr, t.path_grp_off.ptr, static_cast<int>(p.inc_total), s.st));
        }
        s.ok(t.scan_tmp.alloc(s.scan_bytes));
        if (s.e == hipSuccess && p.inc_total > 0x7fffffffull) s.e = hipErrorInvalidValue;
    }
    if (!p.mask_items.empty()) s.ok(t.masks.alloc(p.mask_total));
}

// the storage of the matrices of the global-memory kernel, ahead of everything else
void queueZeroWide(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    if (p.zero_wide.grid == 0) return;
    // (a hipMemsetAsync per wide matrix was up to four fill kernels each: 370 commands per lane on the configs[4] batch)
    zeroWideMatricesKernel<<<dim3(p.zero_wide.grid), dim3(p.zero_wide.block), 0, s.st>>>(
        s.tmp.list_items.matrix.ptr, s.tmp.list_items.chunk.ptr, s.g->mat_val_off.ptr, s.g->mat_rows.ptr, s.g->mat_cols.ptr, s.g->values.ptr);
}

void queuePartition(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    rpvg_hip_groups * g = s.g;
    partitionRowsKernel<kPartitionThreads><<<dim3(p.partition.grid), dim3(p.partition.block), 0, s.st>>>(
        p.M, g->mat_row_off.ptr, g->mat_row0.ptr, g->mat_rows.ptr, s.batch->row_count.ptr, s.batch->row_noise.ptr, g->row_perm.ptr, g->row_count.ptr,
        g->row_noise.ptr, g->mat_fast.ptr, g->mat_mid.ptr, kMidMinRows);
}

// the arguments of the kernels that take a wave per item: the items of the route and, where it has them, its sets (the masks of
// the columns, or the words of the paths) with the first of every matrix
MaskBuildArgs waveKernelArgs(const BuildState & s, const ItemBuffers & items, const uint64_t * set_off, const uint64_t * sets) {
    const rpvg_hip_groups * g = s.g;
    MaskBuildArgs a;
    memset(&a, 0, sizeof(a));
    a.num_items = static_cast<uint32_t>(items.matrix.count);
    a.item_matrix = items.matrix.ptr;
    a.item_chunk = items.chunk.ptr;
    a.mat_val_off = g->mat_val_off.ptr;
    a.mat_row_off = g->mat_row_off.ptr;
    a.mat_row0 = g->mat_row0.ptr;
    a.mat_rows = g->mat_rows.ptr;
    a.mat_cols = g->mat_cols.ptr;
    a.num_paths = s.tmp.num_paths.ptr;
    a.mask_off = set_off;
    a.masks = sets;
    a.row_ent_off = s.batch->row_ent_off.ptr;
    a.ent_path = s.batch->ent_path.ptr;
    a.ent_prob = s.batch->ent_prob.ptr;
    a.row_noise = s.batch->row_noise.ptr;
    a.row_perm = g->row_perm.ptr;
    a.normalise = s.spec->normalise ? 1 : 0;
#ifdef RPVG_HIP_EXPERIMENTS
    a.debug_no_long_rows = RPVG_EXPERIMENT_ENV("RPVG_HIP_BUILD_DEBUG") ? std::atoi(RPVG_EXPERIMENT_ENV("RPVG_HIP_BUILD_DEBUG")) & 1 : 0;
#endif
    a.values = g->values.ptr;
    a.rowmax = g->rowmax.ptr;
    a.collapse_key = g->collapse_key.ptr;
    a.collapse_row = g->collapse_row.ptr;
    a.collapse_mask = g->collapse_mask.ptr;
    return a;
}

// single-path columns, values as they are: one kernel for every width, on the items of the mask route and no masks
void queueDirectRoute(BuildState & s) {
    const Launch & l = s.plan.build_single_paths;
    if (l.grid == 0) return;
    groupsBuildSinglePathKernel<<<dim3(l.grid), dim3(l.block), 0, s.st>>>(waveKernelArgs(s, s.tmp.mask_items, nullptr, nullptr));
}

void queueMaskRoute(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    BuildTemporaries & t = s.tmp;
    if (p.build_masks.grid == 0) return;
    columnMaskKernel<<<dim3(p.column_masks.grid), dim3(p.column_masks.block), 0, s.st>>>(
        p.M, p.num_columns, t.group_off.ptr, t.group_path_off.ptr, t.group_path.ptr, t.num_paths.ptr, t.mask_off.ptr, t.masks.ptr,
        s.g->build_error_flag.ptr);
    groupsBuildMaskKernel<<<dim3(p.build_masks.grid), dim3(p.build_masks.block), 0, s.st>>>(waveKernelArgs(s, t.mask_items, t.mask_off.ptr, t.masks.ptr));
}

void queueWordRoute(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    BuildTemporaries & t = s.tmp;
    if (p.build_words.grid == 0) return;
    pathColumnWordKernel<<<dim3(p.path_words.grid), dim3(p.path_words.block), 0, s.st>>>(
        p.M, p.num_columns, t.group_off.ptr, t.group_path_off.ptr, t.group_path.ptr, t.num_paths.ptr, t.word_off.ptr,
        reinterpret_cast<unsigned long long *>(t.path_words.ptr), s.g->build_error_flag.ptr);
    groupsBuildWordKernel<<<dim3(p.build_words.grid), dim3(p.build_words.block), 0, s.st>>>(
        waveKernelArgs(s, t.word_items, t.word_off.ptr, t.path_words.ptr));
}

// the columns of every path, for the list kernels: degrees, their running sum, the lists
void queueIncidenceInversion(BuildState & s) {
    const GroupBuildPlan & p = s.plan;
    BuildTemporaries & t = s.tmp;
    if (!p.lists_needed) return;
    incidenceCountKernel<<<dim3(p.incidence_count.grid), dim3(p.incidence_count.block), 0, s.st>>>(
        p.M, p.num_columns, t.group_off.ptr, t.group_path_off.ptr, t.group_path.ptr, t.inc_off.ptr, t.num_paths.ptr, t.degree.ptr,
        s.g->build_error_flag.ptr);
    s.ok(hipcub::DeviceScan::ExclusiveSum(t.scan_tmp.ptr, s.scan_bytes, t.degree.ptr, t.path_grp_off.ptr, static_cast<int>(p.inc_total), s.st));
    incidenceFillKernel<<<dim3(p.incidence_fill.grid), dim3(p.incidence_fill.block), 0, s.st>>>(
        p.M, p.num_columns, t.group_off.ptr, t.group_path_off.ptr, t.group_path.ptr, t.inc_off.ptr, t.num_paths.ptr, t.path_grp_off.ptr,
        t.cursor.ptr, t.path_grp.ptr);
}

// the two kernels that read the paths' lists share one signature: through an LDS tile, or in global memory
using ListKernel = decltype(&groupsBuildKernel);
void queueListKernel(BuildState & s, const ListKernel kernel, const Launch & l, const ItemBuffers & items) {
    if (l.grid == 0) return;
    const rpvg_hip_groups * g = s.g;
    const BuildTemporaries & t = s.tmp;
    kernel<<<dim3(l.grid), dim3(l.block), l.lds_bytes, s.st>>>(
        static_cast<uint32_t>(items.matrix.count), items.matrix.ptr, items.chunk.ptr, g->mat_val_off.ptr, g->mat_row_off.ptr, g->mat_row0.ptr,
        g->mat_rows.ptr, g->mat_cols.ptr, t.inc_off.ptr, t.path_grp_off.ptr, t.path_grp.ptr, s.batch->row_ent_off.ptr, s.batch->ent_path.ptr,
        s.batch->ent_prob.ptr, s.batch->row_noise.ptr, g->row_perm.ptr, s.spec->normalise ? 1 : 0, g->values.ptr, g->rowmax.ptr,
        g->collapse_key.ptr, g->collapse_row.ptr, g->collapse_mask.ptr);
}
void queueTileRoute(BuildState & s) { queueListKernel(s, groupsBuildTileKernel, s.plan.build_tiles, s.tmp.tile_items); }
void queueListRoute(BuildState & s) { queueListKernel(s, groupsBuildKernel, s.plan.build_lists, s.tmp.list_items); }

// on the context's collapse stream, behind the build (rpvg_hip_groups::collapse_done)
void queueCollapse(BuildState & s) {
    rpvg_hip_ctx * ctx = s.ctx;
    rpvg_hip_groups * g = s.g;
    hipStream_t collapse_stream = ctx->collapse_stream;
    static const bool same_stream = RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_INLINE") != nullptr;  // A/B knob: on the build's stream (11.5-12.1 vs 10.2-10.4 ms per batch)
    if (same_stream) collapse_stream = s.st;
    s.ok(hipEventCreateWithFlags(&g->built, hipEventDisableTiming));
    s.ok(hipEventCreateWithFlags(&g->collapse_done, hipEventDisableTiming));
    if (s.e == hipSuccess && collapse_stream != s.st) {
        s.ok(hipEventRecord(g->built, s.st));
        s.ok(hipStreamWaitEvent(collapse_stream, g->built, 0));
    }
    const int collapse_span = (s.e == hipSuccess) ? ctx->spanBegin(FAM_COLLAPSE, collapse_stream) : -1;
    // (matrices from the batch's own columns are the diploid search's: it reads them while the collapse finds its runs,
    // rpvg_hip_groups::held_back_runs; RPVG_HIP_COLLAPSE_BEFORE_SEARCH=1: the whole collapse first, as for everybody else)
    const char * before_env = std::getenv("RPVG_HIP_COLLAPSE_BEFORE_SEARCH");  // (read per call: the tests take both ways)
    const bool before_search = before_env != nullptr && std::atoi(before_env) != 0;
    if (s.e == hipSuccess) {
        s.ok(queueRowCollapse(ctx, g, s.plan.row_total, s.spec->collapse_precision, collapse_stream, s.kind == Columns::Sources && !before_search));
    }
    ctx->spanEnd(collapse_span);
    if (s.e == hipSuccess) s.ok(hipEventRecord(g->collapse_done, collapse_stream));
}

int buildGroups(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_group_spec * spec, const Columns kind, rpvg_hip_groups ** groups_out) {
    RPVG_REQUIRE(spec->collapse_precision >= 0 && spec->collapse_precision < 1, "rpvg_hip_groups_build: collapse_precision outside [0, 1)");
    RPVG_REQUIRE(spec->collapse_precision == 0 || spec->normalise,
                 "rpvg_hip_groups_build: the row collapse applies to normalised matrices (src/path_abundance_estimator.cpp:379-380,442-443)");
    static const bool no_collapse = RPVG_EXPERIMENT_ENV("RPVG_HIP_NO_COLLAPSE") != nullptr;  // A/B knob: matrices as built
    const bool collapse = spec->collapse_precision > 0 && !no_collapse;

    std::unique_ptr<rpvg_hip_groups> g(new (std::nothrow) rpvg_hip_groups());
    if (!g) {
        setError("rpvg_hip_groups_build: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    g->batch = batch;
    g->num_matrices = spec->num_matrices;
    g->normalise = spec->normalise;

    std::unique_ptr<HostScope> scope_host(new HostScope("groups_build: host sizes"));
    // host: sizes and offsets only (O(M)); the path -> groups incidence is inverted on the device
    GroupBuildPlan plan = planGroupBuild(batch->h_cluster_row_off.data(), batch->h_cluster_path_off.data(), batch->h_src_max_col_paths.data(),
                                         batch->num_clusters, spec->num_matrices, spec->cluster, spec->group_off, spec->group_path_off,
                                         spec->normalise != 0, collapse, kind, readBuildKnobs());
    if (plan.status != kStatusOk) {
        setError("%s", plan.message.c_str());
        return plan.status;
    }
    g->h_num_cols = plan.cols;
    g->h_num_rows = plan.rows;
    g->h_max_col_paths = std::move(plan.max_col_paths);
    g->h_num_paths = std::move(plan.paths);
    g->h_cluster = std::move(plan.cluster);
    if (plan.M == 0) {
        *groups_out = g.release();
        return RPVG_HIP_OK;
    }

    scope_host.reset();
    HostScope scope_dev("groups_build: upload + kernels + sync");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    std::shared_ptr<BuildTemporaries> tmp = std::make_shared<BuildTemporaries>();
    BuildState s{ctx, batch, spec, kind, collapse, plan, g.get(), *tmp, ctx->stream, hipSetDevice(ctx->device)};
    g->build_temporaries.emplace_back(tmp);
    std::unique_ptr<HostScope> sub(new HostScope("groups_build: uploads"));
    int span = ctx->spanBegin(FAM_H2D);
    uploadPlan(s);
    queueDeviceColumns(s);
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += plan.h2d_bytes;
    sub.reset(new HostScope("groups_build: allocations"));
    allocate(s);
    sub.reset(new HostScope("groups_build: launches"));
    if (s.e == hipSuccess) {
        span = ctx->spanBegin(FAM_BUILD);
        queueZeroWide(s);
        queuePartition(s);
        queueDirectRoute(s);
        queueMaskRoute(s);
        queueWordRoute(s);
        queueIncidenceInversion(s);
        queueTileRoute(s);
        queueListRoute(s);
        sub.reset(new HostScope("groups_build: row collapse launches"));
        if (collapse && s.e == hipSuccess) queueCollapse(s);
        sub.reset();
        ctx->spanEnd(span);
        ctx->stats.build_launches += 3;
        s.ok(hipGetLastError());
        static const bool wait_here = RPVG_EXPERIMENT_ENV("RPVG_HIP_BUILD_SYNC") != nullptr;  // A/B knob: host sync before returning
        if (wait_here) s.ok(hipStreamSynchronize(s.st));
    }
    if (s.e != hipSuccess) {
        setError("rpvg_hip_groups_build: %s", hipGetErrorString(s.e));
        (void) hipStreamSynchronize(s.st);  // whatever was queued before the failure still uses the buffers
        g.reset();
        return (s.e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    *groups_out = g.release();
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" int rpvg_hip_groups_build(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_group_spec * spec,
                                     rpvg_hip_groups ** groups_out) {
    RPVG_REQUIRE(ctx && batch && spec && groups_out, "rpvg_hip_groups_build: NULL argument");
    *groups_out = nullptr;
    RPVG_REQUIRE(spec->num_matrices == 0 || (spec->cluster && spec->group_off && spec->group_path_off && spec->group_path),
                 "rpvg_hip_groups_build: NULL spec arrays");
    return buildGroups(ctx, batch, spec, Columns::Lists, groups_out);
}

// The spec of matrices whose columns the device makes: as many columns, and as many list entries, as `sizes` says of every
// matrix's cluster.  A cluster outside the batch counts for nothing here: the plan refuses it.
template <typename Sizes>
static int buildImpliedGroups(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const uint32_t num_matrices, const uint32_t * clusters, const int32_t normalise,
                              const double collapse_precision, const Columns kind, rpvg_hip_groups ** groups_out, const Sizes sizes) {
    std::vector<uint64_t> group_off(num_matrices + 1, 0), first_path(num_matrices + 1, 0);
    for (uint32_t m = 0; m < num_matrices; ++m) {
        const bool known = clusters[m] < batch->num_clusters;
        group_off[m + 1] = group_off[m] + (known ? sizes(clusters[m]).first : 0);
        first_path[m + 1] = first_path[m] + (known ? sizes(clusters[m]).second : 0);
    }
    rpvg_hip_group_spec spec;
    spec.num_matrices = num_matrices;
    spec.cluster = clusters;
    spec.group_off = group_off.data();
    spec.group_path_off = first_path.data();  // (per MATRIX: the first list entry of its columns)
    spec.group_path = nullptr;
    spec.normalise = normalise;
    spec.collapse_precision = collapse_precision;
    return buildGroups(ctx, batch, &spec, kind, groups_out);
}

extern "C" int rpvg_hip_groups_build_from_sources(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_matrices, const uint32_t * clusters,
                                                  int32_t normalise, double collapse_precision, rpvg_hip_groups ** groups_out) {
    RPVG_REQUIRE(ctx && batch && groups_out && (clusters || num_matrices == 0), "rpvg_hip_groups_build_from_sources: NULL argument");
    *groups_out = nullptr;
    if (!batch->has_source_columns) {
        setError("rpvg_hip_groups_build_from_sources: not taken (the batch was uploaded without PathInfo::source_ids, or their id ranges "
                 "outgrew the device scratch)");
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    for (uint32_t m = 0; m < num_matrices && clusters[m] < batch->num_clusters; ++m) {
        RPVG_REQUIRE(batch->h_src_num_cols[clusters[m]] > 0, "rpvg_hip_groups_build_from_sources: cluster %u has no source (haplotype) ids on its paths",
                     clusters[m]);
    }
    // the columns of matrix m are those of its cluster: the offsets are sums of sizes the upload brought back
    return buildImpliedGroups(ctx, batch, num_matrices, clusters, normalise, collapse_precision, Columns::Sources, groups_out, [batch](const uint32_t k) {
        return std::pair<uint64_t, uint64_t>(batch->h_src_num_cols[k], batch->h_src_col_paths[k]);
    });
}

extern "C" int rpvg_hip_groups_build_single_paths(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_matrices, const uint32_t * clusters,
                                                  int32_t normalise, double collapse_precision, rpvg_hip_groups ** groups_out) {
    RPVG_REQUIRE(ctx && batch && groups_out && (clusters || num_matrices == 0), "rpvg_hip_groups_build_single_paths: NULL argument");
    *groups_out = nullptr;
    // a column is one path, hence one list entry
    return buildImpliedGroups(ctx, batch, num_matrices, clusters, normalise, collapse_precision, Columns::SinglePaths, groups_out, [batch](const uint32_t k) {
        const uint64_t paths = batch->h_cluster_path_off[k + 1] - batch->h_cluster_path_off[k];
        return std::pair<uint64_t, uint64_t>(paths, paths);
    });
}

int rpvg_hip_groups::buildError(hipStream_t stream) const {
    if (build_checked || !build_error_flag.ptr) return RPVG_HIP_OK;
    uint32_t bad = 0;
    hipError_t e = hipMemcpyAsync(&bad, build_error_flag.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        setError("rpvg_hip_groups_build: %s", hipGetErrorString(e));
        return RPVG_HIP_ERR_RUNTIME;
    }
    if (bad) {
        setError(bad == 2 ? "rpvg_hip_groups_build: a group lists a path twice" : "rpvg_hip_groups_build: a group refers to a path outside its cluster");
        return RPVG_HIP_ERR_INVALID;
    }
    build_checked = true;
    return RPVG_HIP_OK;
}

// One built matrix row by row, for the tests of the row collapse (include/rpvg_hip.h): behind waitCollapse, so with the rows of
// every run rewritten — a held-back last stage is queued first.  The matrix's places come from the device's own offset arrays.
extern "C" int rpvg_hip_groups_rows(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t matrix, double * values_out, double * noise_out,
                                    double * rowmax_out, double * count_out) {
    RPVG_REQUIRE(ctx && groups, "rpvg_hip_groups_rows: NULL argument");
    RPVG_REQUIRE(matrix < groups->num_matrices, "rpvg_hip_groups_rows: matrix %u of %u", matrix, groups->num_matrices);
    const uint64_t R = groups->h_num_rows[matrix], G = groups->h_num_cols[matrix];
    RPVG_REQUIRE(R == 0 || (noise_out && rowmax_out && count_out && (values_out || G == 0)), "rpvg_hip_groups_rows: NULL output");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(groups->waitCollapse(st));
    uint64_t val_off = 0, row_off = 0;
    RPVG_HIP_CHECK(hipMemcpyAsync(&val_off, groups->mat_val_off.ptr + matrix, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&row_off, groups->mat_row_off.ptr + matrix, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(waitStream(st));
    RPVG_REQUIRE(val_off + R * G <= groups->values.count && row_off + R <= groups->rowmax.count && row_off + R <= groups->row_count.count &&
                     row_off + R <= groups->row_noise.count,
                 "rpvg_hip_groups_rows: matrix %u lies outside the buffers", matrix);
    if (R * G) RPVG_HIP_CHECK(hipMemcpyAsync(values_out, groups->values.ptr + val_off, R * G * sizeof(double), hipMemcpyDeviceToHost, st));
    if (R) {
        RPVG_HIP_CHECK(hipMemcpyAsync(noise_out, groups->row_noise.ptr + row_off, R * sizeof(double), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipMemcpyAsync(rowmax_out, groups->rowmax.ptr + row_off, R * sizeof(double), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipMemcpyAsync(count_out, groups->row_count.ptr + row_off, R * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    RPVG_HIP_CHECK(waitStream(st));
    return groups->buildError(st);  // the matrices were built without a host sync
}

extern "C" void rpvg_hip_groups_free(rpvg_hip_ctx * ctx, rpvg_hip_groups * groups) {
    if (!groups) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
        static const bool trace = std::getenv("RPVG_AMD_TRACE") != nullptr;
        if (trace && groups->collapse_info.ptr && groups->waitCollapse(ctx->stream) == hipSuccess) {
            uint32_t info[4] = {0, 0, 0, 0};
            // (on the context's stream: a plain hipMemcpy waits for every stream of the device, the other lane's search included)
            if (hipMemcpyAsync(info, groups->collapse_info.ptr, sizeof(info), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                hipStreamSynchronize(ctx->stream) == hipSuccess) {
                std::fprintf(stderr, "[rpvg_hip trace]   row collapse: %u of %u matrices replayed (%u sorted whole), %u active rows, %u rows took their head's values\n",
                             info[0], groups->num_matrices, info[2], info[3], info[1]);
            }
        }
        delete groups;
    } else {
        delete groups;
    }
}
