// Weighted minimum path cover over the whole GPU (gfx950), one cluster at a time: the second route of `-i strains`' greedy set
// cover (path_cover.hip is the first: one workgroup per cluster, at most 9 600 paths).  cover_plan.hpp decides which listed
// cluster takes which; rpvg_hip_min_path_cover_any is the entry point of both.
//
// Every dependency between workgroups is a launch boundary: no flag is handed over inside a kernel, no launch is cooperative,
// no floating-point number is added atomically.
//
// Set-up, once per cluster
//   rows      c = count, or 0 for a row whose noise probability is 1 (cover_terms.hpp); such a row starts covered
//   entries   the row of every entry
//   columns   a STABLE radix sort of the entries by path (hipcub, ceil(log2 N) bits): a path's entries lie together in
//             ascending row order; the column offsets are the run heads; rows and terms count * log(prob) gathered in that order
//   weights   per path ONE chain of IEEE additions from 0.0 over its terms in ascending row order, then x -1.0: the additions
//             of minPathCoverKernel, so a weight has the same bits on both routes and twins tie exactly.  A wavefront per
//             path: the lanes load 64 terms and the next 64 before the chain over the ones they hold starts; the chain reads
//             them out of the lanes' registers (v_readlane), so nothing but the additions is on it
//   gains     gain[j] = sum of c over column j, 64-bit integers (exact in any order); converted to double for the division
//             alone (exact below 2^53, the bound minPathCoverKernel's FP64 sums assume too)
// A round is two launches
//   pick      gain[j] / weight[j], the largest positive value, the lower index among equals at every level (thread, wavefront,
//             workgroup, across workgroups); comparisons are `v > best`, so the NaN of 0 / 0 never wins.  A pair per workgroup
//   strike    every workgroup reduces the pairs itself; workgroup 0 records the choice (bitmap, choice order, round count), or
//             `done` when nothing positive is left; all walk the chosen column: a row not yet covered is claimed with an integer
//             atomic (a malformed row that lists a path twice is struck once) and takes its c off the gain of every path it
//             holds — through an LDS histogram per workgroup for a cluster of at most kHistPaths paths (one global integer
//             atomic per non-zero bin), with global integer atomics for a wider one
// Over all rounds the strikes touch every entry of the cluster once, plus the chosen columns.
// The host queues rounds in chunks without waiting, copies the control record (done, rounds) behind each chunk and looks at the
// chunk before the one just queued (the scheme of em_grid.hip); the kernels of a round after `done` return at once; a cluster
// needs at most N rounds.  The ascending cover comes from the bitmap by a prefix sum over its words.

#include "cover_plan.hpp"
#include "cover_terms.hpp"
#include "device_algos.hpp"

#include <algorithm>
#include <vector>

using namespace rpvg_hip_detail;
using namespace rpvg_cover;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kSetupBlock = 256;
constexpr int kWeightBlock = 256;   // four wavefronts, a path each

struct CoverGridControl {
    uint32_t done;     // nothing positive was left in some round: the kernels of every later round return at once
    uint32_t rounds;   // paths chosen so far
};

// one cluster on the grid route: its part of the batch and its scratch (cover_plan.hpp: GridScratch)
struct GridCluster {
    uint64_t r0, e0;   // first row and first entry of the cluster in the batch
    uint32_t R, E, N;
    const uint64_t * row_ent_off;
    const uint32_t * ent_path;
    const double * ent_prob, * row_count, * row_noise;
    double * row_c;
    uint32_t * covered, * ent_row, * ent_index, * sorted_path, * sorted_index, * col_row;
    double * col_term;
    uint32_t * col_off;
    double * weight;
    unsigned long long * gain;
    uint32_t * chosen;
    double * pair_val;
    uint32_t * pair_idx;
    CoverGridControl * ctl;
    uint32_t * order;   // the paths in the order the rounds chose them
    uint32_t * cover;   // ascending
    uint32_t * cover_size;
    uint32_t pick_blocks;
};

__global__ __launch_bounds__(kSetupBlock) void coverRowsKernel(const GridCluster g) {
    const uint32_t i = blockIdx.x * kSetupBlock + threadIdx.x;
    if (i >= g.R) return;
    const double c = coverRowCount(g.row_count[g.r0 + i], g.row_noise[g.r0 + i]);
    g.row_c[i] = c;
    g.covered[i] = (c > 0.0) ? 0u : 1u;
}

__global__ __launch_bounds__(kSetupBlock) void coverEntriesKernel(const GridCluster g) {
    const uint32_t t = blockIdx.x * kSetupBlock + threadIdx.x;
    if (t >= g.E) return;
    // the row of entry t: the last one that starts at or before it (rows without entries never qualify)
    const uint64_t e = g.e0 + t;
    const uint64_t * off = g.row_ent_off + g.r0;
    uint32_t lo = 0, hi = g.R;  // off[lo] <= e < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    g.ent_row[t] = lo;
    g.ent_index[t] = t;
}

__global__ __launch_bounds__(kSetupBlock) void coverGatherKernel(const GridCluster g) {
    const uint32_t i = blockIdx.x * kSetupBlock + threadIdx.x;
    if (i >= g.E) return;
    const uint32_t t = g.sorted_index[i], row = g.ent_row[t];
    g.col_row[i] = row;
    g.col_term[i] = coverTerm(g.ent_prob[g.e0 + t], g.row_c[row]);
}

// col_off[j] = the first place of the sorted entries whose path is at least j, from the run heads (a path beyond the cluster's —
// the upload refuses such a row — would end up behind column N - 1, in no column)
__global__ __launch_bounds__(kSetupBlock) void coverColumnOffsetsKernel(const GridCluster g) {
    const uint32_t i = blockIdx.x * kSetupBlock + threadIdx.x;
    if (i >= g.E) return;
    const uint64_t p = std::min<uint64_t>(g.sorted_path[i], g.N);
    const uint64_t first = (i == 0) ? 0 : std::min<uint64_t>(g.sorted_path[i - 1], g.N) + 1;
    for (uint64_t j = first; j <= p; ++j) g.col_off[j] = i;
    if (i == g.E - 1) {
        for (uint64_t j = p + 1; j <= g.N; ++j) g.col_off[j] = g.E;
    }
}

// acc + the values of the first `count` lanes, in lane order: one chain of additions, carried by every lane alike (the values come
// out of the lanes' registers, the lane a constant of the unrolled loop; `count` is uniform, the branches are scalar)
__device__ __forceinline__ double addLanesInOrder(double acc, const double value, const uint32_t count) {
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const double x = readLaneF64(value, j);
        if (static_cast<uint32_t>(j) < count) acc = addRounded(acc, x);
    }
    return acc;
}

__global__ __launch_bounds__(kWeightBlock) void coverWeightsKernel(const GridCluster g) {
    const uint32_t j = blockIdx.x * (kWeightBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= g.N) return;
    const uint32_t begin = g.col_off[j], end = g.col_off[j + 1];
    double acc = 0.0;
    unsigned long long covered_reads = 0;
    double term = (begin + lane < end) ? g.col_term[begin + lane] : 0.0;
    unsigned long long c = (begin + lane < end) ? static_cast<unsigned long long>(g.row_c[g.col_row[begin + lane]]) : 0ull;
    for (uint32_t base = begin; base < end; base += 64) {
        const uint64_t ahead = static_cast<uint64_t>(base) + 64 + lane;
        const double next_term = (ahead < end) ? g.col_term[ahead] : 0.0;
        const unsigned long long next_c = (ahead < end) ? static_cast<unsigned long long>(g.row_c[g.col_row[ahead]]) : 0ull;
        const uint32_t held = end - base;
        if (held >= 64) {
#pragma unroll
            for (int l = 0; l < 64; ++l) acc = addRounded(acc, readLaneF64(term, l));
        } else {
            acc = addLanesInOrder(acc, term, held);
        }
        covered_reads += c;
        term = next_term;
        c = next_c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) covered_reads += __shfl_xor(covered_reads, d, 64);
    if (lane == 0) {
        g.weight[j] = mulRounded(acc, -1.0);
        g.gain[j] = covered_reads;
    }
}

// (value, index) of a wavefront, then of the workgroup: the larger value, the lower index among equals; in every thread
template <int BLOCK>
__device__ __forceinline__ void blockBest(double & best_val, uint32_t & best_idx, double * red_val, uint32_t * red_idx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(best_val, d, 64);
        const uint32_t oi = __shfl_xor(best_idx, d, 64);
        if (ov > best_val || (ov == best_val && oi < best_idx)) {
            best_val = ov;
            best_idx = oi;
        }
    }
    if (lane == 0) {
        red_val[wave] = best_val;
        red_idx[wave] = best_idx;
    }
    __syncthreads();
    best_val = red_val[0];
    best_idx = red_idx[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) {
        if (red_val[w] > best_val || (red_val[w] == best_val && red_idx[w] < best_idx)) {
            best_val = red_val[w];
            best_idx = red_idx[w];
        }
    }
}

__global__ __launch_bounds__(kPickBlock) void coverPickKernel(const GridCluster g) {
    __shared__ double red_val[kPickBlock / 64];
    __shared__ uint32_t red_idx[kPickBlock / 64];
    if (g.ctl->done) return;
    // first index with the largest positive covered / weight
    double best_val = 0.0;
    uint32_t best_idx = kNone;
    for (uint64_t tile = blockIdx.x; tile * kPickTile < g.N; tile += gridDim.x) {
#pragma unroll
        for (uint32_t u = 0; u < kPickPerThread; ++u) {
            const uint64_t j = tile * kPickTile + u * kPickBlock + threadIdx.x;
            if (j < g.N) {
                const double v = static_cast<double>(g.gain[j]) / g.weight[j];
                if (v > best_val) {
                    best_val = v;
                    best_idx = static_cast<uint32_t>(j);
                }
            }
        }
    }
    blockBest<kPickBlock>(best_val, best_idx, red_val, red_idx);
    if (threadIdx.x == 0) {
        g.pair_val[blockIdx.x] = best_val;
        g.pair_idx[blockIdx.x] = best_idx;
    }
}

template <bool HISTOGRAM>
__global__ __launch_bounds__(kStrikeBlock) void coverStrikeKernel(const GridCluster g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ double red_val[kStrikeBlock / 64];
    __shared__ uint32_t red_idx[kStrikeBlock / 64];
    static_assert(kPickMaxBlocks <= kStrikeBlock, "a thread per pair");
    if (g.ctl->done) return;
    double best_val = 0.0;
    uint32_t best_idx = kNone;
    if (threadIdx.x < g.pick_blocks) {
        const double v = g.pair_val[threadIdx.x];
        if (v > best_val) {
            best_val = v;
            best_idx = g.pair_idx[threadIdx.x];
        }
    }
    blockBest<kStrikeBlock>(best_val, best_idx, red_val, red_idx);
    const uint32_t best = (best_val > 0.0) ? best_idx : kNone;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (best == kNone) {
            g.ctl->done = 1;
        } else {
            const uint32_t round = g.ctl->rounds;
            g.chosen[best >> 5] |= 1u << (best & 31);
            g.order[round] = best;
            g.ctl->rounds = round + 1;
        }
    }
    if (best == kNone) return;
    const uint32_t begin = g.col_off[best], end = g.col_off[best + 1];
    const uint64_t first = static_cast<uint64_t>(begin) + static_cast<uint64_t>(blockIdx.x) * kStrikeBlock;
    if (first >= end) return;  // (the whole workgroup: nothing of the column is left for it)
    unsigned long long * hist = reinterpret_cast<unsigned long long *>(smem_raw);  // [N]
    if (HISTOGRAM) {
        for (uint32_t j = threadIdx.x; j < g.N; j += kStrikeBlock) hist[j] = 0;
        __syncthreads();
    }
    for (uint64_t i = first + threadIdx.x; i < end; i += static_cast<uint64_t>(gridDim.x) * kStrikeBlock) {
        const uint32_t row = g.col_row[i];
        if (atomicExch(&g.covered[row], 1u) == 0u) {
            const unsigned long long c = static_cast<unsigned long long>(g.row_c[row]);
            const uint64_t e1 = g.row_ent_off[g.r0 + row + 1];
            for (uint64_t e = g.row_ent_off[g.r0 + row]; e < e1; ++e) {
                const uint32_t path = g.ent_path[e];
                if (path < g.N) {
                    if (HISTOGRAM) atomicAdd(&hist[path], c);
                    else atomicAdd(&g.gain[path], 0ull - c);
                }
            }
        }
    }
    if (HISTOGRAM) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < g.N; j += kStrikeBlock) {
            const unsigned long long h = hist[j];
            if (h) atomicAdd(&g.gain[j], 0ull - h);
        }
    }
}

// ascending order (src/path_abundance_estimator.cpp:337): the set bits of `chosen`, each word's place from a prefix sum of the
// words' bit counts
__global__ __launch_bounds__(kSetupBlock) void coverFinishKernel(const GridCluster g) {
    __shared__ uint32_t scan_scratch[kSetupBlock / 64];
    const uint32_t num_words = (g.N + 31) >> 5;
    uint32_t written = 0;
    for (uint32_t w0 = 0; w0 < num_words; w0 += kSetupBlock) {
        const uint32_t w = w0 + threadIdx.x;
        uint32_t bits = (w < num_words) ? g.chosen[w] : 0;
        uint32_t total;
        uint32_t at = written + blockExclusiveSum<kSetupBlock>(static_cast<uint32_t>(__popc(bits)), total, scan_scratch);
        while (bits) {
            g.cover[at++] = (w << 5) + static_cast<uint32_t>(__ffs(static_cast<int>(bits)) - 1);
            bits &= bits - 1;
        }
        written += total;
    }
    if (threadIdx.x == 0) g.cover_size[0] = g.ctl->rounds;
}

// what a run keeps beside its device buffers: two pinned slots for the control record and the events behind their copies
struct ControlLooks {
    CoverGridControl * h_ctl = nullptr;
    hipEvent_t looked[2] = {nullptr, nullptr};
    ~ControlLooks() {
        for (hipEvent_t & ev : looked) {
            if (ev) (void) hipEventDestroy(ev);
        }
        if (h_ctl) pinnedFree(h_ctl);
    }
};

// One cluster over the whole GPU; cover_out and order_out hold N cells each.  Returns with the stream waited for.
int coverOnGrid(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const uint32_t k, uint32_t * cover_out, uint32_t * order_out, uint32_t * size_out) {
    hipStream_t st = ctx->stream;
    GridCluster g;
    g.r0 = batch->h_cluster_row_off[k];
    g.e0 = batch->h_cluster_ent_off[k];
    g.R = static_cast<uint32_t>(batch->h_cluster_row_off[k + 1] - g.r0);
    g.E = static_cast<uint32_t>(batch->h_cluster_ent_off[k + 1] - g.e0);
    g.N = static_cast<uint32_t>(batch->h_cluster_path_off[k + 1] - batch->h_cluster_path_off[k]);
    g.row_ent_off = batch->row_ent_off.ptr;
    g.ent_path = batch->ent_path.ptr;
    g.ent_prob = batch->ent_prob.ptr;
    g.row_count = batch->row_count.ptr;
    g.row_noise = batch->row_noise.ptr;
    const GridScratch sizes = gridScratch(g.N, g.R, g.E);

    DeviceBuffer<double> row_c, col_term, weight, pair_val;
    DeviceBuffer<uint32_t> covered, ent_row, ent_index, sorted_path, sorted_index, col_row, col_off, chosen, pair_idx, order, cover, cover_size;
    DeviceBuffer<unsigned long long> gain;
    DeviceBuffer<CoverGridControl> ctl;
    RPVG_HIP_CHECK(row_c.alloc(sizes.row_count));
    RPVG_HIP_CHECK(covered.alloc(sizes.row_covered));
    RPVG_HIP_CHECK(ent_row.alloc(sizes.ent_row));
    RPVG_HIP_CHECK(ent_index.alloc(sizes.ent_index));
    RPVG_HIP_CHECK(sorted_path.alloc(sizes.sorted_path));
    RPVG_HIP_CHECK(sorted_index.alloc(sizes.sorted_index));
    RPVG_HIP_CHECK(col_row.alloc(sizes.col_row));
    RPVG_HIP_CHECK(col_term.alloc(sizes.col_term));
    RPVG_HIP_CHECK(col_off.alloc(sizes.col_off));
    RPVG_HIP_CHECK(weight.alloc(sizes.weight));
    RPVG_HIP_CHECK(gain.alloc(sizes.gain));
    RPVG_HIP_CHECK(chosen.alloc(sizes.chosen_words));
    RPVG_HIP_CHECK(pair_val.alloc(sizes.pick_pairs));
    RPVG_HIP_CHECK(pair_idx.alloc(sizes.pick_pairs));
    RPVG_HIP_CHECK(ctl.alloc(1));
    RPVG_HIP_CHECK(order.alloc(g.N));
    RPVG_HIP_CHECK(cover.alloc(g.N));
    RPVG_HIP_CHECK(cover_size.alloc(1));
    g.row_c = row_c.ptr;
    g.covered = covered.ptr;
    g.ent_row = ent_row.ptr;
    g.ent_index = ent_index.ptr;
    g.sorted_path = sorted_path.ptr;
    g.sorted_index = sorted_index.ptr;
    g.col_row = col_row.ptr;
    g.col_term = col_term.ptr;
    g.col_off = col_off.ptr;
    g.weight = weight.ptr;
    g.gain = gain.ptr;
    g.chosen = chosen.ptr;
    g.pair_val = pair_val.ptr;
    g.pair_idx = pair_idx.ptr;
    g.ctl = ctl.ptr;
    g.order = order.ptr;
    g.cover = cover.ptr;
    g.cover_size = cover_size.ptr;
    g.pick_blocks = pickBlocks(g.N);

    ControlLooks looks;
    RPVG_HIP_CHECK(pinnedAlloc(reinterpret_cast<void **>(&looks.h_ctl), 2 * sizeof(CoverGridControl)));
    RPVG_HIP_CHECK(hipEventCreateWithFlags(&looks.looked[0], hipEventDisableTiming));
    RPVG_HIP_CHECK(hipEventCreateWithFlags(&looks.looked[1], hipEventDisableTiming));

    // ---- set-up
    uint64_t launches = 0;
    const int span = ctx->spanBegin(FAM_BUILD);
    hipError_t e = zeroAsync(chosen.ptr, sizeof(uint32_t) * sizes.chosen_words, st);
    if (e == hipSuccess) e = zeroAsync(ctl.ptr, sizeof(CoverGridControl), st);
    if (e == hipSuccess) {
        coverRowsKernel<<<gridFor(g.R, kSetupBlock), dim3(kSetupBlock), 0, st>>>(g);
        ++launches;
        if (g.E > 0) {
            coverEntriesKernel<<<gridFor(g.E, kSetupBlock), dim3(kSetupBlock), 0, st>>>(g);
            ++launches;
        } else {
            e = zeroAsync(col_off.ptr, sizeof(uint32_t) * sizes.col_off, st);
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e != hipSuccess) ctx->spanEnd(span);
    RPVG_HIP_CHECK(e);
    if (g.E > 0) {
        // (stable: equal paths keep the ascending rows they come in with)
        if (const int rc = sortPairs(st, g.ent_path + g.e0, g.sorted_path, g.ent_index, g.sorted_index, g.E, sortBits(g.N))) {
            ctx->spanEnd(span);
            return rc;
        }
        coverGatherKernel<<<gridFor(g.E, kSetupBlock), dim3(kSetupBlock), 0, st>>>(g);
        coverColumnOffsetsKernel<<<gridFor(g.E, kSetupBlock), dim3(kSetupBlock), 0, st>>>(g);
        launches += 2;
    }
    coverWeightsKernel<<<gridFor(g.N, kWeightBlock / 64), dim3(kWeightBlock), 0, st>>>(g);
    ++launches;
    e = hipGetLastError();

    // ---- rounds, in chunks: the control record of chunk k is looked at while chunk k + 1 runs
    const bool histogram = strikeUsesHistogram(g.N);
    const size_t strike_lds = histogram ? sizeof(unsigned long long) * g.N : 0;
    const uint32_t strike_blocks = strikeBlocks(g.R);
    const uint64_t max_rounds = maxRounds(g.N);
    uint64_t queued = 0;
    uint32_t chunk = 0;
    bool done = false;
    while (e == hipSuccess && !done) {
        const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(kChunkRounds, max_rounds - queued));
        for (uint32_t r = 0; r < n; ++r) {
            coverPickKernel<<<dim3(g.pick_blocks), dim3(kPickBlock), 0, st>>>(g);
            if (histogram) coverStrikeKernel<true><<<dim3(strike_blocks), dim3(kStrikeBlock), strike_lds, st>>>(g);
            else coverStrikeKernel<false><<<dim3(strike_blocks), dim3(kStrikeBlock), 0, st>>>(g);
        }
        queued += n;
        launches += 2ull * n;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&looks.h_ctl[chunk & 1], ctl.ptr, sizeof(CoverGridControl), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(looks.looked[chunk & 1], st);
        if (e == hipSuccess && chunk > 0) {
            e = waitEvent(looks.looked[(chunk - 1) & 1]);
            done = e == hipSuccess && looks.h_ctl[(chunk - 1) & 1].done != 0;
        }
        if (e == hipSuccess && !done && queued >= max_rounds) done = true;  // the last chunk there can be
        ++chunk;
    }
    if (e == hipSuccess) {
        coverFinishKernel<<<dim3(1), dim3(kSetupBlock), 0, st>>>(g);
        ++launches;
        e = hipGetLastError();
    }
    ctx->spanEnd(span);
    RPVG_HIP_CHECK(e);
    ctx->stats.build_launches += launches;
    RPVG_HIP_CHECK(cover_size.download(size_out, st));
    RPVG_HIP_CHECK(cover.download(cover_out, st));
    RPVG_HIP_CHECK(order.download(order_out, st));
    RPVG_HIP_CHECK(waitStream(st));  // (the buffers of this cluster go back to the pool)
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" void rpvg_hip_cover_limits(rpvg_cover_limits * limits_out) {
    if (!limits_out) return;
    limits_out->workgroup_max_paths = kWorkgroupMaxPaths;
    limits_out->chunk_rounds = kChunkRounds;
    limits_out->default_grid_min_work = kDefaultGridMinWork;
    limits_out->grid_max_rows = kGridMaxRows;
    limits_out->grid_max_entries = kGridMaxEntries;
    limits_out->pick_block = kPickBlock;
    limits_out->pick_per_thread = kPickPerThread;
    limits_out->pick_max_blocks = kPickMaxBlocks;
    limits_out->strike_block = kStrikeBlock;
    limits_out->strike_max_blocks = kStrikeMaxBlocks;
    limits_out->hist_max_paths = kHistPaths;
}

extern "C" int rpvg_hip_min_path_cover_any(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters, const uint32_t * clusters,
                                           const uint64_t * cover_off, uint32_t * cover, uint32_t * cover_size, uint64_t grid_min_work,
                                           uint32_t * choice_order) {
    RPVG_REQUIRE(ctx && batch, "rpvg_hip_min_path_cover_any: NULL argument");
    if (num_clusters == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(clusters && cover_off && cover && cover_size, "rpvg_hip_min_path_cover_any: NULL argument");
    // the route of every listed cluster, before anything is launched
    std::vector<uint32_t> grid_listed, workgroup_listed, workgroup_clusters;
    std::vector<uint64_t> workgroup_off(1, 0);
    size_t widest = 0;
    for (uint32_t i = 0; i < num_clusters; ++i) {
        const uint32_t k = clusters[i];
        RPVG_REQUIRE(k < batch->num_clusters, "rpvg_hip_min_path_cover_any: cluster %u of %u", k, batch->num_clusters);
        const uint64_t N = batch->h_cluster_path_off[k + 1] - batch->h_cluster_path_off[k];
        const uint64_t rows = batch->h_cluster_row_off[k + 1] - batch->h_cluster_row_off[k];
        const uint64_t entries = batch->h_cluster_ent_off[k + 1] - batch->h_cluster_ent_off[k];
        RPVG_REQUIRE(rows > 0 && N > 0, "rpvg_hip_min_path_cover_any: cluster %u is empty", k);
        RPVG_REQUIRE(cover_off[i + 1] - cover_off[i] >= N, "rpvg_hip_min_path_cover_any: output range of cluster %u is smaller than its %llu paths", k,
                     static_cast<unsigned long long>(N));
        if (routeOf(N, rows, entries, grid_min_work) == kRouteGrid) {
            RPVG_REQUIRE(N <= UINT32_MAX && gridFits(rows, entries),
                         "rpvg_hip_min_path_cover_any: cluster %u (%llu paths, %llu rows, %llu entries) is beyond the whole-GPU route (rows and entries "
                         "below 2^31 each)", k, static_cast<unsigned long long>(N), static_cast<unsigned long long>(rows),
                         static_cast<unsigned long long>(entries));
            grid_listed.push_back(i);
            widest = std::max<size_t>(widest, N);
        } else {
            workgroup_listed.push_back(i);
            workgroup_clusters.push_back(k);
            workgroup_off.push_back(workgroup_off.back() + N);
        }
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    if (!workgroup_listed.empty()) {  // side by side, in one launch
        std::vector<uint32_t> found(workgroup_off.back()), sizes(workgroup_listed.size());
        if (const int rc = minPathCoverWorkgroups(ctx, batch, static_cast<uint32_t>(workgroup_listed.size()), workgroup_clusters.data(), workgroup_off.data(),
                                                  found.data(), sizes.data())) {
            return rc;
        }
        for (size_t w = 0; w < workgroup_listed.size(); ++w) {
            const uint32_t i = workgroup_listed[w];
            std::copy(found.begin() + workgroup_off[w], found.begin() + workgroup_off[w] + sizes[w], cover + cover_off[i]);
            cover_size[i] = sizes[w];
            if (choice_order) choice_order[cover_off[i]] = UINT32_MAX;  // (no order on this route)
        }
    }
    std::vector<uint32_t> found(widest), order(widest);
    for (const uint32_t i : grid_listed) {  // one after the other
        uint32_t size = 0;
        if (const int rc = coverOnGrid(ctx, batch, clusters[i], found.data(), order.data(), &size)) return rc;
        std::copy(found.begin(), found.begin() + size, cover + cover_off[i]);
        if (choice_order) std::copy(order.begin(), order.begin() + size, choice_order + cover_off[i]);
        cover_size[i] = size;
        ctx->stats.cover_grid_problems += 1;
        ctx->stats.cover_grid_rounds += size;
    }
    return RPVG_HIP_OK;
}
