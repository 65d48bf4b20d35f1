// gibbs_table.hip — the read-count Gibbs samples of a batch (-n) as the table of `<prefix>_gibbs.txt.gz`: per path its N sample
// columns in the order the writer prints them, the rows it prints, and the per-sample noise totals of the `Unknown` row
// (interface include/rpvg_samples.h).
//
// Takes over   the per-path column vectors, the transposed zero-filled read and the noise totals of
//              ReadCountGibbsSamplesWriter::addSamples                                 src/threaded_output_writer.cpp:114-214
//
// Arithmetic   The table is a copy: the samples move as 64-bit words, so -0.0, subnormals and any other pattern arrive as they are;
//              a cell without a source is the word 0 (+0.0).  The only additions are the noise chains: one chain per sample column
//              over the clusters in ascending order, plain IEEE additions from 0.0 — no atomics, no tree (a tree is another sum).
// Describe     one kernel behind the copy validates every offset, the abundance counts, the path ids and the clusters' numbers of
//              samples (the smallest offender comes back in one word; the host words the message), and writes per cluster S_k and
//              where its noise samples begin, per block its cluster and base_i (the noise samples of a cluster are contiguous over
//              its blocks: base_i = noise_off[b] - noise_off[gibbs_off[k]], no scan), the widest block of every cluster and `listed`.
//              A second, tiny kernel gives every cluster its route (gibbs_table_plan.hpp) and every block with samples its place in
//              the work list of that route.  Nothing below runs on a refused input, and nothing above reads outside the stated sizes.
// Scatter      EVERY CELL IS WRITTEN EXACTLY ONCE, there is no clearing pass (a memset of the table is as many bytes as the table):
//              columns [base_i, base_i + n_i) of all rows of a cluster belong to block i, columns [S_k, N) to the tail kernel.
//                resident   a workgroup per block; per tile of 64 samples the contiguous piece of the source (64 * c doubles) is
//                           loaded flat into LDS at an odd pitch, then a wavefront per path stores 64 consecutive doubles of its row.
//                           The ids of the block sit one in a lane: the column of a path is a ballot, not a table in memory.
//                global     a wavefront per (block, 64 paths): the ids of the block inside its 64 paths (two searches in the ascending
//                           list) sit one in a lane, the samples are read where they lie.  No (path, block) words in memory at all:
//                           they would be paths x blocks words for a cluster (400 MB for 100 000 paths and 1 000 blocks).
//                tail       a wavefront per path of the batch: the columns S_k .. N - 1.
// Noise        one lane per sample column, the clusters in ascending order; lane s reads noise_at[k] + s (coalesced), the loads of
//              the next 32 clusters are in flight while the chain adds the 32 it holds.
// No kernel allocates or uses scratch; every array is sized by K, B, P or N.

#include "device_algos.hpp"
#include "gibbs_table_plan.hpp"
#include "gibbs_samples.hpp"
#include "table_kit.hpp"
#include "table_residents.hpp"
#include "../../include/rpvg_samples.h"

#pragma clang fp contract(off)

using namespace rpvg_hip_detail;
using namespace rpvg_gibbs_table;

// the table of a batch
struct rpvg_hip_gibbs_table {
    uint32_t num_clusters = 0, num_gibbs_samples = 0;
    uint64_t num_blocks = 0, num_paths = 0;
    DeviceBuffer<word64> samples;       // [P * N]
    DeviceBuffer<uint8_t> listed;       // [P] (allocated in words)
    DeviceBuffer<double> noise_counts;  // [N]
    std::vector<double> h_samples, h_noise_counts;
    std::vector<uint8_t> h_listed;
    std::vector<uint64_t> h_cluster_path_off;  // [K+1]
    uint32_t clusters_by_route[kRoutes] = {0, 0};
    bool downloaded = false;
};

namespace {

// bad = min over the offending clusters and blocks (table_kit.hpp: a block is the second kind, so a cluster comes before every block)

enum TableBad {
    kBadGibbsOff = 1, kBadClusterPathOff = 2, kBadTooManySamples = 3,                                        // a cluster's
    kBadPathOff = 4, kBadNoiseOff = 5, kBadAbundOff = 6, kBadAbundCount = 7, kBadPathId = 8, kBadPathOrder = 9  // a block's
};

enum Counter { kBlocksOfRoute = 0, kClustersOfRoute = kRoutes, kGlobalMaxPaths = 2 * kRoutes, kCounters = 2 * kRoutes + 1 };

struct TableArgs {
    uint32_t K, N;
    uint64_t B, P, L, NS, AS;
    const uint64_t * gibbs_off;         // [K+1]
    const uint64_t * path_off;          // [B+1]
    const uint32_t * path;              // [L]
    const uint64_t * noise_off;         // [B+1]
    const double * noise;               // [NS]
    const uint64_t * abund_off;         // [B+1]
    const word64 * abund;               // [AS]
    const uint64_t * cluster_path_off;  // [K+1]
    const double * total_count;         // [K]
    uint32_t * cluster_samples;         // [K] S_k
    uint64_t * cluster_noise_at;        // [K] noise_off[gibbs_off[k]]
    uint32_t * cluster_max_columns;     // [K] the columns of its widest block
    uint32_t * block_cluster;           // [B]
    uint32_t * block_base;              // [B] base_i
    uint32_t * block_list;              // [kRoutes * B] the blocks with samples of route r from r * B
    uint32_t * counters;                // [kCounters]
    word64 * bad;
    word64 * samples;                   // [P * N]
    uint8_t * listed;                   // [P]
    double * noise_counts;              // [N]
};

__device__ __forceinline__ void reportCluster(const TableArgs & a, const uint64_t cluster, const int why) { reportOffender(a.bad, cluster, why); }
__device__ __forceinline__ void reportBlock(const TableArgs & a, const uint64_t block, const int why) { reportOffender(a.bad, block, why, true); }

// thread i: cluster i, block i and path id i.  Every index is checked before it is used: the kernel is the validation, nothing it
// reads is trusted, and every write goes to a slot the checks have placed inside its array.
__global__ __launch_bounds__(kBlock) void describeKernel(const TableArgs a) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < a.K) {
        const uint64_t k = i;
        if (offsetsBad(a.gibbs_off, k, a.K, a.B)) reportCluster(a, k, kBadGibbsOff);
        else if (offsetsBad(a.cluster_path_off, k, a.K, a.P)) reportCluster(a, k, kBadClusterPathOff);
        else if (a.B == 0) {  // (no noise_off to read)
            a.cluster_samples[k] = 0;
            a.cluster_noise_at[k] = 0;
        } else {
            const uint64_t n0 = a.noise_off[a.gibbs_off[k]], n1 = a.noise_off[a.gibbs_off[k + 1]];
            uint32_t samples = 0;
            if (n0 <= n1 && n1 <= a.NS) {  // (a block's thread reports anything else)
                if (n1 - n0 > a.N) reportCluster(a, k, kBadTooManySamples);
                else samples = static_cast<uint32_t>(n1 - n0);
            }
            a.cluster_samples[k] = samples;
            a.cluster_noise_at[k] = n0;
        }
    }
    if (i < a.B) {
        const uint64_t b = i;
        const uint64_t k = lastAtMost(a.gibbs_off, a.K, b);
        const uint64_t g0 = a.gibbs_off[k];
        uint32_t base = 0;
        if (offsetsBad(a.path_off, b, a.B, a.L)) reportBlock(a, b, kBadPathOff);
        else if (offsetsBad(a.noise_off, b, a.B, a.NS)) reportBlock(a, b, kBadNoiseOff);
        else if (offsetsBad(a.abund_off, b, a.B, a.AS)) reportBlock(a, b, kBadAbundOff);
        else {
            const uint64_t c = a.path_off[b + 1] - a.path_off[b], n = a.noise_off[b + 1] - a.noise_off[b];  // both below 2^31
            if (a.abund_off[b + 1] - a.abund_off[b] != n * c) reportBlock(a, b, kBadAbundCount);
            if (g0 <= b) {
                const uint64_t first = a.noise_off[g0];
                if (first <= a.noise_off[b]) base = static_cast<uint32_t>(a.noise_off[b] - first);
                atomicMax(&a.cluster_max_columns[k], static_cast<uint32_t>(c));
            }
        }
        a.block_cluster[b] = static_cast<uint32_t>(k);
        a.block_base[b] = base;
    }
    if (i < a.L && a.B > 0) {
        const uint64_t b = lastAtMost(a.path_off, a.B, i);
        const uint64_t o0 = a.path_off[b], o1 = a.path_off[b + 1];
        if (o0 <= i && i < o1 && o1 <= a.L) {  // (the block's thread reports anything else)
            const uint64_t k = lastAtMost(a.gibbs_off, a.K, b);
            const uint64_t p0 = a.cluster_path_off[k], p1 = a.cluster_path_off[k + 1];
            if (p0 <= p1 && p1 <= a.P) {  // (the cluster's thread reports anything else)
                const uint32_t id = a.path[i];
                if (id >= p1 - p0) reportBlock(a, b, kBadPathId);
                else if (i > o0 && a.path[i - 1] >= id) reportBlock(a, b, kBadPathOrder);
                else if (a.noise_off[b + 1] > a.noise_off[b]) a.listed[p0 + id] = 1;  // (several blocks store the same byte: the same 1)
            }
        }
    }
}

// behind a describe pass without offence.  thread i: the route of cluster i; block i, when it has samples, onto its cluster's list
__global__ __launch_bounds__(kBlock) void routeKernel(const TableArgs a) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    int cluster_route = -1;
    if (i < a.K) {
        const uint64_t paths = a.cluster_path_off[i + 1] - a.cluster_path_off[i];
        cluster_route = routeOf(paths, a.cluster_max_columns[i]);
        if (cluster_route == kRouteGlobal) atomicMax(&a.counters[kGlobalMaxPaths], static_cast<uint32_t>(paths));
    }
    for (int route = 0; route < kRoutes; ++route) {
        const word64 with_route = __ballot(cluster_route == route);
        if (with_route != 0 && (threadIdx.x & 63) == __ffsll(static_cast<long long>(with_route)) - 1) {
            atomicAdd(&a.counters[kClustersOfRoute + route], static_cast<uint32_t>(__popcll(with_route)));
        }
    }
    int block_route = -1;
    if (i < a.B && a.noise_off[i + 1] > a.noise_off[i]) {
        const uint32_t k = a.block_cluster[i];
        if (k < a.K) block_route = routeOf(a.cluster_path_off[k + 1] - a.cluster_path_off[k], a.cluster_max_columns[k]);
    }
    appendToRouteList<kRoutes>(block_route, static_cast<uint32_t>(i), a.counters + kBlocksOfRoute, a.block_list, a.B);
}

// what a scatter kernel knows of its block
struct BlockItem {
    uint64_t p0, paths, n, c, abund_at, first_column;
    const uint32_t * ids;
    bool valid;
};

__device__ __forceinline__ BlockItem blockItem(const TableArgs & a, const int route, const uint32_t listed) {
    BlockItem item = {};
    item.valid = false;
    if (blockIdx.x >= listed) return item;
    const uint32_t b = a.block_list[static_cast<uint64_t>(route) * a.B + blockIdx.x];
    if (b >= a.B) return item;
    const uint32_t k = a.block_cluster[b];
    if (k >= a.K) return item;
    item.p0 = a.cluster_path_off[k];
    item.paths = a.cluster_path_off[k + 1] - item.p0;
    item.n = a.noise_off[b + 1] - a.noise_off[b];
    item.c = a.path_off[b + 1] - a.path_off[b];
    item.abund_at = a.abund_off[b];
    item.first_column = a.block_base[b];
    item.ids = a.path + a.path_off[b];
    item.valid = item.first_column + item.n <= a.N;
    return item;
}

// the resident route: one workgroup per block of the route's list
__global__ __launch_bounds__(kBlock) void residentKernel(const TableArgs a, const uint32_t listed) {
    __shared__ word64 s_piece[kSampleTile * stagedPitch(kResidentColumns)];
    static_assert(sizeof(word64) * kSampleTile * stagedPitch(kResidentColumns) == residentLdsBytes(kResidentColumns), "the plan's bytes");
    const BlockItem item = blockItem(a, kRouteResident, listed);
    if (!item.valid || item.c > kResidentColumns || item.paths > kResidentPaths) return;  // (uniform; not listed for this route)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t c = static_cast<uint32_t>(item.c), paths = static_cast<uint32_t>(item.paths), pitch = stagedPitch(c);
    const uint32_t my_id = lane < c ? item.ids[lane] : 0xffffffffu;
    const uint64_t tiles = tilesOf(item.n);
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint32_t ts = tileSamples(item.n, t);
        const word64 * __restrict__ piece = a.abund + item.abund_at + t * kSampleTile * c;
        if (t > 0) __syncthreads();  // the reads of the tile before
        for (uint32_t i = tid; i < ts * c; i += kBlock) {  // flat: consecutive threads, consecutive doubles
            const uint32_t s = i / c;
            s_piece[s * pitch + (i - s * c)] = piece[i];
        }
        __syncthreads();
        const uint64_t column = item.first_column + t * kSampleTile + lane;
        for (uint32_t p = wave; p < paths; p += kBlock / 64) {
            const word64 holder = __ballot(my_id == p);
            word64 value = 0;
            if (holder != 0 && lane < ts) value = s_piece[lane * pitch + (__ffsll(static_cast<long long>(holder)) - 1)];
            if (lane < ts) a.samples[(item.p0 + p) * a.N + column] = value;
        }
    }
}

// the first position of the ascending list ids[0 .. c) whose id is not below x
__device__ __forceinline__ uint64_t firstNotBelow(const uint32_t * __restrict__ ids, const uint64_t c, const uint64_t x) {
    uint64_t lo = 0, hi = c;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ids[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the global route: blockIdx.x a block of the route's list, blockIdx.y its first segment of kGlobalPaths paths; a wavefront per 64 paths
__global__ __launch_bounds__(kBlock) void globalKernel(const TableArgs a, const uint32_t listed) {
    const BlockItem item = blockItem(a, kRouteGlobal, listed);
    if (!item.valid) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t tiles = tilesOf(item.n);
    for (uint64_t segment = blockIdx.y; segment * kGlobalPaths < item.paths; segment += gridDim.y) {
        const uint64_t q0 = segment * kGlobalPaths + 64ull * wave;
        if (q0 >= item.paths) continue;
        const uint64_t q1 = q0 + 64 < item.paths ? q0 + 64 : item.paths;
        const uint64_t j0 = firstNotBelow(item.ids, item.c, q0), j1 = firstNotBelow(item.ids, item.c, q1);
        const uint64_t held = j1 - j0 < 64 ? j1 - j0 : 64;  // (ascending ids: at most one per path)
        const uint32_t my_id = lane < held ? item.ids[j0 + lane] : 0xffffffffu;
        for (uint64_t t = 0; t < tiles; ++t) {
            const uint32_t ts = tileSamples(item.n, t);
            const uint64_t sample = t * kSampleTile + lane, column = item.first_column + sample;
            for (uint64_t p = q0; p < q1; ++p) {
                const word64 holder = __ballot(my_id == p);
                word64 value = 0;
                if (holder != 0 && lane < ts) value = a.abund[item.abund_at + sample * item.c + j0 + (__ffsll(static_cast<long long>(holder)) - 1)];
                if (lane < ts) a.samples[(item.p0 + p) * a.N + column] = value;
            }
        }
    }
}

// a wavefront per path of the batch: the columns behind the samples of its cluster
__global__ __launch_bounds__(kBlock) void tailKernel(const TableArgs a) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(kBlock / 64) + (threadIdx.x >> 6);
    if (g >= a.P) return;
    const uint64_t k = lastAtMost(a.cluster_path_off, a.K, g);
    for (uint64_t column = a.cluster_samples[k] + (threadIdx.x & 63); column < a.N; column += 64) a.samples[g * a.N + column] = 0;
}

// lane s: the chain of sample column s over the clusters in ascending order.  The cluster's numbers are uniform (scalar loads),
// the noise sample of lane s lies beside that of lane s + 1.  A lane's addend is ONE load from a selected address, its noise sample
// or the cluster's total_count, so nothing branches between the loads of a round and all of them are in flight together (with a
// branch per cluster the kernel took 160 ns per cluster, 0.8 ms at 5 000 clusters, whatever the depth of the prefetch).
__global__ __launch_bounds__(64) void noiseKernel(const TableArgs a) {
    constexpr int kAhead = 32;
    const uint64_t s = blockIdx.x * 64ull + threadIdx.x;
    if (s >= a.N) return;
    double sum = 0.0;
    if (a.K > 0) {
        double held[kAhead], next[kAhead];
        const uint64_t last = a.K - 1;
        const auto load = [&](const uint64_t k) -> double {
            const uint64_t kk = k < last ? k : last;  // (beyond the last cluster: loaded, never added)
            const double * from = s < a.cluster_samples[kk] ? a.noise + (a.cluster_noise_at[kk] + s) : a.total_count + kk;
            return *from;
        };
#pragma unroll
        for (int u = 0; u < kAhead; ++u) held[u] = load(u);
        for (uint64_t k0 = 0; k0 < a.K; k0 += kAhead) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) next[u] = load(k0 + kAhead + u);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (k0 + u < a.K) sum += held[u];
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) held[u] = next[u];
        }
    }
    a.noise_counts[s] = sum;
}

struct TableInputs {
    uint32_t K = 0, N = 0;
    uint64_t B = 0, P = 0, L = 0, NS = 0, AS = 0;
    Source<uint64_t> gibbs_off, path_off, noise_off, abund_off, cluster_path_off;
    Source<uint32_t> path;
    Source<double> noise, abund, total_count;
};

const char * const kReasons[] = {"",
                                 "gibbs_off is not a non-decreasing sequence of offsets from 0 to num_blocks",
                                 "cluster_path_off is not a non-decreasing sequence of offsets from 0 to num_paths",
                                 "more samples than num_gibbs_samples",
                                 "gibbs_path_off is not a non-decreasing sequence of offsets from 0 to num_path_ids",
                                 "gibbs_noise_off is not a non-decreasing sequence of offsets from 0 to num_noise_samples",
                                 "gibbs_abund_off is not a non-decreasing sequence of offsets from 0 to num_abundance_samples",
                                 "the abundance samples are not samples x columns",
                                 "a path id is not below the cluster's number of paths",
                                 "the path ids do not ascend strictly"};

int buildTable(rpvg_hip_ctx * ctx, const TableInputs & in, const char * who, rpvg_hip_gibbs_table ** table_out) {
    const uint32_t K = in.K, N = in.N;
    const uint64_t B = in.B, P = in.P;
    RPVG_REQUIRE(N >= 1, "%s: num_gibbs_samples is 0", who);
    RPVG_REQUIRE(sizesFit(K, B, P, N, in.L, in.NS, in.AS) && tableFits(P, N),
                 "%s: %u clusters, %llu blocks, %llu paths x %u samples, %llu path ids, %llu noise samples, %llu abundance samples exceed one table", who, K,
                 static_cast<unsigned long long>(B), static_cast<unsigned long long>(P), N, static_cast<unsigned long long>(in.L),
                 static_cast<unsigned long long>(in.NS), static_cast<unsigned long long>(in.AS));
    RPVG_REQUIRE(K > 0 || (B == 0 && P == 0), "%s: blocks or paths without clusters", who);
    RPVG_REQUIRE(B > 0 || (in.L == 0 && in.NS == 0 && in.AS == 0), "%s: path ids or samples without blocks", who);
    RPVG_REQUIRE(K == 0 || (in.gibbs_off.from && in.cluster_path_off.from && in.total_count.from), "%s: NULL array", who);
    RPVG_REQUIRE(B == 0 || (in.path_off.from && in.noise_off.from && in.abund_off.from), "%s: NULL array", who);
    RPVG_REQUIRE((in.L == 0 || in.path.from) && (in.NS == 0 || in.noise.from) && (in.AS == 0 || in.abund.from), "%s: NULL array", who);
    std::unique_ptr<rpvg_hip_gibbs_table> t(new (std::nothrow) rpvg_hip_gibbs_table());
    if (!t) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    t->num_clusters = K;
    t->num_gibbs_samples = N;
    t->num_blocks = B;
    t->num_paths = P;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    UploadPack inputs;
    DeviceBuffer<uint64_t> gibbs_off, path_off, noise_off, abund_off, cluster_path_off, cluster_noise_at;
    DeviceBuffer<uint32_t> path, cluster_samples, cluster_max_columns, block_cluster, block_base, block_list, counters;
    DeviceBuffer<double> noise, abund, total_count;
    DeviceBuffer<word64> d_bad;
    takeInput(inputs, gibbs_off, in.gibbs_off, K ? static_cast<size_t>(K) + 1 : 0);
    takeInput(inputs, path_off, in.path_off, B ? B + 1 : 0);
    takeInput(inputs, path, in.path, in.L);
    takeInput(inputs, noise_off, in.noise_off, B ? B + 1 : 0);
    takeInput(inputs, noise, in.noise, in.NS);
    takeInput(inputs, abund_off, in.abund_off, B ? B + 1 : 0);
    takeInput(inputs, abund, in.abund, in.AS);
    takeInput(inputs, cluster_path_off, in.cluster_path_off, K ? static_cast<size_t>(K) + 1 : 0);
    takeInput(inputs, total_count, in.total_count, K);
    inputs.add(d_bad, &kNoBad, 1);
    inputs.addZero(counters, kCounters);
    inputs.addZero(cluster_max_columns, K);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    RPVG_HIP_CHECK(cluster_samples.alloc(K));
    RPVG_HIP_CHECK(cluster_noise_at.alloc(K));
    RPVG_HIP_CHECK(block_cluster.alloc(B));
    RPVG_HIP_CHECK(block_base.alloc(B));
    RPVG_HIP_CHECK(block_list.alloc(static_cast<size_t>(kRoutes) * B));
    const size_t listed_bytes = (static_cast<size_t>(P) + 3) & ~size_t(3);
    RPVG_HIP_CHECK(t->listed.alloc(listed_bytes));
    RPVG_HIP_CHECK(t->noise_counts.alloc(N));
    if (t->samples.alloc(static_cast<size_t>(P) * N) != hipSuccess) {
        (void) hipGetLastError();
        (void) hipDeviceSynchronize();
        setError("%s: no device memory for a table of %llu paths x %u samples", who, static_cast<unsigned long long>(P), N);
        return RPVG_HIP_ERR_ALLOC;
    }
    if (listed_bytes) RPVG_HIP_CHECK(zeroAsync(t->listed.ptr, listed_bytes, st));

    TableArgs a;
    a.K = K;
    a.N = N;
    a.B = B;
    a.P = P;
    a.L = in.L;
    a.NS = in.NS;
    a.AS = in.AS;
    a.gibbs_off = gibbs_off.ptr;
    a.path_off = path_off.ptr;
    a.path = path.ptr;
    a.noise_off = noise_off.ptr;
    a.noise = noise.ptr;
    a.abund_off = abund_off.ptr;
    a.abund = reinterpret_cast<const word64 *>(abund.ptr);
    a.cluster_path_off = cluster_path_off.ptr;
    a.total_count = total_count.ptr;
    a.cluster_samples = cluster_samples.ptr;
    a.cluster_noise_at = cluster_noise_at.ptr;
    a.cluster_max_columns = cluster_max_columns.ptr;
    a.block_cluster = block_cluster.ptr;
    a.block_base = block_base.ptr;
    a.block_list = block_list.ptr;
    a.counters = counters.ptr;
    a.bad = d_bad.ptr;
    a.samples = t->samples.ptr;
    a.listed = t->listed.ptr;
    a.noise_counts = t->noise_counts.ptr;

    SpanScope span(ctx, FAM_BUILD);
    if (K > 0) {
        const uint64_t threads = std::max<uint64_t>(std::max<uint64_t>(K, B), in.L);
        describeKernel<<<gridFor(threads), dim3(kBlock), 0, st>>>(a);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
        word64 bad = kNoBad;
        if (const int rc = fetchDescribed(st, d_bad.ptr, &bad)) return rc;
        if (bad != kNoBad) {
            span.end();
            const Offender o = offenderOf(bad, kBadPathOrder);
            setError("%s: %s %llu: %s", who, o.second_kind ? "block" : "cluster", static_cast<unsigned long long>(o.index), kReasons[o.why]);
            return RPVG_HIP_ERR_INVALID;
        }
        routeKernel<<<gridFor(std::max<uint64_t>(K, B)), dim3(kBlock), 0, st>>>(a);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
        uint32_t counted[kCounters] = {};
        RPVG_HIP_CHECK(hipMemcpyAsync(counted, counters.ptr, sizeof(counted), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        const uint32_t resident_blocks = counted[kBlocksOfRoute + kRouteResident], global_blocks = counted[kBlocksOfRoute + kRouteGlobal];
        if (static_cast<uint64_t>(counted[kClustersOfRoute + kRouteResident]) + counted[kClustersOfRoute + kRouteGlobal] != K ||
            static_cast<uint64_t>(resident_blocks) + global_blocks > B) {
            span.end();
            (void) hipDeviceSynchronize();
            setError("%s: %u + %u clusters routed of %u, %u + %u blocks listed of %llu", who, counted[kClustersOfRoute + kRouteResident],
                     counted[kClustersOfRoute + kRouteGlobal], K, resident_blocks, global_blocks, static_cast<unsigned long long>(B));
            return RPVG_HIP_ERR_RUNTIME;
        }
        for (int r = 0; r < kRoutes; ++r) t->clusters_by_route[r] = counted[kClustersOfRoute + r];
        if (resident_blocks) {
            residentKernel<<<dim3(resident_blocks), dim3(kBlock), 0, st>>>(a, resident_blocks);
            ctx->stats.build_launches += 1;
        }
        if (global_blocks) {
            globalKernel<<<dim3(global_blocks, globalGridY(counted[kGlobalMaxPaths])), dim3(kBlock), 0, st>>>(a, global_blocks);
            ctx->stats.build_launches += 1;
        }
        if (P) {
            tailKernel<<<gridFor(P, kBlock / 64), dim3(kBlock), 0, st>>>(a);
            ctx->stats.build_launches += 1;
        }
        RPVG_HIP_CHECK(hipGetLastError());
    }
    noiseKernel<<<gridFor(N, 64), dim3(64), 0, st>>>(a);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    span.end();
    t->h_cluster_path_off.assign(static_cast<size_t>(K) + 1, 0);
    if (K > 0 && in.cluster_path_off.on_device) {
        RPVG_HIP_CHECK(hipMemcpyAsync(t->h_cluster_path_off.data(), cluster_path_off.ptr, (static_cast<size_t>(K) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    } else if (K > 0) {
        std::copy(in.cluster_path_off.from, in.cluster_path_off.from + K + 1, t->h_cluster_path_off.begin());
    }
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    *table_out = t.release();
    return RPVG_HIP_OK;
}

}  // namespace

// for table_text.hip
rpvg_hip_detail::GibbsTableResident rpvg_hip_detail::residentOf(const rpvg_hip_gibbs_table * table) {
    return GibbsTableResident{table->num_clusters, table->num_gibbs_samples, table->num_paths, reinterpret_cast<const double *>(table->samples.ptr),
                              table->listed.ptr, table->h_cluster_path_off.data()};
}

extern "C" {

void rpvg_hip_gibbs_table_limits(rpvg_gibbs_table_limits * limits_out) {
    if (!limits_out) return;
    limits_out->resident_paths = kResidentPaths;
    limits_out->resident_columns = kResidentColumns;
    limits_out->sample_tile = kSampleTile;
    limits_out->global_paths = kGlobalPaths;
    limits_out->resident_lds_bytes = static_cast<uint32_t>(residentLdsBytes(kResidentColumns));
}

int rpvg_hip_gibbs_table_build(rpvg_hip_ctx * ctx, const rpvg_gibbs_flat * flat, rpvg_hip_gibbs_table ** table_out) {
    RPVG_REQUIRE(ctx && flat && table_out, "rpvg_hip_gibbs_table_build: NULL argument");
    *table_out = nullptr;
    const bool on_device = flat->on_device != 0;
    TableInputs in;
    in.K = flat->num_clusters;
    in.N = flat->num_gibbs_samples;
    in.B = flat->num_blocks;
    in.P = flat->num_paths;
    in.L = flat->num_path_ids;
    in.NS = flat->num_noise_samples;
    in.AS = flat->num_abundance_samples;
    in.gibbs_off = {flat->gibbs_off, on_device};
    in.path_off = {flat->gibbs_path_off, on_device};
    in.path = {flat->gibbs_path, on_device};
    in.noise_off = {flat->gibbs_noise_off, on_device};
    in.noise = {flat->gibbs_noise, on_device};
    in.abund_off = {flat->gibbs_abund_off, on_device};
    in.abund = {flat->gibbs_abund, on_device};
    in.cluster_path_off = {flat->cluster_path_off, on_device};
    in.total_count = {flat->total_count, on_device};
    return buildTable(ctx, in, "rpvg_hip_gibbs_table_build", table_out);
}

int rpvg_hip_gibbs_table_build_resident(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_samples * samples, const rpvg_hip_em_problems * problems,
                                        uint32_t num_clusters, const uint64_t * cluster_path_off, const double * total_count,
                                        uint32_t num_gibbs_samples, rpvg_hip_gibbs_table ** table_out) {
    const char * const who = "rpvg_hip_gibbs_table_build_resident";
    RPVG_REQUIRE(ctx && samples && problems && table_out, "%s: NULL argument", who);
    *table_out = nullptr;
    const uint32_t B = problems->num_problems;
    RPVG_REQUIRE(samples->num_problems == B, "%s: %u problems, the samples are those of %u", who, B, samples->num_problems);
    RPVG_REQUIRE(B == 0 || (problems->cluster && problems->col_off && problems->col_path), "%s: NULL problem arrays", who);
    RPVG_REQUIRE(num_clusters == 0 || (cluster_path_off && total_count), "%s: NULL array", who);
    RPVG_REQUIRE(samples->sample_off.size() == static_cast<size_t>(B) + 1 && samples->abund_sample_off.size() == static_cast<size_t>(B) + 1,
                 "%s: the handle's offsets do not match its problems", who);
    std::vector<uint64_t> gibbs_off(static_cast<size_t>(num_clusters) + 1, 0);
    for (uint32_t p = 0; p < B; ++p) {
        RPVG_REQUIRE(problems->cluster[p] < num_clusters, "%s: problem %u: cluster %u of %u", who, p, problems->cluster[p], num_clusters);
        RPVG_REQUIRE(p == 0 || problems->cluster[p - 1] <= problems->cluster[p], "%s: problem %u: its cluster %u is below its predecessor's %u", who, p,
                     problems->cluster[p], problems->cluster[p - 1]);
        gibbs_off[problems->cluster[p] + 1] += 1;
    }
    for (uint32_t k = 0; k < num_clusters; ++k) gibbs_off[k + 1] += gibbs_off[k];
    TableInputs in;
    in.K = num_clusters;
    in.N = num_gibbs_samples;
    in.B = B;
    in.P = num_clusters ? cluster_path_off[num_clusters] : 0;
    in.L = B ? problems->col_off[B] : 0;
    in.NS = samples->sample_off[B];
    in.AS = samples->abund_sample_off[B];
    in.gibbs_off = {gibbs_off.data(), false};
    in.path_off = {problems->col_off, false};
    in.path = {problems->col_path, false};
    in.noise_off = {samples->sample_off.data(), false};
    in.noise = {samples->d_noise_samples.ptr, true};
    in.abund_off = {samples->abund_sample_off.data(), false};
    in.abund = {samples->d_abund_samples.ptr, true};
    in.cluster_path_off = {cluster_path_off, false};
    in.total_count = {total_count, false};
    return buildTable(ctx, in, who, table_out);
}

int rpvg_hip_gibbs_table_view(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table, rpvg_gibbs_table_view * view) {
    RPVG_REQUIRE(ctx && table && view, "rpvg_hip_gibbs_table_view: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!table->downloaded) {
        const size_t cells = static_cast<size_t>(table->num_paths) * table->num_gibbs_samples;
        try {
            table->h_samples.assign(cells, 0.0);
            table->h_listed.assign(table->num_paths, 0);
            table->h_noise_counts.assign(table->num_gibbs_samples, 0.0);
        } catch (const std::bad_alloc &) {
            setError("rpvg_hip_gibbs_table_view: out of host memory for %llu paths x %u samples (rpvg_hip_gibbs_table_rows takes a range)",
                     static_cast<unsigned long long>(table->num_paths), table->num_gibbs_samples);
            return RPVG_HIP_ERR_ALLOC;
        }
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        if (cells) RPVG_HIP_CHECK(hipMemcpyAsync(table->h_samples.data(), table->samples.ptr, cells * sizeof(double), hipMemcpyDeviceToHost, st));
        if (table->num_paths) RPVG_HIP_CHECK(hipMemcpyAsync(table->h_listed.data(), table->listed.ptr, table->num_paths, hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipMemcpyAsync(table->h_noise_counts.data(), table->noise_counts.ptr, table->num_gibbs_samples * sizeof(double), hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        table->downloaded = true;
    }
    std::memset(view, 0, sizeof(*view));
    view->num_clusters = table->num_clusters;
    view->num_blocks = table->num_blocks;
    view->num_paths = table->num_paths;
    view->num_gibbs_samples = table->num_gibbs_samples;
    view->samples = table->h_samples.data();
    view->listed = table->h_listed.data();
    view->noise_counts = table->h_noise_counts.data();
    view->cluster_path_off = table->h_cluster_path_off.data();
    for (int r = 0; r < kRoutes; ++r) view->clusters_by_route[r] = table->clusters_by_route[r];
    return RPVG_HIP_OK;
}

int rpvg_hip_gibbs_table_rows(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table, uint64_t first_path, uint64_t num_paths, double * rows_out) {
    RPVG_REQUIRE(ctx && table, "rpvg_hip_gibbs_table_rows: NULL argument");
    RPVG_REQUIRE(first_path <= table->num_paths && num_paths <= table->num_paths - first_path, "rpvg_hip_gibbs_table_rows: %llu paths from %llu of %llu",
                 static_cast<unsigned long long>(num_paths), static_cast<unsigned long long>(first_path), static_cast<unsigned long long>(table->num_paths));
    if (num_paths == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(rows_out, "rpvg_hip_gibbs_table_rows: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = table->num_gibbs_samples;
    RPVG_HIP_CHECK(hipMemcpyAsync(rows_out, table->samples.ptr + first_path * N, num_paths * N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

void rpvg_hip_gibbs_table_free(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table) {
    if (!table) return;
    waitAndDelete(ctx);
    delete table;
}

}  // extern "C"
