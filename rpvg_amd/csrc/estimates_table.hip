// estimates_table.hip — the estimates of a batch as the table rpvg reports: per path the haplotype probability, read count and
// transcript count, per set member its transcript count, per cluster its part of the TPM denominator, the totals of the `Unknown`
// rows, and the TPMs for a denominator (interface include/rpvg_table.h).
//
// Takes over   totalTranscriptCount, the TPM denominator                              src/main.cpp:1029-1057
//              the per-path accumulation of HaplotypeAbundanceEstimatesWriter         src/threaded_output_writer.cpp:346-432
//              the per-member transcript counts and TPMs of the joint writer          src/threaded_output_writer.cpp:434-546
//              the noise sums of AbundanceEstimatesWriter and of the joint writer     src/threaded_output_writer.cpp:283-343, :434-546
//
// Arithmetic   Every sum is a chain of plain IEEE additions in the order rpvg_table.h states; every quotient is one IEEE division.  There
//              is no multiply-then-add anywhere in this file, so the compiler has nothing to contract into a fused multiply-add (the
//              TPM is a division followed by a multiplication); the pragma below keeps it that way should one ever appear.  No
//              floating-point atomic is used: the only atomics count integers (the histogram of a counting sort in LDS, the lengths
//              of the work lists, the first offender of the validation).
// Describe     one kernel behind the copy validates the offsets, the members and the abundance counts (the first offending cluster
//              comes back; the host words the message), writes the work list of every route (the offsets may be device memory: the
//              host cannot plan from them) and, per member, its set, whether it counts for the haplotype probability, its
//              transcript count and whether that takes part in the cluster's sum.
// Routes       by the cluster's numbers of paths and members (estimates_plan.hpp):
//                wavefront / workgroup   the members are placed into per-path slot ranges by a STABLE counting sort in LDS — an integer
//                                        histogram by path, a scan, then placement chunk by chunk of 64 members in member order, the rank
//                                        inside a chunk from ballots over the bits of the path — so a path's slots hold its memberships
//                                        in (set, member) order; every lane then owns paths and adds its list sequentially, and the last
//                                        wavefront adds the cluster's transcript count over the members in order (one chain);
//                global                  a stable radix sort of the member positions by the batch-wide path slot, a lane per path that adds
//                                        its run sequentially, a wavefront per cluster for its transcript count (one chain).
// Totals       a single wavefront adds the K cluster counts and the two noise sums in ascending cluster order: the lanes load 256
//              clusters ahead, the additions are one chain.
// No kernel allocates; every array is sized by K, S, M or P.

#include "device_algos.hpp"
#include "estimates_plan.hpp"
#include "table_kit.hpp"
#include "table_residents.hpp"
#include "../../include/rpvg_table.h"

#pragma clang fp contract(off)

using namespace rpvg_hip_detail;
using namespace rpvg_estimates;

// the table of a batch: one device block (DownloadPack) and its host copies
struct rpvg_hip_estimates_table {
    uint32_t num_clusters = 0, ploidy = 0;
    uint64_t num_paths = 0, num_members = 0;
    DownloadPack pack;
    DeviceBuffer<double> haplotype_prob, read_count, transcript_count, tpm;  // [P]
    DeviceBuffer<double> member_transcript_count, member_tpm;                // [M]
    DeviceBuffer<double> cluster_transcript_count;                           // [K]
    DeviceBuffer<double> scalars;                                            // total_transcript_count, noise_count_total, noise_count_share_total
    std::vector<double> h_haplotype_prob, h_read_count, h_transcript_count, h_tpm, h_member_transcript_count, h_member_tpm,
                        h_cluster_transcript_count, h_scalars;
    uint32_t clusters_by_route[kRoutes] = {0, 0, 0};
    double denominator = 0.0;
    bool has_tpm = false, downloaded = false;
};

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kCounted = 1u << 31;    // member info: the member adds its set's posterior to its path
constexpr uint32_t kPositive = 1u << 30;   // ... its transcript count takes part in the cluster's sum (abundances and eff > 0)
constexpr uint32_t kSetMask = kPositive - 1u;
constexpr uint64_t kMaxSets = kSetMask, kMaxItems = 0x7fffffffull;

// bad = min over the offending clusters (table_kit.hpp)
enum TableBad { kBadSetOff = 1, kBadPathOff = 2, kBadAbundOff = 3, kBadMemberOff = 4, kBadMember = 5, kBadAbundCount = 6 };

struct TableArgs {
    uint32_t K;
    uint64_t S, M, A, P;
    const uint64_t * set_off;       // [K+1]
    const uint64_t * member_off;    // [S+1]
    const uint32_t * members;       // [M]
    const double * posteriors;      // [S]
    const uint64_t * abund_off;     // [K+1]
    const double * abundances;      // [A]
    const double * noise_count;     // [K]
    const uint64_t * cluster_path_off;  // [K+1]
    const double * eff;             // [P]
    uint32_t * info;                // [M] set | kCounted | kPositive
    uint32_t * key;                 // [M] the batch-wide path slot of a member of a cluster of the global route, P otherwise
    uint32_t * position;            // [M] m
    uint32_t * route_list;          // [kRoutes * K] the clusters of route r from r * K
    uint32_t * counters;            // [kRoutes] their numbers
    unsigned long long * bad;
    double * haplotype_prob, * read_count, * transcript_count;  // [P]
    double * member_transcript_count;                           // [M]
    double * cluster_transcript_count;                          // [K]
};

__device__ __forceinline__ void reportBad(const TableArgs & a, const uint64_t cluster, const int why) { reportOffender(a.bad, cluster, why); }

// thread i: cluster i, set i (and the end of member_off) and member i.  Every index is checked before it is used: the kernel is the
// validation, nothing it reads is trusted.
__global__ __launch_bounds__(kBlock) void describeKernel(const TableArgs a) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    int my_route = -1;  // of cluster i, when it is valid
    if (i < a.K) {
        const uint64_t k = i;
        const uint64_t s0 = a.set_off[k], s1 = a.set_off[k + 1], a0 = a.abund_off[k], a1 = a.abund_off[k + 1];
        const uint64_t p0 = a.cluster_path_off[k], p1 = a.cluster_path_off[k + 1];
        int why = 0;
        if (offsetsBad(a.set_off, k, a.K, a.S)) why = kBadSetOff;
        else if (offsetsBad(a.cluster_path_off, k, a.K, a.P)) why = kBadPathOff;
        else if (offsetsBad(a.abund_off, k, a.K, a.A)) why = kBadAbundOff;
        else {
            const uint64_t m0 = a.member_off[s0], m1 = a.member_off[s1];
            if (m0 > m1 || m1 > a.M) why = kBadMemberOff;
            else if (a1 != a0 && a1 - a0 != m1 - m0) why = kBadAbundCount;
            else my_route = routeOf(p1 - p0, m1 - m0);
        }
        if (why) reportBad(a, k, why);
    }
    appendToRouteList<kRoutes>(my_route, static_cast<uint32_t>(i), a.counters, a.route_list, a.K);  // the work lists
    if (i <= a.S) {
        const uint64_t s = i;
        bool bad = false;
        if (s < a.S && (a.member_off[s] > a.member_off[s + 1] || a.member_off[s + 1] > a.M)) bad = true;
        if (s == 0 && a.member_off[0] != 0) bad = true;
        if (s == a.S && a.member_off[a.S] != a.M) bad = true;
        if (bad) reportBad(a, lastAtMost(a.set_off, a.K, s), kBadMemberOff);
    }
    if (i < a.M) {
        const uint64_t m = i;
        uint32_t info = 0, key = static_cast<uint32_t>(a.P);
        double value = 0.0;
        if (a.S > 0) {
            const uint64_t s = lastAtMost(a.member_off, a.S, m);
            const uint64_t k = lastAtMost(a.set_off, a.K, s);
            const uint64_t p0 = a.cluster_path_off[k], p1 = a.cluster_path_off[k + 1];
            const uint64_t s0 = a.set_off[k], s1 = a.set_off[k + 1];
            const uint32_t local = a.members[m];
            if (p0 <= p1 && p1 <= a.P && s0 <= s1 && s1 <= a.S) {  // (the cluster's thread reports these)
                if (local >= p1 - p0) {
                    reportBad(a, k, kBadMember);
                } else {
                    const uint64_t g = p0 + local;
                    const uint64_t set_begin = a.member_off[s], m0 = a.member_off[s0], m1 = a.member_off[s1];
                    const uint64_t a0 = a.abund_off[k], a1 = a.abund_off[k + 1];
                    info = static_cast<uint32_t>(s);
                    if (m == set_begin || (m > 0 && a.members[m - 1] != local)) info |= kCounted;
                    if (a1 > a0 && a1 <= a.A && m >= m0 && m - m0 < a1 - a0) {
                        const double e = a.eff[g];
                        if (e > 0) {
                            value = a.abundances[a0 + (m - m0)] / e;
                            info |= kPositive;
                        }
                    }
                    if (m0 <= m1 && routeOf(p1 - p0, m1 - m0) == kRouteGlobal) key = static_cast<uint32_t>(g);
                }
            }
        }
        a.info[m] = info;
        a.key[m] = key;
        a.position[m] = static_cast<uint32_t>(m);
        a.member_transcript_count[m] = value;
    }
}

// what a path's list adds up to, and the path's row of the table
struct PathSums {
    double haplotype_prob = 0.0, read_count = 0.0;
    __device__ __forceinline__ void add(const TableArgs & a, const uint64_t m, const bool has_abundances, const uint64_t abundance_at) {
        const uint32_t info = a.info[m];
        if (info & kCounted) haplotype_prob += a.posteriors[info & kSetMask];
        if (has_abundances) read_count += a.abundances[abundance_at];
    }
    __device__ __forceinline__ void store(const TableArgs & a, const uint64_t g) const {
        const double e = a.eff[g];
        a.haplotype_prob[g] = haplotype_prob;
        a.read_count[g] = read_count;
        a.transcript_count[g] = e > 0 ? read_count / e : 0.0;
    }
};

// acc + the values of the lanes whose bit of `take` is set, in lane order: ONE chain of additions, carried by every lane alike.
// The values come out of the lanes' registers (v_readlane with the lane a constant of the unrolled loop), so nothing but the
// additions themselves is on the chain; `take` is uniform, the branches are scalar.
__device__ __forceinline__ double addLanesInOrder(double acc, const double value, const unsigned long long take) {
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const double x = readLaneF64(value, j);
        if ((take >> j) & 1ull) acc += x;
    }
    return acc;
}

// clusterTranscriptCount (rpvg_amd/host/device_group.cpp), addition for addition: the members in order, those with eff > 0 only.
// Called by a whole wavefront: the lanes load 64 members at a time (the next 64 before the chain over the ones they hold), the
// chain is one (a single lane that loads and adds took 150 ns per member: 1.2 ms for a cluster at the workgroup limit).
__device__ __forceinline__ double clusterSum(const TableArgs & a, const uint64_t m0, const uint64_t m1, const uint32_t lane) {
    double sum = 0.0;
    uint64_t m = m0 + lane;
    bool positive = m < m1 && (a.info[m] & kPositive);
    double value = m < m1 ? a.member_transcript_count[m] : 0.0;
    for (uint64_t c0 = m0; c0 < m1; c0 += 64) {
        const uint64_t next = c0 + 64 + lane;
        const bool next_positive = next < m1 && (a.info[next] & kPositive);
        const double next_value = next < m1 ? a.member_transcript_count[next] : 0.0;
        sum = addLanesInOrder(sum, value, __ballot(positive));
        positive = next_positive;
        value = next_value;
    }
    return sum;
}

// one workgroup per cluster of the route's list
template <int BLOCK, uint32_t MAX_PATHS, uint32_t MAX_MEMBERS>
__global__ __launch_bounds__(BLOCK) void residentKernel(const TableArgs a, const int route, const uint32_t listed) {
    __shared__ uint32_t s_end[MAX_PATHS];      // histogram -> begin of every path's slots -> (after the placement) their end
    __shared__ uint32_t s_slot[MAX_MEMBERS];   // member positions relative to the cluster's first, by path, in member order
    __shared__ uint32_t s_scan[BLOCK / 64];
    static_assert(residentLdsBytes(MAX_PATHS, MAX_MEMBERS, BLOCK) <= kLdsStaticMax, "a static allocation");
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (blockIdx.x >= listed) return;
    const uint32_t k = a.route_list[static_cast<uint64_t>(route) * a.K + blockIdx.x];
    if (k >= a.K) return;
    const uint64_t p0 = a.cluster_path_off[k], s0 = a.set_off[k], s1 = a.set_off[k + 1];
    const uint64_t m0 = a.member_off[s0], a0 = a.abund_off[k];
    const uint64_t N64 = a.cluster_path_off[k + 1] - p0, M64 = a.member_off[s1] - m0;
    if (N64 > MAX_PATHS || M64 > MAX_MEMBERS) return;  // (not listed for this route)
    const uint32_t N = static_cast<uint32_t>(N64), Mk = static_cast<uint32_t>(M64);
    const bool has_abundances = a.abund_off[k + 1] > a0;

    for (uint32_t p = tid; p < N; p += BLOCK) s_end[p] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < Mk; i += BLOCK) {
        const uint32_t path = a.members[m0 + i];
        if (path < N) atomicAdd(&s_end[path], 1u);
    }
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t c0 = 0; c0 < N; c0 += BLOCK) {
        const uint32_t p = c0 + tid;
        const uint32_t count = p < N ? s_end[p] : 0u;
        uint32_t total;
        const uint32_t before = blockExclusiveSum<BLOCK>(count, total, s_scan);
        if (p < N) s_end[p] = run + before;
        run += total;
    }
    __syncthreads();
    if (tid < 64) {
        // the first wavefront places the members, 64 at a time in member order: a member's slot is the cursor of its path plus
        // the number of earlier lanes of the chunk with the same path
        const int bits = bitsFor(N);
        for (uint32_t c0 = 0; c0 < Mk; c0 += 64) {
            const uint32_t i = c0 + lane;
            const uint32_t path = i < Mk ? a.members[m0 + i] : 0u;
            const bool valid = i < Mk && path < N;
            unsigned long long same = __ballot(valid);
            for (int b = 0; b < bits; ++b) {
                const bool bit = (path >> b) & 1u;
                const unsigned long long with_bit = __ballot(bit);
                same &= bit ? with_bit : ~with_bit;
            }
            const uint32_t rank = __popcll(same & ((1ull << lane) - 1ull)), peers = __popcll(same);
            uint32_t begin = 0;
            if (valid) {
                begin = s_end[path];
                if (begin + rank < Mk) s_slot[begin + rank] = i;
            }
            __builtin_amdgcn_wave_barrier();  // every lane has read its cursor
            if (valid && rank + 1 == peers) s_end[path] = begin + peers;
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    for (uint32_t p = tid; p < N; p += BLOCK) {
        const uint32_t q0 = p ? s_end[p - 1] : 0u, q1 = min(s_end[p], Mk);
        PathSums sums;
        for (uint32_t q = q0; q < q1; ++q) {
            const uint32_t i = s_slot[q];
            if (i < Mk) sums.add(a, m0 + i, has_abundances, a0 + i);
        }
        sums.store(a, p0 + p);
    }
    if (tid >= BLOCK - 64) {  // the last wavefront, all of its lanes
        const double sum = clusterSum(a, m0, m0 + Mk, lane);
        if (lane == 63) a.cluster_transcript_count[k] = sum;
    }
}

// the global route: a lane per path of the batch; the paths of the clusters of the other routes have their rows
__global__ __launch_bounds__(kBlock) void globalPathsKernel(const TableArgs a, const uint32_t * __restrict__ key_sorted,
                                                            const uint32_t * __restrict__ position_sorted) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (g >= a.P) return;
    const uint64_t k = lastAtMost(a.cluster_path_off, a.K, g);
    const uint64_t p0 = a.cluster_path_off[k], p1 = a.cluster_path_off[k + 1];
    if (g < p0 || g >= p1) return;
    const uint64_t m0 = a.member_off[a.set_off[k]], m1 = a.member_off[a.set_off[k + 1]], a0 = a.abund_off[k];
    if (routeOf(p1 - p0, m1 - m0) != kRouteGlobal) return;
    const bool has_abundances = a.abund_off[k + 1] > a0;
    uint64_t lo = 0, hi = a.M;  // the first sorted member of path g
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (key_sorted[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    PathSums sums;
    for (uint64_t q = lo; q < a.M && key_sorted[q] == g; ++q) {
        const uint64_t m = position_sorted[q];
        if (m >= m0 && m < m1) sums.add(a, m, has_abundances, a0 + (m - m0));
    }
    sums.store(a, g);
}

__global__ __launch_bounds__(kBlock) void globalClustersKernel(const TableArgs a, const uint32_t listed) {
    const uint32_t t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // a wavefront per cluster
    if (t >= listed) return;
    const uint32_t k = a.route_list[static_cast<uint64_t>(kRouteGlobal) * a.K + t];
    if (k >= a.K) return;
    const double sum = clusterSum(a, a.member_off[a.set_off[k]], a.member_off[a.set_off[k + 1]], lane);
    if (lane == 0) a.cluster_transcript_count[k] = sum;
}

// one wavefront: the three totals in ascending cluster order.  The lanes hold 256 clusters and load the next 256 before the
// chains of additions over the ones they hold (with 64 in flight the kernel waited for memory: 32 ns per cluster); every lane carries the same three chains (the values come out of the lanes'
// registers by v_readlane, so only the additions are on a chain: reading them by a shuffle with a loop index took 62 ns per
// cluster, 3 ms at 47 640 clusters), lane 0 stores them.
__global__ __launch_bounds__(64) void totalsKernel(const uint32_t K, const double * __restrict__ cluster_transcript_count,
                                                   const double * __restrict__ noise_count, const double ploidy, double * __restrict__ scalars) {
    constexpr int kAhead = 4;  // chunks of 64 clusters a lane holds: the loads of the next four are in flight during the chains over these
    const uint32_t lane = threadIdx.x;
    double total = 0.0, noise_total = 0.0, share_total = 0.0;
    double count[kAhead], noise[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
        const uint64_t at = 64ull * u + lane;
        count[u] = at < K ? cluster_transcript_count[at] : 0.0;
        noise[u] = at < K ? noise_count[at] : 0.0;
    }
    for (uint64_t c0 = 0; c0 < K; c0 += 64 * kAhead) {
        double next_count[kAhead], next_noise[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const uint64_t at = c0 + 64ull * (kAhead + u) + lane;
            next_count[u] = at < K ? cluster_transcript_count[at] : 0.0;
            next_noise[u] = at < K ? noise_count[at] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const uint64_t base = c0 + 64ull * u;
            if (base >= K) break;
            const double share = noise[u] / ploidy;
            if (K - base >= 64) {
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    total += readLaneF64(count[u], j);
                    noise_total += readLaneF64(noise[u], j);
                    share_total += readLaneF64(share, j);
                }
            } else {
                const unsigned long long take = (1ull << (K - base)) - 1ull;  // the last clusters
                total = addLanesInOrder(total, count[u], take);
                noise_total = addLanesInOrder(noise_total, noise[u], take);
                share_total = addLanesInOrder(share_total, share, take);
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            count[u] = next_count[u];
            noise[u] = next_noise[u];
        }
    }
    if (lane == 0) {
        scalars[0] = total;
        scalars[1] = noise_total;
        scalars[2] = share_total;
    }
}

// the division, then the multiplication (`transcript_count / total_transcript_count * std::pow(10, 6)`)
__global__ __launch_bounds__(kBlock) void tpmKernel(const uint64_t P, const uint64_t M, const double denominator, const double * __restrict__ transcript_count,
                                                    const double * __restrict__ member_transcript_count, double * __restrict__ tpm,
                                                    double * __restrict__ member_tpm) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < P) {
        const double quotient = transcript_count[i] / denominator;
        tpm[i] = quotient * 1e6;
    } else if (i - P < M) {
        const double quotient = member_transcript_count[i - P] / denominator;
        member_tpm[i - P] = quotient * 1e6;
    }
}

const char * const kReasons[] = {"",
                                 "set_off is not a non-decreasing sequence of offsets from 0 to num_sets",
                                 "cluster_path_off is not a non-decreasing sequence of offsets from 0 to num_paths",
                                 "abund_off is not a non-decreasing sequence of offsets from 0 to num_abundances",
                                 "member_off is not a non-decreasing sequence of offsets from 0 to num_members",
                                 "a member is not below the cluster's number of paths",
                                 "the abundances are neither one per member nor none"};

}  // namespace

// for table_text.hip
rpvg_hip_detail::EstimatesTableResident rpvg_hip_detail::residentOf(const rpvg_hip_estimates_table * table) {
    return EstimatesTableResident{table->num_clusters, table->num_paths, table->num_members, table->has_tpm, table->haplotype_prob.ptr,
                                  table->read_count.ptr, table->tpm.ptr, table->member_tpm.ptr, table->ploidy};
}

extern "C" {

void rpvg_hip_estimates_table_limits(rpvg_estimates_table_limits * limits_out) {
    if (!limits_out) return;
    limits_out->wave_paths = kWavePaths;
    limits_out->wave_members = kWaveMembers;
    limits_out->lds_paths = kLdsPaths;
    limits_out->lds_members = kLdsMembers;
    limits_out->wave_lds_bytes = static_cast<uint32_t>(residentLdsBytes(kWavePaths, kWaveMembers, kWaveBlock));
    limits_out->lds_bytes = static_cast<uint32_t>(residentLdsBytes(kLdsPaths, kLdsMembers, kLdsBlock));
}

int rpvg_hip_estimates_table_build(rpvg_hip_ctx * ctx, const rpvg_estimates_flat * in, uint32_t ploidy, rpvg_hip_estimates_table ** table_out) {
    RPVG_REQUIRE(ctx && in && table_out, "rpvg_hip_estimates_table_build: NULL argument");
    *table_out = nullptr;
    const uint32_t K = in->num_clusters;
    const uint64_t S = in->num_sets, M = in->num_members, A = in->num_abundances, P = in->num_paths;
    RPVG_REQUIRE(ploidy >= 1, "rpvg_hip_estimates_table_build: a ploidy of 0");
    RPVG_REQUIRE(K <= kMaxItems && S <= kMaxSets && M <= kMaxItems && A <= kMaxItems && P <= kMaxItems,
                 "rpvg_hip_estimates_table_build: %u clusters, %llu sets, %llu members, %llu abundances, %llu paths exceed one table", K,
                 static_cast<unsigned long long>(S), static_cast<unsigned long long>(M), static_cast<unsigned long long>(A), static_cast<unsigned long long>(P));
    RPVG_REQUIRE(K > 0 || (S == 0 && M == 0 && A == 0 && P == 0), "rpvg_hip_estimates_table_build: sets, members, abundances or paths without clusters");
    RPVG_REQUIRE(K == 0 || (in->set_off && in->member_off && in->abund_off && in->noise_count && in->cluster_path_off),
                 "rpvg_hip_estimates_table_build: NULL array");
    RPVG_REQUIRE((M == 0 || in->members) && (S == 0 || in->posteriors) && (A == 0 || in->abundances) && (P == 0 || in->path_effective_length),
                 "rpvg_hip_estimates_table_build: NULL array");
    std::unique_ptr<rpvg_hip_estimates_table> t(new (std::nothrow) rpvg_hip_estimates_table());
    if (!t) {
        setError("rpvg_hip_estimates_table_build: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    t->num_clusters = K;
    t->ploidy = ploidy;
    t->num_paths = P;
    t->num_members = M;
    t->h_haplotype_prob.assign(P, 0.0);
    t->h_read_count.assign(P, 0.0);
    t->h_transcript_count.assign(P, 0.0);
    t->h_tpm.assign(P, 0.0);
    t->h_member_transcript_count.assign(M, 0.0);
    t->h_member_tpm.assign(M, 0.0);
    t->h_cluster_transcript_count.assign(K, 0.0);
    t->h_scalars.assign(4, 0.0);
    t->pack.add(t->haplotype_prob, t->h_haplotype_prob.data(), P);
    t->pack.add(t->read_count, t->h_read_count.data(), P);
    t->pack.add(t->transcript_count, t->h_transcript_count.data(), P);
    t->pack.add(t->tpm, t->h_tpm.data(), P);
    t->pack.add(t->member_transcript_count, t->h_member_transcript_count.data(), M);
    t->pack.add(t->member_tpm, t->h_member_tpm.data(), M);
    t->pack.add(t->cluster_transcript_count, t->h_cluster_transcript_count.data(), K);
    t->pack.add(t->scalars, t->h_scalars.data(), 4);

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(t->pack.alloc());
    RPVG_HIP_CHECK(zeroAsync(t->pack.block.ptr, t->pack.total, st));  // the TPMs until there is a denominator; the totals of an empty batch
    if (K == 0) {
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        *table_out = t.release();
        return RPVG_HIP_OK;
    }

    const bool on_device = in->on_device != 0;
    UploadPack inputs;
    DeviceBuffer<uint64_t> set_off, member_off, abund_off, cluster_path_off;
    DeviceBuffer<uint32_t> members, info, key, position, route_list, counters;
    DeviceBuffer<double> posteriors, abundances, noise_count, eff;
    DeviceBuffer<unsigned long long> d_bad;
    takeInput(inputs, set_off, {in->set_off, on_device}, static_cast<size_t>(K) + 1);
    takeInput(inputs, member_off, {in->member_off, on_device}, S + 1);
    takeInput(inputs, members, {in->members, on_device}, M);
    takeInput(inputs, posteriors, {in->posteriors, on_device}, S);
    takeInput(inputs, abund_off, {in->abund_off, on_device}, static_cast<size_t>(K) + 1);
    takeInput(inputs, abundances, {in->abundances, on_device}, A);
    takeInput(inputs, noise_count, {in->noise_count, on_device}, K);
    takeInput(inputs, cluster_path_off, {in->cluster_path_off, on_device}, static_cast<size_t>(K) + 1);
    takeInput(inputs, eff, {in->path_effective_length, on_device}, P);
    inputs.add(d_bad, &kNoBad, 1);
    inputs.addZero(counters, kRoutes);
    SpanScope copies(ctx, FAM_H2D);
    RPVG_HIP_CHECK(inputs.commit(st));
    copies.end();
    if (!on_device) ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    RPVG_HIP_CHECK(info.alloc(M));
    RPVG_HIP_CHECK(key.alloc(M));
    RPVG_HIP_CHECK(position.alloc(M));
    RPVG_HIP_CHECK(route_list.alloc(static_cast<size_t>(kRoutes) * K));

    TableArgs a;
    a.K = K;
    a.S = S;
    a.M = M;
    a.A = A;
    a.P = P;
    a.set_off = set_off.ptr;
    a.member_off = member_off.ptr;
    a.members = members.ptr;
    a.posteriors = posteriors.ptr;
    a.abund_off = abund_off.ptr;
    a.abundances = abundances.ptr;
    a.noise_count = noise_count.ptr;
    a.cluster_path_off = cluster_path_off.ptr;
    a.eff = eff.ptr;
    a.info = info.ptr;
    a.key = key.ptr;
    a.position = position.ptr;
    a.route_list = route_list.ptr;
    a.counters = counters.ptr;
    a.bad = d_bad.ptr;
    a.haplotype_prob = t->haplotype_prob.ptr;
    a.read_count = t->read_count.ptr;
    a.transcript_count = t->transcript_count.ptr;
    a.member_transcript_count = t->member_transcript_count.ptr;
    a.cluster_transcript_count = t->cluster_transcript_count.ptr;

    SpanScope span(ctx, FAM_BUILD);
    const uint64_t describe_threads = std::max<uint64_t>(std::max<uint64_t>(K, S + 1), M);
    describeKernel<<<gridFor(describe_threads), dim3(kBlock), 0, st>>>(a);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    word64 bad = kNoBad;
    uint32_t listed[kRoutes] = {0, 0, 0};
    if (const int rc = fetchDescribed(st, d_bad.ptr, &bad, counters.ptr, listed, kRoutes)) return rc;
    if (bad != kNoBad) {
        span.end();
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        const Offender o = offenderOf(bad, kBadAbundCount);
        setError("rpvg_hip_estimates_table_build: cluster %llu: %s", static_cast<unsigned long long>(o.index), kReasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    const uint32_t waves = listed[kRouteWave], groups = listed[kRouteLds], global = listed[kRouteGlobal];
    if (static_cast<uint64_t>(waves) + groups + global != K) {
        span.end();
        (void) hipDeviceSynchronize();
        setError("rpvg_hip_estimates_table_build: %u + %u + %u clusters listed of %u", waves, groups, global, K);
        return RPVG_HIP_ERR_RUNTIME;
    }
    t->clusters_by_route[kRouteWave] = waves;
    t->clusters_by_route[kRouteLds] = groups;
    t->clusters_by_route[kRouteGlobal] = global;
    if (waves) {
        residentKernel<kWaveBlock, kWavePaths, kWaveMembers><<<dim3(waves), dim3(kWaveBlock), 0, st>>>(a, kRouteWave, waves);
        ctx->stats.build_launches += 1;
    }
    if (groups) {
        residentKernel<kLdsBlock, kLdsPaths, kLdsMembers><<<dim3(groups), dim3(kLdsBlock), 0, st>>>(a, kRouteLds, groups);
        ctx->stats.build_launches += 1;
    }
    RPVG_HIP_CHECK(hipGetLastError());
    DeviceBuffer<uint32_t> key_sorted, position_sorted;
    if (global) {
        RPVG_HIP_CHECK(key_sorted.alloc(M));
        RPVG_HIP_CHECK(position_sorted.alloc(M));
        // (hipcub's radix sort is stable: equal keys keep the ascending member positions they come in with)
        if (const int rc = sortPairs(st, key.ptr, key_sorted.ptr, position.ptr, position_sorted.ptr, M, bitsFor(P + 1))) return rc;
        if (P) globalPathsKernel<<<gridFor(P), dim3(kBlock), 0, st>>>(a, key_sorted.ptr, position_sorted.ptr);
        globalClustersKernel<<<gridFor(global, kBlock / 64), dim3(kBlock), 0, st>>>(a, global);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 2;
    }
    totalsKernel<<<dim3(1), dim3(64), 0, st>>>(K, t->cluster_transcript_count.ptr, noise_count.ptr, static_cast<double>(ploidy), t->scalars.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    span.end();
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    *table_out = t.release();
    return RPVG_HIP_OK;
}

int rpvg_hip_estimates_table_tpm(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table, double denominator) {
    RPVG_REQUIRE(ctx && table, "rpvg_hip_estimates_table_tpm: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = table->num_paths + table->num_members;
    if (n) {
        SpanScope span(ctx, FAM_BUILD);
        tpmKernel<<<gridFor(n), dim3(kBlock), 0, st>>>(table->num_paths, table->num_members, denominator, table->transcript_count.ptr,
                                                       table->member_transcript_count.ptr, table->tpm.ptr, table->member_tpm.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
        span.end();
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
    }
    table->denominator = denominator;
    table->has_tpm = true;
    table->downloaded = false;
    return RPVG_HIP_OK;
}

int rpvg_hip_estimates_table_view(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table, rpvg_estimates_table_view * view) {
    RPVG_REQUIRE(ctx && table && view, "rpvg_hip_estimates_table_view: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);  // (rpvg_hip_estimates_table_tpm on another thread changes the table under it)
    if (!table->downloaded) {
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        RPVG_HIP_CHECK(table->pack.fetch(ctx->stream));
        RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        table->pack.scatter();
        table->downloaded = true;
    }
    std::memset(view, 0, sizeof(*view));
    view->num_clusters = table->num_clusters;
    view->num_paths = table->num_paths;
    view->num_members = table->num_members;
    view->haplotype_prob = table->h_haplotype_prob.data();
    view->read_count = table->h_read_count.data();
    view->transcript_count = table->h_transcript_count.data();
    view->tpm = table->h_tpm.data();
    view->member_transcript_count = table->h_member_transcript_count.data();
    view->member_tpm = table->h_member_tpm.data();
    view->cluster_transcript_count = table->h_cluster_transcript_count.data();
    view->total_transcript_count = table->h_scalars[0];
    view->noise_count_total = table->h_scalars[1];
    view->noise_count_share_total = table->h_scalars[2];
    view->tpm_denominator = table->denominator;
    view->has_tpm = table->has_tpm ? 1 : 0;
    view->ploidy = table->ploidy;
    for (int r = 0; r < kRoutes; ++r) view->clusters_by_route[r] = table->clusters_by_route[r];
    return RPVG_HIP_OK;
}

void rpvg_hip_estimates_table_free(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table) {
    if (!table) return;
    waitAndDelete(ctx);
    delete table;
}

}  // extern "C"
