// read_rows.hip — the step right before the inference hot path, on the GPU: the alignment paths of every read of a
// cluster -> the cluster's merged ReadPathProbabilities rows (interface include/rpvg_rows.h).
//
// Takes over   ReadPathProbabilities::addPathProbs / calcAlignPathLogProbs   src/read_path_probabilities.cpp:39-221
//              the caller's sort + quickMergeIdentical of adjacent rows      src/main.cpp:953-973
//              (operator<, quickMergeIdentical                               src/read_path_probabilities.cpp:223-322)
//
// One wavefront per read.  The reference fills a dense vector over ALL paths of the cluster per read; here only the
// paths the read touches exist:
//   A  per (alignment, path) entry: log prob = score * base (+ fragment log density) - log(effective length); of the
//      entries of one path the one with the longest alignment, then the highest log prob, survives (:128-139) —
//      found by binary search in the other alignments' ascending path lists, no scratch table;
//   B  survivors are ranked into ascending path order from the same sorted lists (prefix counts), optionally folded
//      into name groups (--path-info with -i transcripts, :151-168);
//   C  normalisation by a wave-wide log-sum-exp (the reference folds add_log sequentially: equal up to rounding);
//   D  the precision bucketing of :181-206 is inherently sequential in path order and is kept so: one step per path,
//      the lanes scan the buckets (LDS for the first 256, the read's scratch beyond);
//   E  buckets are ordered as std::sort orders pair<double, vector<uint32_t>> (:219) and written to the read's padded
//      slice; a scan + copy pass packs all reads into the CSR of rpvg_cluster_batch.
// Merging (rows_merge.hip): row ids are merge-sorted with the reference's own tolerant operator< behind the cluster id, runs of
// rows that quickMergeIdentical accepts are found with the reference's compare-with-the-run-head rule, counts are summed.
// The host side is a sequence of stages over one RowsBuild — scratch, row kernels, merge (or not), pack — whose launch shapes
// are the plan's (rows_plan.hpp); the resident alignment batch comes from alignments.hip or align_index.hip.

#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/rpvg_rows.h"
#include "common.hpp"
#include "alignments.hpp"
#include "device_algos.hpp"
#include "path_table.hpp"
#include "frag_length.hpp"
#include "read_rows.hpp"
#include "rows_plan.hpp"
#include "rows_residents.hpp"
#include "table_kit.hpp"

using namespace rpvg_hip_detail;
using namespace rpvg_rows_plan;

namespace {

constexpr double kScoreLogBase = 1.383325268738;  // Utils::score_log_base, src/utils.hpp:83
constexpr double kNoiseScoreLogBase = 1e-6;       // Utils::noise_score_log_base, src/utils.hpp:84
constexpr int kLdsBuckets = 256;

struct RowsIn {
    uint64_t num_reads;
    const uint32_t * read_cluster;
    const uint64_t * cluster_path_off;
    const double * path_eff_len;
    const uint32_t * path_source_count;
    const uint32_t * path_group;  // null = no collapsing
    const uint8_t * read_min_mapq;
    const int32_t * read_noise_score;
    const uint64_t * read_align_off;
    const int32_t * align_score_sum;
    const uint16_t * align_length;
    const uint16_t * align_frag_length;
    const uint64_t * align_path_off;
    const uint32_t * align_path_idx;
    const double * frag_table;  // null = single end
    const double * phred_prob;  // [256] 10^(-q/10)
    double prob_precision, min_noise_prob;
};

__device__ __forceinline__ double waveMaxF64(double v) {
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// first position in [lo, hi) of the ascending list whose value is >= p
__device__ __forceinline__ uint64_t lowerBound(const uint32_t * __restrict__ list, uint64_t lo, uint64_t hi, const uint32_t p) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (list[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void alignLogProbKernel(const uint64_t num_aligns, const int32_t * __restrict__ score_sum,
                                   const uint16_t * __restrict__ frag_length, const double * __restrict__ frag_table,
                                   double * __restrict__ out) {
    const uint64_t a = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (a >= num_aligns) return;
    // src/read_path_probabilities.cpp:56-61
    double lp = score_sum[a] * kScoreLogBase;
    if (frag_table) lp += frag_table[frag_length[a]];
    out[a] = lp;
}

__device__ __forceinline__ double addLogDev(const double x, const double y) {  // Utils::add_log, src/utils.hpp:300-302
    return x > y ? x + log1p(exp(y - x)) : y + log1p(exp(x - y));
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void readRowKernel(const RowsIn in, const RowsScratch sc,
                                                                    const uint64_t num_listed, const uint32_t * __restrict__ listed) {
    __shared__ double lds_mean[kWavesPerBlock][kLdsBuckets];
    __shared__ uint32_t lds_count[kWavesPerBlock][kLdsBuckets];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint64_t slot = blockIdx.x * static_cast<uint64_t>(kWavesPerBlock) + wave;
    if (slot >= num_listed) return;
    const uint64_t r = listed ? listed[slot] : slot;
    volatile double * wmean = lds_mean[wave];
    volatile uint32_t * wcount = lds_count[wave];

    const uint64_t a0 = in.read_align_off[r], a1 = in.read_align_off[r + 1];
    const uint64_t e0 = in.align_path_off[a0], e1 = in.align_path_off[a1];
    const uint32_t E = static_cast<uint32_t>(e1 - e0);
    const uint8_t mapq = in.read_min_mapq[r];
    const int32_t noise_score = in.read_noise_score[r];

    // src/read_path_probabilities.cpp:89-108
    double noise = 1.0;
    bool has_paths = false;
    if (mapq > 0) {
        noise = fmax(in.prob_precision, fmax(in.min_noise_prob, in.phred_prob[mapq]));
        noise += (1 - noise) * exp(noise_score * kNoiseScoreLogBase);
        has_paths = (noise_score != 0);
    }
    if (!has_paths) {
        if (lane == 0) {
            sc.row_noise[r] = noise;
            sc.row_ngroups[r] = 0;
            sc.row_nmembers[r] = 0;
        }
        return;
    }

    const uint32_t k = in.read_cluster[r];
    const uint64_t cp0 = in.cluster_path_off[k];
    const uint32_t * __restrict__ plist = in.align_path_idx;
    uint32_t * S = sc.surv_prefix + r;  // slot of entry e: S[e]

    // ---- A: survivors (:110-149) and their exclusive prefix count -------------------------------------------
    uint32_t num_surv = 0;
    for (uint32_t base = 0; base < E; base += 64) {
        const uint32_t i = base + lane;
        bool keep = false;
        if (i < E) {
            const uint64_t e = e0 + i;
            uint64_t lo = a0, hi = a1 - 1;  // last alignment whose first entry is <= e
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) >> 1;
                if (in.align_path_off[mid] <= e) lo = mid; else hi = mid - 1;
            }
            const uint64_t a = lo;
            const uint32_t p = plist[e];
            keep = in.path_eff_len[cp0 + p] != 0;  // Utils::doubleCompare(x, 0) holds for x == 0 only
            if (keep) {
                const uint16_t al = in.align_length[a];
                const double alp = sc.align_log_prob[a];
                for (uint64_t b = a0; b < a1 && keep; ++b) {
                    if (b == a) continue;
                    const uint64_t b0 = in.align_path_off[b], b1 = in.align_path_off[b + 1];
                    const uint64_t pos = lowerBound(plist, b0, b1, p);
                    if (pos < b1 && plist[pos] == p) {
                        const uint16_t bl = in.align_length[b];
                        const double blp = sc.align_log_prob[b];
                        if (bl > al || (bl == al && (blp > alp || (blp == alp && b < a)))) keep = false;
                    }
                }
            }
        }
        const uint64_t mask = __ballot(keep);
        if (i < E) S[e0 + i] = num_surv + __popcll(mask & ((1ull << lane) - 1ull));
        num_surv += __popcll(mask);
    }
    if (lane == 0) S[e1] = num_surv;
    __threadfence_block();

    // ---- B: survivors in ascending path order ---------------------------------------------------------------
    const bool collapse = in.path_group != nullptr;
    uint32_t * sorted_idx = collapse ? sc.tmp_idx + e0 : sc.unit_idx + e0;
    double * sorted_val = collapse ? sc.tmp_val + e0 : sc.unit_val + e0;
    for (uint32_t base = 0; base < E; base += 64) {
        const uint32_t i = base + lane;
        if (i >= E) continue;
        const uint64_t e = e0 + i;
        if (S[e + 1] == S[e]) continue;  // not a survivor
        const uint32_t p = plist[e];
        uint32_t rank = 0;
        uint64_t own = a0;
        for (uint64_t b = a0; b < a1; ++b) {
            const uint64_t b0 = in.align_path_off[b], b1 = in.align_path_off[b + 1];
            if (e >= b0 && e < b1) own = b;
            const uint64_t pos = (e >= b0 && e < b1) ? e : lowerBound(plist, b0, b1, p);
            rank += S[pos] - S[b0];
        }
        sorted_idx[rank] = p;
        sorted_val[rank] = sc.align_log_prob[own] - log(in.path_eff_len[cp0 + p]);  // :126
    }
    __threadfence_block();

    uint32_t T = num_surv;
    if (collapse && T > 0) {
        // :151-168 — a name group's log prob = add_log, in path order, of member log prob + log(source count);
        // units leave in ascending group index.  Quadratic in the paths the read touches (this mode is
        // `-i transcripts` with --path-info only).
        uint32_t * is_head = sc.bucket_of + e0;  // free until phase D
        for (uint32_t t = lane; t < T; t += 64) {
            const uint32_t g = in.path_group[cp0 + sorted_idx[t]];
            bool head = true;
            for (uint32_t u = 0; u < t && head; ++u) head = in.path_group[cp0 + sorted_idx[u]] != g;
            is_head[t] = head;
        }
        __threadfence_block();
        uint32_t num_units = 0;
        for (uint32_t base = 0; base < T; base += 64) {
            const uint32_t t = base + lane;
            const bool head = (t < T) && is_head[t];
            if (head) {
                const uint32_t g = in.path_group[cp0 + sorted_idx[t]];
                uint32_t rank = 0;
                double glp = -DBL_MAX;
                for (uint32_t u = 0; u < T; ++u) {
                    const uint32_t pu = sorted_idx[u];
                    const uint32_t gu = in.path_group[cp0 + pu];
                    if (gu == g) glp = addLogDev(glp, sorted_val[u] + log(static_cast<double>(in.path_source_count[cp0 + pu])));
                    rank += (gu < g) && is_head[u];
                }
                sc.unit_idx[e0 + rank] = g;
                sc.unit_val[e0 + rank] = glp;
            }
            num_units += __popcll(__ballot(head));
        }
        T = num_units;
        __threadfence_block();
    }

    uint32_t * uidx = sc.unit_idx + e0;
    double * uval = sc.unit_val + e0;

    if (T == 0) {  // every touched path has zero effective length: the reference would assert (:174)
        if (lane == 0) {
            sc.row_noise[r] = noise;
            sc.row_ngroups[r] = 0;
            sc.row_nmembers[r] = 0;
        }
        return;
    }

    // ---- C: normalise (:170-179) -------------------------------------------------------------------------------
    double vmax = -DBL_MAX;
    for (uint32_t t = lane; t < T; t += 64) vmax = fmax(vmax, uval[t]);
    vmax = waveMaxF64(vmax);
    double vsum = 0.0;
    for (uint32_t t = lane; t < T; t += 64) vsum += exp(uval[t] - vmax);
    vsum = waveSumF64(vsum);
    const double log_sum = vmax + log(vsum);
    for (uint32_t t = lane; t < T; t += 64) uval[t] = exp(uval[t] - log_sum);
    __threadfence_block();

    // ---- D: precision buckets, sequential in unit order (:181-211) ---------------------------------------------
    uint32_t nb = 0;
    double low_sum = 0.0;
    for (uint32_t t = 0; t < T; ++t) {
        const double p = uval[t];
        if (p >= in.prob_precision) {
            uint32_t found = kNone;
            for (uint32_t base = 0; base < nb && found == kNone; base += 64) {
                const uint32_t b = base + lane;
                bool hit = false;
                if (b < nb) {
                    const double m = (b < kLdsBuckets) ? wmean[b] : __hip_atomic_load(sc.bucket_mean + e0 + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hit = fabs(m - p) < in.prob_precision;
                }
                const uint64_t mask = __ballot(hit);
                if (mask) found = base + __ffsll(static_cast<unsigned long long>(mask)) - 1;
            }
            if (lane == 0) {
                if (found == kNone) {
                    if (nb < kLdsBuckets) {
                        wmean[nb] = p;
                        wcount[nb] = 1;
                    } else {
                        __hip_atomic_store(sc.bucket_mean + e0 + nb, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        sc.bucket_count[e0 + nb] = 1;
                    }
                    sc.bucket_first[e0 + nb] = t;
                    sc.bucket_of[e0 + t] = nb;
                } else {
                    // running mean (:189)
                    if (found < kLdsBuckets) {
                        const uint32_t c = wcount[found];
                        wmean[found] = (wmean[found] * c + p) / (c + 1);
                        wcount[found] = c + 1;
                    } else {
                        const uint32_t c = sc.bucket_count[e0 + found];
                        const double m = __hip_atomic_load(sc.bucket_mean + e0 + found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(sc.bucket_mean + e0 + found, (m * c + p) / (c + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        sc.bucket_count[e0 + found] = c + 1;
                    }
                    sc.bucket_of[e0 + t] = found;
                }
            }
            if (found == kNone) ++nb;
        } else {
            low_sum += p;
            if (lane == 0) sc.bucket_of[e0 + t] = kNone;
        }
    }
    __threadfence_block();

    // ---- E: scale, order the buckets, write the read's slice (:213-219) ----------------------------------------
    const double scale = 1 - noise;
    auto bucketMean = [&](const uint32_t b) -> double {
        return ((b < kLdsBuckets) ? wmean[b] : __hip_atomic_load(sc.bucket_mean + e0 + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) * scale;
    };
    auto bucketCount = [&](const uint32_t b) -> uint32_t { return (b < kLdsBuckets) ? wcount[b] : sc.bucket_count[e0 + b]; };
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t b = base + lane;
        if (b >= nb) continue;
        const double m = bucketMean(b);
        const uint32_t first = uidx[sc.bucket_first[e0 + b]];
        uint32_t rank = 0;
        for (uint32_t o = 0; o < nb; ++o) {
            if (o == b) continue;
            const double mo = bucketMean(o);
            // pair<double, vector> ordering; member lists are disjoint, so their first elements decide ties
            if (mo < m || (mo == m && uidx[sc.bucket_first[e0 + o]] < first)) ++rank;
        }
        sc.bucket_rank[e0 + b] = rank;
        sc.grp_prob[e0 + rank] = m;
        sc.grp_size[e0 + rank] = bucketCount(b);
        sc.bucket_cursor[e0 + b] = 0;
    }
    __threadfence_block();
    // exclusive member offsets of the sorted groups
    uint32_t running = 0;
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t j = base + lane;
        const uint32_t size = (j < nb) ? sc.grp_size[e0 + j] : 0;
        uint32_t incl = size;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (j < nb) sc.grp_moff[e0 + j] = running + incl - size;
        running += __shfl(incl, 63, 64);
    }
    __threadfence_block();
    // members in ascending unit order inside each group
    if (nb <= 8) {
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t moff = sc.grp_moff[e0 + sc.bucket_rank[e0 + b]];
            uint32_t placed = 0;
            for (uint32_t base = 0; base < T; base += 64) {
                const uint32_t t = base + lane;
                const bool mine = (t < T) && sc.bucket_of[e0 + t] == b;
                const uint64_t mask = __ballot(mine);
                if (mine) sc.member[e0 + moff + placed + __popcll(mask & ((1ull << lane) - 1ull))] = uidx[t];
                placed += __popcll(mask);
            }
        }
    } else if (lane == 0) {
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t b = sc.bucket_of[e0 + t];
            if (b == kNone) continue;
            const uint32_t pos = sc.grp_moff[e0 + sc.bucket_rank[e0 + b]] + sc.bucket_cursor[e0 + b]++;
            sc.member[e0 + pos] = uidx[t];
        }
    }
    if (lane == 0) {
        sc.row_noise[r] = noise + low_sum * scale;  // :216
        sc.row_ngroups[r] = nb;
        sc.row_nmembers[r] = running;
    }
}


// ---- small reads: sixteen lanes per read -----------------------------------------------------------------------
// Most reads touch a handful of paths (3.3 (alignment, path) entries on average in the configs[2] workload); a whole
// wavefront per read then spends its time waiting on the scratch arrays between phases.  A read with at most 16 entries
// is handled by a 16-lane group — four reads per wavefront — entirely in registers: lane = entry, then lane = unit,
// then lane = bucket; the phases talk through width-16 shuffles and ballots.  Same arithmetic, same order of the
// sequential bucketing, same output slices as readRowKernel (which keeps the larger reads and the collapsing mode).

__device__ __forceinline__ uint32_t groupBallot(const bool pred, const int group_shift) {
    return static_cast<uint32_t>((__ballot(pred) >> group_shift) & 0xffffull);
}

__global__ __launch_bounds__(256) void readRowSmallKernel(const RowsIn in, const RowsScratch sc, const uint64_t num_listed,
                                                          const uint32_t * __restrict__ listed) {
    const int g = threadIdx.x & (kGroupLanes - 1);                  // lane inside the group
    const int group_shift = (threadIdx.x & 63) & ~(kGroupLanes - 1);  // first lane of the group inside the wave
    const uint64_t slot = (blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x) / kGroupLanes;
    const bool active = slot < num_listed;
    const uint64_t r = active ? listed[slot] : 0;

    const uint64_t a0 = in.read_align_off[r], a1 = in.read_align_off[r + 1];
    const uint64_t e0 = in.align_path_off[a0], e1 = in.align_path_off[a1];
    const uint32_t E = active ? static_cast<uint32_t>(e1 - e0) : 0;  // <= kGroupLanes
    const uint8_t mapq = in.read_min_mapq[r];
    const int32_t noise_score = in.read_noise_score[r];

    // src/read_path_probabilities.cpp:89-108
    double noise = 1.0;
    bool has_paths = false;
    if (active && mapq > 0) {
        noise = fmax(in.prob_precision, fmax(in.min_noise_prob, in.phred_prob[mapq]));
        noise += (1 - noise) * exp(noise_score * kNoiseScoreLogBase);
        has_paths = (noise_score != 0);
    }
    // every lane of the wave takes part in the shuffles below: groups without work carry E = 0
    const uint32_t n_ent = has_paths ? E : 0;
    // The loops over entries / units / buckets stop at the largest entry count of the wave's four reads (3.3 entries
    // per read on average, 16 at most): wave-uniform trip counts, a fifth of the shuffles.
    uint32_t n_max = n_ent;
    n_max = max(n_max, static_cast<uint32_t>(__shfl_xor(static_cast<int>(n_max), 16, 64)));
    n_max = max(n_max, static_cast<uint32_t>(__shfl_xor(static_cast<int>(n_max), 32, 64)));
    const int n_loop = static_cast<int>(__builtin_amdgcn_readfirstlane(static_cast<int>(n_max)));

    // ---- A: one entry per lane; the survivor of every path (:110-149) -------------------------------------------
    const bool is_entry = static_cast<uint32_t>(g) < n_ent;
    uint32_t p = kNone;
    uint32_t al = 0;
    double alp = 0.0, lp = 0.0;
    uint32_t a_idx = 0;
    bool keep = false;
    if (is_entry) {
        const uint64_t e = e0 + g;
        uint64_t a = a0;
        while (a + 1 < a1 && in.align_path_off[a + 1] <= e) ++a;
        a_idx = static_cast<uint32_t>(a - a0);
        p = in.align_path_idx[e];
        al = in.align_length[a];
        alp = sc.align_log_prob[a];
        const double len = in.path_eff_len[in.cluster_path_off[in.read_cluster[r]] + p];
        keep = len != 0;
        if (keep) lp = alp - log(len);  // :126
    }
    for (int j = 0; j < n_loop; ++j) {
        const uint32_t pj = __shfl(p, j, kGroupLanes);
        const uint32_t alj = __shfl(al, j, kGroupLanes);
        const double alpj = __shfl(alp, j, kGroupLanes);
        const uint32_t aj = __shfl(a_idx, j, kGroupLanes);
        if (is_entry && j != g && static_cast<uint32_t>(j) < n_ent && pj == p) {
            if (alj > al || (alj == al && (alpj > alp || (alpj == alp && aj < a_idx)))) keep = false;
        }
    }
    // ---- B: ascending path order ---------------------------------------------------------------------------------
    uint32_t rank = 0;
    for (int j = 0; j < n_loop; ++j) {
        const uint32_t pj = __shfl(p, j, kGroupLanes);
        const bool kj = __shfl(static_cast<int>(keep), j, kGroupLanes) != 0;
        rank += (kj && pj < p);
    }
    const uint32_t T = __popc(groupBallot(keep, group_shift));
    // unit t lives on lane t: pull (path, log prob) from the survivor whose rank is t
    uint32_t uidx = kNone;
    double uval = -DBL_MAX;
    for (int j = 0; j < n_loop; ++j) {
        const bool kj = __shfl(static_cast<int>(keep), j, kGroupLanes) != 0;
        const uint32_t rj = __shfl(rank, j, kGroupLanes);
        const uint32_t pj = __shfl(p, j, kGroupLanes);
        const double lpj = __shfl(lp, j, kGroupLanes);
        if (kj && rj == static_cast<uint32_t>(g)) {
            uidx = pj;
            uval = lpj;
        }
    }
    const bool is_unit = static_cast<uint32_t>(g) < T;

    // ---- C: normalise (:170-179) ---------------------------------------------------------------------------------
    double vmax = uval;
    for (int d = kGroupLanes / 2; d >= 1; d >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, d, kGroupLanes));
    double vsum = is_unit ? exp(uval - vmax) : 0.0;
    for (int d = kGroupLanes / 2; d >= 1; d >>= 1) vsum += __shfl_xor(vsum, d, kGroupLanes);
    const double prob = is_unit ? exp(uval - (vmax + log(vsum))) : 0.0;

    // ---- D: precision buckets, sequential in unit order (:181-211); bucket b lives on lane b ----------------------
    uint32_t nb = 0, my_bucket = kNone, b_count = 0, b_first = 0;
    double b_mean = 0.0, low_sum = 0.0;
    for (int t = 0; t < n_loop; ++t) {
        const double pt = __shfl(prob, t, kGroupLanes);
        const bool exists = static_cast<uint32_t>(t) < T;  // uniform inside a group
        const bool big = exists && pt >= in.prob_precision;
        const bool hit = big && static_cast<uint32_t>(g) < nb && fabs(b_mean - pt) < in.prob_precision;
        const uint32_t mask = groupBallot(hit, group_shift);
        const uint32_t found = mask ? static_cast<uint32_t>(__ffs(mask) - 1) : nb;
        if (big) {
            if (static_cast<uint32_t>(g) == found) {
                if (mask) {
                    b_mean = (b_mean * b_count + pt) / (b_count + 1);  // running mean (:189)
                    b_count += 1;
                } else {
                    b_mean = pt;
                    b_count = 1;
                    b_first = t;
                }
            }
            if (g == t) my_bucket = found;
            if (!mask) ++nb;
        } else if (exists) {
            low_sum += pt;
        }
    }

    // ---- E: scale, order the buckets, write the read's slice (:213-219) -----------------------------------------
    const double scale = 1 - noise;
    const bool is_bucket = static_cast<uint32_t>(g) < nb;
    const double m = b_mean * scale;
    const uint32_t first_member = __shfl(uidx, static_cast<int>(b_first), kGroupLanes);
    uint32_t brank = 0, moff = 0;
    for (int o = 0; o < n_loop; ++o) {
        const double mo = __shfl(m, o, kGroupLanes);
        const uint32_t fo = __shfl(first_member, o, kGroupLanes);
        if (static_cast<uint32_t>(o) < nb && o != g && (mo < m || (mo == m && fo < first_member))) ++brank;
    }
    for (int o = 0; o < n_loop; ++o) {
        const uint32_t ro = __shfl(brank, o, kGroupLanes);
        const uint32_t co = __shfl(b_count, o, kGroupLanes);
        if (static_cast<uint32_t>(o) < nb && ro < brank) moff += co;
    }
    if (is_bucket) {
        sc.grp_prob[e0 + brank] = m;
        sc.grp_size[e0 + brank] = b_count;
        sc.grp_moff[e0 + brank] = moff;
    }
    // members: unit t goes behind the earlier units of its bucket
    const uint32_t bucket_moff = __shfl(moff, static_cast<int>(my_bucket == kNone ? 0 : my_bucket), kGroupLanes);
    uint32_t before = 0;
    for (int t = 0; t < n_loop; ++t) {
        const uint32_t bt = __shfl(my_bucket, t, kGroupLanes);
        if (t < g && bt == my_bucket) ++before;
    }
    if (is_unit && my_bucket != kNone) sc.member[e0 + bucket_moff + before] = uidx;
    const uint32_t n_members = __popc(groupBallot(is_unit && my_bucket != kNone, group_shift));
    if (active && g == 0) {
        sc.row_noise[r] = has_paths && T > 0 ? noise + low_sum * scale : noise;  // :216
        sc.row_ngroups[r] = nb;
        sc.row_nmembers[r] = n_members;
    }
}

// packs the padded per-read slices into the CSR of rpvg_cluster_batch; sixteen lanes per row.  `source` (optional)
// lists the reads to copy (the merged rows); row j of the output comes from read source[j].
__global__ __launch_bounds__(256) void packRowsKernel(const uint64_t num_rows, const uint32_t * __restrict__ source,
                                                      const uint64_t * __restrict__ read_align_off,
                                                      const uint64_t * __restrict__ align_path_off, const RowsScratch sc,
                                                      const uint64_t * __restrict__ row_grp_off,
                                                      const uint64_t * __restrict__ row_member_off, double * __restrict__ row_noise,
                                                      double * __restrict__ grp_prob, uint64_t * __restrict__ grp_idx_off,
                                                      uint32_t * __restrict__ path_idx) {
    const int lane = threadIdx.x & (kGroupLanes - 1);  // sixteen lanes per row: most rows have a few groups
    const uint64_t j = (blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x) / kGroupLanes;
    if (j >= num_rows) return;
    const uint64_t r = source ? source[j] : j;
    const uint64_t e0 = align_path_off[read_align_off[r]];
    const uint64_t g0 = row_grp_off[j], m0 = row_member_off[j];
    const uint32_t nb = sc.row_ngroups[r], nm = sc.row_nmembers[r];
    for (uint32_t b = lane; b < nb; b += kGroupLanes) {
        grp_prob[g0 + b] = sc.grp_prob[e0 + b];
        grp_idx_off[g0 + b] = m0 + sc.grp_moff[e0 + b];
    }
    for (uint32_t m = lane; m < nm; m += kGroupLanes) path_idx[m0 + m] = sc.member[e0 + m];
    if (lane == 0) {
        row_noise[j] = sc.row_noise[r];
        if (j + 1 == num_rows) grp_idx_off[g0 + nb] = m0 + nm;
    }
}

__global__ void gatherSizesKernel(const uint64_t n, const uint32_t * __restrict__ source, const uint32_t * __restrict__ ngroups,
                                  const uint32_t * __restrict__ nmembers, uint64_t * __restrict__ out_ngroups,
                                  uint64_t * __restrict__ out_nmembers) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = source ? source[i] : static_cast<uint32_t>(i);
    out_ngroups[i] = ngroups[r];
    out_nmembers[i] = nmembers[r];
}

// The per-read slices of one build (RowsScratch points into them).
struct RowsScratchBuffers {
    DeviceBuffer<double> alp, unit_val, tmp_val, bucket_mean, row_noise, grp_prob;
    DeviceBuffer<uint32_t> prefix, unit_idx, tmp_idx, bucket_of, bucket_count, bucket_first, bucket_rank, bucket_cursor, ngroups,
        nmembers, grp_size, grp_moff, member;

    int alloc(const uint64_t N, const uint64_t A, const uint64_t E, const bool collapse) {
        RPVG_HIP_CHECK(alp.alloc(A));
        RPVG_HIP_CHECK(prefix.alloc(E + N + 1));
        RPVG_HIP_CHECK(unit_idx.alloc(E));
        RPVG_HIP_CHECK(unit_val.alloc(E));
        if (collapse) {
            RPVG_HIP_CHECK(tmp_idx.alloc(E));
            RPVG_HIP_CHECK(tmp_val.alloc(E));
        }
        RPVG_HIP_CHECK(bucket_of.alloc(E));
        RPVG_HIP_CHECK(bucket_mean.alloc(E));
        RPVG_HIP_CHECK(bucket_count.alloc(E));
        RPVG_HIP_CHECK(bucket_first.alloc(E));
        RPVG_HIP_CHECK(bucket_rank.alloc(E));
        RPVG_HIP_CHECK(bucket_cursor.alloc(E));
        RPVG_HIP_CHECK(row_noise.alloc(N));
        RPVG_HIP_CHECK(ngroups.alloc(N + 1));
        RPVG_HIP_CHECK(nmembers.alloc(N + 1));
        RPVG_HIP_CHECK(grp_prob.alloc(E));
        RPVG_HIP_CHECK(grp_size.alloc(E));
        RPVG_HIP_CHECK(grp_moff.alloc(E));
        RPVG_HIP_CHECK(member.alloc(E));
        return RPVG_HIP_OK;
    }

    RowsScratch view() const {
        RowsScratch sc;
        sc.align_log_prob = alp.ptr;
        sc.surv_prefix = prefix.ptr;
        sc.unit_idx = unit_idx.ptr;
        sc.unit_val = unit_val.ptr;
        sc.tmp_idx = tmp_idx.ptr;
        sc.tmp_val = tmp_val.ptr;
        sc.bucket_of = bucket_of.ptr;
        sc.bucket_mean = bucket_mean.ptr;
        sc.bucket_count = bucket_count.ptr;
        sc.bucket_first = bucket_first.ptr;
        sc.bucket_rank = bucket_rank.ptr;
        sc.bucket_cursor = bucket_cursor.ptr;
        sc.row_noise = row_noise.ptr;
        sc.row_ngroups = ngroups.ptr;
        sc.row_nmembers = nmembers.ptr;
        sc.grp_prob = grp_prob.ptr;
        sc.grp_size = grp_size.ptr;
        sc.grp_moff = grp_moff.ptr;
        sc.member = member.ptr;
        return sc;
    }
};

// the three timing events of a build, destroyed on every way out
struct BuildEvents {
    hipEvent_t start = nullptr, rows_done = nullptr, packed = nullptr;
    BuildEvents() {}
    BuildEvents(const BuildEvents &) = delete;
    BuildEvents & operator=(const BuildEvents &) = delete;
    hipError_t create() {
        for (hipEvent_t * event : {&start, &rows_done, &packed}) {
            const hipError_t err = hipEventCreate(event);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    ~BuildEvents() {
        for (hipEvent_t event : {start, rows_done, packed}) {
            if (event) (void) hipEventDestroy(event);
        }
    }
};

// One build: what its stages share.
struct RowsBuild {
    rpvg_hip_ctx * ctx = nullptr;
    hipStream_t st = nullptr;
    const rpvg_hip_alignments * al = nullptr;
    const rpvg_row_params * prm = nullptr;
    rpvg_hip_read_rows * out = nullptr;
    DeviceBuffer<double> d_frag, d_phred;
    RowsScratchBuffers buffers;
    RowsIn rin;
    RowsScratch sc;
    // rows to pack: all reads, or the heads of the merged runs (source[j] = the read whose slice holds row j)
    uint64_t num_out = 0;
    DeviceBuffer<uint32_t> d_source;
    const uint32_t * pack_source = nullptr;
};

// a batch without reads: the offsets of no rows
int emptyRows(hipStream_t st, const uint32_t K, rpvg_hip_read_rows * out) {
    out->h_cluster_row_off.assign(K + 1, 0);
    RPVG_HIP_CHECK(out->cluster_row_off.upload(out->h_cluster_row_off.data(), K + 1, st));
    const uint64_t zero = 0;
    RPVG_HIP_CHECK(out->row_grp_off.upload(&zero, 1, st));
    RPVG_HIP_CHECK(out->grp_idx_off.upload(&zero, 1, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

// the two tables, the per-read slices and what the row kernels read
int scratchStage(RowsBuild & b) {
    const rpvg_hip_alignments * al = b.al;
    const rpvg_row_params * prm = b.prm;
    std::vector<double> phred(256);
    for (int q = 0; q < 256; ++q) phred[q] = std::pow(10, -static_cast<double>(q) / 10);  // Utils::phred_to_prob, src/utils.hpp:131-133
    if (!prm->is_single_end) {
        if (prm->frag_length_log_prob) {
            RPVG_HIP_CHECK(b.d_frag.upload(prm->frag_length_log_prob, RPVG_FRAG_LENGTH_TABLE_SIZE, b.st));
        } else {
            b.d_frag.borrow(prm->frag_length_table->log_prob.ptr, RPVG_FRAG_LENGTH_TABLE_SIZE);  // computed on the device (frag_length.hip)
        }
    }
    RPVG_HIP_CHECK(b.d_phred.upload(phred.data(), 256, b.st));
    if (const int rc = b.buffers.alloc(al->num_reads, al->num_aligns, al->num_entries, al->collapse)) return rc;

    RowsIn & rin = b.rin;
    rin.num_reads = al->num_reads;
    rin.read_cluster = al->read_cluster.ptr;
    rin.cluster_path_off = al->cluster_path_off.ptr;
    rin.path_eff_len = al->eff_len.ptr;
    rin.path_source_count = al->source_count.ptr;
    rin.path_group = al->collapse ? al->path_group.ptr : nullptr;
    rin.read_min_mapq = al->mapq.ptr;
    rin.read_noise_score = al->noise_score.ptr;
    rin.read_align_off = al->read_align_off.ptr;
    rin.align_score_sum = al->score.ptr;
    rin.align_length = al->align_length.ptr;
    rin.align_frag_length = al->frag_length.ptr;
    rin.align_path_off = al->align_path_off.ptr;
    rin.align_path_idx = al->path_idx.ptr;
    rin.frag_table = prm->is_single_end ? nullptr : b.d_frag.ptr;
    rin.phred_prob = b.d_phred.ptr;
    rin.prob_precision = prm->prob_precision;
    rin.min_noise_prob = prm->min_noise_prob;
    b.sc = b.buffers.view();
    return RPVG_HIP_OK;
}

// the padded slice of every read
int rowKernelsStage(RowsBuild & b) {
    const rpvg_hip_alignments * al = b.al;
    hipStream_t st = b.st;
    static const bool no_small_kernel = RPVG_EXPERIMENT_ENV("RPVG_HIP_NO_SMALL_READ_KERNEL") != nullptr;
    const RowKernelsPlan plan = planRowKernels(al->num_reads, al->num_aligns, al->num_small, al->num_large, !no_small_kernel);
    SpanScope span(b.ctx, FAM_BUILD);
    alignLogProbKernel<<<dim3(plan.align_log_prob.grid), dim3(plan.align_log_prob.block), 0, st>>>(al->num_aligns, al->score.ptr, al->frag_length.ptr,
                                                                                                  b.rin.frag_table, b.sc.align_log_prob);
    if (plan.small_reads.grid) {
        readRowSmallKernel<<<dim3(plan.small_reads.grid), dim3(plan.small_reads.block), 0, st>>>(b.rin, b.sc, al->num_small, al->small_reads.ptr);
    }
    if (plan.large_reads.grid) {
        readRowKernel<<<dim3(plan.large_reads.grid), dim3(plan.large_reads.block), 0, st>>>(b.rin, b.sc, plan.every_read ? al->num_reads : al->num_large,
                                                                                           plan.every_read ? nullptr : al->large_reads.ptr);
    }
    span.end();
    b.ctx->stats.build_launches += 3;
    RPVG_HIP_CHECK(hipGetLastError());
    return RPVG_HIP_OK;
}

// without a merge every read is a row
int unmergedStage(RowsBuild & b) {
    const rpvg_hip_alignments * al = b.al;
    rpvg_hip_read_rows * out = b.out;
    RPVG_HIP_CHECK(out->row_count.alloc(al->num_reads));
    RPVG_HIP_CHECK(hipMemcpyAsync(out->row_count.ptr, al->read_count.ptr, sizeof(uint32_t) * al->num_reads, hipMemcpyDeviceToDevice, b.st));
    out->h_cluster_row_off = al->h_cluster_read_off;
    RPVG_HIP_CHECK(out->cluster_row_off.upload(out->h_cluster_row_off.data(), al->num_clusters + 1, b.st));
    return RPVG_HIP_OK;
}

// Packs the padded slices of the listed rows (pack_source == nullptr: all reads in order) into the grouped CSR of `out`.
int packStage(RowsBuild & b) {
    const rpvg_hip_alignments * al = b.al;
    rpvg_hip_read_rows * out = b.out;
    hipStream_t st = b.st;
    const uint64_t num_rows = b.num_out;
    const PackPlan plan = planPack(num_rows);
    DeviceBuffer<uint64_t> d_ng64, d_nm64, d_row_member_off;
    RPVG_HIP_CHECK(d_ng64.alloc(num_rows + 1));
    RPVG_HIP_CHECK(d_nm64.alloc(num_rows + 1));
    RPVG_HIP_CHECK(out->row_grp_off.alloc(num_rows + 1));
    RPVG_HIP_CHECK(d_row_member_off.alloc(num_rows + 1));
    RPVG_HIP_CHECK(hipMemsetAsync(d_ng64.ptr, 0, sizeof(uint64_t) * (num_rows + 1), st));
    RPVG_HIP_CHECK(hipMemsetAsync(d_nm64.ptr, 0, sizeof(uint64_t) * (num_rows + 1), st));
    gatherSizesKernel<<<dim3(plan.gather_sizes.grid), dim3(plan.gather_sizes.block), 0, st>>>(num_rows, b.pack_source, b.sc.row_ngroups, b.sc.row_nmembers,
                                                                                             d_ng64.ptr, d_nm64.ptr);
    if (const int rc = exclusiveSum(st, d_ng64.ptr, out->row_grp_off.ptr, num_rows + 1)) return rc;
    if (const int rc = exclusiveSum(st, d_nm64.ptr, d_row_member_off.ptr, num_rows + 1)) return rc;
    uint64_t totals[2] = {0, 0};
    RPVG_HIP_CHECK(hipMemcpyAsync(&totals[0], out->row_grp_off.ptr + num_rows, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&totals[1], d_row_member_off.ptr + num_rows, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t G = totals[0], M = totals[1];

    RPVG_HIP_CHECK(out->row_noise.alloc(num_rows));
    RPVG_HIP_CHECK(out->grp_prob.alloc(G + 1));
    RPVG_HIP_CHECK(out->grp_idx_off.alloc(G + 1));
    RPVG_HIP_CHECK(out->path_idx.alloc(M + 1));
    RPVG_HIP_CHECK(hipMemsetAsync(out->grp_idx_off.ptr + G, 0, sizeof(uint64_t), st));  // G == 0: the terminator is written here only
    packRowsKernel<<<dim3(plan.pack.grid), dim3(plan.pack.block), 0, st>>>(num_rows, b.pack_source, al->read_align_off.ptr, al->align_path_off.ptr, b.sc,
                                                                          out->row_grp_off.ptr, d_row_member_off.ptr, out->row_noise.ptr,
                                                                          out->grp_prob.ptr, out->grp_idx_off.ptr, out->path_idx.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the offset buffers above go out of scope
    out->num_rows = num_rows;
    out->num_groups = G;
    out->num_members = M;
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" int rpvg_hip_read_rows_build(rpvg_hip_ctx * ctx, const rpvg_hip_alignments * al, const rpvg_row_params * prm,
                                        int32_t merge, rpvg_hip_read_rows ** rows_out) {
    RPVG_REQUIRE(ctx && al && prm && rows_out, "rpvg_hip_read_rows_build: NULL argument");
    *rows_out = nullptr;
    RPVG_REQUIRE(prm->is_single_end || prm->frag_length_log_prob || prm->frag_length_table,
                 "rpvg_hip_read_rows_build: paired-end rows need frag_length_log_prob");
    RPVG_REQUIRE(prm->prob_precision > 0 && prm->min_noise_prob >= 0 && prm->min_noise_prob <= 1,
                 "rpvg_hip_read_rows_build: prob_precision / min_noise_prob out of range");

    std::unique_ptr<rpvg_hip_read_rows> out(new (std::nothrow) rpvg_hip_read_rows());
    if (!out) {
        setError("rpvg_hip_read_rows_build: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    out->num_clusters = al->num_clusters;
    out->h_cluster_path_off = al->h_out_path_off;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (al->num_reads == 0) {
        if (const int rc = emptyRows(st, al->num_clusters, out.get())) return rc;
        *rows_out = out.release();
        return RPVG_HIP_OK;
    }

    RowsBuild b{ctx, st, al, prm, out.get()};
    if (const int rc = scratchStage(b)) return rc;
    BuildEvents events;
    RPVG_HIP_CHECK(events.create());
    RPVG_HIP_CHECK(hipEventRecord(events.start, st));
    if (const int rc = rowKernelsStage(b)) return rc;
    RPVG_HIP_CHECK(hipEventRecord(events.rows_done, st));
    if (merge) {
        if (const int rc = mergeRows(ctx, al, b.sc, prm->prob_precision, b.out, &b.d_source, &b.num_out)) return rc;
        b.pack_source = b.d_source.ptr;
    } else {
        b.num_out = al->num_reads;
        if (const int rc = unmergedStage(b)) return rc;
    }
    if (const int rc = packStage(b)) return rc;
    RPVG_HIP_CHECK(hipEventRecord(events.packed, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the scratch slices go out of scope
    float ms01 = 0, ms12 = 0;
    (void) hipEventElapsedTime(&ms01, events.start, events.rows_done);
    (void) hipEventElapsedTime(&ms12, events.rows_done, events.packed);
    out->build_ms = ms01;
    out->merge_ms = ms12;
    *rows_out = out.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_read_rows_view(rpvg_hip_ctx * ctx, rpvg_hip_read_rows * rows, rpvg_cluster_batch * view, double * build_ms,
                                       double * merge_ms) {
    RPVG_REQUIRE(ctx && rows && view, "rpvg_hip_read_rows_view: NULL argument");
    if (!rows->downloaded) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint64_t R = rows->num_rows, G = rows->num_groups, M = rows->num_members;
        rows->h_row_count.resize(R);
        rows->h_row_noise.resize(R);
        rows->h_row_grp_off.assign(R + 1, 0);
        rows->h_grp_prob.resize(G);
        rows->h_grp_idx_off.assign(G + 1, 0);
        rows->h_path_idx.resize(M);
        if (R) {
            RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_row_count.data(), rows->row_count.ptr, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, st));
            RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_row_noise.data(), rows->row_noise.ptr, sizeof(double) * R, hipMemcpyDeviceToHost, st));
            RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_row_grp_off.data(), rows->row_grp_off.ptr, sizeof(uint64_t) * (R + 1), hipMemcpyDeviceToHost, st));
            RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_grp_idx_off.data(), rows->grp_idx_off.ptr, sizeof(uint64_t) * (G + 1), hipMemcpyDeviceToHost, st));
        }
        if (G) RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_grp_prob.data(), rows->grp_prob.ptr, sizeof(double) * G, hipMemcpyDeviceToHost, st));
        if (M) RPVG_HIP_CHECK(hipMemcpyAsync(rows->h_path_idx.data(), rows->path_idx.ptr, sizeof(uint32_t) * M, hipMemcpyDeviceToHost, st));
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        rows->downloaded = true;
    }
    std::memset(view, 0, sizeof(*view));
    view->num_clusters = rows->num_clusters;
    view->cluster_row_off = rows->h_cluster_row_off.data();
    view->cluster_path_off = rows->h_cluster_path_off.data();
    view->row_count = rows->h_row_count.data();
    view->row_noise = rows->h_row_noise.data();
    view->row_grp_off = rows->h_row_grp_off.data();
    view->grp_prob = rows->h_grp_prob.data();
    view->grp_idx_off = rows->h_grp_idx_off.data();
    view->path_idx = rows->h_path_idx.data();
    if (build_ms) *build_ms = rows->build_ms;
    if (merge_ms) *merge_ms = rows->merge_ms;
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_read_rows_sizes(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, rpvg_cluster_batch * view) {
    RPVG_REQUIRE(ctx && rows && view, "rpvg_hip_read_rows_sizes: NULL argument");
    std::memset(view, 0, sizeof(*view));
    view->num_clusters = rows->num_clusters;
    view->cluster_row_off = rows->h_cluster_row_off.data();
    view->cluster_path_off = rows->h_cluster_path_off.data();
    return RPVG_HIP_OK;
}

// the device arrays of the rows where they lie (rows_residents.hpp: rows_text.hip formats the --write-probs dump from them)
ReadRowsResident rpvg_hip_detail::residentOf(const rpvg_hip_read_rows * rows) {
    return ReadRowsResident{rows->num_clusters,       rows->num_rows,        rows->num_groups,      rows->num_members,   rows->h_cluster_row_off.data(),
                            rows->h_cluster_path_off.data(), rows->cluster_row_off.ptr, rows->row_grp_off.ptr, rows->grp_idx_off.ptr, rows->row_count.ptr,
                            rows->path_idx.ptr,       rows->row_noise.ptr,   rows->grp_prob.ptr};
}

// rows -> the device-resident batch the estimators take, without leaving the GPU: the shell and the routine of the upload
// (batch_upload.hip), over the rows' own 64-bit offsets; no validation (the rows were built here) and no path side: the batch has
// no read totals either, until attachPathSide brings both
// (the caller holds ctx->mutex and has set the device)
static int rowsToBatch(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, std::unique_ptr<rpvg_hip_batch> & b) {
    const uint32_t K = rows->num_clusters;
    const uint64_t R = rows->num_rows, M = rows->num_members;
    hipStream_t st = ctx->stream;
    hipError_t shell = hipSuccess;
    b = newBatchShell(K, R, M, rows->h_cluster_path_off[K], shell);
    if (!b) {
        setError("rpvg_hip_read_rows_to_batch: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    RPVG_HIP_CHECK(shell);
    b->h_cluster_row_off = rows->h_cluster_row_off;
    b->h_cluster_path_off = rows->h_cluster_path_off;
    RPVG_HIP_CHECK(b->cluster_row_off.upload(rows->h_cluster_row_off.data(), K + 1, st));
    RPVG_HIP_CHECK(b->cluster_path_off.upload(rows->h_cluster_path_off.data(), K + 1, st));
    RPVG_HIP_CHECK(b->row_noise.alloc(R));
    RPVG_HIP_CHECK(b->ent_path.alloc(M));
    DeviceBuffer<uint64_t> d_cluster_ent_off;
    RPVG_HIP_CHECK(d_cluster_ent_off.alloc(K + 1));
    const int span = ctx->spanBegin(FAM_BUILD);
    if (R) RPVG_HIP_CHECK(hipMemcpyAsync(b->row_noise.ptr, rows->row_noise.ptr, sizeof(double) * R, hipMemcpyDeviceToDevice, st));
    if (M) RPVG_HIP_CHECK(hipMemcpyAsync(b->ent_path.ptr, rows->path_idx.ptr, sizeof(uint32_t) * M, hipMemcpyDeviceToDevice, st));
    GroupedRows grouped;
    grouped.num_groups = rows->num_groups;
    grouped.row_grp_off = rows->row_grp_off.ptr;
    grouped.grp_idx_off = rows->grp_idx_off.ptr;
    grouped.grp_prob = rows->grp_prob.ptr;
    grouped.row_count_u32 = rows->row_count.ptr;
    const hipError_t queued = queueGroupedRows(st, grouped, b.get(), nullptr, d_cluster_ent_off.ptr);
    ctx->spanEnd(span);
    ctx->stats.build_launches += 3;
    RPVG_HIP_CHECK(queued);
    RPVG_HIP_CHECK(hipMemcpyAsync(b->h_cluster_ent_off.data(), d_cluster_ent_off.ptr, sizeof(uint64_t) * (K + 1), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_read_rows_to_batch(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, rpvg_hip_batch ** batch_out) {
    RPVG_REQUIRE(ctx && rows && batch_out, "rpvg_hip_read_rows_to_batch: NULL argument");
    *batch_out = nullptr;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<rpvg_hip_batch> b;
    if (const int rc = rowsToBatch(ctx, rows, b)) return rc;
    *batch_out = b.release();
    return RPVG_HIP_OK;
}

// the same with the path side of the batch from the resident path table (path_table.hip)
extern "C" int rpvg_hip_read_rows_to_batch_with_paths(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, const rpvg_hip_align_index * index,
                                                      const rpvg_hip_path_table * table, rpvg_hip_batch ** batch_out) {
    RPVG_REQUIRE(ctx && rows && index && table && batch_out, "rpvg_hip_read_rows_to_batch_with_paths: NULL argument");
    *batch_out = nullptr;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<rpvg_hip_batch> b;
    if (const int rc = rowsToBatch(ctx, rows, b)) return rc;
    if (const int rc = attachPathSide(ctx, b.get(), rows->row_count.ptr, index, table)) return rc;
    *batch_out = b.release();
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_read_rows_free(rpvg_hip_ctx * ctx, rpvg_hip_read_rows * rows) {
    if (!rows) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
    }
    delete rows;
}
