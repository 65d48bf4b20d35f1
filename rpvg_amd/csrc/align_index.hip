// align_index.hip — the alignment-path index on the GPU (interface include/rpvg_index.h).
//
// Takes over   addAlignmentPathsBufferToIndexes                         src/main.cpp:200-237
//              PathClusters from the lists (+ the sets of addNodeClusters)  src/path_clusters.cpp:12-262
//              the caller's loop: list -> cluster of its anchor path     src/main.cpp:731-754
//                                 clusters by descending (lists, index)  src/main.cpp:811-827
//                                 global path id -> cluster-local index  src/main.cpp:846-857
//
// The reference keeps a hash map of vector<AlignmentPath> on one thread.  Here the stream of lists is appended to flat device
// arrays chunk by chunk (add), and finish() runs
//   histogram   integer atomics, per workgroup in LDS when the bins fit;
//   hash        16 lanes per list: a sum of position-salted 64-bit mixes of the NORMALISED contents (the order of the
//               lanes does not matter), so that a list of three entries does not idle a wavefront;
//   sort        stable radix sort of (hash, stream index): equal lists are neighbours, earliest first;
//   heads       every member of a run of equal hashes is compared — contents, not hashes — with the run's first member; the
//               members that differ (hash collisions) and only they go to collisionKernel, one wavefront per run, which
//               keeps the distinct lists it has met and compares each such member with all of them, 64 at a time;
//   clusters    the union-find of path_clusters.hip on the lists' own path ids and the caller's extra sets;
//   order       clusters by descending (distinct lists, index) — one radix sort of K keys —, the distinct lists by a stable
//               sort on their cluster's rank, which keeps the ascending first occurrence inside a cluster;
//   gather      the cluster-ordered, cluster-local arrays of rpvg_alignment_batch.
// No kernel allocates; every array is sized by F, A, E (lists, alignments, entries of the stream) or P (paths).

#include "alignments.hpp"
#include "common.hpp"
#include "device_algos.hpp"
#include "path_clusters.hpp"
#include "path_table.hpp"
#include "table_kit.hpp"

using namespace rpvg_hip_detail;

namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kMaxItems = 0x7fffffffull;  // the sorts and scans count in int
constexpr uint32_t kLdsHistBins = 8192;        // 32 KiB of LDS per workgroup

// device array that grows by doubling (the stream is appended chunk by chunk)
template <typename T>
struct Growable {
    T * ptr = nullptr;
    size_t capacity = 0;
    Growable() {}
    Growable(const Growable &) = delete;
    Growable & operator=(const Growable &) = delete;
    ~Growable() { if (ptr) poolFree(ptr); }
    // room for `need` elements, the first `used` kept; waits for the copy before the old block goes back to the pool
    hipError_t reserve(const size_t need, const size_t used, hipStream_t st) {
        if (need <= capacity) return hipSuccess;
        const size_t cap = std::max<size_t>(std::max(need, capacity * 2), 1024);
        T * fresh = nullptr;
        hipError_t e = poolAlloc(reinterpret_cast<void **>(&fresh), cap * sizeof(T));
        if (e != hipSuccess) return e;
        if (used) {
            e = hipMemcpyAsync(fresh, ptr, used * sizeof(T), hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                poolFree(fresh);
                return e;
            }
        }
        if (ptr) poolFree(ptr);
        ptr = fresh;
        capacity = cap;
        return hipSuccess;
    }
};

// the stream as the kernels see it
struct StreamView {
    const uint8_t * is_simple;
    const uint8_t * min_mapq;
    const int32_t * noise_score;
    const uint64_t * list_align_off;
    const int32_t * score_sum;
    const uint16_t * align_length;
    const uint16_t * frag_length;
    const uint64_t * align_path_off;
    const uint32_t * path_id;
    uint16_t pre_frag_loc;
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // the finaliser of splitmix64: a bijection of 64 bits
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// The contents that take part in equality (operator== of src/alignment_path.cpp:96-104 over the list, the path-id list standing
// for the search state), after the normalisation of src/main.cpp:218-224: a list of one alignment has score 1, length 1 and
// the prior's location as its fragment length.
__device__ __forceinline__ bool listsEqual(const StreamView & v, const uint32_t x, const uint32_t y) {
    if (x == y) return true;
    if ((v.is_simple[x] != 0) != (v.is_simple[y] != 0) || v.min_mapq[x] != v.min_mapq[y] || v.noise_score[x] != v.noise_score[y]) return false;
    const uint64_t ax = v.list_align_off[x], ay = v.list_align_off[y];
    const uint64_t n = v.list_align_off[x + 1] - ax;
    if (n != v.list_align_off[y + 1] - ay) return false;
    for (uint64_t j = 0; j < n; ++j) {
        if (n > 1 && (v.score_sum[ax + j] != v.score_sum[ay + j] || v.align_length[ax + j] != v.align_length[ay + j] ||
                      v.frag_length[ax + j] != v.frag_length[ay + j])) {
            return false;
        }
        const uint64_t px = v.align_path_off[ax + j], py = v.align_path_off[ay + j];
        const uint64_t np = v.align_path_off[ax + j + 1] - px;
        if (np != v.align_path_off[ay + j + 1] - py) return false;
        for (uint64_t k = 0; k < np; ++k) {
            if (v.path_id[px + k] != v.path_id[py + k]) return false;
        }
    }
    return true;
}

// ---- add: validation of a chunk and its offsets moved behind the stream --------------------------------------------
enum BadReason { kBadListOffsets = 1, kBadNoise, kBadAlignOffsets, kBadPathId, kBadFragLength };

// one thread per list of the chunk; bad = min over the offending lists (table_kit.hpp)
__global__ __launch_bounds__(256) void validateChunkKernel(const uint64_t num_lists, const uint64_t num_aligns, const uint64_t num_entries,
                                                           const uint8_t * __restrict__ is_simple, const uint8_t * __restrict__ min_mapq,
                                                           const int32_t * __restrict__ noise_score, const uint64_t * __restrict__ list_align_off,
                                                           const uint16_t * __restrict__ frag_length, const uint64_t * __restrict__ align_path_off,
                                                           const uint32_t * __restrict__ path_id, const uint32_t num_paths, const bool count_frag,
                                                           const uint32_t frag_min_mapq, const uint32_t max_frag_length,
                                                           unsigned long long * __restrict__ bad) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= num_lists) return;
    int why = 0;
    const uint64_t a0 = list_align_off[i], a1 = list_align_off[i + 1];
    if (!(a0 < a1 && a1 <= num_aligns)) {
        why = kBadListOffsets;
    } else if (noise_score[i] > 0) {
        why = kBadNoise;
    } else {
        for (uint64_t a = a0; a < a1 && !why; ++a) {
            const uint64_t p0 = align_path_off[a], p1 = align_path_off[a + 1];
            if (!(p0 < p1 && p1 <= num_entries)) {
                why = kBadAlignOffsets;
                break;
            }
            for (uint64_t e = p0; e < p1; ++e) {
                if (path_id[e] >= num_paths || (e > p0 && path_id[e - 1] >= path_id[e])) {
                    why = kBadPathId;
                    break;
                }
            }
        }
        if (!why && count_frag && is_simple[i] != 0 && min_mapq[i] >= frag_min_mapq) {
            const uint32_t fl = frag_length[a0];
            if (fl == 0 || fl > max_frag_length) why = kBadFragLength;
        }
    }
    if (why) reportOffender(bad, i, why);
}

// out[base_index + i] = raw[i] + base_value for i = 0 .. n (n + 1 offsets)
__global__ void rebaseOffsetsKernel(const uint64_t n, const uint64_t * __restrict__ raw, const uint64_t base_value, uint64_t * __restrict__ out) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i <= n) out[i] = raw[i] + base_value;
}

// ---- finish ---------------------------------------------------------------------------------------------------------
// counts[front.frag_length]++ iff is_simple && min_mapq >= frag_length_min_mapq (src/main.cpp:213-216), before normalisation
__global__ __launch_bounds__(256) void fragHistKernel(const uint64_t num_lists, const StreamView v, const uint32_t frag_min_mapq, const uint32_t bins,
                                                      const bool use_lds, uint32_t * __restrict__ hist) {
    extern __shared__ uint32_t lds_hist[];
    if (use_lds) {
        for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x) lds_hist[b] = 0;
        __syncthreads();
    }
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < num_lists; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        if (v.is_simple[i] != 0 && v.min_mapq[i] >= frag_min_mapq) {
            const uint32_t fl = v.frag_length[v.list_align_off[i]];
            if (fl < bins) atomicAdd(use_lds ? lds_hist + fl : hist + fl, 1u);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x) {
            if (lds_hist[b]) atomicAdd(hist + b, lds_hist[b]);
        }
    }
}

// first (alignment, path) entry of every list, and the end of the last one: the lists' path ids as id sets
__global__ void listEntryOffKernel(const uint64_t num_lists, const uint64_t * __restrict__ list_align_off,
                                   const uint64_t * __restrict__ align_path_off, uint64_t * __restrict__ list_ent_off) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i <= num_lists) list_ent_off[i] = align_path_off[list_align_off[i]];
}

__device__ __forceinline__ uint64_t groupSum64(uint64_t x) {  // over the 16 lanes of a group, in every lane
    for (int d = kGroupLanes / 2; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(x), d, kGroupLanes);
        const uint32_t hi = __shfl_xor(static_cast<uint32_t>(x >> 32), d, kGroupLanes);
        x += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return x;
}

// 16 lanes per list.  The hash is a SUM of one term per alignment (position, normalised score and lengths, number of paths: the
// alignment boundaries) and one per entry (position in the list, path id), so that lanes may take them in any order, mixed
// with the list's own fields.  Only equality of the hashes of equal lists is relied upon.
__global__ __launch_bounds__(256) void hashListsKernel(const uint64_t num_lists, const StreamView v, const uint64_t * __restrict__ list_ent_off,
                                                       const uint64_t hash_mask, uint64_t * __restrict__ key, uint32_t * __restrict__ list) {
    const int g = threadIdx.x & (kGroupLanes - 1);
    const uint64_t i = (blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x) / kGroupLanes;
    const bool active = i < num_lists;
    uint64_t sum = 0, n = 0;
    if (active) {
        const uint64_t a0 = v.list_align_off[i];
        n = v.list_align_off[i + 1] - a0;
        for (uint64_t j = g; j < n; j += kGroupLanes) {
            const uint64_t a = a0 + j;
            const uint32_t score = n > 1 ? static_cast<uint32_t>(v.score_sum[a]) : 1u;
            const uint64_t alen = n > 1 ? v.align_length[a] : 1, flen = n > 1 ? v.frag_length[a] : v.pre_frag_loc;
            const uint64_t np = v.align_path_off[a + 1] - v.align_path_off[a];
            sum += mix64(mix64((((j + 1) << 32) | score) ^ 0x9e3779b97f4a7c15ull) + (alen | (flen << 16) | (np << 32)));
        }
        const uint64_t e0 = list_ent_off[i], ne = list_ent_off[i + 1] - e0;
        for (uint64_t k = g; k < ne; k += kGroupLanes) sum += mix64((((k + 1) << 32) | v.path_id[e0 + k]) + 0xd1b54a32d192ed03ull);
    }
    sum = groupSum64(sum);
    if (active && g == 0) {
        const uint64_t header = static_cast<uint32_t>(v.noise_score[i]) | (static_cast<uint64_t>(v.min_mapq[i]) << 32) |
                                (static_cast<uint64_t>(v.is_simple[i] != 0) << 40);
        key[i] = mix64(sum ^ mix64(header + n * 0x8cb92ba72f3d8dd7ull)) & hash_mask;
        list[i] = static_cast<uint32_t>(i);
    }
}

// start_or_zero[i] = i where a run of equal keys starts: an inclusive maximum scan turns it into every member's run start
__global__ void runFlagKernel(const uint64_t n, const uint64_t * __restrict__ key_sorted, uint32_t * __restrict__ start_or_zero) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < n) start_or_zero[i] = (i > 0 && key_sorted[i] != key_sorted[i - 1]) ? static_cast<uint32_t>(i) : 0u;
}

// every member against the first member of its run; the sort was stable, so that one is the earliest list of the run
__global__ __launch_bounds__(256) void compareWithHeadKernel(const uint64_t n, const StreamView v, const uint32_t * __restrict__ list_sorted,
                                                             const uint32_t * __restrict__ run_start, uint32_t * __restrict__ rep,
                                                             uint32_t * __restrict__ differs) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = list_sorted[i], h = list_sorted[run_start[i]];
    const bool same = listsEqual(v, m, h);
    if (same) rep[m] = h;
    differs[i] = same ? 0u : 1u;
}

__global__ void compactFlaggedKernel(const uint64_t n, const uint32_t * __restrict__ flag, const uint32_t * __restrict__ pos,
                                     uint32_t * __restrict__ out) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < n && flag[i]) out[pos[i]] = static_cast<uint32_t>(i);
}

// The collision path: `collided` lists the sorted positions of the members that differ from their run's head, ascending — the
// members of one run together, earliest first.  One wavefront per run (the block of the run's first such member; the others
// leave): it keeps the distinct lists met so far in met[first .. first + h) and compares each member with all of them, 64 per
// step.  Walks only these members, never a run.
__global__ __launch_bounds__(64) void collisionKernel(const uint32_t num_collided, const uint32_t * __restrict__ collided, const StreamView v,
                                                      const uint32_t * __restrict__ list_sorted, const uint32_t * __restrict__ run_start,
                                                      uint32_t * met, uint32_t * __restrict__ rep) {
    const uint32_t first = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t run = run_start[collided[first]];
    if (first > 0 && run_start[collided[first - 1]] == run) return;
    uint32_t h = 0;
    for (uint32_t t = first; t < num_collided && run_start[collided[t]] == run; ++t) {
        const uint32_t m = list_sorted[collided[t]];
        uint32_t found = kNone;
        for (uint32_t k = lane; k < h; k += 64) {
            const uint32_t other = __hip_atomic_load(met + first + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (listsEqual(v, m, other)) found = other;
        }
        const unsigned long long votes = __ballot(found != kNone);
        if (votes) {  // the met lists differ from one another: at most one lane found it
            const uint32_t r = __shfl(found, __ffsll(votes) - 1, 64);
            if (lane == 0) rep[m] = r;
        } else {
            if (lane == 0) {
                __hip_atomic_store(met + first + h, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                rep[m] = m;
            }
            ++h;
            __threadfence();
        }
    }
}

// multiplicity of every distinct list (at its first occurrence) and the flag of being one
__global__ void countMembersKernel(const uint64_t n, const uint32_t * __restrict__ rep, uint32_t * __restrict__ multiplicity,
                                   uint32_t * __restrict__ is_distinct) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rep[i];
    atomicAdd(multiplicity + r, 1u);
    is_distinct[i] = r == i ? 1u : 0u;
}

// a distinct list belongs to the cluster of the first path of its first alignment (src/main.cpp:746-748)
__global__ void listClusterKernel(const uint64_t num_distinct, const uint32_t * __restrict__ distinct, const uint64_t * __restrict__ list_ent_off,
                                  const uint32_t * __restrict__ path_id, const uint32_t * __restrict__ path_to_cluster,
                                  uint32_t * __restrict__ list_cluster, uint32_t * __restrict__ cluster_lists) {
    const uint64_t d = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (d >= num_distinct) return;
    const uint32_t c = path_to_cluster[path_id[list_ent_off[distinct[d]]]];
    list_cluster[d] = c;
    atomicAdd(cluster_lists + c, 1u);
}

__global__ void rankKeyKernel(const uint32_t num_clusters, const uint32_t * __restrict__ cluster_lists, uint64_t * __restrict__ rank_key) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < num_clusters) rank_key[c] = (static_cast<uint64_t>(cluster_lists[c]) << 32) | c;
}

// keys in descending order = sort(rbegin, rend) of (number of lists, cluster index), src/main.cpp:827
__global__ void rankClustersKernel(const uint32_t num_clusters, const uint64_t * __restrict__ rank_key_sorted, const uint64_t * __restrict__ cluster_off,
                                   uint32_t * __restrict__ rank_cluster, uint32_t * __restrict__ cluster_rank, uint64_t * __restrict__ rank_lists,
                                   uint64_t * __restrict__ rank_paths) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > num_clusters) return;
    if (r == num_clusters) {  // the scans run over K + 1 cells
        rank_lists[r] = 0;
        rank_paths[r] = 0;
        return;
    }
    const uint32_t c = static_cast<uint32_t>(rank_key_sorted[r]);
    rank_cluster[r] = c;
    cluster_rank[c] = r;
    rank_lists[r] = rank_key_sorted[r] >> 32;
    rank_paths[r] = cluster_off[c + 1] - cluster_off[c];
}

__global__ void listRankKernel(const uint64_t num_distinct, const uint32_t * __restrict__ list_cluster, const uint32_t * __restrict__ cluster_rank,
                               uint32_t * __restrict__ list_rank) {
    const uint64_t d = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (d < num_distinct) list_rank[d] = cluster_rank[list_cluster[d]];
}

// sizes of the lists in output order (D + 1 cells for the scans) and the small / large split of the row kernels
__global__ void orderedSizesKernel(const uint64_t num_distinct, const uint32_t * __restrict__ ordered, const uint64_t * __restrict__ list_align_off,
                                   const uint64_t * __restrict__ list_ent_off, uint64_t * __restrict__ num_aligns, uint64_t * __restrict__ num_entries,
                                   uint32_t * __restrict__ is_small) {
    const uint64_t d = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (d > num_distinct) return;
    if (d == num_distinct) {
        num_aligns[d] = 0;
        num_entries[d] = 0;
        is_small[d] = 0;
        return;
    }
    const uint32_t l = ordered[d];
    num_aligns[d] = list_align_off[l + 1] - list_align_off[l];
    const uint64_t ne = list_ent_off[l + 1] - list_ent_off[l];
    num_entries[d] = ne;
    is_small[d] = rpvg_rows_plan::readIsSmall(ne, false) ? 1u : 0u;  // where the rows collapse, fillAlignments lists every read as large
}

// position of every path in its cluster's ascending member list (src/main.cpp:855-857) and the members in rank order
__global__ void localIndexKernel(const uint32_t num_paths, const uint32_t * __restrict__ path_sorted, const uint32_t * __restrict__ path_to_cluster,
                                 const uint64_t * __restrict__ cluster_off, const uint32_t * __restrict__ cluster_rank,
                                 const uint64_t * __restrict__ out_cluster_path_off, uint32_t * __restrict__ local_index,
                                 uint32_t * __restrict__ out_cluster_paths) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_paths) return;
    const uint32_t p = path_sorted[i], c = path_to_cluster[p];
    const uint32_t local = i - static_cast<uint32_t>(cluster_off[c]);
    local_index[p] = local;
    out_cluster_paths[out_cluster_path_off[cluster_rank[c]] + local] = p;
}

struct OrderedOut {
    uint32_t * read_count;
    uint8_t * read_min_mapq;
    int32_t * read_noise_score;
    uint64_t * first_occurrence;
    int32_t * align_score_sum;
    uint16_t * align_length;
    uint16_t * align_frag_length;
    uint64_t * align_path_off;
    uint32_t * align_path_idx;
};

// one thread per distinct list, in output order: its normalised alignments and cluster-local path indices
__global__ __launch_bounds__(256) void gatherListsKernel(const uint64_t num_distinct, const uint64_t total_aligns, const uint64_t total_entries,
                                                         const uint32_t * __restrict__ ordered, const StreamView v,
                                                         const uint32_t * __restrict__ multiplicity, const uint32_t * __restrict__ local_index,
                                                         const uint64_t * __restrict__ out_align_off, const uint64_t * __restrict__ out_ent_off,
                                                         const OrderedOut out) {
    const uint64_t d = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (d == 0) out.align_path_off[total_aligns] = total_entries;
    if (d >= num_distinct) return;
    const uint32_t l = ordered[d];
    out.read_count[d] = multiplicity[l];
    out.read_min_mapq[d] = v.min_mapq[l];
    out.read_noise_score[d] = v.noise_score[l];
    out.first_occurrence[d] = l;
    const uint64_t a0 = v.list_align_off[l], n = v.list_align_off[l + 1] - a0;
    const uint64_t e0 = v.align_path_off[a0], ne = v.align_path_off[a0 + n] - e0;
    const uint64_t oa = out_align_off[d], oe = out_ent_off[d];
    for (uint64_t j = 0; j < n; ++j) {
        out.align_score_sum[oa + j] = n > 1 ? v.score_sum[a0 + j] : 1;
        out.align_length[oa + j] = n > 1 ? v.align_length[a0 + j] : static_cast<uint16_t>(1);
        out.align_frag_length[oa + j] = n > 1 ? v.frag_length[a0 + j] : v.pre_frag_loc;
        out.align_path_off[oa + j] = oe + (v.align_path_off[a0 + j] - e0);
    }
    for (uint64_t k = 0; k < ne; ++k) out.align_path_idx[oe + k] = local_index[v.path_id[e0 + k]];
}

// the ascending lists of small and large reads (rpvg_hip_alignments): pos = exclusive count of small ones before d
__global__ void splitBySizeKernel(const uint64_t num_distinct, const uint32_t * __restrict__ is_small, const uint32_t * __restrict__ pos,
                                  uint32_t * __restrict__ small_reads, uint32_t * __restrict__ large_reads) {
    const uint64_t d = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (d >= num_distinct) return;
    if (is_small[d]) small_reads[pos[d]] = static_cast<uint32_t>(d);
    else large_reads[d - pos[d]] = static_cast<uint32_t>(d);
}

template <typename T>
__global__ void gatherByPathKernel(const uint32_t num_paths, const uint32_t * __restrict__ cluster_paths, const T * __restrict__ by_global_path,
                                   T * __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < num_paths) out[i] = by_global_path[cluster_paths[i]];
}

// one array of a chunk behind the stream's: from the caller's own pinned memory directly, else through a pinned block of the
// library's (kept in `staging` until the copies are done), as DeviceBuffer::upload does
template <typename T>
hipError_t appendFromHost(T * device_dst, const T * host, const size_t n, hipStream_t st, std::vector<void *> & staging) {
    if (n == 0) return hipSuccess;
    const size_t bytes = n * sizeof(T);
    if (hostIsPinned(host, bytes)) return hipMemcpyAsync(device_dst, host, bytes, hipMemcpyHostToDevice, st);
    void * block = nullptr;
    if (stagedUploads() && pinnedAlloc(&block, bytes) == hipSuccess) {
        staging.push_back(block);
        copyToStaging(block, host, bytes);
        return stagedCopy(device_dst, block, bytes, st);
    }
    return hipMemcpyAsync(device_dst, host, bytes, hipMemcpyHostToDevice, st);
}

struct StagingBlocks {
    std::vector<void *> blocks;
    ~StagingBlocks() { for (void * b : blocks) pinnedFree(b); }
};

template <typename T>
int copyBuffer(hipStream_t st, DeviceBuffer<T> & to, const DeviceBuffer<T> & from, const size_t n) {
    RPVG_HIP_CHECK(to.alloc(n));
    if (n) RPVG_HIP_CHECK(hipMemcpyAsync(to.ptr, from.ptr, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    return RPVG_HIP_OK;
}

}  // namespace

struct rpvg_hip_align_index {
    rpvg_index_params params;
    bool finished = false;
    // the stream: F lists, A alignments, E entries
    uint64_t F = 0, A = 0, E = 0;
    Growable<uint8_t> is_simple, min_mapq;
    Growable<int32_t> noise_score, score_sum;
    Growable<uint64_t> list_align_off, align_path_off;
    Growable<uint16_t> align_length, frag_length;
    Growable<uint32_t> path_id;
    // the result: D distinct lists with DA alignments and DE entries in K clusters, rank order
    uint64_t D = 0, DA = 0, DE = 0, num_collided = 0, num_small = 0;
    uint32_t K = 0;
    DeviceBuffer<uint32_t> frag_counts;
    DeviceBuffer<uint32_t> rank_cluster, path_to_cluster, cluster_paths, read_cluster, read_count, align_path_idx, small_reads, large_reads;
    DeviceBuffer<uint64_t> cluster_read_off, cluster_path_off, read_align_off, out_align_path_off, first_occurrence;
    DeviceBuffer<uint8_t> read_min_mapq;
    DeviceBuffer<int32_t> read_noise_score, out_score_sum;
    DeviceBuffer<uint16_t> out_align_length, out_frag_length;
    std::vector<uint64_t> h_cluster_read_off, h_cluster_path_off;
    // host copies (rpvg_hip_align_index_view)
    bool downloaded = false;
    std::vector<uint32_t> h_rank_cluster, h_path_to_cluster, h_cluster_paths, h_read_count, h_align_path_idx;
    std::vector<uint64_t> h_read_align_off, h_align_path_off, h_first_occurrence;
    std::vector<uint8_t> h_read_min_mapq;
    std::vector<int32_t> h_read_noise_score, h_score_sum;
    std::vector<uint16_t> h_align_length, h_frag_length;

    StreamView view() const {
        return StreamView{is_simple.ptr, min_mapq.ptr, noise_score.ptr, list_align_off.ptr, score_sum.ptr, align_length.ptr,
                          frag_length.ptr, align_path_off.ptr, path_id.ptr, params.pre_frag_loc};
    }
};

extern "C" int rpvg_hip_align_index_create(rpvg_hip_ctx * ctx, const rpvg_index_params * params, rpvg_hip_align_index ** index_out) {
    RPVG_REQUIRE(ctx && params && index_out, "rpvg_hip_align_index_create: NULL argument");
    *index_out = nullptr;
    RPVG_REQUIRE(params->max_frag_length < RPVG_FRAG_LENGTH_TABLE_SIZE, "rpvg_hip_align_index_create: max_frag_length %u: fragment lengths are 16 bits",
                 params->max_frag_length);
    RPVG_REQUIRE(params->num_paths < kMaxItems, "rpvg_hip_align_index_create: %u paths exceed one index", params->num_paths);
    rpvg_hip_align_index * index = new (std::nothrow) rpvg_hip_align_index();
    if (!index) {
        setError("rpvg_hip_align_index_create: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    index->params = *params;
    *index_out = index;
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_align_index_free(rpvg_hip_ctx * ctx, rpvg_hip_align_index * index) {
    if (!index) return;
    waitAndDelete(ctx);
    delete index;
}

extern "C" int rpvg_hip_align_index_add(rpvg_hip_ctx * ctx, rpvg_hip_align_index * ix, const rpvg_fragment_lists * chunk) {
    RPVG_REQUIRE(ctx && ix && chunk, "rpvg_hip_align_index_add: NULL argument");
    RPVG_REQUIRE(!ix->finished, "rpvg_hip_align_index_add: the index is finished");
    const uint64_t Fc = chunk->num_lists;
    if (Fc == 0) return RPVG_HIP_OK;
    RPVG_REQUIRE(chunk->list_is_simple && chunk->list_min_mapq && chunk->list_noise_score && chunk->list_align_off && chunk->align_score_sum &&
                 chunk->align_length && chunk->align_frag_length && chunk->align_path_off && chunk->align_path_id,
                 "rpvg_hip_align_index_add: NULL array");
    RPVG_REQUIRE(Fc < kMaxItems, "rpvg_hip_align_index_add: %llu lists exceed one index", static_cast<unsigned long long>(Fc));
    RPVG_REQUIRE(chunk->list_align_off[0] == 0, "rpvg_hip_align_index_add: list_align_off[0] is not 0");
    const uint64_t Ac = chunk->list_align_off[Fc];
    RPVG_REQUIRE(Ac < kMaxItems, "rpvg_hip_align_index_add: %llu alignments exceed one index", static_cast<unsigned long long>(Ac));
    RPVG_REQUIRE(chunk->align_path_off[0] == 0, "rpvg_hip_align_index_add: align_path_off[0] is not 0");
    const uint64_t Ec = chunk->align_path_off[Ac];
    RPVG_REQUIRE(Ec < kMaxItems, "rpvg_hip_align_index_add: %llu path entries exceed one index", static_cast<unsigned long long>(Ec));
    const uint64_t F = ix->F, A = ix->A, E = ix->E;
    RPVG_REQUIRE(F + Fc < kMaxItems && A + Ac < kMaxItems && E + Ec < kMaxItems, "rpvg_hip_align_index_add: the stream exceeds one index (2^31 - 1 lists, alignments, entries)");

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RPVG_HIP_CHECK(ix->is_simple.reserve(F + Fc, F, st));
    RPVG_HIP_CHECK(ix->min_mapq.reserve(F + Fc, F, st));
    RPVG_HIP_CHECK(ix->noise_score.reserve(F + Fc, F, st));
    RPVG_HIP_CHECK(ix->list_align_off.reserve(F + Fc + 1, F ? F + 1 : 0, st));
    RPVG_HIP_CHECK(ix->score_sum.reserve(A + Ac, A, st));
    RPVG_HIP_CHECK(ix->align_length.reserve(A + Ac, A, st));
    RPVG_HIP_CHECK(ix->frag_length.reserve(A + Ac, A, st));
    RPVG_HIP_CHECK(ix->align_path_off.reserve(A + Ac + 1, A ? A + 1 : 0, st));
    RPVG_HIP_CHECK(ix->path_id.reserve(E + Ec, E, st));

    StagingBlocks staging;
    DeviceBuffer<uint64_t> raw_list_off, raw_align_off;
    DeviceBuffer<unsigned long long> d_bad;
    unsigned long long bad = kNoBad;
    int span = ctx->spanBegin(FAM_H2D);
    RPVG_HIP_CHECK(appendFromHost(ix->is_simple.ptr + F, chunk->list_is_simple, Fc, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->min_mapq.ptr + F, chunk->list_min_mapq, Fc, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->noise_score.ptr + F, chunk->list_noise_score, Fc, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->score_sum.ptr + A, chunk->align_score_sum, Ac, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->align_length.ptr + A, chunk->align_length, Ac, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->frag_length.ptr + A, chunk->align_frag_length, Ac, st, staging.blocks));
    RPVG_HIP_CHECK(appendFromHost(ix->path_id.ptr + E, chunk->align_path_id, Ec, st, staging.blocks));
    RPVG_HIP_CHECK(raw_list_off.upload(chunk->list_align_off, Fc + 1, st));
    RPVG_HIP_CHECK(raw_align_off.upload(chunk->align_path_off, Ac + 1, st));
    RPVG_HIP_CHECK(d_bad.upload(&kNoBad, 1, st));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(Fc) * 14 + static_cast<double>(Ac) * 16 + static_cast<double>(Ec) * 4;

    span = ctx->spanBegin(FAM_BUILD);
    validateChunkKernel<<<gridFor(Fc), dim3(256), 0, st>>>(Fc, Ac, Ec, ix->is_simple.ptr + F, ix->min_mapq.ptr + F, ix->noise_score.ptr + F,
                                                          raw_list_off.ptr, ix->frag_length.ptr + A, raw_align_off.ptr, ix->path_id.ptr + E,
                                                          ix->params.num_paths, ix->params.is_single_end == 0, ix->params.frag_length_min_mapq,
                                                          ix->params.max_frag_length, d_bad.ptr);
    rebaseOffsetsKernel<<<gridFor(Fc + 1), dim3(256), 0, st>>>(Fc, raw_list_off.ptr, A, ix->list_align_off.ptr + F);
    rebaseOffsetsKernel<<<gridFor(Ac + 1), dim3(256), 0, st>>>(Ac, raw_align_off.ptr, E, ix->align_path_off.ptr + A);
    ctx->spanEnd(span);
    ctx->stats.build_launches += 3;
    RPVG_HIP_CHECK(hipGetLastError());
    if (const int rc = fetchDescribed(st, d_bad.ptr, &bad)) return rc;
    if (bad != kNoBad) {
        // the cells behind the stream's end were written and are not part of it (the offset AT its end was rewritten with its own value)
        static const char * const reasons[] = {"", "has no alignments or its offsets are not monotone", "has a positive noise score",
                                               "has an alignment without paths or with offsets that are not monotone",
                                               "has path ids that are not ascending or not below num_paths",
                                               "is counted for the fragment lengths with a length of 0 or above max_frag_length"};
        const Offender o = offenderOf(bad, kBadFragLength);
        const unsigned long long list = o.index;
        setError("rpvg_hip_align_index_add: list %llu of the chunk (%llu of the stream) %s", list, static_cast<unsigned long long>(F) + list,
                 reasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    ix->F = F + Fc;
    ix->A = A + Ac;
    ix->E = E + Ec;
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_align_index_finish(rpvg_hip_ctx * ctx, rpvg_hip_align_index * ix, const uint64_t * extra_set_off,
                                           const uint32_t * extra_set_path, uint64_t num_extra_sets, rpvg_index_info * info) {
    RPVG_REQUIRE(ctx && ix, "rpvg_hip_align_index_finish: NULL argument");
    RPVG_REQUIRE(!ix->finished, "rpvg_hip_align_index_finish: the index is finished already");
    RPVG_REQUIRE(num_extra_sets == 0 || (extra_set_off && extra_set_path), "rpvg_hip_align_index_finish: NULL set arrays");
    const uint32_t P = ix->params.num_paths;
    const uint64_t num_extra_members = num_extra_sets ? extra_set_off[num_extra_sets] : 0;
    RPVG_REQUIRE(num_extra_sets == 0 || P > 0, "rpvg_hip_align_index_finish: id sets without paths");
    for (uint64_t s = 0; s < num_extra_sets; ++s) {
        RPVG_REQUIRE(extra_set_off[s] < extra_set_off[s + 1], "rpvg_hip_align_index_finish: set %llu is empty", static_cast<unsigned long long>(s));
    }
    for (uint64_t e = 0; e < num_extra_members; ++e) {
        RPVG_REQUIRE(extra_set_path[e] < P, "rpvg_hip_align_index_finish: path id %u of %u", extra_set_path[e], P);
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t F = ix->F;
    const StreamView v = ix->view();
    const dim3 block(256);
    const int span = ctx->spanBegin(FAM_BUILD);

    // ---- histogram
    const uint32_t bins = ix->params.max_frag_length + 1;
    RPVG_HIP_CHECK(ix->frag_counts.alloc(bins));
    RPVG_HIP_CHECK(zeroAsync(ix->frag_counts.ptr, sizeof(uint32_t) * bins, st));
    if (F && !ix->params.is_single_end) {
        const bool use_lds = bins <= kLdsHistBins;
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((F + 255) / 256, 2048));
        fragHistKernel<<<dim3(blocks), block, use_lds ? bins * sizeof(uint32_t) : 0, st>>>(F, v, ix->params.frag_length_min_mapq, bins, use_lds,
                                                                                         ix->frag_counts.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
    }

    // ---- equal lists: hash, sort, compare with the run's head, collisions
    DeviceBuffer<uint64_t> list_ent_off;
    DeviceBuffer<uint32_t> rep, multiplicity, is_distinct;
    uint64_t num_collided = 0;
    if (F) {
        RPVG_HIP_CHECK(list_ent_off.alloc(F + 1));
        listEntryOffKernel<<<gridFor(F + 1), block, 0, st>>>(F, v.list_align_off, v.align_path_off, list_ent_off.ptr);
        DeviceBuffer<uint64_t> key, key_sorted;
        DeviceBuffer<uint32_t> list, list_sorted, run_flag, run_start, differs, differs_pos;
        RPVG_HIP_CHECK(key.alloc(F));
        RPVG_HIP_CHECK(key_sorted.alloc(F));
        RPVG_HIP_CHECK(list.alloc(F));
        RPVG_HIP_CHECK(list_sorted.alloc(F));
        RPVG_HIP_CHECK(run_flag.alloc(F));
        RPVG_HIP_CHECK(run_start.alloc(F));
        RPVG_HIP_CHECK(differs.alloc(F));
        RPVG_HIP_CHECK(differs_pos.alloc(F));
        RPVG_HIP_CHECK(rep.alloc(F));
        const uint32_t hash_bits = (ix->params.hash_bits == 0 || ix->params.hash_bits >= 64) ? 64 : ix->params.hash_bits;
        const uint64_t hash_mask = hash_bits == 64 ? ~0ull : ((1ull << hash_bits) - 1);
        hashListsKernel<<<gridFor(F, 256 / kGroupLanes), block, 0, st>>>(F, v, list_ent_off.ptr, hash_mask, key.ptr, list.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = sortPairs(st, key.ptr, key_sorted.ptr, list.ptr, list_sorted.ptr, F, static_cast<int>(hash_bits))) return rc;
        runFlagKernel<<<gridFor(F), block, 0, st>>>(F, key_sorted.ptr, run_flag.ptr);
        if (const int rc = inclusiveScan(st, run_flag.ptr, run_start.ptr, MaxU32(), F)) return rc;
        compareWithHeadKernel<<<gridFor(F), block, 0, st>>>(F, v, list_sorted.ptr, run_start.ptr, rep.ptr, differs.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = exclusiveSum(st, differs.ptr, differs_pos.ptr, F)) return rc;
        uint32_t last_pos = 0, last_flag = 0;
        if (const int rc = fetchOne(st, differs_pos.ptr + (F - 1), &last_pos)) return rc;
        if (const int rc = fetchOne(st, differs.ptr + (F - 1), &last_flag)) return rc;
        num_collided = static_cast<uint64_t>(last_pos) + last_flag;
        if (num_collided) {
            DeviceBuffer<uint32_t> collided, met;
            RPVG_HIP_CHECK(collided.alloc(num_collided));
            RPVG_HIP_CHECK(met.alloc(num_collided));
            compactFlaggedKernel<<<gridFor(F), block, 0, st>>>(F, differs.ptr, differs_pos.ptr, collided.ptr);
            collisionKernel<<<dim3(static_cast<uint32_t>(num_collided)), dim3(64), 0, st>>>(static_cast<uint32_t>(num_collided), collided.ptr, v,
                                                                                          list_sorted.ptr, run_start.ptr, met.ptr, rep.ptr);
            RPVG_HIP_CHECK(hipGetLastError());
            RPVG_HIP_CHECK(hipStreamSynchronize(st));
        }
        RPVG_HIP_CHECK(multiplicity.alloc(F));
        RPVG_HIP_CHECK(is_distinct.alloc(F));
        RPVG_HIP_CHECK(zeroAsync(multiplicity.ptr, sizeof(uint32_t) * F, st));
        countMembersKernel<<<gridFor(F), block, 0, st>>>(F, rep.ptr, multiplicity.ptr, is_distinct.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the sort's buffers leave scope
    }

    // ---- distinct lists in stream order
    uint64_t D = 0;
    DeviceBuffer<uint32_t> distinct_pos, distinct;
    if (F) {
        RPVG_HIP_CHECK(distinct_pos.alloc(F));
        if (const int rc = exclusiveSum(st, is_distinct.ptr, distinct_pos.ptr, F)) return rc;
        uint32_t last_pos = 0, last_flag = 0;
        if (const int rc = fetchOne(st, distinct_pos.ptr + (F - 1), &last_pos)) return rc;
        if (const int rc = fetchOne(st, is_distinct.ptr + (F - 1), &last_flag)) return rc;
        D = static_cast<uint64_t>(last_pos) + last_flag;
        RPVG_HIP_CHECK(distinct.alloc(D));
        compactFlaggedKernel<<<gridFor(F), block, 0, st>>>(F, is_distinct.ptr, distinct_pos.ptr, distinct.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
    }

    // ---- clusters: the paths of every list and of every extra set end up together
    PathClustersDevice pc;
    uint32_t K = 0;
    if (P) {
        if (const int rc = pc.begin(ctx, st, P)) return rc;
        if (const int rc = pc.unite(st, F, list_ent_off.ptr, v.path_id)) return rc;
        DeviceBuffer<uint64_t> d_set_off;
        DeviceBuffer<uint32_t> d_set_path;
        if (num_extra_members) {
            RPVG_HIP_CHECK(d_set_off.upload(extra_set_off, num_extra_sets + 1, st));
            RPVG_HIP_CHECK(d_set_path.upload(extra_set_path, num_extra_members, st));
            if (const int rc = pc.unite(st, num_extra_sets, d_set_off.ptr, d_set_path.ptr)) return rc;
        }
        if (const int rc = pc.finish(st)) return rc;  // synchronises: the sets leave scope
        K = pc.num_clusters;
    }

    // ---- rank order of the clusters, output order of the lists
    DeviceBuffer<uint32_t> list_cluster, cluster_lists, cluster_rank, list_rank, ordered, local_index, is_small, small_pos;
    DeviceBuffer<uint64_t> rank_key, rank_key_sorted, rank_lists, rank_paths, ordered_aligns, ordered_entries, out_ent_off;
    RPVG_HIP_CHECK(ix->cluster_read_off.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(ix->cluster_path_off.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(ix->rank_cluster.alloc(K));
    RPVG_HIP_CHECK(ix->cluster_paths.alloc(P));
    RPVG_HIP_CHECK(ix->read_cluster.alloc(D));
    if (K) {
        RPVG_HIP_CHECK(cluster_lists.alloc(K));
        RPVG_HIP_CHECK(cluster_rank.alloc(K));
        RPVG_HIP_CHECK(rank_key.alloc(K));
        RPVG_HIP_CHECK(rank_key_sorted.alloc(K));
        RPVG_HIP_CHECK(rank_lists.alloc(static_cast<size_t>(K) + 1));
        RPVG_HIP_CHECK(rank_paths.alloc(static_cast<size_t>(K) + 1));
        RPVG_HIP_CHECK(local_index.alloc(P));
        RPVG_HIP_CHECK(zeroAsync(cluster_lists.ptr, sizeof(uint32_t) * K, st));
        if (D) {
            RPVG_HIP_CHECK(list_cluster.alloc(D));
            listClusterKernel<<<gridFor(D), block, 0, st>>>(D, distinct.ptr, list_ent_off.ptr, v.path_id, pc.label.ptr, list_cluster.ptr, cluster_lists.ptr);
        }
        rankKeyKernel<<<gridFor(K), block, 0, st>>>(K, cluster_lists.ptr, rank_key.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        {
            size_t bytes = 0;
            RPVG_HIP_CHECK(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, bytes, rank_key.ptr, rank_key_sorted.ptr, static_cast<int>(K), 0, 64, st));
            DeviceBuffer<uint8_t> tmp;
            RPVG_HIP_CHECK(tmp.alloc(bytes ? bytes : 1));
            RPVG_HIP_CHECK(hipcub::DeviceRadixSort::SortKeysDescending(tmp.ptr, bytes, rank_key.ptr, rank_key_sorted.ptr, static_cast<int>(K), 0, 64, st));
            RPVG_HIP_CHECK(hipStreamSynchronize(st));
        }
        rankClustersKernel<<<gridFor(static_cast<uint64_t>(K) + 1), block, 0, st>>>(K, rank_key_sorted.ptr, pc.cluster_off.ptr, ix->rank_cluster.ptr,
                                                                                   cluster_rank.ptr, rank_lists.ptr, rank_paths.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = exclusiveSum(st, rank_lists.ptr, ix->cluster_read_off.ptr, static_cast<uint64_t>(K) + 1)) return rc;
        if (const int rc = exclusiveSum(st, rank_paths.ptr, ix->cluster_path_off.ptr, static_cast<uint64_t>(K) + 1)) return rc;
        localIndexKernel<<<gridFor(P), block, 0, st>>>(P, pc.path_sorted.ptr, pc.label.ptr, pc.cluster_off.ptr, cluster_rank.ptr,
                                                      ix->cluster_path_off.ptr, local_index.ptr, ix->cluster_paths.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
    } else {
        RPVG_HIP_CHECK(zeroAsync(ix->cluster_read_off.ptr, sizeof(uint64_t), st));
        RPVG_HIP_CHECK(zeroAsync(ix->cluster_path_off.ptr, sizeof(uint64_t), st));
    }

    uint64_t DA = 0, DE = 0, num_small = 0;
    RPVG_HIP_CHECK(ix->read_align_off.alloc(D + 1));
    RPVG_HIP_CHECK(out_ent_off.alloc(D + 1));
    if (D) {
        RPVG_HIP_CHECK(list_rank.alloc(D));
        RPVG_HIP_CHECK(ordered.alloc(D));
        RPVG_HIP_CHECK(ordered_aligns.alloc(D + 1));
        RPVG_HIP_CHECK(ordered_entries.alloc(D + 1));
        RPVG_HIP_CHECK(is_small.alloc(D + 1));
        RPVG_HIP_CHECK(small_pos.alloc(D + 1));
        listRankKernel<<<gridFor(D), block, 0, st>>>(D, list_cluster.ptr, cluster_rank.ptr, list_rank.ptr);
        // stable: the lists of a cluster stay in ascending order of their first occurrence
        if (const int rc = sortPairs(st, list_rank.ptr, ix->read_cluster.ptr, distinct.ptr, ordered.ptr, D, 32)) return rc;
        orderedSizesKernel<<<gridFor(D + 1), block, 0, st>>>(D, ordered.ptr, v.list_align_off, list_ent_off.ptr, ordered_aligns.ptr,
                                                            ordered_entries.ptr, is_small.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
        if (const int rc = exclusiveSum(st, ordered_aligns.ptr, ix->read_align_off.ptr, D + 1)) return rc;
        if (const int rc = exclusiveSum(st, ordered_entries.ptr, out_ent_off.ptr, D + 1)) return rc;
        if (const int rc = exclusiveSum(st, is_small.ptr, small_pos.ptr, D + 1)) return rc;
        uint32_t small32 = 0;
        if (const int rc = fetchOne(st, ix->read_align_off.ptr + D, &DA)) return rc;
        if (const int rc = fetchOne(st, out_ent_off.ptr + D, &DE)) return rc;
        if (const int rc = fetchOne(st, small_pos.ptr + D, &small32)) return rc;
        num_small = small32;
    } else {
        RPVG_HIP_CHECK(zeroAsync(ix->read_align_off.ptr, sizeof(uint64_t), st));
    }

    // ---- gather
    RPVG_HIP_CHECK(ix->read_count.alloc(D));
    RPVG_HIP_CHECK(ix->read_min_mapq.alloc(D));
    RPVG_HIP_CHECK(ix->read_noise_score.alloc(D));
    RPVG_HIP_CHECK(ix->first_occurrence.alloc(D));
    RPVG_HIP_CHECK(ix->out_score_sum.alloc(DA));
    RPVG_HIP_CHECK(ix->out_align_length.alloc(DA));
    RPVG_HIP_CHECK(ix->out_frag_length.alloc(DA));
    RPVG_HIP_CHECK(ix->out_align_path_off.alloc(DA + 1));
    RPVG_HIP_CHECK(ix->align_path_idx.alloc(DE));
    RPVG_HIP_CHECK(ix->small_reads.alloc(num_small));
    RPVG_HIP_CHECK(ix->large_reads.alloc(D - num_small));
    if (D) {
        const OrderedOut out{ix->read_count.ptr, ix->read_min_mapq.ptr, ix->read_noise_score.ptr, ix->first_occurrence.ptr, ix->out_score_sum.ptr,
                             ix->out_align_length.ptr, ix->out_frag_length.ptr, ix->out_align_path_off.ptr, ix->align_path_idx.ptr};
        gatherListsKernel<<<gridFor(D), block, 0, st>>>(D, DA, DE, ordered.ptr, v, multiplicity.ptr, local_index.ptr, ix->read_align_off.ptr,
                                                       out_ent_off.ptr, out);
        splitBySizeKernel<<<gridFor(D), block, 0, st>>>(D, is_small.ptr, small_pos.ptr, ix->small_reads.ptr, ix->large_reads.ptr);
        RPVG_HIP_CHECK(hipGetLastError());
    } else {
        RPVG_HIP_CHECK(zeroAsync(ix->out_align_path_off.ptr, sizeof(uint64_t), st));
    }
    if (P) {
        if (const int rc = copyBuffer(st, ix->path_to_cluster, pc.label, P)) return rc;
    }
    if (const int rc = downloadVector(st, ix->cluster_read_off.ptr, static_cast<size_t>(K) + 1, ix->h_cluster_read_off)) return rc;
    if (const int rc = downloadVector(st, ix->cluster_path_off.ptr, static_cast<size_t>(K) + 1, ix->h_cluster_path_off)) return rc;
    ctx->spanEnd(span);
    RPVG_HIP_CHECK(hipStreamSynchronize(st));

    ix->D = D;
    ix->DA = DA;
    ix->DE = DE;
    ix->K = K;
    ix->num_collided = num_collided;
    ix->num_small = num_small;
    ix->finished = true;
    if (info) {
        info->num_lists = F;
        info->num_distinct = D;
        info->num_clusters = K;
        info->num_collision_lists = num_collided;
    }
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_align_index_frag_counts(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * ix, uint32_t * counts_out) {
    RPVG_REQUIRE(ctx && ix && counts_out, "rpvg_hip_align_index_frag_counts: NULL argument");
    RPVG_REQUIRE(ix->finished, "rpvg_hip_align_index_frag_counts: the index is not finished");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(ix->frag_counts.download(counts_out, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_align_index_view(rpvg_hip_ctx * ctx, rpvg_hip_align_index * ix, rpvg_index_view * view) {
    RPVG_REQUIRE(ctx && ix && view, "rpvg_hip_align_index_view: NULL argument");
    RPVG_REQUIRE(ix->finished, "rpvg_hip_align_index_view: the index is not finished");
    if (!ix->downloaded) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint32_t P = ix->params.num_paths;
        int rc = downloadVector(st, ix->rank_cluster.ptr, ix->K, ix->h_rank_cluster);
        if (!rc) rc = downloadVector(st, ix->path_to_cluster.ptr, P, ix->h_path_to_cluster);
        if (!rc) rc = downloadVector(st, ix->cluster_paths.ptr, P, ix->h_cluster_paths);
        if (!rc) rc = downloadVector(st, ix->read_count.ptr, ix->D, ix->h_read_count);
        if (!rc) rc = downloadVector(st, ix->read_min_mapq.ptr, ix->D, ix->h_read_min_mapq);
        if (!rc) rc = downloadVector(st, ix->read_noise_score.ptr, ix->D, ix->h_read_noise_score);
        if (!rc) rc = downloadVector(st, ix->first_occurrence.ptr, ix->D, ix->h_first_occurrence);
        if (!rc) rc = downloadVector(st, ix->read_align_off.ptr, ix->D + 1, ix->h_read_align_off);
        if (!rc) rc = downloadVector(st, ix->out_score_sum.ptr, ix->DA, ix->h_score_sum);
        if (!rc) rc = downloadVector(st, ix->out_align_length.ptr, ix->DA, ix->h_align_length);
        if (!rc) rc = downloadVector(st, ix->out_frag_length.ptr, ix->DA, ix->h_frag_length);
        if (!rc) rc = downloadVector(st, ix->out_align_path_off.ptr, ix->DA + 1, ix->h_align_path_off);
        if (!rc) rc = downloadVector(st, ix->align_path_idx.ptr, ix->DE, ix->h_align_path_idx);
        if (rc) return rc;
        RPVG_HIP_CHECK(hipStreamSynchronize(st));
        ix->downloaded = true;
    }
    std::memset(view, 0, sizeof(*view));
    view->batch.num_clusters = ix->K;
    view->batch.cluster_read_off = ix->h_cluster_read_off.data();
    view->batch.cluster_path_off = ix->h_cluster_path_off.data();
    view->batch.read_count = ix->h_read_count.data();
    view->batch.read_min_mapq = ix->h_read_min_mapq.data();
    view->batch.read_noise_score = ix->h_read_noise_score.data();
    view->batch.read_align_off = ix->h_read_align_off.data();
    view->batch.align_score_sum = ix->h_score_sum.data();
    view->batch.align_length = ix->h_align_length.data();
    view->batch.align_frag_length = ix->h_frag_length.data();
    view->batch.align_path_off = ix->h_align_path_off.data();
    view->batch.align_path_idx = ix->h_align_path_idx.data();
    view->rank_cluster = ix->h_rank_cluster.data();
    view->path_to_cluster = ix->h_path_to_cluster.data();
    view->cluster_paths = ix->h_cluster_paths.data();
    view->first_occurrence = ix->h_first_occurrence.data();
    return RPVG_HIP_OK;
}

namespace rpvg_hip_detail {
bool alignIndexParts(const rpvg_hip_align_index * ix, AlignIndexParts & parts) {
    if (!ix || !ix->finished) return false;
    parts.num_clusters = ix->K;
    parts.num_paths = ix->params.num_paths;
    parts.cluster_paths = ix->cluster_paths.ptr;
    parts.cluster_path_off = ix->cluster_path_off.ptr;
    parts.h_cluster_path_off = &ix->h_cluster_path_off;
    return true;
}
}  // namespace rpvg_hip_detail

namespace {

// The lists of a finished index as a resident alignment batch; the path arrays are gathered from device arrays by GLOBAL path
// (by_path_count may be NULL).  all_large: every read on the list of readRowKernel (collapsing).  The caller holds ctx->mutex.
int fillAlignments(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * ix, const double * by_path_length, const uint32_t * by_path_count,
                   const bool all_large, rpvg_hip_alignments * al) {
    const uint32_t P = ix->params.num_paths, K = ix->K;
    hipStream_t st = ctx->stream;
    al->num_clusters = K;
    al->num_reads = ix->D;
    al->num_aligns = ix->DA;
    al->num_entries = ix->DE;
    al->num_paths = P;
    al->h_cluster_read_off = ix->h_cluster_read_off;
    al->num_small = all_large ? 0 : ix->num_small;
    al->num_large = ix->D - al->num_small;
    SpanScope span(ctx, FAM_BUILD);
    RPVG_HIP_CHECK(al->eff_len.alloc(P));
    if (P) {
        gatherByPathKernel<double><<<gridFor(P), dim3(256), 0, st>>>(P, ix->cluster_paths.ptr, by_path_length, al->eff_len.ptr);
        if (by_path_count) {
            RPVG_HIP_CHECK(al->source_count.alloc(P));
            gatherByPathKernel<uint32_t><<<gridFor(P), dim3(256), 0, st>>>(P, ix->cluster_paths.ptr, by_path_count, al->source_count.ptr);
        }
        RPVG_HIP_CHECK(hipGetLastError());
    }
    int rc = copyBuffer(st, al->cluster_path_off, ix->cluster_path_off, static_cast<size_t>(K) + 1);
    if (!rc) rc = copyBuffer(st, al->cluster_read_off, ix->cluster_read_off, static_cast<size_t>(K) + 1);
    if (!rc && ix->D) {
        rc = copyBuffer(st, al->read_cluster, ix->read_cluster, ix->D);
        if (!rc) rc = copyBuffer(st, al->read_count, ix->read_count, ix->D);
        if (!rc) rc = copyBuffer(st, al->mapq, ix->read_min_mapq, ix->D);
        if (!rc) rc = copyBuffer(st, al->noise_score, ix->read_noise_score, ix->D);
        if (!rc) rc = copyBuffer(st, al->read_align_off, ix->read_align_off, ix->D + 1);
        if (!rc) rc = copyBuffer(st, al->score, ix->out_score_sum, ix->DA);
        if (!rc) rc = copyBuffer(st, al->align_length, ix->out_align_length, ix->DA);
        if (!rc) rc = copyBuffer(st, al->frag_length, ix->out_frag_length, ix->DA);
        if (!rc) rc = copyBuffer(st, al->align_path_off, ix->out_align_path_off, ix->DA + 1);
        if (!rc) rc = copyBuffer(st, al->path_idx, ix->align_path_idx, ix->DE);
        if (!rc && all_large) {
            RPVG_HIP_CHECK(al->large_reads.alloc(ix->D));
            iotaKernel<<<gridFor(ix->D), dim3(256), 0, st>>>(ix->D, al->large_reads.ptr);
            RPVG_HIP_CHECK(hipGetLastError());
        } else {
            if (!rc && al->num_small) rc = copyBuffer(st, al->small_reads, ix->small_reads, al->num_small);
            if (!rc && al->num_large) rc = copyBuffer(st, al->large_reads, ix->large_reads, al->num_large);
        }
    }
    span.end();
    if (rc) (void) hipDeviceSynchronize();
    return rc;
}

}  // namespace

extern "C" int rpvg_hip_align_index_alignments(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * ix, const double * path_effective_length,
                                               const uint32_t * path_source_count, rpvg_hip_alignments ** out_handle) {
    RPVG_REQUIRE(ctx && ix && out_handle, "rpvg_hip_align_index_alignments: NULL argument");
    *out_handle = nullptr;
    RPVG_REQUIRE(ix->finished, "rpvg_hip_align_index_alignments: the index is not finished");
    const uint32_t P = ix->params.num_paths;
    RPVG_REQUIRE(P == 0 || path_effective_length, "rpvg_hip_align_index_alignments: NULL path_effective_length");
    std::unique_ptr<rpvg_hip_alignments> al(new (std::nothrow) rpvg_hip_alignments());
    if (!al) {
        setError("rpvg_hip_align_index_alignments: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    al->collapse = false;
    al->h_out_path_off = ix->h_cluster_path_off;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<double> by_path_length;
    DeviceBuffer<uint32_t> by_path_count;
    const int span = ctx->spanBegin(FAM_H2D);
    RPVG_HIP_CHECK(by_path_length.upload(path_effective_length, P, st));
    if (path_source_count) RPVG_HIP_CHECK(by_path_count.upload(path_source_count, P, st));
    ctx->spanEnd(span);
    if (const int rc = fillAlignments(ctx, ix, by_path_length.ptr, path_source_count ? by_path_count.ptr : nullptr, false, al.get())) return rc;
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    *out_handle = al.release();
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_align_index_alignments_collapsed(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * ix, const rpvg_hip_path_table * table,
                                                         const rpvg_hip_name_groups * groups, rpvg_hip_alignments ** out_handle) {
    RPVG_REQUIRE(ctx && ix && table && groups && out_handle, "rpvg_hip_align_index_alignments_collapsed: NULL argument");
    *out_handle = nullptr;
    RPVG_REQUIRE(ix->finished, "rpvg_hip_align_index_alignments_collapsed: the index is not finished");
    const uint32_t P = ix->params.num_paths;
    RPVG_REQUIRE(table->num_paths == P && groups->num_paths == P && groups->num_clusters == ix->K,
                 "rpvg_hip_align_index_alignments_collapsed: the table and the groups are not those of the index");
    std::unique_ptr<rpvg_hip_alignments> al(new (std::nothrow) rpvg_hip_alignments());
    if (!al) {
        setError("rpvg_hip_align_index_alignments_collapsed: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    al->collapse = true;
    al->h_out_path_off = groups->h_cluster_group_off;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (const int rc = fillAlignments(ctx, ix, table->effective_length.ptr, table->source_count.ptr, true, al.get())) return rc;
    if (!al->source_count.ptr) RPVG_HIP_CHECK(al->source_count.alloc(P));
    if (const int rc = copyBuffer(st, al->path_group, groups->path_group, P)) return rc;
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    *out_handle = al.release();
    return RPVG_HIP_OK;
}
