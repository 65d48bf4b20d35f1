// estimates_gather.hip — the merged sets the nested calls leave on the device, gathered into the flat estimates of a batch without an
// estimate crossing to the host (interface include/rpvg_table.h: rpvg_estimates_part -> rpvg_estimates_flat with on_device = 1).
//
// Takes over   NestedPathAbundanceEstimator::unpackMergedSolutions / unpackMergedSetSolutions      rpvg_amd/host/path_abundance_estimator.cpp
//              FlatEstimates::add over the containers they fill                                     rpvg_amd/host/estimates_table.hpp
//              (in the reference the containers themselves: src/path_abundance_estimator.cpp:702-749 fills them set by set)
//
// Arithmetic   none: every double is copied.  The only atomics are the integer claim of a cluster by its unit (atomicCAS on an owner
//              word: duplicate detection only, it never decides an order — with a duplicate the call is refused) and the offender word.
// Describe     one wavefront per unit over all parts (the part of a unit from a prefix array of the parts' unit counts): the
//              validations of estimates_gather_plan.hpp in their order, every index checked before it is used; the lanes stride over
//              the unit's subsets and slots, a shuffle reduction gives the unit's member count; the per-cluster set and member counts
//              and the owner are written.
// Offsets      two exclusive sums over the clusters (hipcub): the clusters' first sets and first members.
// Scatter      one wavefront per cluster, 64 sets per step with lane = set: the set's size through an exclusive scan over the
//              wavefront (six __shfl_up steps) plus the running base is its member_off; the lane writes its posterior and its <= 8
//              members and abundances; lane 0 writes set_off, abund_off and noise_count; the wavefront of the last cluster writes
//              the terminal entries of the three offset arrays.
// Every dependency between workgroups is a launch boundary.  One host synchronisation between describe and scatter brings the
// offender word and the totals S and M (the outputs are sized by them): a one-thread kernel puts the two totals next to the word,
// and one copy into page-locked memory fetches the three (fetchDescribedWords, table_kit.hpp).  A part in host memory travels with the other small arrays in
// one upload; its descriptor holds offsets into that block (WirePart), a device part's holds addresses.

#include <deque>

#include "device_algos.hpp"
#include "estimates_gather_plan.hpp"
#include "subset_result.hpp"
#include "table_kit.hpp"
#include "../../include/rpvg_table.h"

using namespace rpvg_hip_detail;
using namespace rpvg_gather;

// the flat estimates of a batch: one device block (DownloadPack) and, after rpvg_hip_flat_estimates_get, its page-locked copy
struct rpvg_hip_flat_estimates {
    uint32_t num_clusters = 0;
    uint64_t num_sets = 0, num_members = 0, num_paths = 0;
    const rpvg_hip_batch * batch = nullptr;  // cluster_path_off is the batch's own array
    DownloadPack pack;
    DeviceBuffer<uint64_t> set_off, member_off, abund_off;  // [K+1] [S+1] [K+1]
    DeviceBuffer<uint32_t> members;                         // [M]
    DeviceBuffer<double> posteriors, abundances, noise_count;  // [S] [M] [K]
    DeviceBuffer<double> eff;                               // [P] uploaded, or the caller's device array (borrowed)
    std::vector<double> h_eff;
    bool eff_on_host = false, downloaded = false;
};

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;

// A part's descriptor on the device: addresses, or — relative != 0, a part that came from host memory — offsets into the upload block.
struct WirePart {
    uint32_t num_units, width;
    uint64_t num_subsets, num_slots, relative;
    uint64_t subset_off, path_off, set_count, cluster_noise_count, set_posterior, set_first, set_second, set_size, set_member, set_abundance;
};

struct GatherArgs {
    uint32_t K, num_parts;
    uint64_t num_units;
    const WirePart * parts;           // [num_parts]
    const unsigned char * base;       // of the upload block
    const uint64_t * unit_prefix;     // [num_parts + 1] units before every part
    const uint32_t * unit_cluster;    // [num_units] the parts' back to back
    const uint64_t * cluster_path_off;  // [K+1] the batch's
    const double * cluster_total;     // [K]
    uint32_t * owner;                 // [K] 1 + the unit (over all parts) that claimed the cluster; 0: none
    uint64_t * cluster_sets;          // [K+1] the last one stays 0: the sums run over K + 1 entries and end with the totals
    uint64_t * cluster_members;       // [K+1]
    word64 * bad;                     // words[0] of the three the host fetches: the offender, then S and M (gatherTotalsKernel)
    const uint64_t * set_base;        // [K+1] exclusive sums of the two
    const uint64_t * member_base;     // [K+1]
    uint64_t S, M;
    uint64_t * set_off, * member_off, * abund_off;
    uint32_t * members;
    double * posteriors, * abundances, * noise_count;
};

template <typename T>
__device__ __forceinline__ const T * wirePointer(const WirePart & w, const unsigned char * base, const uint64_t value) {
    return w.relative ? reinterpret_cast<const T *>(base + value) : reinterpret_cast<const T *>(static_cast<uintptr_t>(value));
}

__device__ __forceinline__ Part partOf(const WirePart & w, const unsigned char * base) {
    Part p;
    p.num_units = w.num_units;
    p.width = w.width;
    p.num_subsets = w.num_subsets;
    p.num_slots = w.num_slots;
    p.subset_off = wirePointer<uint64_t>(w, base, w.subset_off);
    p.path_off = wirePointer<uint64_t>(w, base, w.path_off);
    p.set_count = wirePointer<uint32_t>(w, base, w.set_count);
    p.cluster_noise_count = wirePointer<double>(w, base, w.cluster_noise_count);
    p.set_posterior = wirePointer<double>(w, base, w.set_posterior);
    p.set_first = wirePointer<uint32_t>(w, base, w.set_first);
    p.set_second = wirePointer<uint32_t>(w, base, w.set_second);
    p.set_size = wirePointer<uint32_t>(w, base, w.set_size);
    p.set_member = wirePointer<uint32_t>(w, base, w.set_member);
    p.set_abundance = wirePointer<double>(w, base, w.set_abundance);
    return p;
}

// the wavefront's index in the grid, uniform
__device__ __forceinline__ uint64_t waveIndex() {
    return blockIdx.x * static_cast<uint64_t>(kWaves) + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
}

// One wavefront per unit.  Nothing it reads is trusted: the kernel is the validation.
__global__ __launch_bounds__(kBlock) void gatherDescribeKernel(const GatherArgs a) {
    const uint64_t g = waveIndex();
    const uint32_t lane = threadIdx.x & 63;
    if (g >= a.num_units) return;
    const uint32_t p = static_cast<uint32_t>(lastAtMost(a.unit_prefix, a.num_parts, g));
    const uint64_t before = a.unit_prefix[p];
    if (g < before || g - before >= a.parts[p].num_units) return;  // (the prefix is the host's own: cannot happen)
    const uint32_t u = static_cast<uint32_t>(g - before);
    const Part part = partOf(a.parts[p], a.base);
    const uint32_t c = a.unit_cluster[g];
    if (c >= a.K) {
        if (lane == 0) reportOffender(a.bad, g, kBadUnitCluster);
        return;
    }
    uint32_t claimed = 0;
    if (lane == 0) claimed = atomicCAS(&a.owner[c], 0u, static_cast<uint32_t>(g) + 1u);
    claimed = __shfl(claimed, 0, 64);
    if (claimed != 0) {
        // Every unit that shares its cluster offends; whichever of them won the claim, the smallest is named by a loser (itself, or
        // the one that lost to it).
        if (lane == 0) reportOffender(a.bad, claimed - 1u < g ? claimed - 1u : g, kBadDuplicate);
        return;
    }
    uint64_t s0 = 0, s1 = 0;
    if (unitSubsetsBad(part, u, &s0, &s1)) {
        if (lane == 0) reportOffender(a.bad, g, kBadSubsetOff);
        return;
    }
    bool paths_bad = false;
    for (uint64_t s = s0 + lane; s < s1; s += 64) paths_bad |= subsetPathsBad(part, s);
    if (__any(paths_bad)) {
        if (lane == 0) reportOffender(a.bad, g, kBadPathOff);
        return;
    }
    uint64_t first = 0, slots = 0;
    unitSlots(part, s0, s1, &first, &slots);
    const uint64_t count = part.set_count[u];
    if (count > slots) {
        if (lane == 0) reportOffender(a.bad, g, kBadSetCount);
        return;
    }
    const uint64_t num_paths = a.cluster_path_off[c + 1] - a.cluster_path_off[c];
    unsigned long long my_members = 0;
    bool size_bad = false, member_bad = false;
    for (uint64_t q = lane; q < count; q += 64) {
        uint32_t n = 0;
        const int why = slotOffence(part, first + q, num_paths, &n);
        size_bad |= why == kBadSetSize;
        member_bad |= why == kBadMember;
        my_members += n;
    }
    const bool any_size_bad = __any(size_bad), any_member_bad = __any(member_bad);  // (votes of the whole wavefront: outside the lane-0 branch)
    if (any_size_bad || any_member_bad) {
        if (lane == 0) reportOffender(a.bad, g, any_size_bad ? kBadSetSize : kBadMember);
        return;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) my_members += __shfl_down(my_members, d, 64);
    if (lane == 0) {
        a.cluster_sets[c] = count;
        a.cluster_members[c] = my_members;
    }
}

// The two totals next to the offender word, so that one copy brings all three to the host.
__global__ __launch_bounds__(64) void gatherTotalsKernel(const GatherArgs a) {
    if (threadIdx.x == 0) {
        a.bad[1] = a.set_base[a.K];
        a.bad[2] = a.member_base[a.K];
    }
}

// One wavefront per cluster of the batch.  (The guards against S and M hold whatever the parts hold by now: a part in device
// memory is the caller's and could have changed behind the describe pass.)
__global__ __launch_bounds__(kBlock) void gatherScatterKernel(const GatherArgs a) {
    const uint64_t k = waveIndex();
    const uint32_t lane = threadIdx.x & 63;
    if (k >= a.K) return;
    const uint32_t owner = a.owner[k];
    const uint64_t base_set = a.set_base[k], base_member = a.member_base[k];
    const double total = a.cluster_total[k];
    if (lane == 0) {
        a.set_off[k] = base_set;
        a.abund_off[k] = base_member;
        if (k + 1 == a.K) {  // the terminal entries, once
            a.set_off[a.K] = a.S;
            a.abund_off[a.K] = a.M;
            a.member_off[a.S] = a.M;
        }
    }
    if (owner == 0 || owner - 1u >= a.num_units) {  // a cluster in no unit: no sets, its read count as noise
        if (lane == 0) a.noise_count[k] = total;
        return;
    }
    const uint64_t g = owner - 1u;
    const uint32_t p = static_cast<uint32_t>(lastAtMost(a.unit_prefix, a.num_parts, g));
    const uint32_t u = static_cast<uint32_t>(g - a.unit_prefix[p]);
    const Part part = partOf(a.parts[p], a.base);
    if (lane == 0) a.noise_count[k] = unitNoise(part, u, total);
    const uint64_t first = part.path_off[part.subset_off[u]], count = part.set_count[u];
    uint64_t run = 0;  // members of the cluster's sets before this step
    for (uint64_t q0 = 0; q0 < count; q0 += 64) {
        const uint64_t q = q0 + lane, slot = first + q;
        const bool active = q < count;
        const uint32_t n = active ? min(slotSize(part, slot), maxSetSize(part.width)) : 0u;
        uint32_t inclusive = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inclusive, d, 64);
            if (lane >= static_cast<uint32_t>(d)) inclusive += up;
        }
        const uint32_t step_members = __shfl(inclusive, 63, 64);
        const uint64_t s = base_set + q, m = base_member + run + (inclusive - n);
        if (active && s < a.S && m + n <= a.M) {
            a.member_off[s] = m;
            a.posteriors[s] = part.set_posterior[slot];
#pragma unroll
            for (uint32_t j = 0; j < kMaxWidth; ++j) {
                if (j < n) {
                    a.members[m + j] = slotMember(part, slot, j);
                    a.abundances[m + j] = slotAbundance(part, slot, j);
                }
            }
        }
        run += step_members;
    }
}

uint64_t addressOf(const void * pointer) { return static_cast<uint64_t>(reinterpret_cast<uintptr_t>(pointer)); }

}  // namespace

extern "C" {

int rpvg_hip_subset_em_part(const rpvg_hip_subset_em * result, rpvg_estimates_part * part_out) {
    RPVG_REQUIRE(result && part_out, "rpvg_hip_subset_em_part: NULL argument");
    std::memset(part_out, 0, sizeof(*part_out));
    if (!result->kept.ptr) {
        setError("rpvg_hip_subset_em_part: not taken (the call did not keep its device block: rpvg_hip_subset_em_keep_device was off, or the call had no "
                 "matrix)");
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    if (!result->kept_merged) {
        setError("rpvg_hip_subset_em_part: not taken (the call did no merge on the device: the batch was uploaded without path_group_id)");
        return RPVG_HIP_ERR_UNSUPPORTED;
    }
    const rpvg_subset_full::PackedLayout & lay = result->kept_layout;
    const unsigned char * base = result->kept.ptr;
    part_out->num_units = result->view.num_matrices;
    part_out->num_subsets = result->num_subsets;
    part_out->num_slots = result->kept_slots;
    part_out->width = result->kept_width;
    part_out->subset_off = reinterpret_cast<const uint64_t *>(base + lay.subset_off);
    part_out->path_off = reinterpret_cast<const uint64_t *>(base + lay.path_off);
    part_out->set_count = reinterpret_cast<const uint32_t *>(base + lay.set_count);
    part_out->cluster_noise_count = reinterpret_cast<const double *>(base + lay.cluster_noise);
    part_out->set_posterior = reinterpret_cast<const double *>(base + lay.set_posterior);
    part_out->set_abundance = reinterpret_cast<const double *>(base + lay.set_abund);
    if (result->kept_width == 0) {
        part_out->set_first = reinterpret_cast<const uint32_t *>(base + lay.set_first);
        part_out->set_second = reinterpret_cast<const uint32_t *>(base + lay.set_second);
    } else {
        part_out->set_size = reinterpret_cast<const uint32_t *>(base + lay.set_size);
        part_out->set_member = reinterpret_cast<const uint32_t *>(base + lay.set_member);
    }
    part_out->on_device = 1;
    return RPVG_HIP_OK;
}

uint64_t rpvg_hip_subset_em_kept_bytes(const rpvg_hip_subset_em * result) { return result ? result->kept.count : 0; }

int rpvg_hip_flat_estimates_gather(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_estimates_part * parts, uint32_t num_parts,
                                   const double * path_effective_length, int32_t eff_on_device, rpvg_hip_flat_estimates ** estimates_out) {
    RPVG_REQUIRE(ctx && batch && estimates_out && (num_parts == 0 || parts), "rpvg_hip_flat_estimates_gather: NULL argument");
    *estimates_out = nullptr;
    const uint32_t K = batch->num_clusters;
    const uint64_t P = batch->num_paths;
    RPVG_REQUIRE(!batch->upload, "rpvg_hip_flat_estimates_gather: the batch's upload is not finished");
    RPVG_REQUIRE(batch->h_cluster_total.size() == K,
                 "rpvg_hip_flat_estimates_gather: the batch has no cluster totals (rpvg_hip_read_rows_to_batch without paths): a cluster without sets "
                 "has its read count as noise");
    RPVG_REQUIRE(K <= kMaxItems && P <= kMaxItems, "rpvg_hip_flat_estimates_gather: %u clusters, %llu paths exceed one table", K,
                 static_cast<unsigned long long>(P));
    RPVG_REQUIRE(P == 0 || path_effective_length, "rpvg_hip_flat_estimates_gather: path_effective_length is NULL");
    uint64_t num_units = 0;
    std::vector<uint64_t> unit_prefix(static_cast<size_t>(num_parts) + 1, 0);
    for (uint32_t p = 0; p < num_parts; ++p) {
        const rpvg_estimates_part & part = parts[p];
        RPVG_REQUIRE(part.width <= kMaxWidth, "rpvg_hip_flat_estimates_gather: part %u: a width of %u (at most %u)", p, part.width, kMaxWidth);
        RPVG_REQUIRE(part.num_subsets <= kMaxItems && part.num_slots <= kMaxItems && part.num_units <= kMaxItems,
                     "rpvg_hip_flat_estimates_gather: part %u: its sizes exceed one table", p);
        const bool sets_ok = part.width == 0 ? (part.set_first && part.set_second) : (part.set_size && part.set_member);
        RPVG_REQUIRE(part.num_units == 0 || (part.unit_cluster && part.subset_off && part.path_off && part.set_count && part.cluster_noise_count),
                     "rpvg_hip_flat_estimates_gather: part %u: NULL array", p);
        RPVG_REQUIRE(part.num_units == 0 || part.num_slots == 0 || (part.set_posterior && part.set_abundance && sets_ok),
                     "rpvg_hip_flat_estimates_gather: part %u: NULL array", p);
        num_units += part.num_units;
        unit_prefix[p + 1] = num_units;
    }
    RPVG_REQUIRE(num_units <= kMaxItems, "rpvg_hip_flat_estimates_gather: %llu units exceed one table", static_cast<unsigned long long>(num_units));
    std::unique_ptr<rpvg_hip_flat_estimates> est(new (std::nothrow) rpvg_hip_flat_estimates());
    if (!est) {
        setError("rpvg_hip_flat_estimates_gather: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    est->num_clusters = K;
    est->num_paths = P;
    est->batch = batch;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // the small host arrays, and the parts that are host memory, in one upload
    UploadPack inputs;
    std::deque<DeviceBuffer<unsigned char>> host_pieces;  // (views of the block: the pack binds them)
    auto addBytes = [&](const void * from, const size_t bytes) {
        const uint64_t offset = inputs.copied_bytes;
        host_pieces.emplace_back();
        inputs.add(host_pieces.back(), static_cast<const unsigned char *>(from), from ? bytes : 0);
        return offset;
    };
    std::vector<uint32_t> unit_cluster(num_units);
    std::vector<WirePart> wire(num_parts);
    for (uint32_t p = 0; p < num_parts; ++p) {
        const rpvg_estimates_part & part = parts[p];
        if (part.num_units) std::memcpy(unit_cluster.data() + unit_prefix[p], part.unit_cluster, sizeof(uint32_t) * part.num_units);
        WirePart & w = wire[p];
        std::memset(&w, 0, sizeof(w));
        w.num_units = part.num_units;
        w.width = part.width;
        w.num_subsets = part.num_subsets;
        w.num_slots = part.num_slots;
        if (part.num_units == 0) continue;
        const uint64_t U = part.num_units, S = part.num_subsets, L = part.num_slots, cells = cellsPerSlot(part.width);
        if (part.on_device) {
            w.subset_off = addressOf(part.subset_off);
            w.path_off = addressOf(part.path_off);
            w.set_count = addressOf(part.set_count);
            w.cluster_noise_count = addressOf(part.cluster_noise_count);
            w.set_posterior = addressOf(part.set_posterior);
            w.set_first = addressOf(part.set_first);
            w.set_second = addressOf(part.set_second);
            w.set_size = addressOf(part.set_size);
            w.set_member = addressOf(part.set_member);
            w.set_abundance = addressOf(part.set_abundance);
        } else {
            w.relative = 1;
            w.subset_off = addBytes(part.subset_off, (U + 1) * 8);
            w.path_off = addBytes(part.path_off, (S + 1) * 8);
            w.set_count = addBytes(part.set_count, U * 4);
            w.cluster_noise_count = addBytes(part.cluster_noise_count, U * 8);
            w.set_posterior = addBytes(part.set_posterior, L * 8);
            if (part.width == 0) {
                w.set_first = addBytes(part.set_first, L * 4);
                w.set_second = addBytes(part.set_second, L * 4);
            } else {
                w.set_size = addBytes(part.set_size, L * 4);
                w.set_member = addBytes(part.set_member, L * 4 * cells);
            }
            w.set_abundance = addBytes(part.set_abundance, L * 8 * cells);
        }
    }
    DeviceBuffer<unsigned char> d_wire;
    DeviceBuffer<uint64_t> d_unit_prefix, d_cluster_sets, d_cluster_members;
    DeviceBuffer<uint32_t> d_unit_cluster, d_owner;
    DeviceBuffer<double> d_cluster_total;
    DeviceBuffer<word64> d_words;  // the offender word, S, M
    const word64 initial_words[3] = {kNoBad, 0, 0};
    inputs.add(d_wire, reinterpret_cast<const unsigned char *>(wire.data()), wire.size() * sizeof(WirePart));
    inputs.add(d_unit_prefix, unit_prefix.data(), unit_prefix.size());
    inputs.add(d_unit_cluster, unit_cluster.data(), unit_cluster.size());
    inputs.add(d_cluster_total, batch->h_cluster_total.data(), K);
    inputs.add(d_words, initial_words, 3);
    inputs.addZero(d_owner, K);
    inputs.addZero(d_cluster_sets, static_cast<size_t>(K) + 1);
    inputs.addZero(d_cluster_members, static_cast<size_t>(K) + 1);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
        if (eff_on_device) {
            takeInput(inputs, est->eff, {path_effective_length, true}, P);
        } else {
            RPVG_HIP_CHECK(est->eff.upload(path_effective_length, P, st));
            est->h_eff.assign(path_effective_length, path_effective_length + P);
            est->eff_on_host = true;
        }
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes) + (eff_on_device ? 0.0 : 8.0 * static_cast<double>(P));

    DeviceBuffer<uint64_t> d_set_base, d_member_base;
    RPVG_HIP_CHECK(d_set_base.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(d_member_base.alloc(static_cast<size_t>(K) + 1));

    GatherArgs a;
    std::memset(&a, 0, sizeof(a));
    a.K = K;
    a.num_parts = num_parts;
    a.num_units = num_units;
    a.parts = reinterpret_cast<const WirePart *>(d_wire.ptr);
    a.base = inputs.block.ptr;
    a.unit_prefix = d_unit_prefix.ptr;
    a.unit_cluster = d_unit_cluster.ptr;
    a.cluster_path_off = batch->cluster_path_off.ptr;
    a.cluster_total = d_cluster_total.ptr;
    a.owner = d_owner.ptr;
    a.cluster_sets = d_cluster_sets.ptr;
    a.cluster_members = d_cluster_members.ptr;
    a.bad = d_words.ptr;
    a.set_base = d_set_base.ptr;
    a.member_base = d_member_base.ptr;

    SpanScope span(ctx, FAM_BUILD);
    word64 words[3] = {kNoBad, 0, 0};
    DeviceBuffer<uint8_t> scan_tmp;
    if (num_units) {  // (without clusters too: every unit_cluster offends)
        gatherDescribeKernel<<<gridFor(num_units, kWaves), dim3(kBlock), 0, st>>>(a);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
    }
    if (K > 0) {
        // (both sums on the stream behind one another: one block of temporary storage serves both)
        const int n = static_cast<int>(K) + 1;
        size_t tmp_bytes = 0;
        RPVG_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_cluster_sets.ptr, d_set_base.ptr, n, st));
        RPVG_HIP_CHECK(scan_tmp.alloc(tmp_bytes ? tmp_bytes : 1));
        RPVG_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scan_tmp.ptr, tmp_bytes, d_cluster_sets.ptr, d_set_base.ptr, n, st));
        RPVG_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scan_tmp.ptr, tmp_bytes, d_cluster_members.ptr, d_member_base.ptr, n, st));
        gatherTotalsKernel<<<dim3(1), dim3(64), 0, st>>>(a);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 3;
    }
    if (K > 0 || num_units) {
        if (const int rc = fetchDescribedWords(st, d_words.ptr, words, 3)) return rc;  // one copy, the one wait: the offender word and S, M
    }
    const word64 bad = words[0];
    if (bad != kNoBad) {
        span.end();
        const Offender o = offenderOf(bad, kBadMember);
        const uint32_t p = static_cast<uint32_t>(lastAtMost(unit_prefix.data(), num_parts, o.index));
        setError("rpvg_hip_flat_estimates_gather: part %u, unit %llu: %s", p, static_cast<unsigned long long>(o.index - unit_prefix[p]), reasonOf(o.why));
        return RPVG_HIP_ERR_INVALID;
    }
    const uint64_t S = words[1], M = words[2];
    if (S > kMaxSets || M > kMaxItems) {
        span.end();
        setError("rpvg_hip_flat_estimates_gather: %llu sets, %llu members exceed one table", static_cast<unsigned long long>(S),
                 static_cast<unsigned long long>(M));
        return RPVG_HIP_ERR_INVALID;
    }
    est->num_sets = S;
    est->num_members = M;
    est->pack.add(est->set_off, static_cast<uint64_t *>(nullptr), static_cast<size_t>(K) + 1);
    est->pack.add(est->member_off, static_cast<uint64_t *>(nullptr), S + 1);
    est->pack.add(est->members, static_cast<uint32_t *>(nullptr), M);
    est->pack.add(est->posteriors, static_cast<double *>(nullptr), S);
    est->pack.add(est->abund_off, static_cast<uint64_t *>(nullptr), static_cast<size_t>(K) + 1);
    est->pack.add(est->abundances, static_cast<double *>(nullptr), M);
    est->pack.add(est->noise_count, static_cast<double *>(nullptr), K);
    RPVG_HIP_CHECK(est->pack.alloc());
    if (K == 0) {
        RPVG_HIP_CHECK(zeroAsync(est->pack.block.ptr, est->pack.total, st));  // the three offset arrays of an empty batch: {0}
    } else {
        a.S = S;
        a.M = M;
        a.set_off = est->set_off.ptr;
        a.member_off = est->member_off.ptr;
        a.abund_off = est->abund_off.ptr;
        a.members = est->members.ptr;
        a.posteriors = est->posteriors.ptr;
        a.abundances = est->abundances.ptr;
        a.noise_count = est->noise_count.ptr;
        gatherScatterKernel<<<gridFor(K, kWaves), dim3(kBlock), 0, st>>>(a);
        RPVG_HIP_CHECK(hipGetLastError());
        ctx->stats.build_launches += 1;
    }
    span.end();
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the inputs and the scratch go back to the pool
    *estimates_out = est.release();
    return RPVG_HIP_OK;
}

int rpvg_hip_flat_estimates_view(const rpvg_hip_flat_estimates * estimates, rpvg_estimates_flat * view_out) {
    RPVG_REQUIRE(estimates && view_out, "rpvg_hip_flat_estimates_view: NULL argument");
    std::memset(view_out, 0, sizeof(*view_out));
    view_out->num_clusters = estimates->num_clusters;
    view_out->num_sets = estimates->num_sets;
    view_out->num_members = estimates->num_members;
    view_out->num_abundances = estimates->num_members;
    view_out->num_paths = estimates->num_paths;
    view_out->set_off = estimates->set_off.ptr;
    view_out->member_off = estimates->member_off.ptr;
    view_out->members = estimates->members.ptr;
    view_out->posteriors = estimates->posteriors.ptr;
    view_out->abund_off = estimates->abund_off.ptr;
    view_out->abundances = estimates->abundances.ptr;
    view_out->noise_count = estimates->noise_count.ptr;
    view_out->cluster_path_off = estimates->batch->cluster_path_off.ptr;
    view_out->path_effective_length = estimates->eff.ptr;
    view_out->on_device = 1;
    return RPVG_HIP_OK;
}

int rpvg_hip_flat_estimates_get(rpvg_hip_ctx * ctx, rpvg_hip_flat_estimates * estimates, rpvg_estimates_flat * host_out) {
    RPVG_REQUIRE(ctx && estimates && host_out, "rpvg_hip_flat_estimates_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!estimates->downloaded) {
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        RPVG_HIP_CHECK(estimates->pack.fetch(ctx->stream));
        if (!estimates->eff_on_host) {
            if (const int rc = downloadVector(ctx->stream, estimates->eff.ptr, estimates->num_paths, estimates->h_eff)) return rc;
        }
        RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        estimates->eff_on_host = true;
        estimates->downloaded = true;
    }
    const DownloadPack & pack = estimates->pack;
    const unsigned char * host = static_cast<const unsigned char *>(pack.pinned ? pack.pinned : pack.pageable.data());
    std::memset(host_out, 0, sizeof(*host_out));
    host_out->num_clusters = estimates->num_clusters;
    host_out->num_sets = estimates->num_sets;
    host_out->num_members = estimates->num_members;
    host_out->num_abundances = estimates->num_members;
    host_out->num_paths = estimates->num_paths;
    host_out->set_off = reinterpret_cast<const uint64_t *>(host + pack.pieces[0].offset);
    host_out->member_off = reinterpret_cast<const uint64_t *>(host + pack.pieces[1].offset);
    host_out->members = reinterpret_cast<const uint32_t *>(host + pack.pieces[2].offset);
    host_out->posteriors = reinterpret_cast<const double *>(host + pack.pieces[3].offset);
    host_out->abund_off = reinterpret_cast<const uint64_t *>(host + pack.pieces[4].offset);
    host_out->abundances = reinterpret_cast<const double *>(host + pack.pieces[5].offset);
    host_out->noise_count = reinterpret_cast<const double *>(host + pack.pieces[6].offset);
    host_out->cluster_path_off = estimates->batch->h_cluster_path_off.data();
    host_out->path_effective_length = estimates->h_eff.data();
    host_out->on_device = 0;
    return RPVG_HIP_OK;
}

void rpvg_hip_flat_estimates_free(rpvg_hip_ctx * ctx, rpvg_hip_flat_estimates * estimates) {
    if (!estimates) return;
    waitAndDelete(ctx);
    delete estimates;
}

}  // extern "C"
