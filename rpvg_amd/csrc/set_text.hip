// set_text.hip — the rows of the two result files whose row is a path group SET, formatted on the GPU from the resident estimates table
// (interface include/rpvg_text.h): the second shape of row (SetRows, set_text_plan.hpp) beside that of table_text.hip, whose kernels
// and instantiations this file leaves as they are.  The handle, the guards, the staging block's flush and the scan are shared
// (table_text_device.hpp); _view, _get, _guards and _free of table_text.hip serve a set text unchanged.
//
// Takes over   the rows of JointHaplotypeAbundanceEstimatesWriter (RPVG_TEXT_JOINT)     src/threaded_output_writer.cpp:434-546
//              the rows of JointHaplotypeEstimatesWriter (RPVG_TEXT_POSTERIOR)          src/threaded_output_writer.cpp:233-280
//
// Values       as in table_text.hip: a cell is glibc's "%.*g", byte for byte.  The abundance and the TPM of a member are read, not
//              recomputed: there is no floating-point arithmetic in this file; the filter !(posterior < min_posterior) is a comparison.
// Describe     one kernel behind the copy: thread i checks path i (name_off), cluster i (cluster_path_off, set_off and, for the joint
//              kind, abund_off and one abundance per member) and set i (member_off, a size in 1 .. ploidy, every member a path of the
//              cluster).  The smallest offending path, else the smallest offending cluster, comes back (table_kit.hpp).  Nothing below
//              runs on a refused input.
// Measure      the bytes of every set, 0 for a set the filter drops: a lane per set (a row has at most 8 names and 18 number cells);
//              the cluster of a set by lastAtMost over set_off.  Lengths and offsets are 64-bit.
// Scan         hipcub's exclusive sum over the S lengths and a trailing 0: row_off [S+1].
// Write        a wavefront (a workgroup of its own) per set, the sets in a grid-stride loop.  The up to `ploidy` name slots join the
//              wavefront's staging block in LDS one behind the other, consecutive lanes on consecutive bytes, and the block leaves
//              whenever it is full: a long name is as many steps as it needs.  The number cells are one step: a lane decomposes its
//              cell once, takes its length, a wave prefix sum places the cells and the lanes store their text.  The block leaves as
//              aligned 4-byte words, only the ragged first and last word of a ROW byte by byte (flushPlan): every byte of
//              [row_off[s], row_off[s+1]) is stored exactly once and no other byte is touched.  A row of short names is ONE flush.
// The text lies between two guards of 64 pattern bytes (rpvg_hip_table_text_guards).

#include <mutex>

#include "device_algos.hpp"
#include "set_text_plan.hpp"
#include "table_kit.hpp"
#include "table_residents.hpp"
#include "table_text_device.hpp"
#include "../../include/rpvg_text.h"

using namespace rpvg_hip_detail;
using rpvg_table_text::Cell;
using rpvg_table_text::cellText;
using rpvg_table_text::kStageBytes;
namespace sp = rpvg_set_text;

namespace {

enum SetBad { kSetBadNameOff = 1, kSetBadPathOff = 2, kSetBadSetOff = 3, kSetBadMemberOff = 4, kSetBadSize = 5, kSetBadMember = 6, kSetBadAbundOff = 7, kSetBadAbundCount = 8 };

const char * const kSetReasons[] = {"",
                                    "name_off is not a non-decreasing sequence of offsets from 0 to num_name_bytes",
                                    "cluster_path_off is not a non-decreasing sequence of offsets from 0 to num_paths",
                                    "set_off is not a non-decreasing sequence of offsets from 0 to num_sets",
                                    "member_off of one of its sets is not a non-decreasing sequence of offsets from 0 to num_members",
                                    "a set whose size is not in 1 .. ploidy",
                                    "a set member that is not a path of the cluster",
                                    "abund_off is not a non-decreasing sequence of offsets from 0 to num_abundances",
                                    "not one abundance per set member"};

struct DescribeSetsArgs {
    uint64_t num_paths, num_name_bytes, M, A;
    word64 * bad;
};

// thread i: path i, cluster i and set i.  Every index is checked before it is used; an offence of a set is its cluster's.
__global__ __launch_bounds__(kBlock) void describeSetsKernel(const sp::SetRows t, const DescribeSetsArgs a) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    const uint64_t K = t.num_clusters, S = t.num_sets;
    if (i < a.num_paths && offsetsBad(t.name_off, i, a.num_paths, a.num_name_bytes)) reportOffender(a.bad, i, kSetBadNameOff);
    if (i < K) {
        if (offsetsBad(t.cluster_path_off, i, K, a.num_paths)) reportOffender(a.bad, i, kSetBadPathOff, true);
        if (offsetsBad(t.set_off, i, K, S)) reportOffender(a.bad, i, kSetBadSetOff, true);
        else if (t.joint) {
            if (offsetsBad(t.abund_off, i, K, a.A)) reportOffender(a.bad, i, kSetBadAbundOff, true);
            else if (t.abund_off[i + 1] - t.abund_off[i] != t.member_off[t.set_off[i + 1]] - t.member_off[t.set_off[i]]) reportOffender(a.bad, i, kSetBadAbundCount, true);
        }
    }
    if (i < S) {
        const uint64_t k = lastAtMost(t.set_off, K, i);
        const uint64_t s0 = t.set_off[k], s1 = t.set_off[k + 1];
        if (s0 <= i && i < s1 && s1 <= S) {  // (the cluster's thread reports anything else)
            if (offsetsBad(t.member_off, i, S, a.M)) reportOffender(a.bad, k, kSetBadMemberOff, true);
            else {
                const uint64_t m0 = t.member_off[i], size = t.member_off[i + 1] - m0;
                if (size < 1 || size > t.ploidy) reportOffender(a.bad, k, kSetBadSize, true);
                else if (!offsetsBad(t.cluster_path_off, k, K, a.num_paths)) {
                    const uint64_t paths = t.cluster_path_off[k + 1] - t.cluster_path_off[k];
                    for (uint64_t m = m0; m < m0 + size; ++m) {
                        if (t.members[m] >= paths) reportOffender(a.bad, k, kSetBadMember, true);
                    }
                }
            }
        }
    }
}

// row_len [S+1]: the bytes of every set (a lane each: a row has at most 8 names and 18 number cells) and a trailing 0
__global__ __launch_bounds__(kBlock) void measureSetsKernel(const sp::SetRows t, uint64_t * __restrict__ row_len, word64 * exact_cells) {
    const uint64_t thread = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (thread == 0) row_len[t.num_sets] = 0;
    uint64_t exact = 0;
    if (thread < t.num_sets) row_len[thread] = sp::rowBytes(t, thread, &exact);
    exact = waveSum(exact);
    if ((threadIdx.x & 63) == 0 && exact) atomicAdd(exact_cells, static_cast<word64>(exact));
}

// a workgroup of one wavefront per set (the sets in a grid-stride loop).  The name slots join the staging block one behind the other,
// the block leaving whenever it is full; the number cells are one step, a cell per lane, placed by a wave prefix sum.
__global__ __launch_bounds__(64) void writeSetsKernel(const sp::SetRows t, const uint64_t * __restrict__ row_off, char * text) {
    __shared__ __attribute__((aligned(16))) char stage[(kStageBytes + 15) & ~15];
    const uint32_t lane = threadIdx.x;
    const uint32_t cells = sp::numberCells(t);
    for (uint64_t s = blockIdx.x; s < t.num_sets; s += gridDim.x) {
        const uint64_t begin = row_off[s], end = row_off[s + 1];
        if (begin >= end) continue;  // (uniform)
        const sp::SetRow row = sp::setRow(t, s);
        uint64_t base = begin & ~3ull;
        uint32_t lo = static_cast<uint32_t>(begin & 3u), hi = lo;
        for (uint32_t j = 0; j < t.ploidy; ++j) {
            const sp::NameSlot slot = sp::nameSlot(t, row, j);
            const uint64_t bytes = sp::slotBytes(slot);
            uint64_t done = 0;
            while (done < bytes) {
                const uint32_t piece = sp::pieceOf(bytes - done, hi);
                if (piece == 0) {  // the block is full
                    flush(stage, text, base, lo, hi, false, lane);
                    continue;
                }
                for (uint32_t i = lane; i < piece; i += 64) stage[hi + i] = sp::slotByte(t, slot, done + i);
                hi += piece;
                done += piece;
            }
        }
        if (sp::numbersNeedFlush(t, hi)) flush(stage, text, base, lo, hi, false, lane);
        Cell cell = {};
        uint32_t bytes = 0;
        if (lane < cells) {
            cell = sp::cellOf(t, row, lane);
            bytes = cellText<false>(cell, t.precision, nullptr);
        }
        uint32_t behind = bytes;  // inclusive prefix sum along the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t other = __shfl_up(behind, d, 64);
            if (static_cast<int>(lane) >= d) behind += other;
        }
        const uint32_t total = __shfl(behind, 63, 64);
        if (lane < cells) cellText<true>(cell, t.precision, stage + hi + (behind - bytes));
        hi += total;
        flush(stage, text, base, lo, hi, true, lane);
    }
}

}  // namespace

extern "C" {

int rpvg_hip_estimates_set_text(rpvg_hip_ctx * ctx, const rpvg_hip_estimates_table * table, const rpvg_estimates_flat * estimates,
                                const rpvg_table_labels * labels, int32_t kind, uint32_t ploidy, double min_posterior, int32_t precision,
                                rpvg_hip_table_text ** text_out) {
    const char * const who = "rpvg_hip_estimates_set_text";
    RPVG_REQUIRE(ctx && table && estimates && labels && text_out, "%s: NULL argument", who);
    *text_out = nullptr;
    RPVG_REQUIRE(kind == RPVG_TEXT_JOINT || kind == RPVG_TEXT_POSTERIOR, "%s: no such kind of rows: %d", who, kind);
    const EstimatesTableResident resident = residentOf(table);
    const bool joint = kind == RPVG_TEXT_JOINT;
    const uint32_t K = resident.num_clusters;
    const uint64_t P = resident.num_paths, S = estimates->num_sets, M = estimates->num_members, A = estimates->num_abundances;
    sp::SetRows t = {};
    t.num_sets = S;
    t.num_clusters = K;
    t.ploidy = ploidy;
    t.joint = joint;
    t.min_posterior = min_posterior;
    t.precision = precision;
    if (const char * wrong = sp::descriptorBad(t)) {
        setError("%s: %s (precision %d, ploidy %u)", who, wrong, precision, ploidy);
        return RPVG_HIP_ERR_INVALID;
    }
    RPVG_REQUIRE(estimates->num_clusters == K && estimates->num_paths == P && M == resident.num_members, "%s: the table is not that of the estimates", who);
    RPVG_REQUIRE(!joint || resident.has_tpm, "%s: the table has no TPMs yet (rpvg_hip_estimates_table_tpm)", who);
    RPVG_REQUIRE(!joint || resident.ploidy == ploidy, "%s: the table was built for ploidy %u, the text is asked for ploidy %u", who, resident.ploidy, ploidy);
    RPVG_REQUIRE(labels->num_paths == P && labels->num_clusters == K, "%s: labels of %llu paths in %u clusters, the table has %llu in %u", who,
                 static_cast<unsigned long long>(labels->num_paths), labels->num_clusters, static_cast<unsigned long long>(P), K);
    RPVG_REQUIRE(S < 0x7fffffffull && M < 0x7fffffffull, "%s: %llu sets of %llu members exceed one text", who, static_cast<unsigned long long>(S), static_cast<unsigned long long>(M));
    RPVG_REQUIRE(K == 0 || (labels->cluster_id && estimates->cluster_path_off && estimates->set_off), "%s: NULL array", who);
    RPVG_REQUIRE(P == 0 || (labels->name_off && (labels->num_name_bytes == 0 || labels->name_bytes)), "%s: NULL label array", who);
    RPVG_REQUIRE(S == 0 || (estimates->member_off && estimates->members && estimates->posteriors), "%s: NULL array", who);
    RPVG_REQUIRE(!joint || S == 0 || (estimates->abund_off && (A == 0 || estimates->abundances)), "%s: NULL array", who);
    std::unique_ptr<rpvg_hip_table_text> text(new (std::nothrow) rpvg_hip_table_text());
    if (!text) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    text->ctx = ctx;
    text->num_paths = S;  // the rows of a set text are the sets
    text->h_row_off.assign(static_cast<size_t>(S) + 1, 0);
    if (S == 0) {
        *text_out = text.release();
        return RPVG_HIP_OK;
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    const bool labels_on_device = labels->on_device != 0, on_device = estimates->on_device != 0;
    UploadPack inputs;
    DeviceBuffer<uint64_t> name_off, cluster_path_off, set_off, member_off, abund_off, pow10, row_len, row_off;
    DeviceBuffer<char> name_bytes;
    DeviceBuffer<uint32_t> cluster_id, members;
    DeviceBuffer<double> posteriors, abundances;
    DeviceBuffer<word64> d_bad, d_exact;
    takeInput(inputs, name_off, Source<uint64_t>{labels->name_off, labels_on_device}, static_cast<size_t>(P) + 1);
    takeInput(inputs, name_bytes, Source<char>{labels->name_bytes, labels_on_device}, labels->num_name_bytes);
    takeInput(inputs, cluster_id, Source<uint32_t>{labels->cluster_id, labels_on_device}, K);
    takeInput(inputs, cluster_path_off, Source<uint64_t>{estimates->cluster_path_off, on_device}, static_cast<size_t>(K) + 1);
    takeInput(inputs, set_off, Source<uint64_t>{estimates->set_off, on_device}, static_cast<size_t>(K) + 1);
    takeInput(inputs, member_off, Source<uint64_t>{estimates->member_off, on_device}, static_cast<size_t>(S) + 1);
    takeInput(inputs, members, Source<uint32_t>{estimates->members, on_device}, M);
    takeInput(inputs, posteriors, Source<double>{estimates->posteriors, on_device}, S);
    if (joint) {
        takeInput(inputs, abund_off, Source<uint64_t>{estimates->abund_off, on_device}, static_cast<size_t>(K) + 1);
        takeInput(inputs, abundances, Source<double>{estimates->abundances, on_device}, A);
    }
    inputs.add(pow10, pow10Table(), rpvg_number_text::kPow10Words);
    inputs.add(d_bad, &kNoBad, 1);
    inputs.addZero(d_exact, 1);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    RPVG_HIP_CHECK(row_len.alloc(static_cast<size_t>(S) + 1));
    RPVG_HIP_CHECK(row_off.alloc(static_cast<size_t>(S) + 1));

    t.name_off = name_off.ptr;
    t.name_bytes = name_bytes.ptr;
    t.cluster_path_off = cluster_path_off.ptr;
    t.cluster_id = cluster_id.ptr;
    t.set_off = set_off.ptr;
    t.member_off = member_off.ptr;
    t.members = members.ptr;
    t.posteriors = posteriors.ptr;
    t.abund_off = joint ? abund_off.ptr : nullptr;
    t.abundances = joint ? abundances.ptr : nullptr;
    t.member_tpm = joint ? resident.member_tpm : nullptr;
    t.pow10 = pow10.ptr;
    DescribeSetsArgs d = {};
    d.num_paths = P;
    d.num_name_bytes = labels->num_name_bytes;
    d.M = M;
    d.A = A;
    d.bad = d_bad.ptr;

    SpanScope span(ctx, FAM_BUILD);
    describeSetsKernel<<<gridFor(std::max<uint64_t>(std::max<uint64_t>(P, K), S)), dim3(kBlock), 0, st>>>(t, d);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    word64 bad = kNoBad;
    if (const int rc = fetchDescribed(st, d_bad.ptr, &bad)) return rc;
    if (bad != kNoBad) {
        span.end();
        const Offender o = offenderOf(bad, kSetBadAbundCount);
        setError("%s: %s %llu: %s", who, o.second_kind ? "cluster" : "path", static_cast<unsigned long long>(o.index), kSetReasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    measureSetsKernel<<<gridFor(S), dim3(kBlock), 0, st>>>(t, row_len.ptr, d_exact.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    if (const int rc = exclusiveSum(st, row_len.ptr, row_off.ptr, S + 1)) return rc;
    word64 exact = 0;
    RPVG_HIP_CHECK(hipMemcpyAsync(text->h_row_off.data(), row_off.ptr, (static_cast<size_t>(S) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&exact, d_exact.ptr, sizeof(exact), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    ctx->stats.text_exact_cells += exact;
    text->num_bytes = text->h_row_off[S];
    for (uint64_t s = 0; s < S; ++s) text->num_rows += text->h_row_off[s + 1] > text->h_row_off[s] ? 1 : 0;
    const size_t block_bytes = (static_cast<size_t>(text->num_bytes) + 2 * kGuardBytes + 3) & ~size_t(3);
    if (text->block.alloc(block_bytes) != hipSuccess) {
        (void) hipGetLastError();
        (void) hipDeviceSynchronize();
        span.end();
        setError("%s: no device memory for a text of %llu bytes", who, static_cast<unsigned long long>(text->num_bytes));
        return RPVG_HIP_ERR_ALLOC;
    }
    guardKernel<<<dim3(1), dim3(128), 0, st>>>(text->block.ptr, text->num_bytes);
    ctx->stats.build_launches += 1;
    if (text->num_bytes) {
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(S, kMaxWriteBlocks));
        writeSetsKernel<<<dim3(blocks), dim3(64), 0, st>>>(t, row_off.ptr, text->text());
        ctx->stats.build_launches += 1;
    }
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the inputs of this call go back to the pool
    span.end();
    *text_out = text.release();
    return RPVG_HIP_OK;
}

}  // extern "C"
