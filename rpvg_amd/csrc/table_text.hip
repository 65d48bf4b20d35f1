// table_text.hip — the rows of a result file as text, formatted on the GPU from a resident table: the Gibbs samples file and the two
// per-path estimates files (interface include/rpvg_text.h).  One shape of row (TextRows, table_text_plan.hpp): the three files are
// three descriptors over the same kernels.
//
// Takes over   the rows of ReadCountGibbsSamplesWriter                                src/threaded_output_writer.cpp:160-201
//              the rows of AbundanceEstimatesWriter                                   src/threaded_output_writer.cpp:295-322
//              the rows of HaplotypeAbundanceEstimatesWriter                          src/threaded_output_writer.cpp:358-411
//              each double at setprecision(8), "%.8g"                                  src/threaded_output_writer.cpp:6
//
// Values       A cell is the text glibc's printf("%.*g") gives, byte for byte, for every bit pattern (number_text.hpp: the value times a
//              128-bit power of ten, the rounding decided by an exact multiword comparison inside the product's error band around one
//              half).  There is no floating-point arithmetic in this file.
// Describe     one kernel behind the copy validates name_off (the smallest offending path comes back, the host words the message) and,
//              for the per-path abundance rows, that set i of every cluster is {i} with one abundance each (the first offending cluster).
//              Nothing below runs on a refused input.
// Measure      the bytes of every row, 0 for a row the filter drops: a wavefront per row with the lanes along the cells for rows of more
//              than kNarrowCells cells (a wave reduction), a lane per row otherwise.  Lengths and offsets are 64-bit.
// Scan         hipcub's exclusive sum over the P lengths and a trailing 0: row_off [P+1].
// Write        a wavefront (a workgroup of its own) per row.  Per step of 64 cells every lane decomposes its cell once, takes its length,
//              a wave prefix sum places the cells, and the lanes store their text into the wavefront's staging block in LDS.  The block
//              is laid out at the row's alignment in the text (byte i of the block is byte base + i, base a multiple of 4), so it
//              leaves as aligned 4-byte stores, consecutive lanes on consecutive words; the bytes of a word the step has not finished
//              stay in the block for the next step, and only the ragged first and last word of a ROW are stored byte by byte
//              (flushPlan): every byte of [row_off[r], row_off[r+1]) is stored exactly once and no other byte is touched.  The name is
//              the first steps (a piece of kMaxCellBytes bytes per lane), the integer columns the first cells.
//              The write pass formats again instead of reading lengths the measure pass would have kept (a byte per cell).
// The text lies between two guards of 64 pattern bytes (rpvg_hip_table_text_guards).
// The handle, the guards, the staging block's flush and the wave sum are in table_text_device.hpp, shared with set_text.hip (the rows
// whose unit is a path group set), whose texts _view, _get, _guards and _free below serve as they serve the ones built here.

#include <mutex>

#include "device_algos.hpp"
#include "table_kit.hpp"
#include "table_residents.hpp"
#include "table_text_device.hpp"
#include "table_text_plan.hpp"
#include "../../include/rpvg_text.h"

using namespace rpvg_hip_detail;
using namespace rpvg_table_text;

namespace {

// bad = min over the offending paths and clusters (table_kit.hpp: a cluster is the second kind, so a path comes before every cluster)
enum TextBad { kBadNameOff = 1, kBadPathOff = 2, kBadSetOff = 3, kBadAbundOff = 4, kBadSetCount = 5, kBadNotSingleton = 6 };

const char * const kReasons[] = {"",
                                 "name_off is not a non-decreasing sequence of offsets from 0 to num_name_bytes",
                                 "cluster_path_off is not a non-decreasing sequence of offsets from 0 to num_paths",
                                 "set_off is not a non-decreasing sequence of offsets from 0 to num_sets",
                                 "abund_off is not a non-decreasing sequence of offsets from 0 to num_abundances",
                                 "not one set and one abundance per path",
                                 "set i is not {i} for every path i"};

// what the describe kernel checks beside the descriptor
struct DescribeArgs {
    uint64_t num_name_bytes;
    bool check_path_off;       // cluster_path_off came with the call (the estimates files)
    bool singletons;           // RPVG_TEXT_PER_PATH
    uint64_t S, M, A;
    const uint64_t * set_off;    // [K+1]
    const uint64_t * member_off; // [S+1]
    const uint32_t * members;    // [M]
    const uint64_t * abund_off;  // [K+1]
    uint64_t * member_base;      // [K] member_off[set_off[k]]
    word64 * bad;
};

// thread i: path i and cluster i.  Every index is checked before it is used.
__global__ __launch_bounds__(kBlock) void describeKernel(const TextRows t, const DescribeArgs a) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i < t.num_rows && offsetsBad(t.name_off, i, t.num_rows, a.num_name_bytes)) reportOffender(a.bad, i, kBadNameOff);
    if (i < t.num_clusters && (a.check_path_off || a.singletons)) {
        const uint64_t k = i;
        if (offsetsBad(t.cluster_path_off, k, t.num_clusters, t.num_rows)) reportOffender(a.bad, k, kBadPathOff, true);
        else if (a.singletons) {
            const uint64_t paths = t.cluster_path_off[k + 1] - t.cluster_path_off[k];
            if (offsetsBad(a.set_off, k, t.num_clusters, a.S)) reportOffender(a.bad, k, kBadSetOff, true);
            else if (offsetsBad(a.abund_off, k, t.num_clusters, a.A)) reportOffender(a.bad, k, kBadAbundOff, true);
            else if (a.set_off[k + 1] - a.set_off[k] != paths || a.abund_off[k + 1] - a.abund_off[k] != paths) reportOffender(a.bad, k, kBadSetCount, true);
            else a.member_base[k] = a.member_off[a.set_off[k]];
        }
    }
    if (i < t.num_rows && a.singletons) {
        const uint64_t k = lastAtMost(t.cluster_path_off, t.num_clusters, i);
        const uint64_t p0 = t.cluster_path_off[k], p1 = t.cluster_path_off[k + 1], s0 = a.set_off[k];
        if (p0 <= i && i < p1 && p1 <= t.num_rows && s0 <= a.S && i - p0 < a.S - s0) {  // (the cluster's thread reports anything else)
            const uint64_t set = s0 + (i - p0), first = s0 < a.S ? a.member_off[s0] : 0;
            const uint64_t m0 = a.member_off[set], m1 = a.member_off[set + 1];
            if (m1 != m0 + 1 || m0 >= a.M || m0 - first != i - p0 || a.members[m0] != i - p0) reportOffender(a.bad, k, kBadNotSingleton, true);
        }
    }
}

// row_len [P+1]: the bytes of every row and a trailing 0
template <bool kWavefront>
__global__ __launch_bounds__(kBlock) void measureKernel(const TextRows t, uint64_t * __restrict__ row_len, word64 * exact_cells) {
    const uint64_t thread = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    if (thread == 0) row_len[t.num_rows] = 0;
    uint64_t exact = 0;
    if (kWavefront) {
        const uint64_t r = thread >> 6;
        if (r < t.num_rows) {  // (uniform)
            uint64_t bytes = 0;
            if (printed(t, r)) {
                const uint64_t k = clusterOf(t, r), cells = numCells(t);
                for (uint64_t c = lane; c < cells; c += 64) {
                    const Cell cell = cellOf(t, r, k, c);
                    bytes += cellText<false>(cell, t.precision, nullptr);
                    exact += cell.decimal.exact ? 1u : 0u;
                }
                bytes = waveSum(bytes) + nameBytes(t, r);
            }
            if (lane == 0) row_len[r] = bytes;
        }
    } else if (thread < t.num_rows) {
        row_len[thread] = rowBytes(t, thread, &exact);
    }
    exact = waveSum(exact);
    if (lane == 0 && exact) atomicAdd(exact_cells, static_cast<word64>(exact));
}

// a workgroup of one wavefront per row (the rows in a grid-stride loop)
__global__ __launch_bounds__(64) void writeKernel(const TextRows t, const uint64_t * __restrict__ row_off, char * text) {
    __shared__ __attribute__((aligned(16))) char stage[(kStageBytes + 15) & ~15];
    const uint32_t lane = threadIdx.x;
    for (uint64_t r = blockIdx.x; r < t.num_rows; r += gridDim.x) {
        const uint64_t begin = row_off[r], end = row_off[r + 1];
        if (begin >= end) continue;  // (uniform)
        const uint64_t k = clusterOf(t, r), cells = numCells(t), name = nameBytes(t, r), name_at = t.name_off[r];
        uint64_t base = begin & ~3ull;
        uint32_t lo = static_cast<uint32_t>(begin & 3u), hi = lo;
        constexpr uint64_t kPiece = static_cast<uint64_t>(kStepCells) * kMaxCellBytes;
        for (uint64_t done = 0; done < name; done += kPiece) {
            const uint32_t piece = static_cast<uint32_t>(name - done < kPiece ? name - done : kPiece);
            for (uint32_t i = lane; i < piece; i += 64) stage[hi + i] = t.name_bytes[name_at + done + i];
            hi += piece;
            flush(stage, text, base, lo, hi, false, lane);
        }
        for (uint64_t c0 = 0; c0 < cells; c0 += kStepCells) {
            const uint64_t c = c0 + lane;
            Cell cell = {};
            uint32_t bytes = 0;
            if (c < cells) {
                cell = cellOf(t, r, k, c);
                bytes = cellText<false>(cell, t.precision, nullptr);
            }
            uint32_t behind = bytes;  // inclusive prefix sum along the wavefront
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t other = __shfl_up(behind, d, 64);
                if (static_cast<int>(lane) >= d) behind += other;
            }
            const uint32_t total = __shfl(behind, 63, 64);
            if (c < cells) cellText<true>(cell, t.precision, stage + hi + (behind - bytes));
            hi += total;
            flush(stage, text, base, lo, hi, c0 + kStepCells >= cells, lane);
        }
    }
}

// what an entry point hands over: the descriptor with the table's device pointers in place, the labels and what came with the call
struct TextInputs {
    TextRows rows = {};                      // the pointers of the resident table filled in, the others NULL
    const rpvg_table_labels * labels = nullptr;
    Source<uint64_t> cluster_path_off;       // [K+1]
    bool check_path_off = false;
    bool singletons = false;
    uint64_t S = 0, M = 0, A = 0;
    Source<uint64_t> set_off, member_off, abund_off;
    Source<uint32_t> members;
    Source<double> effective_length, abundances;  // fixed column 0; PER_PATH: column 1 by abund_off
    const double * member_tpm = nullptr;          // PER_PATH: column 2 by member_base
};

int buildText(rpvg_hip_ctx * ctx, TextInputs & in, const char * who, rpvg_hip_table_text ** text_out) {
    const rpvg_table_labels & labels = *in.labels;
    TextRows & t = in.rows;
    const uint64_t P = t.num_rows;
    const uint32_t K = t.num_clusters;
    if (const char * wrong = descriptorBad(t)) {
        setError("%s: %s (precision %d)", who, wrong, t.precision);
        return RPVG_HIP_ERR_INVALID;
    }
    RPVG_REQUIRE(labels.num_paths == P && labels.num_clusters == K, "%s: labels of %llu paths in %u clusters, the table has %llu in %u", who,
                 static_cast<unsigned long long>(labels.num_paths), labels.num_clusters, static_cast<unsigned long long>(P), K);
    RPVG_REQUIRE(P < 0x7fffffffull, "%s: %llu paths exceed one text", who, static_cast<unsigned long long>(P));
    RPVG_REQUIRE(P == 0 || (labels.name_off && labels.cluster_id && (labels.num_name_bytes == 0 || labels.name_bytes)), "%s: NULL label array", who);
    std::unique_ptr<rpvg_hip_table_text> text(new (std::nothrow) rpvg_hip_table_text());
    if (!text) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    text->ctx = ctx;
    text->num_paths = P;
    text->h_row_off.assign(static_cast<size_t>(P) + 1, 0);
    if (P == 0) {
        *text_out = text.release();
        return RPVG_HIP_OK;
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    const bool labels_on_device = labels.on_device != 0;
    UploadPack inputs;
    DeviceBuffer<uint64_t> name_off, cluster_path_off, set_off, member_off, abund_off, member_base, pow10, row_len, row_off;
    DeviceBuffer<char> name_bytes;
    DeviceBuffer<uint32_t> path_length, cluster_id, members;
    DeviceBuffer<double> effective_length, abundances;
    DeviceBuffer<word64> d_bad, d_exact;
    takeInput(inputs, name_off, Source<uint64_t>{labels.name_off, labels_on_device}, static_cast<size_t>(P) + 1);
    takeInput(inputs, name_bytes, Source<char>{labels.name_bytes, labels_on_device}, labels.num_name_bytes);
    takeInput(inputs, cluster_id, Source<uint32_t>{labels.cluster_id, labels_on_device}, K);
    if (labels.path_length) takeInput(inputs, path_length, Source<uint32_t>{labels.path_length, labels_on_device}, P);
    takeInput(inputs, cluster_path_off, in.cluster_path_off, static_cast<size_t>(K) + 1);
    if (in.effective_length.from) takeInput(inputs, effective_length, in.effective_length, P);
    if (in.singletons) {
        takeInput(inputs, set_off, in.set_off, static_cast<size_t>(K) + 1);
        takeInput(inputs, member_off, in.member_off, static_cast<size_t>(in.S) + 1);
        takeInput(inputs, members, in.members, in.M);
        takeInput(inputs, abund_off, in.abund_off, static_cast<size_t>(K) + 1);
        takeInput(inputs, abundances, in.abundances, in.A);
    }
    inputs.add(pow10, pow10Table(), rpvg_number_text::kPow10Words);
    inputs.add(d_bad, &kNoBad, 1);
    inputs.addZero(d_exact, 1);
    inputs.addZero(member_base, in.singletons ? K : 0);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    RPVG_HIP_CHECK(row_len.alloc(static_cast<size_t>(P) + 1));
    RPVG_HIP_CHECK(row_off.alloc(static_cast<size_t>(P) + 1));

    t.name_off = name_off.ptr;
    t.name_bytes = name_bytes.ptr;
    t.cluster_path_off = cluster_path_off.ptr;
    t.cluster_id = cluster_id.ptr;
    t.second_u32 = labels.path_length ? path_length.ptr : nullptr;
    t.pow10 = pow10.ptr;
    if (in.effective_length.from) t.fixed[0] = DoubleColumn{effective_length.ptr, nullptr};
    if (in.singletons) {
        t.fixed[1] = DoubleColumn{abundances.ptr, abund_off.ptr};
        t.fixed[2] = DoubleColumn{in.member_tpm, member_base.ptr};
    }
    DescribeArgs d = {};
    d.num_name_bytes = labels.num_name_bytes;
    d.check_path_off = in.check_path_off;
    d.singletons = in.singletons;
    d.S = in.S;
    d.M = in.M;
    d.A = in.A;
    d.set_off = set_off.ptr;
    d.member_off = member_off.ptr;
    d.members = members.ptr;
    d.abund_off = abund_off.ptr;
    d.member_base = member_base.ptr;
    d.bad = d_bad.ptr;

    SpanScope span(ctx, FAM_BUILD);
    describeKernel<<<gridFor(std::max<uint64_t>(P, K)), dim3(kBlock), 0, st>>>(t, d);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    word64 bad = kNoBad;
    if (const int rc = fetchDescribed(st, d_bad.ptr, &bad)) return rc;
    if (bad != kNoBad) {
        span.end();
        const Offender o = offenderOf(bad, kBadNotSingleton);
        setError("%s: %s %llu: %s", who, o.second_kind ? "cluster" : "path", static_cast<unsigned long long>(o.index), kReasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    if (measuredByWavefront(t)) measureKernel<true><<<gridFor(P, kBlock / 64), dim3(kBlock), 0, st>>>(t, row_len.ptr, d_exact.ptr);
    else measureKernel<false><<<gridFor(P), dim3(kBlock), 0, st>>>(t, row_len.ptr, d_exact.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    if (const int rc = exclusiveSum(st, row_len.ptr, row_off.ptr, P + 1)) return rc;
    word64 exact = 0;
    RPVG_HIP_CHECK(hipMemcpyAsync(text->h_row_off.data(), row_off.ptr, (static_cast<size_t>(P) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&exact, d_exact.ptr, sizeof(exact), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    ctx->stats.text_exact_cells += exact;
    text->num_bytes = text->h_row_off[P];
    for (uint64_t r = 0; r < P; ++r) text->num_rows += text->h_row_off[r + 1] > text->h_row_off[r] ? 1 : 0;
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
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(P, kMaxWriteBlocks));
        writeKernel<<<dim3(blocks), dim3(64), 0, st>>>(t, row_off.ptr, text->text());
        ctx->stats.build_launches += 1;
    }
    RPVG_HIP_CHECK(hipGetLastError());
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the inputs of this call go back to the pool
    span.end();
    *text_out = text.release();
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" {

int rpvg_hip_gibbs_table_text(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_table * table, const rpvg_table_labels * labels, int32_t precision,
                              rpvg_hip_table_text ** text_out) {
    const char * const who = "rpvg_hip_gibbs_table_text";
    RPVG_REQUIRE(ctx && table && labels && text_out, "%s: NULL argument", who);
    *text_out = nullptr;
    const GibbsTableResident resident = residentOf(table);
    TextInputs in;
    in.labels = labels;
    in.rows.num_rows = resident.num_paths;
    in.rows.num_clusters = resident.num_clusters;
    in.rows.run_length = resident.num_gibbs_samples;
    in.rows.run = resident.samples;
    in.rows.run_stride = resident.num_gibbs_samples;
    in.rows.filter = resident.listed;
    in.rows.precision = precision;
    in.cluster_path_off = {resident.host_cluster_path_off, false};  // (validated when the table was built)
    rpvg_table_labels without_lengths = *labels;                    // the Gibbs rows have no Length column
    without_lengths.path_length = nullptr;
    in.labels = &without_lengths;
    return buildText(ctx, in, who, text_out);
}

int rpvg_hip_estimates_table_text(rpvg_hip_ctx * ctx, const rpvg_hip_estimates_table * table, const rpvg_estimates_flat * estimates,
                                  const rpvg_table_labels * labels, int32_t kind, int32_t precision, rpvg_hip_table_text ** text_out) {
    const char * const who = "rpvg_hip_estimates_table_text";
    RPVG_REQUIRE(ctx && table && estimates && labels && text_out, "%s: NULL argument", who);
    *text_out = nullptr;
    RPVG_REQUIRE(kind == RPVG_TEXT_PER_PATH || kind == RPVG_TEXT_HAPLOTYPE, "%s: no such kind of rows: %d", who, kind);
    const EstimatesTableResident resident = residentOf(table);
    RPVG_REQUIRE(estimates->num_clusters == resident.num_clusters && estimates->num_paths == resident.num_paths && estimates->num_members == resident.num_members,
                 "%s: the table is not that of the estimates", who);
    RPVG_REQUIRE(resident.has_tpm, "%s: the table has no TPMs yet (rpvg_hip_estimates_table_tpm)", who);
    RPVG_REQUIRE(resident.num_paths == 0 || labels->path_length, "%s: the labels have no path_length", who);
    RPVG_REQUIRE(resident.num_clusters == 0 || (estimates->cluster_path_off && (resident.num_paths == 0 || estimates->path_effective_length)), "%s: NULL array", who);
    const bool on_device = estimates->on_device != 0;
    TextInputs in;
    in.labels = labels;
    in.rows.num_rows = resident.num_paths;
    in.rows.num_clusters = resident.num_clusters;
    in.rows.precision = precision;
    in.cluster_path_off = {estimates->cluster_path_off, on_device};
    in.check_path_off = true;
    in.effective_length = {estimates->path_effective_length, on_device};
    if (kind == RPVG_TEXT_PER_PATH) {
        RPVG_REQUIRE(resident.num_clusters == 0 || (estimates->set_off && estimates->member_off && estimates->abund_off), "%s: NULL array", who);
        RPVG_REQUIRE((estimates->num_members == 0 || estimates->members) && (estimates->num_abundances == 0 || estimates->abundances), "%s: NULL array", who);
        in.rows.num_fixed = 3;
        in.singletons = true;
        in.S = estimates->num_sets;
        in.M = estimates->num_members;
        in.A = estimates->num_abundances;
        in.set_off = {estimates->set_off, on_device};
        in.member_off = {estimates->member_off, on_device};
        in.members = {estimates->members, on_device};
        in.abund_off = {estimates->abund_off, on_device};
        in.abundances = {estimates->abundances, on_device};
        in.member_tpm = resident.member_tpm;
    } else {
        in.rows.num_fixed = 4;
        in.rows.fixed[1] = DoubleColumn{resident.haplotype_prob, nullptr};
        in.rows.fixed[2] = DoubleColumn{resident.read_count, nullptr};
        in.rows.fixed[3] = DoubleColumn{resident.tpm, nullptr};
    }
    return buildText(ctx, in, who, text_out);
}

int rpvg_hip_table_text_view(rpvg_hip_table_text * text, rpvg_table_text_view * view_out) {
    RPVG_REQUIRE(text && view_out, "rpvg_hip_table_text_view: NULL argument");
    rpvg_hip_ctx * ctx = text->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!text->pinned && text->num_bytes) {
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        if (pinnedAlloc(&text->pinned, text->num_bytes) != hipSuccess) {
            text->pinned = nullptr;
            (void) hipGetLastError();
            setError("rpvg_hip_table_text_view: no page-locked memory for %llu bytes (rpvg_hip_table_text_get takes a range)", static_cast<unsigned long long>(text->num_bytes));
            return RPVG_HIP_ERR_ALLOC;
        }
        RPVG_HIP_CHECK(hipMemcpyAsync(text->pinned, text->text(), text->num_bytes, hipMemcpyDeviceToHost, ctx->stream));
        RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    view_out->num_paths = text->num_paths;
    view_out->num_rows = text->num_rows;
    view_out->num_bytes = text->num_bytes;
    view_out->row_off = text->h_row_off.data();
    view_out->bytes = static_cast<const char *>(text->pinned);
    return RPVG_HIP_OK;
}

int rpvg_hip_table_text_sizes(rpvg_hip_table_text * text, rpvg_table_text_view * view_out) {
    RPVG_REQUIRE(text && view_out, "rpvg_hip_table_text_sizes: NULL argument");
    std::lock_guard<std::mutex> lock(text->ctx->mutex);
    view_out->num_paths = text->num_paths;
    view_out->num_rows = text->num_rows;
    view_out->num_bytes = text->num_bytes;
    view_out->row_off = text->h_row_off.data();
    view_out->bytes = static_cast<const char *>(text->pinned);  // NULL until rpvg_hip_table_text_view has copied the text
    return RPVG_HIP_OK;
}

int rpvg_hip_table_text_get(rpvg_hip_table_text * text, uint64_t byte_begin, uint64_t byte_end, char * dst) {
    RPVG_REQUIRE(text, "rpvg_hip_table_text_get: NULL argument");
    RPVG_REQUIRE(byte_begin <= byte_end && byte_end <= text->num_bytes, "rpvg_hip_table_text_get: bytes %llu to %llu of %llu", static_cast<unsigned long long>(byte_begin),
                 static_cast<unsigned long long>(byte_end), static_cast<unsigned long long>(text->num_bytes));
    if (byte_begin == byte_end) return RPVG_HIP_OK;
    RPVG_REQUIRE(dst, "rpvg_hip_table_text_get: NULL argument");
    rpvg_hip_ctx * ctx = text->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipMemcpyAsync(dst, text->text() + byte_begin, byte_end - byte_begin, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

int rpvg_hip_table_text_guards(rpvg_hip_table_text * text, int32_t * intact_out) {
    RPVG_REQUIRE(text && intact_out, "rpvg_hip_table_text_guards: NULL argument");
    *intact_out = 1;
    if (!text->block.ptr) return RPVG_HIP_OK;  // a text without paths has no block
    rpvg_hip_ctx * ctx = text->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned char guards[2 * kGuardBytes];
    RPVG_HIP_CHECK(hipMemcpyAsync(guards, text->block.ptr, kGuardBytes, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipMemcpyAsync(guards + kGuardBytes, text->block.ptr + kGuardBytes + text->num_bytes, kGuardBytes, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (const unsigned char byte : guards) {
        if (byte != kGuardPattern) *intact_out = 0;
    }
    return RPVG_HIP_OK;
}

void rpvg_hip_table_text_free(rpvg_hip_table_text * text) {
    if (!text) return;
    waitAndDelete(text->ctx);
    delete text;
}

}  // extern "C"
