// rows_text.hip — the --write-probs dump formatted on the GPU from rows in the grouped layout of rpvg_cluster_batch, resident
// (rpvg_hip_read_rows) or given as arrays (interface include/rpvg_text.h): the third shape of row (DumpRows, rows_text_plan.hpp)
// beside those of table_text.hip and set_text.hip, whose kernels this file leaves as they are (a file of its own: set_text.hip
// records what one translation unit did to measureKernel's registers).  The handle, the guards, the staging block's flush and the
// wave sum are shared (table_text_device.hpp); _view, _get, _guards and _free of table_text.hip serve a rows text unchanged.
//
// Takes over   ProbabilityClusterWriter::addCluster          src/threaded_output_writer.cpp:40-95
//              (this project's copy: writeProbabilityClusters, rpvg_amd/host/io/cluster_io.cpp)
//
// Values       every double is glibc's "%.*g", byte for byte; there is no floating-point arithmetic and no filter in this file.
// Describe     one kernel behind the copy: thread i checks position i of cluster_row_off, cluster_path_off, row_grp_off, grp_idx_off
//              and name_off (offsetsBad) and, as row i, that every path_idx of the row is below the path count of the row's cluster.
//              The smallest offending offset position, else the smallest offending row, comes back (table_kit.hpp).  Nothing below
//              runs on a refused input.
// Index        rowCell [R + 1] and clusterCell [K + 1], the closed forms of the plan header, stored once for the bisections.
// Measure      a wavefront per 64 consecutive CELLS of the file (blockWalk): cell_len [C + 1], 64-bit, before the scan.
// Scan         hipcub's exclusive sum over the C cell lengths and a trailing 0: cell_off [C + 1]; the offset of a line is that of
//              its first cell (a gather of L + 1 entries: row_off).
// Write        a wavefront (a workgroup of its own) per 64 consecutive cells, the blocks in a grid-stride loop: the bytes of the 64
//              cells are one contiguous range of the file wherever the line ends fall.  Bounded cells are a lane each (a row of five
//              cells is five lanes, not a wavefront; a row of a thousand indices sixteen wavefronts), a name is all lanes along its
//              bytes.  The cells join the wavefront's staging block in LDS at their offsets, and the block leaves when it is full and
//              at the end of the 64 cells, as aligned 4-byte words, only the ragged first and last word byte by byte (flushPlan):
//              every byte of the text is stored exactly once and no other byte is touched.
// The text lies between two guards of 64 pattern bytes (rpvg_hip_table_text_guards).

#include <mutex>

#include "device_algos.hpp"
#include "rows_residents.hpp"
#include "rows_text_plan.hpp"
#include "table_kit.hpp"
#include "table_text_device.hpp"
#include "../../include/rpvg_text.h"

using namespace rpvg_hip_detail;
using rpvg_table_text::kStageBytes;
namespace rp = rpvg_rows_text;

namespace {

enum RowsBad { kRowsBadRowOff = 1, kRowsBadPathOff = 2, kRowsBadGrpOff = 3, kRowsBadIdxOff = 4, kRowsBadNameOff = 5, kRowsBadIndex = 6 };

const char * const kRowsReasons[] = {"",
                                     "cluster_row_off is not a non-decreasing sequence of offsets from 0 to num_rows",
                                     "cluster_path_off is not a non-decreasing sequence of offsets from 0 to num_paths",
                                     "row_grp_off is not a non-decreasing sequence of offsets from 0 to num_groups",
                                     "grp_idx_off is not a non-decreasing sequence of offsets from 0 to num_entries",
                                     "name_off is not a non-decreasing sequence of offsets from 0 to num_name_bytes",
                                     "a path_idx that is not below the path count of the row's cluster"};

// thread i: position i of the five offset arrays and row i.  Every index is checked before it is used.
__global__ __launch_bounds__(kBlock) void describeRowsKernel(const rp::DumpRows t, const uint64_t num_name_bytes, word64 * bad) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    const uint64_t K = t.num_clusters, R = t.num_rows, G = t.num_groups, M = t.num_entries, P = t.num_paths;
    if (i < K && offsetsBad(t.cluster_row_off, i, K, R)) reportOffender(bad, i, kRowsBadRowOff);
    if (i < K && offsetsBad(t.cluster_path_off, i, K, P)) reportOffender(bad, i, kRowsBadPathOff);
    if (i < R && offsetsBad(t.row_grp_off, i, R, G)) reportOffender(bad, i, kRowsBadGrpOff);
    if (i < G && offsetsBad(t.grp_idx_off, i, G, M)) reportOffender(bad, i, kRowsBadIdxOff);
    if (i < P && offsetsBad(t.name_off, i, P, num_name_bytes)) reportOffender(bad, i, kRowsBadNameOff);
    if (i < R && !offsetsBad(t.row_grp_off, i, R, G)) {
        const uint64_t k = lastAtMost(t.cluster_row_off, K, i);
        if (t.cluster_row_off[k] <= i && i < t.cluster_row_off[k + 1] && !offsetsBad(t.cluster_path_off, k, K, P)) {  // (the offsets' threads report anything else)
            const uint64_t paths = t.cluster_path_off[k + 1] - t.cluster_path_off[k];
            for (uint64_t g = t.row_grp_off[i]; g < t.row_grp_off[i + 1]; ++g) {
                if (offsetsBad(t.grp_idx_off, g, G, M)) continue;
                for (uint64_t m = t.grp_idx_off[g]; m < t.grp_idx_off[g + 1]; ++m) {
                    if (t.path_idx[m] >= paths) reportOffender(bad, i, kRowsBadIndex, true);
                }
            }
        }
    }
}

// rowCell [R + 1] and clusterCell [K + 1] of a described input
__global__ __launch_bounds__(kBlock) void cellIndexKernel(const rp::DumpRows t, uint64_t * __restrict__ row_cell, uint64_t * __restrict__ cluster_cell) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i <= t.num_rows) row_cell[i] = rp::rowCell(t, i);
    if (i <= t.num_clusters) cluster_cell[i] = rp::clusterCell(t, i);
}

// the wavefront of blockWalk: the lane loop runs once
struct MeasureWave {
    uint32_t lane;
    uint64_t * cell_len;
    uint64_t exact;
    __device__ uint32_t laneBegin() const { return lane; }
    __device__ uint32_t laneEnd() const { return lane + 1; }
    __device__ void length(const uint64_t c, const uint64_t bytes) { cell_len[c] = bytes; }
    // (the write side of the walk is not instantiated for a measure)
    char * stage;
    uint32_t hi;
    __device__ void open(uint64_t) {}
    __device__ void flush(bool) {}
};

struct WriteWave {
    uint32_t lane;
    char * stage;
    char * text;
    uint64_t base;
    uint32_t lo, hi;
    uint64_t exact;
    __device__ uint32_t laneBegin() const { return lane; }
    __device__ uint32_t laneEnd() const { return lane + 1; }
    __device__ void length(uint64_t, uint64_t) {}
    __device__ void open(const uint64_t begin) {
        base = begin & ~3ull;
        lo = hi = static_cast<uint32_t>(begin & 3u);
    }
    __device__ void flush(const bool last) { ::flush(stage, text, base, lo, hi, last, lane); }
};

// cell_len [C + 1]: a wavefront per 64 consecutive cells, and a trailing 0
__global__ __launch_bounds__(64) void measureRowsKernel(const rp::DumpRows t, const uint64_t num_cells, uint64_t * __restrict__ cell_len, word64 * exact_cells) {
    if (blockIdx.x == 0 && threadIdx.x == 0) cell_len[num_cells] = 0;
    MeasureWave w = {threadIdx.x, cell_len, 0, nullptr, 0};
    for (uint64_t c0 = blockIdx.x * static_cast<uint64_t>(rp::kBlockCells); c0 < num_cells; c0 += gridDim.x * static_cast<uint64_t>(rp::kBlockCells)) {
        rp::blockWalk<false>(t, nullptr, c0, w);
    }
    const uint64_t exact = waveSum(w.exact);
    if (threadIdx.x == 0 && exact) atomicAdd(exact_cells, static_cast<word64>(exact));
}

// row_off [L + 1]: the offset of the first cell of every line, and the text's length behind the last
__global__ __launch_bounds__(kBlock) void lineOffsetsKernel(const rp::DumpRows t, const uint64_t * __restrict__ cell_off, uint64_t * __restrict__ row_off) {
    const uint64_t j = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (j <= rp::numLines(t)) row_off[j] = cell_off[rp::lineCell(t, j)];
}

__global__ __launch_bounds__(64) void writeRowsKernel(const rp::DumpRows t, const uint64_t num_cells, const uint64_t * __restrict__ cell_off, char * text) {
    __shared__ __attribute__((aligned(16))) char stage[(kStageBytes + 15) & ~15];
    WriteWave w = {threadIdx.x, stage, text, 0, 0, 0, 0};
    for (uint64_t c0 = blockIdx.x * static_cast<uint64_t>(rp::kBlockCells); c0 < num_cells; c0 += gridDim.x * static_cast<uint64_t>(rp::kBlockCells)) {
        rp::blockWalk<true>(t, cell_off, c0, w);
    }
}

// where the arrays of a dump lie
struct RowsSources {
    uint32_t K;
    uint64_t R, G, M, P;
    Source<uint64_t> cluster_row_off, cluster_path_off, row_grp_off, grp_idx_off, num_align_lists, cluster_index;
    Source<uint32_t> row_count, path_idx;
    Source<double> row_noise, grp_prob, path_effective_length;
};

int buildRowsText(rpvg_hip_ctx * ctx, const char * who, const RowsSources & in, const rpvg_table_labels * labels, const double prob_precision, rpvg_hip_table_text ** text_out) {
    *text_out = nullptr;
    if (const char * wrong = rp::probPrecisionBad(prob_precision)) {
        setError("%s: %s (%g)", who, wrong, prob_precision);
        return RPVG_HIP_ERR_INVALID;
    }
    const uint32_t K = in.K;
    const uint64_t R = in.R, G = in.G, M = in.M, P = in.P;
    rp::DumpRows t = {};
    t.num_clusters = K;
    t.num_rows = R;
    t.num_groups = G;
    t.num_entries = M;
    t.num_paths = P;
    t.digits = static_cast<int>(rp::probPrecisionDigits(prob_precision));
    t.num_align_lists = in.num_align_lists.from;
    t.cluster_index = in.cluster_index.from;
    RPVG_REQUIRE(R < (1ull << 40) && G < (1ull << 40) && M < (1ull << 40) && P < (1ull << 40), "%s: sizes beyond any text", who);
    if (const char * wrong = rp::descriptorBad(t)) {
        setError("%s: %s (%u clusters, %llu paths, %llu rows, %llu groups, %llu entries)", who, wrong, K, static_cast<unsigned long long>(P), static_cast<unsigned long long>(R),
                 static_cast<unsigned long long>(G), static_cast<unsigned long long>(M));
        return RPVG_HIP_ERR_INVALID;
    }
    RPVG_REQUIRE(labels->num_paths == P && labels->num_clusters == K, "%s: labels of %llu paths in %u clusters, the rows have %llu in %u", who,
                 static_cast<unsigned long long>(labels->num_paths), labels->num_clusters, static_cast<unsigned long long>(P), K);
    RPVG_REQUIRE(P == 0 || (labels->name_off && labels->path_length && (labels->num_name_bytes == 0 || labels->name_bytes)), "%s: NULL label array (the dump needs name_off, name_bytes and path_length)", who);
    RPVG_REQUIRE(P == 0 || in.path_effective_length.from, "%s: NULL path_effective_length", who);
    RPVG_REQUIRE(K == 0 || (in.cluster_row_off.from && in.cluster_path_off.from), "%s: NULL array", who);
    RPVG_REQUIRE(R == 0 || (in.row_count.from && in.row_noise.from && in.row_grp_off.from && in.grp_idx_off.from), "%s: NULL array", who);
    RPVG_REQUIRE((G == 0 || in.grp_prob.from) && (M == 0 || in.path_idx.from), "%s: NULL array", who);
    const uint64_t L = rp::numLines(t), C = rp::numCells(t);
    std::unique_ptr<rpvg_hip_table_text> text(new (std::nothrow) rpvg_hip_table_text());
    if (!text) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    text->ctx = ctx;
    text->num_paths = L;  // the rows of a rows text are its lines
    text->h_row_off.assign(static_cast<size_t>(L) + 1, 0);
    if (K == 0 || R == 0) {  // no cluster has a row: no bytes
        *text_out = text.release();
        return RPVG_HIP_OK;
    }

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    const bool labels_on_device = labels->on_device != 0;
    UploadPack inputs;
    DeviceBuffer<uint64_t> name_off, cluster_row_off, cluster_path_off, row_grp_off, grp_idx_off, lists, index, pow10, row_cell, cluster_cell, cell_len, cell_off, row_off;
    DeviceBuffer<char> name_bytes;
    DeviceBuffer<uint32_t> path_length, row_count, path_idx;
    DeviceBuffer<double> row_noise, grp_prob, eff_len;
    DeviceBuffer<word64> d_bad, d_exact;
    takeInput(inputs, name_off, Source<uint64_t>{labels->name_off, labels_on_device}, static_cast<size_t>(P) + 1);
    takeInput(inputs, name_bytes, Source<char>{labels->name_bytes, labels_on_device}, labels->num_name_bytes);
    takeInput(inputs, path_length, Source<uint32_t>{labels->path_length, labels_on_device}, P);
    takeInput(inputs, cluster_row_off, in.cluster_row_off, static_cast<size_t>(K) + 1);
    takeInput(inputs, cluster_path_off, in.cluster_path_off, static_cast<size_t>(K) + 1);
    takeInput(inputs, row_count, in.row_count, R);
    takeInput(inputs, row_noise, in.row_noise, R);
    takeInput(inputs, row_grp_off, in.row_grp_off, static_cast<size_t>(R) + 1);
    takeInput(inputs, grp_prob, in.grp_prob, G);
    takeInput(inputs, grp_idx_off, in.grp_idx_off, static_cast<size_t>(G) + 1);
    takeInput(inputs, path_idx, in.path_idx, M);
    takeInput(inputs, eff_len, in.path_effective_length, P);
    if (t.num_align_lists) {
        takeInput(inputs, lists, in.num_align_lists, K);
        takeInput(inputs, index, in.cluster_index, K);
    }
    inputs.add(pow10, pow10Table(), rpvg_number_text::kPow10Words);
    inputs.add(d_bad, &kNoBad, 1);
    inputs.addZero(d_exact, 1);
    {
        SpanScope copies(ctx, FAM_H2D);
        RPVG_HIP_CHECK(inputs.commit(st));
    }
    ctx->stats.h2d_bytes += static_cast<double>(inputs.copied_bytes);
    RPVG_HIP_CHECK(row_cell.alloc(static_cast<size_t>(R) + 1));
    RPVG_HIP_CHECK(cluster_cell.alloc(static_cast<size_t>(K) + 1));
    RPVG_HIP_CHECK(cell_len.alloc(static_cast<size_t>(C) + 1));
    RPVG_HIP_CHECK(cell_off.alloc(static_cast<size_t>(C) + 1));
    RPVG_HIP_CHECK(row_off.alloc(static_cast<size_t>(L) + 1));

    t.name_off = name_off.ptr;
    t.name_bytes = name_bytes.ptr;
    t.path_length = path_length.ptr;
    t.cluster_row_off = cluster_row_off.ptr;
    t.cluster_path_off = cluster_path_off.ptr;
    t.row_count = row_count.ptr;
    t.row_noise = row_noise.ptr;
    t.row_grp_off = row_grp_off.ptr;
    t.grp_prob = grp_prob.ptr;
    t.grp_idx_off = grp_idx_off.ptr;
    t.path_idx = path_idx.ptr;
    t.path_effective_length = eff_len.ptr;
    t.num_align_lists = t.num_align_lists ? lists.ptr : nullptr;
    t.cluster_index = t.cluster_index ? index.ptr : nullptr;
    t.pow10 = pow10.ptr;
    t.row_cell = row_cell.ptr;
    t.cluster_cell = cluster_cell.ptr;

    SpanScope span(ctx, FAM_BUILD);
    describeRowsKernel<<<gridFor(std::max<uint64_t>(std::max<uint64_t>(std::max<uint64_t>(K, P), R), G)), dim3(kBlock), 0, st>>>(t, labels->num_name_bytes, d_bad.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    word64 bad = kNoBad;
    if (const int rc = fetchDescribed(st, d_bad.ptr, &bad)) return rc;
    if (bad != kNoBad) {
        span.end();
        const Offender o = offenderOf(bad, kRowsBadIndex);
        setError("%s: %s %llu: %s", who, o.second_kind ? "row" : "position", static_cast<unsigned long long>(o.index), kRowsReasons[o.why]);
        return RPVG_HIP_ERR_INVALID;
    }
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((C + rp::kBlockCells - 1) / rp::kBlockCells, kMaxWriteBlocks));
    cellIndexKernel<<<gridFor(std::max<uint64_t>(R, K) + 1), dim3(kBlock), 0, st>>>(t, row_cell.ptr, cluster_cell.ptr);
    measureRowsKernel<<<dim3(blocks), dim3(64), 0, st>>>(t, C, cell_len.ptr, d_exact.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 2;
    if (const int rc = exclusiveSum(st, cell_len.ptr, cell_off.ptr, C + 1)) return rc;
    lineOffsetsKernel<<<gridFor(L + 1), dim3(kBlock), 0, st>>>(t, cell_off.ptr, row_off.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    word64 exact = 0;
    RPVG_HIP_CHECK(hipMemcpyAsync(text->h_row_off.data(), row_off.ptr, (static_cast<size_t>(L) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&exact, d_exact.ptr, sizeof(exact), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    ctx->stats.text_exact_cells += exact;
    text->num_bytes = text->h_row_off[L];
    for (uint64_t j = 0; j < L; ++j) text->num_rows += text->h_row_off[j + 1] > text->h_row_off[j] ? 1 : 0;
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
        writeRowsKernel<<<dim3(blocks), dim3(64), 0, st>>>(t, C, cell_off.ptr, text->text());
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

int rpvg_hip_rows_text(rpvg_hip_ctx * ctx, const rpvg_rows_text_input * input, const rpvg_table_labels * labels, double prob_precision,
                       rpvg_hip_table_text ** text_out) {
    const char * const who = "rpvg_hip_rows_text";
    RPVG_REQUIRE(ctx && input && labels && text_out, "%s: NULL argument", who);
    const bool dev = input->on_device != 0;
    RowsSources in = {};
    in.K = input->num_clusters;
    in.R = input->num_rows;
    in.G = input->num_groups;
    in.M = input->num_entries;
    in.P = input->num_paths;
    in.cluster_row_off = Source<uint64_t>{input->cluster_row_off, dev};
    in.cluster_path_off = Source<uint64_t>{input->cluster_path_off, dev};
    in.row_count = Source<uint32_t>{input->row_count, dev};
    in.row_noise = Source<double>{input->row_noise, dev};
    in.row_grp_off = Source<uint64_t>{input->row_grp_off, dev};
    in.grp_prob = Source<double>{input->grp_prob, dev};
    in.grp_idx_off = Source<uint64_t>{input->grp_idx_off, dev};
    in.path_idx = Source<uint32_t>{input->path_idx, dev};
    in.path_effective_length = Source<double>{input->path_effective_length, dev};
    in.num_align_lists = Source<uint64_t>{input->num_align_lists, dev};
    in.cluster_index = Source<uint64_t>{input->cluster_index, dev};
    return buildRowsText(ctx, who, in, labels, prob_precision, text_out);
}

int rpvg_hip_read_rows_text(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, const rpvg_table_labels * labels, const double * path_effective_length,
                            const uint64_t * num_align_lists, const uint64_t * cluster_index, double prob_precision, rpvg_hip_table_text ** text_out) {
    const char * const who = "rpvg_hip_read_rows_text";
    RPVG_REQUIRE(ctx && rows && labels && text_out, "%s: NULL argument", who);
    const ReadRowsResident resident = residentOf(rows);
    RowsSources in = {};
    in.K = resident.num_clusters;
    in.R = resident.num_rows;
    in.G = resident.num_groups;
    in.M = resident.num_members;
    in.P = resident.num_clusters ? resident.host_cluster_path_off[resident.num_clusters] : 0;
    in.cluster_row_off = Source<uint64_t>{resident.cluster_row_off, true};
    in.cluster_path_off = Source<uint64_t>{resident.host_cluster_path_off, false};
    in.row_count = Source<uint32_t>{resident.row_count, true};
    in.row_noise = Source<double>{resident.row_noise, true};
    in.row_grp_off = Source<uint64_t>{resident.row_grp_off, true};
    in.grp_prob = Source<double>{resident.grp_prob, true};
    in.grp_idx_off = Source<uint64_t>{resident.grp_idx_off, true};
    in.path_idx = Source<uint32_t>{resident.path_idx, true};
    in.path_effective_length = Source<double>{path_effective_length, false};
    in.num_align_lists = Source<uint64_t>{num_align_lists, false};
    in.cluster_index = Source<uint64_t>{cluster_index, false};
    return buildRowsText(ctx, who, in, labels, prob_precision, text_out);
}

}  // extern "C"
