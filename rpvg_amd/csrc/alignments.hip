// alignments.hip — the resident alignment batch from host arrays (interface include/rpvg_rows.h): what is refused, the cluster
// of every read, the output columns and the split of the reads between the two row kernels are planAlignmentBatch's
// (rows_plan.hpp); here the plan is copied to the device.  (align_index.hip makes the same batch from a finished index.)

#include "../../include/rpvg_rows.h"
#include "common.hpp"
#include "alignments.hpp"
#include "frag_length.hpp"
#include "rows_plan.hpp"
#include "table_kit.hpp"

using namespace rpvg_hip_detail;

static_assert(rpvg_rows_plan::kStatusOk == RPVG_HIP_OK && rpvg_rows_plan::kStatusInvalid == RPVG_HIP_ERR_INVALID, "rows_plan.hpp restates the status codes");

extern "C" int rpvg_hip_alignments_upload(rpvg_hip_ctx * ctx, const rpvg_alignment_batch * in, rpvg_hip_alignments ** out_handle) {
    RPVG_REQUIRE(ctx && in && out_handle, "rpvg_hip_alignments_upload: NULL argument");
    *out_handle = nullptr;
    const rpvg_rows_plan::AlignmentBatchPlan plan = rpvg_rows_plan::planAlignmentBatch(*in);
    if (plan.status != RPVG_HIP_OK) {
        setError("%s", plan.message.c_str());
        return plan.status;
    }
    const uint32_t K = plan.K;
    const uint64_t N = plan.N, A = plan.A, E = plan.E, P = plan.P;

    std::unique_ptr<rpvg_hip_alignments> al(new (std::nothrow) rpvg_hip_alignments());
    if (!al) {
        setError("rpvg_hip_alignments_upload: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    al->num_clusters = K;
    al->num_reads = N;
    al->num_aligns = A;
    al->num_entries = E;
    al->num_paths = P;
    al->collapse = plan.collapse;
    al->h_cluster_read_off.assign(in->cluster_read_off, in->cluster_read_off + K + 1);
    al->h_out_path_off = plan.h_out_path_off;
    al->num_small = plan.small_reads.size();
    al->num_large = plan.large_reads.size();

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SpanScope span(ctx, FAM_H2D);
    RPVG_HIP_CHECK(al->cluster_path_off.upload(in->cluster_path_off, K + 1, st));
    RPVG_HIP_CHECK(al->cluster_read_off.upload(in->cluster_read_off, K + 1, st));
    RPVG_HIP_CHECK(al->eff_len.upload(in->path_effective_length, P, st));
    if (plan.collapse) {
        RPVG_HIP_CHECK(al->source_count.upload(in->path_source_count, P, st));
        RPVG_HIP_CHECK(al->path_group.upload(in->path_group, P, st));
    }
    if (N) {
        RPVG_HIP_CHECK(al->read_cluster.upload(plan.read_cluster.data(), N, st));
        RPVG_HIP_CHECK(al->read_count.upload(in->read_count, N, st));
        RPVG_HIP_CHECK(al->mapq.upload(in->read_min_mapq, N, st));
        RPVG_HIP_CHECK(al->noise_score.upload(in->read_noise_score, N, st));
        RPVG_HIP_CHECK(al->read_align_off.upload(in->read_align_off, N + 1, st));
        RPVG_HIP_CHECK(al->score.upload(in->align_score_sum, A, st));
        RPVG_HIP_CHECK(al->align_length.upload(in->align_length, A, st));
        RPVG_HIP_CHECK(al->frag_length.upload(in->align_frag_length, A, st));
        RPVG_HIP_CHECK(al->align_path_off.upload(in->align_path_off, A + 1, st));
        RPVG_HIP_CHECK(al->path_idx.upload(in->align_path_idx, E, st));
    }
    if (al->num_small) RPVG_HIP_CHECK(al->small_reads.upload(plan.small_reads.data(), al->num_small, st));
    if (al->num_large) RPVG_HIP_CHECK(al->large_reads.upload(plan.large_reads.data(), al->num_large, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    span.end();
    ctx->stats.h2d_bytes += plan.h2d_bytes;
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the plan's lists leave scope
    *out_handle = al.release();
    return RPVG_HIP_OK;
}

extern "C" void rpvg_hip_alignments_free(rpvg_hip_ctx * ctx, rpvg_hip_alignments * alignments) {
    if (!alignments) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
    }
    delete alignments;
}

// PathInfo::effective_length of every path of the batch from its length (src/main.cpp:880), computed where the rows read it
extern "C" int rpvg_hip_alignments_set_effective_lengths(rpvg_hip_ctx * ctx, rpvg_hip_alignments * al, double loc, double scale, double shape,
                                                         const uint32_t * path_length, double * out) {
    RPVG_REQUIRE(ctx && al, "rpvg_hip_alignments_set_effective_lengths: NULL argument");
    const uint64_t P = al->num_paths;
    RPVG_REQUIRE(P == 0 || path_length, "rpvg_hip_alignments_set_effective_lengths: NULL path_length");
    if (P == 0) return RPVG_HIP_OK;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DeviceBuffer<uint32_t> d_length;
    DeviceBuffer<double> d_lower;
    RPVG_HIP_CHECK(d_length.upload(path_length, P, st));
    if (const int rc = launchEffectiveLengths(st, loc, scale, shape, d_length.ptr, P, al->eff_len.ptr, d_lower)) return rc;
    if (out) RPVG_HIP_CHECK(al->eff_len.download(out, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}
