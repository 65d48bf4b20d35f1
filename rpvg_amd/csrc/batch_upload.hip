// The device batch (rpvg_hip_batch, common.hpp) and its makers: the upload of a host batch in whichever forms it arrives
// (batch_forms.hpp decides them once), the batch pulled from its callers' segments, and the routine that turns grouped rows
// into the arrays of a batch, which the rows built on the device take too (read_rows.hip).  Every maker starts from one shell
// (newBatchShell) and ends in one tail (finishBatch).  gfx950 only.

#include "common.hpp"
#include "batch_forms.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

using namespace rpvg_hip_detail;
using rpvg_batch_forms::BatchForms;
using rpvg_batch_forms::OffsetForm;
using rpvg_batch_forms::groupEntryOffset;
using rpvg_batch_forms::rowGroupOffset;

// ---- kernels: expand (probability, path list) groups to entries -------------

// One thread per probability group: writes the group's probability next to
// each of its path indices (the path indices themselves are uploaded as is).
// (RowOff / GrpOff: the width the caller wrote the two long offset arrays in, include/rpvg_batch.h)
template <typename GrpOff>
__global__ void expandGroupsKernel(const uint64_t num_groups, const uint64_t num_entries, const GrpOff * __restrict__ grp_idx_off,
                                   const double * __restrict__ grp_prob, double * __restrict__ ent_prob) {
    const uint64_t g = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (g >= num_groups) return;
    const double p = grp_prob[g];
    // (clamped: the offsets are checked by validateRowsKernel, whose verdict the host reads after these kernels)
    for (uint64_t e = grp_idx_off[g]; e < min(static_cast<uint64_t>(grp_idx_off[g + 1]), num_entries); ++e) ent_prob[e] = p;
}

// One thread per row: entry range of the row and its count as double.
template <typename RowOff, typename GrpOff>
__global__ void rowMetaKernel(const uint64_t num_rows, const uint64_t num_groups, const RowOff * __restrict__ row_grp_off,
                              const GrpOff * __restrict__ grp_idx_off, const uint32_t * __restrict__ row_count_u32,
                              uint64_t * __restrict__ row_ent_off, double * __restrict__ row_count) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (r > num_rows) return;
    row_ent_off[r] = grp_idx_off[min(static_cast<uint64_t>(row_grp_off[r]), num_groups)];
    if (r < num_rows) row_count[r] = static_cast<double>(row_count_u32[r]);
}

// The row invariants the estimators rely on (src/main.cpp:855-887,953-973; src/read_path_probabilities.cpp:91-105,184,
// 212-219), one thread per row: consistent offsets, noise probability in (0, 1], path indices inside the row's cluster.
// first_bad_row: the smallest row that breaks one (the host words the message: validateClusters).  On the device because
// the host pass over a batch's 280 MB cost more than their copy (8 threads: 5 ms, before the first byte moved).
template <typename RowOff, typename GrpOff>
__global__ void validateRowsKernel(const uint64_t num_rows, const uint64_t num_groups, const uint64_t num_entries, const uint32_t num_clusters,
                                   const uint64_t * __restrict__ cluster_row_off, const uint64_t * __restrict__ cluster_path_off,
                                   const RowOff * __restrict__ row_grp_off, const GrpOff * __restrict__ grp_idx_off,
                                   const double * __restrict__ row_noise, const uint32_t * __restrict__ path_idx,
                                   unsigned long long * __restrict__ first_bad_row) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (r >= num_rows) return;
    bool good = true;
    const uint64_t g0 = row_grp_off[r], g1 = row_grp_off[r + 1];
    good = g0 <= g1 && g1 <= num_groups;
    const double nz = row_noise[r];
    good = good && nz > 0 && nz <= 1;
    if (good) {
        // the row's cluster: the last one that starts at or before it
        uint32_t lo = 0, hi = num_clusters;  // cluster_row_off[lo] <= r < cluster_row_off[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cluster_row_off[mid] <= r) lo = mid;
            else hi = mid;
        }
        const uint64_t n_paths = cluster_path_off[lo + 1] - cluster_path_off[lo];
        uint64_t e = grp_idx_off[g0];
        good = e <= num_entries;
        for (uint64_t g = g0; good && g < g1; ++g) {
            const uint64_t e1 = grp_idx_off[g + 1];
            good = e <= e1 && e1 <= num_entries;
            for (; good && e < e1; ++e) good = path_idx[e] < n_paths;
        }
    }
    if (!good) atomicMin(first_bad_row, static_cast<unsigned long long>(r));
}

namespace {

// counts of one byte -> their running sums in 32 bits: offsets[i] = counts[0] + ... + counts[i - 1], i = 0 .. n
struct CountAt {
    const uint8_t * counts;
    uint64_t n;
    __host__ __device__ uint32_t operator()(const uint64_t i) const { return i < n ? counts[i] : 0u; }
};

hipError_t queueOffsetsFromCounts(hipStream_t stream, const uint8_t * counts, const uint64_t n, uint32_t * offsets, DeviceBuffer<unsigned char> & scratch) {
    hipcub::CountingInputIterator<uint64_t> index(0);
    hipcub::TransformInputIterator<uint32_t, CountAt, hipcub::CountingInputIterator<uint64_t> > values(index, CountAt{counts, n});
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, values, offsets, static_cast<int>(n + 1), stream);
    if (e == hipSuccess) e = scratch.alloc(bytes);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(scratch.ptr, bytes, values, offsets, static_cast<int>(n + 1), stream);
    return e;
}

// the entry offset of every cluster's first row
__global__ void clusterEntryOffsetsKernel(const uint32_t num_clusters, const uint64_t * __restrict__ cluster_row_off, const uint64_t * __restrict__ row_ent_off,
                                          uint64_t * __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= num_clusters) out[k] = row_ent_off[cluster_row_off[k]];
}

// the narrow forms of a batch's copy back in 32 bits: path indices, read counts (a count of 255 stands for "listed": escapeRowCountsKernel), source ids
__global__ __launch_bounds__(256) void widenNarrowKernel(const uint16_t * __restrict__ path16, uint32_t * __restrict__ path32, const uint64_t num_entries,
                                                         const uint8_t * __restrict__ count8, uint32_t * __restrict__ count32, const uint64_t num_rows,
                                                         const uint16_t * __restrict__ source16, uint32_t * __restrict__ source32, const uint64_t num_sources,
                                                         const uint16_t * __restrict__ noise16, const double * __restrict__ noise_table, const uint32_t num_noise_values,
                                                         double * __restrict__ noise, const uint64_t num_noise_rows) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x, first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t i = first; i < num_noise_rows; i += stride) noise[i] = noise16[i] < num_noise_values ? noise_table[noise16[i]] : -1.0;
    for (uint64_t i = first; i < num_entries; i += stride) path32[i] = path16[i];
    for (uint64_t i = first; i < num_rows; i += stride) count32[i] = count8[i];
    for (uint64_t i = first; i < num_sources; i += stride) source32[i] = source16[i];
}

__global__ void escapeRowCountsKernel(const uint32_t * __restrict__ escape_row, const uint32_t * __restrict__ escape_count, const uint64_t num_escapes,
                                      const uint64_t num_rows, uint32_t * __restrict__ count32) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < num_escapes && escape_row[i] < num_rows) count32[escape_row[i]] = escape_count[i];
}

}  // namespace

namespace {
// ---- a batch from its callers' segments (include/rpvg_batch.h, rpvg_cluster_segment) ------------------------------------------
// What the kernel reads per cluster, in page-locked host memory like the segments themselves: the segment's arrays as pointers and
// where the cluster starts in every array of the device batch.
struct SegmentEntry {
    const uint32_t * row_count;
    const double * row_noise;
    const uint32_t * row_grp_off;
    const uint32_t * grp_idx_off;
    const double * grp_prob;
    const uint32_t * path_idx;
    const uint32_t * path_group_id;
    const uint32_t * path_source_off;
    const uint32_t * source_id;
    const uint32_t * col_count;  // the caller's haplotype columns (rpvg_cluster_segment::has_columns), else null
    const uint32_t * col_end;
    const uint32_t * col_path;
    uint32_t R, G, NNZ, P, S, C;  // (with columns S is their total list length L: the cluster's slots in the column arrays)
    uint64_t row_base, ent_base, path_base, src_base;
};

struct SegmentGatherArgs {
    const SegmentEntry * table;  // [K], host memory
    uint32_t num_clusters;
    uint32_t with_paths;
    uint64_t * cluster_row_off;
    uint64_t * cluster_path_off;
    uint64_t * cluster_src_off;
    double * row_count;
    double * row_noise;
    uint64_t * row_ent_off;
    uint32_t * ent_path;
    double * ent_prob;
    uint32_t * path_group_id;
    uint64_t * path_source_off;
    uint32_t * source_id;
    uint32_t with_columns;           // the segments carry their haplotype columns: src_col_* are written here
    uint32_t * src_col_count;
    uint32_t * src_col_end;
    uint32_t * src_col_path;
    unsigned long long * first_bad;  // smallest (cluster << 8 | kind) of an invalid segment; ~0: none
};

constexpr uint32_t kSegmentBadNoise = 1, kSegmentBadPath = 2, kSegmentBadOffsets = 3;

// Workgroups (k, y): cluster k's segment, slice y of its rows, groups, entries, paths and source ids.  Everything a thread reads
// from a segment is an index it has checked against the segment's own sizes first (the host has checked the arrays against the
// block): a caller's inconsistent offsets end in an error, not in a wild read.  Reads are 4 or 8 bytes per lane, a wave's next to
// each other: PCIe reads of 256-512 bytes.
__global__ __launch_bounds__(256) void segmentsGatherKernel(const SegmentGatherArgs a) {
    __shared__ SegmentEntry s_entry;
    const uint32_t k = blockIdx.x;
    if (threadIdx.x < sizeof(SegmentEntry) / 8) {
        reinterpret_cast<unsigned long long *>(&s_entry)[threadIdx.x] = reinterpret_cast<const unsigned long long *>(a.table + k)[threadIdx.x];
    }
    __syncthreads();
    const SegmentEntry & s = s_entry;
    const uint32_t t = blockIdx.y * blockDim.x + threadIdx.x, stride = gridDim.y * blockDim.x;
    uint32_t bad = 0;
    for (uint32_t r = t; r < s.R; r += stride) {
        const double noise = s.row_noise[r];
        const uint32_t g0 = s.row_grp_off[r], g1 = s.row_grp_off[r + 1];
        if (!(noise > 0 && noise <= 1)) bad = bad ? bad : kSegmentBadNoise;
        uint64_t first_entry = 0;
        if (g0 <= g1 && g1 <= s.G && (r > 0 || g0 == 0) && (r + 1 < s.R || g1 == s.G)) {
            first_entry = s.grp_idx_off[g0];
            if (first_entry > s.NNZ) bad = kSegmentBadOffsets;
        } else {
            bad = kSegmentBadOffsets;
        }
        a.row_count[s.row_base + r] = static_cast<double>(s.row_count[r]);
        a.row_noise[s.row_base + r] = noise;
        a.row_ent_off[s.row_base + r] = s.ent_base + first_entry;
    }
    for (uint32_t g = t; g < s.G; g += stride) {
        const uint32_t e0 = s.grp_idx_off[g], e1 = s.grp_idx_off[g + 1];
        if (e0 <= e1 && e1 <= s.NNZ && (g > 0 || e0 == 0) && (g + 1 < s.G || e1 == s.NNZ)) {
            const double prob = s.grp_prob[g];
            for (uint32_t e = e0; e < e1; ++e) a.ent_prob[s.ent_base + e] = prob;
        } else {
            bad = kSegmentBadOffsets;
        }
    }
    for (uint32_t e = t; e < s.NNZ; e += stride) {
        const uint32_t path = s.path_idx[e];
        if (!(path < s.P)) bad = bad ? bad : kSegmentBadPath;
        a.ent_path[s.ent_base + e] = path;
    }
    if (a.with_columns) {
        // the caller's columns into the cluster's slots (src_base: the lists' total lengths of the clusters before it)
        for (uint32_t p = t; p < s.P; p += stride) a.path_group_id[s.path_base + p] = s.path_group_id[p];
        for (uint32_t c = t; c < s.C; c += stride) {
            const uint32_t begin = c ? s.col_end[c - 1] : 0u, end = s.col_end[c];
            if (!(begin < end && end <= s.S && (c + 1 < s.C || end == s.S)) || s.col_count[c] == 0) bad = kSegmentBadOffsets;
            a.src_col_count[s.src_base + c] = s.col_count[c];
            a.src_col_end[s.src_base + c] = end;
        }
        for (uint32_t i = t; i < s.S; i += stride) {
            const uint32_t path = s.col_path[i];
            if (!(path < s.P)) bad = bad ? bad : kSegmentBadPath;
            a.src_col_path[s.src_base + i] = path;
        }
    } else if (a.with_paths) {
        for (uint32_t p = t; p < s.P; p += stride) {
            const uint32_t s0 = s.path_source_off[p], s1 = s.path_source_off[p + 1];
            if (!(s0 <= s1 && s1 <= s.S && (p > 0 || s0 == 0) && (p + 1 < s.P || s1 == s.S))) bad = kSegmentBadOffsets;
            a.path_group_id[s.path_base + p] = s.path_group_id[p];
            a.path_source_off[s.path_base + p] = s.src_base + s0;
        }
        for (uint32_t i = t; i < s.S; i += stride) a.source_id[s.src_base + i] = s.source_id[i];
    }
    if (t == 0) {
        a.cluster_row_off[k] = s.row_base;
        a.cluster_path_off[k] = s.path_base;
        a.row_ent_off[s.row_base + s.R] = s.ent_base + s.NNZ;  // (the next cluster's first row writes the same value)
        if (a.with_paths || a.with_columns) a.cluster_src_off[k] = s.src_base;
        if (a.with_paths && !a.with_columns) a.path_source_off[s.path_base + s.P] = s.src_base + s.S;
        if (k + 1 == a.num_clusters) {
            a.cluster_row_off[k + 1] = s.row_base + s.R;
            a.cluster_path_off[k + 1] = s.path_base + s.P;
            if (a.with_paths || a.with_columns) a.cluster_src_off[k + 1] = s.src_base + s.S;
        }
    }
    if (bad) atomicMin(a.first_bad, (static_cast<unsigned long long>(k) << 8) | bad);
}

}  // namespace

namespace rpvg_hip_detail {

namespace {
template <typename RowOff, typename GrpOff>
void launchGroupedRows(hipStream_t st, const GroupedRows & in, rpvg_hip_batch * b, unsigned long long * d_first_bad_row) {
    const RowOff * row_grp_off = static_cast<const RowOff *>(in.row_grp_off);
    const GrpOff * grp_idx_off = static_cast<const GrpOff *>(in.grp_idx_off);
    const uint64_t R = b->num_rows, G = in.num_groups, NNZ = b->num_entries;
    const uint32_t threads = 256;
    const dim3 group_grid(static_cast<uint32_t>((G + threads - 1) / threads)), meta_grid(static_cast<uint32_t>((R + 1 + threads - 1) / threads)),
        row_grid(static_cast<uint32_t>((R + threads - 1) / threads));
    if (G > 0) expandGroupsKernel<GrpOff><<<group_grid, dim3(threads), 0, st>>>(G, NNZ, grp_idx_off, in.grp_prob, b->ent_prob.ptr);
    rowMetaKernel<RowOff, GrpOff><<<meta_grid, dim3(threads), 0, st>>>(R, G, row_grp_off, grp_idx_off, in.row_count_u32, b->row_ent_off.ptr, b->row_count.ptr);
    if (d_first_bad_row && R > 0) {
        validateRowsKernel<RowOff, GrpOff><<<row_grid, dim3(threads), 0, st>>>(R, G, NNZ, b->num_clusters, b->cluster_row_off.ptr, b->cluster_path_off.ptr, row_grp_off,
                                                                              grp_idx_off, b->row_noise.ptr, b->ent_path.ptr, d_first_bad_row);
    }
}
}  // namespace

hipError_t queueGroupedRows(hipStream_t st, const GroupedRows & in, rpvg_hip_batch * b, unsigned long long * d_first_bad_row, uint64_t * d_cluster_ent_off) {
    // the one dispatch on (row width, group width): whichever widths arrived are read as they are
    if (in.row_off32 && in.grp_off32) launchGroupedRows<uint32_t, uint32_t>(st, in, b, d_first_bad_row);
    else if (in.row_off32) launchGroupedRows<uint32_t, uint64_t>(st, in, b, d_first_bad_row);
    else if (in.grp_off32) launchGroupedRows<uint64_t, uint32_t>(st, in, b, d_first_bad_row);
    else launchGroupedRows<uint64_t, uint64_t>(st, in, b, d_first_bad_row);
    if (d_cluster_ent_off) {
        const uint32_t K = b->num_clusters;
        clusterEntryOffsetsKernel<<<dim3((K + 1 + 255) / 256), dim3(256), 0, st>>>(K, b->cluster_row_off.ptr, b->row_ent_off.ptr, d_cluster_ent_off);
    }
    return hipGetLastError();
}

std::unique_ptr<rpvg_hip_batch> newBatchShell(const uint32_t K, const uint64_t R, const uint64_t NNZ, const uint64_t P, hipError_t & e) {
    std::unique_ptr<rpvg_hip_batch> b(new (std::nothrow) rpvg_hip_batch());
    if (!b) return b;
    b->num_clusters = K;
    b->num_rows = R;
    b->num_entries = NNZ;
    b->num_paths = P;
    b->h_cluster_row_off.assign(static_cast<size_t>(K) + 1, 0);
    b->h_cluster_path_off.assign(static_cast<size_t>(K) + 1, 0);
    b->h_cluster_ent_off.assign(static_cast<size_t>(K) + 1, 0);
    e = b->row_count.alloc(R);
    if (e == hipSuccess) e = b->row_ent_off.alloc(R + 1);
    if (e == hipSuccess) e = b->ent_prob.alloc(NNZ);
    return b;
}

}  // namespace rpvg_hip_detail

namespace {

using Upload = rpvg_hip_batch::UploadInProgress;

// ---- the tail of an upload: the verdict of the device's validation ------------------------------------------------------------
// The word the validating kernel lowers (all ones: nothing found), on stream `st` in front of it.
hipError_t armVerdict(Upload & up, hipStream_t st) {
    const hipError_t e = up.d_first_bad_row.alloc(1);
    return e != hipSuccess ? e : hipMemsetAsync(up.d_first_bad_row.ptr, 0xFF, sizeof(unsigned long long), st);
}

// The word's way back into the page-locked `host_word`, and the event behind everything that has been queued for the batch.
hipError_t queueVerdict(Upload & up, unsigned long long * host_word, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(host_word, up.d_first_bad_row.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&up.finished, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(up.finished, st);
    return e;
}

// Waits for that event, from any thread; then `verdict` — the maker's reading of what came back: RPVG_HIP_OK, or its own wording
// of the error — the sizes of the haplotype columns, and the batch is complete.  (the caller frees a batch that fails)
template <typename Verdict>
int finishBatch(rpvg_hip_batch * b, const char * what, Verdict verdict) {
    Upload & up = *b->upload;
    const hipError_t e = waitEvent(up.finished);
    if (e != hipSuccess) {
        setError("%s: %s", what, hipGetErrorString(e));
        return RPVG_HIP_ERR_RUNTIME;
    }
    int rc = verdict();
    if (rc == RPVG_HIP_OK) rc = finishPathSources(b, up.path_sources);
    if (rc == RPVG_HIP_OK) b->upload.reset();
    return rc;
}

// Words what is wrong with row r of cluster k (validateRowsKernel found it); true: nothing is.
constexpr size_t kProblemChars = rpvg_batch_forms::kMessageChars;
bool validateRow(const rpvg_cluster_batch * hb, const uint32_t k, const uint64_t r, char * message) {
    message[0] = 0;
    const uint64_t n_paths = hb->cluster_path_off[k + 1] - hb->cluster_path_off[k];
    const double nz = hb->row_noise16 ? (hb->row_noise16[r] < hb->num_row_noise_values ? hb->row_noise_table[hb->row_noise16[r]] : -1.0) : hb->row_noise[r];
    if (!(nz > 0 && nz <= 1)) {
        std::snprintf(message, kProblemChars, "rpvg_hip_batch_upload: row %llu has noise probability %g outside (0, 1]",
                      static_cast<unsigned long long>(r), nz);
        return false;
    }
    for (uint64_t e = groupEntryOffset(hb, rowGroupOffset(hb, r)); e < groupEntryOffset(hb, rowGroupOffset(hb, r + 1)); ++e) {
        const uint32_t path = hb->path_idx16 ? hb->path_idx16[e] : hb->path_idx[e];
        if (!(path < n_paths)) {
            std::snprintf(message, kProblemChars, "rpvg_hip_batch_upload: row %llu refers to path %u of a cluster with %llu paths",
                          static_cast<unsigned long long>(r), path, static_cast<unsigned long long>(n_paths));
            return false;
        }
    }
    return true;
}

// The two halves of an upload.  Begin: the plan (planBatchForms: the forms, the argument checks, the cluster offsets), copies
// queued on `ctx` (an uploader's stream, usually).  Finish: the kernels behind the copies — expansion of the (probability, path
// list) groups, row meta data, validation, read totals, the haplotype columns — on any context of the device, and the small
// results they bring back.  Both halves read the plan the upload keeps (Upload::forms).
int uploadBegin(rpvg_hip_ctx * ctx, const rpvg_cluster_batch * hb, rpvg_hip_batch ** batch_out) {
    RPVG_REQUIRE(ctx != nullptr && hb != nullptr && batch_out != nullptr, "rpvg_hip_batch_upload: NULL argument");
    *batch_out = nullptr;
    std::unique_ptr<HostScope> scope(new HostScope("batch_upload: host checks + offsets"));
    BatchForms forms;
    std::vector<uint64_t> cluster_ent_off;
    char message[rpvg_batch_forms::kMessageChars];
    RPVG_REQUIRE(rpvg_batch_forms::planBatchForms(hb, &forms, &cluster_ent_off, message), "%s", message);
    const uint32_t K = forms.K;
    const uint64_t R = forms.R, G = forms.G, NNZ = forms.NNZ;

    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));

    hipError_t e = hipSuccess;
    std::unique_ptr<rpvg_hip_batch> b = newBatchShell(K, R, NNZ, forms.P, e);
    if (!b) {
        setError("rpvg_hip_batch_upload: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    b->h_cluster_row_off.assign(hb->cluster_row_off, hb->cluster_row_off + K + 1);
    b->h_cluster_path_off.assign(hb->cluster_path_off, hb->cluster_path_off + K + 1);
    b->h_cluster_ent_off.swap(cluster_ent_off);  // (with the counts: from the device, behind their sums — uploadFinishWait)
    b->upload.reset(new Upload());
    Upload & up = *b->upload;
    up.forms = forms;
    scope.reset(new HostScope("batch_upload: copies queued"));

    const int span = ctx->spanBegin(FAM_H2D);
    hipStream_t st = ctx->stream;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    ok(b->cluster_row_off.upload(hb->cluster_row_off, K + 1, st));
    ok(b->cluster_path_off.upload(hb->cluster_path_off, K + 1, st));
    if (forms.noise16) {  // (looked up behind the copy: widenNarrowKernel; an index outside the table becomes a noise of -1 and fails the validation)
        ok(up.d_row_noise16.upload(hb->row_noise16, R, st));
        ok(up.d_row_noise_table.upload(hb->row_noise_table, hb->num_row_noise_values, st));
        ok(b->row_noise.alloc(R));
    } else {
        ok(b->row_noise.upload(hb->row_noise, R, st));
    }
    if (forms.count8) {  // (widened behind the copy, the listed rows written over: widenNarrowKernel)
        ok(up.d_row_count8.upload(hb->row_count8, R, st));
        ok(up.d_escape_row.upload(hb->row_count_escape_row, hb->num_row_count_escapes, st));
        ok(up.d_escape_count.upload(hb->row_count_escape_count, hb->num_row_count_escapes, st));
        ok(up.d_row_count_u32.alloc(R));
    } else {
        ok(up.d_row_count_u32.upload(hb->row_count, R, st));
    }
    // the two long offset arrays travel in the form they came in; the kernels behind the copy read either width (queueGroupedRows).
    // (an array of no rows, or of no groups, may be NULL: one zero of its width stands for it)
    const uint64_t zero_off[1] = {0};
    const uint32_t zero_off32[1] = {0};
    if (forms.counts()) {
        ok(up.d_row_grp_count8.upload(hb->row_grp_count8, R, st));
        ok(up.d_grp_idx_count8.upload(hb->grp_idx_count8, G, st));
        ok(up.d_row_grp_off32.alloc(R + 1));
        ok(up.d_grp_idx_off32.alloc(G + 1));
    } else {
        if (forms.row_offsets == OffsetForm::Narrow32) ok(up.d_row_grp_off32.upload(R ? hb->row_grp_off32 : zero_off32, R + 1, st));
        else ok(up.d_row_grp_off.upload(R ? hb->row_grp_off : zero_off, R + 1, st));
        if (forms.group_offsets == OffsetForm::Narrow32) ok(up.d_grp_idx_off32.upload(G ? hb->grp_idx_off32 : zero_off32, G + 1, st));
        else ok(up.d_grp_idx_off.upload(G ? hb->grp_idx_off : zero_off, G + 1, st));
    }
    ok(up.d_grp_prob.upload(hb->grp_prob, G, st));
    if (forms.path16) {
        ok(up.d_path_idx16.upload(hb->path_idx16, NNZ, st));
        ok(b->ent_path.alloc(NNZ));
    } else {
        ok(b->ent_path.upload(hb->path_idx, NNZ, st));
    }
    // the path side, when the caller handed it in: PathInfo::group_id and source_ids (path_sources.hip)
    if (e == hipSuccess) ok(queuePathSourceCopies(ctx, b.get(), hb, up.path_sources));
    ctx->spanEnd(span);
    ctx->stats.h2d_bytes += static_cast<double>(forms.row_copy_bytes);
    if (e != hipSuccess) {
        setError("rpvg_hip_batch_upload: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    *batch_out = b.release();
    return RPVG_HIP_OK;
}

// The second half of an upload in two steps.  Queue: the kernels behind the copies and the copies of their small results into a
// page-locked block, on stream `st` of `ctx` (the copies have been waited for: rpvg_hip_batch_upload_begin), an event behind them.
// Wait: for that event, from any thread, and the host's part (messages, sizes of the haplotype columns).  A pipeline's uploader
// queues them behind every batch's copies on its side stream and goes on copying; the estimator that takes the batch finds them
// done, or nearly (rpvg_amd/host/batch_pipeline.hpp).  (the caller holds no lock; `b` is deleted on failure)
int uploadFinishQueue(rpvg_hip_ctx * ctx, rpvg_hip_batch * b, hipStream_t st) {
    Upload & up = *b->upload;
    const BatchForms & forms = up.forms;
    const uint32_t K = forms.K;
    const uint64_t R = forms.R, G = forms.G, NNZ = forms.NNZ;
    // (the context's lock for its main stream — and its statistics — only: on the side stream of an uploader's context a thread of
    // its own queues these while the uploader queues the next batch's copies)
    const bool own_stream = st == ctx->stream;
    std::unique_lock<std::mutex> lock(ctx->mutex, std::defer_lock);
    if (own_stream) lock.lock();
    hipError_t e = hipSetDevice(ctx->device);
    HostScope scope("batch_upload: kernels queued");
    // (on an uploader's side stream the span is opened and closed under a short hold of the context's lock, and only by a context
    // that times every kernel family — RPVG_HIP_SPANS=2, bench.py's instrumented pass: the thread that queues these stands behind
    // the uploader's copies for it)
    const bool side_span = !own_stream && ctx->span_level >= 2;
    int bspan = -1;
    if (own_stream) {
        bspan = ctx->spanBegin(FAM_BUILD, st);
    } else if (side_span) {
        std::lock_guard<std::mutex> span_lock(ctx->mutex);
        bspan = ctx->spanBegin(FAM_BUILD, st);
    }
    // the narrow forms of the copy (include/rpvg_batch.h): noise, path indices, read counts and source ids back in their full width
    const uint64_t path16 = forms.path16 ? NNZ : 0, count8 = forms.count8 ? R : 0, noise16 = forms.noise16 ? R : 0;
    const uint64_t source16 = up.path_sources.d_source_id16.ptr ? up.path_sources.num_sources_narrow : 0;
    if (e == hipSuccess && (path16 || count8 || noise16 || source16)) {
        const uint64_t most = std::max<uint64_t>(std::max<uint64_t>(path16, std::max<uint64_t>(count8, noise16)), source16);
        widenNarrowKernel<<<dim3(static_cast<uint32_t>(std::min<uint64_t>((most + 1023) / 1024 + 1, 4096))), dim3(256), 0, st>>>(
            up.d_path_idx16.ptr, b->ent_path.ptr, path16, up.d_row_count8.ptr, up.d_row_count_u32.ptr, count8,
            up.path_sources.d_source_id16.ptr, up.path_sources.d_source_id.ptr, source16,
            up.d_row_noise16.ptr, up.d_row_noise_table.ptr, static_cast<uint32_t>(up.d_row_noise_table.count), b->row_noise.ptr, noise16);
        if (up.d_escape_row.count) {
            escapeRowCountsKernel<<<dim3(static_cast<uint32_t>((up.d_escape_row.count + 255) / 256)), dim3(256), 0, st>>>(
                up.d_escape_row.ptr, up.d_escape_count.ptr, up.d_escape_row.count, R, up.d_row_count_u32.ptr);
        }
    }
    if (e == hipSuccess) e = armVerdict(up, st);
    const bool counts = forms.counts();
    if (e == hipSuccess && counts) {  // the offsets the kernels below read: the counts' running sums, in 32 bits
        e = queueOffsetsFromCounts(st, up.d_row_grp_count8.ptr, R, up.d_row_grp_off32.ptr, up.scan_scratch_rows);
        if (e == hipSuccess) e = queueOffsetsFromCounts(st, up.d_grp_idx_count8.ptr, G, up.d_grp_idx_off32.ptr, up.scan_scratch_groups);
        if (e == hipSuccess) e = up.d_cluster_ent_off.alloc(K + 1);
    }
    if (e == hipSuccess) {
        GroupedRows rows;
        rows.num_groups = G;
        rows.row_off32 = forms.row_offsets != OffsetForm::Wide64;
        rows.grp_off32 = forms.group_offsets != OffsetForm::Wide64;
        rows.row_grp_off = rows.row_off32 ? static_cast<const void *>(up.d_row_grp_off32.ptr) : up.d_row_grp_off.ptr;
        rows.grp_idx_off = rows.grp_off32 ? static_cast<const void *>(up.d_grp_idx_off32.ptr) : up.d_grp_idx_off.ptr;
        rows.grp_prob = up.d_grp_prob.ptr;
        rows.row_count_u32 = up.d_row_count_u32.ptr;
        e = queueGroupedRows(st, rows, b, up.d_first_bad_row.ptr, counts ? up.d_cluster_ent_off.ptr : nullptr);
    }
    // read counts per cluster (the host summed three million of them per batch with a team of its own)
    if (e == hipSuccess) e = up.d_cluster_total.alloc(K);
    if (e == hipSuccess) e = queueClusterTotals(st, K, b->cluster_row_off.ptr, up.d_row_count_u32.ptr, up.d_cluster_total.ptr);
    if (e == hipSuccess) e = queuePathSourceKernels(ctx, b, up.path_sources, st);
    if (own_stream) {
        ctx->spanEnd(bspan);
        ctx->stats.build_launches += 5;
    } else if (side_span) {
        std::lock_guard<std::mutex> span_lock(ctx->mutex);
        ctx->spanEnd(bspan);
        ctx->stats.build_launches += 5;
    }
    if (e == hipSuccess) e = hipGetLastError();
    // the small results: [first bad row, 64 bits | the counts' two sums | - | read totals K doubles | entry offsets K + 1]
    const size_t result_bytes = 16 + 8 * static_cast<size_t>(K) + 8 * (static_cast<size_t>(K) + 1);
    if (e == hipSuccess) e = pinnedAlloc(&up.h_results, result_bytes);
    if (e == hipSuccess) {
        unsigned char * host = static_cast<unsigned char *>(up.h_results);
        memset(host, 0, 16);
        if (counts) e = hipMemcpyAsync(host + 8, up.d_row_grp_off32.ptr + R, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(host + 12, up.d_grp_idx_off32.ptr + G, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && K > 0) e = hipMemcpyAsync(host + 16, up.d_cluster_total.ptr, K * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && counts) e = hipMemcpyAsync(host + 16 + 8 * static_cast<size_t>(K), up.d_cluster_ent_off.ptr, (K + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = queueVerdict(up, reinterpret_cast<unsigned long long *>(host), st);
    }
    if (e != hipSuccess) {
        setError("rpvg_hip_batch_upload: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        delete b;
        return RPVG_HIP_ERR_RUNTIME;
    }
    return RPVG_HIP_OK;
}

int uploadFinishWait(rpvg_hip_batch * b, const rpvg_cluster_batch * hb) {
    HostScope scope("batch_upload: wait for the kernels");
    const int rc = finishBatch(b, "rpvg_hip_batch_upload", [b, hb]() {
        const Upload & up = *b->upload;
        const uint32_t K = up.forms.K;
        const uint64_t G = up.forms.G, NNZ = up.forms.NNZ;
        const unsigned char * host = static_cast<const unsigned char *>(up.h_results);
        unsigned long long first_bad_row = ~0ull;
        uint32_t count_totals[2] = {0, 0};  // what the counts add up to (against the totals the caller named)
        memcpy(&first_bad_row, host, sizeof(first_bad_row));
        memcpy(count_totals, host + 8, sizeof(count_totals));
        b->h_cluster_total.resize(K);
        if (K > 0) memcpy(b->h_cluster_total.data(), host + 16, K * sizeof(double));
        if (up.forms.counts()) memcpy(b->h_cluster_ent_off.data(), host + 16 + 8 * static_cast<size_t>(K), (K + 1) * sizeof(uint64_t));
        if (up.forms.counts() && (count_totals[0] != G || count_totals[1] != NNZ)) {
            setError("rpvg_hip_batch_upload: the counts of the rows' groups and of the groups' paths do not add up to num_groups = %llu and num_entries = %llu",
                     static_cast<unsigned long long>(G), static_cast<unsigned long long>(NNZ));
            return RPVG_HIP_ERR_INVALID;
        }
        if (first_bad_row != ~0ull) {  // the message: the host's reading of the offending row's cluster
            const uint32_t k = static_cast<uint32_t>(std::upper_bound(hb->cluster_row_off, hb->cluster_row_off + K + 1, first_bad_row) - hb->cluster_row_off) - 1;
            char message[kProblemChars];
            const uint64_t g0 = rowGroupOffset(hb, first_bad_row), g1 = rowGroupOffset(hb, first_bad_row + 1);
            bool offsets_ok = g0 <= g1 && g1 <= G;
            for (uint64_t g = g0; offsets_ok && g < g1; ++g) offsets_ok = groupEntryOffset(hb, g) <= groupEntryOffset(hb, g + 1) && groupEntryOffset(hb, g + 1) <= NNZ;
            if (!offsets_ok || validateRow(hb, k, first_bad_row, message)) {
                std::snprintf(message, kProblemChars, "rpvg_hip_batch_upload: row %llu has inconsistent group or entry offsets", first_bad_row);
            }
            setError("%s", message);
            return RPVG_HIP_ERR_INVALID;
        }
        return RPVG_HIP_OK;
    });
    if (rc != RPVG_HIP_OK) delete b;
    return rc;
}

int uploadFinish(rpvg_hip_ctx * ctx, rpvg_hip_batch * b, const rpvg_cluster_batch * hb) {
    const int rc = uploadFinishQueue(ctx, b, ctx->stream);
    return rc != RPVG_HIP_OK ? rc : uploadFinishWait(b, hb);
}

}  // namespace

extern "C" {

int rpvg_hip_batch_upload(rpvg_hip_ctx * ctx, const rpvg_cluster_batch * hb, rpvg_hip_batch ** batch_out) {
    rpvg_hip_batch * b = nullptr;
    int rc = uploadBegin(ctx, hb, &b);
    if (rc != RPVG_HIP_OK) return rc;
    rc = uploadFinish(ctx, b, hb);  // (same stream: behind the copies)
    if (rc != RPVG_HIP_OK) return rc;
    *batch_out = b;
    return RPVG_HIP_OK;
}

int rpvg_hip_batch_upload_begin(rpvg_hip_ctx * ctx, const rpvg_cluster_batch * hb, rpvg_hip_batch ** batch_out) {
    rpvg_hip_batch * b = nullptr;
    const int rc = uploadBegin(ctx, hb, &b);
    if (rc != RPVG_HIP_OK) return rc;
    // the copies are done: any context of the device may finish the batch.  (An event, waited for without the context's lock:
    // another thread may queue the kernels behind an earlier batch's copies on this context's side stream meanwhile.)
    hipError_t e = hipSuccess;
    hipEvent_t copied = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(copied, ctx->stream);
    }
    if (e == hipSuccess) e = waitEvent(copied);
    if (copied) (void) hipEventDestroy(copied);
    if (e != hipSuccess) {
        setError("rpvg_hip_batch_upload_begin: %s", hipGetErrorString(e));
        delete b;
        return RPVG_HIP_ERR_RUNTIME;
    }
    *batch_out = b;
    return RPVG_HIP_OK;
}

int rpvg_hip_batch_upload_finish_queue(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch, const rpvg_cluster_batch * hb) {
    RPVG_REQUIRE(ctx != nullptr && batch != nullptr && hb != nullptr, "rpvg_hip_batch_upload_finish_queue: NULL argument");
    RPVG_REQUIRE(batch->upload != nullptr && batch->upload->finished == nullptr, "rpvg_hip_batch_upload_finish_queue: the batch is complete, or queued, already");
    RPVG_REQUIRE(hb->num_clusters == batch->num_clusters && hb->cluster_row_off && hb->cluster_row_off[hb->num_clusters] == batch->num_rows,
                 "rpvg_hip_batch_upload_finish_queue: not the host batch the upload began with");
    // (an uploader's context: its side stream — its main stream carries the next batch's copies)
    return uploadFinishQueue(ctx, batch, ctx->aux_count > 0 && ctx->aux[0] ? ctx->aux[0] : ctx->stream);
}

int rpvg_hip_batch_upload_finish_wait(rpvg_hip_batch * batch, const rpvg_cluster_batch * hb) {
    RPVG_REQUIRE(batch != nullptr && hb != nullptr, "rpvg_hip_batch_upload_finish_wait: NULL argument");
    RPVG_REQUIRE(batch->upload != nullptr && batch->upload->finished != nullptr, "rpvg_hip_batch_upload_finish_wait: nothing queued for this batch");
    return uploadFinishWait(batch, hb);
}

int rpvg_hip_batch_upload_finish(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch, const rpvg_cluster_batch * hb) {
    RPVG_REQUIRE(ctx != nullptr && batch != nullptr && hb != nullptr, "rpvg_hip_batch_upload_finish: NULL argument");
    RPVG_REQUIRE(batch->upload != nullptr, "rpvg_hip_batch_upload_finish: the batch is complete already");
    RPVG_REQUIRE(hb->num_clusters == batch->num_clusters && hb->cluster_row_off && hb->cluster_row_off[hb->num_clusters] == batch->num_rows,
                 "rpvg_hip_batch_upload_finish: not the host batch the upload began with");
    return uploadFinish(ctx, batch, hb);
}

int rpvg_hip_batch_upload_segments(rpvg_hip_ctx * ctx, const rpvg_cluster_segment * segments, uint32_t K, rpvg_hip_batch ** batch_out) {
    RPVG_REQUIRE(ctx != nullptr && batch_out != nullptr && (segments != nullptr || K == 0), "rpvg_hip_batch_upload_segments: NULL argument");
    *batch_out = nullptr;
    std::unique_ptr<HostScope> scope(new HostScope("batch_upload_segments: host checks + table"));
    const bool with_columns = K > 0 && segments[0].has_columns != 0;
    const bool with_paths = K > 0 && segments[0].has_paths != 0 && !with_columns;
    uint64_t R = 0, NNZ = 0, P = 0, S = 0, most_work = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const rpvg_cluster_segment & g = segments[k];
        RPVG_REQUIRE(g.base != nullptr && pinnedCapacity(g.base) >= g.bytes, "rpvg_hip_batch_upload_segments: segment %u does not lie in a block of rpvg_hip_pinned_alloc", k);
        RPVG_REQUIRE((g.has_columns != 0) == with_columns, "rpvg_hip_batch_upload_segments: segment %u: all segments of a batch carry their haplotype columns, or none", k);
        RPVG_REQUIRE(with_columns || (g.has_paths != 0) == with_paths, "rpvg_hip_batch_upload_segments: segment %u: all segments of a batch carry their paths, or none", k);
        RPVG_REQUIRE(g.num_paths <= 0x7fffffffu, "rpvg_hip_batch_upload_segments: segment %u has too many paths", k);
        auto inside = [&](const uint64_t at, const uint64_t count, const uint64_t width) { return (at & 7) == 0 && at <= g.bytes && count * width <= g.bytes - at; };
        bool fits = inside(g.row_count_at, g.num_rows, 4) && inside(g.row_noise_at, g.num_rows, 8) && inside(g.row_grp_off_at, static_cast<uint64_t>(g.num_rows) + 1, 4) &&
                    inside(g.grp_idx_off_at, static_cast<uint64_t>(g.num_groups) + 1, 4) && inside(g.grp_prob_at, g.num_groups, 8) && inside(g.path_idx_at, g.num_entries, 4);
        if (with_paths) {
            fits = fits && inside(g.path_group_id_at, g.num_paths, 4) && inside(g.path_source_off_at, static_cast<uint64_t>(g.num_paths) + 1, 4) && inside(g.source_id_at, g.num_sources, 4);
        }
        if (with_columns) {
            fits = fits && inside(g.path_group_id_at, g.num_paths, 4) && inside(g.col_count_at, g.num_columns, 4) && inside(g.col_end_at, g.num_columns, 4) &&
                   inside(g.col_path_at, g.num_column_paths, 4) && g.num_columns <= g.num_column_paths && g.max_column_paths <= g.num_column_paths &&
                   (g.num_columns > 0) == (g.num_column_paths > 0);
        }
        RPVG_REQUIRE(fits, "rpvg_hip_batch_upload_segments: an array of segment %u is misaligned or outside its block", k);
        RPVG_REQUIRE(g.num_rows > 0 || (g.num_groups == 0 && g.num_entries == 0), "rpvg_hip_batch_upload_segments: segment %u has groups without rows", k);
        R += g.num_rows;
        NNZ += g.num_entries;
        P += g.num_paths;
        const uint32_t slots = with_columns ? g.num_column_paths : (with_paths ? g.num_sources : 0u);
        S += slots;
        most_work = std::max<uint64_t>(most_work, std::max<uint64_t>(std::max(g.num_rows, g.num_groups), std::max(g.num_entries, slots)));
    }
    RPVG_REQUIRE(NNZ < 0xffffffffull, "rpvg_hip_batch_upload_segments: a batch of 2^32 - 1 entries or more");

    std::unique_lock<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    std::unique_ptr<rpvg_hip_batch> b = newBatchShell(K, R, NNZ, P, e);
    if (!b) {
        setError("rpvg_hip_batch_upload_segments: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    b->h_cluster_total.resize(K);
    if (with_paths || with_columns) b->h_cluster_src_off.assign(K + 1, 0);
    if (with_columns) {
        b->h_src_num_cols.resize(K);
        b->h_src_col_paths.resize(K);
        b->h_src_max_col_paths.resize(K);
    }
    b->upload.reset(new Upload());
    Upload & up = *b->upload;
    hipStream_t st = ctx->stream;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
    // the table, and behind it the two words that come back (first invalid segment)
    const size_t table_bytes = std::max<size_t>(K, 1) * sizeof(SegmentEntry);
    void * h_table = nullptr;
    if (pinnedAlloc(&h_table, table_bytes + 16) != hipSuccess) {
        setError("rpvg_hip_batch_upload_segments: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    up.h_results = h_table;  // (freed with the upload)
    SegmentEntry * table = static_cast<SegmentEntry *>(h_table);
    for (uint32_t k = 0; k < K; ++k) {
        const rpvg_cluster_segment & g = segments[k];
        const unsigned char * base = static_cast<const unsigned char *>(g.base);
        SegmentEntry & t = table[k];
        t.row_count = reinterpret_cast<const uint32_t *>(base + g.row_count_at);
        t.row_noise = reinterpret_cast<const double *>(base + g.row_noise_at);
        t.row_grp_off = reinterpret_cast<const uint32_t *>(base + g.row_grp_off_at);
        t.grp_idx_off = reinterpret_cast<const uint32_t *>(base + g.grp_idx_off_at);
        t.grp_prob = reinterpret_cast<const double *>(base + g.grp_prob_at);
        t.path_idx = reinterpret_cast<const uint32_t *>(base + g.path_idx_at);
        t.path_group_id = (with_paths || with_columns) ? reinterpret_cast<const uint32_t *>(base + g.path_group_id_at) : nullptr;
        t.col_count = with_columns ? reinterpret_cast<const uint32_t *>(base + g.col_count_at) : nullptr;
        t.col_end = with_columns ? reinterpret_cast<const uint32_t *>(base + g.col_end_at) : nullptr;
        t.col_path = with_columns ? reinterpret_cast<const uint32_t *>(base + g.col_path_at) : nullptr;
        t.path_source_off = with_paths ? reinterpret_cast<const uint32_t *>(base + g.path_source_off_at) : nullptr;
        t.source_id = with_paths ? reinterpret_cast<const uint32_t *>(base + g.source_id_at) : nullptr;
        t.R = g.num_rows;
        t.G = g.num_groups;
        t.NNZ = g.num_entries;
        t.P = g.num_paths;
        t.S = with_columns ? g.num_column_paths : (with_paths ? g.num_sources : 0);
        t.C = with_columns ? g.num_columns : 0;
        t.row_base = b->h_cluster_row_off[k];
        t.ent_base = b->h_cluster_ent_off[k];
        t.path_base = b->h_cluster_path_off[k];
        t.src_base = (with_paths || with_columns) ? b->h_cluster_src_off[k] : 0;
        b->h_cluster_row_off[k + 1] = t.row_base + t.R;
        b->h_cluster_ent_off[k + 1] = t.ent_base + t.NNZ;
        b->h_cluster_path_off[k + 1] = t.path_base + t.P;
        if (with_paths || with_columns) b->h_cluster_src_off[k + 1] = t.src_base + t.S;
        if (with_columns) {
            b->h_src_num_cols[k] = g.num_columns;
            b->h_src_col_paths[k] = g.num_column_paths;
            b->h_src_max_col_paths[k] = g.max_column_paths;
        }
        b->h_cluster_total[k] = static_cast<double>(g.total_read_count);
    }
    unsigned long long * h_first_bad = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(h_table) + table_bytes);
    *h_first_bad = ~0ull;

    scope.reset(new HostScope("batch_upload_segments: kernels queued"));
    ok(b->cluster_row_off.alloc(K + 1));
    ok(b->cluster_path_off.alloc(K + 1));
    ok(b->row_noise.alloc(R));
    ok(b->ent_path.alloc(NNZ));
    if (e == hipSuccess && with_paths) ok(reservePathSources(b.get(), K, P, S, up.path_sources));
    const bool sources = with_paths && up.path_sources.copied;
    const bool columns = with_columns && P > 0 && S > 0;
    if (e == hipSuccess && columns) {  // the columns come with the segments: their slots, nothing to form
        ok(b->path_group_id.alloc(P));
        ok(b->cluster_src_off.alloc(K + 1));
        ok(b->src_col_count.alloc(S));
        ok(b->src_col_end.alloc(S));
        ok(b->src_col_path.alloc(S));
    }
    if (e == hipSuccess) ok(armVerdict(up, st));
    const int span = ctx->spanBegin(FAM_BUILD, st);
    if (e == hipSuccess && K > 0) {
        SegmentGatherArgs a;
        a.table = table;
        a.num_clusters = K;
        a.with_paths = sources ? 1 : 0;
        a.cluster_row_off = b->cluster_row_off.ptr;
        a.cluster_path_off = b->cluster_path_off.ptr;
        a.cluster_src_off = (sources || columns) ? b->cluster_src_off.ptr : nullptr;
        a.with_columns = columns ? 1 : 0;
        a.src_col_count = columns ? b->src_col_count.ptr : nullptr;
        a.src_col_end = columns ? b->src_col_end.ptr : nullptr;
        a.src_col_path = columns ? b->src_col_path.ptr : nullptr;
        a.row_count = b->row_count.ptr;
        a.row_noise = b->row_noise.ptr;
        a.row_ent_off = b->row_ent_off.ptr;
        a.ent_path = b->ent_path.ptr;
        a.ent_prob = b->ent_prob.ptr;
        a.path_group_id = (sources || columns) ? b->path_group_id.ptr : nullptr;
        a.path_source_off = sources ? up.path_sources.d_path_source_off.ptr : nullptr;
        a.source_id = sources ? up.path_sources.d_source_id.ptr : nullptr;
        a.first_bad = up.d_first_bad_row.ptr;
        // slices per cluster: four items of the largest cluster's longest array per thread, 64 at the most (a cluster of a million
        // rows: sixty passes of 16 384 threads)
        const uint32_t slices = static_cast<uint32_t>(std::min<uint64_t>(64, std::max<uint64_t>(1, (most_work + 1023) / 1024)));
        segmentsGatherKernel<<<dim3(K, slices), dim3(256), 0, st>>>(a);
        ok(hipGetLastError());
    }
    if (e == hipSuccess && sources) ok(queuePathSourceKernels(ctx, b.get(), up.path_sources, st));
    ctx->spanEnd(span);
    ctx->stats.build_launches += sources ? 3 : 1;
    ctx->stats.h2d_bytes += static_cast<double>(R * 16 + NNZ * 4 + P * 8 + S * 4);  // (what the kernel pulls: no copy command)
    if (e == hipSuccess) ok(queueVerdict(up, h_first_bad, st));
    if (e != hipSuccess) {
        setError("rpvg_hip_batch_upload_segments: %s", hipGetErrorString(e));
        (void) hipStreamSynchronize(st);
        return (e == hipErrorOutOfMemory) ? RPVG_HIP_ERR_ALLOC : RPVG_HIP_ERR_RUNTIME;
    }
    lock.unlock();
    scope.reset(new HostScope("batch_upload_segments: wait for the kernels"));
    const int rc = finishBatch(b.get(), "rpvg_hip_batch_upload_segments", [h_first_bad]() {
        if (*h_first_bad == ~0ull) return RPVG_HIP_OK;
        const unsigned long long k = *h_first_bad >> 8, kind = *h_first_bad & 0xff;
        setError("rpvg_hip_batch_upload_segments: cluster %llu of the batch: %s", k,
                 kind == kSegmentBadNoise ? "a row has a noise probability outside (0, 1]"
                 : kind == kSegmentBadPath ? "a row or a haplotype column refers to a path outside its cluster"
                                           : "inconsistent row, group, entry or source offsets");
        return RPVG_HIP_ERR_INVALID;
    });
    if (rc != RPVG_HIP_OK) return rc;
    if (columns) b->has_source_columns = true;
    *batch_out = b.release();
    return RPVG_HIP_OK;
}

void rpvg_hip_batch_free(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch) {
    if (!batch) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mutex);
        (void) hipSetDevice(ctx->device);
        (void) hipStreamSynchronize(ctx->stream);
        delete batch;
    } else {
        delete batch;
    }
}

// Inspection (tests and tools): the row side of a complete batch as the estimators read it.
int rpvg_hip_batch_rows_sizes(const rpvg_hip_batch * batch, uint64_t * num_rows_out, uint64_t * num_entries_out) {
    RPVG_REQUIRE(batch && num_rows_out && num_entries_out, "rpvg_hip_batch_rows_sizes: NULL argument");
    *num_rows_out = batch->num_rows;
    *num_entries_out = batch->num_entries;
    return RPVG_HIP_OK;
}

int rpvg_hip_batch_rows_get(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint64_t * row_ent_off_out, double * row_count_out, double * row_noise_out,
                            uint32_t * ent_path_out, double * ent_prob_out) {
    RPVG_REQUIRE(ctx && batch && row_ent_off_out && (batch->num_rows == 0 || (row_count_out && row_noise_out)) && (batch->num_entries == 0 || (ent_path_out && ent_prob_out)),
                 "rpvg_hip_batch_rows_get: NULL argument");
    RPVG_REQUIRE(batch->upload == nullptr, "rpvg_hip_batch_rows_get: the upload of the batch has not finished");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(batch->row_ent_off.download(row_ent_off_out, ctx->stream));
    RPVG_HIP_CHECK(batch->row_count.download(row_count_out, ctx->stream));
    RPVG_HIP_CHECK(batch->row_noise.download(row_noise_out, ctx->stream));
    RPVG_HIP_CHECK(batch->ent_path.download(ent_path_out, ctx->stream));
    RPVG_HIP_CHECK(batch->ent_prob.download(ent_prob_out, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

}  // extern "C"
