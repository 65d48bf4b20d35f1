// The forms a host batch arrives in (include/rpvg_batch.h), decided once: which of its alternative arrays rpvg_hip_batch_upload
// copies, the sizes they imply, the bytes the copies of the row side move — and every read of the caller's arrays that happens
// before the copy (the argument checks, the O(K) walk of the cluster offsets, the clusters' entry offsets).  Plain C++17 without
// HIP, so that a CPU test reaches every form under the sanitizers (tests/cpp/batch_forms_check.cpp).  batch_upload.hip copies
// and launches what the plan says; both halves of an upload read the one plan (rpvg_hip_batch::UploadInProgress::forms).
#ifndef RPVG_BATCH_FORMS_HPP
#define RPVG_BATCH_FORMS_HPP

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/rpvg_batch.h"

namespace rpvg_batch_forms {

// one of the two long offset arrays: n + 1 offsets of 64 or 32 bits, or n counts of one byte (summed up on the device)
enum class OffsetForm { Wide64, Narrow32, Counts8 };

inline uint64_t offsetArrayBytes(const OffsetForm form, const uint64_t n) {
    return form == OffsetForm::Counts8 ? n : (n + 1) * (form == OffsetForm::Narrow32 ? 4 : 8);
}

struct BatchForms {
    uint32_t K = 0;
    uint64_t R = 0, G = 0, NNZ = 0, P = 0;
    // each offset array is taken in 32 bits INSTEAD of 64 on its own; the counts come for both or not at all
    OffsetForm row_offsets = OffsetForm::Wide64, group_offsets = OffsetForm::Wide64;
    bool noise16 = false;  // row_noise16 + row_noise_table instead of row_noise
    bool count8 = false;   // row_count8 + the listed rows instead of row_count
    bool path16 = false;   // path_idx16 instead of path_idx
    uint64_t row_copy_bytes = 0;  // what the copies of the row side move (the path side counts its own: path_sources.hip)
    bool counts() const { return row_offsets == OffsetForm::Counts8; }
};

constexpr size_t kMessageChars = 256;

// the two long offset arrays of a host batch, in whichever width the caller wrote them; of a batch that came with counts only, by
// adding them up (the wording of an error message: nothing else reads them here then)
inline uint64_t rowGroupOffset(const rpvg_cluster_batch * hb, const uint64_t r) {
    if (hb->row_grp_off32) return hb->row_grp_off32[r];
    if (hb->row_grp_off) return hb->row_grp_off[r];
    uint64_t sum = 0;
    for (uint64_t i = 0; i < r; ++i) sum += hb->row_grp_count8[i];
    return sum;
}
inline uint64_t groupEntryOffset(const rpvg_cluster_batch * hb, const uint64_t g) {
    if (hb->grp_idx_off32) return hb->grp_idx_off32[g];
    if (hb->grp_idx_off) return hb->grp_idx_off[g];
    uint64_t sum = 0;
    for (uint64_t i = 0; i < g; ++i) sum += hb->grp_idx_count8[i];
    return sum;
}

// The plan of an upload of `hb`.  false: an argument error, worded in `message` (kMessageChars).  cluster_ent_off [K + 1]: the
// entry offset of every cluster's first row — with the counts zeros, the device brings them behind its sums.  Nothing here has
// been validated yet beyond the cluster offsets (the rows are, on the device, behind their copy): the group index of a cluster's
// first row is clamped to G as rowMetaKernel clamps it, so that a caller's wild row_grp_off entry reads inside grp_idx_off; the
// device's verdict refuses such a batch afterwards.
inline bool planBatchForms(const rpvg_cluster_batch * hb, BatchForms * forms, std::vector<uint64_t> * cluster_ent_off, char * message) {
#define RPVG_FORMS_REQUIRE(cond, ...)                            \
    do {                                                         \
        if (!(cond)) {                                           \
            std::snprintf(message, kMessageChars, __VA_ARGS__);  \
            return false;                                        \
        }                                                        \
    } while (0)
    BatchForms f;
    const uint32_t K = f.K = hb->num_clusters;
    RPVG_FORMS_REQUIRE(hb->cluster_row_off && hb->cluster_path_off, "rpvg_hip_batch_upload: cluster offsets are NULL");
    const uint64_t R = f.R = hb->cluster_row_off[K];
    f.P = hb->cluster_path_off[K];
    const bool counts = R > 0 && hb->row_grp_count8 != nullptr && hb->grp_idx_count8 != nullptr;  // one byte per row and group instead of the offsets
    RPVG_FORMS_REQUIRE(R == 0 || ((hb->row_count || hb->row_count8) && (hb->row_noise || (hb->row_noise16 && hb->row_noise_table)) && (counts || ((hb->row_grp_off || hb->row_grp_off32) && (hb->grp_idx_off || hb->grp_idx_off32)))),
                       "rpvg_hip_batch_upload: row arrays are NULL");
    RPVG_FORMS_REQUIRE(!counts || (hb->num_groups < 0xffffffffull && hb->num_entries < 0xffffffffull && hb->num_groups > 0),
                       "rpvg_hip_batch_upload: counts of one byte come with their totals (num_groups, num_entries: below 2^32 - 1)");
    const uint64_t G = f.G = counts ? hb->num_groups : (R ? rowGroupOffset(hb, R) : 0);
    const uint64_t NNZ = f.NNZ = counts ? hb->num_entries : (G ? groupEntryOffset(hb, G) : 0);
    RPVG_FORMS_REQUIRE(G == 0 || hb->grp_prob, "rpvg_hip_batch_upload: grp_prob is NULL");
    RPVG_FORMS_REQUIRE(NNZ == 0 || hb->path_idx || hb->path_idx16, "rpvg_hip_batch_upload: path_idx is NULL");
    RPVG_FORMS_REQUIRE(!hb->row_count8 || hb->num_row_count_escapes == 0 || (hb->row_count_escape_row && hb->row_count_escape_count),
                       "rpvg_hip_batch_upload: row_count8 comes with the list of the rows whose count does not fit a byte");
    // validation: the cluster offsets here (O(K)); the rows and entries on the device, behind their copy (validateRowsKernel)
    for (uint32_t k = 0; k < K; ++k) {
        RPVG_FORMS_REQUIRE(hb->cluster_row_off[k] <= hb->cluster_row_off[k + 1] && hb->cluster_path_off[k] <= hb->cluster_path_off[k + 1],
                           "rpvg_hip_batch_upload: cluster %u has decreasing offsets", k);
        RPVG_FORMS_REQUIRE(hb->cluster_path_off[k + 1] - hb->cluster_path_off[k] <= 0x7fffffffu, "rpvg_hip_batch_upload: cluster %u has too many paths", k);
    }
    RPVG_FORMS_REQUIRE(hb->cluster_row_off[0] == 0, "rpvg_hip_batch_upload: the first cluster does not start at row 0");
#undef RPVG_FORMS_REQUIRE

    f.row_offsets = counts ? OffsetForm::Counts8 : (hb->row_grp_off32 ? OffsetForm::Narrow32 : OffsetForm::Wide64);
    f.group_offsets = counts ? OffsetForm::Counts8 : (hb->grp_idx_off32 ? OffsetForm::Narrow32 : OffsetForm::Wide64);
    f.noise16 = hb->row_noise16 != nullptr;
    f.count8 = hb->row_count8 != nullptr;
    f.path16 = hb->path_idx16 != nullptr;
    f.row_copy_bytes = (static_cast<uint64_t>(K) + 1) * 16 + (f.noise16 ? R * 2 + 8 * hb->num_row_noise_values : R * 8) +
                       (f.count8 ? R + 8 * hb->num_row_count_escapes : 4 * R) + offsetArrayBytes(f.row_offsets, R) + offsetArrayBytes(f.group_offsets, G) +
                       G * 8 + NNZ * (f.path16 ? 2 : 4);

    cluster_ent_off->assign(static_cast<size_t>(K) + 1, 0);
    for (uint32_t k = 0; k <= K && R > 0 && !counts; ++k) {
        // (cluster_row_off[k] <= R: the walk above)
        (*cluster_ent_off)[k] = groupEntryOffset(hb, std::min(rowGroupOffset(hb, hb->cluster_row_off[k]), G));
    }
    *forms = f;
    return true;
}

}  // namespace rpvg_batch_forms

#endif
