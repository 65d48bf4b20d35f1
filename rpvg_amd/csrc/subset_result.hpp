// The result object of the three nested calls (subset_em.hip, subset_full.hip, subset_independent.hip): everything in one page-locked
// block, and — when the context asks for it (rpvg_hip_subset_em_keep_device) — the device block the copy was made from, which
// estimates_gather.hip reads where it lies (rpvg_hip_subset_em_part).
#pragma once

#include "common.hpp"
#include "subset_full_plan.hpp"

struct rpvg_hip_subset_em {
    uint32_t num_matrices = 0;
    uint64_t num_subsets = 0;
    void * block = nullptr;
    rpvg_hip_subset_em_view view{};
    rpvg_hip_subset_em_sets_view sets_view{};  // rpvg_hip_nested_full_subset_em's (has_sets)
    bool has_sets = false;
    // rpvg_hip_nested_independent_subset_em's (subset_independent.hip); its units are clusters.  draws: kept for the tests
    // (rpvg_hip_independent_spec::keep_draws), unit k's at draw_off[k], [slot][transcript]
    rpvg_hip_subset_em_independent_view independent_view{};
    bool has_independent = false;
    std::vector<uint32_t> draws;
    std::vector<uint64_t> draw_off;
    // the packed block on the device (kept.ptr != nullptr: kept), laid out by kept_layout like `block`; it has the size of the call's
    // capacities, not of the result.  kept_merged: the merged sets are in it.  kept_width: 0 the diploid form, else the group size.
    rpvg_hip_detail::DeviceBuffer<unsigned char> kept;
    rpvg_subset_full::PackedLayout kept_layout{};
    uint64_t kept_slots = 0;
    uint32_t kept_width = 0;
    bool kept_merged = false;
    // takes the block over from the call (which has waited for its stream): the call's buffer is left empty
    void keep(rpvg_hip_detail::DeviceBuffer<unsigned char> & packed, const rpvg_subset_full::PackedLayout & layout, const uint64_t slots,
              const uint32_t width, const bool merged) {
        if (!packed.ptr || packed.borrowed) return;
        kept.release();
        kept.ptr = packed.ptr;
        kept.count = packed.count;
        packed.ptr = nullptr;
        packed.count = 0;
        kept_layout = layout;
        kept_slots = slots;
        kept_width = width;
        kept_merged = merged;
    }
    ~rpvg_hip_subset_em() {
        if (block) rpvg_hip_detail::pinnedFree(block);
    }
};
