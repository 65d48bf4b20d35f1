#include "estimates_table.hpp"

namespace rpvg_amd {

EstimatesTable::EstimatesTable(std::shared_ptr<HipEngine> engine_in, const std::vector<PathClusterEstimates> & estimates, const uint32_t ploidy) : hip_engine(std::move(engine_in)), table(nullptr), table_view(), has_view(false) {

    for (auto & cluster_estimates: estimates) {

        flat_estimates.add(cluster_estimates);
    }

    build(ploidy);
}

EstimatesTable::EstimatesTable(std::shared_ptr<HipEngine> engine_in, const rpvg_estimates_flat & flat, const uint32_t ploidy) : hip_engine(std::move(engine_in)), table(nullptr), table_view(), has_view(false) {

    if (flat.on_device) {

        throw EngineError("EstimatesTable takes host arrays: a device-resident view goes to rpvg_hip_estimates_table_build");
    }

    flat_estimates = FlatEstimates::copyOf(flat);
    build(ploidy);
}

EstimatesTable::EstimatesTable(std::shared_ptr<HipEngine> engine_in, const ResidentEstimates & resident_in, const uint32_t ploidy) : hip_engine(std::move(engine_in)), resident(&resident_in), table(nullptr), table_view(), has_view(false) {

    if (resident_in.empty()) {

        throw EngineError("EstimatesTable: the resident estimates are empty");
    }

    const rpvg_estimates_flat flat = resident_in.view();
    HipEngine::check(rpvg_hip_estimates_table_build(hip_engine->ctx(), &flat, ploidy, &table), "rpvg_hip_estimates_table_build");
}

void ResidentEstimates::adopt(std::shared_ptr<HipEngine> engine_in, rpvg_hip_flat_estimates * handle_in) {

    reset();
    kept_block_bytes.clear();
    hip_engine = std::move(engine_in);
    handle_ = handle_in;
}

void ResidentEstimates::reset() {

    if (handle_) {

        rpvg_hip_flat_estimates_free(hip_engine->ctx(), handle_);
        handle_ = nullptr;
    }
}

rpvg_estimates_flat ResidentEstimates::view() const {

    rpvg_estimates_flat flat = {};
    HipEngine::check(rpvg_hip_flat_estimates_view(handle_, &flat), "rpvg_hip_flat_estimates_view");
    return flat;
}

rpvg_estimates_flat ResidentEstimates::hostView() const {

    rpvg_estimates_flat flat = {};
    HipEngine::check(rpvg_hip_flat_estimates_get(hip_engine->ctx(), handle_, &flat), "rpvg_hip_flat_estimates_get");
    return flat;
}

EstimatesTable::~EstimatesTable() {

    rpvg_hip_estimates_table_free(hip_engine->ctx(), table);
}

void EstimatesTable::build(const uint32_t ploidy) {

    const rpvg_estimates_flat flat = flat_estimates.view();
    HipEngine::check(rpvg_hip_estimates_table_build(hip_engine->ctx(), &flat, ploidy, &table), "rpvg_hip_estimates_table_build");
}

void EstimatesTable::tpm(const double denominator) {

    has_view = false;
    HipEngine::check(rpvg_hip_estimates_table_tpm(hip_engine->ctx(), table, denominator), "rpvg_hip_estimates_table_tpm");
}

const rpvg_estimates_table_view & EstimatesTable::view() {

    if (!has_view) {

        HipEngine::check(rpvg_hip_estimates_table_view(hip_engine->ctx(), table, &table_view), "rpvg_hip_estimates_table_view");
        has_view = true;
    }

    return table_view;
}

}
