#include "gibbs_samples_table.hpp"

namespace rpvg_amd {

GibbsSamplesTable::GibbsSamplesTable(std::shared_ptr<HipEngine> engine_in, const ClusterEstimatesList & estimates_list, const uint32_t num_gibbs_samples_in) : hip_engine(std::move(engine_in)), num_gibbs_samples(num_gibbs_samples_in), table(nullptr), table_view(), has_view(false) {

    for (auto & cluster_estimates: estimates_list) {

        flat_gibbs.add(cluster_estimates.first, cluster_estimates.second);
    }

    const rpvg_gibbs_flat flat = flat_gibbs.view(num_gibbs_samples);
    HipEngine::check(rpvg_hip_gibbs_table_build(hip_engine->ctx(), &flat, &table), "rpvg_hip_gibbs_table_build");
}

GibbsSamplesTable::~GibbsSamplesTable() {

    rpvg_hip_gibbs_table_free(hip_engine->ctx(), table);
}

const rpvg_gibbs_table_view & GibbsSamplesTable::view() {

    if (!has_view) {

        HipEngine::check(rpvg_hip_gibbs_table_view(hip_engine->ctx(), table, &table_view), "rpvg_hip_gibbs_table_view");
        has_view = true;
    }

    return table_view;
}

std::vector<double> GibbsSamplesTable::rows(const uint64_t first, const uint64_t count) {

    std::vector<double> out(count * static_cast<uint64_t>(num_gibbs_samples), 0.0);
    HipEngine::check(rpvg_hip_gibbs_table_rows(hip_engine->ctx(), table, first, count, out.data()), "rpvg_hip_gibbs_table_rows");

    return out;
}

}
