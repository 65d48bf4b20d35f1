#include "path_table.hpp"

#include <atomic>
#include <stdexcept>
#include <unordered_map>

namespace rpvg_amd {

uint64_t PathTable::nextId() {

    static std::atomic<uint64_t> last_id(0);
    return ++last_id;
}

PathTable PathTable::fromArrays(const rpvg_path_table & flat, const std::vector<std::string> & names_in) {

    const size_t num_paths = flat.num_paths;

    if (!names_in.empty() && names_in.size() != num_paths) {

        throw std::invalid_argument("one name per path");
    }

    if ((flat.source_off == nullptr) != (flat.source_id == nullptr) && flat.num_sources > 0) {

        throw std::invalid_argument("source_off and source_id go together");
    }

    PathTable table;
    table.table_id = nextId();
    table.group_id.assign(flat.group_id, flat.group_id + num_paths);
    table.source_count.assign(flat.source_count, flat.source_count + num_paths);
    table.length.assign(flat.length, flat.length + num_paths);
    table.effective_length.assign(flat.effective_length, flat.effective_length + num_paths);
    table.source_off.assign(1, 0);

    if (flat.source_off) {

        table.source_off.assign(flat.source_off, flat.source_off + num_paths + 1);
        table.source_id.assign(flat.source_id, flat.source_id + flat.num_sources);
        table.has_sources = flat.num_sources > 0;

    } else {

        table.source_off.assign(num_paths + 1, 0);
    }

    if (flat.name_id) {

        table.name_id.assign(flat.name_id, flat.name_id + num_paths);
    }

    table.names = names_in;

    if (table.names.empty()) {

        table.names.reserve(num_paths);

        for (size_t i = 0; i < num_paths; ++i) {

            table.names.emplace_back(flat.name_id ? "n" + std::to_string(flat.name_id[i]) : std::string());
        }
    }

    return table;
}

PathTable PathTable::fromPathInfos(const std::vector<PathInfo> & path_infos) {

    if (path_infos.size() >= 0x7fffffffull) {

        throw std::invalid_argument("too many paths for one table");
    }

    PathTable table;
    table.table_id = nextId();

    const size_t num_paths = path_infos.size();
    table.group_id.reserve(num_paths);
    table.source_count.reserve(num_paths);
    table.name_id.reserve(num_paths);
    table.length.reserve(num_paths);
    table.effective_length.reserve(num_paths);
    table.names.reserve(num_paths);
    table.source_off.reserve(num_paths + 1);
    table.source_off.emplace_back(0);

    std::unordered_map<std::string, uint32_t> name_index;
    name_index.reserve(num_paths);

    for (auto & info: path_infos) {

        table.group_id.emplace_back(info.group_id);
        table.source_count.emplace_back(info.source_count);
        table.length.emplace_back(info.length);
        table.effective_length.emplace_back(info.effective_length);
        table.names.emplace_back(info.name);
        table.name_id.emplace_back(name_index.emplace(info.name, name_index.size()).first->second);

        table.source_id.insert(table.source_id.end(), info.source_ids.begin(), info.source_ids.end());
        table.source_off.emplace_back(table.source_id.size());
    }

    table.has_sources = !table.source_id.empty();

    return table;
}

rpvg_path_table PathTable::view() const {

    rpvg_path_table table_view = {};
    table_view.num_paths = numPaths();
    table_view.num_sources = has_sources ? source_id.size() : 0;
    table_view.group_id = group_id.data();
    table_view.source_count = source_count.data();
    table_view.source_off = has_sources ? source_off.data() : nullptr;
    table_view.source_id = has_sources ? source_id.data() : nullptr;
    table_view.name_id = name_id.empty() && numPaths() > 0 ? nullptr : name_id.data();
    table_view.length = length.data();
    table_view.effective_length = effective_length.data();

    return table_view;
}

std::vector<std::vector<PathInfo> > PathTable::collapsedPaths(const rpvg_name_groups_view & groups) const {

    if (groups.num_paths != numPaths()) {

        throw std::invalid_argument("the groups are not those of this table");
    }

    std::vector<std::vector<PathInfo> > collapsed_paths(groups.num_clusters);

    for (uint32_t i = 0; i < groups.num_clusters; ++i) {

        if (groups.cluster_group_off[i] > groups.cluster_group_off[i + 1]) {

            throw std::invalid_argument("descending group offsets");
        }

        collapsed_paths[i].reserve(groups.cluster_group_off[i + 1] - groups.cluster_group_off[i]);

        for (uint64_t j = groups.cluster_group_off[i]; j < groups.cluster_group_off[i + 1]; ++j) {

            PathInfo info(names.at(groups.group_first_path[j]));
            info.group_id = groups.group_group_id[j];
            info.source_count = groups.group_source_count[j];
            info.length = groups.group_length[j];
            info.effective_length = groups.group_effective_length[j];

            collapsed_paths[i].emplace_back(std::move(info));
        }
    }

    return collapsed_paths;
}

}
