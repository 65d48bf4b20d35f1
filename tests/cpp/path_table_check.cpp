// The host side of the path table (rpvg_amd/host/path_table.hpp) without a device: PathInfos -> the flat table of
// include/rpvg_index.h, and a groups view -> the collapsed PathInfos of every cluster.  Stand-alone; built with
// -fsanitize=address,undefined by tests/test_path_table_model.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "path_table.hpp"

using rpvg_amd::PathInfo;
using rpvg_amd::PathTable;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static PathInfo path(const std::string & name, const uint32_t group_id, const uint32_t source_count, const std::vector<uint32_t> & source_ids, const uint32_t length, const double effective_length) {

    PathInfo info(name);
    info.group_id = group_id;
    info.source_count = source_count;
    info.source_ids.insert(source_ids.begin(), source_ids.end());
    info.length = length;
    info.effective_length = effective_length;

    return info;
}

static void checkRoundTrip(const std::vector<PathInfo> & infos, const PathTable & table) {

    const rpvg_path_table view = table.view();
    CHECK(view.num_paths == infos.size());
    CHECK(table.sourceOffsets().size() == infos.size() + 1 && table.sourceOffsets().front() == 0 && table.sourceOffsets().back() == table.sourceIds().size());

    uint64_t num_sources = 0;

    for (size_t i = 0; i < infos.size(); ++i) {

        CHECK(view.group_id[i] == infos[i].group_id && view.source_count[i] == infos[i].source_count);
        CHECK(view.length[i] == infos[i].length && view.effective_length[i] == infos[i].effective_length);
        CHECK(table.name(i) == infos[i].name);
        CHECK(table.sourceOffsets()[i + 1] - table.sourceOffsets()[i] == infos[i].source_ids.size());

        size_t k = 0;

        for (auto & id: infos[i].source_ids) {

            CHECK(table.sourceIds()[table.sourceOffsets()[i] + k] == id);
            ++k;
        }

        num_sources += infos[i].source_ids.size();

        for (size_t j = 0; j < infos.size(); ++j) {

            CHECK((view.name_id[i] == view.name_id[j]) == (infos[i].name == infos[j].name));
        }
    }

    CHECK(view.num_sources == num_sources);
    CHECK((view.source_off != nullptr) == (num_sources > 0) && (view.source_id != nullptr) == (num_sources > 0));
}

int main() {

    // no paths: one offset, no source arrays in the view
    PathTable table = PathTable::fromPathInfos({});
    CHECK(table.numPaths() == 0 && table.sourceOffsets().size() == 1 && !table.hasSources() && table.view().source_off == nullptr);

    // the hand case of tests/path_table_model.py: names a b a c b
    std::vector<PathInfo> infos = {path("a", 9, 1, {}, 1, 1.5), path("b", 8, 1, {}, 10, 4.0), path("a", 9, 1, {}, 2, 2.5), path("c", 7, 2, {}, 7, 3.0), path("b", 8, 3, {}, 20, 8.0)};
    table = PathTable::fromPathInfos(infos);
    checkRoundTrip(infos, table);
    CHECK((table.nameIds() == std::vector<uint32_t>{0, 1, 0, 2, 1}));
    CHECK(!table.hasSources());

    // the flat arrays taken as they are: ids in the caller's order, repeated ids kept; copies share the identity, new tables do not
    {
        const std::vector<uint32_t> g = {1, 2}, sc = {1, 1}, len = {5, 6}, ids = {9, 3, 3}, nid = {40, 40};
        const std::vector<uint64_t> off = {0, 3, 3};
        const std::vector<double> eff = {1.0, 2.0};
        rpvg_path_table flat = {};
        flat.num_paths = 2;
        flat.num_sources = 3;
        flat.group_id = g.data();
        flat.source_count = sc.data();
        flat.source_off = off.data();
        flat.source_id = ids.data();
        flat.name_id = nid.data();
        flat.length = len.data();
        flat.effective_length = eff.data();
        const PathTable as_given = PathTable::fromArrays(flat);
        CHECK((as_given.sourceIds() == ids) && (as_given.sourceOffsets() == off) && as_given.hasSources());
        CHECK(as_given.name(0) == "n40" && as_given.name(1) == "n40" && as_given.view().num_sources == 3);
        const PathTable copy = as_given;
        CHECK(copy.id() == as_given.id() && PathTable::fromArrays(flat).id() != as_given.id() && as_given.id() != table.id());
        flat.name_id = nullptr;
        CHECK(PathTable::fromArrays(flat).view().name_id == nullptr && PathTable::fromArrays(flat, {"x", "y"}).name(1) == "y");
    }

    // the groups view the device returns for one cluster over the five paths
    const std::vector<uint32_t> path_group = {0, 1, 0, 2, 1}, first_path = {0, 1, 3}, name_id = {0, 1, 2}, group_id = {9, 8, 7}, source_count = {2, 4, 2}, length = {2, 18, 7};
    const std::vector<uint64_t> cluster_group_off = {0, 3};
    const std::vector<double> effective_length = {2.0, 7.0, 3.0};
    rpvg_name_groups_view groups = {};
    groups.num_clusters = 1;
    groups.num_paths = 5;
    groups.path_group = path_group.data();
    groups.cluster_group_off = cluster_group_off.data();
    groups.group_first_path = first_path.data();
    groups.group_name_id = name_id.data();
    groups.group_group_id = group_id.data();
    groups.group_source_count = source_count.data();
    groups.group_length = length.data();
    groups.group_effective_length = effective_length.data();

    auto collapsed = table.collapsedPaths(groups);
    CHECK(collapsed.size() == 1 && collapsed[0].size() == 3);
    CHECK(collapsed[0][0].name == "a" && collapsed[0][1].name == "b" && collapsed[0][2].name == "c");
    CHECK(collapsed[0][1].group_id == 8 && collapsed[0][1].source_count == 4 && collapsed[0][1].length == 18 && collapsed[0][1].effective_length == 7.0);
    CHECK(collapsed[0][2].source_ids.empty());

    // two clusters, the second without groups; a view of another table is refused
    const std::vector<uint64_t> two_off = {0, 3, 3};
    groups.num_clusters = 2;
    groups.cluster_group_off = two_off.data();
    collapsed = table.collapsedPaths(groups);
    CHECK(collapsed.size() == 2 && collapsed[0].size() == 3 && collapsed[1].empty());

    bool thrown = false;
    groups.num_paths = 4;

    try {
        table.collapsedPaths(groups);
    } catch (const std::invalid_argument &) {
        thrown = true;
    }

    CHECK(thrown);

    // a first member outside the table is caught, not read
    groups.num_paths = 5;
    const std::vector<uint32_t> bad_first = {0, 1, 5};
    groups.group_first_path = bad_first.data();
    thrown = false;

    try {
        table.collapsedPaths(groups);
    } catch (const std::out_of_range &) {
        thrown = true;
    }

    CHECK(thrown);

    // random tables: paths without, with one and with hundreds of source ids, repeated names
    std::mt19937 rng(11);

    for (int round = 0; round < 30; ++round) {

        infos.clear();
        const int num_paths = rng() % 120;

        for (int i = 0; i < num_paths; ++i) {

            std::vector<uint32_t> ids;
            const int num_ids = (round % 3 == 0) ? 0 : ((rng() % 10 == 0) ? 300 : rng() % 3);

            for (int k = 0; k < num_ids; ++k) {

                ids.push_back(rng() % 5000);
            }

            infos.emplace_back(path("t" + std::to_string(rng() % 40), rng() % 9, 1 + rng() % 50, ids, rng() % 9000, (rng() % 100000) / 7.0));
        }

        table = PathTable::fromPathInfos(infos);
        checkRoundTrip(infos, table);
    }

    std::printf("ok\n");
    return 0;
}
