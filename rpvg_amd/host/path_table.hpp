// The PathInfo of every path of a run as the flat table of include/rpvg_index.h (rpvg_path_table), and the way back from
// the name groups the device formed (rpvg_name_groups_view) to the collapsed PathInfo of every cluster
// (src/main.cpp:909-951).  Plain host code: needs no engine.
#ifndef RPVG_AMD_PATH_TABLE_HPP
#define RPVG_AMD_PATH_TABLE_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rpvg_index.h"
#include "path_cluster_estimates.hpp"

namespace rpvg_amd {

class PathTable {

    public:

        // One entry per GLOBAL path id.  Equal names get equal ids (a hash map; ids in order of first appearance); the
        // source ids of the paths are laid back to back.  A table none of whose paths has source ids has no source arrays.
        static PathTable fromPathInfos(const std::vector<PathInfo> & path_infos);

        // The arrays of a flat table taken as they are (source ids in the caller's order, nothing sorted or merged); path i is
        // called names[i], or "n<name_id>" when names is empty and the table has name ids.
        static PathTable fromArrays(const rpvg_path_table & flat, const std::vector<std::string> & names_in = std::vector<std::string>());

        // Identifies the contents: set when a table is made, kept by copies (the arrays cannot be changed afterwards).
        uint64_t id() const { return table_id; }

        uint32_t numPaths() const { return group_id.size(); }
        bool hasSources() const { return has_sources; }
        const std::string & name(const uint32_t path_id) const { return names.at(path_id); }

        // valid while the table lives
        rpvg_path_table view() const;

        // The collapsed paths of every cluster from the groups view; every name is that of the group's first member.
        std::vector<std::vector<PathInfo> > collapsedPaths(const rpvg_name_groups_view & groups) const;

        const std::vector<uint32_t> & groupIds() const { return group_id; }
        const std::vector<uint32_t> & sourceCounts() const { return source_count; }
        const std::vector<uint32_t> & sourceIds() const { return source_id; }
        const std::vector<uint64_t> & sourceOffsets() const { return source_off; }
        const std::vector<uint32_t> & nameIds() const { return name_id; }
        const std::vector<uint32_t> & lengths() const { return length; }
        const std::vector<double> & effectiveLengths() const { return effective_length; }

    private:

        static uint64_t nextId();

        std::vector<uint32_t> group_id, source_count, source_id, name_id, length;
        std::vector<uint64_t> source_off;
        std::vector<double> effective_length;

        uint64_t table_id = 0;
        bool has_sources = false;
        std::vector<std::string> names;
};

}

#endif
