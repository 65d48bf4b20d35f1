// The host plan of the group matrix build (group_build.hip): what is refused, which of the five build kernels every matrix of a
// call gets, the per-matrix arrays and the (matrix, chunk) item lists the kernels read, the totals behind the allocations and
// the grid, block and dynamic LDS of every launch — a pure computation on sizes, plain C++17, no HIP types, no getenv, so that a
// CPU test reaches every decision (tests/cpp/group_build_plan_check.cpp).  buildGroups uploads the plan and launches what it
// says.  The constants and tileRows() are the kernels' too: host and device share one definition.
#ifndef RPVG_GROUP_BUILD_PLAN_HPP
#define RPVG_GROUP_BUILD_PLAN_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_group_build {

// Rows per LDS tile for a matrix with G columns: the tile (G x rows doubles) must fit kTileDoubles; a power of two
// of at least 16 rows (128-byte runs per column when the tile is written out).  0 = too wide: global-memory kernel.
constexpr uint32_t kTileDoubles = 4096;  // 32 KB: four workgroups per CU (64 KB tiles, two per CU, were 11 % slower: the rows hang on dependent loads)

RPVG_PLAN_FN uint32_t tileRows(const uint32_t G) {
    if (G * 16u > kTileDoubles) return 0;
    uint32_t rows = 256;
    while (rows * G > kTileDoubles) rows >>= 1;
    return rows;
}

constexpr uint32_t kMaskMaxColumns = 1024;  // (wider matrices, and sets of more than kMaskMaxWords words: the list kernels)
constexpr uint32_t kMaskMaxWords = 16;
constexpr uint32_t kMaskRows = 64;          // rows of an item of the mask, word and single-path kernels: a wave
constexpr uint32_t kWordMaxColumns = 64;
constexpr uint32_t kListRows = 256;         // rows of an item of groupsBuildKernel and zeroWideMatricesKernel: a workgroup

constexpr uint32_t kTileLdsBytes = (kTileDoubles + 256) * sizeof(double);  // the tile with its odd stride (Rc + 1 rows per column)
constexpr uint32_t kPartitionThreads = 1024;

// restated (group_build.hip asserts that they are common.hpp's and rpvg_hip.h's)
constexpr uint32_t kCollapseMaxMatrices = 1u << 20;
constexpr int kStatusOk = 0, kStatusInvalid = -3;

// where the columns of the matrices come from
enum class Columns {
    Lists,        // the caller's: group_path_off per column, group_path
    Sources,      // the batch's source (haplotype) columns, gathered on the device: group_path_off per MATRIX, the first list entry of its columns
    SinglePaths,  // column c = path c of the cluster, written on the device: group_path_off per matrix, as above
};

// What the environment may change (group_build.hip reads it, per call; the plan never does)
struct BuildKnobs {
    bool masks = true;   // RPVG_HIP_BUILD_MASKS >= 1: groupsBuildMaskKernel where it applies
    bool words = true;   // RPVG_HIP_BUILD_MASKS >= 2: groupsBuildWordKernel where it applies
    bool direct = true;  // RPVG_HIP_NO_DIRECT_BUILD unset: groupsBuildSinglePathKernel for single paths as they are
};

struct Launch {
    uint32_t grid = 0, block = 0, lds_bytes = 0;  // grid 0: not launched
};

// the work items of one route: chunk c of matrix m = its rows [c x rows per item, (c + 1) x rows per item)
struct Items {
    std::vector<uint32_t> matrix, chunk;
    size_t size() const { return matrix.size(); }
    bool empty() const { return matrix.empty(); }
    void add(const uint32_t m, const uint64_t rows, const uint32_t rows_per_item) {
        for (uint64_t c = 0; c * rows_per_item < rows; ++c) {
            matrix.push_back(m);
            chunk.push_back(static_cast<uint32_t>(c));
        }
    }
};

struct GroupBuildPlan {
    int status = kStatusOk;  // kStatusInvalid: refused, `message` says why and nothing else below holds
    std::string message;
    uint32_t M = 0;
    // per matrix
    std::vector<uint64_t> val_off, row_off, row0, rows, inc_off, num_paths;
    std::vector<uint64_t> mask_off, word_off;  // ~0: a matrix of other kernels
    std::vector<uint32_t> cols, max_col_paths, paths, cluster;  // longest column list (capped at 2^32 - 1), paths and cluster as the matrices object keeps them
    uint64_t val_total = 0, row_total = 0, inc_total = 0, mask_total = 0, word_total = 0;
    // Which kernel builds a matrix: single-path columns as they are groupsBuildSinglePathKernel (`direct`: every matrix of the
    // call, through the items of the mask kernel and no masks); up to kWordMaxColumns columns groupsBuildWordKernel; up to
    // kMaskMaxColumns columns and kMaskMaxWords words of paths groupsBuildMaskKernel; the rest the list kernels — through an LDS
    // tile where tileRows() finds one, in global memory otherwise.
    Items list_items, tile_items, mask_items, word_items;
    bool lists_needed = false;  // the path -> columns lists of the tile / global-memory kernels
    bool direct = false;
    uint64_t num_columns = 0, num_incidences = 0;
    double h2d_bytes = 0;
    // the launches, in their order on the stream
    Launch gather_columns, single_path_columns;  // the columns made on the device
    Launch zero_wide, partition;
    Launch build_single_paths, column_masks, build_masks;
    Launch path_words, build_words;
    Launch incidence_count, incidence_fill;
    Launch build_tiles, build_lists;
};

namespace detail {
template <typename... Args>
inline GroupBuildPlan refuse(const char * format, Args... args) {
    GroupBuildPlan p;
    char text[512];
    std::snprintf(text, sizeof(text), format, args...);
    p.status = kStatusInvalid;
    p.message = text;
    return p;
}
}  // namespace detail

// Sizes and offsets only, O(M) (and O(columns) for the caller's lists: their longest).  h_cluster_row_off / h_cluster_path_off:
// the batch's [num_clusters + 1] offsets; h_src_max_col_paths: [num_clusters], read for Columns::Sources only; cluster [M],
// group_off [M + 1], group_path_off (see Columns): the spec's.  Nothing is read when M is 0.
inline GroupBuildPlan planGroupBuild(const uint64_t * h_cluster_row_off, const uint64_t * h_cluster_path_off, const uint32_t * h_src_max_col_paths,
                                     const uint32_t num_clusters, const uint32_t M, const uint32_t * cluster, const uint64_t * group_off,
                                     const uint64_t * group_path_off, const bool normalise, const bool collapse, const Columns kind,
                                     const BuildKnobs & knobs) {
    GroupBuildPlan p;
    p.M = M;
    p.direct = kind == Columns::SinglePaths && !normalise && knobs.direct;
    for (auto * v : {&p.val_off, &p.row_off, &p.row0, &p.rows, &p.inc_off, &p.num_paths}) v->assign(M, 0);
    p.mask_off.assign(M, ~0ull);
    p.word_off.assign(M, ~0ull);
    p.cols.assign(M, 0);
    for (uint32_t m = 0; m < M; ++m) {
        const uint32_t k = cluster[m];
        if (k >= num_clusters) return detail::refuse("rpvg_hip_groups_build: matrix %u refers to cluster %u of %u", m, k, num_clusters);
        const uint64_t R = h_cluster_row_off[k + 1] - h_cluster_row_off[k];
        const uint64_t N = h_cluster_path_off[k + 1] - h_cluster_path_off[k];
        const uint64_t g0 = group_off[m], g1 = group_off[m + 1];
        if (R > 0xffffffffull) {
            return detail::refuse("rpvg_hip_groups_build: matrix %u has %llu rows (limit 2^32 - 1)", m, static_cast<unsigned long long>(R));
        }
        if (R == 0 || g1 <= g0) return detail::refuse("rpvg_hip_groups_build: matrix %u has no rows or no columns", m);
        p.rows[m] = R;
        p.cols[m] = static_cast<uint32_t>(g1 - g0);
        uint64_t longest = 0;
        if (kind == Columns::Sources) longest = h_src_max_col_paths[k];
        else if (kind == Columns::SinglePaths) longest = 1;
        else for (uint64_t c = g0; c < g1; ++c) longest = std::max<uint64_t>(longest, group_path_off[c + 1] - group_path_off[c]);
        p.max_col_paths.push_back(static_cast<uint32_t>(std::min<uint64_t>(longest, 0xffffffffu)));
        p.paths.push_back(static_cast<uint32_t>(N));
        p.cluster.push_back(k);
        p.row0[m] = h_cluster_row_off[k];
        p.num_paths[m] = N;
        p.val_off[m] = p.val_total;
        p.row_off[m] = p.row_total;
        p.inc_off[m] = p.inc_total;
        p.val_total += R * (g1 - g0);
        p.row_total += R;
        p.inc_total += N + 1;
        const uint64_t mask_words = (N + 63) / 64;
        if (p.direct) {
            p.mask_items.add(m, R, kMaskRows);
        } else if (knobs.words && p.cols[m] <= kWordMaxColumns) {
            p.word_off[m] = p.word_total;
            p.word_total += N;
            p.word_items.add(m, R, kMaskRows);
        } else if (knobs.masks && p.cols[m] <= kMaskMaxColumns && mask_words <= kMaskMaxWords) {
            p.mask_off[m] = p.mask_total;
            p.mask_total += p.cols[m] * mask_words;
            p.mask_items.add(m, R, kMaskRows);
        } else {
            p.lists_needed = true;
            const uint32_t tile_rows = tileRows(p.cols[m]);
            if (tile_rows) p.tile_items.add(m, R, tile_rows);
            else p.list_items.add(m, R, kListRows);
        }
    }
    // the row collapse keeps the matrix of a row in 20 bits of its sort key and rows in 31 (row_collapse.hip)
    if (collapse && (M >= kCollapseMaxMatrices || p.row_total > 0x7fffffffull)) {
        return detail::refuse("rpvg_hip_groups_build: the row collapse takes up to %u matrices and 2^31 - 1 rows per call (got %u matrices, %llu rows): "
                              "build the matrices of a batch in several calls", kCollapseMaxMatrices - 1, M, static_cast<unsigned long long>(p.row_total));
    }
    if (M == 0) return p;
    p.num_columns = group_off[M];
    p.num_incidences = kind == Columns::Lists ? group_path_off[p.num_columns] : group_path_off[M];
    p.h2d_bytes = static_cast<double>(M * 60 + p.num_columns * 8 + p.num_incidences * 4 + (p.list_items.size() + p.tile_items.size()) * 8);

    const auto items = [](const Items & list) { return static_cast<uint32_t>(list.size()); };
    const auto waves = [](const Items & list) { return list.empty() ? Launch{} : Launch{(static_cast<uint32_t>(list.size()) + 3) / 4, 256, 0}; };
    const uint32_t col_blocks = static_cast<uint32_t>((p.num_columns + 255) / 256);
    const Launch per_column{col_blocks, 256, 0}, per_matrix{M, 256, 0};
    if (kind == Columns::Sources) p.gather_columns = per_matrix;
    if (kind == Columns::SinglePaths) p.single_path_columns = per_matrix;
    if (!p.list_items.empty()) p.zero_wide = p.build_lists = Launch{items(p.list_items), kListRows, 0};
    p.partition = Launch{M, kPartitionThreads, 0};
    if (p.direct) {
        p.build_single_paths = waves(p.mask_items);
    } else if (!p.mask_items.empty()) {
        p.column_masks = per_column;
        p.build_masks = waves(p.mask_items);
    }
    if (!p.word_items.empty()) {
        p.path_words = per_column;
        p.build_words = waves(p.word_items);
    }
    if (p.lists_needed) p.incidence_count = p.incidence_fill = per_column;
    if (!p.tile_items.empty()) p.build_tiles = Launch{items(p.tile_items), 256, kTileLdsBytes};
    return p;
}

}  // namespace rpvg_group_build

#endif
