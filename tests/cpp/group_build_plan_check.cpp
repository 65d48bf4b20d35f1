// The plan of the group matrix build (rpvg_amd/csrc/group_build_plan.hpp) against the arithmetic buildGroups carried before it
// had a plan, written out here literally (two booleans for the kind of the columns, three for the switches): refusals, the
// per-matrix arrays, the route and the items of every matrix, the sentinels, the totals, every launch and the upload's byte
// figure — over a grid of shapes, at the edges of every formula, for the three kinds and every setting of the switches.  Then
// what the kernels rely on, checked on its own: every matrix in exactly one route, its items the chunks 0 .. ceil(R / rows per
// item) - 1 in order, the offsets disjoint, ordered and adding up.  Plain C++17; built with -fsanitize=address,undefined.
// Prints "ok".
#include "group_build_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace rpvg_group_build;

struct Batch {  // cluster k: rows[k] rows, paths[k] paths, the longest of its source columns
    std::vector<uint64_t> row_off{0}, path_off{0};
    std::vector<uint32_t> src_max;
    uint32_t add(const uint64_t rows, const uint64_t paths) {
        row_off.push_back(row_off.back() + rows);
        path_off.push_back(path_off.back() + paths);
        src_max.push_back(static_cast<uint32_t>(1 + (rows + 3 * paths) % 7));
        return static_cast<uint32_t>(src_max.size() - 1);
    }
    uint32_t clusters() const { return static_cast<uint32_t>(src_max.size()); }
};

struct Spec {
    std::vector<uint32_t> cluster;
    std::vector<uint64_t> group_off{0};
    std::vector<uint64_t> group_path_off{0};  // Lists: per column; the other kinds: per matrix
    uint32_t M() const { return static_cast<uint32_t>(cluster.size()); }
};

// matrix of G columns on cluster k; the caller's column c lists 1 + (c + k) % 5 paths, a column of the batch's 3 on average
static void addMatrix(Spec & s, const Columns kind, const uint32_t k, const uint64_t G) {
    s.cluster.push_back(k);
    const uint64_t g0 = s.group_off.back();
    s.group_off.push_back(g0 + G);
    if (kind == Columns::Lists) {
        for (uint64_t c = 0; c < G; ++c) s.group_path_off.push_back(s.group_path_off.back() + 1 + (c + k) % 5);
    } else {
        s.group_path_off.push_back(s.group_path_off.back() + (kind == Columns::SinglePaths ? G : 3 * G));
    }
}

static GroupBuildPlan planOf(const Batch & b, const Spec & s, const bool normalise, const bool collapse, const Columns kind, const BuildKnobs & knobs) {
    return planGroupBuild(b.row_off.data(), b.path_off.data(), b.src_max.data(), b.clusters(), s.M(), s.cluster.data(), s.group_off.data(),
                          s.group_path_off.data(), normalise, collapse, kind, knobs);
}

static uint32_t oldTileRows(const uint32_t G) {
    if (G * 16u > 4096) return 0;
    uint32_t rows = 256;
    while (rows * G > 4096) rows >>= 1;
    return rows;
}

static void requireLaunch(const Launch got, const uint32_t grid, const uint32_t block, const uint32_t lds = 0) {
    REQUIRE(got.grid == grid);
    REQUIRE(got.block == (grid ? block : 0u));
    REQUIRE(got.lds_bytes == (grid ? lds : 0u));
}

static void requireRefused(const GroupBuildPlan & p, const std::string & text) {
    REQUIRE(p.status == -3);
    if (p.message != text) std::fprintf(stderr, "got:      %s\nexpected: %s\n", p.message.c_str(), text.c_str());
    REQUIRE(p.message == text);
}

// what buildGroups computed, statement for statement
// (returns the plan it checked)
static GroupBuildPlan checkAgainstFormulas(const Batch & batch, const Spec & spec, const bool normalise, const bool collapse, const Columns kind, const BuildKnobs & knobs) {
    const GroupBuildPlan p = planOf(batch, spec, normalise, collapse, kind, knobs);
    const bool from_sources = kind == Columns::Sources, single_paths = kind == Columns::SinglePaths;
    const bool build_masks = knobs.masks, build_words = knobs.words;
    const uint32_t M = spec.M();
    const uint32_t num_clusters = batch.clusters();
    char text[512];

    std::vector<uint64_t> val_off(M), row_off(M), row0(M), rows(M), inc_off(M), num_paths(M);
    std::vector<uint32_t> cols(M), item_matrix, item_chunk, tile_matrix, tile_chunk, mask_matrix, mask_chunk, word_matrix, word_chunk;
    std::vector<uint32_t> h_max_col_paths, h_num_paths, h_cluster;
    std::vector<uint64_t> mask_off(M, ~0ull), word_off(M, ~0ull);
    uint64_t val_total = 0, row_total = 0, inc_total = 0, mask_total = 0, word_total = 0;
    bool lists_needed = false;
    const bool direct = single_paths && !normalise && knobs.direct;
    for (uint32_t m = 0; m < M; ++m) {
        const uint32_t k = spec.cluster[m];
        if (k >= num_clusters) {
            std::snprintf(text, sizeof(text), "rpvg_hip_groups_build: matrix %u refers to cluster %u of %u", m, k, num_clusters);
            return requireRefused(p, text), p;
        }
        const uint64_t R = batch.row_off[k + 1] - batch.row_off[k];
        const uint64_t N = batch.path_off[k + 1] - batch.path_off[k];
        const uint64_t g0 = spec.group_off[m], g1 = spec.group_off[m + 1];
        if (R > 0xffffffffull) {
            std::snprintf(text, sizeof(text), "rpvg_hip_groups_build: matrix %u has %llu rows (limit 2^32 - 1)", m, static_cast<unsigned long long>(R));
            return requireRefused(p, text), p;
        }
        if (R == 0 || g1 <= g0) {
            std::snprintf(text, sizeof(text), "rpvg_hip_groups_build: matrix %u has no rows or no columns", m);
            return requireRefused(p, text), p;
        }
        rows[m] = R;
        cols[m] = static_cast<uint32_t>(g1 - g0);
        {
            uint64_t longest = 0;
            if (from_sources) longest = batch.src_max[k];
            else if (single_paths) longest = 1;
            else for (uint64_t c = g0; c < g1; ++c) longest = std::max<uint64_t>(longest, spec.group_path_off[c + 1] - spec.group_path_off[c]);
            h_max_col_paths.push_back(static_cast<uint32_t>(std::min<uint64_t>(longest, 0xffffffffu)));
            h_num_paths.push_back(static_cast<uint32_t>(N));
            h_cluster.push_back(k);
        }
        row0[m] = batch.row_off[k];
        num_paths[m] = N;
        val_off[m] = val_total;
        row_off[m] = row_total;
        inc_off[m] = inc_total;
        val_total += R * (g1 - g0);
        row_total += R;
        inc_total += N + 1;
        const uint64_t mask_words = (N + 63) / 64;
        if (direct) {
            for (uint64_t c = 0; c * 64 < R; ++c) {
                mask_matrix.push_back(m);
                mask_chunk.push_back(static_cast<uint32_t>(c));
            }
            continue;
        }
        if (build_words && cols[m] <= 64) {
            word_off[m] = word_total;
            word_total += N;
            for (uint64_t c = 0; c * 64 < R; ++c) {
                word_matrix.push_back(m);
                word_chunk.push_back(static_cast<uint32_t>(c));
            }
            continue;
        }
        if (build_masks && cols[m] <= 1024 && mask_words <= 16) {
            mask_off[m] = mask_total;
            mask_total += cols[m] * mask_words;
            for (uint64_t c = 0; c * 64 < R; ++c) {
                mask_matrix.push_back(m);
                mask_chunk.push_back(static_cast<uint32_t>(c));
            }
            continue;
        }
        lists_needed = true;
        const uint32_t tile_rows = oldTileRows(cols[m]);
        if (tile_rows) {
            for (uint64_t c = 0; c * tile_rows < R; ++c) {
                tile_matrix.push_back(m);
                tile_chunk.push_back(static_cast<uint32_t>(c));
            }
        } else {
            for (uint64_t c = 0; c * 256 < R; ++c) {
                item_matrix.push_back(m);
                item_chunk.push_back(static_cast<uint32_t>(c));
            }
        }
    }
    if (collapse && (M >= (1u << 20) || row_total > 0x7fffffffull)) {
        std::snprintf(text, sizeof(text),
                      "rpvg_hip_groups_build: the row collapse takes up to %u matrices and 2^31 - 1 rows per call (got %u matrices, %llu rows): "
                      "build the matrices of a batch in several calls", (1u << 20) - 1, M, static_cast<unsigned long long>(row_total));
        return requireRefused(p, text), p;
    }
    REQUIRE(p.status == 0 && p.message.empty() && p.M == M);
    REQUIRE(p.val_off == val_off && p.row_off == row_off && p.row0 == row0 && p.rows == rows && p.cols == cols && p.inc_off == inc_off);
    REQUIRE(p.num_paths == num_paths && p.mask_off == mask_off && p.word_off == word_off);
    REQUIRE(p.max_col_paths == h_max_col_paths && p.paths == h_num_paths && p.cluster == h_cluster);
    REQUIRE(p.val_total == val_total && p.row_total == row_total && p.inc_total == inc_total && p.mask_total == mask_total && p.word_total == word_total);
    REQUIRE(p.list_items.matrix == item_matrix && p.list_items.chunk == item_chunk && p.tile_items.matrix == tile_matrix && p.tile_items.chunk == tile_chunk);
    REQUIRE(p.mask_items.matrix == mask_matrix && p.mask_items.chunk == mask_chunk && p.word_items.matrix == word_matrix && p.word_items.chunk == word_chunk);
    REQUIRE(p.lists_needed == lists_needed && p.direct == direct);
    if (M == 0) {
        for (const Launch & l : {p.gather_columns, p.single_path_columns, p.zero_wide, p.partition, p.build_single_paths, p.column_masks, p.build_masks,
                                 p.path_words, p.build_words, p.incidence_count, p.incidence_fill, p.build_tiles, p.build_lists}) requireLaunch(l, 0, 0);
        REQUIRE(p.num_columns == 0 && p.num_incidences == 0 && p.h2d_bytes == 0);
        return p;
    }
    const uint64_t num_columns = spec.group_off[M];
    const uint64_t num_incidences = (from_sources || single_paths) ? spec.group_path_off[M] : spec.group_path_off[num_columns];
    REQUIRE(p.num_columns == num_columns && p.num_incidences == num_incidences);
    REQUIRE(p.h2d_bytes == static_cast<double>(M * 60 + num_columns * 8 + num_incidences * 4 + (item_matrix.size() + tile_matrix.size()) * 8));

    // the launches: dim3(grid), dim3(block), dynamic LDS of every <<< >>> of the function, in its order
    const uint32_t col_blocks = static_cast<uint32_t>((num_columns + 255) / 256);
    requireLaunch(p.gather_columns, from_sources ? M : 0, 256);
    requireLaunch(p.single_path_columns, single_paths ? M : 0, 256);
    requireLaunch(p.zero_wide, static_cast<uint32_t>(item_matrix.size()), 256);
    requireLaunch(p.partition, M, 1024);
    const uint32_t mask_items = static_cast<uint32_t>(mask_matrix.size()), word_items = static_cast<uint32_t>(word_matrix.size());
    requireLaunch(p.build_single_paths, !mask_matrix.empty() && direct ? (mask_items + 3) / 4 : 0, 256);
    requireLaunch(p.column_masks, !mask_matrix.empty() && !direct ? col_blocks : 0, 256);
    requireLaunch(p.build_masks, !mask_matrix.empty() && !direct ? (mask_items + 3) / 4 : 0, 256);
    requireLaunch(p.path_words, !word_matrix.empty() ? col_blocks : 0, 256);
    requireLaunch(p.build_words, !word_matrix.empty() ? (word_items + 3) / 4 : 0, 256);
    requireLaunch(p.incidence_count, lists_needed ? col_blocks : 0, 256);
    requireLaunch(p.incidence_fill, lists_needed ? col_blocks : 0, 256);
    requireLaunch(p.build_tiles, static_cast<uint32_t>(tile_matrix.size()), 256, (4096 + 256) * sizeof(double));
    requireLaunch(p.build_lists, static_cast<uint32_t>(item_matrix.size()), 256);
    return p;
}

// what the kernels rely on, from the plan alone
static void checkShape(const GroupBuildPlan & p, const BuildKnobs & knobs) {
    REQUIRE(p.status == 0);
    const uint32_t M = p.M;
    struct Route {
        const Items * items;
        uint32_t rows_per_item;  // 0: the matrix's tileRows
    };
    const Route routes[4] = {{&p.list_items, 256}, {&p.tile_items, 0}, {&p.mask_items, 64}, {&p.word_items, 64}};
    std::vector<int> route_of(M, -1);
    for (int r = 0; r < 4; ++r) {
        const Items & it = *routes[r].items;
        REQUIRE(it.matrix.size() == it.chunk.size());
        size_t at = 0;
        uint32_t last = 0;
        while (at < it.size()) {  // runs of one matrix each, matrices ascending, chunks 0 .. ceil(R / rows per item) - 1
            const uint32_t m = it.matrix[at];
            REQUIRE(m < M && route_of[m] == -1 && (at == 0 || m > last));
            route_of[m] = r;
            last = m;
            const uint32_t per_item = routes[r].rows_per_item ? routes[r].rows_per_item : tileRows(p.cols[m]);
            REQUIRE(per_item > 0);
            const uint64_t chunks = (p.rows[m] + per_item - 1) / per_item;
            for (uint64_t c = 0; c < chunks; ++c, ++at) REQUIRE(at < it.size() && it.matrix[at] == m && it.chunk[at] == c);
        }
    }
    uint64_t values = 0, rows = 0, incidences = 0, masks = 0, words = 0;
    bool lists = false;
    for (uint32_t m = 0; m < M; ++m) {
        REQUIRE(route_of[m] >= 0);  // exactly one: no run twice (above), none missing
        const uint64_t N = p.num_paths[m], G = p.cols[m], set_words = (N + 63) / 64;
        // the route, from the widths alone
        const int expected = p.direct ? 2 : knobs.words && G <= 64 ? 3 : knobs.masks && G <= 1024 && N <= 1024 ? 2 : G <= 256 ? 1 : 0;
        REQUIRE(route_of[m] == expected);
        lists |= expected < 2;
        // offsets: each matrix begins where the one before ends
        REQUIRE(p.val_off[m] == values && p.row_off[m] == rows && p.inc_off[m] == incidences);
        values += p.rows[m] * G;
        rows += p.rows[m];
        incidences += N + 1;
        // the sentinels: ~0 exactly for the matrices of other routes (and for every matrix of a direct build: it has no masks)
        const bool has_masks = route_of[m] == 2 && !p.direct, has_words = route_of[m] == 3;
        REQUIRE(p.mask_off[m] == (has_masks ? masks : ~0ull) && p.word_off[m] == (has_words ? words : ~0ull));
        if (has_masks) masks += G * set_words;
        if (has_words) words += N;
        REQUIRE(p.paths[m] == N && p.max_col_paths[m] >= 1);
    }
    REQUIRE(values == p.val_total && rows == p.row_total && incidences == p.inc_total && masks == p.mask_total && words == p.word_total);
    REQUIRE(lists == p.lists_needed);
    REQUIRE(p.zero_wide.grid == p.list_items.size() && p.build_lists.grid == p.list_items.size() && p.build_tiles.grid == p.tile_items.size());
    REQUIRE(4ull * p.build_words.grid >= p.word_items.size() && 4ull * (p.build_masks.grid + p.build_single_paths.grid) >= p.mask_items.size());
    REQUIRE(p.build_masks.grid == 0 || p.build_single_paths.grid == 0);
    REQUIRE(p.partition.grid == M && (M == 0 || p.partition.block == 1024));
}

static std::vector<BuildKnobs> allKnobs() {
    std::vector<BuildKnobs> all;
    for (int bits = 0; bits < 8; ++bits) {
        BuildKnobs k;
        k.masks = bits & 1;
        k.words = bits & 2;
        k.direct = bits & 4;
        all.push_back(k);
    }
    return all;
}

static void checkEverySetting(const Batch & batch, const Spec (&specs)[3]) {
    const Columns kinds[3] = {Columns::Lists, Columns::Sources, Columns::SinglePaths};
    for (int kind = 0; kind < 3; ++kind) {
        for (const BuildKnobs & knobs : allKnobs()) {
            for (int flags = 0; flags < 4; ++flags) {
                const bool normalise = flags & 1, collapse = flags & 2;
                const GroupBuildPlan p = checkAgainstFormulas(batch, specs[kind], normalise, collapse, kinds[kind], knobs);
                if (p.status == 0) checkShape(p, knobs);
            }
        }
    }
}

int main() {
    REQUIRE(kTileDoubles == 4096 && kMaskMaxColumns == 1024 && kMaskMaxWords == 16 && kMaskRows == 64 && kWordMaxColumns == 64 && kListRows == 256);
    const uint32_t tile_at[][2] = {{1, 256}, {16, 256}, {17, 128}, {32, 128}, {33, 64}, {64, 64}, {65, 32}, {128, 32}, {129, 16}, {256, 16}, {257, 0}, {1025, 0}};
    for (const auto & e : tile_at) REQUIRE(tileRows(e[0]) == e[1] && oldTileRows(e[0]) == e[1]);

    // ---- the grid: every (rows, paths) a cluster, every width a matrix on it ----------------------------------------------------------
    const std::vector<uint64_t> Gs = {1, 64, 65, 256, 257, 1024, 1025};
    const std::vector<uint64_t> Ns = {1, 64, 65, 256, 257, 1024, 1025};  // (single paths: as many columns as paths, hence the widths again)
    const std::vector<uint64_t> Rs = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513};  // tileRows: 16, 32, 64, 128, 256
    Batch batch;
    Spec whole[3];  // one call with everything, per kind
    const Columns kinds[3] = {Columns::Lists, Columns::Sources, Columns::SinglePaths};
    for (const uint64_t R : Rs) {
        for (const uint64_t N : Ns) {
            const uint32_t k = batch.add(R, N);
            for (int kind = 0; kind < 3; ++kind) {
                if (kinds[kind] == Columns::SinglePaths) addMatrix(whole[kind], kinds[kind], k, N);
                else for (const uint64_t G : Gs) addMatrix(whole[kind], kinds[kind], k, G);
            }
        }
    }
    checkEverySetting(batch, whole);
    // a matrix in a call of its own (M = 1) on every cluster, the widths in turn, and no matrix at all (M = 0)
    for (uint32_t k = 0; k < batch.clusters(); ++k) {
        const uint64_t N = batch.path_off[k + 1] - batch.path_off[k];
        Spec one[3];
        for (int kind = 0; kind < 3; ++kind) addMatrix(one[kind], kinds[kind], k, kinds[kind] == Columns::SinglePaths ? N : Gs[(k / Ns.size() + k) % Gs.size()]);
        checkEverySetting(batch, one);
    }
    const Spec none[3] = {};
    checkEverySetting(batch, none);
    {
        const GroupBuildPlan p = planGroupBuild(nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, true, true, Columns::Lists, BuildKnobs());
        REQUIRE(p.status == 0 && p.M == 0 && p.rows.empty() && p.partition.grid == 0);  // (nothing is read)
    }
    // a list that repeats and reorders clusters
    {
        Spec mixed[3];
        const uint32_t K = batch.clusters();
        const uint32_t order[] = {K - 1, 3, 3, 0, 40, 7, 3, K - 1, 21, 0, 100, 57, 58, 57};
        uint32_t turn = 0;
        for (const uint32_t k : order) {
            const uint64_t N = batch.path_off[k + 1] - batch.path_off[k];
            for (int kind = 0; kind < 3; ++kind) addMatrix(mixed[kind], kinds[kind], k, kinds[kind] == Columns::SinglePaths ? N : Gs[turn % Gs.size()]);
            ++turn;
        }
        checkEverySetting(batch, mixed);
    }

    // ---- the routes at their edges, one by one (default switches; normalised, so nothing is direct) -------------------------------------
    const BuildKnobs defaults;
    const auto routeOf = [&](const uint64_t R, const uint64_t N, const uint64_t G, const BuildKnobs & knobs) {
        Batch b;
        Spec s;
        addMatrix(s, Columns::Sources, b.add(R, N), G);
        const GroupBuildPlan p = planOf(b, s, true, false, Columns::Sources, knobs);
        REQUIRE(p.status == 0);
        checkShape(p, knobs);
        return !p.word_items.empty() ? 'w' : !p.mask_items.empty() ? 'm' : !p.tile_items.empty() ? 't' : 'l';
    };
    REQUIRE(routeOf(100, 2000, 64, defaults) == 'w' && routeOf(100, 64, 65, defaults) == 'm');
    REQUIRE(routeOf(100, 1024, 1024, defaults) == 'm' && routeOf(100, 1024, 1025, defaults) == 'l' && routeOf(100, 1025, 1024, defaults) == 'l');
    REQUIRE(routeOf(100, 1025, 256, defaults) == 't' && routeOf(100, 1025, 257, defaults) == 'l' && routeOf(100, 1025, 65, defaults) == 't');
    BuildKnobs no_words, lists_only;
    no_words.words = false;
    lists_only.words = lists_only.masks = false;
    REQUIRE(routeOf(100, 64, 64, no_words) == 'm' && routeOf(100, 1025, 64, no_words) == 't');
    REQUIRE(routeOf(100, 64, 1, lists_only) == 't' && routeOf(100, 64, 256, lists_only) == 't' && routeOf(100, 64, 257, lists_only) == 'l');
    // single paths as they are: the direct kernel on the mask route's items, for every width; normalised, or switched off: the general routes
    {
        Batch b;
        Spec s;
        for (const uint64_t N : Ns) addMatrix(s, Columns::SinglePaths, b.add(130, N), N);
        BuildKnobs general;
        general.direct = false;
        const GroupBuildPlan direct = planOf(b, s, false, false, Columns::SinglePaths, defaults);
        REQUIRE(direct.direct && direct.mask_items.size() == 3 * Ns.size() && direct.word_items.empty() && direct.tile_items.empty() && direct.list_items.empty());
        REQUIRE(!direct.lists_needed && direct.mask_total == 0 && direct.word_total == 0 && direct.build_masks.grid == 0 && direct.column_masks.grid == 0);
        requireLaunch(direct.build_single_paths, (3 * static_cast<uint32_t>(Ns.size()) + 3) / 4, 256);
        for (const GroupBuildPlan & p : {planOf(b, s, true, false, Columns::SinglePaths, defaults), planOf(b, s, false, false, Columns::SinglePaths, general)}) {
            REQUIRE(!p.direct && p.build_single_paths.grid == 0 && !p.word_items.empty() && !p.mask_items.empty() && !p.list_items.empty() && p.lists_needed);
        }
    }
    // the longest column: the caller's lists are measured, capped at 32 bits
    {
        Batch b;
        Spec s;
        s.cluster = {b.add(5, 9)};
        s.group_off = {0, 3};
        s.group_path_off = {0, 2, 2 + (1ull << 32) + 5, 2 + (1ull << 32) + 6};
        const GroupBuildPlan p = planOf(b, s, true, false, Columns::Lists, defaults);
        REQUIRE(p.status == 0 && p.max_col_paths[0] == 0xffffffffu && p.num_incidences == 2 + (1ull << 32) + 6);
        s.group_path_off = {0, 2, 9, 10};
        REQUIRE(planOf(b, s, true, false, Columns::Lists, defaults).max_col_paths[0] == 7);
    }

    // ---- the refusals: code and text, at the limit and one beside it -------------------------------------------------------------------
    {
        Batch b;
        const uint32_t small = b.add(10, 4), empty = b.add(0, 4), most = b.add(0xffffffffull, 4), too_many = b.add(1ull << 32, 4);
        const uint32_t half = b.add(0x7fffffffull, 4), one = b.add(1, 4);
        const auto call = [&](const std::vector<uint32_t> & clusters, const std::vector<uint64_t> & widths, const bool collapse, const bool with_formulas = true) {
            Spec s;
            for (size_t m = 0; m < clusters.size(); ++m) {
                s.cluster.push_back(clusters[m]);
                s.group_off.push_back(s.group_off.back() + widths[m]);
                s.group_path_off.push_back(s.group_path_off.back() + widths[m]);
            }
            if (with_formulas) checkAgainstFormulas(b, s, true, collapse, Columns::Sources, defaults);
            return planOf(b, s, true, collapse, Columns::Sources, defaults);
        };
        const uint32_t K = b.clusters();
        requireRefused(call({small, K}, {2, 2}, false), "rpvg_hip_groups_build: matrix 1 refers to cluster " + std::to_string(K) + " of " + std::to_string(K));
        requireRefused(call({0xffffffffu}, {2}, false), "rpvg_hip_groups_build: matrix 0 refers to cluster 4294967295 of " + std::to_string(K));
        REQUIRE(call({small, K - 1}, {2, 2}, false).status == 0);
        requireRefused(call({small, small, too_many}, {2, 2, 2}, false), "rpvg_hip_groups_build: matrix 2 has 4294967296 rows (limit 2^32 - 1)");
        requireRefused(call({small, empty}, {2, 2}, false), "rpvg_hip_groups_build: matrix 1 has no rows or no columns");
        requireRefused(call({small, small}, {2, 0}, false), "rpvg_hip_groups_build: matrix 1 has no rows or no columns");
        {
            Spec backwards;  // (offsets that go back: no columns either)
            backwards.cluster = {small};
            backwards.group_off = {5, 3};
            backwards.group_path_off = {0, 0};
            requireRefused(planOf(b, backwards, true, false, Columns::Sources, defaults), "rpvg_hip_groups_build: matrix 0 has no rows or no columns");
        }
        // (the first fault of the first faulty matrix is the one named)
        requireRefused(call({empty, K}, {2, 2}, false), "rpvg_hip_groups_build: matrix 0 has no rows or no columns");
        requireRefused(call({K, empty}, {2, 2}, false), "rpvg_hip_groups_build: matrix 0 refers to cluster " + std::to_string(K) + " of " + std::to_string(K));
        // rows: 2^32 - 1 of one matrix without the collapse, 2^31 - 1 of all with it (wide matrices on the list route: the fewest items)
        // (millions of items: the plan alone, without its model next to it)
        {
            const GroupBuildPlan largest = call({most}, {1025}, false, false);
            REQUIRE(largest.status == 0 && largest.list_items.size() == (1u << 24) && largest.list_items.chunk.back() == (1u << 24) - 1);
        }
        REQUIRE(call({half}, {1025}, true, false).status == 0);
        requireRefused(call({half, one}, {1025, 1025}, true, false),
                       "rpvg_hip_groups_build: the row collapse takes up to 1048575 matrices and 2^31 - 1 rows per call (got 2 matrices, 2147483648 rows): "
                       "build the matrices of a batch in several calls");
        // matrices: 2^20 - 1 with the collapse
        std::vector<uint32_t> many((1u << 20) - 1, one);
        std::vector<uint64_t> widths(1u << 20, 1);
        const GroupBuildPlan fits = call(many, widths, true);
        REQUIRE(fits.status == 0 && fits.M == (1u << 20) - 1 && fits.word_items.size() == fits.M);
        many.push_back(one);
        requireRefused(call(many, widths, true),
                       "rpvg_hip_groups_build: the row collapse takes up to 1048575 matrices and 2^31 - 1 rows per call (got 1048576 matrices, 1048576 rows): "
                       "build the matrices of a batch in several calls");
        REQUIRE(call(many, widths, false).status == 0);
    }
    std::printf("ok\n");
    return 0;
}
