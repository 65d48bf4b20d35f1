// The plan of the read rows (rpvg_amd/csrc/rows_plan.hpp) against the arithmetic rpvg_hip_alignments_upload, mergeRows and
// rpvg_hip_read_rows_build carried before they had a plan, written out here literally: every refusal of the upload (code and
// text, one fault at a time, the last element of an array as the faulty one, two faults in one batch), the cluster of every
// read, the output columns, the split of the reads, the byte figure; the lists and the launch sequence of the sort for cluster
// sizes at every edge, alone and mixed; the launch shapes of the row kernels and the pack.  Then the one thing no formula
// shows: the planned launches, replayed on the host with the kernels' guards restated, sort every cluster of a call — a
// permutation of its input, in order — on reversed, random and all-equal keys.  Plain C++17; built with
// -fsanitize=address,undefined.  Prints "ok".
#include "rows_plan.hpp"

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

using namespace rpvg_rows_plan;

// ---- a small valid batch ----------------------------------------------------------------------------------------------------
// Cluster 0: 3 paths, reads of 1 and 3 entries; cluster 1: 20 paths, no reads; cluster 2: 40 paths, reads of 1, 15, 16, 17 and
// 33 entries.  A read of up to 20 entries has one alignment (paths 0 .. e - 1), a longer one a second (paths 20 .. e - 1).
// Collapsing: paths 2 g and 2 g + 1 of a cluster form its group g.
struct HostBatch {
    std::vector<uint64_t> cluster_read_off{0}, cluster_path_off{0}, cluster_group_off{0}, read_align_off{0}, align_path_off{0};
    std::vector<double> eff_len;
    std::vector<uint32_t> source_count, path_group, read_count, path_idx;
    std::vector<uint8_t> mapq;
    std::vector<int32_t> noise_score, score;
    std::vector<uint16_t> align_length, frag_length;
    bool collapse = false;

    void addCluster(const uint32_t paths, const std::vector<uint32_t> & read_entries) {
        for (uint32_t q = 0; q < paths; ++q) {
            eff_len.push_back(100.0 + q);
            source_count.push_back(1 + q % 3);
            path_group.push_back(q / 2);
        }
        cluster_path_off.push_back(cluster_path_off.back() + paths);
        cluster_group_off.push_back(cluster_group_off.back() + (paths + 1) / 2);
        for (const uint32_t e : read_entries) {
            read_count.push_back(1 + e % 4);
            mapq.push_back(30);
            noise_score.push_back(-7);
            for (uint32_t first = 0; first < e; first += 20) {
                score.push_back(100);
                align_length.push_back(90);
                frag_length.push_back(250);
                for (uint32_t q = first; q < std::min(e, first + 20); ++q) path_idx.push_back(q);
                align_path_off.push_back(path_idx.size());
            }
            read_align_off.push_back(score.size());
        }
        cluster_read_off.push_back(cluster_read_off.back() + read_entries.size());
    }

    rpvg_alignment_batch view() const {
        rpvg_alignment_batch b{};
        b.num_clusters = static_cast<uint32_t>(cluster_read_off.size() - 1);
        b.cluster_read_off = cluster_read_off.data();
        b.cluster_path_off = cluster_path_off.data();
        b.path_effective_length = eff_len.data();
        b.path_source_count = source_count.data();
        b.path_group = collapse ? path_group.data() : nullptr;
        b.cluster_group_off = collapse ? cluster_group_off.data() : nullptr;
        b.read_count = read_count.data();
        b.read_min_mapq = mapq.data();
        b.read_noise_score = noise_score.data();
        b.read_align_off = read_align_off.data();
        b.align_score_sum = score.data();
        b.align_length = align_length.data();
        b.align_frag_length = frag_length.data();
        b.align_path_off = align_path_off.data();
        b.align_path_idx = path_idx.data();
        return b;
    }
};

static HostBatch validBatch(const bool collapse) {
    HostBatch h;
    h.collapse = collapse;
    h.addCluster(3, {1, 3});
    h.addCluster(20, {});
    h.addCluster(40, {1, 15, 16, 17, 33});
    return h;
}

static void refused(const rpvg_alignment_batch & b, const char * text) {
    const AlignmentBatchPlan p = planAlignmentBatch(b);
    if (p.status != -3 || p.message != text) {
        std::fprintf(stderr, "expected refusal \"%s\", got status %d \"%s\"\n", text, p.status, p.message.c_str());
        std::exit(1);
    }
}

static const char * const kDescending = "rpvg_hip_alignments_upload: descending cluster offsets";
static const char * const kGroup = "rpvg_hip_alignments_upload: a path group outside its cluster or a zero source count";
static const char * const kNoAlignments = "rpvg_hip_alignments_upload: a read without alignments";
static const char * const kNoiseScore = "rpvg_hip_alignments_upload: a read with a positive noise score";
static const char * const kEmptyAlignment = "rpvg_hip_alignments_upload: an alignment without paths or with zero length";
static const char * const kAscending = "rpvg_hip_alignments_upload: path indices of an alignment must be ascending and inside the cluster";

static void checkRefusals() {
    REQUIRE(kStatusOk == 0 && kStatusInvalid == -3);
    for (const bool collapse : {false, true}) {
        REQUIRE(planAlignmentBatch(validBatch(collapse).view()).status == 0);
        // 1: offsets of reads, of paths; one that also leaves the arrays (nothing outside them may be read: the sanitizer watches)
        { HostBatch h = validBatch(collapse); h.cluster_read_off[1] = 3; refused(h.view(), kDescending); }
        { HostBatch h = validBatch(collapse); h.cluster_path_off[2] = 2; refused(h.view(), kDescending); }
        { HostBatch h = validBatch(collapse); h.cluster_read_off[1] = 1000; refused(h.view(), kDescending); }
        { HostBatch h = validBatch(collapse); h.cluster_path_off[1] = 1000; refused(h.view(), kDescending); }
        // 3: the last read has no alignments (its own go to the read before it, which stays valid)
        { HostBatch h = validBatch(collapse); h.read_align_off[6] = h.read_align_off[7]; refused(h.view(), kNoAlignments); }
        { HostBatch h = validBatch(collapse); h.read_align_off[1] = 0; refused(h.view(), kNoAlignments); }
        { HostBatch h = validBatch(collapse); h.read_align_off[1] = 1000; refused(h.view(), kNoAlignments); }
        // 4
        { HostBatch h = validBatch(collapse); h.noise_score.back() = 1; refused(h.view(), kNoiseScore); }
        { HostBatch h = validBatch(collapse); h.noise_score[0] = 5; refused(h.view(), kNoiseScore); }
        { HostBatch h = validBatch(collapse); h.noise_score.back() = 0; REQUIRE(planAlignmentBatch(h.view()).status == 0); }
        // 5: the last alignment without paths (the one before it takes them: 0 .. 32, ascending), or of length zero
        { HostBatch h = validBatch(collapse); h.align_path_off[h.align_path_off.size() - 2] = h.align_path_off.back(); refused(h.view(), kEmptyAlignment); }
        { HostBatch h = validBatch(collapse); h.align_length.back() = 0; refused(h.view(), kEmptyAlignment); }
        { HostBatch h = validBatch(collapse); h.align_length[0] = 0; refused(h.view(), kEmptyAlignment); }
        { HostBatch h = validBatch(collapse); h.align_path_off[1] = 1000; refused(h.view(), kEmptyAlignment); }
        // 6: not ascending, equal neighbours, outside the cluster; the last entry
        { HostBatch h = validBatch(collapse); std::swap(h.path_idx[h.path_idx.size() - 1], h.path_idx[h.path_idx.size() - 2]); refused(h.view(), kAscending); }
        { HostBatch h = validBatch(collapse); h.path_idx[2] = h.path_idx[1]; refused(h.view(), kAscending); }
        { HostBatch h = validBatch(collapse); h.path_idx.back() = 40; refused(h.view(), kAscending); }
        { HostBatch h = validBatch(collapse); h.path_idx[3] = 3; refused(h.view(), kAscending); }  // cluster 0 has paths 0 .. 2
        { HostBatch h = validBatch(collapse); h.path_idx.back() = 39; REQUIRE(planAlignmentBatch(h.view()).status == 0); }
        // two faults: the one the loops meet first (clusters, then reads, then alignments in order; within a read the noise score last)
        { HostBatch h = validBatch(collapse); h.noise_score[0] = 5; h.path_idx.back() = 40; refused(h.view(), kNoiseScore); }
        { HostBatch h = validBatch(collapse); h.path_idx[0] = 3; h.noise_score[1] = 5; refused(h.view(), kAscending); }
        { HostBatch h = validBatch(collapse); h.read_align_off[6] = h.read_align_off[7]; h.noise_score[6] = 2; refused(h.view(), kNoiseScore); }
        { HostBatch h = validBatch(collapse); h.align_length[0] = 0; h.cluster_read_off[2] = 1; refused(h.view(), kEmptyAlignment); }
        { HostBatch h = validBatch(collapse); h.align_length.back() = 0; h.cluster_read_off[1] = 3; refused(h.view(), kDescending); }
    }
    // 2: collapsing only; the last path
    { HostBatch h = validBatch(true); h.path_group.back() = 20; refused(h.view(), kGroup); }
    { HostBatch h = validBatch(true); h.path_group[2] = 2; refused(h.view(), kGroup); }  // cluster 0 has groups 0 and 1
    { HostBatch h = validBatch(true); h.source_count.back() = 0; refused(h.view(), kGroup); }
    { HostBatch h = validBatch(true); h.source_count[0] = 0; h.noise_score[0] = 5; refused(h.view(), kGroup); }
    { HostBatch h = validBatch(false); h.source_count.back() = 0; h.path_group.back() = 99; REQUIRE(planAlignmentBatch(h.view()).status == 0); }
    // the collapse requirement and the NULL arrays, in the order of the checks
    const HostBatch h = validBatch(true);
    { rpvg_alignment_batch b = h.view(); b.cluster_group_off = nullptr; refused(b, "rpvg_hip_alignments_upload: collapsing needs cluster_group_off and path_source_count"); }
    { rpvg_alignment_batch b = h.view(); b.path_source_count = nullptr; refused(b, "rpvg_hip_alignments_upload: collapsing needs cluster_group_off and path_source_count"); }
    { rpvg_alignment_batch b = h.view(); b.path_group = nullptr; b.path_source_count = nullptr; b.cluster_group_off = nullptr; REQUIRE(planAlignmentBatch(b).status == 0); }
    { rpvg_alignment_batch b = h.view(); b.cluster_read_off = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL cluster offsets"); }
    { rpvg_alignment_batch b = h.view(); b.cluster_path_off = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL cluster offsets"); }
    { rpvg_alignment_batch b = h.view(); b.read_count = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL read arrays"); }
    { rpvg_alignment_batch b = h.view(); b.read_min_mapq = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL read arrays"); }
    { rpvg_alignment_batch b = h.view(); b.read_noise_score = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL read arrays"); }
    { rpvg_alignment_batch b = h.view(); b.read_align_off = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL read arrays"); }
    { rpvg_alignment_batch b = h.view(); b.path_effective_length = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL path_effective_length"); }
    { rpvg_alignment_batch b = h.view(); b.align_score_sum = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL alignment arrays"); }
    { rpvg_alignment_batch b = h.view(); b.align_length = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL alignment arrays"); }
    { rpvg_alignment_batch b = h.view(); b.align_frag_length = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL alignment arrays"); }
    { rpvg_alignment_batch b = h.view(); b.align_path_off = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL alignment arrays"); }
    { rpvg_alignment_batch b = h.view(); b.align_path_idx = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL align_path_idx"); }
    { rpvg_alignment_batch b = h.view(); b.read_count = nullptr; b.path_effective_length = nullptr; refused(b, "rpvg_hip_alignments_upload: NULL read arrays"); }
    // the size limits: decided on the totals, before an element is read
    {
        const uint64_t reads[1] = {0xffffffffull}, paths[1] = {0};
        rpvg_alignment_batch b{};
        b.cluster_read_off = reads;
        b.cluster_path_off = paths;
        refused(b, "rpvg_hip_alignments_upload: 4294967295 reads exceed one call");
    }
    {
        HostBatch one;
        one.addCluster(3, {2});
        one.align_path_off[1] = 0x100000000ull;
        refused(one.view(), "rpvg_hip_alignments_upload: 4294967296 path entries exceed one call");
    }
    // no clusters, and clusters without reads or paths: nothing to refuse, nothing read
    {
        const uint64_t zeros[3] = {0, 0, 0};
        rpvg_alignment_batch b{};
        b.cluster_read_off = zeros;
        b.cluster_path_off = zeros;
        for (const uint32_t K : {0u, 2u}) {
            b.num_clusters = K;
            const AlignmentBatchPlan p = planAlignmentBatch(b);
            REQUIRE(p.status == 0 && p.K == K && p.N == 0 && p.A == 0 && p.E == 0 && p.P == 0 && !p.collapse && p.h2d_bytes == 0);
            REQUIRE(p.read_cluster.empty() && p.small_reads.empty() && p.large_reads.empty() && p.h_out_path_off == std::vector<uint64_t>(K + 1, 0));
        }
    }
}

static void checkValidBatches() {
    for (const bool collapse : {false, true}) {
        const HostBatch h = validBatch(collapse);
        const rpvg_alignment_batch in = h.view();
        const AlignmentBatchPlan p = planAlignmentBatch(in);
        REQUIRE(p.status == 0 && p.message.empty());
        const uint32_t K = 3;
        const uint64_t N = 7, A = 8, E = 1 + 3 + 1 + 15 + 16 + 17 + 33, P = 63;
        REQUIRE(p.K == K && p.N == N && p.A == A && p.E == E && p.P == P && p.collapse == collapse);
        REQUIRE(p.read_cluster == (std::vector<uint32_t>{0, 0, 2, 2, 2, 2, 2}));
        // the old arithmetic
        std::vector<uint64_t> h_out_path_off(K + 1, 0);
        for (uint32_t k = 0; k < K; ++k) {
            h_out_path_off[k + 1] = h_out_path_off[k] + (collapse ? in.cluster_group_off[k + 1] - in.cluster_group_off[k]
                                                                  : in.cluster_path_off[k + 1] - in.cluster_path_off[k]);
        }
        REQUIRE(p.h_out_path_off == h_out_path_off);
        REQUIRE(p.h_out_path_off == (collapse ? std::vector<uint64_t>{0, 2, 12, 32} : std::vector<uint64_t>{0, 3, 23, 63}));
        std::vector<uint32_t> small_reads, large_reads;
        for (uint64_t r = 0; r < N; ++r) {
            const uint64_t entries = in.align_path_off[in.read_align_off[r + 1]] - in.align_path_off[in.read_align_off[r]];
            (entries <= static_cast<uint64_t>(16) && !collapse ? small_reads : large_reads).push_back(static_cast<uint32_t>(r));
        }
        REQUIRE(p.small_reads == small_reads && p.large_reads == large_reads);
        // reads 4 and 5 have exactly 16 and 17 entries
        if (collapse) REQUIRE(p.small_reads.empty() && p.large_reads == (std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6}));
        else REQUIRE(p.small_reads == (std::vector<uint32_t>{0, 1, 2, 3, 4}) && p.large_reads == (std::vector<uint32_t>{5, 6}));
        REQUIRE(p.h2d_bytes == static_cast<double>(N) * 25 + static_cast<double>(A) * 16 + static_cast<double>(E) * 4 + static_cast<double>(P) * 8);
        REQUIRE(p.h2d_bytes == 25.0 * 7 + 16.0 * 8 + 4.0 * 86 + 8.0 * 63);
    }
    REQUIRE(kGroupLanes == 16 && kWavesPerBlock == 4 && kSmallSort == 2048);
    REQUIRE(readIsSmall(0, false) && readIsSmall(16, false) && !readIsSmall(17, false) && !readIsSmall(16, true) && !readIsSmall(1, true) && !readIsSmall(17, true));
}

// ---- the sort plan against the loops of mergeRows ---------------------------------------------------------------------------

struct OldLaunch {
    int kind;  // 0 sortTilesBigKernel first, 1 bitonicStepBigKernel, 2 sortTilesBigKernel finish
    uint32_t k, j, grid;
};

static uint32_t gridFor(const uint64_t n, const uint32_t block) { return static_cast<uint32_t>((n + block - 1) / block); }

static void checkSortPlan(const std::vector<uint64_t> & sizes) {
    std::vector<uint64_t> h_cluster_read_off(1, 0);
    for (const uint64_t n : sizes) h_cluster_read_off.push_back(h_cluster_read_off.back() + n);
    const uint32_t K = static_cast<uint32_t>(sizes.size());
    const uint64_t N = h_cluster_read_off.back();
    // mergeRows, as it was
    std::vector<uint32_t> small_clusters, big_clusters, big_padded;
    std::vector<uint64_t> big_pair_off(1, 0);
    uint32_t max_padded = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t n = h_cluster_read_off[k + 1] - h_cluster_read_off[k];
        if (n < 2) continue;
        if (n <= 2048) {
            small_clusters.push_back(k);
        } else {
            uint32_t L = 2048;
            while (L < n) L <<= 1;
            big_clusters.push_back(k);
            big_padded.push_back(L);
            big_pair_off.push_back(big_pair_off.back() + L / 2);
            max_padded = std::max(max_padded, L);
        }
    }
    std::vector<uint32_t> tile_cluster, tile_index;
    std::vector<OldLaunch> launches;
    if (!big_clusters.empty()) {
        const uint32_t num_big = static_cast<uint32_t>(big_clusters.size());
        for (uint32_t b = 0; b < num_big; ++b) {
            for (uint32_t t = 0; t < big_padded[b] / 2048; ++t) {
                tile_cluster.push_back(big_clusters[b]);
                tile_index.push_back(t);
            }
        }
        const uint32_t num_tiles = static_cast<uint32_t>(tile_cluster.size());
        launches.push_back(OldLaunch{0, 0, 0, num_tiles});
        for (uint32_t k = 2 * 2048; k <= max_padded; k <<= 1) {
            for (uint32_t j = k >> 1; j >= 2048; j >>= 1) launches.push_back(OldLaunch{1, k, j, gridFor(big_pair_off.back(), 256)});
            launches.push_back(OldLaunch{2, k, 0, num_tiles});
        }
    }

    const RowSortPlan p = planRowSort(h_cluster_read_off.data(), K);
    REQUIRE(p.small_clusters == small_clusters && p.big_clusters == big_clusters && p.big_padded == big_padded && p.big_pair_off == big_pair_off);
    REQUIRE(p.tile_cluster == tile_cluster && p.tile_index == tile_index && p.max_padded == max_padded);
    REQUIRE(p.iota.grid == gridFor(N, 256) && p.iota.block == 256);
    REQUIRE(p.sort_small.grid == small_clusters.size() && p.sort_small.block == (small_clusters.empty() ? 0u : 256u));
    REQUIRE(p.big_launches.size() == launches.size());
    for (size_t i = 0; i < launches.size(); ++i) {
        const SortLaunch & l = p.big_launches[i];
        const int kind = l.kind == SortStep::TileSort ? 0 : l.kind == SortStep::GlobalStep ? 1 : 2;
        REQUIRE(kind == launches[i].kind && l.k == launches[i].k && l.j == launches[i].j && l.shape.grid == launches[i].grid && l.shape.block == 256);
    }
}

// ---- the planned launches as a sorting network ------------------------------------------------------------------------------

static const uint32_t kNone = 0xffffffffu;

struct Replay {
    std::vector<uint64_t> cluster_read_off;
    std::vector<uint32_t> key, sorted;
    // a strict total order: the key, then the row (RowLess ends on the row id too)
    bool less(const uint32_t a, const uint32_t b) const { return key[a] != key[b] ? key[a] < key[b] : a < b; }

    // SortTile::exchange: padding behaves as +infinity
    void exchange(std::vector<uint32_t> & id, const uint32_t i, const uint32_t l) const {
        const uint32_t a = id[i], b = id[l];
        if (b != kNone && (a == kNone || less(b, a))) std::swap(id[i], id[l]);
    }

    void sortSmallClusters(const RowSortPlan & p) {
        for (uint32_t block = 0; block < p.sort_small.grid; ++block) {
            const uint32_t c = p.small_clusters[block];
            const uint64_t r0 = cluster_read_off[c];
            const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
            const uint32_t L = sortPadded(n);
            REQUIRE(L <= kSmallSort);  // the tile in LDS
            std::vector<uint32_t> id(L);
            for (uint32_t i = 0; i < L; ++i) id[i] = (i < n) ? static_cast<uint32_t>(r0 + i) : kNone;
            for (uint32_t k = 2; k <= L; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = 0; t < (L >> 1); ++t) {
                        uint32_t i, l;
                        bitonicPair(t, k, j, &i, &l);
                        REQUIRE(i < l && l < L);
                        exchange(id, i, l);
                    }
                }
            }
            for (uint32_t i = 0; i < n; ++i) sorted[r0 + i] = id[i];
        }
    }

    void sortTilesBig(const RowSortPlan & p, const SortLaunch & launch) {
        const bool first = launch.kind == SortStep::TileSort;
        const uint32_t k_merge = launch.k;
        REQUIRE(launch.shape.grid == p.tile_cluster.size());
        for (uint32_t block = 0; block < launch.shape.grid; ++block) {
            const uint32_t c = p.tile_cluster[block];
            const uint64_t r0 = cluster_read_off[c];
            const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
            const uint32_t base = p.tile_index[block] * kSmallSort;
            if (base >= n) continue;
            if (!first && k_merge > sortPadded(n)) continue;
            std::vector<uint32_t> id(kSmallSort);
            for (uint32_t i = 0; i < kSmallSort; ++i) id[i] = (base + i < n) ? sorted[r0 + base + i] : kNone;
            if (first) {
                for (uint32_t k = 2; k <= kSmallSort; k <<= 1) {
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        for (uint32_t t = 0; t < (kSmallSort >> 1); ++t) {
                            uint32_t i, l;
                            bitonicPair(t, k, j, &i, &l);
                            REQUIRE(i < l && l < kSmallSort);
                            exchange(id, i, l);
                        }
                    }
                }
            } else {
                for (uint32_t j = kSmallSort >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = 0; t < (kSmallSort >> 1); ++t) {
                        uint32_t i, l;
                        bitonicPair(t, k_merge, j, &i, &l);
                        REQUIRE(i < l && l < kSmallSort);
                        exchange(id, i, l);
                    }
                }
            }
            for (uint32_t i = 0; i < kSmallSort; ++i) {
                if (base + i < n) sorted[r0 + base + i] = id[i];
            }
        }
    }

    void bitonicStepBig(const RowSortPlan & p, const SortLaunch & launch) {
        const uint32_t num_big = static_cast<uint32_t>(p.big_clusters.size()), k = launch.k, j = launch.j;
        const uint64_t threads = static_cast<uint64_t>(launch.shape.grid) * launch.shape.block;
        REQUIRE(threads >= p.big_pair_off[num_big]);  // a thread per pair
        for (uint64_t g = 0; g < threads; ++g) {
            if (g >= p.big_pair_off[num_big]) continue;
            uint32_t lo = 0, hi = num_big - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (p.big_pair_off[mid] <= g) lo = mid; else hi = mid - 1;
            }
            if (k > p.big_padded[lo]) continue;
            const uint32_t c = p.big_clusters[lo];
            const uint64_t r0 = cluster_read_off[c];
            const uint32_t n = static_cast<uint32_t>(cluster_read_off[c + 1] - r0);
            uint32_t i, l;
            bitonicPair(static_cast<uint32_t>(g - p.big_pair_off[lo]), k, j, &i, &l);
            REQUIRE(i < l && l < p.big_padded[lo]);
            if (l >= n) continue;
            const uint32_t a = sorted[r0 + i], b = sorted[r0 + l];
            if (less(b, a)) {
                sorted[r0 + i] = b;
                sorted[r0 + l] = a;
            }
        }
    }

    void run() {
        const uint32_t K = static_cast<uint32_t>(cluster_read_off.size() - 1);
        const uint64_t N = cluster_read_off.back();
        const RowSortPlan p = planRowSort(cluster_read_off.data(), K);
        REQUIRE(static_cast<uint64_t>(p.iota.grid) * p.iota.block >= N);
        sorted.assign(N, kNone);
        for (uint64_t i = 0; i < N; ++i) sorted[i] = static_cast<uint32_t>(i);
        sortSmallClusters(p);
        for (const SortLaunch & launch : p.big_launches) {
            if (launch.kind == SortStep::GlobalStep) bitonicStepBig(p, launch);
            else sortTilesBig(p, launch);
        }
        // every cluster: its own rows, each once, in order
        for (uint32_t c = 0; c < K; ++c) {
            const uint64_t r0 = cluster_read_off[c], r1 = cluster_read_off[c + 1];
            std::vector<uint32_t> rows(sorted.begin() + r0, sorted.begin() + r1);
            for (uint64_t i = r0; i + 1 < r1; ++i) REQUIRE(less(sorted[i], sorted[i + 1]));
            std::sort(rows.begin(), rows.end());
            for (uint64_t i = r0; i < r1; ++i) REQUIRE(rows[i - r0] == i);
        }
    }
};

static void checkNetwork(const std::vector<uint64_t> & sizes) {
    for (int keys = 0; keys < 3; ++keys) {
        Replay r;
        r.cluster_read_off.assign(1, 0);
        for (const uint64_t n : sizes) r.cluster_read_off.push_back(r.cluster_read_off.back() + n);
        const uint64_t N = r.cluster_read_off.back();
        r.key.resize(N);
        uint32_t state = 12345u + static_cast<uint32_t>(sizes.size());
        for (uint64_t i = 0; i < N; ++i) {
            state = state * 1664525u + 1013904223u;
            r.key[i] = keys == 0 ? static_cast<uint32_t>(N - i) : keys == 1 ? (state >> 8) % 1000u : 7u;  // reversed; random with ties; all equal
        }
        r.run();
    }
}

static void checkHelpers() {
    for (uint32_t n = 0; n <= 20000; ++n) {
        uint32_t L;
        if (n <= 2048) {
            L = 2;
            while (L < n) L <<= 1;
        } else {
            L = 2048;
            while (L < n) L <<= 1;
        }
        REQUIRE(sortPadded(n) == L);
    }
    REQUIRE(sortPadded(2048) == 2048 && sortPadded(2049) == 4096 && sortPadded(1u << 31) == (1u << 31));
    // every step of the network pairs every position exactly once
    for (uint32_t L = 2; L <= 64; L <<= 1) {
        for (uint32_t k = 2; k <= L; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                std::vector<int> seen(L, 0);
                for (uint32_t t = 0; t < L / 2; ++t) {
                    uint32_t i, l;
                    bitonicPair(t, k, j, &i, &l);
                    REQUIRE(i < l && l < L && i / k == l / k);
                    ++seen[i];
                    ++seen[l];
                }
                for (const int s : seen) REQUIRE(s == 1);
            }
        }
    }
    // the launch shapes, as the launches spelled them
    const uint64_t counts[] = {1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4096, 100001, 0xfffffffeull};
    for (const uint64_t n : counts) {
        const PackPlan pack = planPack(n);
        REQUIRE(pack.gather_sizes.grid == gridFor(n, 256) && pack.gather_sizes.block == 256);
        REQUIRE(pack.pack.grid == gridFor(n * 16, 256) && pack.pack.block == 256);
        for (const uint64_t num_small : {uint64_t(0), n / 3, n}) {
            const uint64_t num_large = n - num_small, A = n + n / 2;
            const RowKernelsPlan with = planRowKernels(n, A, num_small, num_large, true), without = planRowKernels(n, A, num_small, num_large, false);
            REQUIRE(with.align_log_prob.grid == gridFor(A, 256) && with.align_log_prob.block == 256);
            REQUIRE(without.align_log_prob.grid == gridFor(A, 256) && without.align_log_prob.block == 256);
            REQUIRE(!with.every_read && with.small_reads.grid == (num_small ? gridFor(num_small * 16, 256) : 0u) && (!num_small || with.small_reads.block == 256));
            REQUIRE(with.large_reads.grid == (num_large ? gridFor(num_large, 4) : 0u) && (!num_large || with.large_reads.block == 256));
            REQUIRE(without.every_read && without.small_reads.grid == 0 && without.large_reads.grid == gridFor(n, 4) && without.large_reads.block == 256);
        }
    }
}

int main() {
    checkRefusals();
    checkValidBatches();
    checkHelpers();
    const std::vector<uint64_t> edges = {0, 1, 2, 3, 2047, 2048, 2049, 4096, 4097, 8192, 8193};
    const std::vector<uint64_t> mixed = {4097, 3, 0, 2049, 1, 2, 2047, 2048, 8192, 4096, 8193, 0};
    checkSortPlan({});
    checkSortPlan(mixed);
    checkNetwork(mixed);
    for (const uint64_t n : edges) {
        checkSortPlan({n});
        checkNetwork({n});
        checkSortPlan({5, n, 0, n});
    }
    checkNetwork({8193, 2049, 4097});  // three padded lengths, the longest first
    std::printf("ok\n");
    return 0;
}
