// The plan of a batch upload (rpvg_amd/csrc/batch_forms.hpp) as a program of its own, built against the header alone with
// AddressSanitizer and UBSan: every form a host batch may arrive in, the argument errors with their wording, the bytes the copies
// move against the formula the upload used before the plan existed (written out below), and the host reads that happen before
// anything has been validated.  Every array of every case sits in a heap block of exactly its length, so a read outside one
// ends the program.  Prints "ok".
#include "batch_forms.hpp"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

using namespace rpvg_batch_forms;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

// a heap block of exactly n elements (n = 0: a block of no bytes, not NULL)
template <typename T>
struct Block {
    std::unique_ptr<T[]> p;
    size_t n = 0;
    Block() {}
    explicit Block(const std::vector<T> & v) : p(new T[v.size()]), n(v.size()) { std::copy(v.begin(), v.end(), p.get()); }
    const T * get() const { return p.get(); }
};

// A batch in every form at once; view() hands out the forms a case asks for, everything else NULL.
struct Host {
    std::vector<uint64_t> cluster_row_off{0}, cluster_path_off{0}, row_grp_off{0}, grp_idx_off{0};
    std::vector<uint32_t> row_count, path_idx;
    std::vector<double> row_noise, grp_prob;

    // rows of `groups` groups each, group g of the row with 1 + (g % 3) paths
    void addCluster(const uint32_t paths, const std::vector<uint32_t> & row_groups) {
        for (const uint32_t groups : row_groups) {
            for (uint32_t g = 0; g < groups; ++g) {
                for (uint32_t i = 0; i < 1 + g % 3; ++i) path_idx.push_back((g + i) % paths);
                grp_prob.push_back(0.125 * (1 + g % 7));
                grp_idx_off.push_back(path_idx.size());
            }
            row_count.push_back(row_count.size() % 5 == 2 ? 300u : 1u + static_cast<uint32_t>(row_count.size() % 4));
            row_noise.push_back(row_noise.size() % 2 ? 0.25 : 0.5);
            row_grp_off.push_back(grp_prob.size());
        }
        cluster_row_off.push_back(row_count.size());
        cluster_path_off.push_back(cluster_path_off.back() + paths);
    }

    Block<uint64_t> b_cluster_row_off, b_cluster_path_off, b_row_grp_off, b_grp_idx_off;
    Block<uint32_t> b_row_count, b_path_idx, b_row_grp_off32, b_grp_idx_off32, b_escape_row, b_escape_count;
    Block<double> b_row_noise, b_grp_prob, b_noise_table;
    Block<uint8_t> b_row_grp_count8, b_grp_idx_count8, b_row_count8;
    Block<uint16_t> b_path_idx16, b_row_noise16;

    // the description without its blocks, to be changed and frozen again
    Host unfrozen() const {
        Host copy;
        copy.cluster_row_off = cluster_row_off;
        copy.cluster_path_off = cluster_path_off;
        copy.row_grp_off = row_grp_off;
        copy.grp_idx_off = grp_idx_off;
        copy.row_count = row_count;
        copy.path_idx = path_idx;
        copy.row_noise = row_noise;
        copy.grp_prob = grp_prob;
        return copy;
    }

    void freeze() {
        b_cluster_row_off = Block<uint64_t>(cluster_row_off);
        b_cluster_path_off = Block<uint64_t>(cluster_path_off);
        b_row_grp_off = Block<uint64_t>(row_grp_off);
        b_grp_idx_off = Block<uint64_t>(grp_idx_off);
        b_row_count = Block<uint32_t>(row_count);
        b_path_idx = Block<uint32_t>(path_idx);
        b_row_noise = Block<double>(row_noise);
        b_grp_prob = Block<double>(grp_prob);
        b_row_grp_off32 = Block<uint32_t>(std::vector<uint32_t>(row_grp_off.begin(), row_grp_off.end()));
        b_grp_idx_off32 = Block<uint32_t>(std::vector<uint32_t>(grp_idx_off.begin(), grp_idx_off.end()));
        std::vector<uint8_t> c8;
        for (size_t r = 0; r + 1 < row_grp_off.size(); ++r) c8.push_back(static_cast<uint8_t>(row_grp_off[r + 1] - row_grp_off[r]));
        b_row_grp_count8 = Block<uint8_t>(c8);
        c8.clear();
        for (size_t g = 0; g + 1 < grp_idx_off.size(); ++g) c8.push_back(static_cast<uint8_t>(grp_idx_off[g + 1] - grp_idx_off[g]));
        b_grp_idx_count8 = Block<uint8_t>(c8);
        c8.clear();
        std::vector<uint32_t> escape_row, escape_count;
        for (size_t r = 0; r < row_count.size(); ++r) {
            c8.push_back(static_cast<uint8_t>(std::min<uint32_t>(row_count[r], 255)));
            if (row_count[r] >= 255) {
                escape_row.push_back(static_cast<uint32_t>(r));
                escape_count.push_back(row_count[r]);
            }
        }
        b_row_count8 = Block<uint8_t>(c8);
        b_escape_row = Block<uint32_t>(escape_row);
        b_escape_count = Block<uint32_t>(escape_count);
        b_path_idx16 = Block<uint16_t>(std::vector<uint16_t>(path_idx.begin(), path_idx.end()));
        b_noise_table = Block<double>(std::vector<double>{0.25, 0.5});
        std::vector<uint16_t> n16;
        for (const double nz : row_noise) n16.push_back(nz == 0.25 ? 0 : 1);
        b_row_noise16 = Block<uint16_t>(n16);
    }

    enum Offsets { k64_64, k32_32, k32_64, k64_32, kCounts };

    rpvg_cluster_batch view(const Offsets offsets, const bool noise16, const bool count8, const bool path16) const {
        rpvg_cluster_batch hb;
        std::memset(&hb, 0, sizeof(hb));
        hb.num_clusters = static_cast<uint32_t>(cluster_row_off.size() - 1);
        hb.cluster_row_off = b_cluster_row_off.get();
        hb.cluster_path_off = b_cluster_path_off.get();
        hb.grp_prob = b_grp_prob.get();
        if (offsets == kCounts) {
            hb.row_grp_count8 = b_row_grp_count8.get();
            hb.grp_idx_count8 = b_grp_idx_count8.get();
            hb.num_groups = grp_prob.size();
            hb.num_entries = path_idx.size();
        } else {
            if (offsets == k32_32 || offsets == k32_64) hb.row_grp_off32 = b_row_grp_off32.get();
            else hb.row_grp_off = b_row_grp_off.get();
            if (offsets == k32_32 || offsets == k64_32) hb.grp_idx_off32 = b_grp_idx_off32.get();
            else hb.grp_idx_off = b_grp_idx_off.get();
        }
        if (noise16) {
            hb.row_noise16 = b_row_noise16.get();
            hb.row_noise_table = b_noise_table.get();
            hb.num_row_noise_values = b_noise_table.n;
        } else {
            hb.row_noise = b_row_noise.get();
        }
        if (count8) {
            hb.row_count8 = b_row_count8.get();
            hb.row_count_escape_row = b_escape_row.get();
            hb.row_count_escape_count = b_escape_count.get();
            hb.num_row_count_escapes = b_escape_row.n;
        } else {
            hb.row_count = b_row_count.get();
        }
        if (path16) hb.path_idx16 = b_path_idx16.get();
        else hb.path_idx = b_path_idx.get();
        return hb;
    }
};

// What the upload added to its h2d_bytes statistic before the plan existed, from the caller's pointers (K, R, G, NNZ as the
// upload read them).
static uint64_t formerCopyBytes(const rpvg_cluster_batch * hb, const uint64_t R, const uint64_t G, const uint64_t NNZ) {
    const uint64_t K = hb->num_clusters;
    const bool counts = R > 0 && hb->row_grp_count8 != nullptr && hb->grp_idx_count8 != nullptr;
    return (K + 1) * 16 + (hb->row_noise16 ? R * 2 + 8 * hb->num_row_noise_values : R * 8) + (hb->row_count8 ? R + 8 * hb->num_row_count_escapes : 4 * R) +
           (counts ? R : (R + 1) * (hb->row_grp_off32 ? 4 : 8)) + (counts ? G : (G + 1) * (hb->grp_idx_off32 ? 4 : 8)) + G * 8 + NNZ * (hb->path_idx16 ? 2 : 4);
}

static BatchForms accepted(const rpvg_cluster_batch & hb, std::vector<uint64_t> * cluster_ent_off) {
    BatchForms forms;
    char message[kMessageChars] = "";
    if (!planBatchForms(&hb, &forms, cluster_ent_off, message)) {
        std::fprintf(stderr, "refused: %s\n", message);
        std::exit(1);
    }
    CHECK(forms.K == hb.num_clusters && cluster_ent_off->size() == static_cast<size_t>(forms.K) + 1);
    CHECK(forms.row_copy_bytes == formerCopyBytes(&hb, forms.R, forms.G, forms.NNZ));
    return forms;
}

static void refused(const rpvg_cluster_batch & hb, const char * words) {
    BatchForms forms;
    std::vector<uint64_t> cluster_ent_off;
    char message[kMessageChars] = "";
    CHECK(!planBatchForms(&hb, &forms, &cluster_ent_off, message));
    if (std::string(message) != words) {
        std::fprintf(stderr, "refused with \"%s\", expected \"%s\"\n", message, words);
        std::exit(1);
    }
}

int main() {
    std::vector<uint64_t> ent_off;

    {  // no clusters: one-element cluster offsets, nothing else
        Host h;
        h.freeze();
        rpvg_cluster_batch hb;
        std::memset(&hb, 0, sizeof(hb));
        hb.cluster_row_off = h.b_cluster_row_off.get();
        hb.cluster_path_off = h.b_cluster_path_off.get();
        const BatchForms f = accepted(hb, &ent_off);
        CHECK(f.K == 0 && f.R == 0 && f.G == 0 && f.NNZ == 0 && f.P == 0 && !f.counts() && f.row_copy_bytes == 32 && ent_off == std::vector<uint64_t>{0});
        hb.cluster_row_off = nullptr;
        refused(hb, "rpvg_hip_batch_upload: cluster offsets are NULL");
    }
    {  // one cluster without rows, every row array NULL — also with counts named, which an empty batch does not read
        Host h;
        h.addCluster(3, {});
        h.freeze();
        rpvg_cluster_batch hb;
        std::memset(&hb, 0, sizeof(hb));
        hb.num_clusters = 1;
        hb.cluster_row_off = h.b_cluster_row_off.get();
        hb.cluster_path_off = h.b_cluster_path_off.get();
        BatchForms f = accepted(hb, &ent_off);
        CHECK(f.K == 1 && f.R == 0 && f.G == 0 && f.NNZ == 0 && f.P == 3 && f.row_offsets == OffsetForm::Wide64 && f.group_offsets == OffsetForm::Wide64);
        CHECK(f.row_copy_bytes == 48 && (ent_off == std::vector<uint64_t>{0, 0}));
        hb.row_grp_count8 = h.b_row_grp_count8.get();
        hb.grp_idx_count8 = h.b_grp_idx_count8.get();
        f = accepted(hb, &ent_off);
        CHECK(!f.counts() && f.row_copy_bytes == 48);
        hb.row_grp_off32 = h.b_row_grp_off32.get();  // (one element: the offset of row 0)
        f = accepted(hb, &ent_off);
        CHECK(f.row_offsets == OffsetForm::Narrow32 && f.row_copy_bytes == 44);
    }

    // clusters with and without rows, a row without groups, groups of several paths, read counts of 255 and more
    Host h;
    h.addCluster(4, {2, 0, 5});
    h.addCluster(2, {});
    h.addCluster(7, {1, 3, 3, 9});
    h.addCluster(1, {1});
    h.freeze();
    const uint64_t R = h.row_count.size(), G = h.grp_prob.size(), NNZ = h.path_idx.size();
    std::vector<uint64_t> want_ent_off;
    for (const uint64_t r : h.cluster_row_off) want_ent_off.push_back(h.grp_idx_off[h.row_grp_off[r]]);
    CHECK(R == 8 && h.b_escape_row.n >= 1 && want_ent_off.back() == NNZ);

    const Host::Offsets every_offsets[] = {Host::k64_64, Host::k32_32, Host::k32_64, Host::k64_32, Host::kCounts};
    for (const Host::Offsets offsets : every_offsets) {
        for (int narrow = 0; narrow < 8; ++narrow) {
            const bool noise16 = narrow & 1, count8 = narrow & 2, path16 = narrow & 4;
            const rpvg_cluster_batch hb = h.view(offsets, noise16, count8, path16);
            const BatchForms f = accepted(hb, &ent_off);
            CHECK(f.K == 4 && f.R == R && f.G == G && f.NNZ == NNZ && f.P == 14);
            CHECK(f.noise16 == noise16 && f.count8 == count8 && f.path16 == path16);
            CHECK(f.counts() == (offsets == Host::kCounts) && (f.group_offsets == OffsetForm::Counts8) == f.counts());
            if (!f.counts()) {
                CHECK((f.row_offsets == OffsetForm::Narrow32) == (offsets == Host::k32_32 || offsets == Host::k32_64));
                CHECK((f.group_offsets == OffsetForm::Narrow32) == (offsets == Host::k32_32 || offsets == Host::k64_32));
                CHECK(ent_off == want_ent_off);
            } else {
                CHECK(ent_off == std::vector<uint64_t>(5, 0));  // (the device brings them)
            }
        }
    }
    {  // 32 bits win over 64 where both are given; the counts over both
        rpvg_cluster_batch hb = h.view(Host::k64_64, false, false, false);
        hb.row_grp_off32 = h.b_row_grp_off32.get();
        BatchForms f = accepted(hb, &ent_off);
        CHECK(f.row_offsets == OffsetForm::Narrow32 && f.group_offsets == OffsetForm::Wide64 && ent_off == want_ent_off);
        hb.row_grp_count8 = h.b_row_grp_count8.get();
        f = accepted(hb, &ent_off);
        CHECK(!f.counts());  // (one of the two only: not the count form)
        hb.grp_idx_count8 = h.b_grp_idx_count8.get();
        hb.num_groups = G;
        hb.num_entries = NNZ;
        f = accepted(hb, &ent_off);
        CHECK(f.counts() && f.G == G && f.NNZ == NNZ);
    }

    {  // counts come with their totals
        rpvg_cluster_batch hb = h.view(Host::kCounts, false, false, false);
        const char * words = "rpvg_hip_batch_upload: counts of one byte come with their totals (num_groups, num_entries: below 2^32 - 1)";
        hb.num_groups = 0;
        refused(hb, words);
        hb.num_groups = 0xffffffffull;
        refused(hb, words);
        hb.num_groups = G;
        hb.num_entries = 0xffffffffull;
        refused(hb, words);
        hb.num_entries = 0x100000000ull;
        refused(hb, words);
        hb.num_entries = 0xfffffffeull;  // (the device's sums refuse it later: nothing is read by them here)
        CHECK(accepted(hb, &ent_off).NNZ == 0xfffffffeull);
    }
    {  // the other argument errors
        rpvg_cluster_batch hb = h.view(Host::k64_64, false, false, false);
        hb.row_count = nullptr;
        refused(hb, "rpvg_hip_batch_upload: row arrays are NULL");
        hb = h.view(Host::k32_64, true, false, false);
        hb.row_noise_table = nullptr;
        refused(hb, "rpvg_hip_batch_upload: row arrays are NULL");
        hb = h.view(Host::k64_32, false, false, false);
        hb.grp_idx_off32 = nullptr;
        refused(hb, "rpvg_hip_batch_upload: row arrays are NULL");
        hb = h.view(Host::k32_32, false, false, false);
        hb.grp_prob = nullptr;
        refused(hb, "rpvg_hip_batch_upload: grp_prob is NULL");
        hb = h.view(Host::kCounts, false, false, true);
        hb.path_idx16 = nullptr;
        refused(hb, "rpvg_hip_batch_upload: path_idx is NULL");
        hb = h.view(Host::k64_64, false, true, false);
        hb.row_count_escape_count = nullptr;
        refused(hb, "rpvg_hip_batch_upload: row_count8 comes with the list of the rows whose count does not fit a byte");
    }
    {  // cluster offsets: decreasing, not from row 0, too many paths
        Host bad = h.unfrozen();
        bad.cluster_row_off = {0, 3, 2, 7, 8};
        bad.freeze();
        refused(bad.view(Host::k32_32, false, false, false), "rpvg_hip_batch_upload: cluster 1 has decreasing offsets");
        bad = h.unfrozen();
        bad.cluster_path_off = {0, 4, 6, 5, 14};
        bad.freeze();
        refused(bad.view(Host::kCounts, true, true, true), "rpvg_hip_batch_upload: cluster 2 has decreasing offsets");
        bad = h.unfrozen();
        bad.cluster_row_off[0] = 1;
        bad.freeze();
        refused(bad.view(Host::k64_64, false, false, false), "rpvg_hip_batch_upload: the first cluster does not start at row 0");
        Host wide;
        wide.addCluster(3, {});
        wide.cluster_path_off = {0, 0x80000000ull};  // 2^31 paths
        wide.freeze();
        rpvg_cluster_batch hb;
        std::memset(&hb, 0, sizeof(hb));
        hb.num_clusters = 1;
        hb.cluster_row_off = wide.b_cluster_row_off.get();
        hb.cluster_path_off = wide.b_cluster_path_off.get();
        refused(hb, "rpvg_hip_batch_upload: cluster 0 has too many paths");
        wide.cluster_path_off = {0, 0x7fffffffull};  // the most a cluster may have
        wide.freeze();
        hb.cluster_row_off = wide.b_cluster_row_off.get();
        hb.cluster_path_off = wide.b_cluster_path_off.get();
        CHECK(accepted(hb, &ent_off).P == 0x7fffffffull);
    }
    {  // a wild group offset at a cluster's first row: nothing outside the arrays is read, and there is a plan (the device refuses the batch)
        const Host::Offsets with_offsets[] = {Host::k64_64, Host::k32_32, Host::k32_64, Host::k64_32};
        for (const uint32_t k : {1u, 2u, 3u}) {
            Host wild = h.unfrozen();
            wild.row_grp_off[wild.cluster_row_off[k]] = G + 1000;
            wild.freeze();
            for (const Host::Offsets offsets : with_offsets) {
                const BatchForms f = accepted(wild.view(offsets, false, false, false), &ent_off);
                CHECK(f.G == G && f.NNZ == NNZ);
                for (uint32_t j = 0; j <= 4; ++j) CHECK(ent_off[j] == (h.cluster_row_off[j] == h.cluster_row_off[k] ? NNZ : want_ent_off[j]));
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
