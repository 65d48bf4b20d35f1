// ReadCountGibbsSamplesWriter::addTable() (rpvg_amd/host/io/estimates_writers.cpp) against its addSamples(): the same containers
// written both ways must give the same file bytes for ONE table per writer, the `Unknown` row included.  The table the GPU would
// build is filled here by a host loop in the order include/rpvg_samples.h states (test code: the product has no host computation
// of the table).  With TWO tables into one writer the rows are still the same bytes; the noise totals join in one addition per
// column, which is another order of additions than addSamples()'s chain: the check constructs a column where the two doubles
// differ.  Built with AddressSanitizer and UBSan as a program of its own; prints "ok".
//   gibbs_writer_check <directory for the files>
// It leaves <directory>/one_table.txt.gz (the file of the one-table case) and <directory>/one_table_containers.txt (its
// containers, doubles as %.17g) for the Python model to format and compare.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>

#include <zlib.h>

#include "gibbs_samples_table.hpp"
#include "io/estimates_writers.hpp"

using namespace rpvg_amd;

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "%s:%d: case '%s': %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

static std::string g_case;

static std::string slurp(const std::string & filename) {
    std::ifstream in(filename, std::ios::binary);
    std::stringstream text;
    text << in.rdbuf();
    return text.str();
}

static std::string gunzip(const std::string & filename) {
    gzFile in = gzopen(filename.c_str(), "rb");
    if (!in) return "";
    std::string text;
    char buffer[4096];
    int got;
    while ((got = gzread(in, buffer, sizeof(buffer))) > 0) text.append(buffer, got);
    gzclose(in);
    return text;
}

// the arrays of rpvg_gibbs_table_view from the flat samples, by the loops rpvg_samples.h states
struct HostTable {
    std::vector<double> samples, noise_counts;
    std::vector<uint8_t> listed;
    rpvg_gibbs_table_view view;

    HostTable(const FlatGibbs & flat, const uint32_t N) {
        const size_t K = flat.total_count.size(), P = flat.labels.names.size();
        samples.assign(P * N, 0.0);
        listed.assign(P, 0);
        noise_counts.assign(N, 0.0);
        for (size_t k = 0; k < K; ++k) {
            const uint64_t p0 = flat.cluster_path_off[k];
            uint64_t base = 0;
            for (uint64_t b = flat.gibbs_off[k]; b < flat.gibbs_off[k + 1]; ++b) {
                const uint64_t c = flat.path_off[b + 1] - flat.path_off[b], n = flat.noise_off[b + 1] - flat.noise_off[b];
                for (uint64_t j = 0; j < c; ++j) {
                    const uint64_t g = p0 + flat.path[flat.path_off[b] + j];
                    if (n > 0) listed[g] = 1;
                    for (uint64_t s = 0; s < n; ++s) samples[g * N + base + s] = flat.abund[flat.abund_off[b] + s * c + j];
                }
                base += n;
            }
            for (uint32_t s = 0; s < N; ++s) {
                noise_counts[s] += s < base ? flat.noise[flat.noise_off[flat.gibbs_off[k]] + s] : flat.total_count[k];
            }
        }
        view = rpvg_gibbs_table_view();
        view.num_clusters = K;
        view.num_blocks = flat.path_off.size() - 1;
        view.num_paths = P;
        view.num_gibbs_samples = N;
        view.samples = samples.data();
        view.listed = listed.data();
        view.noise_counts = noise_counts.data();
        view.cluster_path_off = flat.cluster_path_off.data();
    }
};

// what the estimator hands to the writer: the CountSamples without samples dropped (rpvg_amd/host/path_abundance_estimator.cpp)
static std::pair<uint32_t, PathClusterEstimates> forWriter(const std::pair<uint32_t, PathClusterEstimates> & with_empty) {
    auto out = with_empty;
    out.second.gibbs_read_count_samples.clear();
    for (auto & count_samples : with_empty.second.gibbs_read_count_samples) {
        if (!count_samples.noise_samples.empty()) out.second.gibbs_read_count_samples.push_back(count_samples);
    }
    return out;
}

// clusters of random sizes: blocks of random ascending ids, some without samples, some clusters without blocks, S_k <= N
static ClusterEstimatesList makeList(std::mt19937 & rng, const uint32_t N, const size_t clusters, const uint32_t first_id) {
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    ClusterEstimatesList list;
    for (size_t k = 0; k < clusters; ++k) {
        PathClusterEstimates e;
        const uint32_t num_paths = 1 + rng() % 9;
        for (uint32_t p = 0; p < num_paths; ++p) e.paths.emplace_back("c" + std::to_string(first_id + k) + "_path" + std::to_string(p));
        e.total_count = 10.0 + 5000.0 * unit(rng);
        uint32_t left = k % 4 == 0 ? N : rng() % (N + 1);   // S_k = N for every fourth cluster: no tail
        const uint32_t blocks = k % 5 == 3 ? 0 : 1 + rng() % 4;
        for (uint32_t i = 0; i < blocks; ++i) {
            CountSamples count_samples;
            for (uint32_t p = 0; p < num_paths; ++p) {
                if (rng() % 2 || (p + 1 == num_paths && count_samples.path_ids.empty())) count_samples.path_ids.push_back(p);
            }
            const uint32_t n = i + 1 == blocks ? (k % 4 == 0 ? left : left / 2) : (i % 2 ? 0 : rng() % (left + 1));
            left -= n;
            for (uint32_t s = 0; s < n; ++s) {
                count_samples.noise_samples.push_back(0.001 + 300.0 * unit(rng));
                for (size_t j = 0; j < count_samples.path_ids.size(); ++j) count_samples.abundance_samples.push_back(rng() % 7 == 0 ? 0.0 : 1e-3 + 1e5 * unit(rng) * unit(rng));
            }
            e.gibbs_read_count_samples.push_back(count_samples);
        }
        list.emplace_back(first_id + 7 * k, e);
    }
    return list;
}

static void dumpContainers(const std::string & filename, const ClusterEstimatesList & list) {
    std::FILE * out = std::fopen(filename.c_str(), "w");
    if (!out) std::exit(1);
    for (auto & entry : list) {
        std::fprintf(out, "cluster %u %zu %.17g\n", entry.first, entry.second.paths.size(), entry.second.total_count);
        for (auto & path : entry.second.paths) std::fprintf(out, "path %s\n", path.name.c_str());
        for (auto & count_samples : entry.second.gibbs_read_count_samples) {
            std::fprintf(out, "block %zu %zu\n", count_samples.path_ids.size(), count_samples.noise_samples.size());
            std::fprintf(out, "ids");
            for (auto id : count_samples.path_ids) std::fprintf(out, " %u", id);
            std::fprintf(out, "\nnoise");
            for (auto x : count_samples.noise_samples) std::fprintf(out, " %.17g", x);
            std::fprintf(out, "\nabund");
            for (auto x : count_samples.abundance_samples) std::fprintf(out, " %.17g", x);
            std::fprintf(out, "\n");
        }
    }
    std::fclose(out);
}

int main(int argc, char ** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "gibbs_writer_check <directory>\n");
        return 2;
    }
    const std::string dir(argv[1]);
    std::mt19937 rng(20262);
    const uint32_t N = 11;
    {
        g_case = "one table";
        const ClusterEstimatesList list = makeList(rng, N, 23, 3);
        FlatGibbs flat;
        for (auto & entry : list) flat.add(entry.first, entry.second);
        const HostTable table(flat, N);
        size_t empty_blocks = 0, listed = 0;
        for (size_t b = 0; b + 1 < flat.noise_off.size(); ++b) empty_blocks += flat.noise_off[b] == flat.noise_off[b + 1];
        for (auto x : table.listed) listed += x;
        REQUIRE(empty_blocks > 0 && listed > 20 && listed < table.listed.size());
        ReadCountGibbsSamplesWriter a(dir + "/one_samples", N), b(dir + "/one_table", N);
        for (auto & entry : list) a.addSamples(forWriter(entry));
        b.addTable(table.view, flat.labels);
        a.addNoiseTranscript(11);
        b.addNoiseTranscript(11);
        a.close();
        b.close();
        const std::string want = slurp(dir + "/one_samples.txt.gz");
        REQUIRE(want.size() > 100 && want == slurp(dir + "/one_table.txt.gz"));
        const std::string text = gunzip(dir + "/one_table.txt.gz");
        REQUIRE(text.size() > 1000 && text == gunzip(dir + "/one_samples.txt.gz") && text.find("\nUnknown\t0\t") != std::string::npos);
        dumpContainers(dir + "/one_table_containers.txt", list);

        // a view of another number of samples, labels of another size
        ReadCountGibbsSamplesWriter other(dir + "/refused", N + 1);
        bool thrown = false;
        try {
            other.addTable(table.view, flat.labels);
        } catch (const EngineError &) {
            thrown = true;
        }
        REQUIRE(thrown);
        TableLabels fewer = flat.labels;
        fewer.names.pop_back();
        ReadCountGibbsSamplesWriter short_labels(dir + "/refused_labels", N);
        thrown = false;
        try {
            short_labels.addTable(table.view, fewer);
        } catch (const EngineError &) {
            thrown = true;
        }
        REQUIRE(thrown);
    }
    {
        g_case = "two tables";
        ClusterEstimatesList first = makeList(rng, N, 9, 100), second = makeList(rng, N, 8, 500);
        // column 0: the first batch leaves 1e16, the second adds 1.0 twice.  addSamples(): (1e16 + 1.0) + 1.0 = 1e16 (each 1.0 is half
        // a unit in the last place and rounds away); two tables: 1e16 + (1.0 + 1.0) = 1e16 + 2.
        for (auto & entry : first) {
            entry.second.total_count = 0.0;
            for (auto & count_samples : entry.second.gibbs_read_count_samples) {
                for (auto & x : count_samples.noise_samples) x = 0.0;
            }
        }
        first[0].second.gibbs_read_count_samples.clear();
        first[0].second.total_count = 1e16;
        for (size_t k = 0; k < second.size(); ++k) {
            second[k].second.gibbs_read_count_samples.clear();
            second[k].second.total_count = k < 2 ? 1.0 : 0.0;
        }
        FlatGibbs flat_first, flat_second;
        for (auto & entry : first) flat_first.add(entry.first, entry.second);
        for (auto & entry : second) flat_second.add(entry.first, entry.second);
        const HostTable table_first(flat_first, N), table_second(flat_second, N);
        double chain = 0.0;
        for (auto & entry : first) chain += forWriter(entry).second.gibbs_read_count_samples.empty() ? entry.second.total_count : 0.0;
        for (auto & entry : second) chain += entry.second.total_count;
        const double joined = (0.0 + table_first.noise_counts[0]) + table_second.noise_counts[0];
        REQUIRE(chain == 1e16 && joined == 1e16 + 2.0 && chain != joined);   // the caveat: another order, another last digit
        ReadCountGibbsSamplesWriter a(dir + "/two_samples", N), b(dir + "/two_tables", N);
        for (auto & entry : first) a.addSamples(forWriter(entry));
        for (auto & entry : second) a.addSamples(forWriter(entry));
        b.addTable(table_first.view, flat_first.labels);
        b.addTable(table_second.view, flat_second.labels);
        a.addNoiseTranscript(0);
        b.addNoiseTranscript(0);
        a.close();
        b.close();
        const std::string want = gunzip(dir + "/two_samples.txt.gz"), got = gunzip(dir + "/two_tables.txt.gz");
        const size_t unknown = want.find("\nUnknown\t0\t");
        REQUIRE(unknown != std::string::npos && unknown > 500 && got.compare(0, unknown, want, 0, unknown) == 0);   // every path row
    }
    std::printf("ok\n");
    return 0;
}
