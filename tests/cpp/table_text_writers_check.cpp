// addText() of the three writers (rpvg_amd/host/io/estimates_writers.cpp) against their addTable(): for views built by hand the file
// written through addText() from the host line (rpvg_amd/host/table_text.hpp: the kernels' row descriptors on one thread) is the
// file of addTable(), byte for byte, the `Unknown` row included.  Built with AddressSanitizer and UBSan as a program of its own;
// prints "ok".
//   table_text_writers_check <directory for the files>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "io/estimates_writers.hpp"
#include "table_text.hpp"

using namespace rpvg_amd;

static void require(const bool condition, const char * what) {
    if (!condition) {
        std::printf("failed: %s\n", what);
        std::exit(1);
    }
}

static std::string slurp(const std::string & filename) {
    std::ifstream in(filename, std::ios::binary);
    std::stringstream text;
    text << in.rdbuf();
    return text.str();
}

static rpvg_table_text_view viewOf(const HostLine & line, const uint64_t num_paths) {
    rpvg_table_text_view view = {};
    view.num_paths = num_paths;
    view.num_bytes = line.bytes.size();
    view.row_off = line.row_off.data();
    view.bytes = line.bytes.data();
    for (uint64_t r = 0; r < num_paths; ++r) view.num_rows += line.row_off[r + 1] > line.row_off[r] ? 1 : 0;
    return view;
}

int main(int argc, char ** argv) {
    require(argc == 2, "one argument: a directory");
    const std::string dir = std::string(argv[1]) + "/";

    // three clusters of 2, 0 and 3 paths
    TableLabels labels;
    labels.names = {"tx_a", "", "hap|3", "x", std::string(300, 'n')};
    labels.lengths = {1000, 20, 4294967295u, 1, 77};
    labels.cluster_ids = {7, 8, 4000000000u};
    const std::vector<uint64_t> cluster_path_off = {0, 2, 2, 5};
    const FlatLabels flat_labels(labels);
    const rpvg_table_labels flat = flat_labels.view();
    const double quiet_nan = std::nan("");

    {  // the Gibbs file: N = 70 (more than a wavefront's step), the second path of the last cluster not listed
        const uint32_t N = 70;
        std::vector<double> samples(5 * N), noise(N);
        for (size_t i = 0; i < samples.size(); ++i) samples[i] = i % 7 == 0 ? 0.0 : (i % 11 == 0 ? 10000000.5 + static_cast<double>(i % 2) : 0.37 * static_cast<double>(i) * (i % 5 == 0 ? 1e-9 : 1.0));
        samples[3] = -0.0;
        samples[4] = quiet_nan;
        samples[5] = -quiet_nan;
        samples[6] = 5e-324;
        for (uint32_t s = 0; s < N; ++s) noise[s] = 0.125 * s + 3;
        const std::vector<uint8_t> listed = {1, 1, 1, 0, 1};
        rpvg_gibbs_table_view table = {};
        table.num_clusters = 3;
        table.num_paths = 5;
        table.num_gibbs_samples = N;
        table.samples = samples.data();
        table.listed = listed.data();
        table.noise_counts = noise.data();
        table.cluster_path_off = cluster_path_off.data();
        const HostLine line = hostLine(gibbsTextRows(table, flat, 8));
        require(line.exact_cells > 0, "the Gibbs case holds ties");
        ReadCountGibbsSamplesWriter by_table(dir + "gibbs_table", N), by_text(dir + "gibbs_text", N);
        by_table.addTable(table, labels);
        by_table.addNoiseTranscript(5);
        by_table.close();
        by_text.addText(table, viewOf(line, 5));
        by_text.addNoiseTranscript(5);
        by_text.close();
        const std::string want = slurp(dir + "gibbs_table.txt.gz");
        require(want.size() > 100 && slurp(dir + "gibbs_text.txt.gz") == want, "the Gibbs file of addText is the file of addTable");
    }

    {  // the two estimates files: set i = {i}
        rpvg_estimates_flat estimates = {};
        const std::vector<uint64_t> set_off = {0, 2, 2, 5}, member_off = {0, 1, 2, 3, 4, 5}, abund_off = {0, 2, 2, 5};
        const std::vector<uint32_t> members = {0, 1, 0, 1, 2};
        const std::vector<double> posteriors = {1, 1, 1, 1, 1}, abundances = {1.5, 0.0, 123456785.0, 2.5e-10, 99999999.5}, noise_count = {0.5, 0.25, 3.0};
        const std::vector<double> eff = {812.25, 1e-7, 0.0, 123456.78, 1e9};
        estimates.num_clusters = 3;
        estimates.num_sets = 5;
        estimates.num_members = 5;
        estimates.num_abundances = 5;
        estimates.num_paths = 5;
        estimates.set_off = set_off.data();
        estimates.member_off = member_off.data();
        estimates.members = members.data();
        estimates.posteriors = posteriors.data();
        estimates.abund_off = abund_off.data();
        estimates.abundances = abundances.data();
        estimates.noise_count = noise_count.data();
        estimates.cluster_path_off = cluster_path_off.data();
        estimates.path_effective_length = eff.data();
        const std::vector<double> prob = {1.0, 1.0 / 3.0, 0.0, 0.5, 1e-300}, count = {12.0, 99999999.5, 0.0, 1e15, 2.5}, tpm = {1e6, 0.125, 0.0, 123456795.0, 1e-5};
        const std::vector<double> member_tpm = {250000.0, 0.0, 1.0 / 3.0, 1e6, 0.0000999999995};
        rpvg_estimates_table_view table = {};
        table.num_clusters = 3;
        table.num_paths = 5;
        table.num_members = 5;
        table.haplotype_prob = prob.data();
        table.read_count = count.data();
        table.tpm = tpm.data();
        table.member_tpm = member_tpm.data();
        table.noise_count_total = 3.75;
        table.tpm_denominator = 8.0;
        table.has_tpm = 1;
        table.ploidy = 2;
        std::vector<uint64_t> member_base;
        {
            const HostLine line = hostLine(estimatesTextRows(estimates, table, flat, RPVG_TEXT_PER_PATH, 8, &member_base));
            AbundanceEstimatesWriter by_table(dir + "abundance_table", 8.0), by_text(dir + "abundance_text", 8.0);
            by_table.addTable(estimates, table, labels);
            by_table.addNoiseTranscript(5);
            by_table.close();
            by_text.addText(table, viewOf(line, 5));
            by_text.addNoiseTranscript(5);
            by_text.close();
            const std::string want = slurp(dir + "abundance_table.txt");
            require(want.size() > 100 && slurp(dir + "abundance_text.txt") == want, "the abundance file of addText is the file of addTable");
        }
        {
            const HostLine line = hostLine(estimatesTextRows(estimates, table, flat, RPVG_TEXT_HAPLOTYPE, 8, &member_base));
            HaplotypeAbundanceEstimatesWriter by_table(dir + "haplotype_table", 2, 8.0), by_text(dir + "haplotype_text", 2, 8.0);
            by_table.addTable(estimates, table, labels);
            by_table.addNoiseTranscript(5);
            by_table.close();
            by_text.addText(table, viewOf(line, 5));
            by_text.addNoiseTranscript(5);
            by_text.close();
            const std::string want = slurp(dir + "haplotype_table.txt");
            require(want.size() > 100 && slurp(dir + "haplotype_text.txt") == want, "the haplotype file of addText is the file of addTable");
            rpvg_table_text_view other = viewOf(line, 5);
            other.num_paths = 4;
            bool refused = false;
            try {
                by_text.addText(table, other);
            } catch (const std::exception &) {
                refused = true;
            }
            require(refused, "a text of another number of paths is refused");
        }
    }
    std::printf("ok\n");
    return 0;
}
