// The writers' addTable() (rpvg_amd/host/io/estimates_writers.cpp) against their addEstimates(): the same containers written both
// ways must give the same bytes, for the three writers and ploidy 1, 2 and 3.  The table the GPU would build is filled here by
// simple loops of this file's own (test code: the product has no host computation of the table).  Built with AddressSanitizer and
// UBSan as a program of its own; prints "ok".
//   estimates_writers_check <directory for the files>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>

#include "estimates_table.hpp"
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

// the arrays of rpvg_estimates_table_view from the containers, by the loops rpvg_table.h states
struct HostTable {
    std::vector<double> haplotype_prob, read_count, transcript_count, tpm, member_transcript_count, member_tpm, cluster_transcript_count;
    rpvg_estimates_table_view view;

    HostTable(const std::vector<PathClusterEstimates> & estimates, const uint32_t ploidy, const double denominator) {
        double total = 0.0, noise_total = 0.0, share_total = 0.0;
        for (auto & e : estimates) {
            std::vector<double> prob(e.paths.size(), 0.0), count(e.paths.size(), 0.0);
            double part = 0.0;
            size_t a = 0;
            for (size_t i = 0; i < e.path_group_sets.size(); ++i) {
                const auto & set = e.path_group_sets[i];
                for (size_t j = 0; j < set.size(); ++j, ++a) {
                    if (j == 0 || set[j] != set[j - 1]) prob[set[j]] += e.posteriors[i];
                    count[set[j]] += e.abundances[a];
                    const double eff = e.paths[set[j]].effective_length;
                    member_transcript_count.push_back(eff > 0 ? e.abundances[a] / eff : 0.0);
                    if (eff > 0) part += e.abundances[a] / eff;
                }
            }
            for (size_t p = 0; p < e.paths.size(); ++p) {
                haplotype_prob.push_back(prob[p]);
                read_count.push_back(count[p]);
                transcript_count.push_back(e.paths[p].effective_length > 0 ? count[p] / e.paths[p].effective_length : 0.0);
            }
            cluster_transcript_count.push_back(part);
            total += part;
            noise_total += e.noise_count;
            share_total += e.noise_count / ploidy;
        }
        for (double x : transcript_count) tpm.push_back(x / denominator * 1e6);
        for (double x : member_transcript_count) member_tpm.push_back(x / denominator * 1e6);
        view = rpvg_estimates_table_view();
        view.num_clusters = estimates.size();
        view.num_paths = haplotype_prob.size();
        view.num_members = member_tpm.size();
        view.haplotype_prob = haplotype_prob.data();
        view.read_count = read_count.data();
        view.transcript_count = transcript_count.data();
        view.tpm = tpm.data();
        view.member_transcript_count = member_transcript_count.data();
        view.member_tpm = member_tpm.data();
        view.cluster_transcript_count = cluster_transcript_count.data();
        view.total_transcript_count = total;
        view.noise_count_total = noise_total;
        view.noise_count_share_total = share_total;
        view.tpm_denominator = denominator;
        view.has_tpm = 1;
        view.ploidy = ploidy;
    }
};

// clusters of random sizes; sets of 1 .. ploidy sorted paths (one_per_path: set i is {i}, what `transcripts` leaves)
static std::vector<PathClusterEstimates> makeEstimates(std::mt19937 & rng, const uint32_t ploidy, const bool one_per_path) {
    std::vector<PathClusterEstimates> estimates(7);
    std::uniform_real_distribution<double> unit(0.0, 1.0);
    for (size_t k = 0; k < estimates.size(); ++k) {
        auto & e = estimates[k];
        const uint32_t num_paths = k == 3 ? 1 : 2 + rng() % 9;
        for (uint32_t p = 0; p < num_paths; ++p) {
            PathInfo path("c" + std::to_string(k) + "_path" + std::to_string(p));
            path.length = 200 + rng() % 5000;
            path.effective_length = (k == 2 && p == 1) ? 0.0 : 50.0 + 4000.0 * unit(rng);
            e.paths.push_back(path);
        }
        const uint32_t num_sets = one_per_path ? num_paths : (k == 5 ? 0 : 1 + rng() % 12);
        for (uint32_t i = 0; i < num_sets; ++i) {
            std::vector<uint32_t> set;
            if (one_per_path) {
                set.push_back(i);
            } else {
                const uint32_t size = 1 + rng() % ploidy;
                for (uint32_t j = 0; j < size; ++j) set.push_back(rng() % num_paths);
                std::sort(set.begin(), set.end());
            }
            // some posteriors below the joint writer's threshold
            e.posteriors.push_back(i % 5 == 4 ? 1e-12 : unit(rng));
            for (size_t j = 0; j < set.size(); ++j) e.abundances.push_back(i % 4 == 3 ? 0.0 : 700.0 * unit(rng));
            e.path_group_sets.push_back(set);
        }
        e.noise_count = 30.0 * unit(rng);
    }
    return estimates;
}

int main(int argc, char ** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "estimates_writers_check <directory>\n");
        return 2;
    }
    const std::string dir(argv[1]);
    std::mt19937 rng(20261);
    for (uint32_t ploidy = 1; ploidy <= 3; ++ploidy) {
        for (int shape = 0; shape < 2; ++shape) {
            const bool one_per_path = shape == 1;
            g_case = "ploidy " + std::to_string(ploidy) + (one_per_path ? ", one set per path" : ", sets");
            const auto estimates = makeEstimates(rng, ploidy, one_per_path);
            ClusterEstimatesList list;
            FlatEstimates flat_estimates;
            TableLabels labels;
            for (size_t k = 0; k < estimates.size(); ++k) {
                list.emplace_back(10 * k + 3, estimates[k]);
                flat_estimates.add(estimates[k]);
                labels.cluster_ids.push_back(10 * k + 3);
                for (auto & path : estimates[k].paths) {
                    labels.names.push_back(path.name);
                    labels.lengths.push_back(path.length);
                }
            }
            const double denominator = totalTranscriptCount(list);
            REQUIRE(denominator > 0);
            const HostTable table(estimates, ploidy, denominator);
            const rpvg_estimates_flat flat = flat_estimates.view();
            const std::string tag = dir + "/p" + std::to_string(ploidy) + (one_per_path ? "_one" : "_sets");
            {
                HaplotypeAbundanceEstimatesWriter a(tag + "_hap_estimates", ploidy, denominator), b(tag + "_hap_table", ploidy, denominator);
                a.addEstimates(list);
                b.addTable(flat, table.view, labels);
                a.addNoiseTranscript(11);
                b.addNoiseTranscript(11);
                a.close();
                b.close();
                const std::string want = slurp(tag + "_hap_estimates.txt");
                REQUIRE(want.size() > 100 && want == slurp(tag + "_hap_table.txt"));
            }
            {
                JointHaplotypeAbundanceEstimatesWriter a(tag + "_joint_estimates", ploidy, 1e-8, denominator), b(tag + "_joint_table", ploidy, 1e-8, denominator);
                a.addEstimates(list);
                b.addTable(flat, table.view, labels);
                a.addNoiseTranscript(11);
                b.addNoiseTranscript(11);
                a.close();
                b.close();
                const std::string want = slurp(tag + "_joint_estimates.txt");
                REQUIRE(want.size() > 100 && want == slurp(tag + "_joint_table.txt"));
                JointHaplotypeAbundanceEstimatesWriter other(tag + "_joint_other", ploidy + 1, 1e-8, denominator);
                bool thrown = false;
                try {
                    other.addTable(flat, table.view, labels);
                } catch (const EngineError &) {
                    thrown = true;
                }
                REQUIRE(thrown);  // the table's noise share is that of its own ploidy
            }
            if (one_per_path) {
                AbundanceEstimatesWriter a(tag + "_abundance_estimates", denominator), b(tag + "_abundance_table", denominator);
                a.addEstimates(list);
                b.addTable(flat, table.view, labels);
                a.addNoiseTranscript(11);
                b.addNoiseTranscript(11);
                a.close();
                b.close();
                const std::string want = slurp(tag + "_abundance_estimates.txt");
                REQUIRE(want.size() > 100 && want == slurp(tag + "_abundance_table.txt"));
            } else {
                AbundanceEstimatesWriter b(tag + "_abundance_table", denominator);
                bool thrown = false;
                try {
                    b.addTable(flat, table.view, labels);
                } catch (const EngineError &) {
                    thrown = true;
                }
                REQUIRE(thrown);
            }
        }
    }
    {
        // a set {1} at position 0: AbundanceEstimatesWriter::addTable refuses it (addEstimates would write path 1's row first)
        g_case = "set {1} at position 0";
        PathClusterEstimates e;
        for (int p = 0; p < 2; ++p) {
            PathInfo path("p" + std::to_string(p));
            path.length = 100;
            path.effective_length = 80.0;
            e.paths.push_back(path);
        }
        e.path_group_sets = {{1}, {0}};
        e.posteriors = {1.0, 1.0};
        e.abundances = {3.0, 5.0};
        FlatEstimates flat_estimates;
        flat_estimates.add(e);
        const HostTable table({e}, 2, 0.1);
        TableLabels labels;
        labels.names = {"p0", "p1"};
        labels.lengths = {100, 100};
        labels.cluster_ids = {1};
        AbundanceEstimatesWriter b(dir + "/refused", 0.1);
        bool thrown = false;
        try {
            b.addTable(flat_estimates.view(), table.view, labels);
        } catch (const EngineError & error) {
            thrown = std::string(error.what()).find("cluster 0") != std::string::npos;
        }
        REQUIRE(thrown);
        // ... and a table without TPMs, and labels of another size
        rpvg_estimates_table_view no_tpm = table.view;
        no_tpm.has_tpm = 0;
        HaplotypeAbundanceEstimatesWriter h(dir + "/refused_hap", 2, 0.1);
        thrown = false;
        try {
            h.addTable(flat_estimates.view(), no_tpm, labels);
        } catch (const EngineError &) {
            thrown = true;
        }
        REQUIRE(thrown);
        labels.names.pop_back();
        thrown = false;
        try {
            h.addTable(flat_estimates.view(), table.view, labels);
        } catch (const EngineError &) {
            thrown = true;
        }
        REQUIRE(thrown);
    }
    std::printf("ok\n");
    return 0;
}
