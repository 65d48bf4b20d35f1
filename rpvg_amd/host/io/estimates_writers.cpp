#include "estimates_writers.hpp"

#include <cassert>
#include <cmath>
#include <iomanip>
#include <limits>

#include "../hip_engine.hpp"
#include "cluster_io.hpp"
#include "../../csrc/text_deflate_plan.hpp"

namespace rpvg_amd {

// src/threaded_output_writer.cpp:6
static const uint32_t out_precision_digits = 8;

double totalTranscriptCount(const ClusterEstimatesList & path_cluster_estimates) {

    double total_transcript_count = 0;

    for (auto & cur_estimates: path_cluster_estimates) {

        auto abundances_it = cur_estimates.second.abundances.begin();

        for (auto & path_group_set: cur_estimates.second.path_group_sets) {

            for (auto & path: path_group_set) {

                assert(abundances_it != cur_estimates.second.abundances.end());

                const double path_effective_length = cur_estimates.second.paths.at(path).effective_length;

                if (path_effective_length > 0) {

                    total_transcript_count += (*abundances_it / path_effective_length);
                }

                ++abundances_it;
            }
        }
    }

    return total_transcript_count;
}

EstimatesWriter::EstimatesWriter(const std::string & filename_in) : filename(filename_in) {}

void EstimatesWriter::close() {

    if (!has_members) {

        writeTextFile(filename, out.str());
        return;
    }

    frameStream();
    rpvg_text_deflate::appendEof(framed);
    writeRawFile(filename, framed.data(), framed.size());
}

void EstimatesWriter::frameStream() {

    const std::string text = out.str();
    rpvg_text_deflate::frameMembers(text.data(), text.size(), framed);
    out.str(std::string());
}

void EstimatesWriter::appendMembers(const rpvg_text_bgzf_view & members) {

    frameStream();
    has_members = true;

    if (members.num_bytes) {

        framed.append(members.bytes, members.num_bytes);
    }
}

AbundanceEstimatesWriter::AbundanceEstimatesWriter(const std::string filename_prefix, const double total_transcript_count_in) : EstimatesWriter(filename_prefix + ".txt"), total_transcript_count(total_transcript_count_in), noise_count(0) {

    out << "Name\tClusterID\tLength\tEffectiveLength\tReadCount\tTPM" << std::endl;
}

void AbundanceEstimatesWriter::addEstimates(const ClusterEstimatesList & path_cluster_estimates) {

    out << std::setprecision(out_precision_digits);

    for (auto & cur_estimates: path_cluster_estimates) {

        const auto & estimates = cur_estimates.second;

        assert(estimates.paths.size() == estimates.path_group_sets.size());
        assert(estimates.paths.size() == estimates.abundances.size());

        for (size_t i = 0; i < estimates.path_group_sets.size(); ++i) {

            assert(estimates.path_group_sets.at(i).size() == 1);
            const auto & path = estimates.paths.at(estimates.path_group_sets.at(i).front());

            const double transcript_count = (path.effective_length > 0) ? estimates.abundances.at(i) / path.effective_length : 0;

            out << path.name << "\t" << cur_estimates.first << "\t" << path.length << "\t" << path.effective_length;
            out << "\t" << estimates.abundances.at(i) << "\t" << transcript_count / total_transcript_count * std::pow(10, 6) << std::endl;
        }

        noise_count += estimates.noise_count;
    }
}

void AbundanceEstimatesWriter::addNoiseTranscript(const uint32_t unaligned_read_count) {

    out << std::setprecision(out_precision_digits);
    out << "Unknown\t0\t0\t0\t" << noise_count + unaligned_read_count << "\t0" << std::endl;
}

HaplotypeAbundanceEstimatesWriter::HaplotypeAbundanceEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double total_transcript_count_in) : EstimatesWriter(filename_prefix + ".txt"), ploidy(ploidy_in), total_transcript_count(total_transcript_count_in), noise_count(0) {

    out << "Name\tClusterID\tLength\tEffectiveLength\tHaplotypeProbability\tReadCount\tTPM" << std::endl;
}

void HaplotypeAbundanceEstimatesWriter::addEstimates(const ClusterEstimatesList & path_cluster_estimates) {

    out << std::setprecision(out_precision_digits);

    for (auto & cur_estimates: path_cluster_estimates) {

        const auto & estimates = cur_estimates.second;
        assert(estimates.path_group_sets.size() == estimates.posteriors.size());

        // per path: probability of carrying it (a homozygous set counts once) and its read count
        std::vector<double> haplotype_probs(estimates.paths.size(), 0);
        std::vector<double> read_counts(estimates.paths.size(), 0);

        auto abundances_it = estimates.abundances.begin();

        for (size_t i = 0; i < estimates.path_group_sets.size(); ++i) {

            const auto & path_group_set = estimates.path_group_sets.at(i);
            assert(!path_group_set.empty() && path_group_set.size() <= ploidy);

            for (size_t j = 0; j < path_group_set.size(); ++j) {

                if (j == 0 || path_group_set.at(j) != path_group_set.at(j - 1)) {

                    haplotype_probs.at(path_group_set.at(j)) += estimates.posteriors.at(i);
                }

                read_counts.at(path_group_set.at(j)) += *abundances_it;
                ++abundances_it;
            }
        }

        assert(abundances_it == estimates.abundances.end());

        for (size_t i = 0; i < estimates.paths.size(); ++i) {

            const auto & path = estimates.paths.at(i);
            const double transcript_count = (path.effective_length > 0) ? read_counts.at(i) / path.effective_length : 0;

            out << path.name << "\t" << cur_estimates.first << "\t" << path.length << "\t" << path.effective_length;
            out << "\t" << haplotype_probs.at(i) << "\t" << read_counts.at(i) << "\t" << transcript_count / total_transcript_count * std::pow(10, 6) << std::endl;
        }

        noise_count += estimates.noise_count;
    }
}

void HaplotypeAbundanceEstimatesWriter::addNoiseTranscript(const uint32_t unaligned_read_count) {

    out << std::setprecision(out_precision_digits);
    out << "Unknown\t0\t0\t0\t0\t" << noise_count + unaligned_read_count << "\t0" << std::endl;
}

JointHaplotypeAbundanceEstimatesWriter::JointHaplotypeAbundanceEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double min_posterior_in, const double total_transcript_count_in) : EstimatesWriter(filename_prefix + ".txt"), ploidy(ploidy_in), min_posterior(min_posterior_in), total_transcript_count(total_transcript_count_in), noise_counts(ploidy_in, 0) {

    for (uint32_t i = 0; i < ploidy; ++i) {

        out << "Name_" << i + 1 << "\t";
    }

    out << "ClusterID\tHaplotypingProbability";

    for (uint32_t i = 0; i < ploidy; ++i) {

        out << "\tReadCount_" << i + 1 << "\tTPM_" << i + 1;
    }

    out << std::endl;
}

void JointHaplotypeAbundanceEstimatesWriter::addEstimates(const ClusterEstimatesList & path_cluster_estimates) {

    out << std::setprecision(out_precision_digits);

    for (auto & cur_estimates: path_cluster_estimates) {

        const auto & estimates = cur_estimates.second;
        assert(estimates.posteriors.size() == estimates.path_group_sets.size());

        auto abundances_it = estimates.abundances.begin();

        for (size_t i = 0; i < estimates.path_group_sets.size(); ++i) {

            const auto & path_group_set = estimates.path_group_sets.at(i);
            assert(!path_group_set.empty() && path_group_set.size() <= ploidy);

            if (estimates.posteriors.at(i) < min_posterior) {

                // not reported; its abundances are skipped (the reference would trip its end-of-abundances
                // assert here, src/threaded_output_writer.cpp:511 — sets this improbable do not occur there)
                abundances_it += path_group_set.size();
                continue;
            }

            for (auto & path: path_group_set) {

                out << estimates.paths.at(path).name << "\t";
            }

            for (size_t j = path_group_set.size(); j < ploidy; ++j) {

                out << ".\t";
            }

            out << cur_estimates.first << "\t" << estimates.posteriors.at(i);

            for (auto & path: path_group_set) {

                const double path_effective_length = estimates.paths.at(path).effective_length;
                const double transcript_count = (path_effective_length > 0) ? *abundances_it / path_effective_length : 0;

                out << "\t" << *abundances_it << "\t" << transcript_count / total_transcript_count * std::pow(10, 6);
                ++abundances_it;
            }

            for (size_t j = path_group_set.size(); j < ploidy; ++j) {

                out << "\t0\t0";
            }

            out << std::endl;
        }

        assert(abundances_it == estimates.abundances.end());

        // the cluster's noise is spread evenly over the ploidy columns of the Unknown row
        for (auto & noise_count: noise_counts) {

            noise_count += estimates.noise_count / noise_counts.size();
        }
    }
}

void JointHaplotypeAbundanceEstimatesWriter::addNoiseTranscript(const uint32_t unaligned_read_count) {

    out << std::setprecision(out_precision_digits);

    for (uint32_t i = 0; i < ploidy; ++i) {

        out << "Unknown\t";
    }

    out << "0\t0";

    for (auto & noise_count: noise_counts) {

        out << "\t" << noise_count + static_cast<float>(unaligned_read_count) / noise_counts.size() << "\t0";
    }

    out << std::endl;
}

// ---- the same rows from the estimates table of the GPU (include/rpvg_table.h) ------------------------------------------------

// what every addTable() requires of its arguments; `what` names the writer
static void requireTable(const char * what, const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels) {

    const std::string writer(what);

    if (estimates.on_device) {

        throw EngineError(writer + "::addTable: the estimates are device memory");
    }

    if (estimates.num_clusters != table.num_clusters || estimates.num_paths != table.num_paths || estimates.num_members != table.num_members) {

        throw EngineError(writer + "::addTable: the table is not that of the estimates");
    }

    if (!table.has_tpm) {

        throw EngineError(writer + "::addTable: the table has no TPMs yet (EstimatesTable::tpm)");
    }

    if (labels.names.size() != table.num_paths || labels.lengths.size() != table.num_paths || labels.cluster_ids.size() != table.num_clusters) {

        throw EngineError(writer + "::addTable: one name and length per path and one ClusterID per cluster");
    }
}

// the first member and the first abundance of cluster k; throws for a cluster with sets and no abundances (the `haplotypes` model
// has a writer of its own)
static void clusterRanges(const char * what, const rpvg_estimates_flat & estimates, const uint32_t k, uint64_t * first_member, uint64_t * first_abundance) {

    *first_member = estimates.member_off[estimates.set_off[k]];
    *first_abundance = estimates.abund_off[k];

    const uint64_t num_members = estimates.member_off[estimates.set_off[k + 1]] - *first_member;

    if (estimates.abund_off[k + 1] - *first_abundance != num_members) {

        throw EngineError(std::string(what) + "::addTable: cluster " + std::to_string(k) + " does not have one abundance per set member");
    }
}

void AbundanceEstimatesWriter::addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels) {

    requireTable("AbundanceEstimatesWriter", estimates, table, labels);

    // every cluster is checked before a row is written
    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        uint64_t first_member = 0, first_abundance = 0;
        clusterRanges("AbundanceEstimatesWriter", estimates, k, &first_member, &first_abundance);

        const uint64_t num_paths = estimates.cluster_path_off[k + 1] - estimates.cluster_path_off[k];
        const uint64_t first_set = estimates.set_off[k];
        bool one_set_per_path = estimates.set_off[k + 1] - first_set == num_paths;

        for (uint64_t i = 0; one_set_per_path && i < num_paths; ++i) {

            one_set_per_path = estimates.member_off[first_set + i + 1] - estimates.member_off[first_set + i] == 1 && estimates.members[estimates.member_off[first_set + i]] == i;
        }

        if (!one_set_per_path) {

            throw EngineError("AbundanceEstimatesWriter::addTable: cluster " + std::to_string(k) + ": set i is not {i} for every path i");
        }
    }

    out << std::setprecision(out_precision_digits);

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        const uint64_t first_path = estimates.cluster_path_off[k];
        const uint64_t num_paths = estimates.cluster_path_off[k + 1] - first_path;
        const uint64_t first_member = estimates.member_off[estimates.set_off[k]];
        const uint64_t first_abundance = estimates.abund_off[k];

        for (uint64_t i = 0; i < num_paths; ++i) {

            out << labels.names[first_path + i] << "\t" << labels.cluster_ids[k] << "\t" << labels.lengths[first_path + i] << "\t" << estimates.path_effective_length[first_path + i];
            out << "\t" << estimates.abundances[first_abundance + i] << "\t" << table.member_tpm[first_member + i] << std::endl;
        }
    }

    noise_count += table.noise_count_total;
}

// what the two estimates writers' addText() require of their arguments
static void requireText(const char * what, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) {

    if (!table.has_tpm) {

        throw EngineError(std::string(what) + "::addText: the table has no TPMs yet (EstimatesTable::tpm)");
    }

    if (text.num_paths != table.num_paths || (text.num_bytes > 0 && !text.bytes)) {

        throw EngineError(std::string(what) + "::addText: the text is not that of the table");
    }
}

void AbundanceEstimatesWriter::addText(const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) {

    requireText("AbundanceEstimatesWriter", table, text);

    out << std::setprecision(out_precision_digits);
    out.write(text.bytes, text.num_bytes);
    noise_count += table.noise_count_total;
}

void HaplotypeAbundanceEstimatesWriter::addText(const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) {

    requireText("HaplotypeAbundanceEstimatesWriter", table, text);

    out << std::setprecision(out_precision_digits);
    out.write(text.bytes, text.num_bytes);
    noise_count += table.noise_count_total;
}

void HaplotypeAbundanceEstimatesWriter::addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels) {

    requireTable("HaplotypeAbundanceEstimatesWriter", estimates, table, labels);

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        uint64_t first_member = 0, first_abundance = 0;
        clusterRanges("HaplotypeAbundanceEstimatesWriter", estimates, k, &first_member, &first_abundance);
    }

    out << std::setprecision(out_precision_digits);

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        for (uint64_t g = estimates.cluster_path_off[k]; g < estimates.cluster_path_off[k + 1]; ++g) {

            out << labels.names[g] << "\t" << labels.cluster_ids[k] << "\t" << labels.lengths[g] << "\t" << estimates.path_effective_length[g];
            out << "\t" << table.haplotype_prob[g] << "\t" << table.read_count[g] << "\t" << table.tpm[g] << std::endl;
        }
    }

    noise_count += table.noise_count_total;
}

void JointHaplotypeAbundanceEstimatesWriter::addTable(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels) {

    requireTable("JointHaplotypeAbundanceEstimatesWriter", estimates, table, labels);

    if (table.ploidy != ploidy) {

        throw EngineError("JointHaplotypeAbundanceEstimatesWriter::addTable: the table was built for ploidy " + std::to_string(table.ploidy) + ", the writer for " + std::to_string(ploidy));
    }

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        uint64_t first_member = 0, first_abundance = 0;
        clusterRanges("JointHaplotypeAbundanceEstimatesWriter", estimates, k, &first_member, &first_abundance);

        for (uint64_t s = estimates.set_off[k]; s < estimates.set_off[k + 1]; ++s) {

            const uint64_t set_size = estimates.member_off[s + 1] - estimates.member_off[s];

            if (set_size == 0 || set_size > ploidy) {

                throw EngineError("JointHaplotypeAbundanceEstimatesWriter::addTable: cluster " + std::to_string(k) + " has a set of " + std::to_string(set_size) + " paths");
            }
        }
    }

    out << std::setprecision(out_precision_digits);

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        const uint64_t first_path = estimates.cluster_path_off[k];
        const uint64_t first_member = estimates.member_off[estimates.set_off[k]];
        const uint64_t first_abundance = estimates.abund_off[k];

        for (uint64_t s = estimates.set_off[k]; s < estimates.set_off[k + 1]; ++s) {

            if (estimates.posteriors[s] < min_posterior) {

                continue;
            }

            const uint64_t set_begin = estimates.member_off[s], set_end = estimates.member_off[s + 1];

            for (uint64_t m = set_begin; m < set_end; ++m) {

                out << labels.names[first_path + estimates.members[m]] << "\t";
            }

            for (uint64_t j = set_end - set_begin; j < ploidy; ++j) {

                out << ".\t";
            }

            out << labels.cluster_ids[k] << "\t" << estimates.posteriors[s];

            for (uint64_t m = set_begin; m < set_end; ++m) {

                out << "\t" << estimates.abundances[first_abundance + (m - first_member)] << "\t" << table.member_tpm[m];
            }

            for (uint64_t j = set_end - set_begin; j < ploidy; ++j) {

                out << "\t0\t0";
            }

            out << std::endl;
        }
    }

    for (auto & noise_count: noise_counts) {

        noise_count += table.noise_count_share_total;
    }
}

void JointHaplotypeAbundanceEstimatesWriter::addText(const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) {

    if (!table.has_tpm) {

        throw EngineError("JointHaplotypeAbundanceEstimatesWriter::addText: the table has no TPMs yet (EstimatesTable::tpm)");
    }

    if (table.ploidy != ploidy) {

        throw EngineError("JointHaplotypeAbundanceEstimatesWriter::addText: the table was built for ploidy " + std::to_string(table.ploidy) + ", the writer for " + std::to_string(ploidy));
    }

    if (text.num_paths != estimates.num_sets || estimates.num_members != table.num_members || (text.num_bytes > 0 && !text.bytes)) {

        throw EngineError("JointHaplotypeAbundanceEstimatesWriter::addText: the text is not that of the table's sets");
    }

    out << std::setprecision(out_precision_digits);
    out.write(text.bytes, text.num_bytes);

    for (auto & noise_count: noise_counts) {

        noise_count += table.noise_count_share_total;
    }
}

JointHaplotypeEstimatesWriter::JointHaplotypeEstimatesWriter(const std::string filename_prefix, const uint32_t ploidy_in, const double min_posterior_in) : EstimatesWriter(filename_prefix + ".txt"), ploidy(ploidy_in), min_posterior(min_posterior_in) {

    for (uint32_t i = 0; i < ploidy; ++i) {

        out << "Name_" << i + 1 << "\t";
    }

    out << "ClusterID\tHaplotypingProbability" << std::endl;
}

void JointHaplotypeEstimatesWriter::addEstimates(const ClusterEstimatesList & path_cluster_estimates) {

    out << std::setprecision(out_precision_digits);

    for (auto & cur_estimates: path_cluster_estimates) {

        const auto & estimates = cur_estimates.second;
        assert(estimates.posteriors.size() == estimates.path_group_sets.size());

        for (size_t i = 0; i < estimates.path_group_sets.size(); ++i) {

            const auto & path_group_set = estimates.path_group_sets.at(i);
            assert(!path_group_set.empty() && path_group_set.size() <= ploidy);

            if (estimates.posteriors.at(i) < min_posterior) {

                continue;
            }

            for (auto & path: path_group_set) {

                out << estimates.paths.at(path).name << "\t";
            }

            for (size_t j = path_group_set.size(); j < ploidy; ++j) {

                out << ".\t";
            }

            out << cur_estimates.first << "\t" << estimates.posteriors.at(i) << std::endl;
        }
    }
}

void JointHaplotypeEstimatesWriter::addTable(const rpvg_estimates_flat & estimates, const TableLabels & labels) {

    if (estimates.on_device) {

        throw EngineError("JointHaplotypeEstimatesWriter::addTable: the estimates are device memory");
    }

    if (labels.names.size() != estimates.num_paths || labels.cluster_ids.size() != estimates.num_clusters) {

        throw EngineError("JointHaplotypeEstimatesWriter::addTable: one name per path and one ClusterID per cluster");
    }

    // every cluster is checked before a row is written
    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        const uint64_t num_paths = estimates.cluster_path_off[k + 1] - estimates.cluster_path_off[k];

        for (uint64_t s = estimates.set_off[k]; s < estimates.set_off[k + 1]; ++s) {

            const uint64_t set_size = estimates.member_off[s + 1] - estimates.member_off[s];

            if (set_size == 0 || set_size > ploidy) {

                throw EngineError("JointHaplotypeEstimatesWriter::addTable: cluster " + std::to_string(k) + " has a set of " + std::to_string(set_size) + " paths");
            }

            for (uint64_t m = estimates.member_off[s]; m < estimates.member_off[s + 1]; ++m) {

                if (estimates.members[m] >= num_paths) {

                    throw EngineError("JointHaplotypeEstimatesWriter::addTable: cluster " + std::to_string(k) + " has a set member that is not one of its paths");
                }
            }
        }
    }

    out << std::setprecision(out_precision_digits);

    for (uint32_t k = 0; k < estimates.num_clusters; ++k) {

        const uint64_t first_path = estimates.cluster_path_off[k];

        for (uint64_t s = estimates.set_off[k]; s < estimates.set_off[k + 1]; ++s) {

            if (estimates.posteriors[s] < min_posterior) {

                continue;
            }

            const uint64_t set_begin = estimates.member_off[s], set_end = estimates.member_off[s + 1];

            for (uint64_t m = set_begin; m < set_end; ++m) {

                out << labels.names[first_path + estimates.members[m]] << "\t";
            }

            for (uint64_t j = set_end - set_begin; j < ploidy; ++j) {

                out << ".\t";
            }

            out << labels.cluster_ids[k] << "\t" << estimates.posteriors[s] << std::endl;
        }
    }
}

void JointHaplotypeEstimatesWriter::addText(const rpvg_estimates_flat & estimates, const rpvg_table_text_view & text) {

    if (text.num_paths != estimates.num_sets || (text.num_bytes > 0 && !text.bytes)) {

        throw EngineError("JointHaplotypeEstimatesWriter::addText: the text is not that of the estimates' sets");
    }

    out << std::setprecision(out_precision_digits);
    out.write(text.bytes, text.num_bytes);
}

ReadCountGibbsSamplesWriter::ReadCountGibbsSamplesWriter(const std::string filename_prefix, const uint32_t num_gibbs_samples_in) : EstimatesWriter(filename_prefix + ".txt.gz"), num_gibbs_samples(num_gibbs_samples_in), noise_counts(num_gibbs_samples_in, 0) {

    out << "Name\tClusterID";

    for (uint32_t i = 0; i < num_gibbs_samples; ++i) {

        out << "\tReadCountSample_" << i + 1;
    }

    out << std::endl;
}

void ReadCountGibbsSamplesWriter::addSamples(const std::pair<uint32_t, PathClusterEstimates> & path_cluster_estimate) {

    const auto & estimates = path_cluster_estimate.second;

    if (estimates.gibbs_read_count_samples.empty()) {

        // no samples for the cluster: all of its reads count as noise in every sample
        for (auto & noise_count: noise_counts) {

            noise_count += estimates.total_count;
        }

        return;
    }

    const uint32_t no_column = std::numeric_limits<uint32_t>::max();

    // column of every path inside every CountSamples of the cluster
    std::vector<std::vector<uint32_t> > path_gibbs_sampling_index(estimates.paths.size());
    uint32_t noise_count_idx = 0;

    for (size_t i = 0; i < estimates.gibbs_read_count_samples.size(); ++i) {

        const CountSamples & count_samples = estimates.gibbs_read_count_samples.at(i);

        assert(!count_samples.path_ids.empty());
        assert(count_samples.abundance_samples.size() == count_samples.path_ids.size() * count_samples.noise_samples.size());

        for (auto & noise_sample: count_samples.noise_samples) {

            noise_counts.at(noise_count_idx) += noise_sample;
            ++noise_count_idx;
        }

        for (size_t j = 0; j < count_samples.path_ids.size(); ++j) {

            auto & sampling_indices = path_gibbs_sampling_index.at(count_samples.path_ids.at(j));

            if (sampling_indices.empty()) {

                sampling_indices.assign(estimates.gibbs_read_count_samples.size(), no_column);
            }

            sampling_indices.at(i) = j;
        }
    }

    while (noise_count_idx < num_gibbs_samples) {

        noise_counts.at(noise_count_idx) += estimates.total_count;
        ++noise_count_idx;
    }

    out << std::setprecision(out_precision_digits);

    for (size_t i = 0; i < path_gibbs_sampling_index.size(); ++i) {

        const auto & sampling_indices = path_gibbs_sampling_index.at(i);

        if (sampling_indices.empty()) {

            continue;
        }

        out << estimates.paths.at(i).name << "\t" << path_cluster_estimate.first;

        uint32_t num_samples = 0;

        for (size_t j = 0; j < sampling_indices.size(); ++j) {

            const CountSamples & count_samples = estimates.gibbs_read_count_samples.at(j);
            const size_t num_paths = count_samples.path_ids.size();

            for (size_t k = 0; k < count_samples.noise_samples.size(); ++k) {

                if (sampling_indices.at(j) == no_column) {

                    out << "\t0";

                } else {

                    out << "\t" << count_samples.abundance_samples.at(k * num_paths + sampling_indices.at(j));
                }

                ++num_samples;
            }
        }

        while (num_samples < num_gibbs_samples) {

            out << "\t0";
            ++num_samples;
        }

        out << std::endl;
    }
}

void ReadCountGibbsSamplesWriter::addTable(const rpvg_gibbs_table_view & table, const TableLabels & labels) {

    if (table.num_gibbs_samples != num_gibbs_samples) {

        throw EngineError("ReadCountGibbsSamplesWriter::addTable: the table has " + std::to_string(table.num_gibbs_samples) + " samples per path, the writer " + std::to_string(num_gibbs_samples));
    }

    if (labels.names.size() != table.num_paths || labels.cluster_ids.size() != table.num_clusters || !table.cluster_path_off || table.cluster_path_off[table.num_clusters] != table.num_paths) {

        throw EngineError("ReadCountGibbsSamplesWriter::addTable: one name per path and one ClusterID per cluster");
    }

    for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

        noise_counts.at(idx) += table.noise_counts[idx];
    }

    out << std::setprecision(out_precision_digits);

    for (uint32_t k = 0; k < table.num_clusters; ++k) {

        for (uint64_t g = table.cluster_path_off[k]; g < table.cluster_path_off[k + 1]; ++g) {

            if (!table.listed[g]) {

                continue;
            }

            out << labels.names.at(g) << "\t" << labels.cluster_ids.at(k);

            const double * row = table.samples + g * static_cast<uint64_t>(num_gibbs_samples);

            for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

                out << "\t" << row[idx];
            }

            out << std::endl;
        }
    }
}

void ReadCountGibbsSamplesWriter::addText(const rpvg_gibbs_table_view & table, const rpvg_table_text_view & text) {

    if (table.num_gibbs_samples != num_gibbs_samples) {

        throw EngineError("ReadCountGibbsSamplesWriter::addText: the table has " + std::to_string(table.num_gibbs_samples) + " samples per path, the writer " + std::to_string(num_gibbs_samples));
    }

    if (text.num_paths != table.num_paths || (text.num_bytes > 0 && !text.bytes)) {

        throw EngineError("ReadCountGibbsSamplesWriter::addText: the text is not that of the table");
    }

    for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

        noise_counts.at(idx) += table.noise_counts[idx];
    }

    out << std::setprecision(out_precision_digits);
    out.write(text.bytes, text.num_bytes);
}

void ReadCountGibbsSamplesWriter::addCompressedText(const rpvg_gibbs_table_view & table, const rpvg_table_text_view & text, const rpvg_text_bgzf_view & members) {

    if (table.num_gibbs_samples != num_gibbs_samples) {

        throw EngineError("ReadCountGibbsSamplesWriter::addCompressedText: the table has " + std::to_string(table.num_gibbs_samples) + " samples per path, the writer " + std::to_string(num_gibbs_samples));
    }

    if (text.num_paths != table.num_paths) {  // (the text's bytes are not read: a view of its sizes alone will do)

        throw EngineError("ReadCountGibbsSamplesWriter::addCompressedText: the text is not that of the table");
    }

    if (members.num_text_bytes != text.num_bytes || (members.num_bytes > 0 && !members.bytes)) {

        throw EngineError("ReadCountGibbsSamplesWriter::addCompressedText: the members are not those of the text");
    }

    for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

        noise_counts.at(idx) += table.noise_counts[idx];
    }

    appendMembers(members);
}

void ReadCountGibbsSamplesWriter::addNoiseTranscript(const uint32_t unaligned_read_count) {

    out << std::setprecision(out_precision_digits);
    out << "Unknown\t0";

    for (auto & noise_count: noise_counts) {

        out << "\t" << noise_count + unaligned_read_count;
    }

    out << std::endl;
}

}
