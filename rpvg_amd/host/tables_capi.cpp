// C entry points of the harness for the two output tables of a prepared batch: the estimates table (estimates_table.hpp;
// include/rpvg_table.h) and the Gibbs samples table (gibbs_samples_table.hpp; include/rpvg_samples.h), each beside the same file
// or table made from the containers by the writers' own loops, and the text of their rows formatted on the GPU (table_text.hpp;
// include/rpvg_text.h) beside the same rows from one host thread.  Nothing here runs a batch (runner_capi.cpp does).

#include <algorithm>
#include <chrono>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "estimates_table.hpp"
#include "gibbs_samples_table.hpp"
#include "io/estimates_writers.hpp"
#include "path_abundance_estimator.hpp"
#include "runner_handles.hpp"
#include "table_text.hpp"
#include "../csrc/text_deflate_plan.hpp"

using namespace rpvg_amd;
using namespace rpvg_amd_harness;

// ---- estimates table (estimates_table.hpp; include/rpvg_table.h) ------------------------------------------------------------------

namespace {

// what rpvg_amd_run_resident returns: the estimates of a prepared batch resident on the engine's GPU
struct ResidentHandle {

    ResidentEstimates estimates;
};

struct TableHandle {

    std::unique_ptr<EstimatesTable> table;
    TableLabels labels;
    uint32_t ploidy = 0;
};

// rows are called as the existing writers would call them from the prepared batch: the PathInfo's name ("c<k>_p<j>" for a batch
// that came without names) and length, ClusterID k + 1
TableLabels labelsOf(const std::vector<std::vector<PathInfo> > & paths) {

    TableLabels labels;

    for (size_t k = 0; k < paths.size(); ++k) {

        for (size_t j = 0; j < paths[k].size(); ++j) {

            labels.names.emplace_back(paths[k][j].name.empty() ? "c" + std::to_string(k) + "_p" + std::to_string(j) : paths[k][j].name);
            labels.lengths.emplace_back(paths[k][j].length);
        }

        labels.cluster_ids.emplace_back(k + 1);
    }

    return labels;
}

// the containers of a prepared batch as the writers take them, the rows called as labelsOf() calls them
template <typename Prepared>
ClusterEstimatesList labelledListOf(const Prepared & prepared) {

    const TableLabels labels = labelsOf(prepared.paths);
    ClusterEstimatesList list;
    size_t g = 0;

    for (size_t k = 0; k < prepared.estimates.size(); ++k) {

        list.emplace_back(labels.cluster_ids[k], prepared.estimates[k]);

        for (auto & path: list.back().second.paths) {

            path.name = labels.names[g];
            ++g;
        }
    }

    return list;
}

// "abundance": <prefix>.txt of AbundanceEstimatesWriter; "haplotype": <prefix>.txt of HaplotypeAbundanceEstimatesWriter; "joint":
// <prefix>_joint.txt of JointHaplotypeAbundanceEstimatesWriter; "posterior": <prefix>.txt of JointHaplotypeEstimatesWriter, which has no
// `Unknown` row.  add(writer) adds the rows.
template <typename AddRows>
void writeWith(const std::string & writer, const uint32_t ploidy, const double min_posterior, const double denominator, const std::string & prefix, const uint32_t unaligned_read_count, AddRows add) {

    if (writer == "abundance") {

        AbundanceEstimatesWriter out(prefix, denominator);
        add(out);
        out.addNoiseTranscript(unaligned_read_count);
        out.close();

    } else if (writer == "haplotype") {

        HaplotypeAbundanceEstimatesWriter out(prefix, ploidy, denominator);
        add(out);
        out.addNoiseTranscript(unaligned_read_count);
        out.close();

    } else if (writer == "joint") {

        JointHaplotypeAbundanceEstimatesWriter out(prefix + "_joint", ploidy, min_posterior, denominator);
        add(out);
        out.addNoiseTranscript(unaligned_read_count);
        out.close();

    } else if (writer == "posterior") {

        JointHaplotypeEstimatesWriter out(prefix, ploidy, min_posterior);
        add(out);
        out.close();

    } else {

        throw std::runtime_error("no such writer: " + writer);
    }
}

// addText() and addTable() of the four writers behind one signature (writeWith hands its callback any of them)
void addTextTo(AbundanceEstimatesWriter & out, const rpvg_estimates_flat &, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) { out.addText(table, text); }
void addTextTo(HaplotypeAbundanceEstimatesWriter & out, const rpvg_estimates_flat &, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) { out.addText(table, text); }
void addTextTo(JointHaplotypeAbundanceEstimatesWriter & out, const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const rpvg_table_text_view & text) { out.addText(estimates, table, text); }
void addTextTo(JointHaplotypeEstimatesWriter & out, const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view &, const rpvg_table_text_view & text) { out.addText(estimates, text); }

template <typename Writer>
void addTableTo(Writer & out, const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view & table, const TableLabels & labels) { out.addTable(estimates, table, labels); }
void addTableTo(JointHaplotypeEstimatesWriter & out, const rpvg_estimates_flat & estimates, const rpvg_estimates_table_view &, const TableLabels & labels) { out.addTable(estimates, labels); }

}

extern "C" {

// The table of the estimates of a prepared batch, built on the engine's GPU: from a result handle (rpvg_amd_run and the like)
// when there is one, else from the containers the last run on the prepared batch left in it.
void * rpvg_amd_estimates_table_build(void * engine, void * result_handle, void * prepared_batch, uint32_t ploidy) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);
        std::unique_ptr<TableHandle> handle(new TableHandle());
        handle->labels = labelsOf(prepared->paths);
        handle->ploidy = ploidy;

        if (result_handle) {

            const Result * result = static_cast<const Result *>(result_handle);

            if (result->noise_count.size() != prepared->paths.size()) {

                throw std::runtime_error("the result is not that of the prepared batch");
            }

            std::vector<uint64_t> cluster_path_off(1, 0);
            std::vector<double> effective_length;

            for (auto & paths: prepared->paths) {

                for (auto & path: paths) {

                    effective_length.emplace_back(path.effective_length);
                }

                cluster_path_off.emplace_back(effective_length.size());
            }

            rpvg_estimates_flat flat = {};
            flat.num_clusters = result->noise_count.size();
            flat.num_sets = result->posteriors.size();
            flat.num_members = result->members.size();
            flat.num_abundances = result->abundances.size();
            flat.num_paths = effective_length.size();
            flat.set_off = result->set_off.data();
            flat.member_off = result->member_off.data();
            flat.members = result->members.data();
            flat.posteriors = result->posteriors.data();
            flat.abund_off = result->abund_off.data();
            flat.abundances = result->abundances.data();
            flat.noise_count = result->noise_count.data();
            flat.cluster_path_off = cluster_path_off.data();
            flat.path_effective_length = effective_length.data();

            handle->table.reset(new EstimatesTable(static_cast<Engine *>(engine)->hip, flat, ploidy));

        } else {

            if (prepared->estimates.size() != prepared->paths.size()) {

                throw std::runtime_error("the prepared batch has no estimates yet");
            }

            handle->table.reset(new EstimatesTable(static_cast<Engine *>(engine)->hip, prepared->estimates, ploidy));
        }

        return handle.release();
    });
}

// NestedPathAbundanceEstimator::estimateBatchResident on a prepared batch: the estimates stay on the GPU and the containers of the
// prepared batch are not touched.  NULL with an empty rpvg_amd_last_error when the route is not taken (the model is not
// haplotype-transcripts, or the configuration or the batch is none the route covers): the caller runs rpvg_amd_run instead.
void * rpvg_amd_run_resident(void * engine, const char * model, const rpvg_params * params, void * prepared_batch) {

    last_error.clear();

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (!prepared->device) {

            return nullptr;
        }

        auto estimator = makePathEstimator(model, *params, static_cast<Engine *>(engine)->hip);
        NestedPathAbundanceEstimator * nested = dynamic_cast<NestedPathAbundanceEstimator *>(estimator.get());

        if (!nested) {

            return nullptr;
        }

        std::vector<double> effective_length;

        for (auto & paths: prepared->paths) {

            for (auto & path: paths) {

                effective_length.emplace_back(path.effective_length);
            }
        }

        std::unique_ptr<ResidentHandle> handle(new ResidentHandle());

        if (!nested->estimateBatchResident(&handle->estimates, *prepared->device, effective_length, &prepared->paths)) {

            return nullptr;
        }

        return handle.release();
    });
}

// host copies of the resident estimates (rpvg_hip_flat_estimates_get), valid until rpvg_amd_resident_estimates_free
int rpvg_amd_resident_estimates_get(void * resident_handle, rpvg_estimates_flat * flat_out) {

    return guardedInt([&]() -> int {

        *flat_out = static_cast<ResidentHandle *>(resident_handle)->estimates.hostView();
        return 0;
    });
}

// the bytes of the kept device block of every lane (ResidentEstimates::kept_block_bytes): the number of lanes; the first
// `capacity` of them are written
uint32_t rpvg_amd_resident_estimates_kept_bytes(void * resident_handle, uint64_t * bytes_out, uint32_t capacity) {

    const std::vector<uint64_t> & kept = static_cast<ResidentHandle *>(resident_handle)->estimates.kept_block_bytes;

    for (size_t i = 0; i < kept.size() && i < capacity; ++i) {

        bytes_out[i] = kept[i];
    }

    return kept.size();
}

void rpvg_amd_resident_estimates_free(void * resident_handle) {

    delete static_cast<ResidentHandle *>(resident_handle);
}

// The table of resident estimates, built with on_device = 1 and no flattening: a table handle like that of
// rpvg_amd_estimates_table_build (_view, _tpm, _write and the text entry points take it).  The resident estimates must outlive it.
void * rpvg_amd_estimates_table_build_resident(void * engine, void * resident_handle, void * prepared_batch, uint32_t ploidy) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);
        std::unique_ptr<TableHandle> handle(new TableHandle());
        handle->labels = labelsOf(prepared->paths);
        handle->ploidy = ploidy;
        handle->table.reset(new EstimatesTable(static_cast<Engine *>(engine)->hip, static_cast<ResidentHandle *>(resident_handle)->estimates, ploidy));

        return handle.release();
    });
}

int rpvg_amd_estimates_table_tpm(void * table_handle, double denominator) {

    return guardedInt([&]() -> int {

        static_cast<TableHandle *>(table_handle)->table->tpm(denominator);
        return 0;
    });
}

// valid until the next rpvg_amd_estimates_table_tpm or the table's end
int rpvg_amd_estimates_table_view(void * table_handle, rpvg_estimates_table_view * view_out) {

    return guardedInt([&]() -> int {

        *view_out = static_cast<TableHandle *>(table_handle)->table->view();
        return 0;
    });
}

// One of the four files from the table (after rpvg_amd_estimates_table_tpm, which "posterior" does not need): writer = "abundance",
// "haplotype", "joint" or "posterior".
int rpvg_amd_estimates_table_write(void * table_handle, const char * writer, double min_posterior, const char * output_prefix, uint32_t unaligned_read_count) {

    return guardedInt([&]() -> int {

        TableHandle * handle = static_cast<TableHandle *>(table_handle);
        const rpvg_estimates_flat estimates = handle->table->estimates();
        const rpvg_estimates_table_view & view = handle->table->view();

        writeWith(writer, handle->ploidy, min_posterior, view.tpm_denominator, output_prefix, unaligned_read_count, [&](auto & out) { addTableTo(out, estimates, view, handle->labels); });
        return 0;
    });
}

void rpvg_amd_estimates_table_free(void * table_handle) {

    delete static_cast<TableHandle *>(table_handle);
}

// The same file from the containers of the prepared batch by the writer's addEstimates(), the rows called as the table's are;
// total_transcript_count_out: totalTranscriptCount() of the containers (one running sum over all members) and seconds_out the
// time of that sum; write_seconds_out: the writer from its constructor to close().  A denominator of 0 stands for that sum.
int rpvg_amd_estimates_write_from_containers(void * prepared_batch, const char * writer, uint32_t ploidy, double min_posterior, double denominator, const char * output_prefix, uint32_t unaligned_read_count, double * total_transcript_count_out, double * seconds_out, double * write_seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (prepared->estimates.size() != prepared->paths.size()) {

            throw std::runtime_error("the prepared batch has no estimates yet");
        }

        const ClusterEstimatesList list = labelledListOf(*prepared);

        // (a `haplotypes` result has no abundances to sum: the "posterior" writer takes no denominator)
        const bool has_total = !(writer && std::string(writer) == "posterior");
        const auto start = std::chrono::steady_clock::now();
        const double total = has_total ? totalTranscriptCount(list) : 0.0;
        const auto stop = std::chrono::steady_clock::now();

        if (total_transcript_count_out) {

            *total_transcript_count_out = total;
        }

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(stop - start).count();
        }

        if (writer && writer[0]) {

            const auto write_start = std::chrono::steady_clock::now();
            writeWith(writer, ploidy, min_posterior, denominator == 0 ? total : denominator, output_prefix, unaligned_read_count, [&](auto & out) { out.addEstimates(list); });

            if (write_seconds_out) {

                *write_seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - write_start).count();
            }
        }

        return 0;
    });
}

// ---- the Gibbs samples table of a prepared batch (gibbs_samples_table.hpp) -------------------------------------------------------

// The table of the Gibbs samples the last run (-n > 0) left in the containers of the prepared batch, built on the engine's GPU; the
// rows are called as rpvg_amd_estimates_table_build calls them.  seconds_out: flattening the containers and the build.
void * rpvg_amd_gibbs_table_build(void * engine, void * prepared_batch, uint32_t num_gibbs_samples, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (prepared->estimates.size() != prepared->paths.size()) {

            throw std::runtime_error("the prepared batch has no estimates yet");
        }

        const ClusterEstimatesList list = labelledListOf(*prepared);
        const auto start = std::chrono::steady_clock::now();
        std::unique_ptr<GibbsSamplesTable> table(new GibbsSamplesTable(static_cast<Engine *>(engine)->hip, list, num_gibbs_samples));

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return table.release();
    });
}

// valid until the table's end
int rpvg_amd_gibbs_table_view(void * table_handle, rpvg_gibbs_table_view * view_out) {

    return guardedInt([&]() -> int {

        *view_out = static_cast<GibbsSamplesTable *>(table_handle)->view();
        return 0;
    });
}

// <prefix>.txt.gz from the table by ReadCountGibbsSamplesWriter::addTable
int rpvg_amd_gibbs_table_write(void * table_handle, uint32_t num_gibbs_samples, const char * output_prefix, uint32_t unaligned_read_count) {

    return guardedInt([&]() -> int {

        GibbsSamplesTable * table = static_cast<GibbsSamplesTable *>(table_handle);
        ReadCountGibbsSamplesWriter out(output_prefix, num_gibbs_samples);
        out.addTable(table->view(), table->labels());
        out.addNoiseTranscript(unaligned_read_count);
        out.close();
        return 0;
    });
}

void rpvg_amd_gibbs_table_free(void * table_handle) {

    delete static_cast<GibbsSamplesTable *>(table_handle);
}

// The same from the containers on ONE thread.  With a prefix: the file by the writer's addSamples(), cluster by cluster.  With
// samples_out [P * N], listed_out [P] and noise_counts_out [N]: the writer's loops with every stream insertion replaced by a store
// into a dense table (the host comparison of tools/gibbs_table_ab.py); seconds_out is the time of those loops alone.
int rpvg_amd_gibbs_from_containers(void * prepared_batch, uint32_t num_gibbs_samples, const char * output_prefix, uint32_t unaligned_read_count,
                                   double * samples_out, uint8_t * listed_out, double * noise_counts_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (prepared->estimates.size() != prepared->paths.size()) {

            throw std::runtime_error("the prepared batch has no estimates yet");
        }

        const ClusterEstimatesList list = labelledListOf(*prepared);

        if (output_prefix && output_prefix[0]) {

            ReadCountGibbsSamplesWriter out(output_prefix, num_gibbs_samples);

            for (auto & entry: list) {

                out.addSamples(entry);
            }

            out.addNoiseTranscript(unaligned_read_count);
            out.close();
        }

        if (samples_out && listed_out && noise_counts_out) {

            const auto start = std::chrono::steady_clock::now();
            const uint32_t no_column = std::numeric_limits<uint32_t>::max();
            uint64_t g0 = 0;

            for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

                noise_counts_out[idx] = 0;
            }

            for (auto & entry: list) {

                const auto & estimates = entry.second;
                const size_t num_paths = estimates.paths.size();
                std::fill(samples_out + g0 * num_gibbs_samples, samples_out + (g0 + num_paths) * num_gibbs_samples, 0.0);
                std::fill(listed_out + g0, listed_out + g0 + num_paths, 0);

                if (estimates.gibbs_read_count_samples.empty()) {

                    for (uint32_t idx = 0; idx < num_gibbs_samples; ++idx) {

                        noise_counts_out[idx] += estimates.total_count;
                    }

                    g0 += num_paths;
                    continue;
                }

                std::vector<std::vector<uint32_t> > path_gibbs_sampling_index(num_paths);
                uint32_t noise_count_idx = 0;

                for (size_t i = 0; i < estimates.gibbs_read_count_samples.size(); ++i) {

                    const CountSamples & count_samples = estimates.gibbs_read_count_samples.at(i);

                    for (auto & noise_sample: count_samples.noise_samples) {

                        noise_counts_out[noise_count_idx] += noise_sample;
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

                    noise_counts_out[noise_count_idx] += estimates.total_count;
                    ++noise_count_idx;
                }

                for (size_t i = 0; i < num_paths; ++i) {

                    const auto & sampling_indices = path_gibbs_sampling_index.at(i);

                    if (sampling_indices.empty()) {

                        continue;
                    }

                    listed_out[g0 + i] = 1;
                    double * row = samples_out + (g0 + i) * num_gibbs_samples;
                    uint32_t num_samples = 0;

                    for (size_t j = 0; j < sampling_indices.size(); ++j) {

                        const CountSamples & count_samples = estimates.gibbs_read_count_samples.at(j);
                        const size_t num_columns = count_samples.path_ids.size();

                        for (size_t k = 0; k < count_samples.noise_samples.size(); ++k) {

                            if (sampling_indices.at(j) != no_column) {

                                row[num_samples] = count_samples.abundance_samples.at(k * num_columns + sampling_indices.at(j));
                            }

                            ++num_samples;
                        }
                    }
                }

                g0 += num_paths;
            }

            if (seconds_out) {

                *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            }
        }

        return 0;
    });
}

// ---- the text of a table's rows (table_text.hpp; include/rpvg_text.h) -----------------------------------------------------------

namespace {

// a text and the table handle it was made from (which must outlive it)
struct TextHandle {

    std::unique_ptr<TableText> text;
    GibbsSamplesTable * gibbs = nullptr;
    TableHandle * estimates = nullptr;
    int32_t kind = 0, precision = 0;
    bool sets = false;               // a set text: kind RPVG_TEXT_JOINT or RPVG_TEXT_POSTERIOR
    uint32_t ploidy = 0;
    double min_posterior = 0;
    std::unique_ptr<HostLine> line;  // the comparison line, once it has been walked
    // a rows text (the --write-probs dump): a host copy of its arrays, made at the build from arrays and on demand from resident rows
    bool rows = false;
    Engine * engine = nullptr;
    std::unique_ptr<FlatRows> flat;
    rpvg_hip_read_rows * resident = nullptr;
    std::vector<double> effective_lengths;
    std::vector<uint64_t> num_align_lists, cluster_index;
    std::unique_ptr<FlatLabels> resident_labels;
    std::vector<uint32_t> resident_lengths;
    double prob_precision = 0;
};

// the host arrays of a rows text; for resident rows their view (seconds_out: that download, when this is the first look at them)
const FlatRows & flatRowsOf(TextHandle * handle, double * view_seconds_out) {

    const auto start = std::chrono::steady_clock::now();

    if (!handle->flat) {

        rpvg_cluster_batch view = {};
        HipEngine::check(rpvg_hip_read_rows_view(handle->engine->hip->ctx(), handle->resident, &view, nullptr, nullptr), "rpvg_hip_read_rows_view");

        if (view_seconds_out) {

            *view_seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        const uint32_t K = view.num_clusters;
        rpvg_rows_text_input input = {};
        input.num_clusters = K;
        input.num_rows = K ? view.cluster_row_off[K] : 0;
        input.num_groups = input.num_rows ? view.row_grp_off[input.num_rows] : 0;
        input.num_entries = input.num_groups ? view.grp_idx_off[input.num_groups] : 0;
        input.num_paths = K ? view.cluster_path_off[K] : 0;
        input.cluster_row_off = view.cluster_row_off;
        input.cluster_path_off = view.cluster_path_off;
        input.row_count = view.row_count;
        input.row_noise = view.row_noise;
        input.row_grp_off = view.row_grp_off;
        input.grp_prob = view.grp_prob;
        input.grp_idx_off = view.grp_idx_off;
        input.path_idx = view.path_idx;
        input.path_effective_length = handle->effective_lengths.data();
        input.num_align_lists = handle->num_align_lists.empty() ? nullptr : handle->num_align_lists.data();
        input.cluster_index = handle->cluster_index.empty() ? nullptr : handle->cluster_index.data();
        rpvg_table_labels labels = handle->resident_labels->view();
        labels.path_length = handle->resident_lengths.data();
        handle->flat.reset(new FlatRows(input, labels));
    }

    return *handle->flat;
}

// the writer's clusters of flat rows, as io_capi.cpp's clustersFromBatch builds them: one ReadPathProbabilities per row
std::vector<ProbabilityCluster> clustersOf(const FlatRows & flat, const double prob_precision) {

    std::vector<ProbabilityCluster> clusters(flat.cluster_row_off.size() - 1);

    for (size_t k = 0; k < clusters.size(); ++k) {

        for (uint64_t p = flat.cluster_path_off[k]; p < flat.cluster_path_off[k + 1]; ++p) {

            PathInfo path(flat.name_bytes.substr(flat.name_off[p], flat.name_off[p + 1] - flat.name_off[p]));
            path.length = flat.path_length[p];
            path.effective_length = flat.path_effective_length[p];
            clusters[k].paths.emplace_back(std::move(path));
        }

        for (uint64_t r = flat.cluster_row_off[k]; r < flat.cluster_row_off[k + 1]; ++r) {

            ReadPathProbabilities::PathProbs path_probs;

            for (uint64_t g = flat.row_grp_off[r]; g < flat.row_grp_off[r + 1]; ++g) {

                path_probs.emplace_back(flat.grp_prob[g], std::vector<uint32_t>(flat.path_idx.begin() + flat.grp_idx_off[g], flat.path_idx.begin() + flat.grp_idx_off[g + 1]));
            }

            clusters[k].cluster_probs.emplace_back(flat.row_count[r], flat.row_noise[r], path_probs, prob_precision);
        }

        clusters[k].has_rank_key = flat.has_rank_keys;
        clusters[k].num_align_lists = flat.has_rank_keys ? flat.num_align_lists[k] : 0;
        clusters[k].cluster_index = flat.has_rank_keys ? flat.cluster_index[k] : 0;
    }

    return clusters;
}

}

// The rows of ReadCountGibbsSamplesWriter from a table of rpvg_amd_gibbs_table_build.  seconds_out: the build of the text.
void * rpvg_amd_table_text_gibbs(void * engine, void * gibbs_table_handle, int32_t precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::unique_ptr<TextHandle> handle(new TextHandle());
        handle->gibbs = static_cast<GibbsSamplesTable *>(gibbs_table_handle);
        handle->precision = precision;
        const auto start = std::chrono::steady_clock::now();
        handle->text.reset(new TableText(static_cast<Engine *>(engine)->hip, *handle->gibbs, precision));

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return handle.release();
    });
}

// The rows of AbundanceEstimatesWriter (kind RPVG_TEXT_PER_PATH) or HaplotypeAbundanceEstimatesWriter (RPVG_TEXT_HAPLOTYPE) from a
// table of rpvg_amd_estimates_table_build, after rpvg_amd_estimates_table_tpm.
void * rpvg_amd_table_text_estimates(void * engine, void * table_handle, int32_t kind, int32_t precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::unique_ptr<TextHandle> handle(new TextHandle());
        handle->estimates = static_cast<TableHandle *>(table_handle);
        handle->kind = kind;
        handle->precision = precision;
        const auto start = std::chrono::steady_clock::now();
        handle->text.reset(new TableText(static_cast<Engine *>(engine)->hip, *handle->estimates->table, handle->estimates->labels, kind, precision));

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return handle.release();
    });
}

// The rows of JointHaplotypeAbundanceEstimatesWriter (kind RPVG_TEXT_JOINT, after rpvg_amd_estimates_table_tpm) or of
// JointHaplotypeEstimatesWriter (RPVG_TEXT_POSTERIOR) from a table of rpvg_amd_estimates_table_build: a row per path group set.
void * rpvg_amd_table_text_sets(void * engine, void * table_handle, int32_t kind, uint32_t ploidy, double min_posterior, int32_t precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::unique_ptr<TextHandle> handle(new TextHandle());
        handle->estimates = static_cast<TableHandle *>(table_handle);
        handle->kind = kind;
        handle->precision = precision;
        handle->sets = true;
        handle->ploidy = ploidy;
        handle->min_posterior = min_posterior;
        const auto start = std::chrono::steady_clock::now();
        handle->text = TableText::sets(static_cast<Engine *>(engine)->hip, *handle->estimates->table, handle->estimates->labels, kind, ploidy, min_posterior, precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return handle.release();
    });
}

// The --write-probs dump of flat rows in host memory (TableText::rows): in view() and host_line() the rows are the 2 K + R lines.
void * rpvg_amd_table_text_rows(void * engine, const rpvg_rows_text_input * input, const rpvg_table_labels * labels, double prob_precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::unique_ptr<TextHandle> handle(new TextHandle());
        handle->rows = true;
        handle->engine = static_cast<Engine *>(engine);
        handle->prob_precision = prob_precision;
        handle->flat.reset(new FlatRows(*input, *labels));
        const auto start = std::chrono::steady_clock::now();
        handle->text = TableText::rows(handle->engine->hip, *input, *labels, prob_precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return handle.release();
    });
}

// ... of rows resident on the engine's GPU (a rpvg_hip_read_rows of the engine's context, which must outlive the text): host labels
// with path_length, effective lengths [P] and rank keys [K] (both or NULL) of the rows' columns.
void * rpvg_amd_table_text_resident_rows(void * engine, void * read_rows, const rpvg_table_labels * labels, const double * path_effective_length, const uint64_t * num_align_lists, const uint64_t * cluster_index, double prob_precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::unique_ptr<TextHandle> handle(new TextHandle());
        handle->rows = true;
        handle->engine = static_cast<Engine *>(engine);
        handle->prob_precision = prob_precision;
        handle->resident = static_cast<rpvg_hip_read_rows *>(read_rows);

        if (labels->on_device || (labels->num_paths && !(labels->path_length && path_effective_length))) {

            throw std::runtime_error("host labels with path_length and effective lengths");
        }

        TableLabels kept;

        for (uint64_t p = 0; p < labels->num_paths; ++p) {

            kept.names.emplace_back(labels->name_bytes + labels->name_off[p], labels->name_bytes + labels->name_off[p + 1]);
        }

        kept.cluster_ids.assign(labels->num_clusters, 0);
        handle->resident_labels.reset(new FlatLabels(kept));
        handle->resident_lengths.assign(labels->path_length, labels->path_length + labels->num_paths);
        handle->effective_lengths.assign(path_effective_length, path_effective_length + labels->num_paths);

        if (num_align_lists && cluster_index) {

            handle->num_align_lists.assign(num_align_lists, num_align_lists + labels->num_clusters);
            handle->cluster_index.assign(cluster_index, cluster_index + labels->num_clusters);
        }

        const auto start = std::chrono::steady_clock::now();
        handle->text = TableText::rows(handle->engine->hip, handle->resident, *labels, path_effective_length, num_align_lists, cluster_index, prob_precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return handle.release();
    });
}

// The comparison line of the dump without a GPU: hostLineRows() over host arrays (valid offsets and indices are the caller's
// precondition).  bytes_out [the line's bytes] and row_off_out [2 K + R + 1] may be NULL: a first call asks for num_bytes_out.
int rpvg_amd_rows_text_host_line(const rpvg_rows_text_input * input, const rpvg_table_labels * labels, double prob_precision, char * bytes_out, uint64_t * row_off_out, uint64_t * num_bytes_out, uint64_t * exact_cells_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        const rpvg_rows_text::DumpRows rows = dumpTextRows(*input, *labels, prob_precision);
        const auto start = std::chrono::steady_clock::now();
        const HostLine line = hostLineRows(rows);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        if (num_bytes_out) {

            *num_bytes_out = line.bytes.size();
        }

        if (exact_cells_out) {

            *exact_cells_out = line.exact_cells;
        }

        if (bytes_out) {

            std::copy(line.bytes.begin(), line.bytes.end(), bytes_out);
        }

        if (row_off_out) {

            std::copy(line.row_off.begin(), line.row_off.end(), row_off_out);
        }

        return 0;
    });
}

// valid until the text's end
int rpvg_amd_table_text_view(void * text_handle, rpvg_table_text_view * view_out) {

    return guardedInt([&]() -> int {

        *view_out = static_cast<TextHandle *>(text_handle)->text->view();
        return 0;
    });
}

// The file of the text's writer through its addText(): <prefix>.txt.gz for a Gibbs text (num_gibbs_samples the writer's),
// <prefix>.txt for an estimates text (<prefix>_joint.txt for the joint set text).
int rpvg_amd_table_text_write(void * text_handle, uint32_t num_gibbs_samples, const char * output_prefix, uint32_t unaligned_read_count) {

    return guardedInt([&]() -> int {

        TextHandle * handle = static_cast<TextHandle *>(text_handle);

        if (handle->rows) {  // the dump: output_prefix is the file's name (gzip when it ends in ".gz")

            writeProbabilityClustersText(output_prefix, handle->text->view());

        } else if (handle->gibbs) {

            ReadCountGibbsSamplesWriter out(output_prefix, num_gibbs_samples);
            out.addText(handle->gibbs->view(), handle->text->view());
            out.addNoiseTranscript(unaligned_read_count);
            out.close();

        } else {

            const rpvg_estimates_table_view & view = handle->estimates->table->view();
            const rpvg_estimates_flat estimates = handle->estimates->table->estimates();
            const std::string writer = handle->sets ? (handle->kind == RPVG_TEXT_JOINT ? "joint" : "posterior") : (handle->kind == RPVG_TEXT_PER_PATH ? "abundance" : "haplotype");

            writeWith(writer, handle->sets ? handle->ploidy : handle->estimates->ploidy, handle->min_posterior, view.tpm_denominator, output_prefix, unaligned_read_count, [&](auto & out) { addTextTo(out, estimates, view, handle->text->view()); });
        }

        return 0;
    });
}

// The text as BGZF members deflated on the GPU (TableText::bgzf); valid until the text's end.  seconds_out [2], or NULL: the
// compression and the download of the members, each 0 when an earlier call had done it.
int rpvg_amd_table_text_bgzf(void * text_handle, rpvg_text_bgzf_view * view_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        TableText & text = *static_cast<TextHandle *>(text_handle)->text;
        const auto start = std::chrono::steady_clock::now();
        text.deflate();
        const auto deflated = std::chrono::steady_clock::now();
        *view_out = text.bgzf();

        if (seconds_out) {

            seconds_out[0] = std::chrono::duration<double>(deflated - start).count();
            seconds_out[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - deflated).count();
        }

        return 0;
    });
}

// rpvg_amd_table_text_write with the rows as the members the GPU deflated: <prefix>.txt.gz of a Gibbs text through the writer's
// addCompressedText(), the file `output_prefix` of the dump through writeProbabilityClustersBgzf.  The estimates files are plain text
// in the reference and have no such route.
int rpvg_amd_table_text_write_compressed(void * text_handle, uint32_t num_gibbs_samples, const char * output_prefix, uint32_t unaligned_read_count) {

    return guardedInt([&]() -> int {

        TextHandle * handle = static_cast<TextHandle *>(text_handle);

        if (handle->rows) {

            writeProbabilityClustersBgzf(output_prefix, handle->text->bgzf());

        } else if (handle->gibbs) {

            ReadCountGibbsSamplesWriter out(output_prefix, num_gibbs_samples);
            out.addCompressedText(handle->gibbs->view(), handle->text->sizes(), handle->text->bgzf());  // (the plain text is not downloaded)
            out.addNoiseTranscript(unaligned_read_count);
            out.close();

        } else {

            throw std::runtime_error("the estimates files are plain text: only the Gibbs file and the dump are written compressed");
        }

        return 0;
    });
}

// The members of any bytes by the host's model of the device's member (rpvg_amd/csrc/text_deflate_plan.hpp: modelMembers), without a
// GPU.  bytes_out may be NULL: a first call asks for num_bytes_out.
int rpvg_amd_bytes_bgzf_model(const char * bytes, uint64_t n, char * bytes_out, uint64_t * num_bytes_out, uint64_t * num_stored_out) {

    return guardedInt([&]() -> int {

        std::string members;
        uint64_t stored = 0;
        rpvg_text_deflate::modelMembers(bytes, n, members, &stored);

        if (num_bytes_out) {

            *num_bytes_out = members.size();
        }

        if (num_stored_out) {

            *num_stored_out = stored;
        }

        if (bytes_out) {

            std::copy(members.begin(), members.end(), bytes_out);
        }

        return 0;
    });
}

// The same rows from the host views of the table by one host thread: the row descriptors of the kernels walked with number_text.hpp.
// The line is kept with the handle; recompute != 0 walks again.  seconds_out: the walk alone (both passes), written when it ran.
// For a set text the line is hostLineSets() and the rows are the sets.  bytes_out [the line's bytes] and row_off_out [P + 1] may be NULL; equal_out: whether the line's bytes and offsets are the text's.
int rpvg_amd_table_text_host_line(void * text_handle, int32_t recompute, char * bytes_out, uint64_t * row_off_out, uint64_t * num_bytes_out, uint64_t * exact_cells_out, int32_t * equal_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        TextHandle * handle = static_cast<TextHandle *>(text_handle);

        if (!handle->line || recompute) {

            std::vector<uint64_t> member_base;
            rpvg_table_text::TextRows rows = {};
            rpvg_set_text::SetRows set_rows = {};
            std::unique_ptr<FlatLabels> labels;
            rpvg_estimates_flat estimates = {};
            rpvg_rows_text::DumpRows dump_rows = {};
            rpvg_rows_text_input dump_input = {};
            rpvg_table_labels dump_labels = {};

            if (handle->rows) {

                const FlatRows & flat = flatRowsOf(handle, nullptr);
                dump_input = flat.input();
                dump_labels = flat.labels();
                dump_rows = dumpTextRows(dump_input, dump_labels, handle->prob_precision);

            } else if (handle->gibbs) {

                labels.reset(new FlatLabels(handle->gibbs->labels()));
                rows = gibbsTextRows(handle->gibbs->view(), labels->view(), handle->precision);
                rows.second_u32 = nullptr;

            } else if (handle->sets) {

                labels.reset(new FlatLabels(handle->estimates->labels));
                estimates = handle->estimates->table->estimates();
                set_rows = setsTextRows(estimates, handle->estimates->table->view(), labels->view(), handle->kind, handle->ploidy, handle->min_posterior, handle->precision);

            } else {

                labels.reset(new FlatLabels(handle->estimates->labels));
                estimates = handle->estimates->table->estimates();
                rows = estimatesTextRows(estimates, handle->estimates->table->view(), labels->view(), handle->kind, handle->precision, &member_base);
            }

            const auto start = std::chrono::steady_clock::now();
            handle->line.reset(new HostLine(handle->rows ? hostLineRows(dump_rows) : (handle->sets ? hostLineSets(set_rows) : hostLine(rows))));

            if (seconds_out) {

                *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            }
        }

        const HostLine & line = *handle->line;

        if (num_bytes_out) {

            *num_bytes_out = line.bytes.size();
        }

        if (exact_cells_out) {

            *exact_cells_out = line.exact_cells;
        }

        if (bytes_out) {

            std::copy(line.bytes.begin(), line.bytes.end(), bytes_out);
        }

        if (row_off_out) {

            std::copy(line.row_off.begin(), line.row_off.end(), row_off_out);
        }

        if (equal_out) {

            const rpvg_table_text_view & view = handle->text->view();
            *equal_out = view.num_bytes == line.bytes.size() && view.num_paths + 1 == line.row_off.size() && std::equal(line.row_off.begin(), line.row_off.end(), view.row_off) &&
                         (view.num_bytes == 0 || std::equal(line.bytes.begin(), line.bytes.end(), view.bytes));
        }

        return 0;
    });
}

// The route the text replaces, for the timing of tools/table_text_ab.py: the table's host view (view_seconds_out: the download when
// this is the first look at it, next to nothing afterwards) and the writer's addTable() into its stream, without the file
// (add_seconds_out).
int rpvg_amd_table_text_parent_route(void * text_handle, uint32_t num_gibbs_samples, double * view_seconds_out, double * add_seconds_out) {

    return guardedInt([&]() -> int {

        TextHandle * handle = static_cast<TextHandle *>(text_handle);
        const auto start = std::chrono::steady_clock::now();
        auto viewed = start;

        if (handle->rows) {  // rpvg_hip_read_rows_view, one ReadPathProbabilities per row, writeProbabilityClusters into its stream

            const FlatRows & flat = flatRowsOf(handle, nullptr);
            viewed = std::chrono::steady_clock::now();
            const std::string text = formatProbabilityClusters(clustersOf(flat, handle->prob_precision), handle->prob_precision);

            if (text.size() != handle->text->view().num_bytes) {

                throw std::runtime_error("writeProbabilityClusters wrote a text of another length");
            }

        } else if (handle->gibbs) {

            const rpvg_gibbs_table_view & view = handle->gibbs->view();
            viewed = std::chrono::steady_clock::now();
            ReadCountGibbsSamplesWriter out("", num_gibbs_samples);
            out.addTable(view, handle->gibbs->labels());

        } else {

            const rpvg_estimates_table_view & view = handle->estimates->table->view();
            const rpvg_estimates_flat estimates = handle->estimates->table->estimates();
            viewed = std::chrono::steady_clock::now();

            if (handle->sets && handle->kind == RPVG_TEXT_JOINT) {

                JointHaplotypeAbundanceEstimatesWriter out("", handle->ploidy, handle->min_posterior, view.tpm_denominator);
                out.addTable(estimates, view, handle->estimates->labels);

            } else if (handle->sets) {

                JointHaplotypeEstimatesWriter out("", handle->ploidy, handle->min_posterior);
                out.addTable(estimates, handle->estimates->labels);

            } else if (handle->kind == RPVG_TEXT_PER_PATH) {

                AbundanceEstimatesWriter out("", view.tpm_denominator);
                out.addTable(estimates, view, handle->estimates->labels);

            } else {

                HaplotypeAbundanceEstimatesWriter out("", handle->estimates->ploidy, view.tpm_denominator);
                out.addTable(estimates, view, handle->estimates->labels);
            }
        }

        if (view_seconds_out) {

            *view_seconds_out = std::chrono::duration<double>(viewed - start).count();
        }

        if (add_seconds_out) {

            *add_seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - viewed).count();
        }

        return 0;
    });
}

void rpvg_amd_table_text_free(void * text_handle) {

    delete static_cast<TextHandle *>(text_handle);
}

}
