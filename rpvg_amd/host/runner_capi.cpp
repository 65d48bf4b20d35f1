// C entry points over the host-side estimator classes, for harnesses that are
// not C++ (tests and bench.py bind these with ctypes).  A run goes through the
// same classes a C++ caller uses: PathEstimator::estimateBatch() (mode 0) or
// the reference-shaped per-cluster PathEstimator::estimate() (mode 1).

#include <cassert>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rpvg_batch.h"
#include "batch_pipeline.hpp"
#include "device_group.hpp"
#include "estimator_factory.hpp"
#include "align_index.hpp"
#include "read_rows.hpp"
#include "runner_handles.hpp"
#include "trace.hpp"

using namespace rpvg_amd;
using namespace rpvg_amd_harness;

thread_local std::string rpvg_amd_harness::last_error;

namespace {

std::vector<std::vector<PathInfo> > unpackPaths(const rpvg_cluster_batch & batch) {

    std::vector<std::vector<PathInfo> > paths(batch.num_clusters);

    for (uint32_t i = 0; i < batch.num_clusters; ++i) {

        for (uint64_t j = batch.cluster_path_off[i]; j < batch.cluster_path_off[i + 1]; ++j) {

            PathInfo info;
            info.group_id = batch.path_group_id ? batch.path_group_id[j] : 0;
            info.source_count = batch.path_source_count ? batch.path_source_count[j] : 1;

            if (batch.path_source_off) {

                info.source_ids.insert(batch.source_id + batch.path_source_off[j], batch.source_id + batch.path_source_off[j + 1]);
            }

            info.effective_length = batch.path_effective_length ? batch.path_effective_length[j] : 0;
            paths.at(i).emplace_back(std::move(info));
        }
    }

    return paths;
}

std::vector<ReadPathProbabilities> unpackRows(const rpvg_cluster_batch & batch, const uint32_t cluster, const double prob_precision) {

    std::vector<ReadPathProbabilities> rows;

    for (uint64_t i = batch.cluster_row_off[cluster]; i < batch.cluster_row_off[cluster + 1]; ++i) {

        ReadPathProbabilities::PathProbs path_probs;

        for (uint64_t j = rpvg_batch_row_group_offset(&batch, i); j < rpvg_batch_row_group_offset(&batch, i + 1); ++j) {

            path_probs.emplace_back(batch.grp_prob[j], std::vector<uint32_t>(batch.path_idx + rpvg_batch_group_entry_offset(&batch, j), batch.path_idx + rpvg_batch_group_entry_offset(&batch, j + 1)));
        }

        rows.emplace_back(batch.row_count[i], batch.row_noise[i], path_probs, prob_precision);
    }

    return rows;
}

Result * packResult(const std::vector<PathClusterEstimates> & estimates) {

    Result * result = new Result();

    result->set_off.push_back(0);
    result->member_off.push_back(0);
    result->abund_off.push_back(0);
    result->em_off.push_back(0);
    result->em_col_off.push_back(0);

    result->gibbs_off.push_back(0);
    result->gibbs_path_off.push_back(0);
    result->gibbs_noise_off.push_back(0);
    result->gibbs_abund_off.push_back(0);

    for (auto & cluster_estimates: estimates) {

        for (auto & count_samples: cluster_estimates.gibbs_read_count_samples) {

            result->gibbs_path.insert(result->gibbs_path.end(), count_samples.path_ids.begin(), count_samples.path_ids.end());
            result->gibbs_path_off.push_back(result->gibbs_path.size());
            result->gibbs_noise.insert(result->gibbs_noise.end(), count_samples.noise_samples.begin(), count_samples.noise_samples.end());
            result->gibbs_noise_off.push_back(result->gibbs_noise.size());
            result->gibbs_abund.insert(result->gibbs_abund.end(), count_samples.abundance_samples.begin(), count_samples.abundance_samples.end());
            result->gibbs_abund_off.push_back(result->gibbs_abund.size());
        }

        result->gibbs_off.push_back(result->gibbs_path_off.size() - 1);

        for (size_t i = 0; i < cluster_estimates.path_group_sets.size(); ++i) {

            result->members.insert(result->members.end(), cluster_estimates.path_group_sets.at(i).begin(), cluster_estimates.path_group_sets.at(i).end());
            result->member_off.push_back(result->members.size());
            result->posteriors.push_back(cluster_estimates.posteriors.at(i));
        }

        result->set_off.push_back(result->posteriors.size());

        result->abundances.insert(result->abundances.end(), cluster_estimates.abundances.begin(), cluster_estimates.abundances.end());
        result->abund_off.push_back(result->abundances.size());

        result->noise_count.push_back(cluster_estimates.noise_count);
        result->total_count.push_back(cluster_estimates.total_count);

        for (size_t i = 0; i < cluster_estimates.em_iterations.size(); ++i) {

            result->em_iters.push_back(cluster_estimates.em_iterations.at(i));
            result->em_cols.insert(result->em_cols.end(), cluster_estimates.em_problem_paths.at(i).begin(), cluster_estimates.em_problem_paths.at(i).end());
            result->em_col_off.push_back(result->em_cols.size());
        }

        result->em_off.push_back(result->em_iters.size());
    }

    return result;
}

// The alignment-path lists of a flat batch handed to the builder the way a caller of the classes would
void fillBuilder(const rpvg_alignment_batch & alignments, const std::vector<std::vector<PathInfo> > & paths, AlignmentBatchBuilder * builder) {

    const bool collapse = alignments.path_group != nullptr;

    for (uint32_t i = 0; i < alignments.num_clusters; ++i) {

        std::vector<uint32_t> group_name_index;
        uint32_t num_groups = 0;

        if (collapse) {

            group_name_index.assign(alignments.path_group + alignments.cluster_path_off[i], alignments.path_group + alignments.cluster_path_off[i + 1]);
            num_groups = alignments.cluster_group_off[i + 1] - alignments.cluster_group_off[i];
        }

        builder->beginCluster(paths.at(i), group_name_index, num_groups);

        for (uint64_t r = alignments.cluster_read_off[i]; r < alignments.cluster_read_off[i + 1]; ++r) {

            std::vector<AlignmentPath> align_paths;

            for (uint64_t a = alignments.read_align_off[r]; a < alignments.read_align_off[r + 1]; ++a) {

                align_paths.emplace_back(alignments.read_min_mapq[r], alignments.align_score_sum[a], alignments.align_length[a], alignments.align_frag_length[a], std::vector<uint32_t>(alignments.align_path_idx + alignments.align_path_off[a], alignments.align_path_idx + alignments.align_path_off[a + 1]));
            }

            align_paths.emplace_back(alignments.read_min_mapq[r], alignments.read_noise_score[r], 0, 0, std::vector<uint32_t>());
            builder->addAlignmentPaths(align_paths, alignments.read_count[r]);
        }
    }
}

// What the two rpvg_amd_batch_prepare_from_fragments entry points share.  with_table: the caller's flat table goes to the device as it is and the path side of the batch is formed there; collapse_names: the batch's columns are the name groups.
void * prepareFromFragments(void * engine, const rpvg_fragment_lists * chunks, uint32_t num_chunks, const rpvg_index_params * index_params, const uint64_t * extra_set_off, const uint32_t * extra_set_path, uint64_t num_extra_sets, const std::vector<PathInfo> & global_paths, const rpvg_path_table * flat_table, const bool collapse_names, double frag_loc, double frag_scale, double frag_shape, uint32_t frag_sd_max_multi, double min_noise_prob, double prob_precision, rpvg_index_info * info_out, uint32_t * frag_counts_out, uint64_t * cluster_path_off_out, uint32_t * cluster_paths_out, double * seconds_out) {

    PreparedBatch * prepared = new PreparedBatch();
    std::unique_ptr<PreparedBatch> guard(prepared);

    if (global_paths.size() != index_params->num_paths) {

        throw std::runtime_error("one PathInfo per path of the index");
    }

    std::vector<std::vector<uint32_t> > extra_sets;

    for (uint64_t i = 0; i < num_extra_sets; ++i) {

        extra_sets.emplace_back(extra_set_path + extra_set_off[i], extra_set_path + extra_set_off[i + 1]);
    }

    const bool is_single_end = index_params->is_single_end != 0;

    prepared->fragment_length_dist.reset(is_single_end ? new FragmentLengthDist() : new FragmentLengthDist(frag_loc, frag_scale, frag_shape, frag_sd_max_multi));
    prepared->is_single_end = is_single_end;
    prepared->min_noise_prob = min_noise_prob;
    prepared->prob_precision = prob_precision;

    const bool with_table = flat_table != nullptr;
    const auto start = std::chrono::steady_clock::now();

    // the caller's arrays as they are (inside the timed region: it is part of what a run that starts from fragments pays)
    const PathTable table = with_table ? PathTable::fromArrays(*flat_table) : PathTable();

    AlignmentPathsIndex index(static_cast<Engine *>(engine)->hip, *index_params);

    for (uint32_t i = 0; i < num_chunks; ++i) {

        index.add(chunks[i]);
    }

    index.finish(extra_sets);

    const auto cluster_paths = index.clusterPaths();
    std::vector<std::vector<PathInfo> > collapsed_paths;

    if (collapse_names) {

        collapsed_paths = index.nameGroups(table);
        prepared->alignments = index.deviceAlignmentsCollapsed(table);
        prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_dist, is_single_end, min_noise_prob, prob_precision);

    } else {

        std::vector<double> effective_lengths;
        effective_lengths.reserve(global_paths.size());

        for (auto & info: global_paths) {

            effective_lengths.emplace_back(info.effective_length);
        }

        prepared->alignments = index.deviceAlignments(effective_lengths);

        if (with_table) {

            prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_dist, is_single_end, min_noise_prob, prob_precision, index, table);

        } else {

            prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_dist, is_single_end, min_noise_prob, prob_precision);
        }
    }

    if (seconds_out) {

        *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    }

    uint64_t num_cluster_paths = 0;

    for (size_t i = 0; i < cluster_paths.size(); ++i) {

        prepared->paths.emplace_back();

        if (cluster_path_off_out) {

            cluster_path_off_out[i] = num_cluster_paths;
        }

        for (auto & path_id: cluster_paths[i]) {

            if (!collapse_names) {

                prepared->paths.back().emplace_back(global_paths.at(path_id));
            }

            if (cluster_paths_out) {

                cluster_paths_out[num_cluster_paths] = path_id;
            }

            ++num_cluster_paths;
        }

        if (collapse_names) {

            prepared->paths.back() = std::move(collapsed_paths.at(i));
        }
    }

    if (cluster_path_off_out) {

        cluster_path_off_out[cluster_paths.size()] = num_cluster_paths;
    }

    if (info_out) {

        *info_out = index.info();
    }

    if (frag_counts_out) {

        const auto counts = index.fragLengthCounts();
        std::copy(counts.begin(), counts.end(), frag_counts_out);
    }

    return guard.release();
}

}

extern "C" {

const char * rpvg_amd_last_error(void) {

    return last_error.c_str();
}

void * rpvg_amd_engine_create(int device) {

    return guardedHandle([&]() -> void * {

        Engine * engine = new Engine();
        engine->hip = std::make_shared<HipEngine>(device);
        return engine;
    });
}

// an engine for rpvg_amd_batch_reupload next to the engine that estimates (HipEngine(device, uploader = true))
void * rpvg_amd_engine_create_uploader(int device) {

    return guardedHandle([&]() -> void * {

        Engine * engine = new Engine();
        engine->hip = std::make_shared<HipEngine>(device, true);
        return engine;
    });
}

void rpvg_amd_engine_destroy(void * engine) {

    delete static_cast<Engine *>(engine);
}

// The rpvg_hip_ctx of the engine (to read kernel statistics through include/rpvg_hip.h).
void * rpvg_amd_engine_ctx(void * engine) {

    return static_cast<Engine *>(engine)->hip->ctx();
}

// Kernel statistics of the engine, both host lanes together.
int rpvg_amd_engine_stats_get(void * engine, rpvg_hip_kernel_stats * stats_out) {

    return guardedInt([&]() -> int {

        static_cast<Engine *>(engine)->hip->stats(stats_out);
        return 0;
    });
}

// The counters of the independent one-call route (rpvg_hip_independent_stats), both host lanes together.
int rpvg_amd_engine_independent_stats_get(void * engine, rpvg_hip_independent_stats * stats_out) {

    return guardedInt([&]() -> int {

        static_cast<Engine *>(engine)->hip->independentStats(stats_out);
        return 0;
    });
}

int rpvg_amd_engine_stats_reset(void * engine) {

    return guardedInt([&]() -> int {

        static_cast<Engine *>(engine)->hip->resetStats();
        return 0;
    });
}

// The OpenMP team of one host lane of this process (trace.hpp, hostThreads()): what bench.py prints as host_threads_per_lane.
int rpvg_amd_host_threads() {

    return rpvg_amd::hostThreads();
}

// PathEstimator::generatorStateSelfTest (path_estimator.hpp): how the host side of the device sampler reaches the generators' states
int rpvg_amd_generator_state_check(uint32_t rounds) {

    return rpvg_amd::PathEstimator::generatorStateSelfTest(rounds);
}

// Uploads the batch to the GPU.  keep_rows != 0 also keeps ReadPathProbabilities
// objects of every cluster for the per-cluster estimate() mode.
void * rpvg_amd_batch_prepare(void * engine, const rpvg_cluster_batch * batch, int keep_rows) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = new PreparedBatch();
        std::unique_ptr<PreparedBatch> guard(prepared);

        prepared->paths = unpackPaths(*batch);

        if (keep_rows) {

            for (uint32_t i = 0; i < batch->num_clusters; ++i) {

                prepared->rows.emplace_back(unpackRows(*batch, i, 1e-8));
            }

        } else {

            prepared->device.reset(new DeviceClusterBatch(static_cast<Engine *>(engine)->hip, *batch));
        }

        return guard.release();
    });
}

// The same, starting one step earlier: the batch's reads arrive as alignment-path lists (include/rpvg_rows.h) and
// the rows are constructed on the GPU (read_rows.hpp); `path_info` supplies the path arrays of rpvg_cluster_batch
// (the PathInfo of every cluster; its row arrays are ignored).  seconds_out = wall time of the row construction
// with the alignment lists in host memory (upload included).
void * rpvg_amd_batch_prepare_from_alignments(void * engine, const rpvg_alignment_batch * alignments, const rpvg_cluster_batch * path_info, double frag_loc, double frag_scale, double frag_shape, uint32_t frag_sd_max_multi, int is_single_end, double min_noise_prob, double prob_precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = new PreparedBatch();
        std::unique_ptr<PreparedBatch> guard(prepared);

        prepared->paths = unpackPaths(*path_info);
        assert(prepared->paths.size() == alignments->num_clusters);

        AlignmentBatchBuilder builder;
        fillBuilder(*alignments, prepared->paths, &builder);

        prepared->fragment_length_dist.reset(is_single_end ? new FragmentLengthDist() : new FragmentLengthDist(frag_loc, frag_scale, frag_shape, frag_sd_max_multi));
        prepared->is_single_end = is_single_end != 0;
        prepared->min_noise_prob = min_noise_prob;
        prepared->prob_precision = prob_precision;

        const auto start = std::chrono::steady_clock::now();
        prepared->alignments.reset(new DeviceAlignmentBatch(static_cast<Engine *>(engine)->hip, builder));
        prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_dist, prepared->is_single_end, min_noise_prob, prob_precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return guard.release();
    });
}

// The same for a paired-end run that brings neither a fitted distribution nor effective lengths: the counts of the
// observed fragment lengths (FragmentLengthDist's third constructor, src/main.cpp:235) and the length of every path
// (path_length[P], in the order of path_info's paths; src/main.cpp:880).  The fit, the density table and the effective
// lengths are computed on the GPU; path_info's effective lengths are ignored.  fit_out (may be NULL) receives the fit,
// effective_length_out (may be NULL, [P]) the effective lengths that the PathInfo of the batch now hold.  A fit that is
// not a valid distribution (fewer than two samples) is an error.
void * rpvg_amd_batch_prepare_from_alignments_fit(void * engine, const rpvg_alignment_batch * alignments, const rpvg_cluster_batch * path_info, const uint32_t * frag_length_counts, uint32_t num_frag_length_counts, int skew_normal, const uint32_t * path_length, double min_noise_prob, double prob_precision, rpvg_frag_length_fit * fit_out, double * effective_length_out, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = new PreparedBatch();
        std::unique_ptr<PreparedBatch> guard(prepared);

        prepared->paths = unpackPaths(*path_info);
        assert(prepared->paths.size() == alignments->num_clusters);

        AlignmentBatchBuilder builder;
        fillBuilder(*alignments, prepared->paths, &builder);

        auto hip = static_cast<Engine *>(engine)->hip;

        if (num_frag_length_counts == 0 || frag_length_counts[0] != 0 || num_frag_length_counts > RPVG_FRAG_LENGTH_MAX_COUNTS) {

            throw std::runtime_error("fragment length counts: between 1 and 65536 entries, none of length 0");
        }

        prepared->fragment_length_dist.reset(new FragmentLengthDist(std::vector<uint32_t>(frag_length_counts, frag_length_counts + num_frag_length_counts), skew_normal != 0, hip));

        if (fit_out) {

            fit_out->loc = prepared->fragment_length_dist->loc();
            fit_out->scale = prepared->fragment_length_dist->scale();
            fit_out->shape = prepared->fragment_length_dist->shape();
            fit_out->max_length = prepared->fragment_length_dist->maxLength();
            fit_out->sample_size = prepared->fragment_length_dist->fitSampleSize();
            fit_out->iterations = prepared->fragment_length_dist->fitIterations();
            fit_out->evaluations = prepared->fragment_length_dist->fitEvaluations();
            fit_out->valid = prepared->fragment_length_dist->isValid();
        }

        if (!prepared->fragment_length_dist->isValid()) {

            throw std::runtime_error("too few fragment lengths to fit their distribution");
        }

        prepared->is_single_end = false;
        prepared->min_noise_prob = min_noise_prob;
        prepared->prob_precision = prob_precision;

        const uint64_t num_paths = alignments->cluster_path_off[alignments->num_clusters];

        const auto start = std::chrono::steady_clock::now();
        prepared->fragment_length_table.reset(new DeviceFragmentLengthTable(hip, *prepared->fragment_length_dist));
        prepared->alignments.reset(new DeviceAlignmentBatch(hip, builder, std::vector<uint32_t>(path_length, path_length + num_paths), *prepared->fragment_length_dist));
        prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_table, min_noise_prob, prob_precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        const auto & effective_lengths = prepared->alignments->effectiveLengths();
        size_t path = 0;

        for (auto & cluster_paths: prepared->paths) {

            for (auto & info: cluster_paths) {

                info.effective_length = effective_lengths.at(path);
                info.length = path_length[path];
                ++path;
            }
        }

        assert(path == effective_lengths.size());

        if (effective_length_out) {

            std::copy(effective_lengths.begin(), effective_lengths.end(), effective_length_out);
        }

        return guard.release();
    });
}

// The rows of a distribution that was fitted earlier (rpvg_hip_frag_length_fit: it has a maximum length, not the
// sd_max_multi of the parametric constructors): its density table is computed on the GPU and stays there, as in
// rpvg_amd_batch_prepare_from_alignments_fit; the effective lengths are path_info's.
void * rpvg_amd_batch_prepare_from_alignments_fitted(void * engine, const rpvg_alignment_batch * alignments, const rpvg_cluster_batch * path_info, double frag_loc, double frag_scale, double frag_shape, double min_noise_prob, double prob_precision, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = new PreparedBatch();
        std::unique_ptr<PreparedBatch> guard(prepared);

        prepared->paths = unpackPaths(*path_info);
        assert(prepared->paths.size() == alignments->num_clusters);

        AlignmentBatchBuilder builder;
        fillBuilder(*alignments, prepared->paths, &builder);

        if (!(frag_loc >= 0 && frag_scale > 0)) {

            throw std::runtime_error("not a valid fragment length distribution");
        }

        auto hip = static_cast<Engine *>(engine)->hip;

        prepared->fragment_length_dist.reset(new FragmentLengthDist(frag_loc, frag_scale, frag_shape, 10));
        prepared->is_single_end = false;
        prepared->min_noise_prob = min_noise_prob;
        prepared->prob_precision = prob_precision;

        const auto start = std::chrono::steady_clock::now();
        prepared->fragment_length_table.reset(new DeviceFragmentLengthTable(hip, *prepared->fragment_length_dist));
        prepared->alignments.reset(new DeviceAlignmentBatch(hip, builder));
        prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_table, min_noise_prob, prob_precision);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return guard.release();
    });
}

// The same, starting two steps earlier: the reads arrive as the stream of per-fragment alignment-path lists (include/rpvg_index.h),
// `num_chunks` chunks in order, with GLOBAL path ids.  The index (align_index.hpp) counts the fragment lengths, merges equal lists,
// clusters the paths (extra sets: addNodeClusters) and orders the clusters on the GPU; the rows are constructed from its resident
// result.  `path_info` supplies the PathInfo of the global paths: its clusters back to back are paths 0 .. P-1 (its row arrays are
// ignored).  The prepared batch holds the clusters in the index's rank order.  Outputs (any may be NULL): info_out; frag_counts_out
// [max_frag_length + 1]; cluster_path_off_out [P + 1 cells, K + 1 used] and cluster_paths_out [P]: the global paths of every cluster.
// The distribution is the caller's (frag_loc ...), as in rpvg_amd_batch_prepare_from_alignments; seconds_out = wall time from the
// first chunk to the rows.
void * rpvg_amd_batch_prepare_from_fragments(void * engine, const rpvg_fragment_lists * chunks, uint32_t num_chunks, const rpvg_index_params * index_params, const uint64_t * extra_set_off, const uint32_t * extra_set_path, uint64_t num_extra_sets, const rpvg_cluster_batch * path_info, double frag_loc, double frag_scale, double frag_shape, uint32_t frag_sd_max_multi, double min_noise_prob, double prob_precision, rpvg_index_info * info_out, uint32_t * frag_counts_out, uint64_t * cluster_path_off_out, uint32_t * cluster_paths_out, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        std::vector<PathInfo> global_paths;

        for (auto & cluster_paths: unpackPaths(*path_info)) {

            for (auto & info: cluster_paths) {

                global_paths.emplace_back(std::move(info));
            }
        }

        return prepareFromFragments(engine, chunks, num_chunks, index_params, extra_set_off, extra_set_path, num_extra_sets, global_paths, nullptr, false, frag_loc, frag_scale, frag_shape, frag_sd_max_multi, min_noise_prob, prob_precision, info_out, frag_counts_out, cluster_path_off_out, cluster_paths_out, seconds_out);
    });
}

// The same with the PathInfo of the global paths as a path table (include/rpvg_index.h) that is made resident once: the path side
// of the prepared batch — group ids, haplotype columns, read totals — is formed on the GPU (the batch reports has_source_columns
// when the table has source ids), nothing of it is permuted on the host but the PathInfo the estimators label their output with.
// collapse_names (the table needs name_id): `-i transcripts --path-info` — the name groups of every cluster are the columns of
// the batch and its paths are the collapsed ones (src/main.cpp:853-887,909-951); a path named by name_id n is called "n<n>".
void * rpvg_amd_batch_prepare_from_fragments_table(void * engine, const rpvg_fragment_lists * chunks, uint32_t num_chunks, const rpvg_index_params * index_params, const uint64_t * extra_set_off, const uint32_t * extra_set_path, uint64_t num_extra_sets, const rpvg_path_table * table, int collapse_names, double frag_loc, double frag_scale, double frag_shape, uint32_t frag_sd_max_multi, double min_noise_prob, double prob_precision, rpvg_index_info * info_out, uint32_t * frag_counts_out, uint64_t * cluster_path_off_out, uint32_t * cluster_paths_out, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        if (collapse_names && !table->name_id) {

            throw std::runtime_error("collapsing names needs name_id");
        }

        std::vector<PathInfo> global_paths(table->num_paths);

        for (uint32_t i = 0; i < table->num_paths; ++i) {

            auto & info = global_paths[i];
            info.name = table->name_id ? "n" + std::to_string(table->name_id[i]) : std::string();
            info.group_id = table->group_id[i];
            info.source_count = table->source_count[i];
            info.length = table->length[i];
            info.effective_length = table->effective_length[i];

            if (table->source_off && !collapse_names) {

                info.source_ids.insert(table->source_id + table->source_off[i], table->source_id + table->source_off[i + 1]);
            }
        }

        return prepareFromFragments(engine, chunks, num_chunks, index_params, extra_set_off, extra_set_path, num_extra_sets, global_paths, table, collapse_names != 0, frag_loc, frag_scale, frag_shape, frag_sd_max_multi, min_noise_prob, prob_precision, info_out, frag_counts_out, cluster_path_off_out, cluster_paths_out, seconds_out);
    });
}

// 1 when the resident batch holds the haplotype columns of its clusters (DeviceClusterBatch::hasSourceColumns)
int rpvg_amd_batch_has_source_columns(void * prepared) {

    auto * batch = static_cast<PreparedBatch *>(prepared);
    return (batch && batch->device && batch->device->hasSourceColumns()) ? 1 : 0;
}

// A measurement line for the path table, not product: the two loops of the reference's cluster loop on ONE host thread with
// std::unordered_map<std::string, uint32_t> (the reference's spp::sparse_hash_map cannot be built here) — group_name_index
// (src/main.cpp:853-887) and the collapsed paths (:909-951) — over the clusters of an index (cluster_path_off [K+1],
// cluster_paths [P], global ids) and a flat table with name ids; a path's name is "n<name_id>", made before the clock starts.
// Unlike the reference the sums are 64-bit (the device's rule).  Outputs: path_group_out [P], cluster_group_off_out [K+1], and per
// group (capacity P) source_count, length, effective_length; seconds_out: wall time of the two loops.
int rpvg_amd_path_table_host_line(const rpvg_path_table * table, uint32_t num_clusters, const uint64_t * cluster_path_off, const uint32_t * cluster_paths, uint32_t * path_group_out, uint64_t * cluster_group_off_out, uint32_t * group_source_count_out, uint32_t * group_length_out, double * group_effective_length_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        if (!table->name_id) {

            throw std::runtime_error("the host line needs name_id");
        }

        std::vector<std::string> names(table->num_paths);

        for (uint32_t i = 0; i < table->num_paths; ++i) {

            names[i] = "n" + std::to_string(table->name_id[i]);
        }

        struct Collapsed { bool seen = false; uint64_t source_count = 0; uint64_t length = 0; double effective_length = 0; };

        const auto start = std::chrono::steady_clock::now();

        uint64_t num_groups = 0;
        cluster_group_off_out[0] = 0;

        for (uint32_t i = 0; i < num_clusters; ++i) {

            std::unordered_map<std::string, uint32_t> group_name_index;

            for (uint64_t j = cluster_path_off[i]; j < cluster_path_off[i + 1]; ++j) {

                group_name_index.emplace(names[cluster_paths[j]], group_name_index.size());
            }

            std::vector<Collapsed> collapsed_paths(group_name_index.size());

            for (uint64_t j = cluster_path_off[i]; j < cluster_path_off[i + 1]; ++j) {

                const uint32_t path_id = cluster_paths[j];
                const uint32_t group = group_name_index.find(names[path_id])->second;
                path_group_out[j] = group;

                auto & collapsed_path = collapsed_paths[group];
                const double weighted = table->effective_length[path_id] * table->source_count[path_id];

                collapsed_path.source_count += table->source_count[path_id];
                collapsed_path.length += static_cast<uint64_t>(table->length[path_id]) * table->source_count[path_id];
                collapsed_path.effective_length = collapsed_path.seen ? collapsed_path.effective_length + weighted : weighted;
                collapsed_path.seen = true;
            }

            for (auto & collapsed_path: collapsed_paths) {

                group_source_count_out[num_groups] = collapsed_path.source_count;
                group_length_out[num_groups] = std::round(collapsed_path.length / static_cast<double>(collapsed_path.source_count));
                group_effective_length_out[num_groups] = collapsed_path.effective_length / static_cast<double>(collapsed_path.source_count);
                ++num_groups;
            }

            cluster_group_off_out[i + 1] = num_groups;
        }

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return 0;
    });
}

// A measurement line for the index, not product: the structure of addAlignmentPathsBufferToIndexes (src/main.cpp:200-237) on ONE
// host thread — the histogram gate, the normalisation of one-alignment lists, a std::unordered_map keyed by the list's contents
// (the reference's spp::sparse_hash_map and its gbwt search states cannot be built here) — over the same flat chunks.  Outputs
// (any may be NULL): frag_counts_out [max_frag_length + 1]; the distinct lists in order of first occurrence: first_occurrence_out
// and multiplicity_out (capacity: the number of lists of the stream); their number.  seconds_out: wall time of the loop.
namespace {

struct HostLineKey {

    uint8_t is_simple, min_mapq;
    int32_t noise_score;
    std::vector<uint32_t> words;  // per alignment: score, lengths, number of paths, the path ids

    bool operator==(const HostLineKey & other) const { return is_simple == other.is_simple && min_mapq == other.min_mapq && noise_score == other.noise_score && words == other.words; }
};

struct HostLineKeyHash {

    size_t operator()(const HostLineKey & key) const {

        uint64_t h = 1469598103934665603ull ^ key.is_simple ^ (static_cast<uint64_t>(key.min_mapq) << 8) ^ (static_cast<uint64_t>(static_cast<uint32_t>(key.noise_score)) << 16);

        for (auto word: key.words) {

            h = (h ^ word) * 1099511628211ull;
        }

        return h;
    }
};

}

int rpvg_amd_align_index_host_line(const rpvg_fragment_lists * chunks, uint32_t num_chunks, const rpvg_index_params * params, uint32_t * frag_counts_out, uint64_t * num_distinct_out, uint64_t * first_occurrence_out, uint32_t * multiplicity_out, double * seconds_out) {

    return guardedInt([&]() -> int {

        std::vector<uint32_t> frag_length_counts(static_cast<size_t>(params->max_frag_length) + 1, 0);
        std::unordered_map<HostLineKey, std::pair<uint64_t, uint32_t>, HostLineKeyHash> index;  // contents -> (first occurrence, multiplicity)
        uint64_t num_lists = 0;

        const auto start = std::chrono::steady_clock::now();

        for (uint32_t c = 0; c < num_chunks; ++c) {

            const auto & chunk = chunks[c];

            for (uint64_t i = 0; i < chunk.num_lists; ++i) {

                const uint64_t a0 = chunk.list_align_off[i], a1 = chunk.list_align_off[i + 1];

                if (!params->is_single_end && chunk.list_is_simple[i] && chunk.list_min_mapq[i] >= params->frag_length_min_mapq) {

                    frag_length_counts.at(chunk.align_frag_length[a0])++;
                }

                HostLineKey key;
                key.is_simple = chunk.list_is_simple[i] != 0;
                key.min_mapq = chunk.list_min_mapq[i];
                key.noise_score = chunk.list_noise_score[i];

                for (uint64_t a = a0; a < a1; ++a) {

                    const bool single = (a1 - a0 == 1);
                    key.words.emplace_back(single ? 1 : static_cast<uint32_t>(chunk.align_score_sum[a]));
                    key.words.emplace_back(single ? (1u | (static_cast<uint32_t>(params->pre_frag_loc) << 16)) : (chunk.align_length[a] | (static_cast<uint32_t>(chunk.align_frag_length[a]) << 16)));
                    key.words.emplace_back(chunk.align_path_off[a + 1] - chunk.align_path_off[a]);
                    key.words.insert(key.words.end(), chunk.align_path_id + chunk.align_path_off[a], chunk.align_path_id + chunk.align_path_off[a + 1]);
                }

                auto it = index.emplace(std::move(key), std::make_pair(num_lists, 0u));
                it.first->second.second++;
                ++num_lists;
            }
        }

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        if (frag_counts_out) {

            std::copy(frag_length_counts.begin(), frag_length_counts.end(), frag_counts_out);
        }

        if (num_distinct_out) {

            *num_distinct_out = index.size();
        }

        if (first_occurrence_out && multiplicity_out) {

            std::vector<std::pair<uint64_t, uint32_t> > ordered;
            ordered.reserve(index.size());

            for (auto & entry: index) {

                ordered.emplace_back(entry.second);
            }

            std::sort(ordered.begin(), ordered.end());

            for (size_t i = 0; i < ordered.size(); ++i) {

                first_occurrence_out[i] = ordered[i].first;
                multiplicity_out[i] = ordered[i].second;
            }
        }

        return 0;
    });
}

// BASELINE.json configs[1] for the estimator classes: one cluster of `num_rows` rows that each touch all `num_paths` paths,
// generated on the device (rpvg_hip_synth_dense_cluster_batch: the host form of 10^6 x 2 000 rows would be 40 GB) and
// adopted as a resident batch — the caller runs `transcripts` on it like on any other batch.
void * rpvg_amd_batch_prepare_synth_dense(void * engine, uint64_t seed, uint64_t num_rows, uint32_t num_paths) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = new PreparedBatch();
        std::unique_ptr<PreparedBatch> guard(prepared);

        prepared->paths.emplace_back();

        for (uint32_t j = 0; j < num_paths; ++j) {

            PathInfo info;
            info.group_id = 0;
            info.source_count = 1;
            info.effective_length = 1000;
            prepared->paths.back().emplace_back(std::move(info));
        }

        auto hip = static_cast<Engine *>(engine)->hip;

        rpvg_hip_batch * device_batch = nullptr;
        HipEngine::check(rpvg_hip_synth_dense_cluster_batch(hip->ctx(), seed, num_rows, num_paths, &device_batch), "rpvg_hip_synth_dense_cluster_batch");

        const uint64_t cluster_row_off[2] = {0, num_rows};
        const uint64_t cluster_path_off[2] = {0, num_paths};

        rpvg_cluster_batch offsets;
        std::memset(&offsets, 0, sizeof(offsets));
        offsets.num_clusters = 1;
        offsets.cluster_row_off = cluster_row_off;
        offsets.cluster_path_off = cluster_path_off;

        // (every row of the synthetic cluster is one read pair; the multi-gigabyte batch is freed here until the handle has adopted it)
        struct BatchGuard {

            rpvg_hip_ctx * ctx;
            rpvg_hip_batch * batch;
            ~BatchGuard() { if (batch) rpvg_hip_batch_free(ctx, batch); }

        } batch_guard{hip->ctx(), device_batch};

        prepared->device.reset(new DeviceClusterBatch(hip, device_batch, offsets, std::vector<double>(1, static_cast<double>(num_rows))));
        batch_guard.batch = nullptr;

        return guard.release();
    });
}

// A new resident copy of the rows of a prepared batch from the same host arrays (what arrives per batch in a
// running pipeline: the rows; the PathInfo side stays).  `engine` may be another engine on the same GPU than the one
// that estimates — an uploader with a context and stream of its own, so that the copy of batch n + 1 runs under
// the kernels of batch n.  seconds_out = wall time of validation + H2D + expansion on the device.
int rpvg_amd_batch_reupload(void * engine, void * prepared_batch, const rpvg_cluster_batch * batch, double * seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);
        const auto start = std::chrono::steady_clock::now();

        std::unique_ptr<DeviceClusterBatch> fresh(new DeviceClusterBatch(static_cast<Engine *>(engine)->hip, *batch));
        prepared->device = std::move(fresh);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return 0;
    });
}

void rpvg_amd_batch_free(void * prepared) {

    delete static_cast<PreparedBatch *>(prepared);
}

// Runs `model` on a prepared batch.  seconds_out = wall time of the estimator
// call(s) only (inputs already resident on the GPU in batch mode).
void * rpvg_amd_run(void * engine, void * prepared_batch, const char * model, const rpvg_params * params, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);
        auto estimator = makePathEstimator(model, *params, static_cast<Engine *>(engine)->hip);

        // the estimates containers (with PathInfo filled in, as src/main.cpp:855-887 does
        // before estimate()) are created once per prepared batch and reused by every run
        if (prepared->estimates.size() != prepared->paths.size()) {

            prepared->estimates.assign(prepared->paths.size(), PathClusterEstimates());

            for (size_t i = 0; i < prepared->estimates.size(); ++i) {

                prepared->estimates.at(i).paths = prepared->paths.at(i);
            }
        }

        std::vector<PathClusterEstimates> & estimates = prepared->estimates;

        const auto start = std::chrono::steady_clock::now();

        if (prepared->device) {

            estimator->estimateBatchSeeded(&estimates, *prepared->device, params->rng_seed);

        } else {

            // the reference's loop body: one estimate() per cluster (src/main.cpp:976-977)
            for (size_t i = 0; i < estimates.size(); ++i) {

                std::mt19937 mt_rng(params->rng_seed + i);
                estimator->estimate(&estimates.at(i), prepared->rows.at(i), &mt_rng);
            }
        }

        const auto stop = std::chrono::steady_clock::now();

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(stop - start).count();
        }

        PhaseTrace::add("total estimate call", std::chrono::duration<double>(stop - start).count());
        PhaseTrace::report();

        return packResult(estimates);
    });
}

// Where a batch estimate leaves the callers' generators: runs `model` on a device-resident prepared batch with cluster i on
// mt19937(rng_seed + i) and writes every generator's NEXT output to next_out[i] (tests: two routes of a model that draw the same
// numbers leave the generators in the same place).  The estimates stay in the prepared batch's containers.
int rpvg_amd_run_generators_after(void * engine, void * prepared_batch, const char * model, const rpvg_params * params, uint32_t * next_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (!prepared->device) {

            last_error = "rpvg_amd_run_generators_after needs a batch that is resident on the device";
            return -1;
        }

        auto estimator = makePathEstimator(model, *params, static_cast<Engine *>(engine)->hip);

        if (prepared->estimates.size() != prepared->paths.size()) {

            prepared->estimates.assign(prepared->paths.size(), PathClusterEstimates());

            for (size_t i = 0; i < prepared->estimates.size(); ++i) {

                prepared->estimates.at(i).paths = prepared->paths.at(i);
            }
        }

        std::vector<std::mt19937> rngs;

        for (size_t i = 0; i < prepared->estimates.size(); ++i) {

            rngs.emplace_back(params->rng_seed + i);
        }

        estimator->estimateBatch(&prepared->estimates, *prepared->device, &rngs);

        for (size_t i = 0; i < rngs.size(); ++i) {

            next_out[i] = rngs[i]();
        }

        return 0;
    });
}

// The reference's cluster loop (src/main.cpp:829,976-977) on a batch prepared with keep_rows: estimate() once per cluster
// from an OpenMP team of `threads` (schedule(dynamic, 1), clusters in the batch's order), cluster i with mt19937(rng_seed + i).
// The estimates stay in the prepared batch's containers (rpvg_amd_run_team_result flattens them).
int rpvg_amd_run_team(void * engine, void * prepared_batch, const char * model, const rpvg_params * params, int threads, double * seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (prepared->rows.size() != prepared->paths.size()) {

            last_error = "rpvg_amd_run_team needs a batch prepared with keep_rows";
            return -1;
        }

        auto estimator = makePathEstimator(model, *params, static_cast<Engine *>(engine)->hip);

        if (prepared->estimates.size() != prepared->paths.size()) {

            prepared->estimates.assign(prepared->paths.size(), PathClusterEstimates());

            for (size_t i = 0; i < prepared->estimates.size(); ++i) {

                prepared->estimates.at(i).paths = prepared->paths.at(i);
            }
        }

        std::vector<PathClusterEstimates> & estimates = prepared->estimates;
        std::string first_failure;

        const auto start = std::chrono::steady_clock::now();
        ScopedPhase pass_phase("team: one pass of estimate() calls");

        #pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, threads))
        for (size_t i = 0; i < estimates.size(); ++i) {

            try {

                std::mt19937 mt_rng(params->rng_seed + i);
                estimator->estimate(&estimates.at(i), prepared->rows.at(i), &mt_rng);

            } catch (const std::exception & e) {

                #pragma omp critical
                if (first_failure.empty()) {

                    first_failure = e.what();
                }
            }
        }

        pass_phase.stop();

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        PhaseTrace::report();

        if (!first_failure.empty()) {

            last_error = first_failure;
            return -1;
        }

        return 0;
    });
}

void * rpvg_amd_run_team_result(void * prepared_batch) {

    return guardedHandle([&]() -> void * {

        return packResult(static_cast<PreparedBatch *>(prepared_batch)->estimates);
    });
}

// Same run, estimates left in the prepared batch's containers and not flattened
// (timing loops).  Returns 0 on success.
int rpvg_amd_run_inplace(void * engine, void * prepared_batch, const char * model, const rpvg_params * params, double * seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (!prepared->device) {

            last_error = "rpvg_amd_run_inplace needs a batch prepared for estimateBatch()";
            return -1;
        }

        auto estimator = makePathEstimator(model, *params, static_cast<Engine *>(engine)->hip);

        if (prepared->estimates.size() != prepared->paths.size()) {

            prepared->estimates.assign(prepared->paths.size(), PathClusterEstimates());

            for (size_t i = 0; i < prepared->estimates.size(); ++i) {

                prepared->estimates.at(i).paths = prepared->paths.at(i);
            }
        }

        const auto start = std::chrono::steady_clock::now();
        estimator->estimateBatchSeeded(&prepared->estimates, *prepared->device, params->rng_seed);
        const auto stop = std::chrono::steady_clock::now();

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(stop - start).count();
        }

        PhaseTrace::add("total estimate call", std::chrono::duration<double>(stop - start).count());
        PhaseTrace::report();

        return 0;
    });
}

// One pass of the widened path with the alignment-path lists resident on the GPU: rows are constructed and merged on
// the device (read_rows.hpp), become the estimators' batch without leaving it, and `model` runs on them.
// rows_seconds_out / estimate_seconds_out = wall time of the two stages.
int rpvg_amd_run_from_alignments_inplace(void * engine, void * prepared_batch, const char * model, const rpvg_params * params, double * rows_seconds_out, double * estimate_seconds_out) {

    return guardedInt([&]() -> int {

        PreparedBatch * prepared = static_cast<PreparedBatch *>(prepared_batch);

        if (!prepared->alignments) {

            last_error = "rpvg_amd_run_from_alignments_inplace needs a batch prepared from alignment-path lists";
            return -1;
        }

        const auto start = std::chrono::steady_clock::now();

        prepared->device.reset();

        if (prepared->fragment_length_table) {

            prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_table, prepared->min_noise_prob, prepared->prob_precision);

        } else {

            prepared->device = constructReadPathProbabilities(*prepared->alignments, *prepared->fragment_length_dist, prepared->is_single_end, prepared->min_noise_prob, prepared->prob_precision);
        }

        const auto rows_done = std::chrono::steady_clock::now();

        if (rows_seconds_out) {

            *rows_seconds_out = std::chrono::duration<double>(rows_done - start).count();
        }

        return rpvg_amd_run_inplace(engine, prepared_batch, model, params, estimate_seconds_out);
    });
}

// ---- the GPUs of a node behind one call (device_group.hpp) -------------------------------------------------------

struct Group {

    std::unique_ptr<DeviceGroup> devices;
    std::vector<PathClusterEstimates> estimates;
};

void * rpvg_amd_group_create(const int * devices, int num_devices) {

    return guardedHandle([&]() -> void * {

        Group * group = new Group();
        std::unique_ptr<Group> guard(group);
        group->devices.reset(new DeviceGroup(std::vector<int>(devices, devices + num_devices)));
        return guard.release();
    });
}

void rpvg_amd_group_destroy(void * group) {

    delete static_cast<Group *>(group);
}

int rpvg_amd_group_has_communicator(void * group) {

    return static_cast<Group *>(group)->devices->hasCommunicator() ? 1 : 0;
}

// Estimates of every cluster of a host batch, its clusters sharded over the group's GPUs.
void * rpvg_amd_group_run(void * group_handle, const rpvg_cluster_batch * batch, const char * model, const rpvg_params * params, double * seconds_out) {

    return guardedHandle([&]() -> void * {

        Group * group = static_cast<Group *>(group_handle);
        const auto paths = unpackPaths(*batch);

        group->estimates.assign(paths.size(), PathClusterEstimates());

        for (size_t i = 0; i < paths.size(); ++i) {

            group->estimates.at(i).paths = paths.at(i);
        }

        const auto start = std::chrono::steady_clock::now();
        group->devices->estimateBatch(&group->estimates, *batch, model, *params);

        if (seconds_out) {

            *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        }

        return packResult(group->estimates);
    });
}

// GPU of every cluster in the last run.
int rpvg_amd_group_partition(void * group_handle, uint32_t * device_of_cluster, uint64_t num_clusters) {

    Group * group = static_cast<Group *>(group_handle);
    const auto & partition = group->devices->lastPartition();

    for (size_t idx = 0; idx < partition.size(); ++idx) {

        for (auto & cluster: partition.at(idx)) {

            if (cluster >= num_clusters) {

                last_error = "rpvg_amd_group_partition: output too short";
                return -1;
            }

            device_of_cluster[cluster] = idx;
        }
    }

    return 0;
}

// The final gather of the last run: abundances of all clusters in cluster order (capacity doubles available), their
// number, and the TPM denominator.
int rpvg_amd_group_gather(void * group_handle, double * abundances_out, uint64_t capacity, uint64_t * count_out, double * total_transcript_count_out) {

    return guardedInt([&]() -> int {

        Group * group = static_cast<Group *>(group_handle);
        const auto gathered = group->devices->gatherAbundances(group->estimates, total_transcript_count_out);

        if (gathered.size() > capacity) {

            last_error = "rpvg_amd_group_gather: output too short";
            return -1;
        }

        std::copy(gathered.begin(), gathered.end(), abundances_out);
        *count_out = gathered.size();
        return 0;
    });
}

// ---- several batches in flight on one GPU (batch_pipeline.hpp) --------------------------------------------------------

struct Pipeline {

    std::unique_ptr<BatchPipeline> pipeline;

    // the containers the estimates of the batches in flight go to: a harness hands the same host batch in again and again,
    // and every batch in flight needs containers of its own
    std::vector<std::vector<PathClusterEstimates> > slots;
};

void * rpvg_amd_pipeline_create(int device, const char * model, const rpvg_params * params, int workers) {

    return guardedHandle([&]() -> void * {

        Pipeline * pipeline = new Pipeline();
        std::unique_ptr<Pipeline> guard(pipeline);
        pipeline->pipeline.reset(new BatchPipeline(device, model, *params, workers));
        return guard.release();
    });
}

void rpvg_amd_pipeline_destroy(void * pipeline) {

    delete static_cast<Pipeline *>(pipeline);
}

int rpvg_amd_pipeline_workers(void * pipeline) {

    return static_cast<Pipeline *>(pipeline)->pipeline->numWorkers();
}

// `slots` sets of estimates containers with the PathInfo of the batch's clusters filled in (src/main.cpp:855-887).
int rpvg_amd_pipeline_prepare_slots(void * pipeline_handle, const rpvg_cluster_batch * batch, int slots) {

    return guardedInt([&]() -> int {

        Pipeline * pipeline = static_cast<Pipeline *>(pipeline_handle);
        pipeline->pipeline->wait();

        const auto paths = unpackPaths(*batch);
        pipeline->slots.assign(slots, std::vector<PathClusterEstimates>(paths.size()));

        for (auto & slot: pipeline->slots) {

            for (size_t i = 0; i < paths.size(); ++i) {

                slot.at(i).paths = paths.at(i);
            }
        }

        return 0;
    });
}

// The containers of ONE slot, for the clusters (paths) of `batch` — slots may hold different batches (the parts of one data set,
// submitted one behind the other); the slots in front of it exist afterwards, empty if they were not prepared.
int rpvg_amd_pipeline_prepare_slot(void * pipeline_handle, const rpvg_cluster_batch * batch, int slot) {

    return guardedInt([&]() -> int {

        Pipeline * pipeline = static_cast<Pipeline *>(pipeline_handle);
        pipeline->pipeline->wait();

        const auto paths = unpackPaths(*batch);

        if (pipeline->slots.size() <= static_cast<size_t>(slot)) {

            pipeline->slots.resize(slot + 1);
        }

        auto & containers = pipeline->slots.at(slot);
        containers.assign(paths.size(), PathClusterEstimates());

        for (size_t i = 0; i < paths.size(); ++i) {

            containers.at(i).paths = paths.at(i);
        }

        return 0;
    });
}

// Queues one batch (its arrays stay the caller's until rpvg_amd_pipeline_wait returns) with the containers of `slot`.
int rpvg_amd_pipeline_submit(void * pipeline_handle, const rpvg_cluster_batch * batch, int slot) {

    return guardedInt([&]() -> int {

        Pipeline * pipeline = static_cast<Pipeline *>(pipeline_handle);
        pipeline->pipeline->submit(*batch, &pipeline->slots.at(slot));
        return 0;
    });
}

int rpvg_amd_pipeline_wait(void * pipeline_handle) {

    return guardedInt([&]() -> int {

        static_cast<Pipeline *>(pipeline_handle)->pipeline->wait();
        return 0;
    });
}

// The estimates a finished batch left in the containers of `slot` (call after rpvg_amd_pipeline_wait).
void * rpvg_amd_pipeline_result(void * pipeline_handle, int slot) {

    return guardedHandle([&]() -> void * {

        return packResult(static_cast<Pipeline *>(pipeline_handle)->slots.at(slot));
    });
}

int rpvg_amd_pipeline_stats_get(void * pipeline_handle, rpvg_hip_kernel_stats * stats_out, double * mean_upload_seconds_out) {

    return guardedInt([&]() -> int {

        Pipeline * pipeline = static_cast<Pipeline *>(pipeline_handle);
        pipeline->pipeline->stats(stats_out);

        if (mean_upload_seconds_out) {

            uint64_t batches = 0;
            mean_upload_seconds_out[0] = pipeline->pipeline->meanUploadSeconds(&batches);

            // [1], [2]: device milliseconds per batch of the uploads' copies and of the kernels behind them
            pipeline->pipeline->uploadDeviceMs(mean_upload_seconds_out + 1, mean_upload_seconds_out + 2);
            mean_upload_seconds_out[1] /= std::max<uint64_t>(1, batches);
            mean_upload_seconds_out[2] /= std::max<uint64_t>(1, batches);

            // [3], [4], [5]: wall seconds per batch of a worker's upload finish, estimate, and wait for a resident batch
            pipeline->pipeline->workerSeconds(mean_upload_seconds_out + 3, mean_upload_seconds_out + 4, mean_upload_seconds_out + 5);
        }

        return 0;
    });
}

// Completion times of the batches since the last statistics reset (seconds since that reset, in order of completion).
int rpvg_amd_pipeline_completions(void * pipeline_handle, double * seconds_out, uint64_t capacity, uint64_t * count_out) {

    const auto completions = static_cast<Pipeline *>(pipeline_handle)->pipeline->completionSeconds();
    *count_out = completions.size();
    std::copy(completions.begin(), completions.begin() + std::min<size_t>(capacity, completions.size()), seconds_out);
    return 0;
}

int rpvg_amd_pipeline_stats_reset(void * pipeline_handle) {

    return guardedInt([&]() -> int {

        static_cast<Pipeline *>(pipeline_handle)->pipeline->resetStats();
        return 0;
    });
}

void rpvg_amd_result_view(void * result_handle, rpvg_estimates_view * out) {

    Result * result = static_cast<Result *>(result_handle);

    out->num_clusters = result->noise_count.size();
    out->set_off = result->set_off.data();
    out->member_off = result->member_off.data();
    out->members = result->members.data();
    out->posteriors = result->posteriors.data();
    out->abund_off = result->abund_off.data();
    out->abundances = result->abundances.data();
    out->noise_count = result->noise_count.data();
    out->total_count = result->total_count.data();
    out->em_off = result->em_off.data();
    out->em_iters = result->em_iters.data();
    out->em_col_off = result->em_col_off.data();
    out->em_cols = result->em_cols.data();
    out->gibbs_off = result->gibbs_off.data();
    out->gibbs_path_off = result->gibbs_path_off.data();
    out->gibbs_path = result->gibbs_path.data();
    out->gibbs_noise_off = result->gibbs_noise_off.data();
    out->gibbs_noise = result->gibbs_noise.data();
    out->gibbs_abund_off = result->gibbs_abund_off.data();
    out->gibbs_abund = result->gibbs_abund.data();
}

void rpvg_amd_result_free(void * result_handle) {

    delete static_cast<Result *>(result_handle);
}

}
