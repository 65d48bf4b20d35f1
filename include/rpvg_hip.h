/* rpvg_hip.h — C ABI of the MI355X (gfx950) engine behind rpvg's inference
 * hot path.  extern "C", plain pointers and sizes only; implemented by
 * rpvg_amd/csrc/librpvg_hip.so (hand-written HIP kernels).
 *
 * The reference (C++17, no FFI today) does all of this arithmetic inside the
 * PathEstimator class hierarchy with Eigen; each entry point below names the
 * reference code whose arithmetic it takes over (paths relative to the rpvg
 * checkout).  The host-side C++ classes in rpvg_amd/host keep the reference's
 * PathEstimator::estimate() interface and call only these functions;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative rpvg_hip_status
 *     otherwise; never throws, never aborts; rpvg_hip_last_error() describes
 *     the last failure on the calling thread.
 *   - "host" pointers are ordinary host memory owned by the caller; "device"
 *     pointers are memory of the context's GPU (rpvg_hip_malloc).
 *   - a context is bound to one GPU and owns one HIP stream; calls on one
 *     context are serialised internally, different contexts are independent.
 *   - there is NO CPU fallback: without a usable GPU rpvg_hip_create fails.
 */
#ifndef RPVG_HIP_H
#define RPVG_HIP_H

#include <stdint.h>

#include "rpvg_batch.h"
#include "rpvg_rows.h"
#include "rpvg_index.h"
#include "rpvg_table.h"
#include "rpvg_samples.h"
#include "rpvg_text.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rpvg_hip_status {
    RPVG_HIP_OK = 0,
    RPVG_HIP_ERR_NO_DEVICE = -1,  /* no gfx950-compatible GPU / HIP runtime unusable */
    RPVG_HIP_ERR_RUNTIME = -2,    /* a HIP call failed (see last_error)              */
    RPVG_HIP_ERR_INVALID = -3,    /* argument validation failed                      */
    RPVG_HIP_ERR_ALLOC = -4,      /* host or device allocation failed                */
    RPVG_HIP_ERR_UNSUPPORTED = -5 /* the call does not take this input; the caller uses the calls it stands for (nothing was changed) */
} rpvg_hip_status;

typedef struct rpvg_hip_ctx rpvg_hip_ctx;
typedef struct rpvg_hip_batch rpvg_hip_batch;   /* device-resident cluster batch          */
typedef struct rpvg_hip_groups rpvg_hip_groups; /* device-resident group (column-set) matrices */

/* ---- context ------------------------------------------------------------ */
int rpvg_hip_device_count(int * count);
int rpvg_hip_create(int device, rpvg_hip_ctx ** ctx_out);
/* A context for rpvg_hip_batch_upload next to contexts that estimate on the same GPU (the rows of batch n + 1 copied
 * under the kernels of batch n; the reference has no analogue: its rows never leave the host, SURVEY.md section 8d puts
 * the copy inside the metric).  Its stream has the device's highest priority, which gives it a hardware queue of its
 * own: the copies and expansion kernels do not queue behind the estimating contexts' kernels (measured: 10.6 -> 7.3 ms
 * per 280 MB batch while a batch is estimated, 14.7 -> 13.7 ms per batch in steady state). */
int rpvg_hip_create_uploader(int device, rpvg_hip_ctx ** ctx_out);
/* A context with fewer side streams than rpvg_hip_create's six (1..6), for engines that run whole batches next to each other
 * on one GPU (rpvg_amd/host/batch_pipeline.hpp): the runtime maps all streams of a process onto its hardware queues
 * (GPU_MAX_HW_QUEUES, 8 here), commands of streams that share a queue run in order, and four engines of nine streams
 * each put one engine's short kernels behind another's long ones.  The launches that would have had streams of their own
 * follow one another on the streams there are; results are the same. */
int rpvg_hip_create_with_streams(int device, int side_streams, rpvg_hip_ctx ** ctx_out);
void rpvg_hip_destroy(rpvg_hip_ctx * ctx);
const char * rpvg_hip_last_error(void);
int rpvg_hip_synchronize(rpvg_hip_ctx * ctx);
/* name of the GPU, number of CUs, bytes of device memory */
int rpvg_hip_device_info(rpvg_hip_ctx * ctx, char * name, uint32_t name_cap, uint32_t * num_cus, uint64_t * mem_bytes);

/* device memory helpers (for callers that keep matrices resident) */
int rpvg_hip_malloc(rpvg_hip_ctx * ctx, uint64_t bytes, void ** device_ptr_out);
int rpvg_hip_free(rpvg_hip_ctx * ctx, void * device_ptr);
int rpvg_hip_memcpy_h2d(rpvg_hip_ctx * ctx, void * device_dst, const void * host_src, uint64_t bytes);
int rpvg_hip_memcpy_d2h(rpvg_hip_ctx * ctx, void * host_dst, const void * device_src, uint64_t bytes);

/* Page-locks a range of the caller's host memory (hipHostRegister): uploads from inside a registered range go to the
 * GPU straight from it; anything else is staged through pinned blocks of the library's own (one more host copy). */
int rpvg_hip_host_register(void * host, uint64_t bytes);
int rpvg_hip_host_unregister(void * host);

/* ---- cluster batch ------------------------------------------------------ */
/* Copies the sparse rows of K clusters to the GPU once; every later call
 * refers to clusters by their index in this batch.  Replaces the per-call
 * walk over `vector<ReadPathProbabilities>` in constructProbabilityMatrix /
 * constructPartialProbabilityMatrix / constructGroupedProbabilityMatrix
 * (src/path_estimator.cpp:55-154): the (probability, path list) groups are
 * expanded to (path, probability) entries on the GPU. */
int rpvg_hip_batch_upload(rpvg_hip_ctx * ctx, const rpvg_cluster_batch * host_batch, rpvg_hip_batch ** batch_out);
void rpvg_hip_batch_free(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch);
/* The same upload in two halves, for a caller that keeps a copy engine busy (rpvg_amd/host/batch_pipeline.hpp): _begin checks
 * the offsets, queues the copies on `ctx` — an uploader's context — and returns when they are done; _finish runs the kernels
 * behind them (expansion, validation, read totals, haplotype columns) on `ctx` — any context of the same GPU, e.g. the one
 * that estimates the batch next — and returns the upload's verdict.  Between the two the batch takes no other call;
 * host_batch is the same caller-owned batch both times (a batch that fails _finish is freed by it). */
int rpvg_hip_batch_upload_begin(rpvg_hip_ctx * ctx, const rpvg_cluster_batch * host_batch, rpvg_hip_batch ** batch_out);
int rpvg_hip_batch_upload_finish(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch, const rpvg_cluster_batch * host_batch);
/* ... or the second half itself in two steps: _finish_queue puts the kernels behind the copies on a stream of `ctx` (an uploader's
 * context: its side stream, next to the copies of the batch after) and returns; _finish_wait, from any thread and without a
 * context, waits for them and does the host's part — what rpvg_hip_batch_upload_finish does in one call.  A pipeline's uploader
 * queues, the estimator that takes the batch waits (rpvg_amd/host/batch_pipeline.hpp).  On failure the batch is freed. */
int rpvg_hip_batch_upload_finish_queue(rpvg_hip_ctx * ctx, rpvg_hip_batch * batch, const rpvg_cluster_batch * host_batch);
int rpvg_hip_batch_upload_finish_wait(rpvg_hip_batch * batch, const rpvg_cluster_batch * host_batch);
/* A batch from the segments its callers flattened (include/rpvg_batch.h, rpvg_cluster_segment): what the reference's per-cluster
 * loop (src/main.cpp:829,976-977) hands to estimate(), one segment per call in flight, joined on the device.  One kernel reads
 * the segments from page-locked host memory, expands the (probability, path list) groups, validates rows and offsets and writes
 * every device array of the batch; the haplotype columns follow as in rpvg_hip_batch_upload.  Returns when the batch is
 * complete; the segments stay untouched until then.  Same results, entry for entry, as rpvg_hip_batch_upload of the joined
 * batch.  Page-locked blocks for the segments: rpvg_hip_pinned_alloc (cached by size class; a block's capacity is at least the
 * bytes asked for) / rpvg_hip_pinned_free. */
int rpvg_hip_batch_upload_segments(rpvg_hip_ctx * ctx, const rpvg_cluster_segment * segments, uint32_t num_segments, rpvg_hip_batch ** batch_out);
int rpvg_hip_pinned_alloc(uint64_t bytes, void ** host_out);
/* How the calling thread waits for the GPU inside the calls of this library from now on: it queries for `microseconds` and then
 * naps between queries (30 us each).  Default 20: a thread that waits for a millisecond-long batch should not hold a core.  A
 * thread whose callers are blocked behind it for a few hundred microseconds (the leaders of PathEstimator::estimate()'s call
 * combiner) asks for more: a nap costs 50-80 us of latency per wait. */
void rpvg_hip_thread_wait_spin_us(uint32_t microseconds);
void rpvg_hip_pinned_free(void * host);
/* Read count of every cluster of an uploaded batch (the sum of its rows' read counts, exact), added up on the device behind
 * the copy (src/path_abundance_estimator.cpp:44,291,690: `read_counts.sum()`). */
int rpvg_hip_batch_cluster_totals(const rpvg_hip_batch * batch, double * totals_out, uint32_t num_clusters);
/* The path side of a batch.  When host_batch carries path_group_id, path_source_off and source_id, rpvg_hip_batch_upload
 * also copies those and runs NestedPathAbundanceEstimator::findPathSourceGroups (src/path_abundance_estimator.cpp:493-546)
 * for every cluster on the device: haplotypes (source ids) that carry the identical list of paths form one column, its
 * multiplicity is their number, columns in ascending order of their smallest haplotype id.  1 when the batch holds such
 * columns (0: no ids were given, or their ranges are too wide for the device scratch — ids are expected to be small
 * consecutive integers — and the caller groups on the host). */
int rpvg_hip_batch_has_source_columns(const rpvg_hip_batch * batch);
/* Inspection (tests): the columns of one cluster — sizes first, then multiplicities [columns], the end of every column's list
 * within column_paths [columns], and the lists back to back (ascending cluster-local paths) [column paths]. */
int rpvg_hip_batch_source_columns_sizes(const rpvg_hip_batch * batch, uint32_t cluster, uint32_t * num_columns_out,
                                        uint32_t * num_column_paths_out);
int rpvg_hip_batch_source_columns_get(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t cluster,
                                      uint32_t * column_counts_out, uint32_t * column_path_end_out, uint32_t * column_paths_out);
/* Inspection (tests and tools): the row side of a complete batch, however it was made, as the estimators read it — sizes first
 * (rows R, entries NNZ), then host copies of row_ent_off [R + 1], row_count [R] (read counts as doubles), row_noise [R],
 * ent_path [NNZ] (cluster-local path of every entry) and ent_prob [NNZ] (the probability of the entry's group). */
int rpvg_hip_batch_rows_sizes(const rpvg_hip_batch * batch, uint64_t * num_rows_out, uint64_t * num_entries_out);
int rpvg_hip_batch_rows_get(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint64_t * row_ent_off_out, double * row_count_out,
                            double * row_noise_out, uint32_t * ent_path_out, double * ent_prob_out);

/* ---- EM abundance solves ------------------------------------------------ */
/* One EM problem = one cluster restricted to a strictly ascending list of its
 * paths (all of them for `-i transcripts`, a diplotype's path subset for
 * `-i haplotype-transcripts`), plus the noise component. */
typedef struct rpvg_hip_em_problems {
    uint32_t num_problems;
    const uint32_t * cluster;  /* host [P]   index into the uploaded batch          */
    const uint64_t * col_off;  /* host [P+1] range into col_path                    */
    const uint32_t * col_path; /* host       cluster-local path of each column      */
    /* > 0: readCollapseProbabilityMatrix (src/path_estimator.cpp:219-259) on the normalised rows of every problem, with this
     * prob_precision, as MinimumPathAbundanceEstimator and NestedPathAbundanceEstimator do before their EM
     * (src/path_abundance_estimator.cpp:266,668; PathAbundanceEstimator::estimate, :18-45, does not: 0). */
    double collapse_precision;
} rpvg_hip_em_problems;

typedef struct rpvg_hip_em_results {
    double * abundances;   /* host [col_off[P]]  expected read count per column, laid out like col_path */
    double * noise_count;  /* host [P] */
    double * total_count;  /* host [P] */
    uint32_t * iterations; /* host [P] EM iterations executed */
} rpvg_hip_em_results;

/* For every problem: build the row-normalised probability matrix of the
 * column subset with the noise column appended, and run the EM fixed point
 * to the reference's stop rule; everything on the GPU.  Takes over
 *   constructPartialProbabilityMatrix       src/path_estimator.cpp:79-113
 *   addNoiseAndNormalizeProbabilityMatrix   src/path_estimator.cpp:156-166
 *   EMAbundanceEstimator                    src/path_abundance_estimator.cpp:47-114
 * (start value 1/float(C), convergence over components >= 1e-8 for 10
 * consecutive iterations, sub-1e-8 abundances moved to noise_count) and, with
 * problems->collapse_precision > 0,
 *   readCollapseProbabilityMatrix           src/path_estimator.cpp:219-259
 * between the normalisation and the EM: the rows of every problem are put through the reference's tolerant
 * sort and compare-with-run-head merge (the machinery of the group matrices' collapse on the sparse rows); a
 * merged row's read count moves to its run head, and the EM kernels read the merged counts of the problems in
 * which rows were merged.  Rows whose columns all fall into the same multiple of 2^-44 stand for each other
 * there (and merges of rows equal to 1e-13 relative are not replayed: they move nothing; docs/design/kernels-collapse.md).
 * Rows without any selected path are folded into one exact scalar (docs/design/kernels-em.md). */
int rpvg_hip_em_solve(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t max_em_its, double max_rel_em_conv,
                      const rpvg_hip_em_problems * problems, rpvg_hip_em_results * results);

/* gibbsReadCountSampler (src/path_abundance_estimator.cpp:116-212) for a batch of EM problems, on the GPU.
 * Problem p starts from its EM estimate (init_abundances laid out like col_path, in expected read counts,
 * plus init_noise_count[p]) and records num_samples[p] states, one every gibbs_thin_its iterations.
 * Random numbers come from the counter-based Philox4x32-10 generator keyed by seeds[p]: the reference's
 * mt19937 / libstdc++ distribution streams cannot be reproduced on a GPU, parity is statistical.
 * noise_samples: [sum num_samples]; abundance_samples: per problem num_samples[p] x columns, sample-major
 * (the layout of CountSamples::abundance_samples, src/path_cluster_estimates.hpp:35-43).
 * There is no limit on the columns of a problem (rows, entries and iterations: below 2^32 each).  Two routes: a problem runs all its iterations on ONE
 * workgroup (abundances and counts in LDS; its generator is keyed by seeds[p] and streamed by (p, thread), so its samples
 * depend on its index in the call) unless its columns do not fit that workgroup's LDS (~10 000) or its kept rows + entries
 * reach the sampler's threshold (2^16; RPVG_HIP_EM_GRID_MIN_WORK, the EM's variable, overrides it; 0: never for its size).
 * Such a problem takes the whole GPU, one round of launches per iteration (rpvg_amd/csrc/gibbs_grid.hip); its generator is
 * keyed by seeds[p] and counted by (row or column, iteration, draw), so its samples depend on its seed and its data alone:
 * not on its index in the call, on what else is in the call, or on the GPU's size.  The dense problems of the EM's dense
 * route run on their compacted CSR here. */
int rpvg_hip_gibbs_read_counts(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_em_problems * problems,
                               const double * init_abundances, const double * init_noise_count,
                               const uint32_t * num_samples, const uint64_t * seeds, uint32_t gibbs_thin_its,
                               double gamma, double * noise_samples, double * abundance_samples);

/* Same EM on a dense matrix that is already resident on the GPU: row-major,
 * `ld` doubles between rows (ld even), columns [0, C-1) = paths and column
 * C-1 = noise, already normalised; counts = read count per row.  Used for
 * clusters large enough to stream from HBM (one 1M x 2k cluster = 16 GB).
 * abundances (host) receives C-1 values. */
int rpvg_hip_em_dense(rpvg_hip_ctx * ctx, const double * device_matrix, uint64_t num_rows, uint32_t num_cols,
                      uint64_t ld, const double * device_counts, double total_count, uint32_t max_em_its,
                      double max_rel_em_conv, double * abundances, double * noise_count, uint32_t * iterations);

/* Row-sharded form of rpvg_hip_em_dense for ONE cluster spread over the ranks of the context's
 * communicator (rpvg_hip_comm_init): this rank holds num_rows of the cluster's rows; total_count is
 * the read count of the WHOLE cluster.  Every EM iteration all-reduces the C partial column sums
 * t_j = sum_i (c_i / s_i) P_ij over the ranks (RCCL, queued on the context's stream between the
 * streaming pass and the update), then every rank applies the identical update and convergence test
 * (src/path_abundance_estimator.cpp:58-97), so all ranks stop at the same iteration and return the
 * same abundances.  With a one-rank communicator it equals rpvg_hip_em_dense. */
int rpvg_hip_em_dense_sharded(rpvg_hip_ctx * ctx, const double * device_matrix, uint64_t num_rows, uint32_t num_cols,
                              uint64_t ld, const double * device_counts, double total_count, uint32_t max_em_its,
                              double max_rel_em_conv, double * abundances, double * noise_count, uint32_t * iterations);

/* Builds the dense normalised matrix (layout above) of one cluster of an
 * uploaded batch, all paths + noise (constructProbabilityMatrix +
 * addNoiseAndNormalizeProbabilityMatrix, src/path_estimator.cpp:55-77,156-166).
 * device_matrix needs R*ld doubles, device_counts R doubles. */
int rpvg_hip_dense_from_cluster(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t cluster,
                                double * device_matrix, uint64_t ld, double * device_counts, double * total_count);

/* ---- group (haplotype / diplotype) log-likelihoods ---------------------- */
/* A group matrix has one column per path group: M[i][g] = sum of the row's
 * probabilities over the paths of group g (constructGroupedProbabilityMatrix,
 * src/path_estimator.cpp:115-154; a group of one path gives
 * constructProbabilityMatrix).  normalise != 0 applies
 * addNoiseAndNormalizeProbabilityMatrix (as NestedPathAbundanceEstimator does,
 * src/path_abundance_estimator.cpp:440-446); 0 keeps raw probabilities (as
 * PathGroupPosteriorEstimator does, src/path_posterior_estimator.cpp:45). */
typedef struct rpvg_hip_group_spec {
    uint32_t num_matrices;
    const uint32_t * cluster;         /* host [M]   */
    const uint64_t * group_off;       /* host [M+1] columns of each matrix, range into group_path_off */
    const uint64_t * group_path_off;  /* host [G+1] */
    const uint32_t * group_path;      /* host       cluster-local paths of each column (a set: list a path once) */
    int32_t normalise;
    /* > 0 (normalised matrices only): replay readCollapseProbabilityMatrix (src/path_estimator.cpp:197-259, called
     * on every normalised group matrix, src/path_abundance_estimator.cpp:380,443) with this prob_precision — every
     * row takes the values of the head of its run in the reference's tolerant row order; 0: rows stay as built.
     * With the collapse a call takes at most 2^20 - 1 matrices and 2^31 - 1 rows (RPVG_HIP_ERR_INVALID beyond: the
     * matrices of a larger batch are built in several calls). */
    double collapse_precision;
} rpvg_hip_group_spec;

/* Returns once the build is queued on the context's stream (the spec arrays have been consumed by then); a group that
 * refers to a path outside its cluster (or, with RPVG_HIP_BUILD_MASKS=1, lists a path twice: the columns of
 * constructGroupedProbabilityMatrix are sets of paths, src/path_abundance_estimator.cpp:493-546) is reported by the first call that uses the matrices
 * (RPVG_HIP_ERR_INVALID from rpvg_hip_group_loglik / _conditionals / rpvg_hip_bounded_pair_posteriors). */
int rpvg_hip_groups_build(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_group_spec * spec,
                          rpvg_hip_groups ** groups_out);
/* The matrices of NestedPathAbundanceEstimator::inferAbundancesCollapsedGroups (src/path_abundance_estimator.cpp:428-446) for
 * the listed clusters, their columns being the batch's own haplotype columns: findPathSourceGroups
 * (src/path_abundance_estimator.cpp:493-546) ran on the device when the batch was uploaded with PathInfo::source_ids
 * (rpvg_hip_batch_upload; rpvg_amd/csrc/path_sources.hip), so no column list crosses the ABI.  Column c of a matrix is the
 * c-th distinct path list among its cluster's haplotypes in ascending order of the smallest haplotype id that carries it; the
 * columns' multiplicities (path_counts) stay on the device with the matrices: rpvg_hip_bounded_pair_posteriors and
 * rpvg_hip_nested_subset_em take column_counts = NULL for them.  Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing,
 * for a batch without device-resident columns (the caller groups on the host and calls rpvg_hip_groups_build). */
int rpvg_hip_groups_build_from_sources(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_matrices,
                                       const uint32_t * clusters, int32_t normalise, double collapse_precision,
                                       rpvg_hip_groups ** groups_out);
/* The matrices whose column c is path c of the cluster alone — the raw path posteriors of PathPosteriorEstimator /
 * PathGroupPosteriorEstimator (src/path_posterior_estimator.cpp:9-31, 35-71: one group per path) — for the listed clusters: the
 * same matrices as rpvg_hip_groups_build with one single-entry list per path, without the lists crossing the ABI (configs[4]:
 * 500 000 of them per batch, flattened, copied and uploaded every call). */
int rpvg_hip_groups_build_single_paths(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_matrices,
                                       const uint32_t * clusters, int32_t normalise, double collapse_precision,
                                       rpvg_hip_groups ** groups_out);
void rpvg_hip_groups_free(rpvg_hip_ctx * ctx, rpvg_hip_groups * groups);
/* What the row collapse of these matrices did (waits for their build; any output may be NULL): matrices that held
 * rows within collapse_precision of each other but not equal up to rounding, whose runs were therefore replayed as
 * the reference forms them; rows that took the values of their run head and were changed by it (a bit-for-bit copy of
 * its head is not counted); matrices that were sorted as a whole
 * (otherwise only the rows close to such a pair are); rows that took part in a replay. */
int rpvg_hip_groups_collapse_info(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t * matrices_replayed,
                                  uint32_t * rows_replaced, uint32_t * matrices_sorted_whole, uint32_t * active_rows);
/* A test entry, not part of the estimators' path: matrix `matrix` as its readers see it, copied to the host — values_out [R * G]
 * column-major (column g at values_out + g * R), noise_out, rowmax_out and count_out [R], the rows in the matrix's own order (a
 * permutation of its cluster's rows that does not depend on collapse_precision).  It waits for the row collapse like every
 * reader, so a last stage that was held back for the search is queued first and the rows of every run hold their head's
 * values.  RPVG_HIP_ERR_INVALID for a NULL argument (outputs of a matrix without rows may be NULL) or a matrix out of range. */
int rpvg_hip_groups_rows(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t matrix, double * values_out, double * noise_out,
                         double * rowmax_out, double * count_out);
/* A test entry, not part of the estimators' path: the segment sort at the head of the row collapse on caller-supplied words, so
 * that its network is testable without a whole collapse.  Segment s is words[segment_off[s] .. segment_off[s + 1])
 * (segment_off[0] = 0, ascending, num_segments + 1 entries, fewer than 2^31 words in all); out receives every segment's words
 * in ascending order, at the segment's place.  The words of a segment must be distinct and below UINT64_MAX (the collapse's
 * words carry their row; UINT64_MAX pads).  It runs the device routines and launches of the collapse — the small kernel for
 * segments of up to 1 024 words, the chunk kernel, the merge rounds the longest segment needs, the read-back of every
 * chunked segment from the buffer its own last round left it in — without the computation of the rows' keys and without
 * the positions, "equal to its predecessor" and stretch starts the collapse writes. */
int rpvg_hip_segment_sort_words(rpvg_hip_ctx * ctx, const uint64_t * words, const uint64_t * segment_off, uint32_t num_segments,
                                uint64_t * out);

/* Evaluates, for every request q,
 *   out[q] = sum_i count_i * log( noise_i + ( sum_{m < width, members[q*width+m] != UINT32_MAX}
 *                                             M[i][members[q*width+m]]  +  (add_rowmax[q] ? max_g M[i][g] : 0) ) / divisor )
 * on matrix[q].  This is the `read_counts * (...).array().log().matrix()`
 * contraction of calculatePathGroupPosteriorsFull (src/path_estimator.cpp:354-361),
 * calculatePathGroupPosteriorsBounded (:424-427 with add_rowmax, :439) and the
 * conditional of estimatePathGroupPosteriorsGibbs (:527-545); adding log
 * frequencies, permutation counts, pruning and log-sum-exp stay on the host. */
int rpvg_hip_group_loglik(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_requests,
                          const uint32_t * matrix, const uint32_t * members, uint32_t width, double divisor,
                          const uint8_t * add_rowmax, double * out);

/* A whole conditional of estimatePathGroupPosteriorsGibbs (src/path_estimator.cpp:527-545) per request: request q
 * fixes the other width-1 members of a group (others[q*(width-1) ..], slot order) on matrix[q] and receives, for
 * EVERY column k of that matrix,
 *   sum_i count_i * log( noise_i + ( sum_o M[i][others] + M[i][k] ) / divisor ).
 * out holds the requests back to back, one value per column of the request's matrix.  Same arithmetic as
 * rpvg_hip_group_loglik with members = (others..., k); the request list is O(1) per conditional instead of O(columns). */
int rpvg_hip_group_conditionals(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_requests,
                                const uint32_t * matrix, const uint32_t * others, uint32_t width, double divisor,
                                double * out);

/* ---- full enumeration of the group posteriors, on the device ---------------------- */
/* calculatePathGroupPosteriorsFull (src/path_estimator.cpp:332-377) for group sizes 1 .. 8: for every problem q (matrix[q]
 * of `groups`, G_q columns) the posterior of every multiset of group_size columns,
 *   exp( sum_i count_i * log( noise_i + sum_m M[i][m] / group_size ) + sum_m log_freq[m] + log(numPermutations) - logsum ),
 * in lexicographic order of the non-decreasing member lists (the order of PathClusterEstimates::generateGroups), the
 * rpvg_hip_full_set_count(G_q, group_size) sets of each problem back to back in `posteriors`.  The sets are enumerated
 * on the device from their ranks; log_freq holds calcPathLogFrequences of every column, problems back to back.
 * numPermutations is the reference's n! / (n - u + 1)! truncated to an integer (src/utils.hpp:95-117, u distinct members:
 * the multinomial only up to n = 3).  logsum is formed per problem as max + log(sum exp(x - max)) in a fixed order (two
 * calls give the same bits; the reference folds add_log set by set: the last bits may differ).
 * Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing, when a problem has more than RPVG_HIP_FULL_MAX_SETS sets.
 * A batch is split into launches of at most 2^27 sets (one larger problem alone). */
#define RPVG_HIP_FULL_MAX_SETS 0x7fffffffull
int rpvg_hip_group_full_posteriors(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, uint32_t num_problems,
                                   const uint32_t * matrix, uint32_t group_size, const double * log_freq,
                                   double * posteriors);
/* C(columns + group_size - 1, group_size): the multisets of group_size out of `columns` (0 for no columns); UINT64_MAX when
 * it does not fit in 64 bits. */
uint64_t rpvg_hip_full_set_count(uint32_t columns, uint32_t group_size);

/* ---- the Gibbs sampler of the group posteriors, on the device ---------------------- */
/* estimatePathGroupPosteriorsGibbs (src/path_estimator.cpp:475-589) for group sizes 1 and 2, draw for draw up to the
 * floating-point reduction order of a distribution's sums (the conditional's log-sum-exp, the weight sum and the partial sums
 * are added wave-parallel here, one after the other in std::discrete_distribution: a last-ulp difference in a partial sum can
 * move a draw that lands exactly on a boundary — never seen in 1 300 swept configurations, not excluded): the chains
 * of every problem (:505), their starts (uniform_int_distribution, :491,509), the conditional of a slot given the other
 * member (:527-555: the contraction of rpvg_hip_group_conditionals, + log frequency, log-sum-exp, exp, then
 * std::discrete_distribution's own normalisation and partial sums), one draw per slot and iteration (:556) and the
 * counting of the sorted sets after the burn-in (:559-574).  The generators are the caller's std::mt19937s: the caller
 * passes the NEXT 624 outputs of each (drawn from a copy) — their untempered values are the generator's state — and
 * moves the original past the words_consumed[g] words the chains took (discard(), or the state words of the view), which
 * leaves it where the reference's sampler would.
 * Problems that share a generator (the transcripts of one cluster, src/path_abundance_estimator.cpp:371-412) are listed
 * under it in the order the reference runs them.  libstdc++'s streams (GCC 11: Lemire's rejection for the starts, two
 * words per generate_canonical<double, 53>, no draw at all from a distribution of fewer than two weights) are restated in
 * rpvg_amd/csrc/gibbs_streams.hpp and checked against libstdc++ on the CPU (tests/cpp/gibbs_streams_check.cpp).
 * The chain counts and lengths are the caller's (src/path_estimator.cpp:501-503).
 * The sets of a problem come in the order the reference appends them to path_group_sets (first appearance).
 * Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing, for other group sizes, when the distributions outgrow the
 * memory reserved for them (RPVG_HIP_GIBBS_BYTES; default: room for every column of every problem as the other member,
 * at most a quarter of the free device memory and 32 GiB) and when the chains are not done after 8 192 rounds of requests:
 * the caller then drives the sampler itself through rpvg_hip_group_conditionals. */
typedef struct rpvg_hip_gibbs_spec {
    uint32_t num_problems;
    uint32_t group_size;                    /* rpvg_hip_group_gibbs: 1 or 2; rpvg_hip_group_gibbs_polyploid: 3 .. 8    */
    const uint32_t * matrix;                /* [P]   matrix of `groups` the problem samples on                         */
    const uint32_t * num_chains;            /* [P]   :501                                                              */
    const uint32_t * num_burn_its;          /* [P]   :502                                                              */
    const uint32_t * num_gibbs_its;         /* [P]   :503                                                              */
    const double * log_freq;                /*       calcPathLogFrequences of every column, problems back to back      */
    uint32_t num_generators;
    const uint32_t * generator_problem_off; /* [NG+1]                                                                  */
    const uint32_t * generator_problem;     /* [P]   the problems of each generator, in the order it serves them       */
    const uint32_t * generator_words;       /* [NG x 624] the next 624 outputs of each generator                       */
} rpvg_hip_gibbs_spec;

typedef struct rpvg_hip_gibbs_sets rpvg_hip_gibbs_sets;
typedef struct rpvg_hip_gibbs_sets_view {
    uint32_t num_problems;
    uint32_t group_size;
    const uint64_t * set_off;        /* [P+1] sampled sets of each problem                                             */
    const uint32_t * first;          /* [sets] smaller member (the member, for group size 1); NULL for group sizes 3 .. 8 */
    const uint32_t * second;         /* [sets] larger member; NULL for group sizes 3 .. 8                              */
    const uint32_t * count;          /* [sets] samples that produced the set (:573); posterior = count / (chains x its) */
    const uint64_t * words_consumed; /* [NG]  32-bit words the sampler took from each generator                        */
    const uint32_t * generator_state;/* [NG x 624] for a generator that gave at least 624 words: the state words before its
                                      * next output — seeding the std::mt19937 with a seed sequence that hands these out
                                      * ([rand.eng.mers]: copied into the state, regenerated on the next call) continues
                                      * the stream at output words_consumed[g]; others are moved by discard()          */
    uint32_t rounds;                 /* rounds of (advance, conditionals) the call queued                              */
    uint64_t conditionals;           /* conditional distributions evaluated                                            */
    const uint32_t * members;        /* [sets x group_size] rpvg_hip_group_gibbs_polyploid: every set ascending, the sets of
                                      * a problem in order of first appearance; NULL from rpvg_hip_group_gibbs          */
} rpvg_hip_gibbs_sets_view;

int rpvg_hip_group_gibbs(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, const rpvg_hip_gibbs_spec * spec,
                         rpvg_hip_gibbs_sets ** result_out);
/* The same sampler for group sizes 3 .. 8 (same spec, same result type; the view's `members` instead of `first` / `second`),
 * draw for draw on the caller's generators: group_size start draws per chain, two words per conditional draw.
 * The conditional of a slot depends on the multiset of the other group_size - 1 members, so the memo of a problem is a hash
 * table keyed by those members, sorted and packed into 64 bits, floor(64 / group_size) bits each with all-ones reserved: a
 * problem may have at most 2 097 151 columns at group size 3, 65 535 at 4, 4 095 at 5, 1 023 at 6, 511 at 7 and 255 at 8.
 * The others are added to a row's noise in ascending column order (the reference adds them in the slot order of whichever
 * chain asks first): a distribution's bits do not depend on which chain got there first, and can differ from the
 * host-driven sampler's in the last bit of a row's base.
 * Both tables of a problem are sized from what its chains can make — sampled sets: min(multisets of group_size columns,
 * chains x its); conditionals: min(multisets of group_size - 1 columns, chains x (burn + its) x group_size) — times two,
 * rounded up to a power of two; 16 bytes per set slot, 48 per conditional slot, together at most a quarter of the free
 * device memory and 16 GiB.  The distributions (32 bytes per column each) are handed out of RPVG_HIP_GIBBS_BYTES (default: a
 * quarter of the free device memory, at most 32 GiB) as they are asked for.
 * Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing, for other group sizes, a problem with more columns than the key
 * holds, tables or distributions that outgrow their memory and chains not done after 8 192 rounds: the caller then drives
 * the sampler itself through rpvg_hip_group_conditionals.  RPVG_HIP_ERR_INVALID for a matrix index out of range. */
int rpvg_hip_group_gibbs_polyploid(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, const rpvg_hip_gibbs_spec * spec,
                                   rpvg_hip_gibbs_sets ** result_out);
int rpvg_hip_gibbs_sets_get(const rpvg_hip_gibbs_sets * result, rpvg_hip_gibbs_sets_view * view_out);
void rpvg_hip_gibbs_sets_free(rpvg_hip_gibbs_sets * result);

/* The whole diploid branch-and-bound of calculatePathGroupPosteriorsBounded
 * (src/path_estimator.cpp:379-473) on the GPU, one workgroup per matrix:
 * marginal posteriors (the nested group-size-1 Full call, :397-412), the
 * descending (posterior, index) order (:412), the optimistic bound of each
 * first column (:414,424-433), the pair loop with its running-maximum pruning
 * in the reference's exact sequence (:435-450), the late-loser zeroing and the
 * log-sum-exp normalisation (:453-470).  column_counts holds `path_counts` of
 * every column of every matrix, concatenated in matrix order.  The result
 * lists, per matrix, the kept pairs in the order the reference keeps them. */
typedef struct rpvg_hip_pair_posteriors rpvg_hip_pair_posteriors;

typedef struct rpvg_hip_pair_posteriors_view {
    uint32_t num_matrices;
    const uint64_t * pair_off;   /* [M+1] kept pairs of each matrix            */
    const uint32_t * first;      /* [pairs] column index (first path)          */
    const uint32_t * second;     /* [pairs] column index (second path)         */
    const double * posterior;    /* [pairs]                                    */
} rpvg_hip_pair_posteriors_view;

int rpvg_hip_bounded_pair_posteriors(rpvg_hip_ctx * ctx, const rpvg_hip_groups * groups, const uint32_t * column_counts,
                                     double min_rel_likelihood, rpvg_hip_pair_posteriors ** result_out);
int rpvg_hip_pair_posteriors_get(const rpvg_hip_pair_posteriors * result, rpvg_hip_pair_posteriors_view * view_out);
void rpvg_hip_pair_posteriors_free(rpvg_hip_pair_posteriors * result);

/* ---- diploid search -> retained path subsets -> EM, in one call ------------------- */
/* NestedPathAbundanceEstimator::inferAbundancesCollapsedGroups (src/path_abundance_estimator.cpp:428-471) from the group
 * matrices on: rpvg_hip_bounded_pair_posteriors, then selectPathSubsetIndices (:569-606: diplotypes with posterior >=
 * min_hap_prob, each expanded to the sorted list of the paths of its two haplotype columns, identical lists merged,
 * weights renormalised), then for every subset that keeps a weight >= min_hap_prob (:627-630) the EM of rpvg_hip_em_solve
 * on its distinct paths (:637-671; collapse_precision as in rpvg_hip_em_problems: the subset's rows are collapsed first, :668) —
 * with nothing but a 64-byte header crossing to the host in between (round 2 made two
 * round trips there: 1.2 ms of a lane's critical path at 32 host threads, 8 ms at 4).  The posterior-weighted merge of
 * the solutions (:702-749) stays with the caller.
 * Subsets of a matrix come in lexicographic order of their path lists.  Returns RPVG_HIP_ERR_UNSUPPORTED, having changed
 * nothing, when it does not take the input (min_hap_prob below 1/1024; a cluster too wide for LDS-resident EM vectors;
 * more subsets than the capacity it reserved — it then reserves by what it saw on the next call): the caller makes the
 * three calls instead. */
typedef struct rpvg_hip_subset_em rpvg_hip_subset_em;
typedef struct rpvg_hip_subset_em_view {
    uint32_t num_matrices;
    const uint64_t * subset_off;   /* [M+1] retained subsets of each matrix                                        */
    const double * weight;         /* [S]   normalised posterior mass of the subset (:602-605)                        */
    const uint64_t * path_off;     /* [S+1]                                                                          */
    const uint32_t * path;         /*       sorted cluster-local paths of the subset, a homozygous path twice (:583-593) */
    const uint64_t * col_off;      /* [S+1]                                                                          */
    const uint32_t * col_path;     /*       its distinct paths = the columns of its EM problem (:637-656)            */
    const double * abundances;     /*       expected read counts, laid out like col_path                             */
    const double * noise_count;    /* [S]                                                                            */
    const double * total_count;    /* [S]                                                                            */
    const uint32_t * iterations;   /* [S]   EM iterations executed                                                   */
    /* The posterior-weighted merge of the solutions (src/path_abundance_estimator.cpp:702-749), done on the device when the
     * batch was uploaded with PathInfo::group_id (rpvg_cluster_batch::path_group_id); all NULL otherwise.  The path group
     * sets of matrix m — one per (transcript, paths of that transcript in a retained subset), in lexicographic order of their
     * path lists — sit in the slots [path_off[subset_off[m]], + set_count[m]) of the set_* arrays: one path (set_second =
     * UINT32_MAX) or two, the sum of the weights of the subsets that hold the set, and per path the sum over those subsets of
     * weight x abundance / multiplicity, added in subset order with the host's roundings (bit-equal to the host merge).
     * cluster_noise_count[m] = sum of weight x noise_count over the subsets + (1 - sum of weights) x total_count (:712,749);
     * a matrix without retained subsets has set_count 0 and leaves its noise count (= its total count) to the caller. */
    const uint32_t * set_count;           /* [M] */
    const double * cluster_noise_count;   /* [M] */
    const uint32_t * set_first;
    const uint32_t * set_second;
    const double * set_posterior;
    const double * set_abundance;         /* two per set slot */
} rpvg_hip_subset_em_view;
int rpvg_hip_nested_subset_em(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups,
                              const uint32_t * column_counts, double min_rel_likelihood, double min_hap_prob,
                              uint32_t max_em_its, double max_rel_em_conv, double collapse_precision,
                              rpvg_hip_subset_em ** result_out);
int rpvg_hip_subset_em_get(const rpvg_hip_subset_em * result, rpvg_hip_subset_em_view * view_out);
void rpvg_hip_subset_em_free(rpvg_hip_subset_em * result);

/* ---- full enumeration -> retained sets -> path subsets -> EM -> weighted merge, in one call: group sizes 1 and 3 .. 8 ---- */
/* NestedPathAbundanceEstimator::inferAbundancesCollapsedGroups (src/path_abundance_estimator.cpp:428-471) with exact posteriors at
 * any ploidy but two (rpvg_hip_nested_subset_em is the diploid call): the posteriors of rpvg_hip_group_full_posteriors (same kernels,
 * same launches of at most 2^27 sets, log_freq as there: the columns of every matrix of `groups` back to back), the sets with
 * posterior >= min_hap_prob kept per matrix in ascending rank (src/path_abundance_estimator.cpp:574-600), each expanded to the
 * ascending concatenation of the path lists of its group_size columns, identical lists merged (masses added in ascending rank, then
 * one division by the sum over the kept sets), subsets in lexicographic order of their lists, the EM of rpvg_hip_em_solve on every
 * subset's distinct paths, and the posterior-weighted merge (:702-749) for sets of up to group_size paths of one transcript.  No
 * array proportional to the number of sets reaches the host or outlives its launch.
 * Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing, with rpvg_hip_last_error naming the reason: group size 0, 2 or above 8;
 * min_hap_prob below 1/1024; a matrix with more than RPVG_HIP_FULL_MAX_SETS sets; a cluster too wide for LDS-resident EM vectors; a
 * batch uploaded without path_group_id; RPVG_HIP_NO_DEVICE_SUBSETS in the environment (read per call); capacities that did not
 * fit after one retry; a transcript with more than group_size paths in one subset. */
typedef struct rpvg_hip_subset_em_sets_view {
    uint32_t num_matrices;
    uint32_t group_size;
    const uint64_t * subset_off;   /* [M+1]  as rpvg_hip_subset_em_view, from here ...                              */
    const double * weight;         /* [S]                                                                            */
    const uint64_t * path_off;     /* [S+1]                                                                          */
    const uint32_t * path;         /*        sorted cluster-local paths, a path once per column of the set that lists it */
    const uint64_t * col_off;      /* [S+1]                                                                          */
    const uint32_t * col_path;
    const double * abundances;
    const double * noise_count;    /* [S]                                                                            */
    const double * total_count;    /* [S]                                                                            */
    const uint32_t * iterations;   /* [S]    ... to here                                                             */
    /* the sets the first stage kept: of matrix m [retained_off[m], retained_off[m + 1]), ascending by rank; the rank is the set's
     * position in the order of rpvg_hip_group_full_posteriors (lexicographic among the multisets of the matrix's columns) */
    const uint64_t * retained_off;        /* [M+1] */
    const uint64_t * retained_rank;
    const double * retained_posterior;
    /* the merged path group sets: those of matrix m in the slots [path_off[subset_off[m]], + set_count[m]), in lexicographic order of
     * their member lists (a shorter list before its extensions); members in list order, repeats kept */
    const uint32_t * set_count;           /* [M]                                                   */
    const double * cluster_noise_count;   /* [M]                                                   */
    const uint32_t * set_size;            /* members of the set: 1 .. group_size                   */
    const uint32_t * set_member;          /* group_size per slot, unused cells UINT32_MAX          */
    const double * set_posterior;
    const double * set_abundance;         /* group_size per slot, unused cells 0                   */
} rpvg_hip_subset_em_sets_view;
int rpvg_hip_nested_full_subset_em(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups,
                                   uint32_t group_size, const double * log_freq, double min_hap_prob, uint32_t max_em_its,
                                   double max_rel_em_conv, double collapse_precision, rpvg_hip_subset_em ** result_out);
int rpvg_hip_subset_em_get_sets(const rpvg_hip_subset_em * result, rpvg_hip_subset_em_sets_view * view_out);

/* ---- independent haplotype inference: posteriors -> draws -> path subsets -> EM -> weighted merge, in one call: group sizes 1 .. 8 ---- */
/* NestedPathAbundanceEstimator::inferAbundancesIndependentGroups (src/path_abundance_estimator.cpp:356-426) with exact posteriors.
 * The unit of the call is the CLUSTER: its transcripts are consecutive matrices of `groups`, each with one column per path of the
 * transcript (one path per column), normalised and row-collapsed (:379-380).  Per transcript the posteriors of
 * rpvg_hip_bounded_pair_posteriors (group size 2, min_rel_likelihood = min_hap_prob, :403; the kept pairs in the reference's order,
 * late losers listed with posterior 0) or rpvg_hip_group_full_posteriors (every other group size; EVERY set is a weight) stay on the
 * device; a std::discrete_distribution is constructed over them as libstdc++ does (rpvg_amd/csrc/gibbs_streams.hpp: one chain of
 * additions for the sum, separately rounded quotients, one chain for the partial sums, the last one 1.0; fewer than two sets draw
 * nothing), and S = floor(1 / min_hap_prob) sets per transcript are drawn from the cluster's std::mt19937 draw for draw (:548-567):
 * the caller passes the NEXT 624 outputs of each cluster's generator, drawing transcript d of a cluster takes the words
 * [2 S d, 2 S (d + 1)) of its stream, two per draw, the first one the low part.  Sample slot s of a cluster is the union over its
 * transcripts of the paths of the set drawn for slot s, sorted (a homozygous path twice); identical samples are one subset whose
 * weight is the CHAIN of as many additions of 1 / double(S) from 0.0 as samples produced it (:421) — 1 000 of 0.001 give
 * 1.0000000000000007 —, retained when that weight is >= min_hap_prob (:627-630).  Subsets of a cluster come in lexicographic order
 * of their path lists; the EM of rpvg_hip_em_solve on every subset's distinct paths and the posterior-weighted merge (:702-749) follow as
 * in rpvg_hip_nested_full_subset_em.  cluster_noise_count is unclamped and may be a hair negative, as on the host.
 * The caller moves every cluster's generator past words_consumed[k] words (discard(), or the state words of the view, as with
 * rpvg_hip_gibbs_sets_view); the call itself moves nothing.  The caveat of the Gibbs sampler holds here too: posteriors that differ
 * from another implementation's in their last bits can move a draw that falls within an ulp of a partial sum.
 * Returns RPVG_HIP_ERR_UNSUPPORTED, having changed nothing, with rpvg_hip_last_error naming the reason: group size 0 or above 8;
 * min_hap_prob below 1/1024 or above 1; a transcript with more than 65 536 sets (one wavefront adds its sums as one chain); a matrix
 * with no set; a cluster too wide for LDS-resident EM vectors; a batch uploaded without path_group_id; RPVG_HIP_NO_DEVICE_SUBSETS
 * in the environment (read per call); capacities that did not fit after one retry.  RPVG_HIP_ERR_INVALID when the matrices of one
 * unit are not of one cluster, and when the columns of a unit's transcripts do not partition the cluster's paths by path_group_id. */
typedef struct rpvg_hip_independent_spec {
    uint32_t num_clusters;
    const uint32_t * matrix_off;      /* [K+1] the transcripts of unit k are the matrices [matrix_off[k], matrix_off[k+1]) of
                                         `groups`, in findPathGroups order (:473-491); all of one cluster of the batch */
    uint32_t group_size;              /* 1 .. 8 */
    const uint32_t * column_counts;   /* path_counts of every column, matrices back to back (group size 2) */
    const double * log_freq;          /* calcPathLogFrequences of every column (other group sizes) */
    double min_hap_prob;
    uint32_t max_em_its; double max_rel_em_conv; double collapse_precision;
    const uint32_t * generator_words; /* [K x 624] the next 624 outputs of each cluster's std::mt19937 */
    int32_t keep_draws;               /* tests: keep draw[k][slot][transcript] for rpvg_hip_independent_draws_get */
} rpvg_hip_independent_spec;

typedef struct rpvg_hip_subset_em_independent_view {
    uint32_t num_clusters;
    uint32_t group_size;
    uint32_t num_samples;          /* S = floor(1 / min_hap_prob)                                                    */
    const uint64_t * subset_off;   /* [K+1]  as rpvg_hip_subset_em_sets_view with clusters in place of matrices, from here ... */
    const double * weight;         /* [S]    the chain of sample_count additions of 1 / double(num_samples)          */
    const uint64_t * path_off;     /* [S+1]                                                                          */
    const uint32_t * path;         /*        sorted cluster-local paths: group_size per transcript, a homozygous path twice */
    const uint64_t * col_off;      /* [S+1]                                                                          */
    const uint32_t * col_path;
    const double * abundances;
    const double * noise_count;    /* [S]                                                                            */
    const double * total_count;    /* [S]                                                                            */
    const uint32_t * iterations;   /* [S]                                                                            */
    const uint32_t * set_count;           /* [K]                                                   */
    const double * cluster_noise_count;   /* [K]                                                   */
    const uint32_t * set_size;
    const uint32_t * set_member;
    const double * set_posterior;
    const double * set_abundance;  /*        ... to here                                                             */
    const uint32_t * sample_count;        /* [S]   samples that produced the subset                                  */
    const uint64_t * words_consumed;      /* [K]   2 x num_samples x (transcripts of the cluster with at least two sets) */
    const uint32_t * generator_state;     /* [K x 624] as rpvg_hip_gibbs_sets_view::generator_state, for words_consumed >= 624 */
} rpvg_hip_subset_em_independent_view;

typedef struct rpvg_independent_limits {
    uint32_t max_group_size;         /* 8 */
    uint32_t max_samples;            /* 1 024: min_hap_prob >= 1 / 1024 */
    uint64_t max_transcript_sets;    /* 65 536 */
    uint32_t words_per_draw;         /* 2 */
    uint32_t state_words;            /* 624 */
    uint64_t max_work_bytes;         /* draws and sample lists of one call */
} rpvg_independent_limits;

typedef struct rpvg_hip_independent_stats {
    uint64_t calls_completed;        /* calls that returned RPVG_HIP_OK with at least one cluster */
    uint64_t draws;                  /* sets drawn (two generator words each) */
    uint64_t subsets;                /* retained subsets = EM problems */
} rpvg_hip_independent_stats;

int rpvg_hip_nested_independent_subset_em(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_groups * groups,
                                          const rpvg_hip_independent_spec * spec, rpvg_hip_subset_em ** result_out);
int rpvg_hip_subset_em_get_independent(const rpvg_hip_subset_em * result, rpvg_hip_subset_em_independent_view * view_out);
/* the draws of unit `unit` (spec.keep_draws != 0): draws_out[slot x T + transcript], the index of the drawn set among the
 * transcript's posteriors; 0 for a transcript that draws nothing */
int rpvg_hip_independent_draws_get(const rpvg_hip_subset_em * result, uint32_t unit, uint32_t * draws_out);
void rpvg_hip_independent_limits(rpvg_independent_limits * limits_out);
/* counters of this call, kept apart from rpvg_hip_kernel_stats; rpvg_hip_stats_reset zeroes them too */
int rpvg_hip_independent_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_independent_stats * stats_out);

/* ---- minimum path cover (`-i strains`) ------------------------------------ */
/* For every listed cluster: the read-path cover and path weights of MinimumPathAbundanceEstimator::estimate
 * (src/path_abundance_estimator.cpp:233-257) and the greedy weightedMinimumPathCover (:297-340) on the GPU.
 * cover[cover_off[i] .. cover_off[i] + cover_size[i]) receives the ascending cover of clusters[i];
 * the range cover_off[i+1] - cover_off[i] must hold the cluster's number of paths (it may be larger: the cells behind
 * cover_size[i] are left as they are).  A cluster may be listed more than once: every entry of `clusters` is a problem
 * of its own.  The weight of a path is the sum of its terms in ascending row order, as the reference adds them: paths
 * with the same rows and probabilities tie exactly and the lower index is taken; two calls give the same covers.
 * A cluster may have at most 9600 paths (two vectors of doubles per path in LDS); a call that lists a larger one fails
 * with RPVG_HIP_ERR_INVALID before anything is launched.  A cluster of one path has the cover {0}; a cluster none of
 * whose rows count (noise probability 1) has the empty cover. */
int rpvg_hip_min_path_cover(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters,
                            const uint32_t * clusters, const uint64_t * cover_off, uint32_t * cover, uint32_t * cover_size);
/* The same for clusters of any size: every listed cluster takes one of two routes (rpvg_amd/csrc/cover_plan.hpp) — the workgroup
 * route of rpvg_hip_min_path_cover (all such clusters of the call side by side in one launch), or the whole GPU, one cluster after
 * the other (rpvg_amd/csrc/path_cover_grid.hip): a cluster of more than rpvg_cover_limits::workgroup_max_paths paths, or of at
 * least grid_min_work rows + entries.  grid_min_work: 0 the library default (rpvg_cover_limits::default_grid_min_work), 1 every
 * cluster of at least two paths on the whole-GPU route, UINT64_MAX every cluster that fits on the workgroup route.  A cluster of
 * one path never takes the whole-GPU route.  Both routes add a path's weight up in the same order and give the same covers.
 * The first seven arguments are those of rpvg_hip_min_path_cover (the cells behind cover_size[i] are left as they are).
 * choice_order may be NULL; it has the ranges of `cover` and receives, for a cluster of the whole-GPU route, the paths of the
 * cover in the order the greedy rounds chose them; a cluster of the workgroup route gets UINT32_MAX in its first cell.
 * A cluster of the whole-GPU route with 2^31 rows or entries or more is refused with RPVG_HIP_ERR_INVALID (named in last_error)
 * before anything is launched. */
int rpvg_hip_min_path_cover_any(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t num_clusters,
                                const uint32_t * clusters, const uint64_t * cover_off, uint32_t * cover, uint32_t * cover_size,
                                uint64_t grid_min_work, uint32_t * choice_order);
/* the numbers of rpvg_amd/csrc/cover_plan.hpp */
typedef struct rpvg_cover_limits {
    uint32_t workgroup_max_paths;     /* the widest cluster of the workgroup route */
    uint32_t chunk_rounds;            /* greedy rounds queued between two looks at the control record */
    uint64_t default_grid_min_work;   /* rows + entries; UINT64_MAX: width only */
    uint64_t grid_max_rows;           /* the largest cluster of the whole-GPU route */
    uint64_t grid_max_entries;
    uint32_t pick_block;              /* threads of a workgroup of the pick kernel */
    uint32_t pick_per_thread;         /* paths of a thread within its workgroup's tile (pick_block apart) */
    uint32_t pick_max_blocks;
    uint32_t strike_block;
    uint32_t strike_max_blocks;
    uint32_t hist_max_paths;          /* the widest cluster whose struck gains go through an LDS histogram */
} rpvg_cover_limits;
void rpvg_hip_cover_limits(rpvg_cover_limits * limits_out);

/* ---- path clustering ------------------------------------------------------- */
/* PathClusters (src/path_clusters.cpp:12-86 constructor, :163-207 createPathClusters, :88-262 addNodeClusters +
 * mergeClusters): the paths of every id set — the paths one alignment-path list locates, or the paths through one
 * node — end up in one cluster.  Clusters are numbered by ascending smallest path id and list their members in
 * ascending order, as the reference does (test src/tests/path_clusters_test.cpp:82-87,130-135).
 * set s = set_path[set_off[s] .. set_off[s+1]) (non-empty; ids < num_paths).  Outputs (host): path_to_cluster
 * [num_paths]; *num_clusters_out; cluster_off[num_clusters + 1] (capacity num_paths + 1); cluster_paths [num_paths]. */
int rpvg_hip_path_clusters(rpvg_hip_ctx * ctx, uint32_t num_paths, uint64_t num_sets, const uint64_t * set_off,
                           const uint32_t * set_path, uint32_t * path_to_cluster, uint32_t * num_clusters_out,
                           uint64_t * cluster_off, uint32_t * cluster_paths);

/* ---- row construction: the step before the path (include/rpvg_rows.h) ------- */
/* ReadPathProbabilities::addPathProbs for every read of every cluster of the batch (src/read_path_probabilities.cpp:
 * 39-221) and, when merge != 0, the caller's sort + quickMergeIdentical of adjacent rows (src/main.cpp:953-973,
 * src/read_path_probabilities.cpp:223-322), on the GPU.
 *   rpvg_hip_alignments_upload   validates the alignment-path lists and makes them resident in HBM;
 *   rpvg_hip_read_rows_build     resident alignments -> resident rows (grouped layout of rpvg_cluster_batch; with
 *                                name-group collapsing the "paths" of a cluster are its groups);
 *   rpvg_hip_read_rows_to_batch  resident rows -> the rpvg_hip_batch the estimators take, without leaving the GPU;
 *   rpvg_hip_read_rows_sizes     the cluster offsets of the rows only (cluster_row_off, cluster_path_off; no copy);
 *   rpvg_hip_read_rows_view      host copy of the rows (row fields of rpvg_cluster_batch; valid until the rows are
 *                                freed) and the device time of the row kernels / of sort + merge + pack. */
typedef struct rpvg_hip_alignments rpvg_hip_alignments;
typedef struct rpvg_hip_read_rows rpvg_hip_read_rows;
int rpvg_hip_alignments_upload(rpvg_hip_ctx * ctx, const rpvg_alignment_batch * alignments, rpvg_hip_alignments ** out);
void rpvg_hip_alignments_free(rpvg_hip_ctx * ctx, rpvg_hip_alignments * alignments);
int rpvg_hip_read_rows_build(rpvg_hip_ctx * ctx, const rpvg_hip_alignments * alignments, const rpvg_row_params * params,
                             int32_t merge, rpvg_hip_read_rows ** rows_out);
int rpvg_hip_read_rows_to_batch(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, rpvg_hip_batch ** batch_out);
int rpvg_hip_read_rows_sizes(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, rpvg_cluster_batch * view);
int rpvg_hip_read_rows_view(rpvg_hip_ctx * ctx, rpvg_hip_read_rows * rows, rpvg_cluster_batch * view, double * build_ms,
                            double * merge_ms);
void rpvg_hip_read_rows_free(rpvg_hip_ctx * ctx, rpvg_hip_read_rows * rows);

/* ---- fragment-length model (rpvg_frag.h; rpvg_amd/csrc/frag_length.hip) ------------------------------------------
 *   rpvg_hip_frag_length_fit       FragmentLengthDist(counts, skew_normal) in one kernel launch of one workgroup.
 *                                  RPVG_HIP_ERR_INVALID for n == 0, counts[0] != 0 or n > 65536; fewer than two samples
 *                                  are RPVG_HIP_OK with valid = 0 (loc = the sum of the lengths, scale = shape = 0).
 *   rpvg_hip_frag_length_table     logProb(v), v = 0 .. 65535, computed into a device table that rpvg_row_params can name;
 *                                  _get copies it to the host ([RPVG_FRAG_LENGTH_TABLE_SIZE]).
 *   rpvg_hip_effective_lengths     PathsIndex::effectivePathLength for n path lengths (host arrays).
 *   rpvg_hip_alignments_set_effective_lengths   the same for the paths of a resident alignment batch: replaces its
 *                                  path_effective_length on the device and returns the values ([P], for PathInfo).
 *   rpvg_hip_frag_length_eval      for tests and measurements: rows of five doubles -> one double each.
 *                                  what = 0: skew_normal_cdf(x, m, s, a)   1: truncated mean (m, s, a, c, d)   2: Owen's T(h, a) */
int rpvg_hip_frag_length_fit(rpvg_hip_ctx * ctx, const uint32_t * counts, uint32_t n, int skew_normal, rpvg_frag_length_fit * out);
int rpvg_hip_frag_length_table(rpvg_hip_ctx * ctx, double loc, double scale, double shape, rpvg_hip_frag_table ** out);
int rpvg_hip_frag_length_table_get(rpvg_hip_ctx * ctx, const rpvg_hip_frag_table * table, double * log_prob_out);
void rpvg_hip_frag_length_table_free(rpvg_hip_ctx * ctx, rpvg_hip_frag_table * table);
int rpvg_hip_effective_lengths(rpvg_hip_ctx * ctx, double loc, double scale, double shape, const uint32_t * path_length, uint64_t n,
                               double * out);
int rpvg_hip_alignments_set_effective_lengths(rpvg_hip_ctx * ctx, rpvg_hip_alignments * alignments, double loc, double scale,
                                              double shape, const uint32_t * path_length, double * out);
int rpvg_hip_frag_length_eval(rpvg_hip_ctx * ctx, int what, const double * rows, uint64_t n, double * out);

/* ---- alignment-path index (rpvg_index.h; rpvg_amd/csrc/align_index.hip) ---------------------------------------------
 * A stream of per-fragment alignment-path lists in, a resident rpvg_hip_alignments in the reference's cluster order out
 * (addAlignmentPathsBufferToIndexes, src/main.cpp:200-237; PathClusters; the caller's loop, :731-754,811-827,846-857).
 *   rpvg_hip_align_index_create     RPVG_HIP_ERR_INVALID for max_frag_length >= 65536.
 *   rpvg_hip_align_index_add        copies one chunk to the device (pinned staging), validates it there and appends it;
 *                                   any number of times: the stream is the chunks in the order they were added.  A chunk
 *                                   that fails (RPVG_HIP_ERR_INVALID: the first offending list is named in last_error — a
 *                                   list without alignments, an alignment without paths, ids not ascending or >= num_paths,
 *                                   a noise score > 0, non-monotone offsets, a counted fragment length of 0 or above
 *                                   max_frag_length) leaves the index as it was.
 *   rpvg_hip_align_index_finish     histogram, normalisation, dedupe, clustering, ordering.  The optional extra id sets
 *                                   (set s = extra_set_path[extra_set_off[s] .. extra_set_off[s+1]), non-empty, ids <
 *                                   num_paths: the node-sharing sets of addNodeClusters) join the union-find of
 *                                   rpvg_hip_path_clusters.  Once; no chunk can be added afterwards.  info may be NULL.
 *   rpvg_hip_align_index_frag_counts   host copy of the histogram ([max_frag_length + 1]) for rpvg_hip_frag_length_fit.
 *   rpvg_hip_align_index_view       host copies of the result (rpvg_index_view).
 *   rpvg_hip_align_index_alignments the resident rpvg_hip_alignments that rpvg_hip_alignments_upload would have made from
 *                                   the view, without the lists leaving the device.  path_effective_length (and the
 *                                   optional path_source_count) are per GLOBAL path ([num_paths]);
 *                                   rpvg_hip_alignments_set_effective_lengths takes path lengths in the order of the view's
 *                                   cluster_paths.  Freed with rpvg_hip_alignments_free; independent of the index. */
int rpvg_hip_align_index_create(rpvg_hip_ctx * ctx, const rpvg_index_params * params, rpvg_hip_align_index ** index_out);
void rpvg_hip_align_index_free(rpvg_hip_ctx * ctx, rpvg_hip_align_index * index);
int rpvg_hip_align_index_add(rpvg_hip_ctx * ctx, rpvg_hip_align_index * index, const rpvg_fragment_lists * chunk);
int rpvg_hip_align_index_finish(rpvg_hip_ctx * ctx, rpvg_hip_align_index * index, const uint64_t * extra_set_off,
                                const uint32_t * extra_set_path, uint64_t num_extra_sets, rpvg_index_info * info);
int rpvg_hip_align_index_frag_counts(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * index, uint32_t * counts_out);
int rpvg_hip_align_index_view(rpvg_hip_ctx * ctx, rpvg_hip_align_index * index, rpvg_index_view * view_out);
int rpvg_hip_align_index_alignments(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * index, const double * path_effective_length,
                                    const uint32_t * path_source_count, rpvg_hip_alignments ** alignments_out);

/* ---- path table (rpvg_index.h; rpvg_amd/csrc/path_table.hip) ----------------------------------------------------------
 *   rpvg_hip_path_table_upload      copies the table to the device and validates it there: source_off non-decreasing and
 *                                   ending at num_sources (RPVG_HIP_ERR_INVALID, the first offending path named in last_error).
 *   rpvg_hip_read_rows_to_batch_with_paths   the batch of rpvg_hip_read_rows_to_batch plus its path side: path_group_id and the
 *                                   source-id lists gathered into the index's cluster order, the haplotype columns formed from
 *                                   them as rpvg_hip_batch_upload forms them, and the read total of every cluster.  The rows
 *                                   must be those of the index's clusters (not collapsed).  A table without source ids, or with
 *                                   more than 2^32 - 16 of them (the limit of rpvg_hip_batch_upload's columns), gives a batch
 *                                   without columns (rpvg_hip_batch_has_source_columns is 0: the caller groups on the host);
 *                                   its group ids and totals are filled all the same.  To the host come the 3K + 4 size words
 *                                   of the columns, the K + 1 slot offsets of the clusters and the K totals; no list.
 *   rpvg_hip_batch_path_group_ids   host copy of path_group_id ([paths of the batch]) of a batch that has a path side.
 *   rpvg_hip_align_index_name_groups   the name groups of every cluster and the collapsed PathInfo of every group (the table
 *                                   needs name_id).  RPVG_HIP_ERR_INVALID for a source count of 0 and for a group whose summed
 *                                   source count or length exceeds 32 bits (cluster and group named in last_error).
 *   rpvg_hip_align_index_alignments_collapsed   the resident rpvg_hip_alignments that rpvg_hip_alignments_upload would have
 *                                   made from the view with the groups' path_group / cluster_group_off and the table's source
 *                                   counts and effective lengths: every read on the list of the wavefront-per-read kernel. */
int rpvg_hip_path_table_upload(rpvg_hip_ctx * ctx, const rpvg_path_table * table, rpvg_hip_path_table ** table_out);
void rpvg_hip_path_table_free(rpvg_hip_ctx * ctx, rpvg_hip_path_table * table);
int rpvg_hip_read_rows_to_batch_with_paths(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, const rpvg_hip_align_index * index,
                                           const rpvg_hip_path_table * table, rpvg_hip_batch ** batch_out);
int rpvg_hip_batch_path_group_ids(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, uint32_t * group_ids_out);
void rpvg_hip_name_groups_limits(rpvg_name_groups_limits * limits_out);
int rpvg_hip_align_index_name_groups(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * index, const rpvg_hip_path_table * table,
                                     rpvg_hip_name_groups ** groups_out);
int rpvg_hip_name_groups_view(rpvg_hip_ctx * ctx, rpvg_hip_name_groups * groups, rpvg_name_groups_view * view_out);
void rpvg_hip_name_groups_free(rpvg_hip_ctx * ctx, rpvg_hip_name_groups * groups);
int rpvg_hip_align_index_alignments_collapsed(rpvg_hip_ctx * ctx, const rpvg_hip_align_index * index, const rpvg_hip_path_table * table,
                                              const rpvg_hip_name_groups * groups, rpvg_hip_alignments ** alignments_out);

/* ---- estimates table (rpvg_table.h; rpvg_amd/csrc/estimates_table.hip) ---------------------------------------------------
 *   rpvg_hip_estimates_table_build   the table of a batch's estimates, every sum in the order rpvg_table.h states: per path the
 *                                   haplotype probability and read count of HaplotypeAbundanceEstimatesWriter::addEstimates
 *                                   (src/threaded_output_writer.cpp:346-432), per member the transcript count of the joint writer
 *                                   (:434-546), per cluster its part of totalTranscriptCount (src/main.cpp:1029-1057) and their sum
 *                                   in cluster order, the noise totals of the `Unknown` rows (:283-343; evenly over `ploidy`
 *                                   columns :434-546).  Host arrays are copied as one block; device arrays (on_device = 1) are read
 *                                   where they lie.  One kernel validates behind the copy: RPVG_HIP_ERR_INVALID for offsets that
 *                                   are not non-decreasing from 0 to the array sizes, a member at or beyond its cluster's number
 *                                   of paths, or a cluster whose abundances are neither none nor one per member (the first such
 *                                   cluster is named in last_error).  To the host come one word for the first offender and three
 *                                   for the routes' numbers of clusters.
 *   rpvg_hip_estimates_table_tpm     transcript count / denominator * 1e6 for every path and member (the last step of the three
 *                                   writers' rows, :324, :413, :519): a second step because the denominator of a run spans batches
 *                                   and ranks; the table's own total_transcript_count when the batch is the run.
 *   rpvg_hip_estimates_table_view    host copies of the table, fetched as one packed copy when the table has changed.
 *   rpvg_hip_estimates_table_limits  the sizes at which a cluster changes its route (rpvg_amd/csrc/estimates_plan.hpp). */
int rpvg_hip_estimates_table_build(rpvg_hip_ctx * ctx, const rpvg_estimates_flat * estimates, uint32_t ploidy, rpvg_hip_estimates_table ** table_out);
int rpvg_hip_estimates_table_tpm(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table, double denominator);
int rpvg_hip_estimates_table_view(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table, rpvg_estimates_table_view * view_out);
void rpvg_hip_estimates_table_limits(rpvg_estimates_table_limits * limits_out);
void rpvg_hip_estimates_table_free(rpvg_hip_ctx * ctx, rpvg_hip_estimates_table * table);

/* ---- resident estimates (rpvg_table.h; rpvg_amd/csrc/estimates_gather.hip) -------------------------------------------------
 * The link between the nested calls and the table: their merged sets, still on the device, gathered into rpvg_estimates_flat with
 * on_device = 1 — what NestedPathAbundanceEstimator::unpackMergedSolutions / unpackMergedSetSolutions and FlatEstimates::add do on
 * the host, without an estimate crossing to it.
 *   rpvg_hip_subset_em_keep_device   a property of the context, read by rpvg_hip_nested_subset_em, rpvg_hip_nested_full_subset_em and
 *                                   rpvg_hip_nested_independent_subset_em: with keep != 0 a successful call hands its packed device
 *                                   block to its result instead of releasing it; rpvg_hip_subset_em_free returns it to the pool.
 *                                   THE KEPT BLOCK HAS THE SIZE OF THE CALL'S CAPACITIES (what it reserved for subsets, lists and
 *                                   columns), NOT OF THE RESULT.  With the default, 0, nothing changes in launches, copies,
 *                                   allocations or memory held.  The property is set, not counted: a caller that switches it on
 *                                   and off around a call (NestedPathAbundanceEstimator::estimateBatchResident does, on each lane's
 *                                   context) leaves it off, whatever it was before.
 *   rpvg_hip_subset_em_kept_bytes    the device memory a result's kept block holds (its capacity); 0 when none was kept.
 *   rpvg_hip_subset_em_part          the merged sets of a kept result as a part (on_device = 1, pointers into the kept block, valid
 *                                   until the result is freed); unit_cluster is left NULL for the caller to fill.
 *                                   RPVG_HIP_ERR_UNSUPPORTED when the block was not kept or the call did no merge on the device (a
 *                                   batch without path_group_id).
 *   rpvg_hip_flat_estimates_gather   the flat estimates of `batch` (K clusters) from num_parts parts.  Cluster c = unit_cluster[u] of
 *                                   a unit u gets that unit's sets in slot order, each with its posterior, its members in list order
 *                                   (repeats kept) and as many abundances; noise_count[c] = cluster_noise_count[u] when the unit has
 *                                   subsets, the batch's read count of the cluster otherwise; a cluster in no unit has no sets and
 *                                   its read count as noise.  abund_off[k] = member_off[set_off[k]].  Every double is copied: no
 *                                   floating-point operation is executed.  path_effective_length: [num_paths of the batch], host
 *                                   (copied) or device (eff_on_device != 0: borrowed, it must outlive the handle's use).
 *                                   RPVG_HIP_ERR_INVALID, the smallest offending (part, unit) named in last_error and the context
 *                                   left usable, for: a unit_cluster >= K; a cluster listed by two units (every unit that shares its
 *                                   cluster offends); subset_off or path_off that are not non-decreasing offsets from 0 to S and L;
 *                                   a set_count beyond the unit's slots; a set size outside 1 .. width (1 .. 2 at width 0); a member
 *                                   at or beyond its cluster's number of paths; width > 8; a batch without cluster totals
 *                                   (rpvg_hip_read_rows_to_batch).  One word for the first offender and the totals S and M come to
 *                                   the host.
 *   rpvg_hip_flat_estimates_view     the device view (on_device = 1; the sizes are host values; cluster_path_off is the batch's own
 *                                   array, so the batch must outlive the view's use).
 *   rpvg_hip_flat_estimates_get      host copies (on_device = 0): one packed copy to page-locked memory, valid until _free. */
int rpvg_hip_subset_em_keep_device(rpvg_hip_ctx * ctx, int32_t keep);
int rpvg_hip_subset_em_part(const rpvg_hip_subset_em * result, rpvg_estimates_part * part_out);
uint64_t rpvg_hip_subset_em_kept_bytes(const rpvg_hip_subset_em * result);
int rpvg_hip_flat_estimates_gather(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_estimates_part * parts, uint32_t num_parts,
                                   const double * path_effective_length, int32_t eff_on_device, rpvg_hip_flat_estimates ** estimates_out);
int rpvg_hip_flat_estimates_view(const rpvg_hip_flat_estimates * estimates, rpvg_estimates_flat * view_out);
int rpvg_hip_flat_estimates_get(rpvg_hip_ctx * ctx, rpvg_hip_flat_estimates * estimates, rpvg_estimates_flat * host_out);
void rpvg_hip_flat_estimates_free(rpvg_hip_ctx * ctx, rpvg_hip_flat_estimates * estimates);

/* ---- Gibbs samples table (rpvg_samples.h; rpvg_amd/csrc/gibbs_table.hip) ---------------------------------------------------
 *   rpvg_hip_gibbs_table_build           the table of `<prefix>_gibbs.txt.gz` for a batch, every value as rpvg_samples.h states it: per
 *                                       path its N sample columns, what ReadCountGibbsSamplesWriter::addSamples reads transposed
 *                                       through its per-path column vectors and fills with zeros (src/threaded_output_writer.cpp:114-214),
 *                                       the rows it prints (listed), and the per-sample noise totals of its `Unknown` row (the chain
 *                                       of `noise_counts.at(idx) +=` over the clusters, same lines).  Host arrays are copied as one
 *                                       block; device arrays (on_device = 1) are read where they lie.  One kernel validates behind the
 *                                       copy and before any table kernel: RPVG_HIP_ERR_INVALID for offsets that are not non-decreasing
 *                                       from 0 to the stated sizes, a block whose abundance samples are not samples x columns, path ids
 *                                       that do not ascend strictly or reach the cluster's number of paths, a cluster with more than N
 *                                       samples, or N = 0; last_error names the smallest offending cluster, or else the smallest
 *                                       offending block.
 *   rpvg_hip_gibbs_table_view            host copies of samples, listed and noise_counts, and the clusters per route.
 *   rpvg_hip_gibbs_table_rows            the sample rows of paths [first_path, first_path + num_paths) only (num_paths x N doubles to
 *                                       host memory): a writer streams a table it could not hold twice.
 *   rpvg_hip_gibbs_table_limits          the sizes at which a cluster changes its route (rpvg_amd/csrc/gibbs_table_plan.hpp).
 *   rpvg_hip_gibbs_read_counts_resident  rpvg_hip_gibbs_read_counts (src/path_abundance_estimator.cpp:116-212) without its two
 *                                       downloads: the same samples, left on the GPU in a handle with their two offset arrays.  A call
 *                                       with no problem or no sample gives an empty handle.
 *   rpvg_hip_gibbs_samples_get           the handle's samples to host memory, in the layout of rpvg_hip_gibbs_read_counts.
 *   rpvg_hip_gibbs_table_build_resident  the table from a handle: the problems of the sampler call are the blocks (problem p: block p
 *                                       of cluster problems->cluster[p], its col_path the block's path ids), which must come cluster
 *                                       by cluster — RPVG_HIP_ERR_INVALID names the first problem whose cluster is below its
 *                                       predecessor's.  cluster_path_off [K+1] and total_count [K] are host arrays. */
int rpvg_hip_gibbs_table_build(rpvg_hip_ctx * ctx, const rpvg_gibbs_flat * samples, rpvg_hip_gibbs_table ** table_out);
int rpvg_hip_gibbs_table_view(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table, rpvg_gibbs_table_view * view_out);
int rpvg_hip_gibbs_table_rows(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table, uint64_t first_path, uint64_t num_paths, double * rows_out);
void rpvg_hip_gibbs_table_limits(rpvg_gibbs_table_limits * limits_out);
void rpvg_hip_gibbs_table_free(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_table * table);
int rpvg_hip_gibbs_read_counts_resident(rpvg_hip_ctx * ctx, const rpvg_hip_batch * batch, const rpvg_hip_em_problems * problems,
                                        const double * init_abundances, const double * init_noise_count, const uint32_t * num_samples,
                                        const uint64_t * seeds, uint32_t gibbs_thin_its, double gamma, rpvg_hip_gibbs_samples ** samples_out);
int rpvg_hip_gibbs_samples_get(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_samples * samples, double * noise_samples, double * abundance_samples);
void rpvg_hip_gibbs_samples_free(rpvg_hip_ctx * ctx, rpvg_hip_gibbs_samples * samples);
int rpvg_hip_gibbs_table_build_resident(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_samples * samples, const rpvg_hip_em_problems * problems,
                                        uint32_t num_clusters, const uint64_t * cluster_path_off, const double * total_count,
                                        uint32_t num_gibbs_samples, rpvg_hip_gibbs_table ** table_out);

/* ---- table text (rpvg_text.h; rpvg_amd/csrc/table_text.hip) ------------------------------------------------------------------
 *   rpvg_hip_gibbs_table_text      the rows ReadCountGibbsSamplesWriter prints for a batch (src/threaded_output_writer.cpp:160-201),
 *                                 `name \t ClusterID (\t sample){N} \n` for the listed paths in path order, formatted on the GPU from
 *                                 the table's resident samples (a table built from arrays or from the sampler's handle alike).
 *   rpvg_hip_estimates_table_text  RPVG_TEXT_PER_PATH: the rows of AbundanceEstimatesWriter (src/threaded_output_writer.cpp:295-322),
 *                                 name, ClusterID, Length, EffectiveLength, abundance, member_tpm; set i of every cluster must be {i}
 *                                 (checked on the device: RPVG_HIP_ERR_INVALID names the first offending cluster).
 *                                 RPVG_TEXT_HAPLOTYPE: the rows of HaplotypeAbundanceEstimatesWriter (src/threaded_output_writer.cpp:358-411),
 *                                 name, ClusterID, Length, EffectiveLength, haplotype_prob, read_count, tpm.  The table must have its
 *                                 TPMs (rpvg_hip_estimates_table_tpm); `estimates` is the flat input the table was built from, host or device.
 *                                 Both refuse, before anything is queued, a precision outside 1 .. 17 and labels whose sizes are not
 *                                 the table's; a name_off that is not a non-decreasing sequence of offsets from 0 to num_name_bytes
 *                                 is refused by a kernel before any text kernel runs (last_error names the smallest offending path).
 *   rpvg_hip_estimates_set_text    the rows whose unit is a path group set (rpvg_text.h): RPVG_TEXT_JOINT, the rows of
 *                                 JointHaplotypeAbundanceEstimatesWriter (src/threaded_output_writer.cpp:434-546), from a table with its
 *                                 TPMs that was built for `ploidy`; RPVG_TEXT_POSTERIOR, the rows of JointHaplotypeEstimatesWriter
 *                                 (:233-280), which reads neither abundances nor TPMs.  A set is printed iff
 *                                 !(posterior < min_posterior).  Refused before anything is queued: a precision outside 1 .. 17, a
 *                                 ploidy outside 1 .. 8, a joint text from a table without TPMs or of another ploidy, labels whose
 *                                 sizes are not the table's.  Refused by a kernel before any text kernel runs: offsets that do not
 *                                 run from 0 to their totals, a set whose size is not in 1 .. ploidy, a member that is no path of its
 *                                 cluster and, for the joint kind, a cluster without one abundance per member (last_error names the
 *                                 smallest offending path, else the smallest offending cluster).  The handle is that of the other
 *                                 texts: in its view num_paths is the number of sets S and row_off has S + 1 entries.
 *   rpvg_hip_table_text_view       row_off and ONE copy of the whole text into page-locked memory of the library's pool.
 *   rpvg_hip_table_text_sizes      the view without the copy: the sizes and row_off, which the host holds since the build; bytes is NULL
 *                                 unless rpvg_hip_table_text_view has run.  For a caller that takes the text as BGZF members and never
 *                                 downloads it.
 *   rpvg_hip_table_text_get        bytes [byte_begin, byte_end) of the text to host memory: a writer streams a text of gigabytes in pieces.
 *   rpvg_hip_table_text_guards     test hook: the text lies in a device block between two runs of 64 pattern bytes; *intact_out says
 *                                 whether both still hold the pattern. */
int rpvg_hip_gibbs_table_text(rpvg_hip_ctx * ctx, const rpvg_hip_gibbs_table * table, const rpvg_table_labels * labels, int32_t precision,
                              rpvg_hip_table_text ** text_out);
int rpvg_hip_estimates_table_text(rpvg_hip_ctx * ctx, const rpvg_hip_estimates_table * table, const rpvg_estimates_flat * estimates,
                                  const rpvg_table_labels * labels, int32_t kind, int32_t precision, rpvg_hip_table_text ** text_out);
int rpvg_hip_estimates_set_text(rpvg_hip_ctx * ctx, const rpvg_hip_estimates_table * table, const rpvg_estimates_flat * estimates,
                                const rpvg_table_labels * labels, int32_t kind, uint32_t ploidy, double min_posterior, int32_t precision,
                                rpvg_hip_table_text ** text_out);
/*   rpvg_hip_rows_text             the --write-probs dump (rpvg_text.h; rpvg_amd/csrc/rows_text.hip) from host or device arrays: marker,
 *                                 path line and row lines of every cluster that has paths and rows.  labels: the names and
 *                                 path_length of the P paths (cluster_id is not read).  Refused before anything is queued: a
 *                                 prob_precision outside (0, 1) or one that asks for more than 17 digits, one rank-key array without
 *                                 the other, labels whose sizes are not the input's or without path_length, 2^31 - 1 or more lines
 *                                 (2 K + R) or cells (3 K + 3 P + 2 R + G + M).  Refused by a kernel before any text kernel runs:
 *                                 offsets that do not run from 0 to their totals and a path_idx that is not below its cluster's path
 *                                 count (last_error names the array and the smallest offending position).  The handle is that of the
 *                                 other texts: in its view num_paths is the number of lines and row_off has 2 K + R + 1 entries.
 *   rpvg_hip_read_rows_text        the same from resident rows (rpvg_hip_read_rows_build), read where they lie: nothing is downloaded
 *                                 and the rows stay usable.  labels: those of the rows' columns (the name groups of a collapsed
 *                                 build); path_effective_length [P] host; num_align_lists and cluster_index [K] host, both or NULL. */
int rpvg_hip_rows_text(rpvg_hip_ctx * ctx, const rpvg_rows_text_input * input, const rpvg_table_labels * labels, double prob_precision,
                       rpvg_hip_table_text ** text_out);
int rpvg_hip_read_rows_text(rpvg_hip_ctx * ctx, const rpvg_hip_read_rows * rows, const rpvg_table_labels * labels,
                            const double * path_effective_length, const uint64_t * num_align_lists, const uint64_t * cluster_index,
                            double prob_precision, rpvg_hip_table_text ** text_out);
int rpvg_hip_table_text_view(rpvg_hip_table_text * text, rpvg_table_text_view * view_out);
int rpvg_hip_table_text_sizes(rpvg_hip_table_text * text, rpvg_table_text_view * view_out);
int rpvg_hip_table_text_get(rpvg_hip_table_text * text, uint64_t byte_begin, uint64_t byte_end, char * dst);
int rpvg_hip_table_text_guards(rpvg_hip_table_text * text, int32_t * intact_out);
void rpvg_hip_table_text_free(rpvg_hip_table_text * text);
/*   rpvg_hip_table_text_bgzf       a resident text of any of the builders above as BGZF members (rpvg_text.h; rpvg_amd/csrc/text_deflate.hip),
 *                                 deflated on the GPU: only the compressed bytes are left to download.  The text stays as it is.
 *   rpvg_hip_bytes_bgzf            the same for any n bytes, host memory (on_device = 0) or device memory of the context's GPU, copied by
 *                                 the call.  Refused: n > 0 with a NULL pointer.  No bytes: no members, no error.
 *   rpvg_hip_text_bgzf_view        the sizes, member_off and ONE copy of the members into page-locked memory of the library's pool.
 *   rpvg_hip_text_bgzf_get         bytes [byte_begin, byte_end) of the members to host memory; a range outside them or reversed is refused.
 *   rpvg_hip_text_bgzf_guards      test hook: the members lie in a device block between two runs of 64 pattern bytes. */
int rpvg_hip_table_text_bgzf(rpvg_hip_table_text * text, rpvg_hip_text_bgzf ** bgzf_out);
int rpvg_hip_bytes_bgzf(rpvg_hip_ctx * ctx, const char * bytes, uint64_t n, int32_t on_device, rpvg_hip_text_bgzf ** bgzf_out);
int rpvg_hip_text_bgzf_view(rpvg_hip_text_bgzf * bgzf, rpvg_text_bgzf_view * view_out);
int rpvg_hip_text_bgzf_get(rpvg_hip_text_bgzf * bgzf, uint64_t byte_begin, uint64_t byte_end, char * dst);
int rpvg_hip_text_bgzf_guards(rpvg_hip_text_bgzf * bgzf, int32_t * intact_out);
void rpvg_hip_text_bgzf_free(rpvg_hip_text_bgzf * bgzf);
/*   rpvg_hip_text_rows             the --write-probs dump read back (rpvg_text.h; rpvg_amd/csrc/rows_parse.hip): n bytes of text in host
 *                                 memory (on_device = 0, copied by the call) or in device memory of the context's GPU, parsed on the
 *                                 GPU into resident rows and the dump's path side.  Refused before anything is queued: a
 *                                 prob_precision the writer would refuse, a text of 2^31 - 1 bytes or more, n > 0 with a NULL
 *                                 pointer.  Refused by the kernels: the texts rpvg_text.h lists (RPVG_HIP_ERR_INVALID; last_error
 *                                 names the 1-based number of the first offending line; the context stays usable).  No bytes: no
 *                                 clusters, no error.
 *   rpvg_hip_table_text_rows       the same for a resident text, parsed where it lies: nothing is downloaded.
 *   rpvg_hip_parsed_dump_rows      the resident rows the dump owns (freed with the dump, not with rpvg_hip_read_rows_free).
 *   rpvg_hip_parsed_dump_view      host copies of the path side: the block of the small arrays and the names, one wait.
 *   rpvg_hip_parsed_dump_labels    the names, lengths and ClusterIDs (k + 1) as labels with on_device = 1, valid until the dump is
 *                                 freed: parsed rows go back to text (rpvg_hip_read_rows_text) without a copy of the names. */
int rpvg_hip_text_rows(rpvg_hip_ctx * ctx, const char * bytes, uint64_t n, int32_t on_device, double prob_precision, rpvg_hip_parsed_dump ** dump_out);
int rpvg_hip_table_text_rows(rpvg_hip_table_text * text, double prob_precision, rpvg_hip_parsed_dump ** dump_out);
rpvg_hip_read_rows * rpvg_hip_parsed_dump_rows(rpvg_hip_parsed_dump * dump);
int rpvg_hip_parsed_dump_view(rpvg_hip_parsed_dump * dump, rpvg_parsed_dump_view * view_out);
int rpvg_hip_parsed_dump_labels(rpvg_hip_parsed_dump * dump, rpvg_table_labels * labels_out);
void rpvg_hip_parsed_dump_free(rpvg_hip_parsed_dump * dump);
/* counters of the two parse calls, kept apart from rpvg_hip_kernel_stats (whose layout stays); rpvg_hip_stats_reset zeroes them too */
typedef struct rpvg_hip_parse_stats {
    uint64_t calls_completed;        /* parses that returned RPVG_HIP_OK */
    uint64_t exact_tokens;           /* numbers whose rounding was decided by the exact multiword comparison: exact ties and decimals
                                        within 2^-73 relative of the middle of two doubles (rpvg_amd/csrc/number_parse.hpp); those of
                                        refused texts included */
} rpvg_hip_parse_stats;
int rpvg_hip_parse_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_parse_stats * stats_out);

/* ---- communicator (RCCL over xGMI; one process per GPU) --------------------- */
/* The reference is one process with OpenMP threads (src/main.cpp:829) and has no exchange step; the
 * only collectives of this engine are the per-iteration all-reduce of rpvg_hip_em_dense_sharded and
 * the sum of one double behind the TPM denominator (total_transcript_count, src/main.cpp:1029-1057)
 * when clusters are sharded over ranks.  RCCL is opened at run time (librccl.so.1) by the first of
 * these calls, so the rest of the library has no dependency on it.
 * rpvg_hip_comm_unique_id: rank 0 fills id (RPVG_HIP_COMM_ID_BYTES) and hands it to the other ranks by
 * any means (the harness broadcasts it with torch.distributed); every rank then calls
 * rpvg_hip_comm_init(ctx, id, world, rank) — collective over the ranks. */
#define RPVG_HIP_COMM_ID_BYTES 128
int rpvg_hip_comm_unique_id(uint8_t * id_out);
int rpvg_hip_comm_init(rpvg_hip_ctx * ctx, const uint8_t * id, int world_size, int rank);
int rpvg_hip_comm_destroy(rpvg_hip_ctx * ctx);
/* The same for the contexts of ONE process — one host thread per GPU instead of one process per GPU, the shape of
 * the reference's own parallelism (one process, `#pragma omp parallel for` over clusters, src/main.cpp:829):
 * context i becomes rank i of num_contexts; the contexts must sit on different GPUs. */
int rpvg_hip_comm_init_all(rpvg_hip_ctx * const * ctxs, int num_contexts);
/* In-place sum over ranks of n doubles in device memory (stream-ordered; synchronises before returning). */
int rpvg_hip_comm_allreduce_sum_f64(rpvg_hip_ctx * ctx, double * device_buf, uint64_t n);
/* The one collective of a run whose clusters are sharded over GPUs: the final gather of per-path abundances
 * (what the writers need in one place: src/main.cpp:1020-1083).  Collective over the ranks of the context's
 * communicator (every rank calls it, from its own host thread or process): rank r brings counts[r] host values,
 * every rank receives all of them in rank order (all_values: sum of counts; ncclAllGather over xGMI, ragged
 * lengths padded to the longest).  A context without a communicator is a world of one. */
int rpvg_hip_gather(rpvg_hip_ctx * ctx, const double * local_values, uint64_t local_count, const uint64_t * counts, double * all_values);

/* ---- synthetic workload (bench / tests only) ---------------------------- */
/* Fills a dense normalised R x C matrix (layout of rpvg_hip_em_dense) and unit
 * counts on the GPU from a counter-based generator: the "1M read pairs x 2k
 * paths single dense cluster" configuration. */
int rpvg_hip_synth_dense_cluster(rpvg_hip_ctx * ctx, uint64_t seed, uint64_t num_rows, uint32_t num_paths,
                                 double * device_matrix, uint64_t ld, double * device_counts);
/* Rows [row_begin, row_begin + num_rows) of the same cluster (a rank's shard of it). */
int rpvg_hip_synth_dense_rows(rpvg_hip_ctx * ctx, uint64_t seed, uint64_t row_begin, uint64_t num_rows, uint32_t num_paths,
                              double * device_matrix, uint64_t ld, double * device_counts);

/* The same cluster as a cluster batch resident on the GPU (one cluster, every row holding all num_paths paths) — what
 * the estimator classes take: BASELINE.json configs[1] behind `-i transcripts` without 40 GB of host arrays (SURVEY.md
 * section 8d S2 generates it on the device for the same reason).  Freed with rpvg_hip_batch_free. */
int rpvg_hip_synth_dense_cluster_batch(rpvg_hip_ctx * ctx, uint64_t seed, uint64_t num_rows, uint32_t num_paths,
                                       rpvg_hip_batch ** batch_out);

/* Test hook: the FP64 logarithm of the log-likelihood kernels (positive normal x) evaluated on the device,
 * with (use_table != 0) or without the LDS table — tests/test_hip_kernels.py measures its error. */
int rpvg_hip_debug_log(rpvg_hip_ctx * ctx, uint64_t n, const double * x, double * out, int32_t use_table);

/* ---- instrumentation ----------------------------------------------------- */
/* The EM kernels of rpvg_hip_em_solve (rpvg_amd/csrc/em_sparse.hip): one variant per size bin of the problems; each
 * carries its own device time (HIP events on the stream it is launched on), launches, problems, EM iterations and
 * algorithmic bytes (per iteration of a problem 12 B/entry + 20 B/row + 16 B/column, DESIGN.md section 3, docs/design/kernels-em.md). */
#define RPVG_HIP_EM_KERNELS 12
typedef struct rpvg_hip_em_kernel_stats {
    double ms;               /* sum over launches of the HIP-event span around the launch on its own stream */
    uint64_t launches;
    uint64_t problems;
    uint64_t iterations;     /* EM iterations of all problems of all launches */
    uint64_t max_iterations; /* sum over launches of the iteration count of the launch's slowest problem */
    double alg_bytes;
} rpvg_hip_em_kernel_stats;
/* "emRegisterKernel<1,16>", "emSparseKernel<64,true>", ...; NULL for an index outside [0, RPVG_HIP_EM_KERNELS) */
const char * rpvg_hip_em_kernel_name(int index);

/* Device time (HIP events on the stream the kernels are launched on) and launch count of the
 * kernels of each family since the last reset, plus the algorithmic bytes
 * they processed (DESIGN.md defines the per-launch figure). */
typedef struct rpvg_hip_kernel_stats {
    double em_sparse_ms;      uint64_t em_sparse_launches;   double em_sparse_alg_bytes;
    double em_dense_ms;       uint64_t em_dense_launches;    double em_dense_alg_bytes;
    double loglik_ms;         uint64_t loglik_launches;      double loglik_evals;   /* evals = FP64 log evaluations */
    double build_ms;          uint64_t build_launches;
    double h2d_ms;            double h2d_bytes;
    uint64_t em_iterations_total;
    /* diploid branch-and-bound (rpvg_hip_bounded_pair_posteriors): pairs of columns the searched matrices have
     * (G (G + 1) / 2 each), pairs among them that belong to matrices on the pair-table path (all of them evaluated),
     * and pairs kept — the reference evaluates the kept pairs plus the ones it prunes one by one. */
    double search_pairs_possible; double search_pairs_table; double search_pairs_kept;
    /* em_sparse_* split by kernel variant (em_sparse_ms is the span of a whole rpvg_hip_em_solve's kernels, whose bins
     * run side by side on several streams; the per-kernel spans overlap each other) */
    rpvg_hip_em_kernel_stats em_kernel[RPVG_HIP_EM_KERNELS];
    double collapse_ms;       /* row collapse of the group matrices (row_collapse.hip), on the collapse stream */
    /* length of the union of all timed spans of this context (kernels and copies; a span runs from the first command of
     * a stage to its last on the stage's stream, so this is an upper bound of the time the GPU worked for the context) */
    double busy_ms;
    /* rpvg_hip_group_gibbs, rpvg_hip_group_gibbs_polyploid: the span from the sampler's first kernel to its last (chains, request bookkeeping, distributions AND the
     * conditionals, whose own spans are in loglik_ms: gibbs_ms - loglik_ms is what the chains and their bookkeeping take) */
    double gibbs_ms;
    /* pairTile2Kernel alone (round 6): its own HIP-event spans on the stream it runs on and its launches — the kernel the row-pair
     * evaluations of loglik_evals belong to on the diploid search's table path (loglik_ms also holds the kernels behind it, and the
     * spans of batches in flight overlap); timed by contexts that time every kernel family (RPVG_HIP_SPANS=2) */
    double search_tile_ms;    uint64_t search_tile_launches;
    /* calls of rpvg_hip_group_gibbs and rpvg_hip_group_gibbs_polyploid that returned their sets (RPVG_HIP_OK with at least one
     * problem): a call that gave up on the way (RPVG_HIP_ERR_UNSUPPORTED) has a span in gibbs_ms and no count here */
    uint64_t gibbs_calls_completed;
    /* rpvg_hip_gibbs_read_counts: problems that took the whole-GPU route (gibbs_grid.hip) and their Gibbs iterations
     * (num_samples x gibbs_thin_its each) */
    uint64_t gibbs_count_grid_problems;
    uint64_t gibbs_count_grid_iterations;
    /* rpvg_hip_min_path_cover_any: clusters that took the whole-GPU route (path_cover_grid.hip) and the paths their greedy rounds chose */
    uint64_t cover_grid_problems;
    uint64_t cover_grid_rounds;
    /* rpvg_hip_gibbs_table_text, rpvg_hip_estimates_table_text, rpvg_hip_estimates_set_text, rpvg_hip_rows_text, rpvg_hip_read_rows_text: cells whose rounding was decided by the exact multiword comparison
     * (exact ties and doubles within 2^-60 relative of one; rpvg_amd/csrc/number_text.hpp) */
    uint64_t text_exact_cells;
    /* rpvg_hip_nested_full_subset_em: calls that returned RPVG_HIP_OK with at least one matrix, the sets they enumerated and the
     * sets they retained (posterior >= min_hap_prob) */
    uint64_t nested_full_calls;
    uint64_t nested_full_sets;
    uint64_t nested_full_retained;
} rpvg_hip_kernel_stats;

int rpvg_hip_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_kernel_stats * stats_out);
int rpvg_hip_stats_reset(rpvg_hip_ctx * ctx);
/* The timed spans behind the statistics since the last reset, as intervals in milliseconds on a clock shared by all
 * contexts of the GPU (so that a caller with several contexts on one GPU — the host lanes of rpvg_amd::HipEngine — can
 * take the union over them).  Writes at most `capacity` intervals (any array may be NULL) and the number there are. */
int rpvg_hip_stats_intervals(rpvg_hip_ctx * ctx, uint64_t capacity, double * start_ms, double * stop_ms, int32_t * family,
                             uint64_t * count_out);

#ifdef __cplusplus
}
#endif

#endif /* RPVG_HIP_H */
