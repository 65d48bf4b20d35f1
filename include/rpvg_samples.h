/* rpvg_samples.h — the read-count Gibbs samples of a batch (-n) as the table of `<prefix>_gibbs.txt.gz`, built on the GPU
 * (rpvg_amd/csrc/gibbs_table.hip): the step between PathClusterEstimates::gibbs_read_count_samples (the gibbs_* arrays of
 * rpvg_estimates_view, include/rpvg_batch.h) and ReadCountGibbsSamplesWriter.
 *
 * What it replaces in the reference (paths relative to the rpvg checkout):
 *   - the per-path column vectors and the transposed, zero-filled read of ReadCountGibbsSamplesWriter::addSamples
 *                                                                          src/threaded_output_writer.cpp:114-214
 *   - the per-sample noise totals of its `Unknown` row                     src/threaded_output_writer.cpp:114-214 (noise_counts)
 * The functions that take a rpvg_hip_ctx are declared in rpvg_hip.h.
 *
 * K clusters; cluster k owns blocks [gibbs_off[k], gibbs_off[k+1]) of B blocks (one CountSamples each).  Block b has c_b
 * strictly ascending cluster-local path ids, n_b >= 0 samples: n_b noise samples and n_b * c_b abundance samples, sample-major.
 * N is -n.  g = cluster_path_off[k] + local is the batch-wide slot of a path.  base_i is the sum of n over the blocks of the
 * cluster before block i, S_k the sum over all of its blocks.  Every value is stated so that a host loop in the same order
 * gives the same bytes:
 *   samples[g * N + base_i + s]   s < n_i: the bits of abundance_samples[abund_off[b] + s * c_b + j] if the path is column j of
 *                                 block i, +0.0 if it is not; columns S_k .. N - 1 are +0.0.  A copy is a copy: -0.0 and
 *                                 subnormals arrive as they are.  Every cell of the P x N table is defined, the rows of paths in
 *                                 no block and of clusters without blocks included.
 *   listed[g]                     1 iff the path is a column of a block with n_b > 0: the rows the writer prints.  Blocks with
 *                                 n_b = 0 (dropped before the writer sees them) are legal input and contribute nothing.
 *   noise_counts[s]               from 0.0, over the clusters in ascending order: + noise_samples[noise_off[gibbs_off[k]] + s]
 *                                 if s < S_k, + total_count[k] otherwise (S_k = 0 for a cluster without blocks).  One chain per
 *                                 column in cluster order: the writer's `noise_counts.at(idx) += ...`.
 */
#ifndef RPVG_SAMPLES_H
#define RPVG_SAMPLES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The Gibbs samples of a batch in the flat form of rpvg_estimates_view's gibbs_* arrays, with the two arrays of the batch and
 * of the estimates the table needs beside them and the sizes the offsets must end at (the arrays may be device memory, which
 * the host cannot read).  At most 2^31 - 1 clusters, blocks, paths, path ids and noise samples, 2^40 abundance samples.
 * on_device = 0: host pointers, copied by the call.  on_device = 1: device pointers of the context's GPU (rpvg_hip_malloc),
 * read where they lie; they must stay valid until the call returns. */
typedef struct rpvg_gibbs_flat {
    uint32_t num_clusters;              /* K */
    uint64_t num_blocks;                /* B */
    uint64_t num_paths;                 /* P */
    uint32_t num_gibbs_samples;         /* N */
    uint64_t num_path_ids;              /* the total of gibbs_path  */
    uint64_t num_noise_samples;         /* the total of gibbs_noise */
    uint64_t num_abundance_samples;     /* the total of gibbs_abund */
    const uint64_t * gibbs_off;         /* [K+1] */
    const uint64_t * gibbs_path_off;    /* [B+1] */
    const uint32_t * gibbs_path;        /* cluster-local paths, strictly ascending inside a block */
    const uint64_t * gibbs_noise_off;   /* [B+1] */
    const double * gibbs_noise;
    const uint64_t * gibbs_abund_off;   /* [B+1] */
    const double * gibbs_abund;
    const uint64_t * cluster_path_off;  /* [K+1] rpvg_cluster_batch::cluster_path_off */
    const double * total_count;         /* [K]   rpvg_estimates_view::total_count */
    int32_t on_device;
} rpvg_gibbs_flat;

/* The routes of a cluster by its number of paths and the columns of its widest block (rpvg_amd/csrc/gibbs_table_plan.hpp holds
 * the rule). */
#define RPVG_GIBBS_ROUTE_RESIDENT 0 /* a (block, sample tile) staged in LDS, every path of the cluster behind it */
#define RPVG_GIBBS_ROUTE_GLOBAL 1   /* (block, sample tile, 64 paths) per wavefront, the samples read where they lie */
#define RPVG_GIBBS_ROUTES 2

/* Host copies of a table (valid until the table is freed). */
typedef struct rpvg_gibbs_table_view {
    uint32_t num_clusters;        /* K */
    uint64_t num_blocks;          /* B */
    uint64_t num_paths;           /* P */
    uint32_t num_gibbs_samples;   /* N */
    const double * samples;       /* [P * N] path-major */
    const uint8_t * listed;       /* [P] */
    const double * noise_counts;  /* [N] */
    const uint64_t * cluster_path_off; /* [K+1] the clusters' ranges of the P rows, as given to the build */
    uint32_t clusters_by_route[RPVG_GIBBS_ROUTES];
} rpvg_gibbs_table_view;

/* A cluster of at most resident_paths paths whose blocks have at most resident_columns columns each takes the resident route
 * (resident_lds_bytes of LDS per workgroup), every other cluster the global route.  sample_tile: the samples of a work item;
 * global_paths: the paths of a workgroup's item on the global route. */
typedef struct rpvg_gibbs_table_limits {
    uint32_t resident_paths;
    uint32_t resident_columns;
    uint32_t sample_tile;
    uint32_t global_paths;
    uint32_t resident_lds_bytes;
} rpvg_gibbs_table_limits;

typedef struct rpvg_hip_gibbs_table rpvg_hip_gibbs_table;
typedef struct rpvg_hip_gibbs_samples rpvg_hip_gibbs_samples; /* the samples of one sampler call, resident on the GPU */

#ifdef __cplusplus
}
#endif

#endif /* RPVG_SAMPLES_H */
