/* rpvg_table.h — the estimates of a batch as the table rpvg reports, built on the GPU (rpvg_amd/csrc/estimates_table.hip): the
 * step between the estimators' result (rpvg_estimates_view, include/rpvg_batch.h) and the writers.
 *
 * What it replaces in the reference (paths relative to the rpvg checkout):
 *   - totalTranscriptCount, the TPM denominator                          src/main.cpp:1029-1057
 *   - the per-path accumulation of HaplotypeAbundanceEstimatesWriter     src/threaded_output_writer.cpp:346-432
 *     (haplotype probability with a homozygous set counted once, read count over the set memberships)
 *   - the per-member transcript counts and TPMs of the joint writer      src/threaded_output_writer.cpp:434-546
 *   - the noise totals of the `Unknown` rows                              src/threaded_output_writer.cpp:283-343, :434-546
 * The functions that take a rpvg_hip_ctx are declared in rpvg_hip.h.
 *
 * Every sum is a chain of plain IEEE additions in a stated order (below), so a table can be compared bit for bit with a host
 * loop that adds in the same order.  Write g = cluster_path_off[k] + local for the batch-wide slot of a path of cluster k.
 *   haplotype_prob[g]           from 0.0: + posteriors[i] for the sets i of the cluster in ascending order and the member positions j
 *                               of a set in ascending order, where the member is path g and (j == 0 || member[j] != member[j - 1])
 *                               (the writer's adjacent-duplicate rule, kept literally: an unsorted set {a, b, a} counts a twice)
 *   read_count[g]               the same walk, + the member's abundance at every position; 0 for a cluster without abundances
 *   transcript_count[g]         eff[g] > 0 ? read_count[g] / eff[g] : 0
 *   member_transcript_count[m]  eff > 0 ? abundance[m] / eff : 0; 0 for a cluster without abundances
 *   cluster_transcript_count[k] from 0.0: + abundance / eff over the cluster's members in (set, member) order, members with eff > 0 only
 *   total_transcript_count      from 0.0: + cluster_transcript_count[k] in ascending cluster order
 *   noise_count_total           from 0.0: + noise_count[k] in ascending cluster order
 *   noise_count_share_total     from 0.0: + noise_count[k] / ploidy in ascending cluster order
 *   tpm[g], member_tpm[m]       transcript count / denominator * 1e6: the division, then the multiplication
 */
#ifndef RPVG_TABLE_H
#define RPVG_TABLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The estimates of a batch of K clusters in the flat form of rpvg_estimates_view, with the two arrays of the batch the table
 * needs beside them and the sizes the offsets must end at (the arrays may be device memory, which the host cannot read).
 * The abundances of a cluster are one per member in (set, member) order (`transcripts`, `strains`, `haplotype-transcripts`)
 * or none (`haplotypes`).  At most 2^30 - 1 sets and 2^31 - 1 members, abundances and paths.
 * on_device = 0: host pointers, copied by the call.  on_device = 1: device pointers of the context's GPU (rpvg_hip_malloc),
 * read where they lie; they must stay valid until the call returns. */
typedef struct rpvg_estimates_flat {
    uint32_t num_clusters;                /* K */
    uint64_t num_sets;                    /* S */
    uint64_t num_members;                 /* M */
    uint64_t num_abundances;              /* A */
    uint64_t num_paths;                   /* P */
    const uint64_t * set_off;             /* [K+1] */
    const uint64_t * member_off;          /* [S+1] */
    const uint32_t * members;             /* [M]   cluster-local paths */
    const double * posteriors;            /* [S]   */
    const uint64_t * abund_off;           /* [K+1] */
    const double * abundances;            /* [A]   */
    const double * noise_count;           /* [K]   */
    const uint64_t * cluster_path_off;    /* [K+1] rpvg_cluster_batch::cluster_path_off */
    const double * path_effective_length; /* [P]   rpvg_cluster_batch::path_effective_length */
    int32_t on_device;
} rpvg_estimates_flat;

/* The routes of a cluster by its numbers of paths and members (rpvg_amd/csrc/estimates_plan.hpp holds the rule). */
#define RPVG_TABLE_ROUTE_WAVE 0   /* one wavefront, its lists in LDS */
#define RPVG_TABLE_ROUTE_LDS 1    /* one workgroup, its lists in LDS */
#define RPVG_TABLE_ROUTE_GLOBAL 2 /* global memory: a stable radix sort of the members by path */
#define RPVG_TABLE_ROUTES 3

/* Host copies of a table (valid until the table is freed or rpvg_hip_estimates_table_tpm is called on it). */
typedef struct rpvg_estimates_table_view {
    uint32_t num_clusters;                   /* K */
    uint64_t num_paths;                      /* P */
    uint64_t num_members;                    /* M */
    const double * haplotype_prob;           /* [P] */
    const double * read_count;               /* [P] */
    const double * transcript_count;         /* [P] */
    const double * tpm;                      /* [P] zeros until rpvg_hip_estimates_table_tpm */
    const double * member_transcript_count;  /* [M] */
    const double * member_tpm;               /* [M] zeros until rpvg_hip_estimates_table_tpm */
    const double * cluster_transcript_count; /* [K] */
    double total_transcript_count;
    double noise_count_total;
    double noise_count_share_total;
    double tpm_denominator;                  /* of the last rpvg_hip_estimates_table_tpm */
    int32_t has_tpm;
    uint32_t ploidy;                         /* of noise_count_share_total */
    uint32_t clusters_by_route[RPVG_TABLE_ROUTES];
} rpvg_estimates_table_view;

/* A cluster of at most wave_paths paths and wave_members members takes the wavefront route, one of at most lds_paths paths and
 * lds_members members the workgroup route (lds_bytes of LDS at the limits), every other cluster the global route. */
typedef struct rpvg_estimates_table_limits {
    uint32_t wave_paths;
    uint32_t wave_members;
    uint32_t lds_paths;
    uint32_t lds_members;
    uint32_t wave_lds_bytes;
    uint32_t lds_bytes;
} rpvg_estimates_table_limits;

typedef struct rpvg_hip_estimates_table rpvg_hip_estimates_table;

/* ---- the merged sets of some clusters as the nested calls leave them, and the flat form gathered from them on the GPU ----
 * (rpvg_amd/csrc/estimates_gather.hip; the rules are rpvg_amd/csrc/estimates_gather_plan.hpp)
 *
 * A part is what rpvg_hip_subset_em_view (width 0) or rpvg_hip_subset_em_sets_view / rpvg_hip_subset_em_independent_view (width =
 * their group size) describe: U units — the matrices of the collapsed calls, the clusters of the independent call — with S path
 * subsets and L list entries; the merged sets of unit u sit in the slots first + q, first = path_off[subset_off[u]], q <
 * set_count[u].
 *   width 0      the diploid form: set_first, set_second (UINT32_MAX: the set has one path), two abundances per slot
 *   width 1..8   set_size (1 .. width), set_member and set_abundance with `width` cells per slot
 * A batch's clusters are split over the lanes of an engine, so a batch is gathered from one or more parts; unit_cluster names
 * the batch cluster of every unit and is always host memory.  on_device = 1: every other array is device memory of the context's
 * GPU, read where it lies; on_device = 0: host memory, copied by the call. */
typedef struct rpvg_estimates_part {
    uint32_t num_units;                  /* U */
    uint64_t num_subsets;                /* S */
    uint64_t num_slots;                  /* L */
    uint32_t width;                      /* 0: diploid; 1..8 */
    const uint32_t * unit_cluster;       /* [U]   host memory */
    const uint64_t * subset_off;         /* [U+1] */
    const uint64_t * path_off;           /* [S+1] */
    const uint32_t * set_count;          /* [U]   */
    const double * cluster_noise_count;  /* [U]   */
    const double * set_posterior;        /* [L]   */
    const uint32_t * set_first;          /* [L]   width 0 */
    const uint32_t * set_second;         /* [L]   width 0 */
    const uint32_t * set_size;           /* [L]   width > 0 */
    const uint32_t * set_member;         /* [L x width] width > 0 */
    const double * set_abundance;        /* [L x 2] (width 0) or [L x width] */
    int32_t on_device;
} rpvg_estimates_part;

/* The flat estimates of a batch, resident on the GPU (rpvg_hip_flat_estimates_gather, rpvg_hip.h). */
typedef struct rpvg_hip_flat_estimates rpvg_hip_flat_estimates;

#ifdef __cplusplus
}
#endif

#endif /* RPVG_TABLE_H */
