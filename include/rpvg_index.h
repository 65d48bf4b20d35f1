/* rpvg_index.h — the alignment-path index of a run, built on the GPU (rpvg_amd/csrc/align_index.hip): the step between the
 * alignment parser and row construction (include/rpvg_rows.h).
 *
 * What it replaces in the reference (paths relative to the rpvg checkout):
 *   - addAlignmentPathsBufferToIndexes                                src/main.cpp:200-237
 *     (fragment-length counts, normalisation of one-alignment lists, align_paths_index with multiplicities)
 *   - PathClusters from the lists (+ addNodeClusters' sets)            src/path_clusters.cpp:12-262
 *   - the caller's loop: a list's cluster from its anchor path         src/main.cpp:731-754
 *     clusters by descending (number of lists, cluster index)          src/main.cpp:811-827
 *     global path ids -> cluster-local indices                         src/main.cpp:846-857
 * The functions that take a rpvg_hip_ctx are declared in rpvg_hip.h.
 *
 * Not taken over: the consecutive-duplicate rule of addAlignmentPathsToBuffer (src/main.cpp:72-89) stays with the producer
 * of the lists; an index holds at most 2^31 - 1 lists, alignments and (alignment, path) entries.
 *
 * The path table (rpvg_path_table, rpvg_amd/csrc/path_table.hip) is the PathInfo of every global path, resident once per run
 * and read by kernels in the index's cluster order.  With it the device also forms
 *   - the path side of a batch made from rows (group ids, haplotype columns, read totals):  rpvg_hip_read_rows_to_batch_with_paths
 *   - the name groups of `-i transcripts --path-info` (group_name_index)                   src/main.cpp:853-887
 *     and the collapsed PathInfo of every group                                             src/main.cpp:909-951
 */
#ifndef RPVG_INDEX_H
#define RPVG_INDEX_H

#include <stdint.h>

#include "rpvg_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One chunk of the stream: what addAlignmentPathsToBuffer emits, one alignment-path list per fragment, flattened.  The
 * trailing noise entry of a list is carried as list_noise_score and not listed among the alignments (as in rpvg_rows.h).
 * Caller-owned host memory, read-only for the callee. */
typedef struct rpvg_fragment_lists {
    uint64_t num_lists;                 /* F */
    const uint8_t * list_is_simple;     /* [F] align_paths.front().is_simple */
    const uint8_t * list_min_mapq;      /* [F] align_paths.front().min_mapq */
    const int32_t * list_noise_score;   /* [F] align_paths.back().score_sum (<= 0) */
    const uint64_t * list_align_off;    /* [F+1] alignments of each list (>= 1 each); list_align_off[0] = 0 */
    const int32_t * align_score_sum;    /* [A] */
    const uint16_t * align_length;      /* [A] */
    const uint16_t * align_frag_length; /* [A] */
    const uint64_t * align_path_off;    /* [A+1] paths of each alignment (>= 1 each); align_path_off[0] = 0 */
    const uint32_t * align_path_id;     /* [E] global path ids, strictly ascending within an alignment */
} rpvg_fragment_lists;

typedef struct rpvg_index_params {
    uint32_t num_paths;             /* P: path ids are < num_paths */
    int32_t is_single_end;          /* -e: no fragment length is counted */
    uint32_t frag_length_min_mapq;  /* 30, src/main.cpp:42 */
    uint32_t max_frag_length;       /* pre_frag_length_dist.maxLength(): max_frag_length + 1 bins, at most 65 536 */
    uint16_t pre_frag_loc;          /* what `frag_length = pre_frag_length_dist.loc()` stores, src/main.cpp:223 */
    uint32_t hash_bits;             /* 0 (or >= 64): all 64 bits of the internal hash; 1 .. 63: only that many low bits — for
                                     * tests of the collision path; no result depends on it */
} rpvg_index_params;

typedef struct rpvg_index_info {
    uint64_t num_lists;            /* F: lists of the stream */
    uint64_t num_distinct;         /* D: distinct lists after normalisation */
    uint32_t num_clusters;         /* K */
    uint64_t num_collision_lists;  /* lists that differed from the first list with their hash: resolved by the exact slow path */
} rpvg_index_info;

/* Host copies of a finished index (valid until the index is freed).  `batch` holds the distinct lists in the layout of
 * rpvg_alignment_batch: clusters in rank order — descending (number of distinct lists, PathClusters index) —, the lists of
 * a cluster in ascending order of their first occurrence in the stream, read_count = multiplicity, align_path_idx
 * cluster-local.  Its path arrays (path_effective_length, path_source_count, path_group, cluster_group_off) are NULL:
 * the index does not know them. */
typedef struct rpvg_index_view {
    rpvg_alignment_batch batch;
    const uint32_t * rank_cluster;      /* [K] the PathClusters index (ascending smallest path id) of the cluster at every rank */
    const uint32_t * path_to_cluster;   /* [P] PathClusters index of every global path */
    const uint32_t * cluster_paths;     /* [P] global path ids, clusters in rank order (batch.cluster_path_off), ascending within one */
    const uint64_t * first_occurrence;  /* [D] index in the stream of the first list equal to this one */
} rpvg_index_view;

typedef struct rpvg_hip_align_index rpvg_hip_align_index;

/* The PathInfo of every path of a run by GLOBAL path id (P = rpvg_index_params::num_paths).  Caller-owned host memory,
 * read-only for the callee and free again when rpvg_hip_path_table_upload returns. */
typedef struct rpvg_path_table {
    uint32_t num_paths;               /* P */
    uint64_t num_sources;             /* S: length of source_id (0 without haplotype ids) */
    const uint32_t * group_id;        /* [P] PathInfo::group_id */
    const uint32_t * source_count;    /* [P] PathInfo::source_count */
    const uint64_t * source_off;      /* [P+1] non-decreasing, source_off[P] = S; NULL together with source_id: no haplotype ids */
    const uint32_t * source_id;       /* [S] PathInfo::source_ids, the lists of the paths back to back */
    const uint32_t * name_id;         /* [P] or NULL; equal ids = equal PathInfo::name.  Neither dense nor ordered. */
    const uint32_t * length;          /* [P] PathInfo::length */
    const double * effective_length;  /* [P] PathInfo::effective_length */
} rpvg_path_table;

typedef struct rpvg_hip_path_table rpvg_hip_path_table;

/* The routes of rpvg_hip_align_index_name_groups by the number of paths of a cluster: at most wave_paths one wavefront, at
 * most lds_paths one workgroup with a sort in LDS, beyond that global memory. */
typedef struct rpvg_name_groups_limits {
    uint32_t wave_paths;
    uint32_t lds_paths;
} rpvg_name_groups_limits;

/* Host copies of the name groups of a finished index (valid until the groups are freed).  Groups of a cluster are numbered by
 * the first appearance of their name along the cluster's paths (group_name_index.emplace(name, size), src/main.cpp:885); the
 * group arrays hold the collapsed PathInfo of src/main.cpp:909-951, clusters back to back in rank order. */
typedef struct rpvg_name_groups_view {
    uint32_t num_clusters;                 /* K */
    uint32_t num_paths;                    /* P */
    const uint32_t * path_group;           /* [P] cluster order: cluster-local group of every path */
    const uint64_t * cluster_group_off;    /* [K+1] */
    const uint32_t * group_first_path;     /* [G] GLOBAL id of the group's first member: its name and group_id come from it */
    const uint32_t * group_name_id;        /* [G] */
    const uint32_t * group_group_id;       /* [G] */
    const uint32_t * group_source_count;   /* [G] sum of the members' source counts */
    const uint32_t * group_length;         /* [G] round(sum(length * source_count) / double(sum(source_count))), half away from zero */
    const double * group_effective_length; /* [G] (sum in member order of effective_length * double(source_count)) / double(sum) */
} rpvg_name_groups_view;

typedef struct rpvg_hip_name_groups rpvg_hip_name_groups;

#ifdef __cplusplus
}
#endif

#endif /* RPVG_INDEX_H */
