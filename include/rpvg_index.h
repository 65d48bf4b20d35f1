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
 * of the lists; the name-group collapsing of `-i transcripts --path-info` stays with the caller, who can build path_group
 * from the view; an index holds at most 2^32 - 2 lists, alignments and (alignment, path) entries.
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

#ifdef __cplusplus
}
#endif

#endif /* RPVG_INDEX_H */
