/* rpvg_frag.h — the fragment-length model of a paired-end run, fitted and tabulated on the GPU (rpvg_amd/csrc/frag_length.hip).
 *
 * What it replaces in the reference (paths relative to the rpvg checkout):
 *   - FragmentLengthDist(frag_length_counts, skew_normal)            src/fragment_length_dist.cpp:60-285  (src/main.cpp:235)
 *   - FragmentLengthDist::logProb for every uint16_t fragment length src/fragment_length_dist.cpp:385-427
 *   - PathsIndex::effectivePathLength                                src/paths_index.cpp:190-229          (src/main.cpp:880)
 *     with Utils::truncated_skew_normal_expected_value               src/utils.hpp:229-247
 * The functions that take a rpvg_hip_ctx are declared in rpvg_hip.h.
 */
#ifndef RPVG_FRAG_H
#define RPVG_FRAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPVG_FRAG_LENGTH_MAX_COUNTS 65536 /* AlignmentPath::frag_length is uint16_t (src/alignment_path.hpp:35) */

typedef struct rpvg_frag_length_fit {
    double loc, scale, shape;  /* FragmentLengthDist::loc() / scale() / shape() */
    uint32_t max_length;       /* maxLength(): the number of counts */
    uint32_t sample_size;      /* sum of the counts (a uint32_t in the reference) */
    uint32_t iterations;       /* passes of the alternating alpha / mu search (at most 100; 0 for the normal fit) */
    uint32_t evaluations;      /* log-likelihood sums evaluated, one after the other */
    int32_t valid;             /* isValid(): loc >= 0 && scale > 0; 0 when fewer than two samples were counted */
} rpvg_frag_length_fit;

/* logProb(v) for v = 0 .. 65535 resident on the GPU; rpvg_row_params can point at it */
typedef struct rpvg_hip_frag_table rpvg_hip_frag_table;

#ifdef __cplusplus
}
#endif

#endif /* RPVG_FRAG_H */
