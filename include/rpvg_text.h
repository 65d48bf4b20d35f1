/* rpvg_text.h — the rows of a result file as text, formatted on the GPU from a resident table (rpvg_amd/csrc/table_text.hip): the
 * last step of the output side, behind the estimates table (rpvg_table.h) and the Gibbs samples table (rpvg_samples.h).
 *
 * What it replaces in the reference (paths relative to the rpvg checkout):
 *   - the stream insertions of the writers' rows at setprecision(8), i.e. "%.8g"   src/threaded_output_writer.cpp:6
 *   - the rows of ReadCountGibbsSamplesWriter                                      src/threaded_output_writer.cpp:160-201
 *   - the rows of AbundanceEstimatesWriter                                         src/threaded_output_writer.cpp:295-322
 *   - the rows of HaplotypeAbundanceEstimatesWriter                                src/threaded_output_writer.cpp:358-411
 * The header row and the `Unknown` row stay with the host writers: they depend on the writer's running noise totals and on the
 * unaligned read count.  The functions that take a rpvg_hip_ctx are declared in rpvg_hip.h.
 *
 * A double is written as glibc's printf("%.*g", precision, v) writes it in round-to-nearest, byte for byte, for every bit pattern:
 * correctly rounded to `precision` significant digits (the exact binary value, ties to even), trailing zeros and a bare point
 * removed, fixed notation for a decimal exponent -4 <= X < precision after the rounding and exponent notation with a sign and at
 * least two digits otherwise, `0`, `-0`, `inf`, `-inf`, `nan` and — glibc's spelling for a NaN with the sign bit set, which the
 * host writers therefore produce — `-nan`.  precision is 1 .. 17.
 */
#ifndef RPVG_TEXT_H
#define RPVG_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* TableLabels of rpvg_amd/host/io/estimates_writers.hpp, flat: the name of path g is name_bytes[name_off[g] .. name_off[g + 1]).
 * on_device = 0: host pointers, copied by the call.  on_device = 1: device pointers of the context's GPU. */
typedef struct rpvg_table_labels {
    uint32_t num_clusters;              /* K */
    uint64_t num_paths;                 /* P */
    uint64_t num_name_bytes;
    const uint64_t * name_off;          /* [P+1] non-decreasing from 0 to num_name_bytes */
    const char * name_bytes;
    const uint32_t * path_length;       /* [P]; may be NULL for the Gibbs file */
    const uint32_t * cluster_id;        /* [K] */
    int32_t on_device;
} rpvg_table_labels;

#define RPVG_TEXT_PER_PATH 0  /* name, ClusterID, Length, EffectiveLength, abundance, member_tpm  (AbundanceEstimatesWriter) */
#define RPVG_TEXT_HAPLOTYPE 1 /* name, ClusterID, Length, EffectiveLength, haplotype_prob, read_count, tpm  (HaplotypeAbundanceEstimatesWriter) */

/* The rows of a set text (rpvg_hip_estimates_set_text): one per path group set s of cluster k, n = its number of members (1 .. ploidy),
 *   ( name(member) '\t' ){n} ( '.' '\t' ){ploidy - n}  ClusterID '\t' posterior  [ joint: ( '\t' abundance '\t' member_tpm ){n} ( "\t0\t0" ){ploidy - n} ]  '\n'
 * printed iff !(posterior < min_posterior): a posterior equal to min_posterior and a NaN posterior are printed. */
#define RPVG_TEXT_JOINT 2     /* JointHaplotypeAbundanceEstimatesWriter (src/threaded_output_writer.cpp:434-546): needs the table's TPMs and one abundance per member */
#define RPVG_TEXT_POSTERIOR 3 /* JointHaplotypeEstimatesWriter (src/threaded_output_writer.cpp:233-280): no pairs; needs neither abundances nor TPMs */

/* Host copies of a text (valid until the text is freed).  Row g lies in bytes [row_off[g], row_off[g + 1]); a path that is not
 * printed has an empty range.  In the view of a set text the rows are the sets: num_paths is the number of sets S, row_off has
 * S + 1 entries, and a set that is not printed has an empty range. */
typedef struct rpvg_table_text_view {
    uint64_t num_paths;
    uint64_t num_rows;                  /* printed */
    uint64_t num_bytes;
    const uint64_t * row_off;           /* [P+1] */
    const char * bytes;                 /* page-locked memory of the library's pool; NULL for an empty text */
} rpvg_table_text_view;

typedef struct rpvg_hip_table_text rpvg_hip_table_text;

#ifdef __cplusplus
}
#endif

#endif /* RPVG_TEXT_H */
