// The rows of the two files whose row is a path group SET (table_text.hip; interface include/rpvg_text.h): the joint file of
// `-i haplotype-transcripts` (JointHaplotypeAbundanceEstimatesWriter) and the posterior file of `-i haplotypes`
// (JointHaplotypeEstimatesWriter), described by SetRows.  The second shape of row beside TextRows (table_text_plan.hpp), from which
// this takes Cell, cellText, flushPlan and the staging constants; the digits are number_text.hpp's.  Plain C++17 under the
// RPVG_PLAN_FN convention, so the kernels and the CPU check (tests/cpp/set_text_plan_check.cpp) walk the same code.
//
// For set s of cluster k, with members m in [member_off[s], member_off[s+1]) and n the number of those members (1 .. ploidy):
//
//   row s  =  ( name(cluster_path_off[k] + members[m]) '\t' ){n}  ( '.' '\t' ){ploidy - n}
//             cluster_id[k]  '\t' posteriors[s]
//             [ joint: ( '\t' abundances[abund_off[k] + m - member_off[set_off[k]]] '\t' member_tpm[m] ){n}  ( "\t0\t0" ){ploidy - n} ]  '\n'
//
// The cells of a row are numbered: the name slots 0 .. ploidy - 1 (names, then pads), then the number cells: ClusterID, the posterior
// and for the joint kind 2 * ploidy cells of pairs and pads.  In bytes the tab that follows a name slot is carried by the cell behind
// it: every cell but slot 0 begins with its tab, so that cellText serves the number cells as it is and the last of them carries the
// '\n'.  A set is printed iff !(posteriors[s] < min_posterior), the writers' test kept literally (a NaN is printed); a set that is
// not printed has no bytes.
#ifndef RPVG_HIP_SET_TEXT_PLAN_HPP
#define RPVG_HIP_SET_TEXT_PLAN_HPP

#include <cstdint>

#include "table_text_plan.hpp"

namespace rpvg_set_text {

using rpvg_table_text::Cell;
using rpvg_table_text::cellText;
using rpvg_table_text::kMaxCellBytes;
using rpvg_table_text::kStageBytes;

constexpr uint32_t kMaxPloidy = 8;
constexpr uint32_t kMaxNumberCells = 2 + 2 * kMaxPloidy;  // a wavefront's one step of number cells: a cell per lane
static_assert(kMaxNumberCells <= static_cast<uint32_t>(rpvg_table_text::kStepCells), "the number cells of a row are one step of a wavefront");
static_assert(kMaxNumberCells * kMaxCellBytes + 4 <= static_cast<uint32_t>(kStageBytes), "the number cells of a row fit the staging block behind a carried word");

struct SetRows {
    uint64_t num_sets;                 // S
    uint32_t num_clusters;             // K
    uint32_t ploidy;                   // 1 .. kMaxPloidy
    bool joint;                        // RPVG_TEXT_JOINT: the pairs behind the posterior
    const uint64_t * name_off;         // [P+1]
    const char * name_bytes;
    const uint64_t * cluster_path_off; // [K+1]
    const uint32_t * cluster_id;       // [K]
    const uint64_t * set_off;          // [K+1]
    const uint64_t * member_off;       // [S+1]
    const uint32_t * members;          // [M] cluster-local paths
    const double * posteriors;         // [S]
    const uint64_t * abund_off;        // [K+1]  joint only
    const double * abundances;         // [A]    joint only: one per member in every cluster
    const double * member_tpm;         // [M]    joint only
    double min_posterior;
    int precision;
    const uint64_t * pow10;            // rpvg_number_text::buildPow10Table
};

// NULL, or what is wrong with the numbers of a descriptor (the pointers are the builder's)
RPVG_PLAN_FN const char * descriptorBad(const SetRows & t) {
    if (t.precision < rpvg_number_text::kMinPrecision || t.precision > rpvg_number_text::kMaxPrecision) return "precision outside 1 .. 17";
    if (t.ploidy < 1 || t.ploidy > kMaxPloidy) return "ploidy outside 1 .. 8";
    if (t.num_clusters == 0 && t.num_sets != 0) return "sets without clusters";
    return nullptr;
}

RPVG_PLAN_FN uint32_t numberCells(const SetRows & t) { return 2u + (t.joint ? 2u * t.ploidy : 0u); }
RPVG_PLAN_FN uint32_t numCells(const SetRows & t) { return t.ploidy + numberCells(t); }
RPVG_PLAN_FN bool printed(const SetRows & t, const uint64_t s) { return !(t.posteriors[s] < t.min_posterior); }
RPVG_PLAN_FN uint64_t clusterOf(const SetRows & t, const uint64_t s) { return rpvg_hip_detail::lastAtMost(t.set_off, t.num_clusters, s); }

// where the parts of set s lie, read once per row
struct SetRow {
    uint64_t set, cluster;
    uint64_t first_member;  // member_off[s]
    uint32_t size;          // n
    uint64_t first_path;    // cluster_path_off[k]
    uint64_t first_abund;   // of member first_member (joint)
};

RPVG_PLAN_FN SetRow setRow(const SetRows & t, const uint64_t s) {
    SetRow row;
    row.set = s;
    row.cluster = clusterOf(t, s);
    row.first_member = t.member_off[s];
    row.size = static_cast<uint32_t>(t.member_off[s + 1] - row.first_member);
    row.first_path = t.cluster_path_off[row.cluster];
    row.first_abund = t.joint ? t.abund_off[row.cluster] + (row.first_member - t.member_off[t.set_off[row.cluster]]) : 0;
    return row;
}

// ---- the name slots: cells 0 .. ploidy - 1 ---------------------------------------------------------------------------------------
struct NameSlot {
    uint64_t at, length;  // name_bytes[at .. at + length)
    bool pad;             // '.' instead
    bool tab;             // a tab in front: every slot but the first
};

RPVG_PLAN_FN NameSlot nameSlot(const SetRows & t, const SetRow & row, const uint32_t j) {
    NameSlot slot;
    slot.pad = j >= row.size;
    slot.tab = j > 0;
    slot.at = slot.length = 0;
    if (!slot.pad) {
        const uint64_t path = row.first_path + t.members[row.first_member + j];
        slot.at = t.name_off[path];
        slot.length = t.name_off[path + 1] - slot.at;
    }
    return slot;
}

RPVG_PLAN_FN uint64_t slotBytes(const NameSlot & slot) { return (slot.tab ? 1u : 0u) + (slot.pad ? 1u : slot.length); }

// byte i < slotBytes(slot) of the slot's text
RPVG_PLAN_FN char slotByte(const SetRows & t, const NameSlot & slot, const uint64_t i) {
    if (slot.tab && i == 0) return '\t';
    return slot.pad ? '.' : t.name_bytes[slot.at + i - (slot.tab ? 1u : 0u)];
}

// ---- the number cells: cell ploidy + c, c < numberCells ---------------------------------------------------------------------------
// c = 0 the ClusterID, c = 1 the posterior, c = 2 + 2 * j the abundance and c = 3 + 2 * j the TPM of member j (a 0 behind the set's end).
// Read and decomposed once: a lane measures it and stores it from the same value.  The values are read, never recomputed.
RPVG_PLAN_FN Cell cellOf(const SetRows & t, const SetRow & row, const uint32_t c) {
    Cell cell;
    cell.u32 = 0;
    cell.last = c + 1 == numberCells(t);
    cell.decimal = rpvg_number_text::Decimal{0, 0, rpvg_number_text::kZero, false, false, false, false};
    const uint32_t j = c >= 2 ? (c - 2u) >> 1 : 0u;
    cell.is_u32 = c == 0 || (c >= 2 && j >= row.size);
    if (c == 0) cell.u32 = t.cluster_id[row.cluster];
    else if (c == 1) cell.decimal = rpvg_number_text::decompose(t.posteriors[row.set], t.precision, t.pow10);
    else if (!cell.is_u32) {
        const double value = ((c - 2u) & 1u) ? t.member_tpm[row.first_member + j] : t.abundances[row.first_abund + j];
        cell.decimal = rpvg_number_text::decompose(value, t.precision, t.pow10);
    }
    return cell;
}

// the bytes of set s, one cell behind the other (a lane of the measure kernel; the host line)
RPVG_PLAN_FN uint64_t rowBytes(const SetRows & t, const uint64_t s, uint64_t * exact_cells) {
    if (!printed(t, s)) return 0;
    const SetRow row = setRow(t, s);
    uint64_t bytes = 0;
    for (uint32_t j = 0; j < t.ploidy; ++j) bytes += slotBytes(nameSlot(t, row, j));
    const uint32_t cells = numberCells(t);
    for (uint32_t c = 0; c < cells; ++c) {
        const Cell cell = cellOf(t, row, c);
        bytes += cellText<false>(cell, t.precision, nullptr);
        *exact_cells += cell.decimal.exact ? 1u : 0u;
    }
    return bytes;
}

// set s written to out (rowBytes(s) bytes) by one thread
RPVG_PLAN_FN uint64_t rowWrite(const SetRows & t, const uint64_t s, char * out) {
    if (!printed(t, s)) return 0;
    const SetRow row = setRow(t, s);
    uint64_t at = 0;
    for (uint32_t j = 0; j < t.ploidy; ++j) {
        const NameSlot slot = nameSlot(t, row, j);
        const uint64_t bytes = slotBytes(slot);
        for (uint64_t i = 0; i < bytes; ++i) out[at + i] = slotByte(t, slot, i);
        at += bytes;
    }
    const uint32_t cells = numberCells(t);
    for (uint32_t c = 0; c < cells; ++c) at += cellText<true>(cellOf(t, row, c), t.precision, out + at);
    return at;
}

// ---- a wavefront's walk along a row (the write kernel) ------------------------------------------------------------------------------
// The name slots are appended to the staging block one behind the other, 64 bytes of a slot per pass of the lanes; the block leaves
// (flushPlan, not the row's end) whenever it is full, so a name of any length is as many steps as it needs, each of the up to
// `ploidy` names of a row.  Then the number cells join in one step, a cell per lane, behind a flush if they might not fit.
//   pieceOf: how much of a slot's remaining bytes fits the block now (0: flush first)
RPVG_PLAN_FN uint32_t pieceOf(const uint64_t remaining, const uint32_t hi) {
    const uint32_t room = static_cast<uint32_t>(kStageBytes) - hi;
    return remaining < room ? static_cast<uint32_t>(remaining) : room;
}
RPVG_PLAN_FN bool numbersNeedFlush(const SetRows & t, const uint32_t hi) { return hi + numberCells(t) * kMaxCellBytes > static_cast<uint32_t>(kStageBytes); }

}  // namespace rpvg_set_text

#endif
