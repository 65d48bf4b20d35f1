// What the kernels of rows_parse.hip compute per byte of a --write-probs dump, in plain C++17 under the RPVG_PLAN_FN convention, so
// that the CPU runs the same bodies over serial scans and the kernels are loops around them: rpvg_amd_rows_parse_plan of
// rpvg_amd/host/io/parse_capi.cpp, which tests/test_rows_parse_model.py holds to the plain-Python model, refusals included, and
// tests/cpp/rows_parse_plan_check.cpp under the sanitizers, every array at its exact size.  The grammar is the file of
// rows_text.hip (include/rpvg_text.h); the reader it replaces is readProbabilityClusters (rpvg_amd/host/io/cluster_io.cpp:135-251).
//
// Every decision is a function of the text and of four inclusive max-scans over its bytes, each "position + 1 of the last ... at or
// before byte i" (0: none): the start of a non-empty line, the start of a field (a maximal run without ' ' and '\n'), a ':' and a
// ','.  Nobody walks a line: a byte finds its line's start, its field's start, the field in front of it and the separators
// behind it with a constant number of loads.
//   line kinds   a line is a marker iff it is "#" or starts with "# "; the first non-empty line behind a marker is its path line
//                unless it is a marker itself; every other line is a row.  The host reader's rule, kept literally.
//   counts       five flags per byte, summed exclusively: markers (at the line's first byte), path fields and groups (at the
//                field's first byte), rows (at the line's first byte), indices (at the token's LAST byte).  The sums are the output
//                positions; their totals are K, P, R, G, M.
//   fill         the thread of a token's last byte parses it (the first ':' of a group parses the probability in front of it) and
//                stores it at its position.  Every store's index is a sum of the flags above, so it is below the total the arrays
//                were sized by, whatever the text holds.
//   refusals     reported as (byte offset of the line's start, reason): the minimum is the first offending line and, of its
//                offences, the smallest reason (table_kit.hpp).  Stricter than the host reader: see kReasons and parity.md.
//   group order  the constructor's std::sort over pair<double, vector<uint32_t>> (rpvg_amd/host/read_path_probabilities.cpp:17-21):
//                lessGroup.  A group compares with the one in front of it; only a row with a descent is sorted (insertion, by
//                one thread: such rows do not come out of this project's writer, which prints sorted rows; above
//                kMaxUnsortedGroups groups such a row is refused).
#ifndef RPVG_HIP_ROWS_PARSE_PLAN_HPP
#define RPVG_HIP_ROWS_PARSE_PLAN_HPP

#include "number_parse.hpp"
#include "table_kit.hpp"

namespace rpvg_rows_parse {

// a row whose groups are out of order is sorted by one thread, by insertion: above this many groups such a row is refused by name
// (65 536 list comparisons in one lane at the most; a row in order has no limit)
constexpr uint64_t kMaxUnsortedGroups = 1024;
constexpr uint64_t kMaxTextBytes = 0x7ffffffeull;  // a text of fewer than 2^31 - 1 bytes: positions + 1 fit 32 bits with room to spare

enum Why {
    kWhyOrphan = 1,
    kWhyMarker = 2,
    kWhyPathField = 3,
    kWhyShortRow = 4,
    kWhyNoColon = 5,
    kWhyIndex = 6,
    kWhyTooBig = 7,
    kWhyNoise = 8,
    kWhyOverflow = 9,
    kWhyTooLong = 10,
    kWhyMalformed = 11,
    kWhyEmptyField = 12,
    kWhyUnsortedRow = 13,
    kWhyLast = 13
};

inline const char * reasonOf(const int why) {
    static const char * const kReasons[] = {"",
                                            "data before the first cluster marker",
                                            "a cluster marker that is neither \"#\" nor \"# <lists> <index>\" with two numbers of at most 19 digits",
                                            "a path field with fewer than two commas",
                                            "a row with fewer than two fields",
                                            "a probability group without ':'",
                                            "a path index at or beyond the cluster's path count",
                                            "an integer above 4294967295 where 32 bits are kept (read count, path length, path index)",
                                            "a noise probability outside (0, 1]",
                                            "a number that rounds to infinity",
                                            "a number of more than 19 significant digits",
                                            "a malformed number (empty, a sign other than '-', hex, bytes behind it, a second ':')",
                                            "an empty field (a space at the start or the end of a line, or two in a row)",
                                            "a row of more than 1024 groups that are not in the order of the reader's sort"};
    return why >= 0 && why <= kWhyLast ? kReasons[why] : "";
}

enum Kind { kMarker = 0, kPathLine = 1, kRow = 2 };

// the text and the four max-scans (position + 1, 0: none)
struct Scanned {
    const char * text;
    uint32_t n;
    const uint32_t * line_at;
    const uint32_t * field_at;
    const uint32_t * colon_at;
    const uint32_t * comma_at;
};

// the five exclusive sums [n + 1]
struct Counted {
    const uint32_t * markers;
    const uint32_t * paths;
    const uint32_t * rows;
    const uint32_t * groups;
    const uint32_t * indices;
};

// everything the fill stores; the arrays have the exact sizes of the totals
struct Parsed {
    uint64_t K, P, R, G, M;
    uint64_t * cluster_row_off;        // [K + 1]
    uint64_t * cluster_path_off;       // [K + 1]
    uint8_t * has_rank_key;            // [K]
    uint64_t * num_align_lists;        // [K]
    uint64_t * cluster_index;          // [K]
    uint32_t * cluster_id;             // [K]: k + 1, the ClusterID of the writers
    uint64_t * name_len;               // [P + 1]: the name's bytes, a trailing 0; summed in place into name_off
    uint32_t * name_src;               // [P]: where the name starts in the text
    uint32_t * path_length;            // [P]
    double * path_effective_length;    // [P]
    uint32_t * row_count;              // [R]
    double * row_noise;                // [R]
    uint64_t * row_grp_off;            // [R + 1]
    uint32_t * row_line;               // [R]: where the row's line starts in the text
    double * text_prob;                // [G] in the text's order
    uint64_t * text_idx_off;           // [G + 1]
    uint32_t * text_idx;               // [M]
    const uint64_t * pow10;
};

RPVG_PLAN_FN bool isDelim(const char c) { return c == ' ' || c == '\n'; }

RPVG_PLAN_FN bool lineStartsAt(const char * __restrict__ t, const uint32_t i) { return t[i] != '\n' && (i == 0 || t[i - 1] == '\n'); }
RPVG_PLAN_FN bool fieldStartsAt(const char * __restrict__ t, const uint32_t i) { return !isDelim(t[i]) && (i == 0 || isDelim(t[i - 1])); }
RPVG_PLAN_FN bool markerAt(const char * __restrict__ t, const uint32_t n, const uint32_t s) {
    return t[s] == '#' && (s + 1 == n || t[s + 1] == '\n' || t[s + 1] == ' ');
}

// stage 1: the inputs of the four max-scans
RPVG_PLAN_FN void rawFlags(const char * __restrict__ t, const uint32_t i, uint32_t * line, uint32_t * field, uint32_t * colon, uint32_t * comma) {
    line[i] = lineStartsAt(t, i) ? i + 1 : 0;
    field[i] = fieldStartsAt(t, i) ? i + 1 : 0;
    colon[i] = t[i] == ':' ? i + 1 : 0;
    comma[i] = t[i] == ',' ? i + 1 : 0;
}

// the kind of the non-empty line that starts at s
RPVG_PLAN_FN int kindOfLine(const Scanned & x, const uint32_t s) {
    if (markerAt(x.text, x.n, s)) return kMarker;
    const uint32_t before = s ? x.line_at[s - 1] : 0;  // the non-empty line in front
    return before && markerAt(x.text, x.n, before - 1) ? kPathLine : kRow;
}

// the index of the field that starts at f in the line that starts at s: 0, 1, 2, or 3 for anything later (and for a field behind
// a space at the line's start, which is refused)
RPVG_PLAN_FN int fieldIndex(const Scanned & x, const uint32_t s, const uint32_t f) {
    if (f == s) return 0;
    const uint32_t p1 = x.field_at[f - 1];  // f > s >= 0
    if (p1 < s + 1) return 3;
    if (p1 - 1 == s) return 1;
    const uint32_t p2 = x.field_at[p1 - 2];  // p1 - 1 > s >= 0
    if (p2 < s + 1) return 3;
    return p2 - 1 == s ? 2 : 3;
}

// whether byte i, a byte of a group field that starts at f, lies behind the field's first ':'
RPVG_PLAN_FN bool behindColon(const Scanned & x, const uint32_t f, const uint32_t i) { return i > f && x.colon_at[i - 1] >= f + 1; }

RPVG_PLAN_FN bool endsToken(const Scanned & x, const uint32_t i) { return i + 1 == x.n || isDelim(x.text[i + 1]) || x.text[i + 1] == ','; }

// byte i is the last byte of a path index
RPVG_PLAN_FN bool indexEndsAt(const Scanned & x, const uint32_t s, const uint32_t f, const uint32_t i) {
    return x.text[i] != ',' && behindColon(x, f, i) && endsToken(x, i) && fieldIndex(x, s, f) >= 2;
}

// stage 2: the inputs of the five sums
RPVG_PLAN_FN void countFlags(const Scanned & x, const uint32_t i, uint32_t * markers, uint32_t * paths, uint32_t * rows, uint32_t * groups, uint32_t * indices) {
    uint32_t is_marker = 0, is_path = 0, is_row = 0, is_group = 0, is_index = 0;
    const char c = x.text[i];
    if (!isDelim(c)) {
        const uint32_t s = x.line_at[i] - 1, f = x.field_at[i] - 1;
        const int kind = kindOfLine(x, s);
        if (i == s) {
            is_marker = kind == kMarker;
            is_row = kind == kRow;
        }
        if (i == f) {
            is_path = kind == kPathLine;
            is_group = kind == kRow && fieldIndex(x, s, f) >= 2;
        }
        is_index = kind == kRow && indexEndsAt(x, s, f, i);
    }
    markers[i] = is_marker;
    paths[i] = is_path;
    rows[i] = is_row;
    groups[i] = is_group;
    indices[i] = is_index;
}

RPVG_PLAN_FN int whyOfStatus(const int status) {
    return status == rpvg_number_parse::kOverflow ? kWhyOverflow : (status == rpvg_number_parse::kTooLong ? kWhyTooLong : kWhyMalformed);
}

// stage 3: the offsets of the clusters, which the fill reads (byte 0 stores the ends of the offset arrays)
RPVG_PLAN_FN void markerByte(const Scanned & x, const Counted & c, const Parsed & o, const uint32_t i) {
    if (i == 0) {
        o.cluster_row_off[o.K] = o.R;
        o.cluster_path_off[o.K] = o.P;
        o.row_grp_off[o.R] = o.G;
        o.text_idx_off[o.G] = o.M;
        o.name_len[o.P] = 0;
    }
    if (!lineStartsAt(x.text, i) || !markerAt(x.text, x.n, i)) return;
    const uint32_t k = c.markers[i];
    o.cluster_row_off[k] = c.rows[i];
    o.cluster_path_off[k] = c.paths[i];
    o.has_rank_key[k] = i + 1 < x.n && x.text[i + 1] == ' ';
    o.num_align_lists[k] = 0;
    o.cluster_index[k] = 0;
    o.cluster_id[k] = k + 1;
}

// stage 4: Sink has report(line_start, why), nameBytes(n) and exactToken()
template <typename Sink>
RPVG_PLAN_FN void fillByte(const Scanned & x, const Counted & c, const Parsed & o, const uint32_t i, Sink & sink) {
    namespace np = rpvg_number_parse;
    const char * const t = x.text;
    const char ch = t[i];
    if (ch == '\n') return;
    const uint32_t s = x.line_at[i] - 1;
    const int kind = kindOfLine(x, s);
    if (kind != kMarker && c.markers[s] == 0) {
        if (i == s) sink.report(s, kWhyOrphan);
        return;
    }
    if (ch == ' ') {
        if (i == s || i + 1 == x.n || isDelim(t[i + 1])) sink.report(s, kWhyEmptyField);
        return;
    }
    const uint32_t k = c.markers[s] - (kind == kMarker ? 0u : 1u);
    const uint32_t f = x.field_at[i] - 1;
    const int fi = fieldIndex(x, s, f);
    const bool field_ends = i + 1 == x.n || isDelim(t[i + 1]);
    const bool line_ends = i + 1 == x.n || t[i + 1] == '\n';

    // what this byte parses, if anything: one integer and one double at the most
    enum Target { kNone, kLists, kIndex, kPathLength, kReadCount, kPathIdx, kEffLength, kNoise, kProb };
    int int_target = kNone, dbl_target = kNone;
    uint32_t int_begin = 0, int_end = 0, dbl_begin = 0, dbl_end = 0;
    uint64_t at = 0, dbl_at = 0;

    if (kind == kMarker) {
        if (field_ends) {
            if (fi == 1 || fi == 2) {
                int_target = fi == 1 ? kLists : kIndex;
                int_begin = f;
                int_end = i + 1;
                at = k;
            }
            if (fi >= 3 || (fi == 1 && line_ends)) sink.report(s, kWhyMarker);
        }
    } else if (kind == kPathLine) {
        if (field_ends) {
            const uint32_t c2 = x.comma_at[i];
            const uint32_t c1 = c2 >= f + 1 && c2 >= 2 ? x.comma_at[c2 - 2] : 0;
            if (c2 < f + 1 || c1 < f + 1) {
                sink.report(s, kWhyPathField);
            } else {
                const uint64_t p = c.paths[f];
                o.name_src[p] = f;
                o.name_len[p] = c1 - 1 - f;
                sink.nameBytes(c1 - 1 - f);
                int_target = kPathLength;
                int_begin = c1;
                int_end = c2 - 1;
                at = p;
                dbl_target = kEffLength;
                dbl_begin = c2;
                dbl_end = i + 1;
                dbl_at = p;
            }
        }
    } else {
        const uint64_t r = c.rows[s];
        if (i == s) {
            o.row_grp_off[r] = c.groups[s];
            o.row_line[r] = s;
        }
        if (line_ends && fi == 0) sink.report(s, kWhyShortRow);
        if (fi == 0 && field_ends) {
            int_target = kReadCount;
            int_begin = f;
            int_end = i + 1;
            at = r;
        } else if (fi == 1 && field_ends) {
            dbl_target = kNoise;
            dbl_begin = f;
            dbl_end = i + 1;
            dbl_at = r;
        } else if (fi >= 2) {
            const uint64_t g = c.groups[f];
            if (field_ends) {
                o.text_idx_off[g] = c.indices[f];
                if (x.colon_at[i] < f + 1) sink.report(s, kWhyNoColon);
            }
            const bool behind = behindColon(x, f, i);
            if (ch == ':' && !behind) {
                dbl_target = kProb;
                dbl_begin = f;
                dbl_end = i;
                dbl_at = g;
            }
            if (ch == ':' && behind) sink.report(s, kWhyMalformed);                                           // a second ':'
            // an empty index; a ':' that ends its field is a group without indices, which the host reader takes and the writer prints
            if (ch == ',' && behind && endsToken(x, i)) sink.report(s, kWhyMalformed);
            if (ch == ':' && !behind && !field_ends && endsToken(x, i)) sink.report(s, kWhyMalformed);
            if (ch != ',' && behind && endsToken(x, i)) {
                const uint32_t colon = x.colon_at[i - 1], comma = x.comma_at[i - 1];
                int_target = kPathIdx;
                int_begin = colon > comma ? colon : comma;
                int_end = i + 1;
                at = c.indices[i];
            }
        }
    }

    if (int_target != kNone) {
        uint64_t v = 0;
        const int status = np::parseU64(t + int_begin, int_end - int_begin, &v);
        if (status != np::kOk) {
            sink.report(s, int_target == kLists || int_target == kIndex ? kWhyMarker : whyOfStatus(status));
        } else if (int_target == kLists) {
            o.num_align_lists[at] = v;
        } else if (int_target == kIndex) {
            o.cluster_index[at] = v;
        } else if (v > 0xffffffffull) {
            sink.report(s, kWhyTooBig);
        } else if (int_target == kPathLength) {
            o.path_length[at] = static_cast<uint32_t>(v);
        } else if (int_target == kReadCount) {
            o.row_count[at] = static_cast<uint32_t>(v);
        } else {
            if (v >= c.paths[s] - o.cluster_path_off[k]) sink.report(s, kWhyIndex);  // (the paths of cluster k: every path field in front of this row, less those of the clusters in front)
            o.text_idx[at] = static_cast<uint32_t>(v);
        }
    }
    if (dbl_target != kNone) {
        const np::Parsed d = np::parseDouble(t + dbl_begin, dbl_end - dbl_begin, o.pow10);
        if (d.exact) sink.exactToken();
        if (d.status != np::kOk) {
            sink.report(s, whyOfStatus(d.status));
        } else if (dbl_target == kEffLength) {
            o.path_effective_length[dbl_at] = d.value;
        } else if (dbl_target == kNoise) {
            if (!(d.value > 0 && d.value <= 1)) sink.report(s, kWhyNoise);
            o.row_noise[dbl_at] = d.value;
        } else {
            o.text_prob[dbl_at] = d.value;
        }
    }
}

// ---- the order of a row's groups ------------------------------------------------------------------------------------------------

struct Groups {
    uint64_t R, G, M;
    const uint64_t * row_grp_off;   // [R + 1]
    const double * text_prob;       // [G]
    const uint64_t * text_idx_off;  // [G + 1]
    const uint32_t * text_idx;      // [M]
    uint32_t * row_unsorted;        // [R], zeroed
    uint64_t * source;              // [G]: the group of the text that becomes group g
    uint64_t * grp_idx_off;         // [G + 1]: of the groups in their final order
};

// operator< of pair<double, vector<uint32_t>>
RPVG_PLAN_FN bool lessGroup(const Groups & q, const uint64_t a, const uint64_t b) {
    const double pa = q.text_prob[a], pb = q.text_prob[b];
    if (pa < pb) return true;
    if (pb < pa) return false;
    const uint64_t a0 = q.text_idx_off[a], a1 = q.text_idx_off[a + 1], b0 = q.text_idx_off[b], b1 = q.text_idx_off[b + 1];
    const uint64_t na = a1 - a0, nb = b1 - b0, common = na < nb ? na : nb;
    for (uint64_t j = 0; j < common; ++j) {
        const uint32_t ia = q.text_idx[a0 + j], ib = q.text_idx[b0 + j];
        if (ia != ib) return ia < ib;
    }
    return na < nb;
}

// group g against the one in front of it: the identity, and the row's mark when g belongs in front
template <typename Mark>
RPVG_PLAN_FN void orderGroup(const Groups & q, const uint64_t g, Mark mark) {
    q.source[g] = g;
    q.grp_idx_off[g] = q.text_idx_off[g];
    if (g == 0) q.grp_idx_off[q.G] = q.M;
    const uint64_t r = rpvg_hip_detail::lastAtMost(q.row_grp_off, q.R, g);
    if (q.row_grp_off[r] < g && lessGroup(q, g, g - 1)) mark(r);
}

// a marked row: insertion sort of its groups (stable), then the offsets of their indices; refuse(r) for one too long for that
template <typename Refuse>
RPVG_PLAN_FN void sortRow(const Groups & q, const uint64_t r, Refuse refuse) {
    if (!q.row_unsorted[r]) return;
    const uint64_t begin = q.row_grp_off[r], end = q.row_grp_off[r + 1];
    if (end - begin > kMaxUnsortedGroups) {
        refuse(r);
        return;
    }
    for (uint64_t j = begin + 1; j < end; ++j) {
        const uint64_t moved = q.source[j];
        uint64_t at = j;
        while (at > begin && lessGroup(q, moved, q.source[at - 1])) {
            q.source[at] = q.source[at - 1];
            --at;
        }
        q.source[at] = moved;
    }
    uint64_t off = q.text_idx_off[begin];
    for (uint64_t j = begin; j < end; ++j) {
        q.grp_idx_off[j] = off;
        off += q.text_idx_off[q.source[j] + 1] - q.text_idx_off[q.source[j]];
    }
}

// position j of the final arrays: probability j (j < G) and index j (j < M)
RPVG_PLAN_FN void placeEntry(const Groups & q, const uint64_t j, double * grp_prob, uint32_t * path_idx) {
    if (j < q.G) grp_prob[j] = q.text_prob[q.source[j]];
    if (j < q.M) {
        const uint64_t g = rpvg_hip_detail::lastAtMost(q.grp_idx_off, q.G, j);
        path_idx[j] = q.text_idx[q.text_idx_off[q.source[g]] + (j - q.grp_idx_off[g])];
    }
}

// byte b of the names: name_off [P + 1]
RPVG_PLAN_FN char nameByte(const char * __restrict__ text, const uint64_t * __restrict__ name_off, const uint32_t * __restrict__ name_src, const uint64_t P, const uint64_t b) {
    const uint64_t p = rpvg_hip_detail::lastAtMost(name_off, P, b);
    return text[name_src[p] + (b - name_off[p])];
}

}  // namespace rpvg_rows_parse

#endif
