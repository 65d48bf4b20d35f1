"""Plain-Python model of the --write-probs dump read back (include/rpvg_text.h, rpvg_amd/csrc/rows_parse_plan.hpp): split, float,
int and sorted.  parse(data) gives the flat arrays of rpvg_amd.table_text.PARSED_ARRAYS, or raises Refused(line, why) with the
1-based line and the reason of the first offending line (of several reasons on that line, the smallest).
tests/test_rows_parse_model.py pins it to hand-written texts, to readProbabilityClusters and to tests/rows_text_model.py."""
import math
import re

import numpy as np

from tests import rows_text_model as R

ORPHAN, MARKER, PATH_FIELD, SHORT_ROW, NO_COLON, INDEX, TOO_BIG, NOISE, OVERFLOW, TOO_LONG, MALFORMED, EMPTY_FIELD, UNSORTED_ROW = range(1, 14)
REASONS = ["",
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
           "a row of more than 1024 groups that are not in the order of the reader's sort"]
MAX_UNSORTED_GROUPS = 1024  # kMaxUnsortedGroups: a longer row must arrive in order
U32_MAX = 2 ** 32 - 1
_NUMBER = re.compile(rb"-?(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE][+-]?[0-9]+)?")


class Refused(Exception):
    def __init__(self, line, why):
        super().__init__(f"line {line}: {REASONS[why]}")
        self.line, self.why = line, why


def parse_double(token: bytes):
    """(value, 0) or (None, OVERFLOW | TOO_LONG | MALFORMED): Python's float() behind the grammar of number_parse.hpp"""
    if token in (b"inf", b"-inf", b"nan", b"-nan"):
        return float(token.decode()), 0
    m = _NUMBER.fullmatch(token)
    if not m:
        return None, MALFORMED
    digits = (m.group(1) or b"") + (m.group(2) or b"") + (m.group(3) or b"")
    if len(digits.lstrip(b"0")) > 19:
        return None, TOO_LONG
    value = float(token.decode())
    return (None, OVERFLOW) if math.isinf(value) else (value, 0)


def parse_u64(token: bytes):
    """(value, 0) or (None, TOO_LONG | MALFORMED): digits only, at most 19"""
    if not re.fullmatch(rb"[0-9]+", token):
        return None, MALFORMED
    return (None, TOO_LONG) if len(token) > 19 else (int(token), 0)


def is_marker(line: bytes) -> bool:
    return line == b"#" or line.startswith(b"# ")


def parse(data: bytes) -> dict:
    clusters = []  # dicts: rank (None or (lists, index)), paths [(name, length, eff)], rows [(count, noise, [(prob, [idx])])]
    refused = too_long = None
    before = None  # the non-empty line in front
    for number, line in enumerate(bytes(data).split(b"\n"), 1):
        if not line:
            continue
        why = set()
        marker_before, before = before is not None and is_marker(before), line
        if not is_marker(line) and not clusters:
            why.add(ORPHAN)
        else:
            if line.startswith(b" ") or line.endswith(b" ") or b"  " in line:
                why.add(EMPTY_FIELD)
            fields = [f for f in line.split(b" ") if f]
            open_end = line.endswith(b" ")  # the last field does not end the line
            if is_marker(line):
                rank = []
                for f in fields[1:3]:
                    value, bad = parse_u64(f)
                    if bad:
                        why.add(MARKER)
                    rank.append(value)
                if len(fields) > 3 or (len(fields) == 2 and not open_end):
                    why.add(MARKER)
                clusters.append(dict(rank=tuple(rank) if len(line) > 1 else None, paths=[], rows=[]))
            elif marker_before:
                for f in fields:
                    parts = f.rsplit(b",", 2)
                    if len(parts) < 3:
                        why.add(PATH_FIELD)
                        continue
                    length, bad = parse_u64(parts[1])
                    if not bad and length > U32_MAX:
                        bad = TOO_BIG
                    eff, bad_eff = parse_double(parts[2])
                    why |= {b for b in (bad, bad_eff) if b}
                    clusters[-1]["paths"].append((parts[0], length, eff))
            else:
                num_paths = len(clusters[-1]["paths"])
                shifted = line.startswith(b" ")  # every field counts as a group then (and the line is refused)
                if len(fields) == 1 and not open_end and not shifted:
                    why.add(SHORT_ROW)
                count, noise, groups = None, None, []
                for j, f in enumerate(fields):
                    if j == 0 and not shifted:
                        count, bad = parse_u64(f)
                        if not bad and count > U32_MAX:
                            bad = TOO_BIG
                        why |= {bad} if bad else set()
                    elif j == 1 and not shifted:
                        noise, bad = parse_double(f)
                        if not bad and not (noise > 0 and noise <= 1):
                            bad = NOISE
                        why |= {bad} if bad else set()
                    elif b":" not in f:
                        why.add(NO_COLON)
                    else:
                        head, tail = f.split(b":", 1)
                        prob, bad = parse_double(head)
                        why |= {bad} if bad else set()
                        members = []
                        for token in (tail.split(b",") if tail else []):
                            value, bad = parse_u64(token)
                            if not bad and value > U32_MAX:
                                bad = TOO_BIG
                            if not bad and value >= num_paths:
                                bad = INDEX
                            why |= {bad} if bad else set()
                            members.append(value)
                        groups.append((prob, members))
                if not why:
                    if len(groups) > MAX_UNSORTED_GROUPS and groups != sorted(groups) and too_long is None:
                        too_long = Refused(number, UNSORTED_ROW)  # found behind the fill: only a text without another offence gets here
                    groups = sorted(groups)
                clusters[-1]["rows"].append((count, noise, groups))
        if why and refused is None:
            refused = Refused(number, min(why))
    if refused is not None or too_long is not None:
        raise refused or too_long
    return flatten(clusters)


def flatten(clusters) -> dict:
    flat = R.flatten([dict(num_paths=len(c["paths"]), rows=c["rows"]) for c in clusters])
    names = [p[0] for c in clusters for p in c["paths"]]
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    name_off[1:] = np.cumsum([len(n) for n in names])
    flat.update(name_off=name_off, name_bytes=b"".join(names), path_length=np.array([p[1] for c in clusters for p in c["paths"]], dtype=np.uint32),
                path_effective_length=np.array([p[2] for c in clusters for p in c["paths"]], dtype=np.float64),
                has_rank_key=np.array([c["rank"] is not None for c in clusters], dtype=np.uint8),
                num_align_lists=np.array([c["rank"][0] if c["rank"] else 0 for c in clusters], dtype=np.uint64),
                cluster_index=np.array([c["rank"][1] if c["rank"] else 0 for c in clusters], dtype=np.uint64))
    return flat


def names_of(flat) -> list:
    off = [int(x) for x in flat["name_off"]]
    return [flat["name_bytes"][off[p]:off[p + 1]] for p in range(len(off) - 1)]


def print_back(flat, prob_precision=1e-8) -> bytes:
    """The text rows_text_model prints of parsed arrays: ranked markers iff any cluster has a rank key."""
    ranked = bool(np.asarray(flat["has_rank_key"]).any())
    return R.rows_text(flat, names_of(flat), flat["path_length"], flat["path_effective_length"], prob_precision,
                       flat["num_align_lists"] if ranked else None, flat["cluster_index"] if ranked else None)[0]


def same(got, want) -> list:
    """The names of the arrays of `want` that differ from those of `got` byte for byte (empty: equal)."""
    from rpvg_amd.table_text import PARSED_ARRAYS
    differ = []
    for name in PARSED_ARRAYS:
        a, b = got[name], want[name]
        if isinstance(b, bytes):
            if bytes(a) != b:
                differ.append(name)
        elif np.asarray(a).dtype != np.asarray(b).dtype or np.asarray(a).tobytes() != np.asarray(b).tobytes():
            differ.append(name)
    return differ
