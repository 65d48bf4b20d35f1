"""Plain-Python model of the path table (include/rpvg_index.h, rpvg_amd/csrc/path_table.hip): dicts and loops over the output
of tests/align_index_model.py.

A table is a dict of per-GLOBAL-path lists: group_id, source_count, source_ids (a list of ids per path, or None for a table
without haplotype ids), name_id (or None), length, effective_length.

  - name_groups restates src/main.cpp:853-887: `group_name_index.emplace(name, group_name_index.size())` over the cluster's
    paths in ascending order, so the group of a path is the rank of the first appearance of its name;
  - collapsed_paths restates src/main.cpp:909-951: the first member of a group brings name and group_id, source counts and
    length * source_count add up, effective_length * source_count is added member by member in a double (a rounded product,
    then a rounded sum), and the two closing divisions, `round` being C's (half away from zero).  Unlike the reference, whose
    uint32 products wrap, the sums are exact integers and a result beyond 32 bits is an error (docs/design/parity.md item 12);
  - path_side permutes group ids and source-id lists into cluster order: what a host would hand to rpvg_hip_batch_upload.
"""
import math
from fractions import Fraction

import numpy as np

UINT32_MAX = 0xffffffff


class InvalidGroup(ValueError):
    def __init__(self, cluster, group, why):
        super().__init__(f"group {group} of cluster {cluster}: {why}")
        self.cluster, self.group = cluster, group


def c_round(x):
    """C's round(): to the nearest integer, halves away from zero (x >= 0 here)."""
    assert x >= 0
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f  # (x - floor(x) is exact in binary floating point)


def cluster_lists(index_arrays):
    """[[global path id ...] per cluster in rank order] from the arrays of align_index_model's result."""
    off = [int(x) for x in index_arrays["cluster_path_off"]]
    paths = [int(x) for x in index_arrays["cluster_paths"]]
    return [paths[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def name_groups(clusters, name_id):
    """clusters: [[global path id ...] ...].  Returns (path_group in cluster order, cluster_group_off)."""
    path_group, cluster_group_off = [], [0]
    for paths in clusters:
        group_name_index = {}
        for path_id in paths:                                                  # :855
            group_name_index.setdefault(name_id[path_id], len(group_name_index))  # :885 emplace(name, size)
        path_group.extend(group_name_index[name_id[p]] for p in paths)
        cluster_group_off.append(cluster_group_off[-1] + len(group_name_index))
    return path_group, cluster_group_off


def sequential_sum(eff, counts):
    """The reference's loop (:931, :940): acc = e0 * c0; acc += e * c, every product and every sum rounded once."""
    acc = eff[0] * float(counts[0])
    for e, c in zip(eff[1:], counts[1:]):
        acc = acc + e * float(c)
    return acc


def reversed_sum(eff, counts):
    return sequential_sum(eff[::-1], counts[::-1])


def fused_sum(eff, counts):
    """What a fused multiply-add would give: acc = round(e * c + acc), one rounding per member."""
    acc = 0.0
    for e, c in zip(eff, counts):
        acc = float(Fraction(e) * c + Fraction(acc))  # (float(Fraction) rounds once, to nearest even)
    return acc


def three_sums_differ(eff, counts):
    return len({sequential_sum(eff, counts), reversed_sum(eff, counts), fused_sum(eff, counts)}) == 3


def collapsed_paths(clusters, table):
    """Per cluster the list of collapsed paths, each a dict(first_path, name_id, group_id, source_count, length, effective_length)."""
    out = []
    for k, paths in enumerate(clusters):
        group_name_index = {}
        for p in paths:
            group_name_index.setdefault(table["name_id"][p], len(group_name_index))
        collapsed = [None] * len(group_name_index)                             # :912
        for p in paths:                                                        # :914
            g = group_name_index[table["name_id"][p]]
            sc = int(table["source_count"][p])
            if sc == 0:
                raise InvalidGroup(k, g, "source count 0")
            if collapsed[g] is None:                                           # :924-931
                collapsed[g] = dict(first_path=p, name_id=int(table["name_id"][p]), group_id=int(table["group_id"][p]), source_count=sc,
                                    length=int(table["length"][p]) * sc, effective_length=float(table["effective_length"][p]) * float(sc))
            else:                                                              # :938-940
                c = collapsed[g]
                c["source_count"] += sc
                c["length"] += int(table["length"][p]) * sc
                c["effective_length"] = c["effective_length"] + float(table["effective_length"][p]) * float(sc)
        for g, c in enumerate(collapsed):                                      # :944-948
            if c["source_count"] > UINT32_MAX:
                raise InvalidGroup(k, g, "source counts beyond 32 bits")
            c["length"] = c_round(float(c["length"]) / float(c["source_count"]))
            if c["length"] > UINT32_MAX:
                raise InvalidGroup(k, g, "length beyond 32 bits")
            c["effective_length"] = c["effective_length"] / float(c["source_count"])
        out.append(collapsed)
    return out


def first_invalid_group(clusters, table):
    """(cluster, group) of the first group, in cluster then group order, that collapsed_paths refuses; None if there is none."""
    for k, paths in enumerate(clusters):
        groups, off = name_groups([paths], table["name_id"])
        for g in range(off[1]):
            members = [p for p, pg in zip(paths, groups) if pg == g]
            total = sum(int(table["source_count"][p]) for p in members)
            if any(int(table["source_count"][p]) == 0 for p in members) or total > UINT32_MAX:
                return k, g
    return None


def path_side(clusters, table):
    """group ids, source offsets and source ids in cluster order (source arrays None for a table without haplotype ids)."""
    group_id = [int(table["group_id"][p]) for paths in clusters for p in paths]
    if table["source_ids"] is None:
        return group_id, None, None
    off, ids = [0], []
    for paths in clusters:
        for p in paths:
            ids.extend(int(s) for s in table["source_ids"][p])
            off.append(len(ids))
    return group_id, off, ids


# ---- tables and cases ------------------------------------------------------------------------------------------------------

def make_table(num_paths, name_id=None, source_ids=None, source_count=None, length=None, effective_length=None, group_id=None, seed=0):
    rng = np.random.default_rng(seed)
    return dict(
        group_id=list(group_id) if group_id is not None else [int(x) for x in rng.integers(0, 50, size=num_paths)],
        source_count=list(source_count) if source_count is not None else [int(x) for x in rng.integers(1, 900, size=num_paths)],
        source_ids=source_ids,
        name_id=list(name_id) if name_id is not None else None,
        length=list(length) if length is not None else [int(x) for x in rng.integers(200, 9000, size=num_paths)],
        effective_length=list(effective_length) if effective_length is not None else [float(x) for x in rng.uniform(50.0, 8000.0, size=num_paths)])


THREE_SUM_TRIPLE = ((3443.520070245456, 4568.900641887635, 852.3741444655479), (418, 633, 776))


def random_triples(seed, n):
    rng = np.random.default_rng(seed)
    return [(tuple(float(x) for x in rng.uniform(50.0, 8000.0, size=3)), tuple(int(x) for x in rng.integers(1, 900, size=3))) for _ in range(n)]


def three_sum_cases(seed, n):
    """n (effective lengths, counts) triples whose sequential, reversed and fused sums are three different doubles."""
    out, s = [THREE_SUM_TRIPLE], seed
    while len(out) < n:
        out.extend(t for t in random_triples(s, 64) if three_sums_differ(*t))
        s += 1
    return out[:n]


def non_monotone_names(rng, n, num_names):
    """n name ids over at most num_names names whose sequence along the cluster is neither ascending nor descending; the ids are
    large, sparse and unrelated to the order of first appearance."""
    assert n >= 3 and num_names >= 2
    values = [int(x) for x in rng.choice(np.arange(1, 2 ** 32 - 1, 65521, dtype=np.uint64), size=num_names, replace=False)]
    while True:
        ids = [values[int(i)] for i in rng.integers(0, num_names, size=n)]
        steps = [b - a for a, b in zip(ids, ids[1:]) if b != a]
        if any(s > 0 for s in steps) and any(s < 0 for s in steps):
            return ids


def is_monotone(ids):
    steps = [b - a for a, b in zip(ids, ids[1:])]
    return all(s >= 0 for s in steps) or all(s <= 0 for s in steps)


def hand_case():
    """One cluster of five paths named a b a c b (src/main.cpp:853-887) with the collapsed paths of :909-951 worked by hand."""
    a, b, c = 70, 20, 50   # name ids: neither dense nor in the order of appearance
    table = make_table(5, name_id=[a, b, a, c, b], source_count=[1, 1, 1, 2, 3], length=[1, 10, 2, 7, 20],
                       effective_length=[1.5, 4.0, 2.5, 3.0, 8.0], group_id=[9, 8, 9, 7, 8])
    expected_groups = [0, 1, 0, 2, 1]
    expected = [
        dict(first_path=0, name_id=a, group_id=9, source_count=2, length=2, effective_length=2.0),    # (1 + 2) / 2 = 1.5 -> 2; (1.5 + 2.5) / 2
        dict(first_path=1, name_id=b, group_id=8, source_count=4, length=18, effective_length=7.0),   # (10 + 60) / 4 = 17.5 -> 18; (4 + 24) / 4
        dict(first_path=3, name_id=c, group_id=7, source_count=2, length=7, effective_length=3.0),    # 14 / 2; 6 / 2
    ]
    return [[0, 1, 2, 3, 4]], table, expected_groups, expected
