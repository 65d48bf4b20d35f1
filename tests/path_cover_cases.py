"""The weighted minimum path cover of `-i strains` restated, and clusters at the edges of minPathCoverKernel (test-only;
plain Python and numpy, no GPU).

cover_model restates src/path_abundance_estimator.cpp:233-257 (cover matrix, path weights) and :297-340 (the greedy
rounds) with the weight of a path as the CORRECTLY ROUNDED sum of its terms count * log(prob) (math.fsum: independent of
any order of additions) and the covered read counts as Python integers.  Next to the cover it returns its decision
margin: over every round and every two candidate paths (positive covered count) that are not twins, the smallest relative
distance of their ratios covered / weight.  Twins are two columns with the same rows and the same (row, probability
group) membership: their terms are the same numbers, the reference adds them in the same (row) order, so their weights
are bit-equal there and its ascending scan (:320-327) keeps the lower index.

Every case has a margin of at least MIN_MARGIN = 1e-9.  That is derived, not measured: the terms of a weight have one
sign, so any order of additions of R <= 4096 terms is within R * 2^-53 ~ 4.5e-13 relative of the exact sum, and the
device's log adds a few ulp per term.  A kernel whose weights are sums of the right terms in ANY order therefore takes the
model's decision in every round — except between twins, where only bit-equal weights give the reference's lower index.

parent_order_weights emulates the one order that is known to break the tie: LDS atomics from the 256 threads of a
workgroup, a thread per row walking the row's entry list, served (position in the entry list, lane) — a path's terms
then arrive in an order that depends on which other paths stand before it in each row.  The twin cases are drawn (seeds
chosen here, on the CPU) so that this order gives the SECOND twin the smaller weight: a kernel that adds that way returns
the higher index.

Rows obey the invariants tests/em_bin_cases.py states as far as the cover reads them: probabilities ascending within a
row, noise in (0, 1].  The members of a probability group are listed in any order (the kernel's entry list is the groups
one after the other, members as listed).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import np_oracle
from rpvg_amd.batch import ClusterBatch

MIN_MARGIN = 1e-9
BLOCK = 256          # kBlock of path_cover.hip
MAX_PATHS = 9600     # kMaxPaths: two vectors of doubles per path in 150 KiB of LDS

Row = Tuple[int, float, List[Tuple[float, List[int]]]]


@dataclass
class Cluster:
    n_paths: int
    rows: List[Row]    # (read count, noise, [(prob, [path...])...]) with the probabilities ascending

    def as_dict(self) -> dict:
        return dict(paths=[dict(group_id=0, source_ids=[j], source_count=1, effective_length=100.0) for j in range(self.n_paths)],
                    rows=self.rows)


def batch_of(clusters: Sequence[Cluster]) -> ClusterBatch:
    return ClusterBatch.from_clusters([c.as_dict() for c in clusters])


# ---- the model --------------------------------------------------------------------------------------------------------
def read_counts(cluster: Cluster, noise_rule: bool = True) -> List[int]:
    """:234-237 — a row whose noise passes Utils::doubleCompare(noise, 1) counts 0."""
    return [0 if (noise_rule and np_oracle.double_compare(noise, 1.0)) else int(c) for c, noise, _ in cluster.rows]


def columns(cluster: Cluster) -> List[List[Tuple[int, int, int, float]]]:
    """Per path its entries (row, probability group of the row, position in the row's entry list, probability)."""
    cols: List[List[Tuple[int, int, int, float]]] = [[] for _ in range(cluster.n_paths)]
    for r, (_, _, groups) in enumerate(cluster.rows):
        pos = 0
        for g, (prob, members) in enumerate(groups):
            for j in members:
                cols[j].append((r, g, pos, prob))
                pos += 1
    return cols


def twin_classes(cluster: Cluster) -> List[int]:
    """Per path the smallest index among the paths with the same (row, probability group) entries."""
    first: Dict[tuple, int] = {}
    return [first.setdefault(tuple((r, g) for r, g, _, _ in col), j) for j, col in enumerate(columns(cluster))]


def _terms(cluster: Cluster, counts: Sequence[int]) -> List[List[Tuple[int, int, float]]]:
    """Per path (row, position, count * log(prob)): each product rounded once, as :246 computes it."""
    return [[(r, pos, math.log(prob) * float(counts[r])) for r, _, pos, prob in col] for col in columns(cluster)]


def exact_weights(cluster: Cluster, noise_rule: bool = True) -> List[float]:
    return [-math.fsum(t for _, _, t in col) for col in _terms(cluster, read_counts(cluster, noise_rule))]


def _sequential(terms: Sequence[float]) -> float:
    acc = 0.0
    for t in terms:
        acc += t
    return -1.0 * acc


def row_order_weights(cluster: Cluster) -> List[float]:
    """The reference's and the oracle's own order (oracle/rpvg_oracle.cpp:750-762): ascending rows."""
    return [_sequential([t for _, _, t in sorted(col)]) for col in _terms(cluster, read_counts(cluster))]


def parent_order_weights(cluster: Cluster) -> List[float]:
    """The order of a thread per row adding with LDS atomics, were the 256 threads in lockstep and lanes that meet served
    in lane order: (stride of 256 rows, position in the row's entry list, row)."""
    return [_sequential([t for _, _, _, t in sorted((r // BLOCK, pos, r % BLOCK, t) for r, pos, t in col)])
            for col in _terms(cluster, read_counts(cluster))]


def _round_margin(cands: Sequence[Tuple[float, int]], classes: Optional[Sequence[int]]) -> float:
    reps: Dict[int, float] = {}
    for ratio, j in cands:
        key = j if classes is None else classes[j]
        assert reps.setdefault(key, ratio) == ratio, "twins with different ratios"
    v = sorted(reps.values())
    margin = math.inf
    for a, b in zip(v, v[1:]):
        margin = min(margin, (0.0 if math.isinf(a) else 1.0) if math.isinf(b) else (b - a) / b)
    return margin


def greedy_cover(n_paths: int, col_rows: Sequence[Sequence[int]], counts: Sequence[int], weights: Sequence[float],
                 classes: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int], float]:
    """:297-340 — (cover ascending, the paths in the order the rounds chose them, decision margin)."""
    if n_paths == 1:
        return [0], [0], math.inf
    uncovered = [int(c) for c in counts]
    present = [j for j in range(n_paths) if len(col_rows[j])]
    order: List[int] = []
    margin = math.inf
    while max(uncovered, default=0) > 0:
        best, best_j, cands = 0.0, -1, []
        for j in present:
            cov = sum(uncovered[r] for r in col_rows[j])
            if cov <= 0:
                continue
            ratio = math.inf if weights[j] == 0 else cov / weights[j]
            cands.append((ratio, j))
            if ratio > best:   # first index among equals
                best, best_j = ratio, j
        assert best_j >= 0
        margin = min(margin, _round_margin(cands, classes))
        order.append(best_j)
        for r in col_rows[best_j]:
            uncovered[r] = 0
    return sorted(order), order, margin


@dataclass
class CoverResult:
    cover: List[int]
    order: List[int]
    margin: float


def cover_model(cluster: Cluster, noise_rule: bool = True, weights: Optional[Sequence[float]] = None) -> CoverResult:
    col_rows = [[r for r, _, _, _ in col] for col in columns(cluster)]
    w = exact_weights(cluster, noise_rule) if weights is None else weights
    return CoverResult(*greedy_cover(cluster.n_paths, col_rows, read_counts(cluster, noise_rule), w,
                                     twin_classes(cluster) if weights is None else None))


def dense_cover(cluster: Cluster) -> np.ndarray:
    """read_path_cover of :229-249, rows x paths."""
    cover = np.zeros((len(cluster.rows), cluster.n_paths), dtype=np.uint8)
    for j, col in enumerate(columns(cluster)):
        cover[[r for r, _, _, _ in col], j] = 1
    return cover


# ---- clusters ---------------------------------------------------------------------------------------------------------
def _noise(rng, n_rows: int) -> np.ndarray:
    """Pairwise distinct noise in (1e-4, 0.2): a permutation of evenly spaced values."""
    return 1e-4 + (0.2 - 1e-4) * (rng.permutation(n_rows) + 0.5) / n_rows


def _row(count: int, noise: float, groups: List[Tuple[float, List[int]]]) -> Row:
    groups = sorted(groups, key=lambda g: g[0])
    assert all(a[0] < b[0] for a, b in zip(groups, groups[1:]))
    return int(count), float(noise), groups


def twin_cluster(seed: int, n_rows: int, n_paths: int, first: int = 0, second: int = 2, middle: int = 1,
                 descending: bool = False, decoys: Optional[Sequence[int]] = None) -> Cluster:
    """Twins `first` and `second` share a probability group in ~85 % of the rows; `middle` stands between them in that
    group's member list in about half of those rows (so the second twin is one or two places behind the first, row by
    row) and alone in some of the others.  The other paths (`decoys`: every other path by default) have groups of their
    own at lower probabilities, which sort in front of the twins' group."""
    rng = np.random.default_rng(seed)
    others = [j for j in range(n_paths) if j not in (first, second, middle)] if decoys is None else list(decoys)
    noise = _noise(rng, n_rows)
    rows = []
    for r in range(n_rows):
        scale = 1.0 - noise[r]
        groups: List[Tuple[float, List[int]]] = []
        if rng.random() < 0.85:
            members = [first] + ([middle] if rng.random() < 0.5 else []) + [second]
            groups.append((float(rng.uniform(0.15, 0.3) * scale), members[::-1] if descending else members))
        elif rng.random() < 0.6 or not others:
            groups.append((float(rng.uniform(0.15, 0.3) * scale), [middle]))
        for j in others:
            if rng.random() < (0.4 if len(others) <= 8 else 2.0 / len(others)) or (not groups and j == others[-1]):
                groups.append((float(rng.uniform(0.01, 0.1) * scale), [j]))
        rows.append(_row(rng.integers(1, 21), noise[r], groups))
    return Cluster(n_paths, rows)


REDUCTION_PATHS = 600
REDUCTION_PAIRS = ((0, 256), (63, 64), (255, 256), (5, 300), (257, 513))


def reduction_cluster(seed: int, pair: Tuple[int, int]) -> Cluster:
    """N = 600 with the twins at `pair`: on one thread in two strides of the argmax, on neighbouring lanes across a
    wavefront edge, across the block stride, in different wavefronts.  The member between them in the group is a third
    path (the group's list need not ascend); twenty decoys at low probabilities."""
    rng = np.random.default_rng(seed)
    a, b = pair
    rest = [j for j in range(REDUCTION_PATHS) if j not in pair]
    picked = [int(x) for x in rng.choice(rest, size=21, replace=False)]
    return twin_cluster(seed, 48, REDUCTION_PATHS, first=a, second=b, middle=picked[0], decoys=sorted(picked[1:]))


def wide_planted(n_paths: int) -> List[int]:
    """At most 8 paths at the low end, the wavefront and stride edges and the high end."""
    return sorted({j for j in (0, 63, 64, 255, 256, 257, n_paths - 2, n_paths - 1) if 0 <= j < n_paths})[:8]


def wide_cluster(seed: int, n_paths: int) -> Cluster:
    """64 rows; row r belongs to one planted path (probability 0.3 .. 0.6), next to up to two of 40 decoys (probability
    below 0.01): the cover is the planted paths."""
    rng = np.random.default_rng(seed)
    planted = wide_planted(n_paths)
    pool = [int(x) for x in rng.choice([j for j in range(n_paths) if j not in planted], size=min(40, n_paths - len(planted)), replace=False)]
    noise = _noise(rng, 64)
    rows = []
    for r in range(64):
        scale = 1.0 - noise[r]
        groups = [(float(rng.uniform(0.3, 0.6) * scale), [planted[r % len(planted)]])]
        for j in rng.choice(pool, size=int(rng.integers(0, 3)), replace=False):
            groups.append((float(rng.uniform(1e-3, 1e-2) * scale), [int(j)]))
        rows.append(_row(rng.integers(1, 21), noise[r], groups))
    return Cluster(n_paths, rows)


def long_cover_cluster(seed: int, n: int = 600) -> Cluster:
    """Row i holds one path, each path one row: a cover of all n paths in n rounds, chosen by descending probability —
    a random order of the indices."""
    rng = np.random.default_rng(seed)
    noise = _noise(rng, n)
    path = rng.permutation(n)
    prob = rng.uniform(0.01, 0.9, size=n) * (1.0 - noise)
    return Cluster(n, [_row(rng.integers(1, 21), noise[i], [(float(prob[i]), [int(path[i])])]) for i in range(n)])


NOISE_ONE = (1.0, 1.0 - 1e-14)         # pass doubleCompare(noise, 1): the row counts 0
NOISE_NOT_ONE = (1.0 - 4e-14, 0.5)     # do not
NOISE_ONE_WINNER = 1                   # the path that only rows counting 0 contain


def noise_one_cluster(seed: int) -> Cluster:
    """Path 1 sits only in rows whose noise is 1.0 or 1 - 1e-14, with large counts and high probabilities: if those rows
    counted it would be the first choice.  The rows that count (noise 1 - 4e-14 and 0.5) hold paths 0, 2, 3, 4."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(8):
        groups = [(float(rng.uniform(0.5, 0.6)), [NOISE_ONE_WINNER])]
        if i % 2:
            groups.append((float(rng.uniform(0.01, 0.1)), [int(rng.choice([0, 2, 3, 4]))]))
        rows.append(_row(rng.integers(40, 60), NOISE_ONE[i % 2], groups))
    for i in range(12):
        members = [int(x) for x in rng.choice([0, 2, 3, 4], size=int(rng.integers(1, 4)), replace=False)]
        rows.append(_row(rng.integers(1, 21), NOISE_NOT_ONE[i % 2], [(float(rng.uniform(0.01, 0.4)), [j]) for j in members]))
    return Cluster(5, [rows[i] for i in rng.permutation(len(rows))])


def nothing_to_cover_cluster(seed: int) -> Cluster:
    rng = np.random.default_rng(seed)
    return Cluster(3, [_row(rng.integers(1, 21), NOISE_ONE[i % 2], [(float(rng.uniform(0.01, 0.4)), [int(rng.integers(0, 3))])])
                       for i in range(6)])


def single_path_cluster(seed: int, all_noise_one: bool) -> Cluster:
    rng = np.random.default_rng(seed)
    return Cluster(1, [_row(rng.integers(1, 21), 1.0 if all_noise_one else float(rng.uniform(0.01, 0.2)),
                            [(float(rng.uniform(0.1, 0.7)), [0])]) for _ in range(6)])


# ---- the table --------------------------------------------------------------------------------------------------------
@dataclass
class CoverCase:
    name: str
    kind: str
    build: Callable[[], Cluster]
    twins: Optional[Tuple[int, int]] = None    # (first, second): the cover holds the first and not the second
    _cluster: Optional[Cluster] = field(default=None, repr=False)
    _model: Optional[CoverResult] = field(default=None, repr=False)

    def cluster(self) -> Cluster:
        if self._cluster is None:
            self._cluster = self.build()
        return self._cluster

    def model(self) -> CoverResult:
        """Computed once; shared by every test that needs it."""
        if self._model is None:
            self._model = cover_model(self.cluster())
        return self._model


def twin_seed_ok(cluster: Cluster, first: int, second: int) -> bool:
    """What a twin case needs: the margin; the twins the first choice of a round (the model keeps the first); and the
    emulated parent order giving the second twin the smaller weight, hence the cover with the second twin."""
    m = cover_model(cluster)
    if m.margin < MIN_MARGIN or first not in m.cover or second in m.cover:
        return False
    w = parent_order_weights(cluster)
    if not w[second] < w[first]:
        return False
    emulated = cover_model(cluster, weights=w)
    return second in emulated.cover and first not in emulated.cover


def find_seeds(make: Callable[[int], Cluster], first: int, second: int, start: int, want: int) -> List[int]:
    """How the seeds below were chosen (not run by any test)."""
    out, seed = [], start
    while len(out) < want:
        if twin_seed_ok(make(seed), first, second):
            out.append(seed)
        seed += 1
    return out


# The first seeds that pass, e.g. find_seeds(lambda s: twin_cluster(s, 48, 3 + s % 4, descending=False), 0, 2, 1000, 8);
# keyed by `descending`; the searches started at 1000 / 2000, 3000 / 4000 and 9000 + 100 * (index of the pair).
ONE_WAVEFRONT_SEEDS = {False: (1000, 1001, 1006, 1016, 1017, 1020, 1021, 1031), True: (2002, 2004, 2005, 2010, 2023, 2025, 2029, 2031)}
MANY_WAVEFRONTS_SEEDS = {False: (3001, 3005, 3006, 3008), True: (4000, 4006, 4007, 4008)}
REDUCTION_SEEDS = {(0, 256): 9001, (63, 64): 9100, (255, 256): 9202, (5, 300): 9303, (257, 513): 9405}


def _cases() -> List[CoverCase]:
    cases: List[CoverCase] = []
    for desc in (False, True):
        tag = "desc" if desc else "asc"
        for s in ONE_WAVEFRONT_SEEDS[desc]:
            cases.append(CoverCase(f"twins_one_wavefront_{tag}_{s}", "twins_one_wavefront",
                                   lambda s=s, desc=desc: twin_cluster(s, 48, 3 + s % 4, descending=desc), (0, 2)))
        for s in MANY_WAVEFRONTS_SEEDS[desc]:
            cases.append(CoverCase(f"twins_many_wavefronts_{tag}_{s}", "twins_many_wavefronts",
                                   lambda s=s, desc=desc: twin_cluster(s, 300, 3 + s % 4, descending=desc), (0, 2)))
    for pair in REDUCTION_PAIRS:
        s = REDUCTION_SEEDS[pair]
        cases.append(CoverCase(f"twins_across_the_reduction_{pair[0]}_{pair[1]}", "twins_across_the_reduction",
                               lambda s=s, pair=pair: reduction_cluster(s, pair), pair))
    for n in (255, 256, 257, 4096, 4097, MAX_PATHS):
        cases.append(CoverCase(f"wide_{n}", "wide", lambda n=n: wide_cluster(5000 + n, n)))
    cases.append(CoverCase("long_cover", "long_cover", lambda: long_cover_cluster(6001)))
    cases.append(CoverCase("noise_one", "noise_one", lambda: noise_one_cluster(7001)))
    cases.append(CoverCase("nothing_to_cover", "nothing_to_cover", lambda: nothing_to_cover_cluster(7101)))
    cases.append(CoverCase("single_path", "single_path", lambda: single_path_cluster(7201, False)))
    cases.append(CoverCase("single_path_noise_one", "single_path", lambda: single_path_cluster(7202, True)))
    return cases


CASES: List[CoverCase] = _cases()
BY_NAME: Dict[str, CoverCase] = {c.name: c for c in CASES}
TWIN_CASES = [c for c in CASES if c.twins is not None]


def several_in_one_call() -> Tuple[List[CoverCase], Dict[str, Tuple[List[int], List[int]]]]:
    """The cases of one batch (every kind; the widest left out) and four ways to list them in one call: (indices into
    the batch, cells each output range has beyond the cluster's paths)."""
    base = [c for c in CASES if c.name not in ("wide_4097", f"wide_{MAX_PATHS}")]
    n = len(base)
    rng = np.random.default_rng(8001)
    perm = [int(x) for x in rng.permutation(n)]
    twice = BY_NAME["long_cover"]
    dup = [base.index(twice), 0, n - 1, base.index(twice), 3]
    return base, {"permutation": (perm, [0] * n),
                  "subset": (perm[::3], [0] * len(perm[::3])),
                  "one cluster twice": (dup, [0] * len(dup)),
                  "larger output ranges": (list(range(n)), [(7 * i) % 41 for i in range(n)])}
