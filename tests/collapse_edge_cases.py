"""Case table of the row collapse (rpvg_amd/csrc/row_collapse.hip: readCollapseProbabilityMatrix, src/path_estimator.cpp:197-259,
on every normalised group matrix and on the rows of every EM problem) at the sizes where its replay takes another route, and the
model the cases are judged by.  Plain numpy, no GPU: tests/test_collapse_edge_cases.py asserts the conditions the cases have
to meet, tests/test_hip_collapse_edges.py runs them on the device.

THE MODEL.  collapse_heads(P, counts, precision) -> head[r]: the reference's tolerant sort (probabilityCountRowSorter,
src/path_estimator.cpp:13-31) and its compare-with-the-run-head rule (:226-255), returning for every row the row whose values
it takes.  P holds the noise as its last column, as the reference's matrix does.

HOW THE CASES ARE PLANTED.  Every case is a cluster whose columns are single paths, so a matrix value is a row's own entry,
normalised: (p / s) * (1 - noise) with s the row's sum (src/path_estimator.cpp:156-166).  The entries are integers times
U = 2^-40 that add up, with the noise, to 1: s and 1 - noise are then exact and equal, and two rows of one noise that share an
entry share the value BIT FOR BIT — so a pair can differ in chosen columns only, by chosen amounts: multiples of Q = 2750 U =
0.2501e-8 ("a quarter"), rungs of 6597 U = 0.6e-8, steps of 12 U = 1.1e-11 inside a crowd.  A row sums to 1 - noise, so an
offset in one column is taken back elsewhere: "a pair that differs only in column c" is a pair whose only column with a
distance ABOVE the precision is c (+5 quarters there, -2 and -3 in two other columns) or whose largest distance is in c (+2
there, -1 and -1): a replay that does not look at c merges the first and would still merge the second.  A pair that differs
only in the noise has equal entries, so its columns differ by the noise's step times the value.  Anchor rows ascend in
column 0 in steps of 1e-3 (less where more than 600 anchors have to fit below 1: 0.6 / anchors, four orders above the
precision), so a row's sorted position is known: anchors in index order, satellites next to their anchor.

THREE LISTS.  CASES: the group matrices' cases, one batch, built plain and collapsed.  HELD_CASES: matrices from the batch's own
columns, searched while the collapse's last stage is held back — their columns are level (all near 1 / G, anchors 1e-5 apart), so
that no pair of columns is dropped by the search.  EM_CASES: EM problems of three columns, every other anchor with its columns 1 and
2 exchanged and the counts balanced, so that two paths keep an abundance and a merge shows in it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

PRECISION = 1e-8
DOUBLE_PRECISION = float(np.finfo(np.float64).eps) * 100   # src/utils.hpp:81
EQUIVALENT_RELATIVE = 1e-13     # kEquivalentRelative: close rows no further apart are left alone by the device
APART_RELATIVE = 1e-11          # condition (a): two values of a column are bit-identical or at least this far apart
CLOSE_BELOW, APART_ABOVE = 0.9e-8, 1.1e-8   # condition (b)
EM_BAR = 1e-10                  # abundances of a collapsed EM solve against the oracle's (test_hip_collapse.py's bar)

U = 2.0 ** -40
ONE = 1 << 40
Q = 2750                        # a quarter of the precision: 0.2501e-8
RUNG = 6597                     # 0.6e-8
CROWD_STEP = 12                 # 1.1e-11
NOISE = 109951163               # 1e-4
STEP_1E3 = 1099511628           # 1e-3 (rounded up)
A0 = ONE // 20
MID_TOTAL = ONE // 5

# the constants of row_collapse.hip / collapse_plan.hpp / common.hpp that the targets are restated from
LDS_TABLE_ROWS = 128            # kLdsTableRows
PAIRWISE_ROWS = 1024            # kPairwiseRows
LIST_LDS_ROWS = 2048            # kListLdsRows
MAX_WINDOW_COMPARES = 256       # kMaxWindowCompares
PAIR_CHUNK = 256                # kPairChunk
BETWEEN_ROWS = 512              # kBetweenRows
BATCH = 8                       # kBatch (forEachColumnPair)
PATTERN_COLUMNS = 64            # columns with a bit in the zero pattern
KEY_FRACTION_BITS = 22          # kCollapseKeyFractionBits
PRODUCT_MIN_NOISE = 2.0 ** -30  # kProductMinNoise
MID_MAX_COUNT = 8               # kMidMaxCount
STAGE_ROWS = 32                 # kStageRows (adjustSearchSums)
ADJUST_SLICES = 16              # kAdjustSlices
SEARCH_CHUNK_ROWS = 1024        # rows per chunk of the tile kernel's sums (search_plan.hpp)

ROUTES = ("table_lds", "table_global", "sort_lds", "sort_global")


def list_route(listed: int) -> str:
    """The replay's route for a list of `listed` rows that is not a whole matrix."""
    if listed <= LDS_TABLE_ROWS:
        return "table_lds"
    if listed <= PAIRWISE_ROWS:
        return "table_global"
    padded = 1
    while padded < listed:
        padded <<= 1
    return "sort_lds" if padded <= LIST_LDS_ROWS else "sort_global"


# ---- the model --------------------------------------------------------------------------------------------------------------

def tolerant_equal(a: float, b: float) -> bool:   # Utils::doubleCompare, src/utils.hpp:87-93
    return a == b or abs(a - b) < abs(min(a, b)) * DOUBLE_PRECISION


def tolerant_order(P: np.ndarray, counts: np.ndarray) -> List[int]:
    """The rows in the order of probabilityCountRowSorter (src/path_estimator.cpp:13-31): column by column, the first pair of
    values that is not tolerantly equal decides; then the counts.  (sorted() is stable and std::sort is not: they differ on rows
    that compare equal, which under condition (a) are bit-for-bit copies with equal counts.)"""
    rows = [tuple(float(v) for v in P[i]) for i in range(P.shape[0])]
    cnt = [float(c) for c in counts]

    def cmp(i, j):
        for x, y in zip(rows[i], rows[j]):
            if x != y and not abs(x - y) < abs(min(x, y)) * DOUBLE_PRECISION:
                return -1 if x < y else 1
        if not tolerant_equal(cnt[i], cnt[j]):
            return -1 if cnt[i] < cnt[j] else 1
        return 0

    return sorted(range(len(rows)), key=functools.cmp_to_key(cmp))


def rows_close(P: np.ndarray, a: int, b: int, precision: float) -> bool:
    return bool(np.all(np.abs(P[a] - P[b]) < precision))   # src/path_estimator.cpp:232-239


def collapse_heads(P: np.ndarray, counts: np.ndarray, precision: float = PRECISION, rule: str = "head", skip: np.ndarray = None) -> np.ndarray:
    """head[r] = the row whose values row r takes.  rule "head": the reference's (a row joins the run if it is close to the
    run's HEAD, else it becomes the head); "predecessor": the deliberately wrong rule of condition (e).  skip: rows the walk does
    not see (the other wrong model: inactive rows in between ignored)."""
    R = P.shape[0]
    head = np.arange(R, dtype=np.int64)
    h = prev = -1
    for r in tolerant_order(P, counts):
        if skip is not None and skip[r]:
            continue
        if h >= 0 and rows_close(P, h if rule == "head" else prev, r, precision):
            head[r] = h
        else:
            h = r
        prev = r
    return head


def merged(P: np.ndarray, counts: np.ndarray, head: np.ndarray):
    """What the reference's function returns for these heads: the head rows in sorted order, the counts of their runs added up."""
    order = [r for r in tolerant_order(P, counts) if head[r] == r]
    total = np.zeros(P.shape[0])
    np.add.at(total, head, counts)
    return P[order], total[order]


def close_partners(P: np.ndarray, precision: float = PRECISION, identical_too: bool = False) -> np.ndarray:
    """Per row: has another row within the precision in every column (that is not its bit-for-bit copy)."""
    R = P.shape[0]
    out = np.zeros(R, dtype=bool)
    order = np.argsort(P[:, 0], kind="stable")   # close rows are close in column 0: a window over it
    v = P[order, 0]
    hi = np.searchsorted(v, v + precision, side="left")
    for i in range(R):
        j = np.arange(i + 1, hi[i])
        if len(j) == 0:
            continue
        d = np.abs(P[order[j]] - P[order[i]])
        ok = np.all(d < precision, axis=1)
        if not identical_too:
            ok &= np.any(d != 0, axis=1)
        if ok.any():
            out[order[i]] = True
            out[order[j[ok]]] = True
    return out


def wrong_heads(P: np.ndarray, counts: np.ndarray, which: str) -> np.ndarray:
    """The three deliberately wrong models of condition (e)."""
    if which == "predecessor":
        return collapse_heads(P, counts, rule="predecessor")
    if which == "ignore_inactive":
        return collapse_heads(P, counts, skip=~close_partners(P, identical_too=True))
    if which == "no_wide_columns":
        keep = list(range(min(P.shape[1] - 1, PATTERN_COLUMNS))) + [P.shape[1] - 1]
        return collapse_heads(P[:, keep], counts)
    raise ValueError(which)


WRONG_MODELS = ("predecessor", "ignore_inactive", "no_wide_columns")


def replaced_rows(P: np.ndarray, head: np.ndarray) -> int:
    """Rows that take the values of another row and are changed by it (rpvg_hip_groups_collapse_info's rows_replaced)."""
    return int(np.sum(np.any(P != P[head], axis=1)))


# ---- the device's side of things, restated ----------------------------------------------------------------------------------------

def row_class(count: float, noise: float) -> int:   # rowClass, common.hpp
    if not noise >= PRODUCT_MIN_NOISE:
        return MID_MAX_COUNT
    if count == 1.0:
        return 0
    for c in range(2, MID_MAX_COUNT + 1):
        if count == float(c):
            return c - 1
    return MID_MAX_COUNT


def matrix_row_order(counts: np.ndarray, noise: np.ndarray) -> np.ndarray:
    """The cluster row behind every row of a built matrix: by class, in cluster order within a class (partitionRowsKernel)."""
    cls = np.array([row_class(float(c), float(z)) for c, z in zip(counts, noise)])
    return np.argsort(cls, kind="stable")


def collapse_weight(column: int) -> float:   # collapseWeight, common.hpp
    return float(((column * 0x9E3779B1 & 0xFFFFFFFF) >> 8) & 0xFFFF) / 32768.0


def window_candidates(P: np.ndarray, precision: float = PRECISION):
    """(largest number of candidates the forward window scan lists for one row, candidate pairs in all) counted twice: the rows
    behind a row whose projection keys SURELY lie within windowQuanta() of its own, and those that MAY — the device compares keys
    cut to quanta of 2^-22, so a difference counts for sure up to a quantum below the window and is out for sure a quantum above
    it.  A target holds where both counts agree.  Bit-for-bit copies count once (the scan steps from stretch to stretch).  The
    filter on the largest values can only take candidates away from rows that are not close; between close rows it passes."""
    G = P.shape[1] - 1
    w = np.array([collapse_weight(c) for c in range(G + 1)])
    quantum = 2.0 ** -KEY_FRACTION_BITS
    _, first = np.unique(P, axis=0, return_index=True)
    key = np.sort(P[first] @ w)
    window_q = int((2.0001 * (G + 1) * precision + 1e-12) / quantum) + 2   # windowQuanta()
    out = []
    for quanta in (window_q - 1, window_q + 1):
        listed = np.searchsorted(key, key + quanta * quantum, side="right") - np.arange(len(key)) - 1
        out += [int(listed.max()) if len(key) else 0, int(listed.sum())]
    return tuple(out)


def pair_capacity(total_rows: int) -> int:   # planCollapse, collapse_plan.hpp
    return 4 * total_rows + 4096


# ---- cases ------------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    G: int
    rows: list                                   # [(entries [G] in units of U, noise in units of U, count)] in cluster row order
    kind: str = "exact"                          # "exact" | "rounding" (satellites an ulp or two from their anchor)
    route: str = "table_lds"                     # the replay's route (list_route of its listed rows) or "whole"
    listed: int = None                           # listed rows, where the case is about them
    whole: int = 0                               # 1: the matrix is sorted as a whole
    bites: tuple = ()                            # the wrong models that change a head on this case; none: a pure route case
    marks: dict = field(default_factory=dict)    # named rows (cluster row indices) the targets are asserted on
    columns: dict = field(default_factory=dict)  # {(row a, row b): the column the pair "differs only in" (deciding_column)}
    order_columns: dict = field(default_factory=dict)  # {(row a, row b): the first column in which the pair differs}
    raw: dict = field(default_factory=dict)      # rounding class: {(row, column): ulps} applied to the raw entry

    @property
    def R(self) -> int:
        return len(self.rows)

    def cluster(self) -> dict:
        rows = []
        for r, (entries, noise, count) in enumerate(self.rows):
            groups = []
            for c, v in enumerate(entries):
                if v:
                    p = v * U
                    p = float(p + self.raw.get((r, c), 0) * np.spacing(p))   # (ulps of p: a few thousand at the most, one binade)
                    groups.append((p, [c]))
            rows.append((int(count), noise * U, groups))
        # every path its own haplotype, path 0 a second one: the haplotype columns the upload forms are the single paths in
        # order (rpvg_hip_groups_build_from_sources), column 0 with a multiplicity of two
        paths = [dict(source_ids=[p] + ([self.G] if p == 0 else [])) for p in range(self.G)]
        return dict(paths=paths, rows=rows)

    def multiplicities(self) -> np.ndarray:
        return np.array([2] + [1] * (self.G - 1), dtype=np.uint32)

    def matrix(self):
        return _matrix(self.name)


def build_matrix(cluster: dict, G: int):
    """(P [R x (G + 1)] normalised, noise last; counts) in cluster row order: constructProbabilityMatrix +
    addNoiseAndNormalizeProbabilityMatrix (src/path_estimator.cpp:55-77,156-166), the sum of a row added up column by column."""
    R = len(cluster["rows"])
    M = np.zeros((R, G))
    noise, counts = np.zeros(R), np.zeros(R)
    for r, (count, z, groups) in enumerate(cluster["rows"]):
        counts[r], noise[r] = count, z
        for p, idxs in groups:
            for c in idxs:
                M[r, c] = p
    s = np.zeros(R)
    for c in range(G):
        s = s + M[:, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        Qn = (M / s[:, None]) * (1 - noise)[:, None]
    Qn[np.isnan(Qn)] = 0
    return np.concatenate([Qn, noise[:, None]], axis=1), counts


@functools.lru_cache(maxsize=None)
def _matrix(name: str):
    case = BY_NAME[name]
    P, counts = build_matrix(case.cluster(), case.G)
    P.setflags(write=False)
    counts.setflags(write=False)
    return P, counts


@functools.lru_cache(maxsize=None)
def heads_of(name: str) -> np.ndarray:
    P, counts = _matrix(name)
    head = collapse_heads(P, counts) if len(counts) else np.zeros(0, dtype=np.int64)
    head.setflags(write=False)
    return head


class _Builder:
    """Rows of one case: anchors ascending in column 0, satellites offset from them."""

    def __init__(self, G: int, anchors: int, zeros: Sequence[int] = (), level: bool = False):
        """level: every column near 1 / G and the anchors 1e-5 apart (the cases of the search: its pairs' sums stay within the
        650 log units in which no pair is dropped)."""
        self.G, self.zeros, self.level = G, tuple(zeros), level
        self.step = min(STEP_1E3, (ONE * 6 // 10) // max(anchors, 1)) if not level else STEP_1E3 // 100
        self.rows: list = []
        self.next_anchor = 0

    def anchor_entries(self, i: int, noise: int = NOISE, zeros: Sequence[int] = None) -> List[int]:
        G = self.G
        zeros = self.zeros if zeros is None else zeros
        if G == 1:
            return [ONE - noise]
        e = [0] * G
        e[0] = (ONE // G - ONE // 100 if self.level else A0) + i * self.step
        mid = ONE // G if self.level else MID_TOTAL // max(G - 2, 1)
        for c in range(1, G - 1):
            e[c] = 0 if c in zeros else mid
        e[G - 1] = ONE - noise - sum(e[:G - 1])
        assert e[G - 1] > ONE // 10 or self.level
        return e

    def add(self, entries: Sequence[int], noise: int = NOISE, count: int = 1, sums_to_one: bool = True) -> int:
        assert (sum(entries) + noise == ONE or not sums_to_one) and all(v >= 0 for v in entries), (sum(entries) + noise - ONE)
        self.rows.append((list(entries), int(noise), int(count)))
        return len(self.rows) - 1

    def anchor(self, count: int = 1, zeros: Sequence[int] = None) -> Tuple[int, List[int]]:
        """A new anchor (G == 1: the anchors descend in the noise, so that column 0 = 1 - noise ascends)."""
        i = self.next_anchor
        self.next_anchor += 1
        if self.G == 1:
            noise = NOISE + (4000 - i) * (STEP_1E3 // (800 if self.level else 8))
            return self.add([ONE - noise], noise, count), [ONE - noise]
        e = self.anchor_entries(i, zeros=zeros)
        return self.add(e, NOISE, count), e

    def sat(self, entries: Sequence[int], offsets: Dict[int, int], count: int = 1, noise: int = NOISE) -> int:
        """A row offset from `entries` by offsets[column] units (they add up to nothing: the row still sums to 1 - noise)."""
        assert sum(offsets.values()) == 0, offsets
        e = list(entries)
        for c, d in offsets.items():
            e[c] += d
        return self.add(e, noise, count)

    def fill(self, n: int):
        for _ in range(n):
            self.anchor()


def _companions(G: int, c: int) -> List[int]:
    """The two columns that take an offset in column c back: the next two, else the ones before."""
    return [x for x in (c + 1, c + 2, c - 1, c - 2) if 0 <= x < G][:2]


def _only_column(G: int, c: int, units: Tuple[int, int, int]) -> Dict[int, int]:
    """+units[0] in column c, taken back as -units[1], -units[2] in its companions (one companion: all of it)."""
    comp = _companions(G, c)
    if len(comp) == 1:
        return {c: units[0], comp[0]: -units[0]}
    return {c: units[0], comp[0]: -units[1], comp[1]: -units[2]}


CLOSE_IN = (2 * Q, Q, Q)        # largest distance 0.5e-8, in column c
APART_IN = (5 * Q, 2 * Q, 3 * Q)  # 1.25e-8 in column c alone


def _list_case(listed: int) -> Case:
    """`listed` active rows and no others: separated close pairs, one triple where the number is odd.  Every third pair has its
    satellite BELOW the anchor (the satellite is the head)."""
    pairs, triple = divmod(listed, 2)
    if triple:
        pairs -= 1
    b = _Builder(3, pairs + triple)
    for k in range(pairs):
        _, e = b.anchor()
        b.sat(e, {1: -2 * Q, 2: 2 * Q} if k % 3 == 2 else {1: 2 * Q, 2: -2 * Q})
    if triple:
        _, e = b.anchor()
        b.sat(e, {1: 2 * Q, 2: -2 * Q})
        b.sat(e, {1: 3 * Q, 2: -3 * Q})
    rows = _shuffled(b.rows, listed)
    return Case(f"list_{listed}", 3, rows, route=list_route(listed), listed=listed)


def _shuffled(rows: list, seed: int, keep: Sequence[int] = ()) -> list:
    """The rows in an order of the seed's (rows `keep` stay where they are)."""
    rng = np.random.default_rng(seed)
    free = [i for i in range(len(rows)) if i not in set(keep)]
    perm = rng.permutation(len(free))
    out = list(rows)
    for place, k in zip(free, perm):
        out[place] = rows[free[k]]
    return out


def _crowd_case(size: int) -> Case:
    """`size` mutually close rows (steps of 1.1e-11 in column 1) and six rows far from them: the lowest row of the crowd has
    size - 1 candidates in its forward window."""
    b = _Builder(3, 7)
    b.fill(3)
    _, e = b.anchor()
    for k in range(1, size):
        b.sat(e, {1: k * CROWD_STEP, 2: -k * CROWD_STEP})
    b.fill(3)
    whole = 1 if size - 1 > MAX_WINDOW_COMPARES else 0
    return Case(f"crowd_{size}", 3, _shuffled(b.rows, size), route="whole" if whole else list_route(size), listed=size, whole=whole)


def _ladder_case() -> Case:
    """Ladders of 2 .. 9 rungs 0.6e-8 apart in column 1: rung k joins rung k - 1 only where that one is a head."""
    b = _Builder(3, 8)
    for rungs in range(2, 10):
        _, e = b.anchor()
        for k in range(1, rungs):
            b.sat(e, {1: k * RUNG, 2: -k * RUNG})
    return Case("ladders", 3, _shuffled(b.rows, 29), listed=sum(range(2, 10)), bites=("predecessor",))


def _between_case() -> Case:
    """Inactive rows next to close pairs, G = 6; the pair A, B = A + 2 quarters differs first in column 3.
    between_shared:   X = A + 1 quarter in column 3 and 1e-7 away in column 4: sorts between them, close to neither — B stays a head;
    outside:          the same X at + 3 quarters: behind B — B joins A;
    other_pattern:    X between them in column 3, with an entry where the pair has none (column 1): behind both — B joins A;
    zero_behind:      the pair has no entry in column 4, BEHIND the deciding column, and X has one: between — B stays a head;
    below:            X = A - 1 quarter in column 3: in front of A — B joins A."""
    b = _Builder(6, 12)
    marks, far = {}, 40 * Q

    def trio(name, zeros, pair, x):
        i, e = b.anchor(zeros=zeros)
        marks[name] = (i, b.sat(e, pair), b.sat(e, x))

    trio("between_shared", (1,), {3: 2 * Q, 4: -2 * Q}, {3: Q, 4: far, 5: -far - Q})
    trio("outside", (1,), {3: 2 * Q, 4: -2 * Q}, {3: 3 * Q, 4: far, 5: -far - 3 * Q})
    trio("other_pattern", (1,), {3: 2 * Q, 4: -2 * Q}, {1: Q, 3: Q, 4: far, 5: -far - 2 * Q})
    trio("zero_behind", (1, 4), {3: 2 * Q, 5: -2 * Q}, {3: Q, 4: far, 5: -far - Q})
    trio("below", (1,), {3: 2 * Q, 4: -2 * Q}, {3: -Q, 4: far, 5: -far + Q})
    b.fill(4)
    return Case("between", 6, b.rows, listed=10, bites=("ignore_inactive",), marks=marks,
                order_columns={(marks[k][0], marks[k][1]): 3 for k in marks})


def _between_rows_case() -> Case:
    """The in-between pass at its edges, G = 4.  A list of 600 rows, so that its neighbour pairs are staged in three chunks of
    kPairChunk, with a triple A, A + 2, A + 3 quarters at list positions 255, 256, 257 — both of its neighbour pairs joinable, the
    last of one chunk and the first of the next — parted by the inactive rows X1 (+ 1 quarter in column 1, 1e-7 away in column 2)
    and X2 (+ 2.5 quarters, 1.5e-7 away), and the pair behind it parted by X3.  X1, X2 and X3 are rows 511, 512, 513 of the
    matrix (kBetweenRows = 512: the last row of one work item and the first two of the next); nothing merges around them."""
    b = _Builder(4, 310)
    marks, xs = {}, []
    pair, third = {1: 2 * Q, 2: -2 * Q}, {1: 3 * Q, 2: -3 * Q}
    _, e = b.anchor()                       # list positions 0, 1, 2
    b.sat(e, pair)
    b.sat(e, third)
    for k in range(1, 127):                 # pair k at list positions 2 k + 1, 2 k + 2
        _, e = b.anchor()
        b.sat(e, pair)
    i, e = b.anchor()                       # 255, 256, 257
    marks["triple"] = (i, b.sat(e, pair), b.sat(e, third))
    xs.append((e, {1: Q, 2: 40 * Q, 3: -41 * Q}))
    xs.append((e, {1: 5 * Q // 2, 2: 60 * Q, 3: -60 * Q - 5 * Q // 2}))
    i, e = b.anchor()                       # 258, 259
    marks["pair"] = (i, b.sat(e, pair))
    xs.append((e, {1: Q, 2: 40 * Q, 3: -41 * Q}))
    for k in range(129, 299):
        _, e = b.anchor()
        b.sat(e, pair)
    assert len(b.rows) == 600
    listed, b.rows = b.rows, []
    marks["between"] = tuple(BETWEEN_ROWS - 1 + k for k in range(3))
    for e, o in xs:
        b.sat(e, o)
    inbetween, b.rows = b.rows, []
    b.fill(5)
    place = {old: (old if old < BETWEEN_ROWS - 1 else old + 3) for old in range(600)}
    rows = listed[:BETWEEN_ROWS - 1] + inbetween + listed[BETWEEN_ROWS - 1:] + b.rows
    marks["triple"] = tuple(place[r] for r in marks["triple"])
    marks["pair"] = tuple(place[r] for r in marks["pair"])
    return Case("between_rows", 4, rows, route=list_route(600), listed=600, bites=("ignore_inactive",), marks=marks)


def _columns_case(G: int) -> Case:
    """Pairs that differ only in column 0, 7, 8, 63, 64 or G - 1 (a close and an apart pair each), only in the noise (close,
    apart), only in the count (bit-for-bit copies), and rows with a single entry (a close pair in column 0, an apart pair in
    column G - 1: 1 - noise there, the noises 2 and 5 quarters apart)."""
    b = _Builder(G, 40)
    marks, columns, order_columns = {}, {}, {}
    if G == 1:   # one column: the value IS 1 - noise — every pair differs in the noise and with it in column 0
        for name, d in (("noise_close", 2 * Q), ("noise_apart", 5 * Q)):
            i, e = b.anchor()
            noise = ONE - e[0]
            marks[name] = (i, b.add([e[0] - d], noise + d))
        i, e = b.anchor()
        marks["count"] = (i, b.add(e, ONE - e[0], 3))
        b.fill(2)
        return Case("columns_1", 1, b.rows, listed=2, marks=marks)
    deciding = [c for c in sorted({0, 7, 8, 63, 64, G - 1}) if c < G]
    for c in deciding:
        for name, units in (("close", CLOSE_IN), ("apart", APART_IN)):
            i, e = b.anchor()
            j = b.sat(e, _only_column(G, c, units))
            marks[f"{name}_{c}"] = (i, j)
            if G > 2:
                columns[(i, j)] = c
            else:   # two columns move together: the pair differs in both, column 0 orders it
                order_columns[(i, j)] = 0
    for name, d in (("noise_close", 2 * Q), ("noise_apart", 5 * Q)):
        i, e = b.anchor()
        marks[name] = (i, b.add(e, NOISE + d, sums_to_one=False))   # the entries as they are: the row's sum stays, 1 - noise moves
    i, e = b.anchor()
    marks["count"] = (i, b.add(e, NOISE, 3))
    for name, c, d in (("single_close", 0, 2 * Q), ("single_apart", G - 1, 5 * Q)):
        hot = [0] * G
        hot[c] = ONE - 2 * NOISE
        i = b.add(hot, 2 * NOISE)
        hot[c] -= d
        marks[name] = (i, b.add(hot, 2 * NOISE + d))
    b.fill(3)
    wide = any(c >= PATTERN_COLUMNS for c in deciding)
    return Case(f"columns_{G}", G, b.rows, listed=2 * len(deciding) + 4, bites=("no_wide_columns",) if wide else (), marks=marks, columns=columns,
                order_columns=order_columns)


def _ends_case() -> Case:
    """The close pair at rows 0 and R - 1 of the matrix."""
    b = _Builder(3, 70)
    _, e = b.anchor()
    b.fill(68)
    last = b.sat(e, {1: 2 * Q, 2: -2 * Q})
    return Case("ends", 3, b.rows, listed=2, marks={"pair": (0, last)})


SORTED_EDGES = (64, 512, 1024, 2048)


def _sorted_edges_case(stretch: bool) -> Case:
    """Runs across the sorted positions 63 | 64, 511 | 512, 1 023 | 1 024, 2 047 | 2 048 of a matrix of 2 100 rows: a close pair at
    e - 1 and e — or, with `stretch`, three bit-for-bit copies of the anchor at e - 2, e - 1, e and their close satellite at e + 1."""
    b = _Builder(3, 2100)
    marks = {}
    while len(b.rows) < 2100:
        at = len(b.rows)
        edge = next((e for e in SORTED_EDGES if at == (e - 2 if stretch else e - 1)), None)
        i, e = b.anchor()
        if edge is not None:
            copies = [b.add(e) for _ in range(2)] if stretch else []
            marks[f"edge_{edge}"] = (i, *copies, b.sat(e, {1: 2 * Q, 2: -2 * Q}))
    name = "sorted_edges_stretches" if stretch else "sorted_edges_pairs"
    order = np.random.default_rng(5 if stretch else 4).permutation(len(b.rows))
    place = {int(old): new for new, old in enumerate(order)}
    rows = [b.rows[int(old)] for old in order]
    marks = {k: tuple(place[r] for r in v) for k, v in marks.items()}
    return Case(name, 3, rows, listed=(4 if stretch else 2) * len(SORTED_EDGES), marks=marks)


def _rows_case(R: int) -> Case:
    """A matrix of R rows: a close pair on its first and on its last anchor, a ladder of three in the middle, an in-between trio
    (R >= 16), single rows otherwise."""
    if R == 1:
        b = _Builder(4, 1)
        b.anchor()
        return Case("rows_1", 4, b.rows, route="none", listed=0)
    b = _Builder(4, R)
    pair = {1: 2 * Q, 2: -2 * Q}
    _, e = b.anchor()
    b.sat(e, pair)
    bites, marks, listed = [], {}, 2
    if R >= 16:
        b.fill((R - 12) // 2)
        _, e = b.anchor()
        b.sat(e, {1: RUNG, 2: -RUNG})
        b.sat(e, {1: 2 * RUNG, 2: -2 * RUNG})
        i, e = b.anchor()
        marks["between"] = (i, b.sat(e, pair), b.sat(e, {1: Q, 2: 40 * Q, 3: -41 * Q}))
        bites, listed = ["predecessor", "ignore_inactive"], 9
        b.fill(R - len(b.rows) - 2)
        _, e = b.anchor()
        b.sat(e, pair)
    assert len(b.rows) == R
    return Case(f"rows_{R}", 4, _shuffled(b.rows, R) if R >= 16 else b.rows, listed=listed, bites=tuple(bites),
                marks={} if R >= 16 else marks)


def _empty_case() -> Case:
    return Case("no_rows", 2, [], route="none", listed=0)


def _rounding_case() -> Case:
    """Satellites one and two ulps from their anchor in one raw entry (the row's sum may move by an ulp with it, and then every
    column does): equal for the tolerant order, within the precision — the reference merges them, the device leaves such rows
    alone (kEquivalentRelative), 1e-13 relative at most from what the reference keeps."""
    b = _Builder(5, 8)
    raw = {}
    for ulps in (1, 2, -1, -2):
        _, e = b.anchor()
        j = b.add(e)
        raw[(j, 2)] = ulps
    b.fill(2)
    return Case("rounding_equal", 5, b.rows, kind="rounding", route="none", listed=0, raw=raw)


def _between_first_case() -> Case:
    """Three columns, the pair ordered by column 0 itself: A, B = A + 2 quarters there, and X = A + 1 quarter, 1e-7 away in
    column 1, between them — B stays a head; next to a pair that joins and a ladder of four."""
    b = _Builder(3, 8)
    marks = {}
    b.fill(1)
    i, e = b.anchor()
    marks["parted"] = (i, b.sat(e, {0: 2 * Q, 1: -2 * Q}), b.sat(e, {0: Q, 1: 40 * Q, 2: -41 * Q}))
    i, e = b.anchor()
    marks["joined"] = (i, b.sat(e, {0: 2 * Q, 1: -2 * Q}), b.sat(e, {0: 3 * Q, 1: 40 * Q, 2: -43 * Q}))
    _, e = b.anchor()
    for k in range(1, 4):
        b.sat(e, {1: k * RUNG, 2: -k * RUNG})
    b.fill(2)
    return Case("between_first_column", 3, b.rows, listed=8, bites=("predecessor", "ignore_inactive"), marks=marks,
                order_columns={(marks[k][0], marks[k][1]): 0 for k in marks})


# ---- the held-back stage: matrices from the batch's own columns, searched as built, their sums adjusted (adjustSearchSums) ----------

def _held_case(G: int, rewritten: int) -> Case:
    """`rewritten` rows take the values of their head (kStageRows = 32 staged at a time), G columns (G x G cells on kAdjustSlices = 16
    slices): close pairs, every third with its satellite in front; G = 1: pairs in the noise."""
    b = _Builder(G, rewritten + 4, level=True)
    b.fill(2)
    for k in range(rewritten):
        i, e = b.anchor()
        if G == 1:
            b.add([e[0] - 2 * Q], ONE - e[0] + 2 * Q)
        elif G == 2:
            b.sat(e, {0: 2 * Q, 1: -2 * Q})
        else:
            b.sat(e, {1: -2 * Q, 2: 2 * Q} if k % 3 == 2 else {1: 2 * Q, 2: -2 * Q})
    b.fill(2)
    return Case(f"held_{G}x{rewritten}", G, _shuffled(b.rows, 7 * G + rewritten), listed=2 * rewritten)


LOG1P_ROWS = 4


def _held_log1p_case() -> Case:
    """Rows whose first two columns are about 1e-5 and whose noise is 2e-6: a satellite 2 quarters (5e-9) off in column 1 moves
    the search's log arguments of the cells (0, 1), (1, 1) by 2e-4 to 4e-4 of themselves — the log1p branch of the adjustment
    (|x| >= 1e-4) — next to ordinary pairs, which take the series."""
    b = _Builder(3, 12, level=True)
    small, noise = 10995116, 2199023   # 1e-5, 2e-6
    marks = {"log1p": []}
    for k in range(LOG1P_ROWS):
        e = [small + k * (small // 10), small, 0]
        e[2] = ONE - noise - e[0] - e[1]
        i = b.add(e, noise, 1 + k)
        marks["log1p"].append((i, b.sat(e, {1: 2 * Q, 2: -2 * Q}, count=2, noise=noise)))
    marks["log1p"] = tuple(marks["log1p"])
    for k in range(5):
        _, e = b.anchor()
        b.sat(e, {1: 2 * Q, 2: -2 * Q})
    b.fill(2)
    return Case("held_log1p", 3, b.rows, listed=2 * LOG1P_ROWS + 10, marks=marks)


def _held_chunks_case() -> Case:
    """1 100 rows, all of count 1 (the matrix keeps the cluster's order): close pairs at rows 10 | 11, 1 023 | 1 024 — the last row of
    the tile kernel's first chunk of 1 024 and the first of its second — and 1 050 | 1 051."""
    b = _Builder(3, 1100, level=True)
    marks = {}
    while len(b.rows) < 1100:
        at = len(b.rows)
        i, e = b.anchor()
        if at in (10, SEARCH_CHUNK_ROWS - 1, 1050):
            marks[f"row_{at}"] = (i, b.sat(e, {1: 2 * Q, 2: -2 * Q}))
    return Case("held_chunks", 3, b.rows, listed=6, marks=marks)


def _em_cells_case() -> Case:
    """EM problems: a stretch of 40 rows that agree in their cells of 2^-44 but not bit for bit (one raw entry 0 .. 3 ulps up), their
    close satellite of count 60, and single rows."""
    b = _Builder(3, 12)
    raw = {}
    b.fill(3)
    i, e = b.anchor()
    # (the entries are multiples of 2^-40, on the edge of a cell: half a cell up first)
    half = [int(2.0 ** -45 / np.spacing(v * U)) for v in e]
    for k in range(40):
        j = b.add(e, count=1 + k % 3) if k else i
        for c in range(3):
            raw[(j, c)] = half[c] + (k % 4 if c == 1 else 0)
    b.sat(e, {1: 2 * Q, 2: -2 * Q}, count=60)
    b.fill(3)
    return Case("cells", 3, b.rows, kind="rounding", route="none", listed=0, raw=raw)


def _em_variant(case: Case, count: int = None) -> Case:
    """The case as an EM problem whose merges show in the abundances: every other anchor, with its satellites, has its columns 1
    and 2 exchanged (so both paths keep an abundance: as planted, column 2 is every row's largest and takes all of it), the
    rows that join a head get `count` reads, and the lighter of the two halves has its counts multiplied up to the other's."""
    assert case.G == 3
    col0 = sorted((e[0], r) for r, (e, _, _) in enumerate(case.rows))
    group, g = {}, 0
    for k, (v, r) in enumerate(col0):
        if k and v - col0[k - 1][0] > ONE // 10 ** 5:
            g += 1
        group[r] = g
    head = collapse_heads(*build_matrix(case.cluster(), case.G))
    rows, raw = [], {}
    for r, (e, z, c) in enumerate(case.rows):
        swap = group[r] % 2 == 1
        rows.append(([e[0], e[2], e[1]] if swap else list(e), z, count if count and head[r] != r else c))
        for col in range(3):
            if (r, col) in case.raw:
                raw[(r, (3 - col) if swap and col else col)] = case.raw[(r, col)]
    weight = [sum(c for r, (_, _, c) in enumerate(rows) if group[r] % 2 == half) for half in (0, 1)]
    light = 0 if weight[0] < weight[1] else 1
    factor = max(1, round(weight[1 - light] / weight[light]))
    rows = [(e, z, c * factor if group[r] % 2 == light else c) for r, (e, z, c) in enumerate(rows)]
    return Case("em_" + case.name, 3, rows, kind=case.kind, route=case.route, listed=case.listed, whole=case.whole, bites=case.bites, raw=raw)


LIST_SIZES = (2, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049)
CROWD_SIZES = (MAX_WINDOW_COMPARES + 1, MAX_WINDOW_COMPARES + 2)   # 256 and 257 candidates of the crowd's lowest row
COLUMN_COUNTS = (1, 2, 8, 9, 63, 64, 65, 70)
ROW_COUNTS = (1, 2, 512, 513, 1024, 1025, 2048, 2049, 4097)


def _build_cases() -> List[Case]:
    cases = [_list_case(n) for n in LIST_SIZES]
    cases += [_crowd_case(n) for n in CROWD_SIZES]
    cases += [_ladder_case(), _between_case(), _between_first_case(), _between_rows_case()]
    cases += [_columns_case(G) for G in COLUMN_COUNTS]
    cases += [_ends_case(), _sorted_edges_case(False), _sorted_edges_case(True)]
    cases += [_rows_case(R) for R in ROW_COUNTS[:3]] + [_empty_case()] + [_rows_case(R) for R in ROW_COUNTS[3:]]
    cases += [_rounding_case()]
    return cases


CASES: List[Case] = _build_cases()
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
TWICE = "between"   # the cluster that the joint call lists a second time

HELD_SHAPES = ((3, 31), (4, 32), (5, 33), (1, 3))   # (columns, rewritten rows)
HELD_CASES: List[Case] = [_held_case(G, n) for G, n in HELD_SHAPES] + [_held_log1p_case(), _held_chunks_case()]
EM_CASES: List[Case] = [_em_variant(BY_NAME["ladders"], 7), _em_variant(BY_NAME["between_first_column"], 9),
                        _em_variant(BY_NAME[f"crowd_{CROWD_SIZES[1]}"], 3), _em_variant(_em_cells_case())]
for _c in HELD_CASES + EM_CASES:
    assert _c.name not in BY_NAME
    BY_NAME[_c.name] = _c


def joint_listing() -> List[int]:
    """The clusters of the joint call: every case with rows once, in table order, and TWICE again at the end.  (The cluster
    without rows is in the batch, between the others; a matrix on it is refused by the build: planGroupBuild, "no rows or no
    columns".)"""
    return [k for k, c in enumerate(CASES) if c.R] + [[c.name for c in CASES].index(TWICE)]


def batch_of(cases: Sequence[Case]):
    from rpvg_amd.batch import ClusterBatch
    return ClusterBatch.from_clusters([c.cluster() for c in cases])


# ---- conditions ---------------------------------------------------------------------------------------------------------------------

def column_gaps(P: np.ndarray) -> float:
    """Condition (a): the smallest relative distance between two values of one column that are not bit-identical."""
    worst = float("inf")
    for c in range(P.shape[1]):
        v = np.unique(P[:, c])
        v = v[v != 0]
        if len(v) > 1:
            worst = min(worst, float(np.min((v[1:] - v[:-1]) / v[:-1])))
    return worst


def pair_distance_gap(P: np.ndarray) -> Tuple[float, float]:
    """Condition (b): (largest pair distance below the precision, smallest at or above it), a pair's distance being its largest
    column distance.  Pairs further apart than 1e-6 in column 0 are apart."""
    order = np.argsort(P[:, 0], kind="stable")
    S = P[order]
    hi = np.searchsorted(S[:, 0], S[:, 0] + 1e-6, side="right")
    below, above = 0.0, float("inf")
    for i in range(len(S)):
        if hi[i] > i + 1:
            d = np.max(np.abs(S[i + 1:hi[i]] - S[i]), axis=1)
            if np.any(d < PRECISION):
                below = max(below, float(d[d < PRECISION].max()))
            if np.any(d >= PRECISION):
                above = min(above, float(d[d >= PRECISION].min()))
    return below, above


def first_differing_column(P: np.ndarray, a: int, b: int) -> int:
    for c in range(P.shape[1]):
        if not tolerant_equal(float(P[a, c]), float(P[b, c])):
            return c
    return -1


def deciding_column(P: np.ndarray, a: int, b: int) -> int:
    """The column a pair "differs only in": the one column at or above the precision, else the column of the largest distance."""
    d = np.abs(P[a] - P[b])
    apart = np.flatnonzero(d >= PRECISION)
    if len(apart):
        return int(apart[0]) if len(apart) == 1 else -1
    return int(np.argmax(d))
