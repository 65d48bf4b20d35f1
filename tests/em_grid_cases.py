"""EM problems at the edges of the whole-GPU EM routes (test-only; numpy, no GPU).

With RPVG_HIP_EM_GRID_MIN_WORK=1 every problem of an rpvg_hip_em_solve call takes the grid bin (rpvg_amd/csrc/em_grid.hip):
its CSR route (emGridAccumKernel<LANES,4> + emGridUpdateKernel) or, when emDenseRule holds, a dense copy and the streaming
kernels of em_dense.hip.  Which kernel variant runs, over how many workgroups, with which strides, is planEmGridCsr /
planEmDense (rpvg_amd/csrc/em_plan.hpp).  This module

  * restates those plans in Python (csr_launch_shape, dense_launch_shape, dense_rule; tests/test_em_grid_cases.py holds them
    to the C++ for every case shape),
  * holds a model of the EM in np.longdouble (EmModel): the reference's start vector 1 / float(C) widened, the read counts of
    the rows without a selected path (Z) on the noise column, the 10-consecutive stop rule, the 1e-8 epilogue, and the
    smallest relative gap of any comparison that decided an iteration's verdict,
  * and builds one small problem for every place where that code changes shape, chosen by the restatement at 256 CUs.

The tolerance of the GPU tests (KERNEL_REL) is not chosen: it is 64 x the largest distance of the double-precision oracle
(pyoracle.em_dense, same inputs) from the long-double model over this table — ORACLE_DISTANCE below, measured on the CPU and
re-measured by tests/test_em_grid_cases.py.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import np_oracle
from tests import em_bin_cases as ebc
from tests.em_bin_cases import Cluster, make_cluster

CUS = 256                 # the case table is chosen at this many CUs (MI355X)
MIN_EM_ABUNDANCE = 1e-8   # src/path_abundance_estimator.cpp:11
MIN_EM_CONV_ITS = 10      # src/path_abundance_estimator.cpp:10
COLLAPSE_PRECISION = 1e-8

# ---- the plans restated (em_plan.hpp: emGridRowLanes, planEmGridCsr, planEmDense, emDenseRule) ---------------------------
GRID_BLOCK = 256          # kEmGridBlock
GRID_UNROLL = 4           # kEmGridUnroll
UPDATE_COLUMNS = 16       # kEmGridUpdateColumns
UPDATE_SLICES = 64        # kEmGridUpdateBlock / kEmGridUpdateColumns
DENSE_CHUNK_ITS = 8       # kEmDenseChunkIts
DENSE_REDUCE_SLICES = 16  # kEmDenseReduceSlices
DENSE_MAX_COLS = ebc.DENSE_MAX_COLS

dense_rule = ebc.dense_rule


def row_lanes(rows: int, entries: int) -> int:
    mean = float(entries) / float(max(1, rows))
    return 1 if mean < 6.0 else 4 if mean < 24.0 else 16 if mean < 96.0 else 64


def csr_launch_shape(C: int, rows: int, entries: int, cus: int = CUS) -> Dict[str, int]:
    """planEmGridCsr without knobs."""
    lanes = row_lanes(rows, entries)
    csr_bytes = 12 * entries + 20 * rows
    slots = GRID_BLOCK // lanes
    blocks = -(-rows // slots)
    blocks = min(blocks, cus * (2 if lanes == 1 else 4))
    blocks = min(blocks, max(16, csr_bytes // (16 * C)))
    blocks = max(1, min(blocks, rows))
    rows_per_block = -(-rows // blocks)
    iteration_us = float(csr_bytes) / 4.0e6 + 8.0
    return dict(lanes=lanes, grid=-(-rows // rows_per_block), rows_per_block=rows_per_block, partial_ld=(C + 63) & ~63,
                update_grid=-(-C // UPDATE_COLUMNS), lds=8 * 5 * C, chunk_its=int(min(32.0, max(4.0, 500.0 / iteration_us))))


def dense_launch_shape(C: int, rows: int, cus: int = CUS) -> Dict[str, int]:
    """planEmDense without knobs."""
    wide = C > 256
    per_trip = 2 if wide else 4
    grid = max(1, min(-(-rows // per_trip), cus * (4 if wide else 2)))
    return dict(wide=int(wide), nchunk=-(-C // 512) if wide else -(-C // 128), grid=grid,
                partial_ld=-(-C // 512) * 512 if wide else (C + 1) & ~1, reduce_slices=DENSE_REDUCE_SLICES if wide else 0,
                chunk_its=DENSE_CHUNK_ITS)


def block_rows(shape: Dict[str, int], rows: int) -> List[int]:
    """Rows of every workgroup of the CSR pass."""
    rpb = shape["rows_per_block"]
    return [min(rows, (b + 1) * rpb) - b * rpb for b in range(shape["grid"])]


# ---- the model -------------------------------------------------------------------------------------------------------
LD = np.longdouble


@dataclass
class ModelResult:
    abundances: np.ndarray     # longdouble [C - 1]: expected read counts, 0 where the model's abundance is below 1e-8
    live: np.ndarray           # bool [C - 1]: the model's abundance is at least 1e-8
    noise_count: LD
    total: LD
    iterations: int
    gap: float                 # smallest relative gap of a comparison that decided an iteration's verdict (inf: none made)


class EmModel:
    """The reference's EM (src/path_abundance_estimator.cpp:47-114) in long double on a normalised dense matrix (last column:
    noise).  Rows without a path entry put their read count Z on the noise column (they multiply out to exactly that); the
    iterates are kept, so one trajectory serves every budget and both stop rules."""

    def __init__(self, Pn: np.ndarray, counts: np.ndarray):
        Pn = np.asarray(Pn, dtype=np.float64)
        counts = np.asarray(counts, dtype=np.float64)
        keep = (Pn[:, :-1] != 0).any(axis=1)
        self.C = Pn.shape[1]
        self.total = LD(counts.sum())
        self.Z = LD(counts[~keep].sum())
        K = Pn[keep]
        self.count = counts[keep].astype(LD)
        r, c = np.nonzero(K)               # row-major: sorted by row
        self.val = K[r, c].astype(LD)
        self.col = c
        self.row_start = np.searchsorted(r, np.arange(K.shape[0]))
        assert K.shape[0] == 0 or np.all(np.diff(np.concatenate([self.row_start, [len(r)]])) > 0)   # noise or a path in every row
        self.row_of = r
        order = np.argsort(c, kind="stable")
        self.by_col = order
        self.col_start = np.searchsorted(c[order], np.arange(self.C))
        self.col_empty = np.diff(np.concatenate([self.col_start, [len(c)]])) == 0
        self.iterates = [np.full(self.C, LD(np.float64(np.float32(1) / np.float32(self.C))))]

    def _reduce(self, x, starts, empty):
        if len(x) == 0:
            return np.zeros(len(starts), dtype=LD)
        out = np.add.reduceat(x, np.minimum(starts, len(x) - 1))
        out[empty] = 0
        return out

    def iterate(self, n: int) -> np.ndarray:
        """The abundances after n iterations."""
        while len(self.iterates) <= n:
            a = self.iterates[-1]
            s = self._reduce(self.val * a[self.col], self.row_start, np.zeros(len(self.row_start), dtype=bool))
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(self.count != 0, self.count / s, LD(0))
            t = self._reduce((w[self.row_of] * self.val)[self.by_col], self.col_start, self.col_empty)
            an = a * t
            an[-1] += self.Z
            self.iterates.append(an / self.total)
        return self.iterates[n]

    def run(self, max_em_its: int = 10000, max_rel_em_conv: float = 1e-3) -> ModelResult:
        conv, gap, its = 0, float("inf"), 0
        for it in range(1, max_em_its + 1):
            its = it
            prev, an = self.iterate(it - 1), self.iterate(it)
            live = an >= MIN_EM_ABUNDANCE
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(an > 0, np.abs(an - prev) / an, LD(0))
            over = rel > max_rel_em_conv
            viol = live & over
            if max_rel_em_conv > 0:
                live_gap = np.abs(an - MIN_EM_ABUNDANCE) / MIN_EM_ABUNDANCE
                rel_gap = np.abs(rel - max_rel_em_conv) / max_rel_em_conv
                if viol.any():   # the verdict stands while one violator stands
                    gap = min(gap, float(np.max(np.minimum(live_gap[viol], rel_gap[viol]))))
                else:            # every live component's comparison counts, and the life of a dead one that would violate
                    if live.any():
                        gap = min(gap, float(np.min(rel_gap[live])))
                    if (~live & over).any():
                        gap = min(gap, float(np.min(live_gap[~live & over])))
            if viol.any():
                conv = 0
            else:
                conv += 1
                if conv == MIN_EM_CONV_ITS:
                    break
        a = self.iterate(its)
        live = a[:-1] >= MIN_EM_ABUNDANCE
        # the epilogue's comparison decides where a component is reported
        gap = min(gap, float(np.min(np.abs(a[:-1] - MIN_EM_ABUNDANCE) / MIN_EM_ABUNDANCE)))
        return ModelResult(abundances=np.where(live, a[:-1] * self.total, LD(0)), live=live,
                           noise_count=a[-1] * self.total + (a[:-1][~live] * self.total).sum(), total=self.total, iterations=its, gap=gap)


def distance(abundances, noise_count, model: ModelResult) -> float:
    """The relative distance of a double-precision result from the model: the maximum over the components the model keeps
    (abundance >= 1e-8) and the noise count — which carries the components below (relative to the read total: a noise count
    may be far smaller than what is moved in and out of it)."""
    ab = np.asarray(abundances).astype(LD)
    d = 0.0
    if model.live.any():
        d = float(np.max(np.abs(ab[model.live] - model.abundances[model.live]) / model.abundances[model.live]))
    return max(d, float(abs(LD(noise_count) - model.noise_count) / model.total))


# ---- clusters --------------------------------------------------------------------------------------------------------
def concat_clusters(seed: int, parts: Sequence[Cluster]) -> Cluster:
    """The rows of several clusters over the same paths, shuffled together."""
    n_paths = parts[0].n_paths
    assert all(p.n_paths == n_paths for p in parts)
    counts = np.concatenate([p.count for p in parts])
    noise = np.concatenate([p.noise for p in parts])
    k = np.concatenate([np.diff(p.ent_off.astype(np.int64)) for p in parts])
    starts = np.concatenate([[0], np.cumsum(k)])[:-1]
    path = np.concatenate([p.ent_path for p in parts])
    prob = np.concatenate([p.ent_prob for p in parts])
    order = np.random.default_rng(seed).permutation(len(counts))
    take = np.concatenate([np.arange(starts[i], starts[i] + k[i]) for i in order]) if len(order) else np.zeros(0, dtype=np.int64)
    return Cluster(n_paths=n_paths, count=counts[order], noise=noise[order], ent_off=np.concatenate([[0], np.cumsum(k[order])]).astype(np.uint64),
                   ent_path=path[take].astype(np.uint32), ent_prob=prob[take].astype(np.float64))


def with_duplicates(seed: int, base: Cluster, copies: int) -> Cluster:
    """`copies` rows of the cluster once more, bit for bit, with read counts of their own: what a row collapse merges (the count
    goes to the run's first row, the others stay with count 0)."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(base.count), size=copies, replace=True)   # (a row may be copied several times: runs of three and more)
    off = base.ent_off.astype(np.int64)
    dup = Cluster(n_paths=base.n_paths, count=rng.integers(1, 9, size=copies).astype(np.uint32), noise=base.noise[rows],
                  ent_off=np.concatenate([[0], np.cumsum(off[rows + 1] - off[rows])]).astype(np.uint64),
                  ent_path=np.concatenate([base.ent_path[off[r]:off[r + 1]] for r in rows]),
                  ent_prob=np.concatenate([base.ent_prob[off[r]:off[r + 1]] for r in rows]))
    return concat_clusters(seed + 1, [base, dup])


# ---- the table -------------------------------------------------------------------------------------------------------
@dataclass
class EmGridCase:
    name: str
    route: str                   # "csr" | "dense": what the restatement must say at CUS
    build: object                # () -> Cluster
    columns: Optional[object] = None   # None: every path of the cluster; else () -> sorted path list
    max_em_its: int = 10000      # the cap of the run to convergence (a large case: capped, so that the suite stays quick)
    collapse: bool = False       # solved with collapse_precision = COLLAPSE_PRECISION
    tags: Tuple[str, ...] = ()
    _cluster: Optional[Cluster] = field(default=None, repr=False)
    _shape: Optional[Tuple[int, int, int]] = field(default=None, repr=False)
    _inputs: Optional[tuple] = field(default=None, repr=False)
    _model: Optional[EmModel] = field(default=None, repr=False)

    def cluster(self) -> Cluster:
        if self._cluster is None:
            self._cluster = self.build()
        return self._cluster

    def cols(self) -> List[int]:
        return list(range(self.cluster().n_paths)) if self.columns is None else list(self.columns())

    def shape(self) -> Tuple[int, int, int]:
        """(C, kept rows, kept entries) of the problem, counted from its rows (a row collapse keeps every row: a merged
        row stays with count 0)."""
        if self._shape is None:
            rows, entries = self.cluster().kept(None if self.columns is None else self.cols())
            self._shape = (len(self.cols()) + 1, rows, entries)
        return self._shape

    def collapse_precision(self) -> float:
        return COLLAPSE_PRECISION if self.collapse else 0.0

    def inputs(self) -> Tuple[np.ndarray, np.ndarray]:
        """The normalised dense matrix (last column: noise) and the read counts the reference's EM gets."""
        if self._inputs is None:
            cl = self.cluster()
            P, noise, counts = np_oracle.dense_matrix(cl.rows(), cl.n_paths, self.cols())
            Pn = np_oracle.add_noise_and_normalize(P, noise)
            if self.collapse:
                Pn, counts = np_oracle.read_collapse(Pn, counts, COLLAPSE_PRECISION)
            self._inputs = (Pn, counts)
        return self._inputs

    def model(self) -> EmModel:
        if self._model is None:
            self._model = EmModel(*self.inputs())
        return self._model

    def zero_mass(self) -> float:
        return float(self.model().Z)

    def launch_shape(self, cus: int = CUS) -> Dict[str, int]:
        s = self.shape()
        return dense_launch_shape(s[0], s[1], cus) if dense_rule(*s) else csr_launch_shape(*s, cus)


FIXED_BUDGET = 12                                  # the budget of every case (max_rel_em_conv = 0)
CHUNK_BUDGETS = (1, 7, 8, 9, 31, 32, 33, 64, 65)   # both chunk sizes (8 dense, 32 CSR) and two chunks in flight
BUDGET_CASES = ("csr_lanes16_lo", "dense_c128")    # a representative case of each route
HEAVY_CAP = 40                                     # max_em_its of the cases of 10^5 entries and more


def _case(name, route, seed, n_paths, rows, entries=None, tags=(), max_em_its=10000, collapse=False, full=False, **kw):
    if full:   # every row holds every path
        kw.setdefault("pool", list(range(n_paths)))
        kw["most"], entries = n_paths, rows * n_paths
    return EmGridCase(name, route, lambda: make_cluster(seed, n_paths, rows, entries, **kw), None, max_em_its, collapse, tuple(tags))


def _subset_case(name, route, seed, n_paths, chosen, kept, entries, dropped, tags=(), **kw):
    """A problem over `chosen` of the cluster's paths; `kept` rows touch chosen paths only, `dropped` rows only paths outside
    them: their read counts are the problem's zero mass."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(n_paths, size=chosen, replace=False))
    rest = np.setdiff1d(np.arange(n_paths), cols)
    return EmGridCase(name, route, lambda: make_cluster(seed, n_paths, kept, entries, pool=cols, dropped_rows=dropped, other=rest, **kw),
                      lambda: [int(x) for x in cols], 10000, False, tuple(tags))


def _mixed_case(name, route, seed, n_paths, parts, tags=()):
    """Rows of several kinds over the same paths: parts = [(rows, entries per row), ...]"""
    return EmGridCase(name, route, lambda: concat_clusters(seed, [make_cluster(seed + 10 * (i + 1), n_paths, r, r * k, most=k)
                                                                  for i, (r, k) in enumerate(parts)]), None, 10000, False, tuple(tags))


def _collapsed_case(name, route, seed, n_paths, rows, entries, copies, tags=(), **kw):
    return EmGridCase(name, route, lambda: with_duplicates(seed + 5, make_cluster(seed, n_paths, rows, entries, **kw), copies), None, 10000, True,
                      tuple(tags))


def _cases() -> List[EmGridCase]:
    c: List[EmGridCase] = []
    # CSR, lanes: the mean row length on both sides of 6, 24 and 96 (one entry apart); C wide enough that emDenseRule is false
    c.append(_case("csr_lanes1_hi", "csr", 101, 39, 1000, 5999, most=12))
    c.append(_case("csr_lanes4_lo", "csr", 102, 39, 1000, 6000, most=12))
    c.append(_case("csr_lanes4_hi", "csr", 103, 69, 500, 11999, most=40))
    c.append(_case("csr_lanes16_lo", "csr", 104, 69, 500, 12000, most=40))
    c.append(_case("csr_lanes16_hi", "csr", 105, 159, 300, 28799, most=150))
    c.append(_case("csr_lanes64_lo", "csr", 106, 159, 300, 28800, most=150))
    # CSR, rows and blocks: one workgroup of 1, 3, 255, 256 rows; 257 rows in two workgroups
    for rows in (1, 3, 255, 256, 257):
        c.append(_case(f"csr_rows{rows}", "csr", 110 + rows, 19, rows, 2 * rows))
    # ... a last workgroup of one row (65 rows under 64 lanes: 16 workgroups of 4 and one of 1), a remainder (100 rows under
    # 16 lanes: 6 workgroups of 15 and one of 10)
    c.append(_case("csr_last_block_1", "csr", 120, 199, 65, 65 * 100, most=100))
    c.append(_case("csr_remainder_l16", "csr", 121, 99, 100, 3000, most=30))
    # ... a workgroup's rows against the rows it holds at once (256 / LANES) and walks per trip (4 x 256 / LANES):
    # 282 rows under 1 lane (a second row for 26 slots), 70 under 4 lanes, 25 and 75 under 64 lanes (second and fifth trip)
    c.append(_case("csr_trips_l1", "csr", 122, 799, 4500, 9000, most=3))
    c.append(_case("csr_trips_l4", "csr", 123, 999, 1120, 11200, most=10))
    c.append(_case("csr_trips_l16", "csr", 124, 1499, 640, 19200, most=30))
    c.append(_case("csr_trips_l64", "csr", 125, 2999, 400, 38400, most=96))
    c.append(_case("csr_long_trips_l64", "csr", 126, 3599, 1200, 115200, most=96, max_em_its=HEAVY_CAP))
    # CSR, mixed rows: one-entry rows among 300-entry rows under 64 lanes; one 200-entry row under 1 lane
    c.append(_mixed_case("csr_mixed_l64", "csr", 130, 320, [(200, 1), (200, 300)]))
    c.append(_mixed_case("csr_mixed_l1", "csr", 131, 259, [(1000, 2), (1, 200)]))
    # CSR, columns (C = paths + 1) at the update kernel's 16 columns and the partials' stride of 64; C = 2 can only be dense
    for C in (15, 16, 17, 63, 64, 65):
        c.append(_case(f"csr_cols{C}", "csr", 140 + C, C - 1, 300, 600, tags=("columns",)))
    c.append(_case("dense_cols2", "dense", 142, 1, 300, 300, pool=[0], tags=("columns",)))
    # CSR, partial counts: 64 n - 5 rows under 4 lanes, 16 n - 3 under 16, 4 n - 1 under 64: n workgroups
    for n in (63, 64, 65):
        c.append(_case(f"csr_partials{n}", "csr", 150 + n, 32, 64 * n - 5, 10 * (64 * n - 5), most=20, tags=("partials",)))
    for n in (192, 193):
        c.append(_case(f"csr_partials{n}", "csr", 150 + n, 99, 16 * n - 3, 30 * (16 * n - 3), most=60, tags=("partials",), max_em_its=HEAVY_CAP))
    for n in (256, 257):
        c.append(_case(f"csr_partials{n}", "csr", 150 + n, 159, 4 * n - 1, 96 * (4 * n - 1), most=96, tags=("partials",), max_em_its=HEAVY_CAP))
    # ... and the caps: 4 per CU under 64 lanes (5 117 rows of 96 entries: 1 024 workgroups of 5 rows, the last of 2), 2 per CU
    # under 1 lane — 512 workgroups of 256 rows and more, the one case beyond 5 000 rows: nothing smaller reaches that cap
    c.append(_case("csr_cap_l64", "csr", 160, 199, 5117, 96 * 5117, most=96, tags=("partials",), max_em_its=HEAVY_CAP))
    c.append(_case("csr_cap_l1", "csr", 161, 8, 131372, 2 * 131372, most=3, tags=("partials",), max_em_its=HEAVY_CAP))
    # dense route through em_solve: the narrow kernel's one | two chunks, narrow | wide, the widest row; 2049 columns: CSR
    c.append(_case("dense_c128", "dense", 170, 127, 301, full=True))
    c.append(_case("dense_c129", "dense", 171, 128, 301, full=True))
    c.append(_case("dense_c256", "dense", 172, 255, 601, full=True, max_em_its=HEAVY_CAP))
    c.append(_case("dense_c257", "dense", 173, 256, 601, full=True, max_em_its=HEAVY_CAP))
    c.append(_case("dense_c2048", "dense", 174, 2047, 201, full=True, max_em_its=HEAVY_CAP))
    c.append(_case("csr_c2049", "csr", 175, 2048, 201, full=True, max_em_its=HEAVY_CAP))
    # zero mass: path-less rows, and a column subset with rows that touch none of it
    c.append(_case("csr_pathless", "csr", 180, 39, 700, 2100, most=6, noise_only_rows=37, tags=("zero_mass",)))
    c.append(_case("dense_pathless", "dense", 181, 3, 700, 1400, pool=[0, 1, 2], noise_only_rows=37, tags=("zero_mass",)))
    c.append(_subset_case("csr_subset", "csr", 182, 60, 25, 900, 1795, 400, tags=("zero_mass",)))
    c.append(_subset_case("dense_subset", "dense", 183, 40, 3, 900, 1795, 400, tags=("zero_mass",)))
    # collapsed problems: rows once more with counts of their own
    c.append(_collapsed_case("csr_collapsed", "csr", 290, 29, 500, 1500, 300, most=5, tags=("collapsed",)))
    c.append(_collapsed_case("dense_collapsed", "dense", 191, 3, 500, 1000, 300, pool=[0, 1, 2], tags=("collapsed",)))
    # a count of a million next to counts of 1
    c.append(_case("csr_big_count", "csr", 195, 39, 800, 2400, most=6, big_count=True, max_count=1, tags=("counts",)))
    c.append(_case("dense_big_count", "dense", 196, 3, 800, 1600, pool=[0, 1, 2], big_count=True, max_count=1, tags=("counts",)))
    return c


CASES: List[EmGridCase] = _cases()
BY_NAME: Dict[str, EmGridCase] = {c.name: c for c in CASES}

# ---- the tolerance -----------------------------------------------------------------------------------------------------
# distance() of the double-precision oracle (pyoracle.em_dense on the case's inputs) from the model, per case: the largest over
# the fixed budget (and the chunk budgets of BUDGET_CASES) with max_rel_em_conv = 0 and the run to convergence (or to the case's
# cap); measured on the CPU, rounded up to two digits, re-measured by tests/test_em_grid_cases.py.
ORACLE_DISTANCE: Dict[str, float] = {
    "csr_lanes1_hi": 4.6e-15, "csr_lanes4_lo": 2.9e-15, "csr_lanes4_hi": 2.0e-15, "csr_lanes16_lo": 4.8e-15,
    "csr_lanes16_hi": 4.3e-15, "csr_lanes64_lo": 2.1e-15, "csr_rows1": 7.4e-16, "csr_rows3": 9.9e-16,
    "csr_rows255": 8.1e-16, "csr_rows256": 1.5e-15, "csr_rows257": 6.6e-16, "csr_last_block_1": 2.2e-15,
    "csr_remainder_l16": 2.0e-15, "csr_trips_l1": 1.8e-14, "csr_trips_l4": 2.8e-15, "csr_trips_l16": 2.2e-15,
    "csr_trips_l64": 8.2e-16, "csr_long_trips_l64": 2.2e-14, "csr_mixed_l64": 3.9e-15, "csr_mixed_l1": 2.7e-15,
    "csr_cols15": 3.0e-15, "csr_cols16": 9.1e-16, "csr_cols17": 1.9e-15, "csr_cols63": 1.1e-15, "csr_cols64": 1.6e-15,
    "csr_cols65": 2.1e-15, "dense_cols2": 7.0e-16, "csr_partials63": 8.3e-15, "csr_partials64": 1.9e-14,
    "csr_partials65": 7.3e-15, "csr_partials192": 1.7e-14, "csr_partials193": 6.8e-15, "csr_partials256": 6.9e-15,
    "csr_partials257": 5.7e-15, "csr_cap_l64": 1.3e-14, "csr_cap_l1": 2.0e-14, "dense_c128": 4.8e-15,
    "dense_c129": 2.2e-15, "dense_c256": 8.1e-15, "dense_c257": 2.3e-15, "dense_c2048": 2.6e-15, "csr_c2049": 5.2e-15,
    "csr_pathless": 2.2e-15, "dense_pathless": 7.6e-16, "csr_subset": 2.2e-15, "dense_subset": 1.9e-15,
    "csr_collapsed": 1.5e-15, "dense_collapsed": 1.2e-15, "csr_big_count": 7.4e-16, "dense_big_count": 8.1e-16,
}
MAX_ORACLE_DISTANCE = 2.2e-14                 # max(ORACLE_DISTANCE.values()): csr_long_trips_l64
# The kernels' bound: 64 x the oracle's own distance — room for the reciprocal-plus-Newton quotient, the FMA contractions and
# up to 1 024 partial vectors added in another order; five orders of magnitude below the 1e-7 of the tests at full size.
KERNEL_REL = 64 * MAX_ORACLE_DISTANCE         # 1.408e-12


# ---- matrices of the raw dense ABI (rpvg_hip_em_dense) ----------------------------------------------------------------
RAW_COLUMNS = (2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048)
RAW_ROWS = (1, 2, 3, 4, 5, 31)
RAW_CAP_ROWS = (2047, 2048, 2049)             # the grid cap of both kernels (512 x 4 and 1 024 x 2 rows) - 1, + 0, + 1
RAW_CAP_COLUMNS = (256, 257, 2048)


def raw_dense_problem(seed: int, R: int, C: int) -> Tuple[np.ndarray, np.ndarray]:
    """A normalised R x C matrix (last column: noise, positive) with about half its path cells exactly zero (a row keeps at
    least one), read counts with zeros and one of 10^6."""
    rng = np.random.default_rng(seed)
    noise = rng.uniform(1e-4, 0.3, size=R)
    W = rng.lognormal(0.0, 1.0, size=(R, C - 1)) * (rng.random((R, C - 1)) < 0.5)
    for i in np.nonzero(W.sum(axis=1) == 0)[0]:
        W[i, rng.integers(0, C - 1)] = 1.0
    P = W / W.sum(axis=1, keepdims=True) * (1.0 - noise)[:, None]
    counts = rng.integers(1, 9, size=R).astype(np.float64)
    if R >= 4:
        counts[rng.choice(R, size=max(1, R // 8), replace=False)] = 0.0
    counts[rng.choice(np.nonzero(counts)[0])] = 1_000_000.0
    return np.concatenate([P, noise[:, None]], axis=1), counts


def padded(Pn: np.ndarray, ld: int) -> np.ndarray:
    """The matrix with `ld` doubles per row, every padding cell NaN."""
    out = np.full((Pn.shape[0], ld), np.nan)
    out[:, :Pn.shape[1]] = Pn
    return out
