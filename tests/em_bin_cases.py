"""EM problems on both sides of every size-bin edge of rpvg_hip_em_solve (test-only; numpy, no GPU).

rpvg_hip_em_solve gives every problem one of twelve kernel variants by its columns C (paths + noise), kept rows and kept
entries alone (emBinOf, rpvg_amd/csrc/em_sparse.hip).  This module restates that rule in Python (em_bin, routes) and builds
one problem on each side of every edge: the register bins at C = 16/17 and 32/33 and rows = 64/65, 128/129, 256/257, the
LDS byte limits of the resident bins, the streamed bins at C = 1173/1174 and 3992/3993, the grid bin at rows + entries =
2^18 on its CSR and its dense sub-route and at its LDS cut (C = 3993/3994), the move of a few mid-size problems to the grid
(8 against 9 of them, and the 2^16 - 1 work line), column subsets whose kept rows sit on a register edge, and the column
maps of the fill kernel (clusters of 16 384 and 16 385 paths).

Rows follow the invariants of ReadPathProbabilities (src/read_path_probabilities.cpp:184,212-219): probabilities already
multiplied by (1 - noise), at least prob_precision, ascending inside a row, one path per (probability, path) group.  The
noise of the kept rows of a cluster is pairwise farther apart than prob_precision, so no two normalised rows are within
prob_precision of each other: what a problem keeps is exactly the rows and entries the case built.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from rpvg_amd.batch import ClusterBatch

PROB_PRECISION = 1e-8

# ---- the rule (emLdsBytes, emGridLdsBytes, emBinOf, emDenseRule, emOrderKernel / accountEmSolve) -------------------------
LDS_LIMIT = 156 * 1024          # kEmLdsLimit
GRID_MIN_WORK = 1 << 18         # emGridMinWork() without RPVG_HIP_EM_GRID_MIN_WORK
MID_GRID_MAX = 8                # kEmMidGridMax
MID_GRID_MIN_WORK = (1 << 16) - 1  # kEmMidGridLog2: floor(log2(work + 1)) >= 16
DENSE_MAX_COLS = 2048           # kEmDenseMaxCols
LDS_MAP_PATHS = 16384           # kLdsMapPaths
GRID_BIN, STREAMED_BIN = 11, 3
REGISTER_BINS = (4, 5, 6, 8, 9)
REGISTER_SLOT = 4               # the one launch of the register bins (emRegisterKernel) is counted under bin 4's index
BIN_NAMES = ("emSparseKernel<64,true>", "emSparseKernel<256,true>", "emSparseKernel<256,false>", "emSparseKernel<1024,false>",
             "emRegisterBinKernel<1,16>", "emRegisterBinKernel<2,16>", "emRegisterBinKernel<4,16>", "emSparseKernel<1024,true>",
             "emRegisterBinKernel<1,32>", "emRegisterBinKernel<2,32>", "emSparseKernel<1024,false,WIDE>", "emGridAccumKernel")
# workgroups per CU of each bin's persistent launch (rpvg_hip_em_solve: grid(per_cu))
PER_CU = {0: 2, 1: 2, 7: 1, 4: 2, 5: 2, 6: 2, 8: 2, 9: 2}


def lds_bytes(cols: int, rows: int, entries: int, block: int, resident: bool) -> int:
    b = 8 * ((1 + block // 64) * cols + block // 64 + 2)
    if resident:
        b += rows * 16 + entries * 8 + (rows + 1 + entries) * 4 + 8
    return (b + 15) & ~15


def grid_lds_bytes(cols: int) -> int:
    return 8 * 5 * cols


def em_bin(C: int, rows: int, entries: int) -> int:
    """emBinOf with the default rule (register kernels on, RPVG_HIP_EM_STREAM_SMALL = 0, grid from 2^18)."""
    work = rows + entries
    if work >= GRID_MIN_WORK and grid_lds_bytes(C) <= LDS_LIMIT:
        return GRID_BIN
    if C <= 16 and rows <= 256:
        return 4 if rows <= 64 else 5 if rows <= 128 else 6
    if C <= 32 and rows <= 128:
        return 8 if rows <= 64 else 9
    if lds_bytes(C, rows, entries, 64, True) <= 8 * 1024:
        return 0
    if lds_bytes(C, rows, entries, 256, True) <= 40 * 1024:
        return 1
    if lds_bytes(C, rows, entries, 1024, True) <= 152 * 1024:
        return 7
    if lds_bytes(C, 0, 0, 256, False) > LDS_LIMIT:
        return 10
    if lds_bytes(C, 0, 0, 1024, False) > LDS_LIMIT:
        return 2
    return 2 if work == 0 else 3


def is_mid(C: int, rows: int, entries: int) -> bool:
    """A streamed problem of 2^16 - 1 rows + entries or more, below the grid threshold (emOrderKernel's candidates)."""
    return em_bin(C, rows, entries) == STREAMED_BIN and rows + entries >= MID_GRID_MIN_WORK


def routes(shapes: Sequence[Tuple[int, int, int]]) -> List[int]:
    """The bin every problem of ONE rpvg_hip_em_solve call runs in: emBinOf, then the mid-size problems of the streamed bin
    move to the grid when the call has at most MID_GRID_MAX of them.  shapes: (C, kept rows, kept entries)."""
    mid = sum(is_mid(*s) for s in shapes)
    moved = 0 < mid <= MID_GRID_MAX
    return [GRID_BIN if moved and is_mid(*s) else em_bin(*s) for s in shapes]


def dense_rule(C: int, rows: int, entries: int) -> bool:
    """emDenseRule: a grid problem is solved on a dense row-major copy."""
    if C > DENSE_MAX_COLS or C < 2:
        return False
    ld = (C + 1) & ~1
    return 8 * rows * ld <= 12 * entries + 20 * rows


def expected_stats(shapes: Sequence[Tuple[int, int, int]], register_launches: int = 1) -> Tuple[Dict[int, int], int]:
    """(problems per statistics slot, grid problems on the dense sub-route) of one call, as accountEmSolve counts them."""
    slots: Dict[int, int] = {}
    dense = 0
    for s, b in zip(shapes, routes(shapes)):
        slot = REGISTER_SLOT if (b in REGISTER_BINS and register_launches == 1) else b
        slots[slot] = slots.get(slot, 0) + 1
        dense += int(b == GRID_BIN and dense_rule(*s))
    return slots, dense


# ---- clusters ---------------------------------------------------------------------------------------------------------
@dataclass
class Cluster:
    """One cluster as flat arrays: rows with their entries (one path per group)."""
    n_paths: int
    count: np.ndarray      # u32 [R]
    noise: np.ndarray      # f64 [R]
    ent_off: np.ndarray    # u64 [R+1]
    ent_path: np.ndarray   # u32 [E]
    ent_prob: np.ndarray   # f64 [E]

    def rows(self):
        """The rows as np_oracle / ClusterBatch.from_clusters take them."""
        off = self.ent_off.astype(np.int64)
        path, prob = self.ent_path.tolist(), self.ent_prob.tolist()
        return [(int(c), float(n), [(prob[e], [path[e]]) for e in range(off[r], off[r + 1])])
                for r, (c, n) in enumerate(zip(self.count.tolist(), self.noise.tolist()))]

    def kept(self, columns: Optional[Sequence[int]]) -> Tuple[int, int]:
        """Rows that touch a selected path, and their selected entries."""
        sel = np.ones(len(self.ent_path), dtype=bool) if columns is None else np.isin(self.ent_path, np.asarray(columns, dtype=np.uint32))
        row_of = np.repeat(np.arange(len(self.count)), np.diff(self.ent_off.astype(np.int64)))
        return int(len(np.unique(row_of[sel]))), int(sel.sum())


def batch_of(clusters: Sequence[Cluster]) -> ClusterBatch:
    rows = [len(c.count) for c in clusters]
    paths = [c.n_paths for c in clusters]
    ent_off, base = [np.zeros(1, dtype=np.uint64)], 0
    for c in clusters:
        ent_off.append(c.ent_off[1:].astype(np.uint64) + np.uint64(base))
        base += int(c.ent_off[-1])
    row_grp_off = np.concatenate(ent_off)
    G = int(row_grp_off[-1])
    P = sum(paths)
    return ClusterBatch(
        cluster_row_off=np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64),
        cluster_path_off=np.concatenate([[0], np.cumsum(paths)]).astype(np.uint64),
        row_count=np.concatenate([c.count for c in clusters]).astype(np.uint32),
        row_noise=np.concatenate([c.noise for c in clusters]).astype(np.float64),
        row_grp_off=row_grp_off, grp_prob=np.concatenate([c.ent_prob for c in clusters]).astype(np.float64),
        grp_idx_off=np.arange(G + 1, dtype=np.uint64), path_idx=np.concatenate([c.ent_path for c in clusters]).astype(np.uint32),
        path_group_id=np.zeros(P, dtype=np.uint32), path_source_count=np.ones(P, dtype=np.uint32),
        path_source_off=np.arange(P + 1, dtype=np.uint64), source_id=np.zeros(P, dtype=np.uint32),
        path_effective_length=np.full(P, 1000.0))


def _per_row(rng, rows: int, entries: int, most: int) -> np.ndarray:
    """Entries per row: at least one, at most `most`, `entries` in all (spread at random)."""
    assert rows <= entries <= rows * most, (rows, entries, most)
    k = np.ones(rows, dtype=np.int64)
    extra = entries - rows
    while extra > 0:
        room = np.nonzero(k < most)[0]
        pick = rng.choice(room, size=min(extra, len(room)), replace=False)
        k[pick] += 1
        extra -= len(pick)
    return k


def make_cluster(seed: int, n_paths: int, kept_rows: int, kept_entries: Optional[int] = None, most: int = 3,
                 pool: Optional[Sequence[int]] = None, dropped_rows: int = 0, other: Optional[Sequence[int]] = None,
                 noise_only_rows: int = 0, big_count: bool = False, noise_range: Tuple[float, float] = (1e-4, 0.2),
                 max_count: int = 20) -> Cluster:
    """kept_rows rows over the paths of `pool` (all paths but the last, which no row touches, by default) with kept_entries
    entries in all (at random between 1 and `most` per row); dropped_rows rows over the paths of `other` only (they touch
    no path of a problem over `pool`); noise_only_rows rows without a path.  The rows are shuffled together."""
    rng = np.random.default_rng(seed)
    pool = np.arange(max(1, n_paths - 1)) if pool is None else np.asarray(pool)
    other = np.zeros(0, dtype=np.int64) if other is None else np.asarray(other)
    ks = [_per_row(rng, kept_rows, kept_rows if kept_entries is None else kept_entries, min(most, len(pool)))]
    pools = [pool]
    if dropped_rows:
        ks.append(_per_row(rng, dropped_rows, dropped_rows, 1) + rng.integers(0, min(3, len(other)), size=dropped_rows))
        pools.append(other)
    R = kept_rows + dropped_rows
    # pairwise distinct noise: a permutation of R evenly spaced values (spacing >= 1e-7 for the sizes here)
    lo, hi = noise_range
    assert R < 2 or (hi - lo) / R > 10 * PROB_PRECISION
    noise = lo + (hi - lo) * (rng.permutation(R) + 0.5) / R
    theta = rng.lognormal(0.0, 1.5, size=n_paths)
    k_all = np.concatenate(ks)
    row_path, row_prob = [None] * R, [None] * R
    at = 0
    for k, pl in zip(ks, pools):
        n = len(pl)
        # distinct paths per row: an arithmetic progression modulo n with a step coprime to n
        steps = np.array([s for s in range(1, min(n, 64) + 1) if np.gcd(s, n) == 1] or [1])
        start = rng.integers(0, n, size=len(k))
        step = rng.choice(steps, size=len(k))
        for width in np.unique(k):
            rows = np.nonzero(k == width)[0]
            idx = pl[(start[rows, None] + step[rows, None] * np.arange(width)[None, :]) % n]
            w = theta[idx] * (rng.random(idx.shape) + 0.05)
            p = np.maximum(w / w.sum(axis=1, keepdims=True) * (1.0 - noise[at + rows])[:, None], 10 * PROB_PRECISION)
            order = np.argsort(p, axis=1, kind="stable")
            idx = np.take_along_axis(idx, order, axis=1)
            p = np.take_along_axis(p, order, axis=1)
            for j, r in enumerate(rows):
                row_path[at + r], row_prob[at + r] = idx[j], p[j]
        at += len(k)
    counts = rng.integers(1, max_count + 1, size=R + noise_only_rows).astype(np.uint32)
    if big_count:
        counts[0] = 1_000_000 + int(rng.integers(0, 1000))
    row_path += [np.zeros(0, dtype=np.int64)] * noise_only_rows
    row_prob += [np.zeros(0)] * noise_only_rows
    noise = np.concatenate([noise, np.ones(noise_only_rows)])
    k_all = np.concatenate([k_all, np.zeros(noise_only_rows, dtype=np.int64)])
    order = rng.permutation(R + noise_only_rows)
    return Cluster(n_paths=n_paths, count=counts[order], noise=noise[order],
                   ent_off=np.concatenate([[0], np.cumsum(k_all[order])]).astype(np.uint64),
                   ent_path=np.concatenate([row_path[i] for i in order]).astype(np.uint32),
                   ent_prob=np.concatenate([row_prob[i] for i in order]).astype(np.float64))


# ---- the table --------------------------------------------------------------------------------------------------------
@dataclass
class EmBinCase:
    name: str
    bin: int                     # emBinOf's bin (before the mid-size move of a call)
    build: object                # () -> Cluster
    columns: Optional[object] = None   # None: every path of the cluster; else () -> sorted path list
    max_em_its: int = 10000
    _cluster: Optional[Cluster] = field(default=None, repr=False)
    _shape: Optional[Tuple[int, int, int]] = field(default=None, repr=False)

    def cluster(self) -> Cluster:
        if self._cluster is None:
            self._cluster = self.build()
        return self._cluster

    def cols(self) -> List[int]:
        return list(range(self.cluster().n_paths)) if self.columns is None else list(self.columns())

    def shape(self) -> Tuple[int, int, int]:
        """(C, kept rows, kept entries) of the problem, counted from its rows."""
        if self._shape is None:
            rows, entries = self.cluster().kept(None if self.columns is None else self.cols())
            self._shape = (len(self.cols()) + 1, rows, entries)
        return self._shape


def _case(name, bin_, seed, n_paths, rows, entries=None, max_em_its=10000, **kw):
    return EmBinCase(name, bin_, lambda: make_cluster(seed, n_paths, rows, entries, **kw), None, max_em_its)


def _subset_case(name, bin_, seed, n_paths, chosen, kept, dropped, **kw):
    """A problem over `chosen` of the cluster's paths (the last of them touched by no row); `kept` rows touch the chosen
    paths only, `dropped` rows only paths outside them."""
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(n_paths, size=chosen, replace=False))
    rest = np.setdiff1d(np.arange(n_paths), cols)
    return EmBinCase(name, bin_, lambda: make_cluster(seed, n_paths, kept, 2 * kept - 5, pool=cols[:-1], dropped_rows=dropped,
                                                     other=rest, **kw),
                     lambda: [int(x) for x in cols], 10000)


# register bins: paths -> bins at 64, 65, 128, 129, 256, 257 rows (C = paths + 1 = 16 | 17 and 32 | 33)
REGISTER_EDGE_BINS = {15: (4, 5, 5, 6, 6, 1), 16: (8, 9, 9, 0, 1, 1), 31: (8, 9, 9, 0, 1, 1), 32: (0, 0, 0, 0, 1, 1)}
REGISTER_EDGE_ROWS = (64, 65, 128, 129, 256, 257)


def _cases() -> List[EmBinCase]:
    cases: List[EmBinCase] = []
    # register bins, two entries per row on average; the last path of every cluster is touched by no row (its abundance
    # goes to 0, below kMinEmAbundance); a few iteration caps around kMinEmConvIts, a count of a million, path-less rows
    for paths, bins in REGISTER_EDGE_BINS.items():
        for rows, b in zip(REGISTER_EDGE_ROWS, bins):
            its = {(15, 64): 1, (16, 65): 10, (31, 128): 11}.get((paths, rows), 10000)
            cases.append(_case(f"reg_p{paths}_r{rows}", b, 1000 + 7 * paths + rows, paths, rows, 2 * rows, max_em_its=its,
                               big_count=(paths, rows) == (16, 64), noise_only_rows=3 if rows == 129 else 0))
    cases.append(_case("one_path", 4, 11, 1, 40, 40, pool=[0]))   # C = 2
    cases.append(_case("one_row", 4, 12, 6, 1, 3))
    # LDS-resident bins at C = 33, one entry per row: CSR + vectors in 8 / 40 / 152 KB
    for rows, b in ((238, 0), (239, 1), (1236, 1), (1237, 7), (4718, 7), (4719, 3)):
        cases.append(_case(f"lds_r{rows}", b, 2000 + rows, 32, rows, rows))
    # streamed bins: four wavefronts from C = 1174, vectors in global memory from C = 3993
    for paths, b in ((1172, 3), (1173, 2), (3991, 2), (3992, 10)):
        cases.append(_case(f"streamed_p{paths}", b, 3000 + paths, paths, 300, 600, max_em_its=200))
    # the grid bin at rows + entries = 2^18 (emGridMinWork): CSR sub-route (C = 33, two entries per row) and dense sub-route
    # (C = 4, one entry per row: emDenseRule holds); one work unit less is a streamed problem of mid size
    cases.append(_case("grid_csr_lo", 3, 4001, 32, 87381, GRID_MIN_WORK - 1 - 87381, max_em_its=60))
    cases.append(_case("grid_csr_hi", 11, 4002, 32, 87381, GRID_MIN_WORK - 87381, max_em_its=60))
    cases.append(_case("grid_dense_lo", 3, 4003, 3, 131071, 131072, max_em_its=60))
    cases.append(_case("grid_dense_hi", 11, 4004, 3, 131072, 131072, max_em_its=60))
    # the grid's LDS cut: 40 C bytes fit 156 KB up to C = 3993; C = 3994 stays in the wide bin
    cases.append(_case("grid_lds_p3992", 11, 4005, 3992, 4096, GRID_MIN_WORK - 4096, most=63, max_em_its=10))
    cases.append(_case("grid_lds_p3993", 10, 4006, 3993, 4096, GRID_MIN_WORK - 4096, most=63, max_em_its=10))
    # mid-size streamed problems (emOrderKernel): rows + entries 2^16 - 2 | 2^16 - 1, and nine of 2^16 .. 2^18 for 8 | 9
    cases.append(_case("mid_work_lo", 3, 5001, 32, 32767, 32767, max_em_its=100))
    cases.append(_case("mid_work_hi", 3, 5002, 32, 32767, 32768, max_em_its=100))
    for i in range(9):
        rows = 26000 + 4500 * i
        cases.append(_case(f"mid_{i}", 3, 5100 + i, 32, rows, rows + 14000 + 1000 * i, max_em_its=100))
    # column subsets: kept rows on a register edge, next to rows that touch only paths outside the subset
    cases.append(_subset_case("subset_kept64", 4, 6001, 40, 12, 64, 50, noise_only_rows=4))
    cases.append(_subset_case("subset_kept65", 5, 6002, 40, 12, 65, 50))
    cases.append(_subset_case("subset_kept128", 9, 6003, 60, 25, 128, 70))
    cases.append(_subset_case("subset_kept129", 0, 6004, 60, 25, 129, 70))
    # the fill kernel's column map: in LDS up to 16 384 cluster paths, bisection in the sorted column list above
    cases.append(_subset_case("map_p16384", 9, 7001, LDS_MAP_PATHS, 24, 100, 200))
    cases.append(_subset_case("map_p16385", 9, 7002, LDS_MAP_PATHS + 1, 24, 100, 200))
    return cases


CASES: List[EmBinCase] = _cases()
BY_NAME: Dict[str, EmBinCase] = {c.name: c for c in CASES}
MID_COUNT_CASES = [f"mid_{i}" for i in range(9)]


def quantity(case: EmBinCase, what: str) -> int:
    C, rows, entries = case.shape()
    return {"C": C, "rows": rows, "work": rows + entries, "cluster_paths": case.cluster().n_paths}[what]


# Every named boundary: (quantity, its last value on the low side, case on the low side, case on the high side).  The two
# cases differ in that quantity by exactly one (test_em_bin_cases.py).
BOUNDARIES = {
    "C 16|17 at 64 rows": ("C", 16, "reg_p15_r64", "reg_p16_r64"),
    "C 16|17 at 128 rows": ("C", 16, "reg_p15_r128", "reg_p16_r128"),
    "C 16|17 at 256 rows": ("C", 16, "reg_p15_r256", "reg_p16_r256"),
    "C 32|33 at 64 rows": ("C", 32, "reg_p31_r64", "reg_p32_r64"),
    "C 32|33 at 128 rows": ("C", 32, "reg_p31_r128", "reg_p32_r128"),
    "rows 64|65 at C 16": ("rows", 64, "reg_p15_r64", "reg_p15_r65"),
    "rows 64|65 at C 17": ("rows", 64, "reg_p16_r64", "reg_p16_r65"),
    "rows 64|65 at C 32": ("rows", 64, "reg_p31_r64", "reg_p31_r65"),
    "rows 128|129 at C 16": ("rows", 128, "reg_p15_r128", "reg_p15_r129"),
    "rows 128|129 at C 17": ("rows", 128, "reg_p16_r128", "reg_p16_r129"),
    "rows 128|129 at C 32": ("rows", 128, "reg_p31_r128", "reg_p31_r129"),
    "rows 256|257 at C 16": ("rows", 256, "reg_p15_r256", "reg_p15_r257"),
    "LDS 8 KB (bins 0|1)": ("rows", 238, "lds_r238", "lds_r239"),
    "LDS 40 KB (bins 1|7)": ("rows", 1236, "lds_r1236", "lds_r1237"),
    "LDS 152 KB (bins 7|3)": ("rows", 4718, "lds_r4718", "lds_r4719"),
    "C 1173|1174 (bins 3|2)": ("C", 1173, "streamed_p1172", "streamed_p1173"),
    "C 3992|3993 (bins 2|10)": ("C", 3992, "streamed_p3991", "streamed_p3992"),
    "grid work 2^18, CSR": ("work", GRID_MIN_WORK - 1, "grid_csr_lo", "grid_csr_hi"),
    "grid work 2^18, dense": ("work", GRID_MIN_WORK - 1, "grid_dense_lo", "grid_dense_hi"),
    "grid LDS C 3993|3994": ("C", 3993, "grid_lds_p3992", "grid_lds_p3993"),
    "mid-size work 2^16 - 1": ("work", MID_GRID_MIN_WORK - 1, "mid_work_lo", "mid_work_hi"),
    "subset kept rows 64|65": ("rows", 64, "subset_kept64", "subset_kept65"),
    "subset kept rows 128|129": ("rows", 128, "subset_kept128", "subset_kept129"),
    "column map 16384|16385 paths": ("cluster_paths", LDS_MAP_PATHS, "map_p16384", "map_p16385"),
}


# ---- the fill kernel's work items (rpvg_hip_em_solve: problem list -> segments -> fillSegmentsKernel) ------------------------
FILL_SEGMENT_ROWS = 1024        # kFillSegmentRows
FILL_WORKGROUPS_PER_CU = 8      # fill_grid = min(items, 8 x CUs)


def fill_sequences(cluster_rows: Sequence[int], cus: int) -> List[List[int]]:
    """The problems every workgroup of fillSegmentsKernel meets, in its order: problem p has ceil(rows / 1 024) items (the
    segments of its cluster's rows, the problems' items one after the other), and the kernel is grid-stride — workgroup b
    takes items b, b + G, b + 2 G, ... with G = min(items, 8 x CUs)."""
    item_problem = [p for p, r in enumerate(cluster_rows) for _ in range(-(-r // FILL_SEGMENT_ROWS))]
    G = min(len(item_problem), FILL_WORKGROUPS_PER_CU * cus)
    return [[item_problem[i] for i in range(b, len(item_problem), G)] for b in range(G)]


def map_switches(clusters: Sequence[Cluster], problems: Sequence[Tuple[int, Sequence[int]]], cus: int) -> int:
    """How often a fill workgroup goes from one problem that uses the LDS column map straight to ANOTHER problem over other
    columns of the SAME cluster (the map it holds, mapped_problem, must then be rebuilt)."""
    def uses_map(p):
        k, cols = problems[p]
        n = clusters[k].n_paths
        return n <= LDS_MAP_PATHS and len(cols) != n

    switches = 0
    for seq in fill_sequences([len(clusters[k].count) for k, _ in problems], cus):
        for p, q in zip(seq, seq[1:]):
            if p != q and uses_map(p) and uses_map(q) and problems[p][0] == problems[q][0] and list(problems[p][1]) != list(problems[q][1]):
                switches += 1
    return switches


MAP_LANE_PROBLEMS = 4   # subset problems of one cluster that one fill workgroup takes in a row


def map_cache_call(cus: int, seed: int = 8001) -> Tuple[List[Cluster], List[Tuple[int, List[int]]]]:
    """One call of 4 x (8 x CUs) problems of one fill item each: identity-column fillers (every path of a small cluster: no
    map) and, at item indices b, b + G, b + 2 G, b + 3 G of a few workgroups b, four subset problems of ONE cluster — so
    that each of those workgroups builds the column map of a subset and then has to replace it by the next one's."""
    rng = np.random.default_rng(seed)
    clusters = [make_cluster(seed, 40, 1000, 2000), make_cluster(seed + 1, 28, 700, 1500, most=4), make_cluster(seed + 2, 6, 12, 20)]
    G = FILL_WORKGROUPS_PER_CU * cus
    problems: List[Tuple[int, List[int]]] = [(2, list(range(clusters[2].n_paths)))] * (MAP_LANE_PROBLEMS * G)
    for b, k in ((0, 0), (5, 0), (G // 2 + 3, 1), (G - 1, 1)):
        n = clusters[k].n_paths
        for j in range(MAP_LANE_PROBLEMS):
            size = int(rng.integers(3, n - 2))
            problems[b + j * G] = (k, sorted(int(x) for x in rng.choice(n, size=size, replace=False)))
    return clusters, problems


def fillers(bin_: int, n_distinct: int = 8) -> List[EmBinCase]:
    """Problems of one bin, sizes spread over the bin: the queue of a persistent launch takes them largest first."""
    out = []
    for i in range(n_distinct):
        f = (i + 0.5) / n_distinct
        if bin_ in (0, 1, 7):
            lo, hi = {0: (140, 238), 1: (239, 1236), 7: (1237, 4718)}[bin_]
            rows = int(lo + f * (hi - lo))
            out.append(_case(f"fill{bin_}_{i}", bin_, 9000 + 100 * bin_ + i, 32, rows, rows))
        else:
            paths = {4: 9, 5: 12, 6: 15, 8: 20, 9: 31}[bin_]
            lo, hi = {4: (2, 64), 5: (65, 128), 6: (129, 256), 8: (2, 64), 9: (65, 128)}[bin_]
            rows = int(lo + f * (hi - lo))
            out.append(_case(f"fill{bin_}_{i}", bin_, 9000 + 100 * bin_ + i, paths, rows, 2 * rows))
    return out
