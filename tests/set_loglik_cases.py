"""Cases and model of the set log-likelihoods of any group size: rpvg_hip_group_loglik (groupLoglikKernel<W>),
rpvg_hip_group_conditionals (groupConditionalKernel<W>) and rpvg_hip_group_full_posteriors (groupFullKernel<GS> with
groupFullNormaliseKernel) — rpvg_amd/csrc/loglik.hip, group_full.hip, sumCountLogs / sumCountLogsMulti of common.hpp.

The cases are matrices with one path per column, not normalised, without row collapse, every one a cluster of its own in one
batch: the smallest shapes at which a mechanism of the three kernels can still go wrong, named after the edge they stand on —
the ends of the three row classes, the lane strides and the segments between two folds of the running products (4 x 64 x 30 =
7 680 rows in sumCountLogs, 64 x 30 = 1 920 in sumCountLogsMulti<4, 64>), the two accumulators of the logarithm rows, the clamp
of the four candidate columns, the rank <-> members arithmetic of the enumeration and its 256-thread normalisation.  The rows,
the row classes and the batch are those of tests/pair_search_cases.py (Case, draw_rows, device_rows, row_class, batch_of).

The model is a plain numpy restatement in np.longdouble (math.fsum where longdouble is only 64 bits: _weighted_log_sums):
    set sum         sum_i c_i log(noise_i + sum_w M[i, m_w] / g (+ rowmax_i / g)), a kNoMember slot adding nothing
    conditionals    the set sums of (others..., k) for every candidate column k
    enumeration     every multiset in lexicographic order: set sum + sum_w log f_(m_w) + log numPermutations, normalised by
                    a log-sum-exp in the same precision

tests/test_set_loglik_cases.py asserts, on the model and the FP64 reference (oracle/np_oracle.py) alone, the conditions under
which the device tests can neither pass nor fail by accident; tests/test_hip_set_loglik.py holds the device to the model.
"""
from __future__ import annotations

import functools
import itertools
import math
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import np_oracle
from tests.pair_search_cases import (BITE, FLOOR, FOLD_FACTORS, MID_MAX_COUNT, SUB_FLOOR, Case, _weighted_log_sums, batch_of,  # noqa: F401
                                     device_rows, draw_rows, row_class)

NO_MEMBER = 0xFFFFFFFF        # kNoMember (loglik.hip)
WIDTHS = tuple(range(1, 9))
LOGLIK_SEGMENT = 4 * 64 * FOLD_FACTORS     # sumCountLogs: four chains per lane, a fold of each per segment
MULTI_SEGMENT = 64 * FOLD_FACTORS          # sumCountLogsMulti<4, 64>
CANDIDATES = 4                             # kCand, kFullCand
NORMALISE_THREADS = 256                    # kFullNormBlock
MAX_SPREAD = 650.0                         # every posterior a normal double: exp(-650 - log(6 435)) = 1e-286
UNDERFLOW = 760.0                          # below exp(-760) a posterior is 0 in FP64 whatever the last bits (denormals end at exp(-745))


# ---- the model --------------------------------------------------------------------------------------------------------------------

def _arguments(M, noise, members, g, add_rowmax, dtype):
    """noise + the members in slot order, each divided by g (+ the row maximum / g): [R] in dtype."""
    x = noise.astype(dtype)
    Mw = M.astype(dtype)
    for m in members:
        if m != NO_MEMBER:
            x = x + Mw[:, int(m)] / dtype(g)
    if add_rowmax:
        x = x + Mw.max(axis=1) / dtype(g)
    return x


def set_loglik_model(M, noise, counts, members, g, add_rowmax=False):
    return _weighted_log_sums(counts, _arguments(M, noise, members, g, add_rowmax, np.longdouble)[:, None])[0]


def conditionals_model(M, noise, counts, others, g):
    base = _arguments(M, noise, others, g, False, np.longdouble)
    return _weighted_log_sums(counts, base[:, None] + M.astype(np.longdouble) / np.longdouble(g))


def multisets(G: int, g: int) -> List[Tuple[int, ...]]:
    return list(itertools.combinations_with_replacement(range(G), g))


def _set_sums(M, noise, counts, sets: np.ndarray, g: int) -> np.ndarray:
    wide = np.longdouble
    Mw = M.astype(wide)
    out = np.zeros(len(sets), dtype=wide)
    step = max(1, 200000 // max(1, M.shape[0]))
    for s0 in range(0, len(sets), step):
        block = sets[s0:s0 + step]
        x = np.repeat(noise.astype(wide)[:, None], len(block), axis=1)
        for w in range(g):   # ascending members, as the enumeration adds them
            x = x + Mw[:, block[:, w]] / wide(g)
        out[s0:s0 + step] = _weighted_log_sums(counts, x)
    return out


def full_model(M, noise, counts, path_counts, g):
    """(multisets in lexicographic order, their log posteriors, their log-likelihoods before the normalisation)."""
    wide = np.longdouble
    sets = multisets(M.shape[1], g)
    idx = np.array(sets, dtype=np.int64).reshape(len(sets), g)
    pc = np.asarray(path_counts, dtype=np.float64)
    lf = np.log(pc.astype(wide) / wide(int(pc.sum())))
    assert np.allclose(lf.astype(np.float64), np_oracle.log_freqs(path_counts), rtol=1e-14, atol=0)
    ll = _set_sums(M, noise, counts, idx, g) + lf[idx].sum(axis=1)
    ll = ll + np.log(np.array([np_oracle.num_permutations(s) for s in sets], dtype=np.float64).astype(wide))
    top = ll.max()
    lse = top + np.log(np.sum(np.exp(ll - top)))
    return sets, ll - lse, ll


# ---- the mechanisms, restated -----------------------------------------------------------------------------------------------------

def loglik_chain_factors(fast_end: int) -> int:
    """The most factors one product of sumCountLogs multiplies between two folds over a count-1 class of fast_end rows: per segment
    of 7 680 rows a lane takes row lane, + 256, ... into four chains while four rows are left (i + 192 < end), the up to three rows
    that remain into chain 0, then folds."""
    most = 0
    for seg in range(0, fast_end, LOGLIK_SEGMENT):
        end = min(fast_end, seg + LOGLIK_SEGMENT)
        for lane in range(64):
            chain = [0, 0, 0, 0]
            i = seg + lane
            while i + 192 < end:
                for c in range(4):
                    chain[c] += 1
                i += 256
            while i < end:
                chain[0] += 1
                i += 64
            most = max(most, max(chain))
    return most


def multi_chain_factors(fast_end: int) -> int:
    """The same of sumCountLogsMulti<4, 64>: one product per lane and candidate, rows lane, + 64, ... of a segment of 1 920."""
    most = 0
    for seg in range(0, fast_end, MULTI_SEGMENT):
        end = min(fast_end, seg + MULTI_SEGMENT)
        most = max(most, len(range(seg, end, 64)))
    return most


def unfolded_sum(counts, x, fast_end: int, lanes_stride: int = 64) -> float:
    """A wrong model: the count-1 rows (the first fast_end of x, in the matrix's row order) multiplied into one FP64 product per
    lane that is never folded — it underflows to 0 after 35 factors of 2^-30 —, every other row by its logarithm."""
    total = 0.0
    with np.errstate(under="ignore", divide="ignore"):
        for lane in range(min(lanes_stride, fast_end)):
            p = 1.0
            for v in x[lane:fast_end:lanes_stride]:
                p *= float(v)
            total += math.log(p) if p > 0 else -math.inf
    return total + float(counts[fast_end:] @ np.log(x[fast_end:]))


def members_of_rank(G: int, g: int, rank: int) -> Tuple[int, ...]:
    """groupFullKernel's arithmetic: a non-decreasing m_1 .. m_g over G columns is the combination m_i + i - 1 of G + g - 1,
    found from its lexicographic rank through the combinatorial number system."""
    n, x, out = G + g - 1, 0, []
    for i in range(g):
        while x < n:
            c = math.comb(n - 1 - x, g - 1 - i)
            if rank < c:
                break
            rank -= c
            x += 1
        out.append(x - i)
        x += 1
    return tuple(out)


def rank_of_members(G: int, members: Sequence[int]) -> int:
    g, n, x, rank = len(members), G + len(members) - 1, 0, 0
    for i, m in enumerate(members):
        b = m + i
        while x < b:
            rank += math.comb(n - 1 - x, g - 1 - i)
            x += 1
        x += 1
    return rank


def clamp_reads_last_column(cond: np.ndarray) -> np.ndarray:
    """A wrong model: the conditionals of one request with every live candidate of the last block of four reading column G - 1."""
    G = len(cond)
    out = cond.copy()
    out[CANDIDATES * ((G - 1) // CANDIDATES):] = cond[G - 1]
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# routes of a case: "sets" — rpvg_hip_group_loglik and rpvg_hip_group_conditionals at every width 1 .. 8 —, "full" — the enumeration
# at the group sizes of `full` —.  Segments as in pair_search_cases.draw_rows; `zeros` = (segment, columns) whose cells are set to 0.

@dataclass(frozen=True)
class SetCase(Case):
    ends: tuple = None        # (fast_end, mid_end) the name promises: asserted from device_rows, and from the built matrix on the device
    zeros: tuple = ()
    full: tuple = ()          # group sizes of the enumeration
    columns: tuple = None     # the columns member lists may name (None: all)
    wrong: tuple = ()         # the wrong models the case names: "clamp", "fold_loglik", "fold_multi"
    underflow: bool = False

    def matrix(self):
        return _matrix(self)

    def reference(self):
        return _reference(self)


@functools.lru_cache(maxsize=None)
def _matrix(case: SetCase):
    """(M [R x G] in cluster row order, noise, counts, column multiplicities)."""
    rng = np.random.default_rng(case.seed)
    M, noise, counts = draw_rows(rng, case.G, case.segments)
    mult = rng.choice((1, 1, 2, 3, 7), size=case.G).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum([s[1] for s in case.segments])])
    for seg, cols in case.zeros:
        M[first[seg]:first[seg + 1], list(cols)] = 0.0
    if "full" in case.routes and case.G > 1:
        # a row without entries weighs the same in every set: the posteriors would not see it dropped.  It gets one cell
        empty = ~np.any(M, axis=1)
        M[empty, 0] = (1.0 - noise[empty]) / case.G
    for a in (M, noise, counts, mult):
        a.setflags(write=False)
    return M, noise, counts, mult


def _rows(fast=(), mid=(), slow=(), floor=0, sub=()) -> tuple:
    """Segments in cluster order — logarithm rows, then counts 2 .. 8 descending, then count 1: the matrix's row order (by class,
    stable) is a true permutation of it.  fast: row counts of ("fix", n, 1) segments; mid: (count, n); slow: (count, n); floor:
    leading rows of noise exactly 2^-30 and count 1; sub: (count, n) rows of noise nextafter(2^-30, 0)."""
    seg = [("sub_fix", n, c) for c, n in sub if n]
    seg += [("fix", n, c) for c, n in slow if n]
    seg += [("fix", n, c) for c, n in sorted(mid, reverse=True) if n]
    if floor:
        seg.append(("floor_fix", floor, 1))
    seg += [("fix", n, 1) for n in fast if n]
    return tuple(seg)


def _ends_of(segments) -> Tuple[int, int]:
    fast = sum(s[1] for s in segments if s[0] in ("fix", "floor_fix") and s[2] == 1)
    mid = sum(s[1] for s in segments if s[0] in ("fix", "floor_fix") and 2 <= s[2] <= MID_MAX_COUNT)
    return fast, fast + mid


# (G, g) of the enumeration
FULL_SHAPES = ([(1, g) for g in WIDTHS] + [(2, 8), (3, 5), (4, 4), (5, 4), (5, 8), (9, 3), (12, 5), (8, 8), (23, 3), (40, 2),
                                            (255, 1), (256, 1), (257, 1)])
LOGLIK_COUNT_1 = (0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 7679, 7680, 7681)
MULTI_COUNT_1 = (0, 1, 63, 64, 65, 1919, 1920, 1921, 3841)
MID_ROWS = (0, 1, 64, 65)
LOG_ROWS = (0, 1, 63, 64, 65, 127, 128, 129)
CONDITIONAL_COLUMNS = (1, 2, 3, 4, 5, 7, 8, 9, 65)
FOLD_BOUND_ROWS = 15296        # 7 680 + 7 616: in the second segment every lane has 29 rounds of four rows and three rows left


def _build_cases() -> List[SetCase]:
    cases: List[SetCase] = []
    seed = [61000]

    def add(name, G, segments, routes=("sets",), **more):
        seed[0] += 1
        more.setdefault("ends", _ends_of(segments))
        cases.append(SetCase(name, G, tuple(segments), SEEDS.get(name, seed[0]), tuple(routes), 0, **more))

    # --- sumCountLogs (groupLoglikKernel): 3 columns.  The other classes are there (2 rows of count 3, 3 logarithm rows) unless
    # the name says otherwise
    for n in LOGLIK_COUNT_1:
        add(f"loglik_count_1_rows_{n}", 3, _rows(fast=(n,), mid=((3, 2),), slow=((9, 3),)))
    # columns 0 and 1 are zero in the 15 296 rows of noise 2^-30: a request over them multiplies factors of exactly 2^-30
    add("loglik_fold_bound", 3, _rows(floor=FOLD_BOUND_ROWS, mid=((3, 20),), slow=((9, 20),)), zeros=((2, (0, 1)),), columns=(0, 1),
        wrong=("fold_loglik",))
    for c in range(2, MID_MAX_COUNT + 1):
        for n in MID_ROWS[1:]:
            add(f"count_{c}_rows_{n}", 3, _rows(fast=(5,), mid=((c, n),), slow=((40, 3),)))
    add("counts_2_to_8_rows_0", 3, _rows(fast=(5,), slow=((40, 3),)))
    add("counts_8_and_9", 3, _rows(fast=(3,), mid=((8, 5),), slow=((9, 5),)))
    for n in LOG_ROWS:
        add(f"log_rows_{n}", 3, _rows(fast=(4,), mid=((2, 2),), slow=((9, n - n // 2), (40, n // 2))))
    add("only_log_rows_below_the_floor", 3, _rows(sub=((1, 40), (8, 30))))
    add("no_log_rows", 3, _rows(fast=(20,), mid=((2, 3), (8, 3))))
    add("no_count_1_rows", 3, _rows(mid=((5, 7),), slow=((9, 6),)))
    add("one_row", 3, _rows(fast=(1,)))
    add("one_log_row", 3, _rows(slow=((9, 1),)))
    add("two_rows", 3, _rows(fast=(1,), mid=((3, 1),)))

    # --- sumCountLogsMulti<4, 64> (groupConditionalKernel, groupFullKernel): 5 columns, the enumeration at group size 2 on a few
    for n in MULTI_COUNT_1:
        add(f"multi_count_1_rows_{n}", 5, _rows(fast=(n,), mid=((3, 2),), slow=((9, 3),)),
            ("sets", "full") if n in (1919, 1920, 1921) else ("sets",), full=(2,) if n in (1919, 1920, 1921) else ())
    # every cell of the 1 920 rows of noise 2^-30 is zero: 30 factors of exactly 2^-30 per fold, whatever the candidate
    add("multi_fold_bound", 5, _rows(floor=MULTI_SEGMENT, mid=((3, 20),), slow=((9, 20),)), zeros=((2, (0, 1, 2, 3, 4)),))
    # ... and two such segments and a row: 61 factors in lane 0, which no product survives unfolded
    add("multi_fold_run", 5, _rows(floor=2 * MULTI_SEGMENT + 1, mid=((3, 20),), slow=((9, 20),)), zeros=((2, (0, 1, 2, 3, 4)),),
        wrong=("fold_multi",))

    # --- the candidate clamp: every remainder of 4
    for G in CONDITIONAL_COLUMNS:
        add(f"columns_{G}", G, _rows(fast=(9,), mid=((2, 3), (8, 2)), slow=((9, 3), (40, 2))),
            wrong=("clamp",) if (G - 1) % CANDIDATES else ())

    # --- the enumeration: at most 70 rows
    for G, g in FULL_SHAPES:
        if G == 1 and g > 1:
            continue
        rows = 70 if (G, g) == (8, 8) else 24
        add(f"full_{G}_columns" + ("" if G == 1 else f"_sets_of_{g}"), G, (("mix", rows),), ("full",), ends=None,
            full=WIDTHS if G == 1 else (g,))
    # one column without entries in 100 rows of noise 1e-4 .. 0.5 next to columns that explain them: the sets of that column alone
    # (and of it with little else) lie hundreds of log units below the rest
    add("full_underflow", 4, (("fix", 140, 3), ("mix", 10)), ("full",), ends=None, zeros=((0, (2, 3)),), full=(3,), underflow=True)
    return cases


SEEDS: Dict[str, int] = {}

CASES: List[SetCase] = _build_cases()
BY_NAME: Dict[str, SetCase] = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
INDEX: Dict[str, int] = {c.name: i for i, c in enumerate(CASES)}


def cases_of(route: str) -> List[SetCase]:
    return [c for c in CASES if route in c.routes]


# ---- the requests -----------------------------------------------------------------------------------------------------------------

def _columns(case: SetCase) -> Tuple[int, ...]:
    return tuple(range(case.G)) if case.columns is None else case.columns


@functools.lru_cache(maxsize=None)
def loglik_requests(case: SetCase, width: int) -> Tuple[Tuple[Tuple[int, ...], int], ...]:
    """(members, add_rowmax) of the case at a width: drawn members, one member in every slot, the same members in two slot orders,
    the row maximum on and off within the call, and at widths 2, 5 and 8 kNoMember in the first, a middle and the last slot."""
    rng = np.random.default_rng(7000 + 10 * case.seed + width)
    cols = _columns(case)
    drawn = tuple(int(c) for c in rng.choice(cols, size=width))
    reqs = [(drawn, 0), (drawn[::-1], 0), ((int(rng.choice(cols)),) * width, 0), (drawn, 1)]
    if width in (2, 5, 8):
        for slot in (0, width // 2, width - 1):
            for rowmax in (0, 1):
                reqs.append((drawn[:slot] + (NO_MEMBER,) + drawn[slot + 1:], rowmax))
    return tuple(dict.fromkeys(reqs))


@functools.lru_cache(maxsize=None)
def conditional_requests(case: SetCase, width: int) -> Tuple[Tuple[int, ...], ...]:
    """The others of the case's requests at a width: drawn, and one member in every slot."""
    rng = np.random.default_rng(9000 + 10 * case.seed + width)
    cols = _columns(case)
    reqs = [tuple(int(c) for c in rng.choice(cols, size=width - 1)), (int(rng.choice(cols)),) * (width - 1)]
    return tuple(dict.fromkeys(reqs))


def outputs_of(case: SetCase) -> List[Tuple[Tuple[int, ...], int, int]]:
    """Every set sum the "sets" route asks of the case, as (members, g, add_rowmax): the member-list requests of every width, then
    the conditionals of every width expanded over the candidate columns, in the order the device returns them."""
    out = []
    for w in WIDTHS:
        out += [(m, w, r) for m, r in loglik_requests(case, w)]
    for w in WIDTHS:
        for others in conditional_requests(case, w):
            out += [(others + (k,), w, 0) for k in range(case.G)]
    return out


# ---- references -------------------------------------------------------------------------------------------------------------------

def oracle_set_loglik(M, noise, counts, members, g, add_rowmax=False) -> float:
    """np_oracle.set_loglik (FP64, the members added in slot order); the row maximum as one more column, kNoMember slots dropped."""
    P = np.concatenate([M, M.max(axis=1, keepdims=True)], axis=1) if add_rowmax else M
    cols = [int(m) for m in members if m != NO_MEMBER] + ([M.shape[1]] if add_rowmax else [])
    return np_oracle.set_loglik(P, noise, counts, cols, g)


def tolerance(deviation: float, max_abs_ll: float) -> float:
    """8 x the FP64 reference's own deviation from the model, at least 2^-50 max |ll| (item 3 of docs/design/parity.md)."""
    return max(8.0 * deviation, 2.0 ** -50 * max_abs_ll)


def full_deviation(log_posterior: np.ndarray, posteriors: np.ndarray, keep: np.ndarray = None):
    """(largest |d_k - d_best| over the kept sets, its rank, d_best) with d_k = log(got_k) - log(want_k)."""
    with np.errstate(divide="ignore"):
        d = np.log(np.asarray(posteriors, dtype=np.float64).astype(np.longdouble)) - log_posterior
    best = int(np.argmax(log_posterior))
    rel = np.abs(d - d[best])
    if keep is not None:
        rel = np.where(keep, rel, 0)
    worst = int(np.argmax(rel))
    return float(rel[worst]), worst, float(d[best])


@dataclass
class FullReference:
    sets: list
    log_posterior: np.ndarray
    ll: np.ndarray
    kept: np.ndarray              # sets above exp(-760): all but in the underflow case
    oracle_posteriors: np.ndarray
    oracle_deviation: float
    oracle_best: float
    max_abs_ll: float
    tol: float


@dataclass
class Reference:
    model: np.ndarray             # per output of outputs_of (empty without the "sets" route)
    oracle: np.ndarray
    oracle_deviation: float
    max_abs_ll: float
    tol: float
    full: Dict[int, FullReference]

    def loglik(self, case: SetCase, width: int) -> np.ndarray:
        first = sum(len(loglik_requests(case, w)) for w in WIDTHS if w < width)
        return self.model[first:first + len(loglik_requests(case, width))]

    def conditionals(self, case: SetCase, width: int) -> np.ndarray:
        """[requests x G]"""
        first = sum(len(loglik_requests(case, w)) for w in WIDTHS)
        first += sum(len(conditional_requests(case, w)) for w in WIDTHS if w < width) * case.G
        n = len(conditional_requests(case, width))
        return self.model[first:first + n * case.G].reshape(n, case.G)


@functools.lru_cache(maxsize=None)
def _reference(case: SetCase) -> Reference:
    """Model and FP64 reference of a case, computed once and shared; the tolerances come from these two alone."""
    M, noise, counts, mult = case.matrix()
    model, oracle = np.zeros(0, dtype=np.longdouble), np.zeros(0)
    if "sets" in case.routes:
        outs = outputs_of(case)
        model = np.array([set_loglik_model(M, noise, counts, m, g, r) for m, g, r in outs], dtype=np.longdouble)
        oracle = np.array([oracle_set_loglik(M, noise, counts, m, g, r) for m, g, r in outs])
    dev = float(np.max(np.abs(oracle - model))) if len(model) else 0.0
    top = float(np.max(np.abs(model))) if len(model) else 0.0
    full = {}
    for g in case.full:
        sets, lp, ll = full_model(M, noise, counts, mult, g)
        osets, opost = np_oracle.posteriors_full(M, noise, counts, mult, g)
        assert osets == sets
        kept = lp >= -UNDERFLOW
        fdev, _, d_best = full_deviation(lp, opost, kept)
        ftop = float(np.max(np.abs(ll[kept])))
        full[g] = FullReference(sets, lp, ll, kept, opost, fdev, abs(d_best), ftop, tolerance(fdev, ftop))
    return Reference(model, oracle, dev, top, tolerance(dev, top), full)


# ---- conditions (asserted by tests/test_set_loglik_cases.py) ------------------------------------------------------------------------

def output_terms(case: SetCase) -> np.ndarray:
    """[R x outputs] the term c_r log(x_r) of every row in every output of outputs_of (FP64: what a row weighs needs no more)."""
    M, noise, counts, _ = case.matrix()
    outs = outputs_of(case)
    terms = np.zeros((M.shape[0], len(outs)))
    for j, (m, g, r) in enumerate(outs):
        terms[:, j] = counts * np.log(_arguments(M, noise, m, g, r, np.float64))
    return terms


def column_bites(case: SetCase) -> Dict[int, float]:
    """Per column that an output names: the largest change of an output when the column's cells are replaced by its neighbour's
    (a + 1; a - 1 for the last) in every slot that names it."""
    M, noise, counts, _ = case.matrix()
    G = case.G
    bites: Dict[int, float] = {}
    if G == 1:
        return bites
    for m, g, r in outputs_of(case):
        own = float(counts @ np.log(_arguments(M, noise, m, g, r, np.float64)))
        for a in set(m) - {NO_MEMBER}:
            n = a + 1 if a + 1 < G else a - 1
            moved = tuple(n if x == a else x for x in m)
            there = float(counts @ np.log(_arguments(M, noise, moved, g, r, np.float64)))
            bites[a] = max(bites.get(a, 0.0), abs(there - own))
    return bites
