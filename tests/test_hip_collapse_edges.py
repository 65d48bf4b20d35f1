"""The replay of the row collapse (rpvg_amd/csrc/row_collapse.hip) pinned to the reference's run rule at the sizes where it takes
another route: the cases of tests/collapse_edge_cases.py — whose conditions tests/test_collapse_edge_cases.py asserts on the
CPU — built on the device and read back row by row (rpvg_hip_groups_rows).

Group matrices: every case is built plain and with collapse_precision = 1e-8; collapse_heads runs on the downloaded plain
matrix, on which conditions (a) and (b) are asserted again, and every row of the collapsed build must equal the plain build's
row head[r] bit for bit — columns, noise, row maximum — with its own count.  No tolerance; the rounding-equal class, which the
device leaves alone, is held to kEquivalentRelative = 1e-13 per value.  rpvg_hip_groups_collapse_info confirms the route: the
listed rows (the list's size decides between the pair table in LDS, in global memory, the network in LDS and in global
memory), the matrices sorted whole, the rows replaced.

The held-back stage: matrices from the batch's own columns are searched as built and the search's sums adjusted for the rows the
last stage rewrites; every pair's posterior against tests/pair_search_cases.pair_model on the model-collapsed matrix, the
tolerance formed as tests/test_hip_pair_search.py forms it (8 x the CPU oracle's own distance from the model, at least
2^-50 max |ll|), and against the same call with the whole collapse in front of the search.

EM problems: rpvg_hip_em_solve with collapse_precision against read_collapse + the oracle's EM, iteration count exact.

The tests print what they measured (pytest -s); the MI355X figures are in docs/design/parity.md.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import hip
from tests import collapse_edge_cases as cc
from tests import pair_search_cases as psc
from tests import small_cases

pytestmark = pytest.mark.gpu

IDS = lambda c: c.name  # noqa: E731
INDEX = {c.name: i for i, c in enumerate(cc.CASES)}                 # cluster of the batch
LISTED = [c for c in cc.CASES if c.R]
AT = {cc.CASES[k].name: m for m, k in reversed(list(enumerate(cc.joint_listing())))}   # matrix of the joint call (first listing)


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case a cluster of its own, uploaded as one batch."""
    dev = hip_ctx.upload(cc.batch_of(cc.CASES))
    yield dev
    dev.free()


def _build(hip_ctx, table, listing, precision):
    """One call: the matrices of the listed clusters (column c = path c alone, normalised), each downloaded as
    (P [R x (G + 1)] with the noise last, row maxima, counts), and the counters of the collapse."""
    dg = hip_ctx.groups(table, listing, None, True, collapse_precision=precision)
    try:
        out = []
        for m in range(len(listing)):
            values, noise, rowmax, count = dg.rows(m)
            out.append((np.concatenate([values, noise[:, None]], axis=1), rowmax, count))
        return out, dg.collapse_info()
    finally:
        dg.free()


_CACHE = {}


def _joint(hip_ctx, table, precision):
    key = ("joint", precision)
    if key not in _CACHE:
        _CACHE[key] = _build(hip_ctx, table, cc.joint_listing(), precision)
    return _CACHE[key]


def _alone(hip_ctx, table, case, precision):
    key = (case.name, precision)
    if key not in _CACHE:
        mats, info = _build(hip_ctx, table, [INDEX[case.name]], precision)
        _CACHE[key] = (mats[0], info)
    return _CACHE[key]


def _heads(case, P, counts):
    """collapse_heads on the downloaded plain matrix (once per case)."""
    key = ("heads", case.name)
    if key not in _CACHE:
        _CACHE[key] = cc.collapse_heads(P, counts) if len(counts) else np.zeros(0, dtype=np.int64)
    return _CACHE[key]


def _same_bits(x, y):
    return all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(x, y))


def _expected_counters(cases, total_rows):
    """(matrices replayed, rows replaced, matrices sorted whole, listed rows) of a call on these cases, from the model and the
    restated constants; a call whose candidate pairs outgrow its pair buffer sorts the crowded matrix whole."""
    replayed = replaced = whole = listed = 0
    pairs = sum(cc.window_candidates(c.matrix()[0])[3] for c in cases if c.R)
    for c in cases:
        if c.kind != "exact" or c.listed < 2:
            continue
        P, _ = c.matrix()
        as_whole = c.whole or pairs > cc.pair_capacity(total_rows)
        assert not (pairs > cc.pair_capacity(total_rows)) or len(cases) == 1   # (which matrix overflows is only known of a call of one)
        replayed += 1
        replaced += cc.replaced_rows(P, cc.heads_of(c.name))
        whole += 1 if as_whole else 0
        listed += c.R if as_whole else c.listed
    return replayed, replaced, whole, listed


@pytest.mark.parametrize("case", LISTED, ids=IDS)
def test_the_plain_build_is_the_restatement_in_the_matrix_row_order(hip_ctx, table, case):
    """What rows() returns: the normalised matrix of the numpy restatement, bit for bit, rows by class and cluster order."""
    (P, rowmax, counts), _ = _joint(hip_ctx, table, 0.0)[0][AT[case.name]], None
    want, want_counts = case.matrix()
    order = cc.matrix_row_order(want_counts, want[:, -1])
    assert P.shape == (case.R, case.G + 1)
    assert np.array_equal(counts, want_counts[order])
    assert P.tobytes() == np.ascontiguousarray(want[order]).tobytes(), case.name
    assert np.array_equal(rowmax, P[:, :-1].max(axis=1))


@pytest.mark.parametrize("case", LISTED, ids=IDS)
def test_every_row_holds_the_values_of_its_head(hip_ctx, table, case):
    m = AT[case.name]
    P0, rowmax0, counts0 = _joint(hip_ctx, table, 0.0)[0][m]
    P1, rowmax1, counts1 = _joint(hip_ctx, table, cc.PRECISION)[0][m]
    assert np.array_equal(counts1, counts0)   # a row keeps its own count
    head = _heads(case, P0, counts0)
    if case.kind == "exact":
        assert cc.column_gaps(P0) >= cc.APART_RELATIVE                     # (a) on the device's own values
        below, above = cc.pair_distance_gap(P0)
        assert below <= cc.CLOSE_BELOW and above >= cc.APART_ABOVE          # (b)
        wrong = np.flatnonzero(np.any(P1 != P0[head], axis=1) | (rowmax1 != rowmax0[head]))
        assert len(wrong) == 0, (f"{case.name} ({case.route}, {case.R} rows, {case.G} columns): {len(wrong)} rows do not hold their head's values, "
                                 f"first row {wrong[0]} (head {head[wrong[0]]}): {P1[wrong[0]]} against {P0[head[wrong[0]]]}")
        assert P1.tobytes() == np.ascontiguousarray(P0[head]).tobytes() and rowmax1.tobytes() == np.ascontiguousarray(rowmax0[head]).tobytes()
    else:
        want, want_max = P0[head], rowmax0[head]
        assert np.all(np.abs(P1 - want) <= cc.EQUIVALENT_RELATIVE * np.minimum(np.abs(P1), np.abs(want))), case.name
        assert np.all(np.abs(rowmax1 - want_max) <= cc.EQUIVALENT_RELATIVE * want_max)
        assert P1.tobytes() == P0.tobytes()   # left alone, in fact


def test_the_joint_call_reports_the_models_counters(hip_ctx, table):
    cases = [cc.CASES[k] for k in cc.joint_listing()]
    _, info = _joint(hip_ctx, table, cc.PRECISION)
    want = _expected_counters(cases, sum(c.R for c in cases))
    print(f"joint call of {len(cases)} matrices, {sum(c.R for c in cases)} rows: (replayed, replaced, whole, listed) = {info}, model {want}")
    assert info == want
    assert _joint(hip_ctx, table, 0.0)[1] == (0, 0, 0, 0)


@pytest.mark.parametrize("case", LISTED, ids=IDS)
def test_a_case_alone_gives_the_bytes_of_the_joint_call_and_its_own_counters(hip_ctx, table, case):
    alone, info = _alone(hip_ctx, table, case, cc.PRECISION)
    assert _same_bits(alone, _joint(hip_ctx, table, cc.PRECISION)[0][AT[case.name]]), case.name
    want = _expected_counters([case], case.R)
    print(f"{case.name:26s} {case.R:5d} rows {case.G:3d} columns, route {case.route:12s}: (replayed, replaced, whole, listed) = {info}, model {want}")
    assert info == want, case.name
    if case.route in cc.ROUTES and not want[2]:
        assert cc.list_route(info[3]) == case.route   # the list the device made takes the route the case is there for
    plain, _ = _alone(hip_ctx, table, case, 0.0)
    assert _same_bits(plain, _joint(hip_ctx, table, 0.0)[0][AT[case.name]]), case.name


def test_the_crowds_take_the_whole_matrix_route_on_one_side_only(hip_ctx, table):
    """In the joint call, whose pair buffer holds every candidate pair, the crowd of 257 rows (256 candidates of its lowest row)
    is listed and the crowd of 258 is sorted whole: the joint counters say one whole matrix and the sum of the lists says which."""
    cases = [cc.CASES[k] for k in cc.joint_listing()]
    _, info = _joint(hip_ctx, table, cc.PRECISION)
    small, large = (cc.BY_NAME[f"crowd_{n}"] for n in cc.CROWD_SIZES)
    assert (small.whole, large.whole) == (0, 1) and info[2] == 1
    others = sum(c.listed for c in cases if c.kind == "exact" and c.listed >= 2 and not c.name.startswith("crowd_"))
    assert info[3] == others + small.listed + large.R
    for case in (small, large):   # alone, a crowd's pairs outgrow the buffer of its call: sorted whole, the same bytes (above)
        assert _alone(hip_ctx, table, case, cc.PRECISION)[1][2] == 1


def test_a_cluster_listed_twice_gives_the_same_bytes_twice(hip_ctx, table):
    listing = cc.joint_listing()
    assert listing[-1] == INDEX[cc.TWICE] and listing.count(listing[-1]) == 2
    for precision in (0.0, cc.PRECISION):
        mats, _ = _joint(hip_ctx, table, precision)
        assert _same_bits(mats[-1], mats[AT[cc.TWICE]])


def test_two_runs_give_the_same_bytes(hip_ctx, table):
    first, info = _joint(hip_ctx, table, cc.PRECISION)
    again, info_again = _build(hip_ctx, table, cc.joint_listing(), cc.PRECISION)
    assert info == info_again
    for x, y in zip(first, again):
        assert _same_bits(x, y)


def test_a_matrix_without_rows_is_refused_by_the_build(hip_ctx, table):
    """The cluster without rows travels in the batch between the others; the build takes no matrix on it (planGroupBuild)."""
    k = INDEX["no_rows"]
    assert cc.CASES[k].R == 0 and 0 < k < len(cc.CASES) - 1
    for precision in (0.0, cc.PRECISION):
        with pytest.raises(hip.EngineError, match="no rows or no columns"):
            hip_ctx.groups(table, [INDEX["rows_1"], k], None, True, collapse_precision=precision)


def test_rows_refuses_what_it_cannot_read(hip_ctx, table):
    dg = hip_ctx.groups(table, [INDEX["ends"]], None, True)
    try:
        R, G = cc.BY_NAME["ends"].R, 3
        bufs = [np.zeros(R * G), np.zeros(R), np.zeros(R), np.zeros(R)]
        ptr = [C.c_void_p(b.ctypes.data) for b in bufs]
        call = hip.lib().rpvg_hip_groups_rows
        assert call(hip_ctx.handle, dg.handle, C.c_uint32(0), *ptr) == 0
        assert call(hip_ctx.handle, dg.handle, C.c_uint32(1), *ptr) == -3       # RPVG_HIP_ERR_INVALID: matrix out of range
        assert call(None, dg.handle, C.c_uint32(0), *ptr) == -3
        assert call(hip_ctx.handle, None, C.c_uint32(0), *ptr) == -3
        for k in range(4):
            assert call(hip_ctx.handle, dg.handle, C.c_uint32(0), *[None if i == k else p for i, p in enumerate(ptr)]) == -3
    finally:
        dg.free()


# ---- the held-back stage ----------------------------------------------------------------------------------------------------------------

HELD_INDEX = {c.name: i for i, c in enumerate(cc.HELD_CASES)}


@pytest.fixture(scope="module")
def held_table(hip_ctx):
    dev = hip_ctx.upload(cc.batch_of(cc.HELD_CASES))
    yield dev
    dev.free()


def _search(hip_ctx, held_table, before_search: bool):
    """One call on every held-back case: matrices from the batch's own columns with the collapse, the diploid search with every
    pair kept, then the matrices as the search left them.  before_search: RPVG_HIP_COLLAPSE_BEFORE_SEARCH=1, the whole collapse
    first."""
    key = ("search", before_search)
    if key in _CACHE:
        return _CACHE[key]
    name, old = "RPVG_HIP_COLLAPSE_BEFORE_SEARCH", os.environ.get("RPVG_HIP_COLLAPSE_BEFORE_SEARCH")
    try:
        if before_search:
            os.environ[name] = "1"
        else:
            os.environ.pop(name, None)
        dg = hip.DeviceGroups.from_sources(hip_ctx, held_table, list(range(len(cc.HELD_CASES))), True, cc.PRECISION)
        try:
            found = dg.bounded_pair_posteriors(None, psc.MIN_REL_LIKELIHOOD)
            mats = [dg.rows(m) for m in range(len(cc.HELD_CASES))]
            info = dg.collapse_info()
        finally:
            dg.free()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old
    _CACHE[key] = (found, mats, info)
    return _CACHE[key]


def _by_pair(pairs, log_values):
    return {(min(a, b), max(a, b)): float(v) for (a, b), v in zip(pairs, log_values)}


def _deviation(got: dict, want: dict):
    """(largest |d_k - d_best|, d_best) with d_k = log got_k - log want_k, best = the model's most likely pair."""
    best = max(want, key=lambda k: want[k])
    d = {k: got[k] - want[k] for k in want}
    return max(abs(d[k] - d[best]) for k in want), d[best]


@pytest.mark.parametrize("case", cc.HELD_CASES, ids=IDS)
def test_the_search_in_front_of_the_last_stage_gives_the_models_posteriors(hip_ctx, held_table, case):
    k = HELD_INDEX[case.name]
    assert held_table.has_source_columns()
    assert held_table.source_columns(k) == ([int(x) for x in case.multiplicities()], [[p] for p in range(case.G)])
    P, counts = case.matrix()
    order = cc.matrix_row_order(counts, P[:, -1])
    P, counts = np.ascontiguousarray(P[order]), counts[order]
    head = cc.collapse_heads(P, counts)
    Pc = P[head]
    M, noise, mult = np.ascontiguousarray(Pc[:, :-1]), np.ascontiguousarray(Pc[:, -1]), case.multiplicities()
    model = psc.pair_model(M, noise, counts, mult)
    want = _by_pair(model.sequence, model.log_posterior)
    sets, post = pyoracle.group_posteriors(M, noise, counts, mult, 2, bounded=True, min_rel_lik=psc.MIN_REL_LIKELIHOOD)
    assert len(sets) == len(want)
    oracle_dev, oracle_best = _deviation(_by_pair(sets, np.log(np.asarray(post, dtype=np.float64))), want)
    tol = max(8.0 * oracle_dev, 2.0 ** -50 * float(np.max(np.abs(model.seq_ll))))

    results = {}
    for before_search in (False, True):
        found, mats, info = _search(hip_ctx, held_table, before_search)
        pairs, posteriors = found[k]
        assert len(pairs) == len(want) and {(min(a, b), max(a, b)) for a, b in pairs} == set(want), (case.name, before_search)
        with np.errstate(divide="ignore"):
            got = _by_pair(pairs, np.log(posteriors))
        worst, d_best = _deviation(got, want)
        results[before_search] = (worst, got)
        assert abs(float(posteriors.sum()) - 1) < 1e-9
        assert worst <= tol, f"{case.name}, collapse {'before' if before_search else 'behind'} the search: log posterior off by {worst:.3e} (tolerance {tol:.3e})"
        assert abs(d_best) <= tol + abs(oracle_best)
        # behind the search the matrices hold their heads' values, whichever way round
        values, noise_d, rowmax, count = mats[k]
        assert np.concatenate([values, noise_d[:, None]], axis=1).tobytes() == Pc.tobytes() and np.array_equal(count, counts)
        assert np.array_equal(rowmax, Pc[:, :-1].max(axis=1))
    behind, front = results[False][1], results[True][1]
    best = max(want, key=lambda key: want[key])
    between = max(abs((behind[key] - front[key]) - (behind[best] - front[best])) for key in want)
    ratio = lambda x: x / tol if tol else 0.0   # noqa: E731 (one column: one pair, its posterior 1 on every side)
    print(f"{case.name:14s} {case.R:5d} rows {case.G} columns: worst |d_k - d_best| behind the search {results[False][0]:.1e} "
          f"({ratio(results[False][0]):.2f} tol), in front {results[True][0]:.1e} ({ratio(results[True][0]):.2f} tol), between the two {between:.1e} "
          f"({ratio(between):.2f} tol); oracle {oracle_dev:.1e}, tol {tol:.1e}")
    assert between <= 2 * tol


def test_the_held_back_call_reports_the_models_counters(hip_ctx, held_table):
    want = _expected_counters(cc.HELD_CASES, sum(c.R for c in cc.HELD_CASES))
    for before_search in (False, True):
        assert _search(hip_ctx, held_table, before_search)[2] == want, before_search


# ---- EM problems --------------------------------------------------------------------------------------------------------------------------

def test_em_problems_are_collapsed_as_the_reference_collapses_them(hip_ctx):
    cases = cc.EM_CASES
    dev = hip_ctx.upload(cc.batch_of(cases))
    try:
        cols = [list(range(c.G)) for c in cases]
        abund, noise, total, iters = hip_ctx.em_solve(dev, list(range(len(cases))), cols, collapse_precision=cc.PRECISION)
        plain, _, _, plain_iters = hip_ctx.em_solve(dev, list(range(len(cases))), cols)
    finally:
        dev.free()
    for k, case in enumerate(cases):
        cluster = case.cluster()
        P, pn, pc = np_oracle.dense_matrix(cluster["rows"], case.G, cols[k])
        Pn = np_oracle.add_noise_and_normalize(P, pn)
        assert Pn.tobytes() == case.matrix()[0].tobytes()
        Pc, merged_counts = np_oracle.read_collapse(Pn, pc, cc.PRECISION)
        ab_o, nc_o, tot_o, its_o, _ = pyoracle.em_dense(Pc, merged_counts)
        worst = float(np.max(np.abs(abund[k] - ab_o) / np.maximum(ab_o, 1e-300)))
        off = float(np.max(np.abs(plain[k] - ab_o) / np.maximum(ab_o, 1e-300)))
        print(f"{case.name:26s} {case.R:4d} rows -> {len(merged_counts):3d}: iterations {int(iters[k])} (oracle {its_o}), abundances {worst:.1e} relative "
              f"from the oracle's (uncollapsed device solve: {off:.1e})")
        assert total[k] == tot_o and int(iters[k]) == its_o, case.name
        assert small_cases.rel_close(abund[k], ab_o, rel=cc.EM_BAR, floor=0.0), (case.name, abund[k], ab_o)
