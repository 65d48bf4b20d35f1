"""rpvg_hip_bounded_pair_posteriors with every pair kept (min_rel_likelihood 1e-300) against the longdouble model of
tests/pair_search_cases.py: the list in the reference's visiting order — its length pins the compaction, its order the rank of
every marginal, its posteriors every pair's sum relative to the best pair.

Every case meets, on the CPU (tests/test_pair_search_cases.py): the pairs span at most 650 log units, so none is dropped; the
smallest gap between two marginals is at least 1 000 tolerances, so the order is decided; removing any row — but the few rows of
noise 1 without entries, which add log 1 = 0 by design and lie off every edge of a class, chunk or block — or reading any
column's neighbour moves some pair's sum by at least 1 000 tolerances.  The tolerance of a case is 8 x the largest deviation of
the CPU oracle (FP64, rows added one after the other) from the model on that case, at least 2^-50 max |ll| — measured against
the reference, never against the device.  No case is skipped, masked or loosened here.  The tests print the device's worst
deviation per case (pytest -s); the MI355X figures are in docs/design/parity.md.
"""
import os

import numpy as np
import pytest

from tests import pair_search_cases as psc

pytestmark = pytest.mark.gpu

INDEX = {c.name: i for i, c in enumerate(psc.CASES)}
ROUTE_CASES = [(route, case) for route in psc.ROUTES for case in psc.cases_of(route)]


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case a cluster of its own, uploaded as one batch."""
    dev = hip_ctx.upload(psc.batch_of(psc.CASES))
    yield dev
    dev.free()


def _search(hip_ctx, table, cases, route):
    """One call: the matrices of `cases` (column c = path c alone, not normalised, no row collapse), searched on `route`."""
    groups = [[[p] for p in range(c.G)] for c in cases]
    dg = hip_ctx.groups(table, [INDEX[c.name] for c in cases], groups, False)
    before = {name: os.environ.get(name) for name in psc.KNOBS}
    try:
        for name in psc.KNOBS:   # every knob of the plan set or removed: the route is what the caller names, whatever was set outside
            if name in psc.ROUTES[route]:
                os.environ[name] = psc.ROUTES[route][name]
            else:
                os.environ.pop(name, None)
        return dg.bounded_pair_posteriors(np.concatenate([c.matrix()[3] for c in cases]), psc.MIN_REL_LIKELIHOOD)
    finally:
        for name, value in before.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value
        dg.free()


_TOGETHER, _ALONE = {}, {}


def _together(hip_ctx, table, route):
    """All cases of a route in one call (computed once): {case name: (pairs, posteriors)}."""
    if route not in _TOGETHER:
        cases = psc.cases_of(route)
        _TOGETHER[route] = dict(zip([c.name for c in cases], _search(hip_ctx, table, cases, route)))
    return _TOGETHER[route]


def _alone(hip_ctx, table, route, case):
    if (route, case.name) not in _ALONE:
        _ALONE[(route, case.name)] = _search(hip_ctx, table, [case], route)[0]
    return _ALONE[(route, case.name)]


def _same_bits(x, y):
    return x[0] == y[0] and x[1].tobytes() == y[1].tobytes()


def _rows_of(case, route):
    _, noise, counts, _ = case.matrix()
    _, fast_end, mid_end = psc.device_rows(counts, noise)
    chunk = int(psc.ROUTES[route].get("RPVG_HIP_PAIR_CHUNK_ROWS", psc.CHUNK_ROWS))
    return f"{case.R} rows (count 1 below {fast_end}, counts 2 .. 8 below {mid_end}) in chunks of {chunk}"


@pytest.mark.parametrize("route,case", ROUTE_CASES, ids=lambda x: x if isinstance(x, str) else x.name)
def test_every_pair_equals_the_model(hip_ctx, table, route, case):
    pairs, posteriors = _together(hip_ctx, table, route)[case.name]
    ref = case.reference()
    model = ref.model
    where = f"{case.name} on route {route}: {case.G} columns, {_rows_of(case, route)}"

    # the kept list is the model's, in order: length, order, every (first, second)
    if pairs != model.sequence:
        assert len(pairs) == len(model.sequence), f"{where}: {len(pairs)} pairs kept of {len(model.sequence)}"
        k = next(i for i, (x, y) in enumerate(zip(pairs, model.sequence)) if x != y)
        got_order = list(dict.fromkeys(a for a, _ in pairs))
        pytest.fail(f"{where}: pair {k} of the list is {pairs[k]}, the model's {model.sequence[k]}; columns in visiting order from the first "
                    f"difference: {[(g, w) for g, w in zip(got_order, model.order) if g != w][:4]} (device, model); "
                    f"{psc.place_of_pair(case.G, *model.sequence[k])}")

    # every pair's posterior relative to the best pair's
    worst, k, d_best = psc.deviation(model, posteriors)
    print(f"{route:8s} {case.name:45s} worst |d_k - d_best| {worst:.1e} (oracle {ref.oracle_deviation:.1e}, tol {ref.tol:.1e}), "
          f"|d_best| {abs(d_best):.1e} (oracle {ref.oracle_best:.1e})")
    assert worst <= ref.tol, (f"{where}: log posterior off by {worst:.3e} relative to the best pair (tolerance {ref.tol:.3e}, oracle "
                              f"{ref.oracle_deviation:.3e}) at position {k} of the list; {psc.place_of_pair(case.G, *model.sequence[k])}")
    # the normaliser
    assert abs(float(posteriors.sum()) - 1) < 1e-9, where
    assert abs(d_best) <= ref.tol + ref.oracle_best, f"{where}: the best pair's log posterior is off by {d_best:.3e}"


@pytest.mark.parametrize("route,case", ROUTE_CASES, ids=lambda x: x if isinstance(x, str) else x.name)
def test_a_case_alone_gives_the_bits_of_the_batch(hip_ctx, table, route, case):
    assert _same_bits(_alone(hip_ctx, table, route, case), _together(hip_ctx, table, route)[case.name]), (route, case.name)


@pytest.mark.parametrize("route", list(psc.ROUTES))
def test_two_runs_give_the_same_bits(hip_ctx, table, route):
    cases = psc.cases_of(route)
    first = _together(hip_ctx, table, route)
    for case, again in zip(cases, _search(hip_ctx, table, cases, route)):
        assert _same_bits(again, first[case.name]), (route, case.name)


def test_a_cluster_listed_twice_gives_the_same_bits_twice(hip_ctx, table):
    listings = {"tiles": ("rows_64x1025", "cols_65", "rows_64x1025", "classes_12_ends_in_different_chunks", "cols_1025", "cols_65"),
                "chunk256": ("rows_88x513", "classes_64_ends_on_chunk_edges", "rows_88x513", "rows_12x257"),
                "table": ("rows_88x2049", "cols_97", "rows_88x2049"),
                "walk": ("rows_129x513", "cols_208", "rows_129x513")}
    for route, names in listings.items():
        listed = [psc.BY_NAME[n] for n in names]
        assert len(set(names)) < len(names) and all(route in c.routes for c in listed)
        for case, got in zip(listed, _search(hip_ctx, table, listed, route)):
            assert _same_bits(got, _together(hip_ctx, table, route)[case.name]), (route, case.name)
