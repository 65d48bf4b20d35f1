"""rpvg_hip_group_loglik, rpvg_hip_group_conditionals and rpvg_hip_group_full_posteriors against the long-double model of
tests/set_loglik_cases.py, on matrices that stand on the edges of their mechanisms: the ends of the row classes, the lane
strides, the segments between two folds of the running products, the candidate clamp, the rank <-> members arithmetic and the
256-thread normalisation.

Every case meets, on the CPU (tests/test_set_loglik_cases.py): the FP64 reference agrees with the model; the posteriors of an
enumeration span at most 650 log units (but in the underflow case); removing any row or reading any named column's neighbour
moves some output by at least 1 000 tolerances; a row class left out, a clamp that reads column G - 1 for a live candidate and a
product that is never folded miss by as much.  The tolerance of a case is 8 x the largest deviation of the FP64 reference
(oracle/np_oracle.py: rows added one after the other) from the model on that case, at least 2^-50 max |ll| — measured against
the reference, never against the device.  No output is skipped, masked or floored.  Before anything is compared the built
matrix of every case is downloaded and its counts and noise are held to the class ends the case names: a case cannot quietly
miss its edge.  The tests print the device's worst deviation per case in tolerances (pytest -s); the MI355X figures are in
docs/design/parity.md, item 21.
"""
import numpy as np
import pytest

from oracle import np_oracle
from tests import set_loglik_cases as slc

pytestmark = pytest.mark.gpu

SET_CASES = slc.cases_of("sets")
FULL_PROBLEMS = [(case, g) for case in slc.cases_of("full") for g in case.full]
NORMALISED = ("loglik_count_1_rows_7680", "loglik_count_1_rows_7681", "multi_count_1_rows_1920", "multi_count_1_rows_1921", "counts_8_and_9")


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case a cluster of its own, uploaded as one batch."""
    dev = hip_ctx.upload(slc.batch_of(slc.CASES))
    yield dev
    dev.free()


def _groups(hip_ctx, table, cases, normalise=False):
    """The matrices of `cases`: column c = path c alone, no row collapse."""
    return hip_ctx.groups(table, [slc.INDEX[c.name] for c in cases], [[[p] for p in range(c.G)] for c in cases], normalise)


def _assert_the_matrix_stands_on_its_edge(dg, m, case):
    """The matrix as the kernels read it: the rows of the case ordered by class, the class ends where the case names them."""
    M, noise, counts, _ = case.matrix()
    values, got_noise, rowmax, got_counts = dg.rows(m)
    classes = np.array([slc.row_class(c, z) for c, z in zip(got_counts, got_noise)])
    assert np.all(np.diff(classes) >= 0), case.name
    fast_end, mid_end = int(np.sum(classes == 0)), int(np.sum(classes < slc.MID_MAX_COUNT))
    if case.ends is not None:
        assert (fast_end, mid_end) == case.ends, case.name
    perm, want_fast, want_mid = slc.device_rows(counts, noise)
    assert (fast_end, mid_end) == (want_fast, want_mid), case.name
    assert np.array_equal(values, M[perm]) and np.array_equal(got_noise, noise[perm]) and np.array_equal(got_counts, counts[perm]), case.name
    assert np.array_equal(rowmax, M[perm].max(axis=1)), case.name


def _set_sums(hip_ctx, table, cases, check_rows=False, normalise=False, requests=None):
    """One groups object; per width one call of rpvg_hip_group_loglik and one of rpvg_hip_group_conditionals with the requests of
    all `cases`.  Returns ({case name: {("loglik", w): [requests], ("conditionals", w): [requests x G]}}, the matrices of
    dg.rows() where asked for)."""
    dg = _groups(hip_ctx, table, cases, normalise)
    try:
        rows = {}
        if check_rows or normalise:
            for m, case in enumerate(cases):
                if check_rows:
                    _assert_the_matrix_stands_on_its_edge(dg, m, case)
                rows[case.name] = dg.rows(m)
        num_cols = [c.G for c in cases]
        out = {case.name: {} for case in cases}
        for w in slc.WIDTHS:
            reqs = [(m, members, rowmax) for m, case in enumerate(cases) for members, rowmax in slc.loglik_requests(case, w)]
            got = dg.loglik([r[0] for r in reqs], [r[1] for r in reqs], float(w), add_rowmax=[r[2] for r in reqs])
            at = 0
            for case in cases:
                n = len(slc.loglik_requests(case, w))
                out[case.name][("loglik", w)] = got[at:at + n]
                at += n
            reqs = [(m, others) for m, case in enumerate(cases) for others in slc.conditional_requests(case, w)]
            got = dg.conditionals([r[0] for r in reqs], [list(r[1]) for r in reqs], w, float(w), num_cols)
            at = 0
            for case in cases:
                n = len(slc.conditional_requests(case, w))
                out[case.name][("conditionals", w)] = np.array(got[at:at + n]).reshape(n, case.G)
                at += n
        return out, rows
    finally:
        dg.free()


_JOINT = {}


def _joint(hip_ctx, table):
    """All cases of the "sets" route in one groups object and one call per entry point and width (computed once)."""
    if "sets" not in _JOINT:
        _JOINT["sets"] = _set_sums(hip_ctx, table, SET_CASES, check_rows=True)[0]
    return _JOINT["sets"]


def _flat(case, got):
    """The outputs of a case in the order of slc.outputs_of."""
    return np.concatenate([got[("loglik", w)] for w in slc.WIDTHS] + [got[("conditionals", w)].ravel() for w in slc.WIDTHS])


def _same_bits(x, y):
    return set(x) == set(y) and all(x[k].tobytes() == y[k].tobytes() for k in x)


@pytest.mark.parametrize("case", SET_CASES, ids=lambda c: c.name)
def test_every_set_sum_equals_the_model(hip_ctx, table, case):
    got = _flat(case, _joint(hip_ctx, table)[case.name])
    ref = case.reference()
    outs = slc.outputs_of(case)
    assert got.shape == ref.model.shape and not np.any(np.isnan(got))
    err = np.abs(got.astype(np.longdouble) - ref.model)
    first_conditional = sum(len(slc.loglik_requests(case, w)) for w in slc.WIDTHS)
    k = int(np.argmax(err))
    print(f"{case.name:32s} loglik {float(err[:first_conditional].max()) / ref.tol:6.3f} tol, conditionals {float(err[first_conditional:].max()) / ref.tol:6.3f} tol "
          f"(tol {ref.tol:.1e}, oracle {ref.oracle_deviation / ref.tol:5.3f} tol)")
    assert float(err[k]) <= ref.tol, (f"{case.name} ({case.R} rows, count 1 below {case.ends[0]}, counts 2 .. 8 below {case.ends[1]}; {case.G} columns): "
                                      f"{'rpvg_hip_group_loglik' if k < first_conditional else 'rpvg_hip_group_conditionals'} is off by {float(err[k]):.3e} "
                                      f"(tolerance {ref.tol:.3e}, oracle {ref.oracle_deviation:.3e}) at (members, g, add_rowmax) = {outs[k]}")


@pytest.mark.parametrize("width", slc.WIDTHS)
def test_conditionals_equal_member_list_requests(hip_ctx, table, width):
    """For every candidate column exactly what rpvg_hip_group_loglik returns for the member list (others..., candidate): the same
    sums in another association (four chains and a joint logarithm against one chain per candidate)."""
    joint = _joint(hip_ctx, table)
    reqs = [(m, others + (k,)) for m, case in enumerate(SET_CASES) for others in slc.conditional_requests(case, width) for k in range(case.G)]
    dg = _groups(hip_ctx, table, SET_CASES)
    try:
        listed = dg.loglik([r[0] for r in reqs], [r[1] for r in reqs], float(width))
    finally:
        dg.free()
    at, worst = 0, 0.0
    for case in SET_CASES:
        got = joint[case.name][("conditionals", width)].ravel()
        want = listed[at:at + len(got)]
        at += len(got)
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        assert np.allclose(got, want, rtol=1e-13, atol=0), case.name
    assert at == len(listed)
    print(f"width {width}: conditionals against member lists, worst relative difference {worst:.1e}")


def test_requests_over_matrices_of_different_widths_find_their_matrix(hip_ctx, table):
    """23 requests in one call over matrices of different numbers of columns, the last matrix of the groups object among them and
    one matrix listed twice in it: the search over item_off."""
    cases = [slc.BY_NAME[f"columns_{G}"] for G in (65, 1, 9, 2, 7, 9, 3, 8, 5, 4)]
    assert len({c.name for c in cases}) < len(cases)
    rng = np.random.default_rng(23)
    req_m = [int(m) for m in rng.integers(0, len(cases), size=22)] + [len(cases) - 1]
    req_o = [tuple(int(x) for x in rng.integers(0, cases[m].G, size=2)) for m in req_m]
    assert len(req_m) == 23 and len({cases[m].G for m in req_m}) >= 6
    dg = _groups(hip_ctx, table, cases)
    try:
        got = dg.conditionals(req_m, [list(o) for o in req_o], 3, 3.0, [c.G for c in cases])
        again = dg.conditionals(req_m, [list(o) for o in req_o], 3, 3.0, [c.G for c in cases])
    finally:
        dg.free()
    worst = 0.0
    for m, others, g, g2 in zip(req_m, req_o, got, again):
        case = cases[m]
        M, noise, counts, _ = case.matrix()
        want = slc.conditionals_model(M, noise, counts, others, 3)
        oracle = np.array([slc.oracle_set_loglik(M, noise, counts, others + (k,), 3) for k in range(case.G)])
        tol = slc.tolerance(float(np.max(np.abs(oracle - want))), float(np.max(np.abs(want))))      # the rule of the cases, on this request
        assert g.shape == (case.G,) and g.tobytes() == g2.tobytes()
        worst = max(worst, float(np.max(np.abs(g.astype(np.longdouble) - want))) / tol)
        assert np.all(np.abs(g.astype(np.longdouble) - want) <= tol), (case.name, others)
    for i in range(len(req_m)):      # a matrix listed twice (columns_9 at 2 and 5) answers the same request with the same bits
        for j in range(i):
            if cases[req_m[i]].name == cases[req_m[j]].name and req_o[i] == req_o[j]:
                assert got[i].tobytes() == got[j].tobytes()
    dg = _groups(hip_ctx, table, cases)
    try:
        twice = dg.conditionals([2, 5], [[1, 8], [1, 8]], 3, 3.0, [c.G for c in cases])
        sums = dg.loglik([2, 5, 5, 2], [[1, 8, 4]] * 4, 3.0)
    finally:
        dg.free()
    assert twice[0].tobytes() == twice[1].tobytes() and len(set(sums.tolist())) == 1
    print(f"23 requests over {len(cases)} matrices: worst {worst:.3f} tol")


@pytest.mark.parametrize("case", SET_CASES, ids=lambda c: c.name)
def test_a_case_alone_gives_the_bits_of_the_joint_call(hip_ctx, table, case):
    alone = _set_sums(hip_ctx, table, [case])[0][case.name]
    assert _same_bits(alone, _joint(hip_ctx, table)[case.name]), case.name


def test_two_runs_of_the_set_sums_give_the_same_bits(hip_ctx, table):
    first = _joint(hip_ctx, table)
    again = _set_sums(hip_ctx, table, SET_CASES)[0]
    for case in SET_CASES:
        assert _same_bits(again[case.name], first[case.name]), case.name


@pytest.mark.parametrize("name", NORMALISED)
def test_normalised_matrices_through_the_same_contraction(hip_ctx, table, name):
    """normalise=True on cases that cross a class or segment edge.  The model is evaluated on the matrix the device built
    (DeviceGroups.rows: values, noise, row maxima, counts): the contraction alone is under test, with the tolerance rule of the
    other cases applied to that matrix."""
    case = slc.BY_NAME[name]
    got, rows = _set_sums(hip_ctx, table, [case], normalise=True)
    values, noise, rowmax, counts = rows[name]
    classes = np.array([slc.row_class(c, z) for c, z in zip(counts, noise)])
    assert (int(np.sum(classes == 0)), int(np.sum(classes < slc.MID_MAX_COUNT))) == case.ends and np.all(np.diff(classes) >= 0)
    filled = values.any(axis=1)      # (a row without entries stays without)
    assert np.allclose(values[filled].sum(axis=1) + noise[filled], 1.0, rtol=1e-12) and np.sum(filled) > 0.9 * case.R
    P = np.concatenate([values, rowmax[:, None]], axis=1)      # the row maximum as the device holds it: one more column, added last
    outs = [(tuple(m) + ((case.G,) if r else ()), g) for m, g, r in slc.outputs_of(case)]
    model = np.array([slc.set_loglik_model(P, noise, counts, m, g) for m, g in outs], dtype=np.longdouble)
    oracle = np.array([slc.oracle_set_loglik(P, noise, counts, m, g) for m, g in outs])
    tol = slc.tolerance(float(np.max(np.abs(oracle - model))), float(np.max(np.abs(model))))
    err = np.abs(_flat(case, got[name]).astype(np.longdouble) - model)
    print(f"{name:32s} normalised: worst {float(err.max()) / tol:6.3f} tol (tol {tol:.1e})")
    assert float(err.max()) <= tol, (name, outs[int(np.argmax(err))], float(err.max()), tol)


# ---- the enumeration ------------------------------------------------------------------------------------------------------------------

def _enumerate(hip_ctx, table, problems, check_rows=False):
    """One groups object over the matrices of `problems` [(case, g)] as listed (a case named twice is listed twice); one call of
    rpvg_hip_group_full_posteriors per group size with every problem of that size.  Returns the posteriors per problem."""
    cases = [case for case, _ in problems]
    dg = _groups(hip_ctx, table, cases)
    try:
        if check_rows:
            for m, case in enumerate(cases):
                _assert_the_matrix_stands_on_its_edge(dg, m, case)
        out = [None] * len(problems)
        for g in sorted({g for _, g in problems}):
            which = [m for m, (_, size) in enumerate(problems) if size == g]
            got = dg.full_posteriors(which, g, [np_oracle.log_freqs(cases[m].matrix()[3]) for m in which], [c.G for c in cases])
            for m, posteriors in zip(which, got):
                out[m] = posteriors
        return out
    finally:
        dg.free()


def _joint_full(hip_ctx, table):
    if "full" not in _JOINT:
        _JOINT["full"] = _enumerate(hip_ctx, table, FULL_PROBLEMS, check_rows=True)
    return _JOINT["full"]


@pytest.mark.parametrize("case,g", FULL_PROBLEMS, ids=lambda x: x.name if isinstance(x, slc.SetCase) else f"sets_of_{x}")
def test_every_posterior_equals_the_model(hip_ctx, table, case, g):
    posteriors = _joint_full(hip_ctx, table)[FULL_PROBLEMS.index((case, g))]
    ref = case.reference().full[g]
    where = f"{case.name}: {case.R} rows, {case.G} columns, {len(ref.sets)} sets of {g}"
    assert posteriors.shape == (len(ref.sets),) and not np.any(np.isnan(posteriors)), where
    # what the model puts below exp(-760) is exactly 0 (the underflow case alone has such sets); everything else is compared
    assert np.all(posteriors[~ref.kept] == 0) and np.all(posteriors[ref.kept] > 0), where
    worst, k, d_best = slc.full_deviation(ref.log_posterior, posteriors, ref.kept)
    print(f"{case.name:32s} sets of {g}: worst |d_k - d_best| {worst / ref.tol:6.3f} tol (oracle {ref.oracle_deviation / ref.tol:5.3f} tol, tol {ref.tol:.1e}), "
          f"|d_best| {abs(d_best):.1e} (oracle {ref.oracle_best:.1e})")
    assert worst <= ref.tol, (f"{where}: log posterior off by {worst:.3e} relative to the best set (tolerance {ref.tol:.3e}, oracle "
                              f"{ref.oracle_deviation:.3e}) at rank {k} = {ref.sets[k]}; rank_of_members gives {slc.rank_of_members(case.G, ref.sets[k])}")
    # the normaliser
    assert abs(float(posteriors.sum()) - 1) < 1e-9, where
    assert abs(d_best) <= ref.tol + ref.oracle_best, f"{where}: the best set's log posterior is off by {d_best:.3e}"


@pytest.mark.parametrize("case,g", FULL_PROBLEMS, ids=lambda x: x.name if isinstance(x, slc.SetCase) else f"sets_of_{x}")
def test_an_enumeration_alone_gives_the_bits_of_the_joint_call(hip_ctx, table, case, g):
    alone = _enumerate(hip_ctx, table, [(case, g)])[0]
    assert alone.tobytes() == _joint_full(hip_ctx, table)[FULL_PROBLEMS.index((case, g))].tobytes(), (case.name, g)


def test_two_runs_of_the_enumeration_give_the_same_bits(hip_ctx, table):
    first = _joint_full(hip_ctx, table)
    for (case, g), a, b in zip(FULL_PROBLEMS, _enumerate(hip_ctx, table, FULL_PROBLEMS), first):
        assert a.tobytes() == b.tobytes(), (case.name, g)


def test_a_matrix_listed_twice_is_enumerated_to_the_same_bits_twice(hip_ctx, table):
    names = [("full_23_columns_sets_of_3", 3), ("full_9_columns_sets_of_3", 3), ("full_23_columns_sets_of_3", 3), ("full_underflow", 3),
             ("full_1_columns", 3), ("full_9_columns_sets_of_3", 3)]
    problems = [(slc.BY_NAME[n], g) for n, g in names]
    assert len(set(names)) < len(names)
    joint = _joint_full(hip_ctx, table)
    for problem, got in zip(problems, _enumerate(hip_ctx, table, problems)):
        assert got.tobytes() == joint[FULL_PROBLEMS.index(problem)].tobytes(), problem[0].name
