"""The whole-GPU EM routes (rpvg_amd/csrc/em_grid.hip, em_dense.hip) at the edges of their launch shapes against a long-double
model (tests/em_grid_cases.py).

With RPVG_HIP_EM_GRID_MIN_WORK=1 (read per call) every problem of an rpvg_hip_em_solve call takes the grid bin.  Every case of the
table is solved alone: the statistics must show it in the grid slot on the route the restated plan names; with a fixed budget
(max_rel_em_conv = 0) it runs exactly max_em_its iterations and its abundances and noise count are within KERNEL_REL of the
model after that many; with the default rule it stops at the model's and the oracle's iteration.  KERNEL_REL is 64 x the largest
distance of the double-precision oracle from the model over the table (em_grid_cases.ORACLE_DISTANCE) — not chosen here.  Then
all cases in one call, bit-equal to each alone and to a second run, and rpvg_hip_em_dense on uploaded matrices at every switch
of its two kernels."""
import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd import hip
from tests import em_bin_cases as ebc, em_grid_cases as egc

pytestmark = pytest.mark.gpu

GRID_SLOT = ebc.GRID_BIN
ONE_CALL_ITS = egc.HEAVY_CAP


@pytest.fixture(autouse=True)
def every_problem_takes_the_grid(monkeypatch):
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "1")


@pytest.fixture(scope="module")
def table(hip_ctx):
    dev = hip_ctx.upload(ebc.batch_of([c.cluster() for c in egc.CASES]))
    yield dict(dev=dev)
    dev.free()


def _solve(hip_ctx, table, cases, max_em_its, max_rel_em_conv=1e-3):
    precision = {c.collapse_precision() for c in cases}
    assert len(precision) == 1
    return hip_ctx.em_solve(table["dev"], [egc.CASES.index(c) for c in cases], [c.cols() for c in cases], max_em_its=max_em_its,
                            max_rel_em_conv=max_rel_em_conv, collapse_precision=precision.pop())


def _solve_alone(hip_ctx, table, case, max_em_its, max_rel_em_conv=1e-3):
    """One case in a call of its own; the statistics show it in the grid slot, its iterations on the route the restated plan
    names: the CSR route counts them under the grid kernel, the dense route as launches of em_dense.hip's streaming pass."""
    hip_ctx.reset_stats()
    ab, nz, tot, its = _solve(hip_ctx, table, [case], max_em_its, max_rel_em_conv)
    stats = hip_ctx.stats()
    problems = {i: int(stats["em_kernel"][hip.em_kernel_name(i)]["problems"]) for i in range(hip.EM_KERNELS)}
    assert problems == {i: int(i == GRID_SLOT) for i in range(hip.EM_KERNELS)}, (case.name, problems)
    dense = egc.dense_rule(*case.shape())
    assert dense == (case.route == "dense")
    assert int(stats["em_dense_launches"]) == (int(its[0]) if dense else 0), case.name
    assert int(stats["em_kernel"][hip.em_kernel_name(GRID_SLOT)]["iterations"]) == (0 if dense else int(its[0])), case.name
    return ab[0], float(nz[0]), float(tot[0]), int(its[0])


def _check_model(name, ab, nz, want):
    """Within KERNEL_REL of the model: every component the model keeps, and the noise count — through which the components
    the model puts below 1e-8 are compared (they must be reported as 0)."""
    assert want.gap > 1e-6, (name, want.gap)   # (no component within reach of the 1e-8 line: the model's verdicts are the kernel's)
    d = egc.distance(ab, nz, want)
    print(f"{name:28s} iterations {want.iterations:5d} distance {d:.2e} (bound {egc.KERNEL_REL:.2e})")
    assert np.all(np.asarray(ab)[~want.live] == 0), name
    assert d <= egc.KERNEL_REL, (name, d)


@pytest.mark.parametrize("case", egc.CASES, ids=lambda c: c.name)
def test_fixed_budget_alone_matches_the_model(hip_ctx, table, case):
    ab, nz, tot, its = _solve_alone(hip_ctx, table, case, egc.FIXED_BUDGET, 0.0)
    want = case.model().run(egc.FIXED_BUDGET, 0.0)
    assert its == egc.FIXED_BUDGET and tot == float(want.total)
    _check_model(case.name, ab, nz, want)


@pytest.mark.parametrize("budget", egc.CHUNK_BUDGETS)
@pytest.mark.parametrize("name", egc.BUDGET_CASES)
def test_budgets_around_the_chunks_of_queued_iterations(hip_ctx, table, name, budget):
    """The CSR route queues 32 iterations per chunk with two chunks in flight, the dense route 8: the loop stops at exactly
    the budget on both sides of one and of two chunks."""
    case = egc.BY_NAME[name]
    chunk = case.launch_shape()["chunk_its"]
    assert chunk == (egc.DENSE_CHUNK_ITS if case.route == "dense" else 32)
    ab, nz, tot, its = _solve_alone(hip_ctx, table, case, budget, 0.0)
    assert its == budget
    _check_model(f"{name} budget {budget}", ab, nz, case.model().run(budget, 0.0))


_ORACLE_ITS = {}


@pytest.mark.parametrize("case", egc.CASES, ids=lambda c: c.name)
def test_convergence_alone_stops_at_the_models_iteration(hip_ctx, table, case):
    ab, nz, tot, its = _solve_alone(hip_ctx, table, case, case.max_em_its)
    want = case.model().run(case.max_em_its)
    if case.name not in _ORACLE_ITS:
        Pn, counts = case.inputs()
        _ORACLE_ITS[case.name] = pyoracle.em_dense(Pn, counts, case.max_em_its)[3]
    assert its == want.iterations == _ORACLE_ITS[case.name], (case.name, its, want.iterations, _ORACLE_ITS[case.name])
    assert tot == float(want.total)
    _check_model(case.name, ab, nz, want)
    assert abs(ab.sum() + nz - tot) <= 1e-9 * tot, case.name


@pytest.mark.parametrize("collapsed", [False, True], ids=["plain", "collapsed"])
def test_all_cases_in_one_call_equal_each_alone_and_a_second_run(hip_ctx, table, collapsed):
    """Several CSR problems share the two grid streams, and the pool hands buffers on between the dense problems: every
    result bit-equal to the case alone, and to a second run of the call."""
    cases = [c for c in egc.CASES if c.collapse == collapsed]
    assert len(cases) >= 2 and {c.route for c in cases} == {"csr", "dense"}
    hip_ctx.reset_stats()
    first = _solve(hip_ctx, table, cases, ONE_CALL_ITS)
    stats = hip_ctx.stats()
    assert int(stats["em_kernel"][hip.em_kernel_name(GRID_SLOT)]["problems"]) == len(cases)
    assert int(stats["em_dense_launches"]) == sum(int(n) for c, n in zip(cases, first[3]) if c.route == "dense")
    assert int(stats["em_kernel"][hip.em_kernel_name(GRID_SLOT)]["iterations"]) == sum(int(n) for c, n in zip(cases, first[3]) if c.route == "csr")
    second = _solve(hip_ctx, table, cases, ONE_CALL_ITS)
    for k, c in enumerate(cases):
        alone = _solve(hip_ctx, table, [c], ONE_CALL_ITS)
        for other, what in ((second, k), (alone, 0)):
            assert np.array_equal(first[0][k], other[0][what]), c.name
            assert first[1][k] == other[1][what] and first[2][k] == other[2][what] and first[3][k] == other[3][what], c.name
        assert int(first[3][k]) == c.model().run(ONE_CALL_ITS).iterations, c.name


# ---- the raw dense ABI ---------------------------------------------------------------------------------------------------
def _raw_dense(hip_ctx, Pn, counts, ld, budget):
    R, C = Pn.shape
    matrix = Pn if ld == C else egc.padded(Pn, ld)
    d_matrix, d_counts = hip_ctx.malloc(8 * R * ld), hip_ctx.malloc(8 * R)
    try:
        hip_ctx.h2d(d_matrix, matrix)
        hip_ctx.h2d(d_counts, counts)
        return hip_ctx.em_dense(d_matrix, R, C, ld, d_counts, float(counts.sum()), max_em_its=budget, max_rel_em_conv=0.0)
    finally:
        hip_ctx.free(d_matrix)
        hip_ctx.free(d_counts)


def _check_raw(hip_ctx, C, R):
    Pn, counts = egc.raw_dense_problem(1000 * C + R, R, C)
    assert 0.35 < float((Pn[:, :-1] == 0).mean()) < 0.65 or R * (C - 1) < 64
    assert np.all(Pn[:, -1] > 0) and counts.max() == 1_000_000 and (R < 4 or (counts == 0).any())
    want = egc.EmModel(Pn, counts).run(egc.FIXED_BUDGET, 0.0)
    assert want.iterations == egc.FIXED_BUDGET
    min_ld = (C + 1) & ~1
    for ld in (min_ld, min_ld + 2):   # the smallest stride, and one with two more cells per row: every padding cell NaN
        ab, nz, its = _raw_dense(hip_ctx, Pn, counts, ld, egc.FIXED_BUDGET)
        assert its == egc.FIXED_BUDGET
        _check_model(f"raw C {C} R {R} ld {ld}", ab, nz, want)


@pytest.mark.parametrize("C", egc.RAW_COLUMNS)
def test_raw_dense_abi_at_every_switch_of_its_kernels(hip_ctx, C):
    """emDenseAccumKernel<1|2> up to 256 columns, emDenseAccumWideKernel<1..4> above: an odd C with its padding column,
    ld > C, a single row, an odd row count in the wide kernel (two rows per trip), fewer partials than the 16 reduce slices,
    zero counts and zero cells."""
    for R in egc.RAW_ROWS:
        _check_raw(hip_ctx, C, R)


@pytest.mark.parametrize("R", egc.RAW_CAP_ROWS)
@pytest.mark.parametrize("C", egc.RAW_CAP_COLUMNS)
def test_raw_dense_abi_at_the_grid_cap(hip_ctx, C, R):
    """2 048 rows fill the grid of both kernels (512 workgroups of four wavefronts a row each; 1 024 workgroups of two rows):
    one row fewer, and one more — a second trip for one wavefront, or for the first workgroup with the other half of its
    double-buffered row sums."""
    _, cus, _ = hip_ctx.info()
    shape = egc.dense_launch_shape(C, R, cus)
    if cus == egc.CUS:
        assert shape["grid"] == (1024 if C > 256 else 512)
    _check_raw(hip_ctx, C, R)


def test_raw_dense_abi_refuses_2049_columns(hip_ctx):
    Pn, counts = egc.raw_dense_problem(7, 3, 2049)
    with pytest.raises(hip.EngineError, match="exceed the register-resident row limit"):
        _raw_dense(hip_ctx, Pn, counts, 2050, egc.FIXED_BUDGET)
