"""rpvg_hip_em_solve at the edges of its size bins (tests/em_bin_cases.py) against the CPU oracle.

Every case is solved alone: the statistics must show it in the bin the Python restatement of emBinOf names, its iteration
count and read total must equal the oracle's, its abundances and noise must be within 1e-7 relative.  Then all cases go
into one call next to thousands of problems of the LDS-resident and register-resident bins — more than their persistent
workgroups, so that one workgroup solves a large problem and then smaller ones in the same LDS — and every result must
be bit-equal to the same problem solved alone.  The register bins in one launch and in five, the move of 8 (not 9)
mid-size problems to the grid, and the nested model's subset EM on both sides of its 3991-path line close the file.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import make_params
from tests import em_bin_cases as ebc, large_cases, small_cases

pytestmark = pytest.mark.gpu

REL = 1e-7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_CALL_ITS = 300   # the iteration cap of the calls that hold many problems (one cap per call)


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case of the table and the fillers of the persistent bins, uploaded as one batch."""
    clusters = [c.cluster() for c in ebc.CASES]
    filler_cases = {b: ebc.fillers(b) for b in (0, 1, 7) + ebc.REGISTER_BINS}
    filler_index = {}
    for b, fs in filler_cases.items():
        for f in fs:
            filler_index[f.name] = len(clusters)
            clusters.append(f.cluster())
    dev = hip_ctx.upload(ebc.batch_of(clusters))
    yield dict(dev=dev, filler_cases=filler_cases, filler_index=filler_index)
    dev.free()


_ORACLE = {}


def _oracle_of(cl, cols, max_em_its):
    P, noise, counts = np_oracle.dense_matrix(cl.rows(), cl.n_paths, cols)
    Pn = np_oracle.add_noise_and_normalize(P, noise)
    ab, nc, tot, its, _ = pyoracle.em_dense(Pn, counts, max_em_its)
    return ab, nc, tot, its


def _oracle(case, max_em_its):
    key = (case.name, max_em_its)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_of(case.cluster(), case.cols(), max_em_its)
    return _ORACLE[key]


def _slot_problems(stats):
    return {i: int(stats["em_kernel"][hip.em_kernel_name(i)]["problems"]) for i in range(hip.EM_KERNELS)}


def _check_route(stats, shapes, iters):
    """The statistics of one call show every problem in the bin the restated rule names (grid problems on the dense
    sub-route: in the grid slot with no iterations of its own, the iterations as em_dense_launches).  The per-bin problem
    counts are the host's own repeat of emBinOf and of the mid-size move (accountEmSolve), not a record of what the device
    launched; em_dense_launches is: emDenseIterate counts the launches it makes for the grid problems the device described
    (the mid-size test leans on that to see emOrderKernel's own verdict)."""
    slots, dense = ebc.expected_stats(shapes)
    got = _slot_problems(stats)
    assert got == {i: slots.get(i, 0) for i in range(hip.EM_KERNELS)}, (got, slots)
    routes = ebc.routes(shapes)
    dense_its = sum(int(n) for s, b, n in zip(shapes, routes, iters) if b == ebc.GRID_BIN and ebc.dense_rule(*s))
    csr_its = sum(int(n) for s, b, n in zip(shapes, routes, iters) if b == ebc.GRID_BIN and not ebc.dense_rule(*s))
    assert stats["em_dense_launches"] == dense_its
    assert stats["em_kernel"][hip.em_kernel_name(ebc.GRID_BIN)]["iterations"] == csr_its
    return dense


def _check_oracle(case, ab, nz, tot, its, max_em_its):
    _check_against(case.name, _oracle(case, max_em_its), ab, nz, tot, its)


def _check_against(name, want, ab, nz, tot, its):
    want_ab, want_nz, want_tot, want_its = want
    assert tot == want_tot, name
    assert int(its) == want_its, (name, int(its), want_its)
    assert small_cases.rel_close(ab, want_ab, rel=REL), name
    assert abs(nz - want_nz) <= REL * max(1.0, want_tot), name
    assert abs(ab.sum() + nz - tot) <= 1e-9 * tot, name


@pytest.mark.parametrize("case", ebc.CASES, ids=lambda c: c.name)
def test_case_alone_lands_in_its_bin_and_matches_the_oracle(hip_ctx, table, case):
    i = ebc.CASES.index(case)
    hip_ctx.reset_stats()
    ab, nz, tot, its = hip_ctx.em_solve(table["dev"], [i], [case.cols()], max_em_its=case.max_em_its)
    stats = hip_ctx.stats()
    _check_route(stats, [case.shape()], its)
    _check_oracle(case, ab[0], nz[0], tot[0], its[0], case.max_em_its)
    if case.max_em_its < 10000:
        assert int(its[0]) <= case.max_em_its


MID_CALL_ITS = 60


def test_mid_size_problems_take_the_grid_when_eight_and_stay_when_nine(hip_ctx, table):
    """emOrderKernel moves the streamed problems of 2^16 - 1 rows + entries and more to the grid when a call has at most
    kEmMidGridMax = 8 of them; with nine they stay in the streamed bin.  One of them (grid_dense_lo, one unit of work below
    the grid threshold) satisfies emDenseRule: moved, it runs em_dense.hip's kernels, whose launches the statistics count
    as they are made — the device's own verdict, not the host's repeat of it.  The ninth problem is grid_csr_lo, so both
    problems just below 2^18 are also checked against the oracle in the streamed bin.  The oracle's answer either way."""
    mids = [ebc.BY_NAME[n] for n in ebc.MID_COUNT_CASES[:7]]
    lo_dense, lo_csr = ebc.BY_NAME["grid_dense_lo"], ebc.BY_NAME["grid_csr_lo"]
    for part, where in ((mids + [lo_dense], ebc.GRID_BIN), (mids + [lo_dense, lo_csr], ebc.STREAMED_BIN)):
        n = len(part)
        hip_ctx.reset_stats()
        ab, nz, tot, its = hip_ctx.em_solve(table["dev"], [ebc.CASES.index(c) for c in part], [c.cols() for c in part], max_em_its=MID_CALL_ITS)
        stats = hip_ctx.stats()
        assert all(ebc.is_mid(*c.shape()) for c in part)
        assert ebc.routes([c.shape() for c in part]) == [where] * n
        _check_route(stats, [c.shape() for c in part], its)
        assert _slot_problems(stats)[where] == n
        dense_its = int(its[n - 1 if where == ebc.GRID_BIN else n - 2])
        assert stats["em_dense_launches"] == (dense_its if where == ebc.GRID_BIN else 0)
        assert dense_its > 0
        for k, c in enumerate(part):
            _check_oracle(c, ab[k], nz[k], tot[k], its[k], MID_CALL_ITS)


def _one_call_problems(hip_ctx, table):
    """The table and the fillers (>= 3 x CUs x workgroups per CU of each persistent bin, sizes mixed), in a seeded
    shuffled order."""
    _, cus, _ = hip_ctx.info()
    probs = [(i, c.cols(), c.shape(), ("case", c.name)) for i, c in enumerate(ebc.CASES)]
    for b, fs in table["filler_cases"].items():
        reps = math.ceil(3 * cus * ebc.PER_CU[b] / len(fs))
        for f in fs:
            probs += [(table["filler_index"][f.name], f.cols(), f.shape(), ("filler", f.name))] * reps
    rng = np.random.default_rng(17)
    return [probs[j] for j in rng.permutation(len(probs))], cus


def _solve(hip_ctx, dev, probs):
    return hip_ctx.em_solve(dev, [p[0] for p in probs], [p[1] for p in probs], max_em_its=ONE_CALL_ITS)


def test_all_cases_in_one_call_equal_each_solved_alone(hip_ctx, table):
    probs, cus = _one_call_problems(hip_ctx, table)
    shapes = [p[2] for p in probs]
    in_call = ebc.routes(shapes)
    per_bin = {b: in_call.count(b) for b in set(in_call)}
    for b in (0, 1, 7) + ebc.REGISTER_BINS:
        assert per_bin[b] >= 3 * cus * ebc.PER_CU[b], (b, per_bin[b])
    dev = table["dev"]
    hip_ctx.reset_stats()
    first = _solve(hip_ctx, dev, probs)
    stats = hip_ctx.stats()
    _check_route(stats, shapes, first[3])
    second = _solve(hip_ctx, dev, probs)
    _assert_same(probs, in_call, first, second)
    # every distinct problem solved alone — or, for the mid-size problems, which a call of their own would move to the grid,
    # in a call of all of them (more than kEmMidGridMax: the streamed bin, as in the big call)
    mids = [j for j, s in enumerate(shapes) if ebc.is_mid(*s)]
    assert len(mids) > ebc.MID_GRID_MAX and all(in_call[j] == ebc.STREAMED_BIN for j in mids)
    mid_probs = list({probs[j][3]: probs[j] for j in mids}.values())
    assert ebc.routes([p[2] for p in mid_probs]) == [ebc.STREAMED_BIN] * len(mid_probs)
    alone_probs, alone_res = mid_probs, list(zip(*_solve(hip_ctx, dev, mid_probs)))
    seen = {p[3] for p in mid_probs}
    for j, p in enumerate(probs):
        if p[3] in seen:
            continue
        seen.add(p[3])
        assert ebc.routes([p[2]]) == [in_call[j]], p[3]
        alone_probs.append(p)
        alone_res.append(tuple(x[0] for x in _solve(hip_ctx, dev, [p])))
    by_key = dict(zip([p[3] for p in alone_probs], alone_res))
    _assert_same(probs, in_call, first, tuple(zip(*[by_key[p[3]] for p in probs])))


def _assert_same(probs, bins, x, y):
    """Bit-equal results — but for the wide bin, whose M-step adds into one vector in global memory with atomics, in the
    order the wavefronts happen to reach it (emSparseProblem): there the iteration count is equal and the rest within 1e-12.
    (The order of those additions could in principle move an abundance across the convergence test and change the count by
    one; at the shapes here the relative changes are far below max_rel_em_conv's margins.  If it ever flakes, this is why.)"""
    for j, p in enumerate(probs):
        if bins[j] == 10:
            assert small_cases.rel_close(x[0][j], y[0][j], rel=1e-12, floor=1e-300), p[3]
            assert abs(x[1][j] - y[1][j]) <= 1e-12 * max(1.0, x[2][j]) and x[2][j] == y[2][j] and x[3][j] == y[3][j], p[3]
        else:
            assert np.array_equal(x[0][j], y[0][j]), p[3]
            assert x[1][j] == y[1][j] and x[2][j] == y[2][j] and x[3][j] == y[3][j], p[3]


def test_fill_map_cache_switches_between_subsets_of_one_cluster(hip_ctx):
    """fillSegmentsKernel keeps the column map of the last problem it built one for (mapped_problem) and rebuilds it when
    the next item belongs to another problem.  Here four fill workgroups each take four subset problems of one cluster in
    a row (tests/em_bin_cases.py, map_cache_call: the restated grid-stride says so); the rest of the call is identity-column
    fillers.  Every subset problem must be bit-equal to itself solved alone (one item: a fresh map) and match the oracle."""
    _, cus, _ = hip_ctx.info()
    clusters, problems = ebc.map_cache_call(cus)
    assert ebc.map_switches(clusters, problems, cus) == 4 * (ebc.MAP_LANE_PROBLEMS - 1)
    dev = hip_ctx.upload(ebc.batch_of(clusters))
    try:
        together = hip_ctx.em_solve(dev, [k for k, _ in problems], [c for _, c in problems], max_em_its=ONE_CALL_ITS)
        subsets = [j for j, (k, _) in enumerate(problems) if k != 2]
        assert len(subsets) == 4 * ebc.MAP_LANE_PROBLEMS
        for j in subsets:
            k, cols = problems[j]
            ab, nz, tot, its = hip_ctx.em_solve(dev, [k], [cols], max_em_its=ONE_CALL_ITS)
            assert np.array_equal(together[0][j], ab[0]), (j, k)
            assert together[1][j] == nz[0] and together[2][j] == tot[0] and together[3][j] == its[0], (j, k)
            _check_against(f"subset {j} of cluster {k}", _oracle_of(clusters[k], cols, ONE_CALL_ITS), ab[0], nz[0], tot[0], its[0])
        filler = _oracle_of(clusters[2], problems[1][1], ONE_CALL_ITS)
        for j in (1, 2, len(problems) - 2):
            _check_against(f"filler {j}", filler, together[0][j], together[1][j], together[2][j], together[3][j])
    finally:
        dev.free()


_CHILD = (
    "import json, sys, zlib\n"
    "import numpy as np\n"
    "from rpvg_amd import hip\n"
    "from tests import em_bin_cases as ebc\n"
    "cases = [c for c in ebc.CASES if c.name.startswith(('reg_', 'one_', 'subset_'))]\n"
    "fill = [f for b in ebc.REGISTER_BINS for f in ebc.fillers(b)]\n"
    "ctx = hip.Context(0)\n"
    "_, cus, _ = ctx.info()\n"
    "dev = ctx.upload(ebc.batch_of([c.cluster() for c in cases + fill]))\n"
    "reps = -(-3 * cus * 2 // 8)\n"
    "idx = list(range(len(cases))) + [len(cases) + j for j in range(len(fill)) for _ in range(reps)]\n"
    "allc = cases + fill\n"
    "ctx.reset_stats()\n"
    "ab, nz, tot, its = ctx.em_solve(dev, idx, [allc[i].cols() for i in idx], max_em_its=2000)\n"
    "st = ctx.stats()\n"
    "slots = {i: int(st['em_kernel'][hip.em_kernel_name(i)]['problems']) for i in range(hip.EM_KERNELS)}\n"
    "want = ebc.expected_stats([allc[i].shape() for i in idx], int(sys.argv[1]))[0]\n"
    "print(json.dumps(dict(crc=[zlib.crc32(np.concatenate(ab).tobytes()), zlib.crc32(nz.tobytes()), zlib.crc32(its.tobytes())],\n"
    "                      slots=slots, want={int(k): v for k, v in want.items()}, problems=len(idx))))\n"
    "dev.free()\n"
    "ctx.close()\n")


def test_register_bins_in_one_launch_equal_five_launches():
    """RPVG_HIP_EM_REGISTER_LAUNCHES is read once per process: the register bins in one launch of emRegisterKernel (the
    default) and in five launches of emRegisterBinKernel, in child processes — abundances, noise and iterations bit-equal;
    the five launches count their problems per bin, as the table says."""
    outs = {}
    for launches in ("1", "5"):
        env = dict(os.environ)
        env.pop("RPVG_HIP_EM_REGISTER_LAUNCHES", None)
        if launches == "5":
            env["RPVG_HIP_EM_REGISTER_LAUNCHES"] = "5"
        res = subprocess.run([sys.executable, "-c", _CHILD, launches], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        outs[launches] = json.loads(res.stdout.strip().splitlines()[-1])
    one, five = outs["1"], outs["5"]
    assert one["crc"] == five["crc"]
    for out in (one, five):
        assert {int(k): v for k, v in out["slots"].items()} == {i: out["want"].get(str(i), 0) for i in range(hip.EM_KERNELS)}, out
    per_bin = {int(k): v for k, v in five["slots"].items()}
    assert all(per_bin[b] >= 1 for b in ebc.REGISTER_BINS), per_bin
    assert {int(k): v for k, v in one["slots"].items()}[ebc.REGISTER_SLOT] == sum(per_bin[b] for b in ebc.REGISTER_BINS)


def _route_counters(stats):
    return {k: stats[k] for k in ("build_launches", "em_sparse_launches", "em_dense_launches", "loglik_launches", "em_iterations_total")}


@pytest.mark.parametrize("paths,device_route", [(3991, True), (3992, False)])
def test_nested_subset_em_on_both_sides_of_its_path_limit(paths, device_route, monkeypatch):
    """rpvg_hip_nested_subset_em restates the LDS rule of the streamed bins: a cluster of up to 3991 paths takes the device
    route, one of 3992 is refused and the host runs the separate calls.  Both against the oracle and against their own
    RPVG_HIP_NO_DEVICE_SUBSETS=1 run (read per call)."""
    batch = large_cases.cluster_batch(300, paths, 3, seed=paths, groups=4, haplotypes=3)
    params = make_params(max_em_its=50)
    eng = eng_mod.Engine(0)
    try:
        prep = eng.prepare(batch)
        monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
        eng.reset_stats()
        fused, _ = eng.run("haplotype-transcripts", params, prep)
        fused_stats = _route_counters(eng.stats())
        monkeypatch.setenv("RPVG_HIP_NO_DEVICE_SUBSETS", "1")
        eng.reset_stats()
        separate, _ = eng.run("haplotype-transcripts", params, prep)
        separate_stats = _route_counters(eng.stats())
        monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS")
        prep.free()
    finally:
        eng.close()
    # the refused call leaves the host route: the same launches as with RPVG_HIP_NO_DEVICE_SUBSETS=1
    assert (fused_stats != separate_stats) == device_route, (fused_stats, separate_stats)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 1)
    for f, s, r in zip(fused, separate, ref):
        fk, sk, rk = f.keyed(), s.keyed(), r.keyed()
        assert set(fk) == set(sk) == set(rk)
        assert len(rk) > 0
        for key in rk:
            assert fk[key][0] == sk[key][0], key
            assert small_cases.rel_close(fk[key][1], sk[key][1], rel=1e-12, floor=1e-300), key
            assert small_cases.rel_close(fk[key][0], rk[key][0], rel=1e-6, floor=1e-8), key
            assert small_cases.rel_close(fk[key][1], rk[key][1], rel=1e-6), key
        assert list(f.em_iters) == list(s.em_iters) and dict(zip(f.em_cols, f.em_iters)) == dict(zip(r.em_cols, r.em_iters))
        assert f.total_count == s.total_count == r.total_count
