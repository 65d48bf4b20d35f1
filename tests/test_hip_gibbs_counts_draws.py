"""The read-count Gibbs sampler (-n) against tests/gibbs_counts_model.py, draw for draw.

rpvg_hip_gibbs_read_counts is deterministic (Philox4x32-10 keyed by the problem's seed, the counter laid out in
rpvg_amd/csrc/gibbs_random.hpp, gibbsReadCountKernel and gibbs_grid.hip), so a plain restatement of its kernels follows it
exactly: the same uniforms give the same integer counts, and the recorded abundances then differ by the last bits of log,
sqrt, cospi and the order of a few sums.  Per case:

  before the sampler runs   the model's smallest decision margin (the relative distance of the two sides of any comparison that
                            chooses a branch) is at least 1e-9: the device's lgamma, exp and fused multiply-adds move a
                            threshold by ~1e-12 relative at the most, so no draw is near enough to a threshold to fall on
                            its other side there.  No draw is left out or masked.
  against the device        every recorded abundance within 1e-12 relative, every noise sample within 1e-12 of the total,
                            what the model zeroes under the 1e-8 rule exactly 0.  (A read on the wrong column changes a
                            gamma's shape by one, which moves it by at least 1e-4 relative at these counts.)

The chains start from em_solve's abundances; the routes are forced with RPVG_HIP_EM_GRID_MIN_WORK as in
tests/test_hip_gibbs_counts_grid.py, whose statistical checks against the reference stay as they are.
"""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.batch import ClusterBatch
from tests import gibbs_counts_model as model
from tests import large_cases, small_cases

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-9
TOLERANCE = 1e-12


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _columns(b):
    return [list(range(int(b.cluster_path_off[k + 1] - b.cluster_path_off[k]))) for k in range(b.num_clusters)]


def _em(ctx, batch):
    dev = ctx.upload(batch)
    abund, noise, total, _ = ctx.em_solve(dev, list(range(batch.num_clusters)), _columns(batch))
    return dev, abund, noise, total


def _assert_margin(run, what):
    m = run.margin
    print(what, "|", run.route, "| decisions", m.decisions, "smallest margin", m.smallest, "at", m.where)
    assert m.smallest >= MIN_MARGIN, "the model's run has a decision too close to its threshold: choose another seed"


def _assert_follows(device, run, total, thin, what):
    noise, ab = device
    assert ab.shape == run.abundances.shape and noise.shape == run.noise.shape
    zeroed = run.abundances == 0.0
    scale = np.where(zeroed, 1.0, run.abundances)
    rel = np.where(zeroed, np.where(ab == 0.0, 0.0, np.inf), np.abs(ab - run.abundances) / scale)
    noise_dev = np.abs(noise - run.noise)
    print(what, "| worst relative deviation of an abundance", float(rel.max()), "| of a noise sample (of the total)",
          float(noise_dev.max() / total), "| entries zeroed by the 1e-8 rule", int(zeroed.sum()))
    bad = np.argwhere(rel > TOLERANCE)
    if len(bad):
        s, j = (int(x) for x in bad[0])
        it = (s + 1) * thin
        print("first difference: iteration", it, "column", j, "model count", int(run.counts[it - 1, j]), "model", run.abundances[s, j],
              "device", ab[s, j], "| model counts of that iteration", run.counts[it - 1].tolist()[:64])
    assert len(bad) == 0
    late = np.nonzero(noise_dev > TOLERANCE * total)[0]
    if len(late):
        s = int(late[0])
        it = (s + 1) * thin
        print("first difference: iteration", it, "noise column", run.counts.shape[1] - 1, "model count", int(run.counts[it - 1, -1]), "model",
              run.noise[s], "device", noise[s])
    assert len(late) == 0
    assert np.all(ab[zeroed] == 0.0)


def _grid_case(ctx, monkeypatch, batch, seed, n, thin, route, what, kinds=()):
    """One cluster over the grid route: the model first, then the device."""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "1000")
    dev, abund, noise, total = _em(ctx, batch)
    try:
        csr = model.compacted_csr(batch, 0, _columns(batch)[0])
        assert csr.total_mass == total[0] == float(batch.row_count.sum())
        run = model.grid(csr, abund[0], noise[0], n, thin, seed)
        assert run.route == route
        _assert_margin(run, what)
        for kind in kinds:
            assert run.margin.kinds.get(kind, 0) > 0, kind
        ctx.reset_stats()
        got = ctx.gibbs_read_counts(dev, [0], _columns(batch), abund, noise, [n], [seed], thin)
        stats = ctx.stats()
        assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n * thin
    finally:
        dev.free()
    _assert_follows(got[0], run, total[0], thin, what)
    return run, got[0], abund[0], noise[0]


def test_one_workgroup_two_problems_in_one_call(ctx, monkeypatch):
    """The problem's index is in the counter.  300 x 12 x 3 with up to 400 reads per row: a thread takes two rows, the binomial
    walks from 0 and from the mode, rows without a path.  40 x 300 x 3: a thread takes two columns.  (Both clusters have rows
    without a path: with none the EM leaves a noise abundance of ~1e-12, the last entry of a row's chain then has p within
    6e-12 of 1, and p >= 1 is one of the comparisons whose margin the model records.)"""
    monkeypatch.delenv("RPVG_HIP_EM_GRID_MIN_WORK", raising=False)
    tall = large_cases.cluster_batch(300, 12, 3, seed=31, noise_only_frac=0.02, max_count=400)
    wide = large_cases.cluster_batch(40, 300, 3, seed=32, noise_only_frac=0.1)
    assert np.any(tall.row_noise == 1.0) and np.any(wide.row_noise == 1.0)
    batch = ClusterBatch.concat([tall, wide])
    n, thin, seeds = 4, 2, [77, 78]
    dev, abund, noise, total = _em(ctx, batch)
    try:
        runs = []
        for p in range(2):
            csr = model.compacted_csr(batch, p, _columns(batch)[p])
            assert csr.total_mass == total[p]
            runs.append(model.one_workgroup(csr, abund[p], noise[p], n, thin, seeds[p], p))
            _assert_margin(runs[p], "one workgroup, problem %d" % p)
        assert runs[0].margin.kinds.get("binomial u <= up", 0) > 0 and runs[0].margin.kinds.get("binomial u > pmf", 0) > 0
        ctx.reset_stats()
        got = ctx.gibbs_read_counts(dev, [0, 1], _columns(batch), abund, noise, [n, n], seeds, thin)
        assert ctx.stats()["gibbs_count_grid_problems"] == 0
    finally:
        dev.free()
    for p in range(2):
        _assert_follows(got[p], runs[p], total[p], thin, "one workgroup, problem %d" % p)


@pytest.fixture(scope="module")
def short_rows():
    return large_cases.cluster_batch(600, 40, 3, seed=31, noise_only_frac=0.01, max_count=400)


def test_grid_thread_per_row_columns_in_lds(ctx, monkeypatch, short_rows):
    _grid_case(ctx, monkeypatch, short_rows, 77, 4, 2, "grid, thread per row, columns in LDS", "600 x 40 x 3",
               kinds=("binomial u <= up", "binomial u > pmf"))


def test_grid_wavefront_per_row_columns_in_lds(ctx, monkeypatch):
    """130 entries per row: chunks of 64, 64 and 2; rows of at most 64 reads draw them one by one over the prefix sums, the
    others keep the chain of binomials, four rows have no path."""
    batch = large_cases.cluster_batch(40, 200, 130, seed=31, noise_only_frac=0.1, max_count=100)
    assert np.any(batch.row_count <= 64) and np.any(batch.row_count > 64) and np.any(batch.row_noise == 1.0)
    _grid_case(ctx, monkeypatch, batch, 77, 4, 2, "grid, wavefront per row, columns in LDS", "40 x 200 x 130",
               kinds=("categorical t < incl", "binomial u > pmf"))


def test_grid_wavefront_per_row_columns_in_global_memory(ctx, monkeypatch):
    batch = large_cases.cluster_batch(40, 4200, 64, seed=31, noise_only_frac=0.1, max_count=400)
    assert np.any(batch.row_count <= 64) and np.any(batch.row_count > 64) and np.any(batch.row_noise == 1.0)
    _grid_case(ctx, monkeypatch, batch, 77, 3, 1, "grid, wavefront per row, columns in global memory", "40 x 4200 x 64",
               kinds=("categorical t < incl", "binomial u <= up"))


def test_grid_thread_per_row_columns_in_global_memory(ctx, monkeypatch):
    batch = large_cases.cluster_batch(400, 4200, 3, seed=31, noise_only_frac=0.01, max_count=400)
    _grid_case(ctx, monkeypatch, batch, 77, 3, 1, "grid, thread per row, columns in global memory", "400 x 4200 x 3",
               kinds=("binomial u <= up", "binomial u > pmf"))


def test_grid_problem_alone_and_as_the_third_of_a_call(ctx, monkeypatch, short_rows):
    """The same samples bit for bit, and the model's: neither the problem's index nor its neighbours are in the counter."""
    run, alone, abund, noise = _grid_case(ctx, monkeypatch, short_rows, 78, 4, 2, "grid, thread per row, columns in LDS", "600 x 40 x 3, alone")
    small = ClusterBatch.from_clusters(small_cases.make_batch_clusters(811, n_clusters=2, with_empty=False))
    mixed = ClusterBatch.concat([small, short_rows])
    dev, abund3, noise3, total3 = _em(ctx, mixed)
    try:
        ctx.reset_stats()
        behind = ctx.gibbs_read_counts(dev, [0, 1, 2], _columns(mixed), list(abund3[:2]) + [abund], list(noise3[:2]) + [noise], [4] * 3,
                                       [5, 6, 78], 2)
        assert ctx.stats()["gibbs_count_grid_problems"] == 1
    finally:
        dev.free()
    assert np.array_equal(alone[0], behind[2][0]) and np.array_equal(alone[1], behind[2][1])
    _assert_follows(behind[2], run, total3[2], 2, "600 x 40 x 3, third of a call")


@pytest.mark.parametrize("gamma", [0.5, float("nan")])
def test_gamma_below_one_is_an_invalid_argument(ctx, monkeypatch, gamma):
    """sampleGamma is defined for shape >= 1 only (below, its loop need not end): the host refuses before anything is queued —
    nothing is written and no kernel is counted, on either route."""
    batch = large_cases.cluster_batch(50, 6, 3, seed=3)
    for threshold in ("0", "10"):
        monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", threshold)
        dev, abund, noise, total = _em(ctx, batch)
        try:
            ctx.reset_stats()
            before = ctx.stats()
            with pytest.raises(hip.EngineError, match=r"\(-3\).*gamma must be >= 1"):
                ctx.gibbs_read_counts(dev, [0], _columns(batch), abund, noise, [4], [77], 2, gamma=gamma)
            after = ctx.stats()
            for key in ("em_sparse_launches", "build_launches", "gibbs_count_grid_problems", "gibbs_count_grid_iterations"):
                assert after[key] == before[key], key
            # the context is as good as before
            got = ctx.gibbs_read_counts(dev, [0], _columns(batch), abund, noise, [4], [77], 2)
            assert got[0][1].shape == (4, 6) and np.all(np.isfinite(got[0][1]))
        finally:
            dev.free()
