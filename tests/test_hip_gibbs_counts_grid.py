"""-n > 0 read-count Gibbs samples (gibbsReadCountSampler, src/path_abundance_estimator.cpp:116-212) for clusters too wide or
too large for one workgroup: rpvg_hip_gibbs_read_counts sends such a problem over the whole GPU, one round of launches per
Gibbs iteration (rpvg_amd/csrc/gibbs_grid.hip).  A forced threshold (RPVG_HIP_EM_GRID_MIN_WORK, read per call) makes small
clusters take that route.  Parity with the CPU oracle is statistical; the margins are those of
tests/test_hip_models.py::test_gibbs_read_count_samples_transcripts.
"""
import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import ClusterBatch, make_params
from tests import large_cases, small_cases
from tests.test_hip_large_clusters import _compare, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def short_rows_batch():
    """3 000 rows x 40 paths, three paths per row: a thread per row, twelve workgroups."""
    return large_cases.cluster_batch(3000, 40, 3, seed=31, noise_only_frac=0.01)


def _only_block(est):
    assert len(est.gibbs_samples) == 1
    ids, noise, ab = est.gibbs_samples[0]
    return ids, noise, ab


def _assert_conserved(noise, ab, total):
    assert np.all(ab >= 0) and np.all(noise >= 0)
    assert np.all(np.abs(ab.sum(axis=1) + noise - total) <= 1e-9 * total)


def _assert_means(ga, ra, total):
    n, width = ga.shape
    se = np.sqrt(ga.var(axis=0, ddof=1) / n + ra.var(axis=0, ddof=1) / n)
    limit = 5 * se + 0.02 * total / max(1, width) + 0.5
    diff = np.abs(ga.mean(axis=0) - ra.mean(axis=0))
    print("means: worst fraction of the limit", float(np.max(diff / limit)))
    assert np.all(diff <= limit)


def _assert_spreads(ga, ra):
    sg, sr = ga.std(axis=0, ddof=1), ra.std(axis=0, ddof=1)
    big = sr > 1.0
    assert big.any()
    print("spreads: ratio range", float(np.min(sg[big] / sr[big])), float(np.max(sg[big] / sr[big])))
    assert np.all(sg[big] < 1.6 * sr[big]) and np.all(sg[big] > 0.6 * sr[big])


def _assert_scatter_around_em(ga, abundances, total):
    n = ga.shape[0]
    sg = ga.std(axis=0, ddof=1)
    assert np.all(np.abs(ga.mean(axis=0) - abundances) <= 6 * sg / np.sqrt(n) + 0.05 * total + 1.0)


def test_wide_cluster_is_sampled_over_the_whole_gpu(engine):
    """10 400 paths: more columns than the one-workgroup sampler's LDS holds (the call was an error).  Far below the size
    threshold, so only its width sends it to the grid route.  The columns no row touches always have count 0, so their share
    of the mass in a recorded state is Beta(E, T + C + 1 - E) whatever the chain does elsewhere: an exact law that catches
    counts or gamma draws on the wrong column, a noise column that moved and a wrong normalisation."""
    batch = large_cases.cluster_batch(400, 10400, 3, seed=31, noise_only_frac=0.01, max_count=400)
    n = 40
    got, stats = _run(engine, "transcripts", make_params(num_gibbs_samples=n, gibbs_thin_its=1, max_em_its=5, rng_seed=5), batch)
    ref, _ = pyoracle.run("transcripts", make_params(max_em_its=5), batch, 1)
    _compare(got, ref)
    ids, noise, ab = _only_block(got[0])
    paths = 10400
    assert ids == tuple(range(paths)) and ab.shape == (n, paths) and noise.shape == (n,)
    total = got[0].total_count
    _assert_conserved(noise, ab, total)
    assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n
    untouched = np.setdiff1d(np.arange(paths), np.unique(batch.path_idx))
    E = len(untouched)
    assert E > 9000 and total == float(batch.row_count.sum())
    m = E / (total + paths + 1)
    sd = np.sqrt(m * (1 - m) / (total + paths + 2))
    share = ab[:, untouched].sum(axis=1) / total
    print("share of the untouched columns: worst sample (sd)", float(np.max(np.abs(share - m)) / sd), "mean (se)",
          float(abs(share.mean() - m) / (sd / np.sqrt(n))))
    assert np.all(np.abs(share - m) <= 6 * sd)
    assert abs(share.mean() - m) <= 6 * sd / np.sqrt(n)


def test_wide_cluster_with_long_rows(engine, monkeypatch):
    """The wavefront-per-row kernel with the columns in global memory: 4 200 paths (more than a workgroup of the grid route
    keeps in LDS; the forced threshold sends the cluster there), 64 per row, rows of up to 400 reads (categorical draws and
    chains of binomials), three rows without a path.  Chains on long rows with large counts mix slowly (at this shape with
    200 rows the oracle misses the means margin against itself), so the check is the exact law of the untouched columns,
    which does not care how the chain mixes: 6 sd per sample and 6 standard errors for the mean, as for the 10 400-path
    cluster above (the oracle alone over seven seeds: at most 2.8 sd and 1.5 standard errors)."""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "1000")
    paths, n = 4200, 40
    batch = large_cases.cluster_batch(40, paths, 64, seed=31, noise_only_frac=0.1, max_count=400)
    assert np.any(batch.row_count <= 64) and np.any(batch.row_count > 64) and np.any(batch.row_noise == 1.0)
    got, stats = _run(engine, "transcripts", make_params(num_gibbs_samples=n, gibbs_thin_its=1, max_em_its=5, rng_seed=5), batch)
    ref, _ = pyoracle.run("transcripts", make_params(max_em_its=5), batch, 1)
    _compare(got, ref)
    ids, noise, ab = _only_block(got[0])
    assert ab.shape == (n, paths)
    total = got[0].total_count
    _assert_conserved(noise, ab, total)
    assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n
    untouched = np.setdiff1d(np.arange(paths), np.unique(batch.path_idx))
    E = len(untouched)
    assert E > 2000
    m = E / (total + paths + 1)
    sd = np.sqrt(m * (1 - m) / (total + paths + 2))
    share = ab[:, untouched].sum(axis=1) / total
    print("share of the untouched columns: worst sample (sd)", float(np.max(np.abs(share - m)) / sd), "mean (se)",
          float(abs(share.mean() - m) / (sd / np.sqrt(n))))
    assert np.all(np.abs(share - m) <= 6 * sd)
    assert abs(share.mean() - m) <= 6 * sd / np.sqrt(n)


def test_short_rows_take_the_thread_per_row_kernel(engine, monkeypatch, short_rows_batch):
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    n, thin = 300, 3
    params = make_params(num_gibbs_samples=n, gibbs_thin_its=thin, rng_seed=5)
    got, stats = _run(engine, "transcripts", params, short_rows_batch)
    ref, _ = pyoracle.run("transcripts", params, short_rows_batch, 1)
    _compare(got, ref)
    (gi, gn, ga), (ri, rn, ra) = _only_block(got[0]), _only_block(ref[0])
    assert gi == ri and ga.shape == ra.shape == (n, 40) and gn.shape == (n,)
    total = got[0].total_count
    _assert_conserved(gn, ga, total)
    _assert_means(ga, ra, total)
    _assert_spreads(ga, ra)
    _assert_scatter_around_em(ga, got[0].abundances, total)
    assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n * thin


def test_long_rows_take_the_wavefront_per_row_kernel(engine, monkeypatch):
    """128 entries per row, at most four reads per row: the lanes stride the entries and the reads are categorical draws over
    the wave's prefix sums.  (No scatter-around-EM check: with 128 columns and gamma = 1 the prior's pseudo-counts move the
    posterior mean off the EM mode, and the reference itself is 1.9x outside that margin.)"""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    batch = large_cases.cluster_batch(600, 128, 128, seed=31, noise_only_frac=0.01)
    n, thin = 400, 5
    params = make_params(num_gibbs_samples=n, gibbs_thin_its=thin, rng_seed=5)
    got, stats = _run(engine, "transcripts", params, batch)
    ref, _ = pyoracle.run("transcripts", params, batch, 1)
    _compare(got, ref)
    (gi, gn, ga), (ri, rn, ra) = _only_block(got[0]), _only_block(ref[0])
    assert gi == ri and ga.shape == ra.shape == (n, 128)
    total = got[0].total_count
    _assert_conserved(gn, ga, total)
    _assert_means(ga, ra, total)
    _assert_spreads(ga, ra)
    assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n * thin


def test_long_rows_with_large_counts(engine, monkeypatch):
    """Up to 300 reads per row over 96 entries: rows of more than 64 reads keep the chain of binomials (and reach the
    binomial's walk from the mode), the others are categorical.  The chain mixes slowly: thinned by 25, means only (at a
    thinning of 4 the reference fails the means check against itself)."""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    batch = large_cases.cluster_batch(300, 96, 96, seed=31, noise_only_frac=0.01, max_count=300)
    n, thin = 200, 25
    params = make_params(num_gibbs_samples=n, gibbs_thin_its=thin, rng_seed=5)
    got, stats = _run(engine, "transcripts", params, batch)
    ref, _ = pyoracle.run("transcripts", params, batch, 1)
    _compare(got, ref)
    (gi, gn, ga), (ri, rn, ra) = _only_block(got[0]), _only_block(ref[0])
    assert gi == ri and ga.shape == ra.shape == (n, 96)
    total = got[0].total_count
    _assert_conserved(gn, ga, total)
    _assert_means(ga, ra, total)
    assert stats["gibbs_count_grid_problems"] == 1 and stats["gibbs_count_grid_iterations"] == n * thin


def test_co_members_of_a_grid_problem_keep_their_bits(engine, monkeypatch, short_rows_batch):
    """Six small clusters and a cluster that takes the grid route: the small ones run on the one-workgroup kernel under their
    own indices either way."""
    small = ClusterBatch.from_clusters(small_cases.make_batch_clusters(811, n_clusters=6, with_empty=False))
    batch = ClusterBatch.concat([small, short_rows_batch])
    params = make_params(num_gibbs_samples=20, gibbs_thin_its=3, rng_seed=1)
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    with_grid, stats_grid = _run(engine, "transcripts", params, batch)
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "0")
    without, stats_without = _run(engine, "transcripts", params, batch)
    assert stats_grid["gibbs_count_grid_problems"] == 1 and stats_without["gibbs_count_grid_problems"] == 0
    assert len(with_grid) == len(without) == 7
    for a, b in zip(with_grid[:6], without[:6]):
        (ai, an, aa), (bi, bn, ba) = _only_block(a), _only_block(b)
        assert ai == bi and aa.shape[0] == 20
        assert np.array_equal(an, bn) and np.array_equal(aa, ba)
    for est in (with_grid[6], without[6]):
        ids, noise, ab = _only_block(est)
        assert ab.shape == (20, 40)
        _assert_conserved(noise, ab, est.total_count)


def test_grid_samples_depend_on_the_seed_and_the_data_alone(monkeypatch, short_rows_batch):
    """The same cluster as the only problem of a call and as the fourth behind three small ones, with the same seed: the same
    samples bit for bit."""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    small = ClusterBatch.from_clusters(small_cases.make_batch_clusters(811, n_clusters=3, with_empty=False))
    mixed = ClusterBatch.concat([small, short_rows_batch])

    def columns(b):
        return [list(range(int(b.cluster_path_off[k + 1] - b.cluster_path_off[k]))) for k in range(b.num_clusters)]

    n, thin = 12, 2
    ctx = hip.Context(0)
    try:
        alone = ctx.upload(short_rows_batch)
        abund, noise, total, _ = ctx.em_solve(alone, [0], columns(short_rows_batch))
        ctx.reset_stats()
        first = ctx.gibbs_read_counts(alone, [0], columns(short_rows_batch), abund, noise, [n], [77], thin)
        again = ctx.gibbs_read_counts(alone, [0], columns(short_rows_batch), abund, noise, [n], [77], thin)
        other = ctx.gibbs_read_counts(alone, [0], columns(short_rows_batch), abund, noise, [n], [78], thin)
        assert ctx.stats()["gibbs_count_grid_problems"] == 3 and ctx.stats()["gibbs_count_grid_iterations"] == 3 * n * thin
        alone.free()
        dev = ctx.upload(mixed)
        abund4, noise4, _, _ = ctx.em_solve(dev, [0, 1, 2, 3], columns(mixed))
        ctx.reset_stats()
        behind = ctx.gibbs_read_counts(dev, [0, 1, 2, 3], columns(mixed), list(abund4[:3]) + [abund[0]], list(noise4[:3]) + [noise[0]],
                                       [n] * 4, [5, 6, 7, 77], thin)
        assert ctx.stats()["gibbs_count_grid_problems"] == 1
        dev.free()
    finally:
        ctx.close()
    assert first[0][1].shape == (n, 40) and first[0][0].shape == (n,)
    _assert_conserved(first[0][0], first[0][1], total[0])
    assert np.array_equal(first[0][0], again[0][0]) and np.array_equal(first[0][1], again[0][1])
    assert np.array_equal(first[0][0], behind[3][0]) and np.array_equal(first[0][1], behind[3][1])
    assert not np.array_equal(first[0][1], other[0][1])
    for k in range(3):
        assert behind[k][1].shape[0] == n and np.all(behind[k][1] >= 0)


def test_nested_model_samples_the_subsets_of_a_large_cluster(engine, monkeypatch):
    """haplotype-transcripts: the -n samples of a cluster are split over its path subsets, and the subsets of a large cluster
    reach the grid route."""
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "5000")
    batch = large_cases.cluster_batch(30000, 24, 2, seed=9, groups=3, haplotypes=6)
    n = 20
    params = make_params(num_gibbs_samples=n, gibbs_thin_its=2, rng_seed=9)
    got, stats = _run(engine, "haplotype-transcripts", params, batch)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 1)
    _compare(got, ref)
    for g, r in zip(got, ref):
        assert sum(len(s[1]) for s in g.gibbs_samples) == sum(len(s[1]) for s in r.gibbs_samples) <= n
        subsets = set(g.em_cols)
        for ids, noise, ab in g.gibbs_samples:
            assert ids in subsets and ab.shape == (len(noise), len(ids))
            _assert_conserved(noise, ab, g.total_count)
    assert stats["gibbs_count_grid_problems"] >= 1
