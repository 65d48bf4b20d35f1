"""tests/gibbs_counts_model.py draws from the right laws.

The model restates the read-count Gibbs sampler's kernels draw for draw (tests/test_hip_gibbs_counts_draws.py holds the
device to it); here the model's own generator, binomial, gamma, normal and the two ways it splits a row's reads are checked
against known answers and scipy.stats, on the CPU.  alpha = 1e-6 throughout: the seeds are fixed, so a test either always
passes or always fails; a correct sampler fails a given test with that probability over the choice of the seed.
"""
import math

import numpy as np
import pytest
from scipy import stats

from tests import gibbs_counts_model as model

ALPHA = 1e-6
SEED = 0x5EED0000C0FFEE


# ---- Philox ------------------------------------------------------------------------------------------------------------

KNOWN_ANSWERS = [  # the Random123 known-answer vectors of philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr, key, expected", KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, expected):
    assert model.philox4x32_10(ctr, key) == expected
    many = model.philox4x32_10_many(np.array([ctr, ctr], dtype=np.uint64), key)
    assert [tuple(int(x) for x in row) for row in many] == [expected, expected]


def test_stream_hands_the_words_out_last_first_and_carries_the_counter():
    seed = 0x299f31d0a4093822
    s = model.Stream(seed, [0xffffffff, 5, 0x13198a2e, 2])
    assert s.key == (0xa4093822, 0x299f31d0)
    first = model.philox4x32_10((0xffffffff, 5, 0x13198a2e, 2), s.key)
    second = model.philox4x32_10((0, 6, 0x13198a2e, 2), s.key)  # ctr[0] wrapped into ctr[1]
    words = [s.next() for _ in range(8)]
    assert words == [first[3], first[2], first[1], first[0], second[3], second[2], second[1], second[0]]
    assert s.ctr == [1, 6, 0x13198a2e, 2]
    # without a wrap the second word stays
    s = model.Stream(seed, [7, 5, 1, 2])
    s.next()
    assert s.ctr == [8, 5, 1, 2]


def test_uniform_and_normal_are_built_from_the_words_as_the_kernel_builds_them():
    s, t = model.Stream(SEED, [0, 3, 9, 1]), model.Stream(SEED, [0, 3, 9, 1])
    w = [t.next() for _ in range(8)]
    u = [s.uniform() for _ in range(2)]
    assert u[0] == (float(((w[0] << 32) | w[1]) >> 11) + 0.5) * 2.0 ** -53
    assert u[1] == (float(((w[2] << 32) | w[3]) >> 11) + 0.5) * 2.0 ** -53
    assert 0.0 < min(u) and max(u) < 1.0 and s.uniforms == 2
    s = model.Stream(SEED, [0, 3, 9, 1])
    assert s.normal() == math.sqrt(-2.0 * math.log(u[0])) * model.cospi(2.0 * u[1])
    # the vectorised generator hands out the same uniforms
    many = model.uniforms_many(SEED, [9, 10], 5, domain=1, iteration=3)
    s = model.Stream(SEED, [0, 3, 9, 1])
    assert [s.uniform() for _ in range(5)] == list(many[0])
    s = model.Stream(SEED, [0, 3, 10, 1])
    assert [s.uniform() for _ in range(5)] == list(many[1])


def test_cospi_reduces_its_argument_exactly():
    assert model.cospi(0.5) == 0.0 and model.cospi(1.5) == 0.0 and model.cospi(1.0) == -1.0 and model.cospi(0.0) == 1.0
    pi = np.longdouble("3.14159265358979323846264338327950288")
    for t in (1e-9, 0.2, 0.25, 0.3, 0.5 - 1e-12, 0.5 + 1e-12, 0.75, 0.8, 1.1, 1.5 - 1e-12, 1.9, 2.0 - 1e-13):
        # (next to a zero of the cosine the extended-precision value itself has lost seven digits)
        exact = float(np.cos(pi * np.longdouble(t)))
        assert model.cospi(t) == pytest.approx(exact, rel=1e-6 if abs(exact) < 1e-9 else 1e-14, abs=0)
    t = np.array([1e-9, 0.2, 0.3, 0.6, 0.8, 1.1, 1.4, 1.9])
    assert list(model.cospi_many(t)) == [model.cospi(float(x)) for x in t]


# ---- binomial: the inversion is exact ------------------------------------------------------------------------------------

BINOMIAL_CASES = [(1, .3), (1, .7), (4, .5), (64, .2), (64, .25), (65, .25), (400, .0399), (400, .0401), (400, .5), (400, .93),
                  (300, .999), (1000, 1e-6), (100000, .3)]


@pytest.mark.parametrize("n, p", BINOMIAL_CASES)
def test_binomial_inversion_cuts_the_unit_interval_into_the_pmf(n, p):
    """The inversion maps an interval of length pmf(k) to k, so of the regular grid u = (i + 0.5) / N exactly N pmf(k), up to
    one point, land on every k.  The cases sit on both sides of the n p = 16 switch between the walk from 0 and the walk
    from the mode, on both sides of the p > 0.5 flip, at mode = 0 and at mode = n."""
    N = 20000
    grid = model.GridUniforms((i + 0.5) / N for i in range(N))
    hits = {}
    for _ in range(N):
        k, margin = model.sample_binomial(grid, n, p)
        assert 0 <= k <= n and margin >= 0.0
        hits[k] = hits.get(k, 0) + 1
    assert grid.uniforms == N  # one uniform per draw
    ks = np.arange(min(hits), max(hits) + 1)
    got = np.array([hits.get(int(k), 0) for k in ks])
    worst = float(np.max(np.abs(got - N * stats.binom.pmf(ks, n, p))))
    print("n", n, "p", p, "range", int(ks[0]), int(ks[-1]), "worst deviation from N pmf", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("n, p, expected", [(0, 0.3, 0), (7, 0.0, 0), (7, -0.25, 0), (7, float("nan"), 0), (7, 1.0, 7), (7, 1.5, 7)])
def test_binomial_corners_consume_no_uniform(n, p, expected):
    stream = model.Stream(SEED, [0, 0, 0, 0])
    k, _ = model.sample_binomial(stream, n, p)
    assert k == expected and stream.uniforms == 0 and stream.have == 0 and stream.ctr == [0, 0, 0, 0]


def test_binomial_reports_the_margin_of_its_closest_comparison():
    grid = model.GridUniforms([0.5])
    record = model.Margin()
    k, margin = model.sample_binomial(grid, 4, 0.25, record)
    # pmf(0) = 81/256: u = 0.5 passes 0 (0.5 > 0.3164) and stops in 1 (0.1836 <= 0.4219); p against 1 and 0.5 and n p against 16
    # are further from their thresholds
    assert k == 1
    assert margin == record.smallest == pytest.approx((0.5 - 81 / 256) / 0.5, rel=1e-12)
    assert record.where[0] == "binomial u > pmf" and record.decisions == 5


# ---- gamma and normal: Kolmogorov-Smirnov ------------------------------------------------------------------------------

KS_N = 1000000
KS_LIMIT = math.sqrt(math.log(2.0 / ALPHA) / (2.0 * KS_N))  # Dvoretzky-Kiefer-Wolfowitz: P(D > limit) <= alpha


def _ks(sample, cdf):
    x = np.sort(sample)
    f = cdf(x)
    n = len(x)
    return float(max(np.max(np.arange(1, n + 1) / n - f), np.max(f - np.arange(n) / n)))


@pytest.mark.parametrize("shape", [1.0, 1.5, 2.0, 17.0, 401.0, 100001.0])
def test_gamma_draws_follow_the_gamma_law(shape):
    """N = 1 000 000 streams (one draw each, as the grid's update kernel draws them), limit 0.002693.  Observed statistics:
    shape 1: 0.001647, 1.5: 0.001571, 2: 0.001522, 17: 0.001686, 401: 0.001708, 100 001: 0.001702 (the six shapes share their
    uniforms, so they move together: over the seeds 1, 2, 3 and 77 shape 17 gave 0.00110, 0.00090, 0.00065 and 0.00080)."""
    draws = model.gammas_many(SEED, shape, KS_N)
    # the vectorised loop is the scalar one
    for j in (0, 1, 2, 3, 500, KS_N - 1):
        one, margin = model.sample_gamma(model.Stream(SEED, [0, 0, j, model.DOMAIN_COLUMN]), shape)
        assert one == pytest.approx(draws[j], rel=1e-14) and margin > 0.0
    d = _ks(draws, stats.gamma(shape).cdf)
    print("shape", shape, "KS statistic", d, "limit", KS_LIMIT)
    assert d < KS_LIMIT


def test_normal_draws_follow_the_normal_law():
    """N = 1 000 000, limit 0.002693; observed statistic 0.001014."""
    u = model.uniforms_many(SEED, np.arange(KS_N), 2)
    x = model.normals_many(u[:, 0], u[:, 1])
    s = model.Stream(SEED, [0, 0, 17, 0])
    assert s.normal() == pytest.approx(x[17], rel=1e-14)
    d = _ks(x, stats.norm.cdf)
    print("KS statistic", d, "limit", KS_LIMIT)
    assert d < KS_LIMIT


def test_gamma_follows_every_rejection():
    """A stream whose first normal gives v <= 0 draws no third uniform for that round; the scalar and the vectorised loop agree
    on all of the first 20 000 streams at shape 1, where both kinds of rejection occur."""
    draws = model.gammas_many(SEED, 1.0, 20000)
    rounds_with_two, rounds_with_three = 0, 0
    for j in range(20000):
        s = model.Stream(SEED, [0, 0, j, model.DOMAIN_COLUMN])
        one, _ = model.sample_gamma(s, 1.0)
        assert one == pytest.approx(draws[j], rel=1e-14)
        rounds_with_two += s.uniforms % 3 != 0
        rounds_with_three += s.uniforms > 3 and s.uniforms % 3 == 0
    assert rounds_with_two > 0 and rounds_with_three > 0


# ---- a row's reads over its entries: multinomial -------------------------------------------------------------------------

ROW_TERMS = [(0, 0.02), (1, 0.05), (2, 0.13), (3, 0.30), (4, 0.45)]  # (column, val * a); noise takes the rest of s
ROW_S = 1.0
ROW_P = np.array([0.02, 0.05, 0.13, 0.30, 0.45, 0.05])
ROWS = 20000


def _assert_multinomial(counts, reads):
    """counts [rows x 6]: the column totals against the multinomial's (Pearson, 5 degrees of freedom), every column's histogram
    against Binomial(reads, p_j) (cells of expected count below 5 pooled into the tails), and every pair's covariance sign
    through the conditional law: given the reads before it, a column is Binomial(reads left, p_j / mass left)."""
    assert np.all(counts.sum(axis=1) == reads)
    rows = counts.shape[0]
    total = counts.sum(axis=0)
    chi2 = float(np.sum((total - rows * reads * ROW_P) ** 2 / (rows * reads * ROW_P)))
    p_total = float(stats.chi2.sf(chi2, len(ROW_P) - 1))
    print("totals: chi-square", chi2, "p", p_total)
    assert p_total >= ALPHA
    for j, pj in enumerate(ROW_P):
        expected = rows * stats.binom.pmf(np.arange(reads + 1), reads, pj)
        observed = np.bincount(counts[:, j], minlength=reads + 1).astype(float)
        keep = np.nonzero(expected >= 5.0)[0]
        lo, hi = int(keep[0]), int(keep[-1])
        e = np.concatenate([[expected[:lo].sum()], expected[lo:hi + 1], [expected[hi + 1:].sum()]])
        o = np.concatenate([[observed[:lo].sum()], observed[lo:hi + 1], [observed[hi + 1:].sum()]])
        cells = e > 0
        chi2 = float(np.sum((o[cells] - e[cells]) ** 2 / e[cells]))
        pv = float(stats.chi2.sf(chi2, int(cells.sum()) - 1))
        print("column", j, "cells", int(cells.sum()), "chi-square", chi2, "p", pv)
        assert pv >= ALPHA
    # two columns together are Binomial(reads, p_i + p_j): their dependence is the multinomial's
    for i, j in ((0, 4), (3, 4), (2, 5)):
        both = counts[:, i] + counts[:, j]
        pij = ROW_P[i] + ROW_P[j]
        z = (both.mean() - reads * pij) / math.sqrt(reads * pij * (1 - pij) / rows)
        ratio = both.var(ddof=1) / (reads * pij * (1 - pij))
        print("columns", i, j, "mean z", float(z), "variance ratio", float(ratio))
        assert abs(z) < stats.norm.isf(ALPHA / 2)
        # (the variance of a sample variance is sigma^4 (2 / (rows - 1) + excess kurtosis / rows); a binomial's excess
        # kurtosis, (1 - 6 p q) / (reads p q), is below 0.2 here: ten per cent on the standard deviation covers it)
        assert abs(ratio - 1.0) < stats.norm.isf(ALPHA / 2) * math.sqrt(2.0 / (rows - 1)) * 1.1


def test_chain_of_binomials_draws_a_multinomial():
    """200 reads: the first entries take the walk from 0, the later ones the walk from the mode, the last one the flip."""
    reads = 200
    counts = np.zeros((ROWS, 6), dtype=np.int64)
    record = model.Margin()
    for r in range(ROWS):
        c = [0] * 6
        c[5] += model._chain_of_binomials(model.Stream(SEED, [0, 1, r, model.DOMAIN_ROW_CHAIN]), reads, ROW_TERMS, ROW_S, c, record)
        counts[r] = c
    print("decisions", record.decisions, "smallest margin", record.smallest, record.where)
    assert record.decisions > ROWS * 5
    _assert_multinomial(counts, reads)


def test_categorical_draws_draw_a_multinomial():
    reads = 40
    counts = np.zeros((ROWS, 6), dtype=np.int64)
    record = model.Margin()
    for r in range(ROWS):
        c = [0] * 6
        model._categorical_draws(SEED, 1, r, reads, ROW_TERMS, ROW_S, c, record)
        counts[r] = c
    print("decisions", record.decisions, "smallest margin", record.smallest, record.where)
    assert record.decisions >= ROWS * reads
    _assert_multinomial(counts, reads)


# ---- the kernels' models on a small problem --------------------------------------------------------------------------------

def _small_csr():
    from tests import large_cases
    batch = large_cases.cluster_batch(30, 7, 3, seed=4, noise_only_frac=0.2, max_count=90)
    return batch, model.compacted_csr(batch, 0, list(range(7)))


def test_compacted_csr_is_the_reference_matrix_without_its_zeros():
    """Against np_oracle.add_noise_and_normalize on the dense matrix: same kept rows, same values (the row sums run in another
    order: a few ulp), rows without a path counted in zero_mass."""
    from oracle import np_oracle
    batch, csr = _small_csr()
    rows = len(batch.row_count)
    dense = np.zeros((rows, 7))
    for r in range(rows):
        for g in range(int(batch.row_grp_off[r]), int(batch.row_grp_off[r + 1])):
            for e in range(int(batch.grp_idx_off[g]), int(batch.grp_idx_off[g + 1])):
                dense[r, int(batch.path_idx[e])] = batch.grp_prob[g]
    has = dense.sum(axis=1) > 0
    assert 0 < has.sum() < rows
    q = np_oracle.add_noise_and_normalize(dense[has], np.asarray(batch.row_noise, dtype=float)[has])
    assert csr.rows == int(has.sum()) and csr.entries == int((dense > 0).sum())
    assert csr.zero_mass == float(np.asarray(batch.row_count)[~has].sum()) and csr.total_mass == float(np.asarray(batch.row_count).sum())
    assert np.array_equal(csr.count, np.asarray(batch.row_count, dtype=float)[has])
    assert np.array_equal(csr.noise, q[:, 7])
    for i in range(csr.rows):
        e0, e1 = int(csr.off[i]), int(csr.off[i + 1])
        assert sorted(csr.col[e0:e1]) == list(np.nonzero(q[i, :7])[0])
        assert np.allclose(csr.val[e0:e1], q[i, csr.col[e0:e1]], rtol=1e-15, atol=0)
    # a subset of the columns: entries of the other paths are dropped and the rows renormalised over what is kept
    sub = model.compacted_csr(batch, 0, [1, 4, 6])
    assert sub.columns == 3 and sub.total_mass == csr.total_mass and sub.zero_mass >= csr.zero_mass
    assert set(sub.col) <= {0, 1, 2}


@pytest.mark.parametrize("route", ["one workgroup", "grid"])
def test_models_conserve_the_reads_and_record_every_thin_th_state(route):
    batch, csr = _small_csr()
    init = np.full(7, (csr.total_mass - csr.zero_mass) / 8)
    init_noise = csr.zero_mass + (csr.total_mass - csr.zero_mass) / 8
    if route == "grid":
        run = model.grid(csr, init, init_noise, 3, 2, SEED)
        again = model.grid(csr, init, init_noise, 3, 2, SEED)
        other = model.grid(csr, init, init_noise, 3, 2, SEED + 1)
        assert run.route == "grid, thread per row, columns in LDS"
    else:
        run = model.one_workgroup(csr, init, init_noise, 3, 2, SEED, 0)
        again = model.one_workgroup(csr, init, init_noise, 3, 2, SEED, 0)
        other = model.one_workgroup(csr, init, init_noise, 3, 2, SEED, 1)  # the problem's index is in the counter
    assert run.counts.shape == (6, 8) and np.all(run.counts.sum(axis=1) == int(csr.total_mass))
    assert np.all(run.counts[:, 7] >= int(csr.zero_mass))
    assert run.abundances.shape == (3, 7) and run.noise.shape == (3,)
    assert np.allclose(run.abundances.sum(axis=1) + run.noise, csr.total_mass, rtol=1e-12)
    assert np.array_equal(run.abundances, again.abundances) and np.array_equal(run.noise, again.noise)
    assert not np.array_equal(run.counts, other.counts)
    assert 0.0 < run.margin.smallest < 1.0 and run.margin.where is not None and run.margin.decisions > 100


def test_grid_model_follows_the_route_rule():
    assert model.gibbs_row_lanes(600, 1800) == 1 and model.gibbs_row_lanes(40, 5200) == 64
    assert model.gibbs_row_lanes(10, 119) == 1 and model.gibbs_row_lanes(10, 120) == 64 and model.gibbs_row_lanes(0, 0) == 1
