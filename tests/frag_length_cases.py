"""The fragment-length model restated in numpy + scipy.special, sequentially, as the reference computes it — what the GPU
tests of tests/test_hip_frag_length.py check the device against, itself pinned to the reference's own vectors by
tests/test_frag_length_model.py.

  fit()                  FragmentLengthDist(frag_length_counts, skew_normal)        src/fragment_length_dist.cpp:60-285
                         (with the right-hand bracketing loop of alpha re-evaluating at alpha + LEFT radius, :230)
  log_skew_normal_pdf()  Utils::log_skew_normal_pdf with log_Phi's three ranges     src/utils.hpp:165-220
  skew_normal_cdf(), truncated_mean()                                               src/utils.hpp:229-247
  effective_lengths()    PathsIndex::effectivePathLength                            src/paths_index.cpp:190-229
Owen's T is scipy.special.owens_t.
"""
import functools
import json
import math
import os

import numpy as np
from scipy.special import ndtr, owens_t

PI = 3.141592653589793238462643383279    # Utils::pi
DOUBLE_PRECISION = np.finfo(np.float64).eps * 100  # Utils::double_precision
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frag_length_fixture.json")

# 2 053 path lengths: every length below 2 048, a few large ones, the largest uint32_t; not a multiple of 64
PATH_LENGTHS = np.array(list(range(2048)) + [5000, 100000, 4000000, 2 ** 32 - 1, 1], dtype=np.uint32)
NORMAL_DISTRIBUTIONS = [(5.0, 2.0, 0.0), (20.0, 1.0, 0.0)]  # src/tests/paths_index_test.cpp:69,74


def min_comparable_lengths(name):
    """How many of PATH_LENGTHS must have a truncated-mean denominator >= 1e-6 (and are then compared): 1 000 of the
    2 053, except for the 3 001-entry vector.  Its sample was drawn at loc 1500, scale 300, shape 4: the distribution has
    no mass below about 1 200, so of the lengths 0 .. 2047 only the upper 840 or so can qualify, however the code behaves."""
    return 800 if name.endswith("L3001") else 1000


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def count_vectors():
    """name -> uint32 counts: the reference's two vectors and the five seeded ones."""
    fx = fixture()
    out = {"reference_mle_92": fx["counts_mle"], "reference_real_data_1000": fx["counts_real_data"]}
    for s in fx["seeded"]:
        out["seeded_a%g_loc%g_scale%g_n%d_L%d" % (s["a"], s["loc"], s["scale"], s["n"], len(s["counts"]))] = s["counts"]
    return {k: np.asarray(v, dtype=np.uint32) for k, v in out.items()}


def double_compare(a, b):
    """Utils::doubleCompare, src/utils.hpp:87-93"""
    a, b = float(a), float(b)
    return a == b or abs(a - b) < abs(min(a, b)) * DOUBLE_PRECISION


def phi_cdf(z):
    """Utils::Phi (the cephes ndtr the reference adapted; scipy's ndtr is the same function)."""
    return ndtr(np.asarray(z, dtype=np.float64))


def _log_phi_series(z):
    log_lhs = -0.5 * z * z - math.log(-z) - 0.5 * math.log(2 * PI)
    last_total, rhs, numerator, denom_factor, denom_cons, sign, i = 0.0, 1.0, 1.0, 1.0, 1.0 / (z * z), 1, 0
    while abs(last_total - rhs) > np.finfo(np.float64).eps:
        i += 1
        last_total = rhs
        sign = -sign
        denom_factor *= denom_cons
        numerator *= 2 * i - 1
        rhs += sign * numerator * denom_factor
    return log_lhs + math.log(rhs)


def log_phi(z):
    """Utils::log_Phi: z > 6, z > -20, and the asymptotic series below."""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    out = np.empty_like(z)
    hi = z > 6.0
    mid = ~hi & (z > -20.0)
    lo = ~hi & ~mid
    out[hi] = -phi_cdf(-z[hi])
    with np.errstate(divide="ignore"):
        out[mid] = np.log(phi_cdf(z[mid]))
    out[lo] = [_log_phi_series(float(v)) for v in z[lo]]
    return out


def log_skew_normal_pdf(x, m, s, a):
    z = (np.asarray(x, dtype=np.float64) - m) / s
    return math.log(2.0 / math.sqrt(2.0 * PI)) + log_phi(a * z) - math.log(s) - 0.5 * z * z


def log_normal_pdf(x, m, s):
    z = (np.asarray(x, dtype=np.float64) - m) / s
    return math.log(0.3989422804014327) - math.log(s) - 0.5 * z * z


def log_prob(x, loc, scale, shape):
    """FragmentLengthDist::logProb, src/fragment_length_dist.cpp:385-427"""
    return log_normal_pdf(x, loc, scale) if double_compare(shape, 0.0) else log_skew_normal_pdf(x, loc, scale, shape)


def _sequential_sum(terms):
    return float(np.cumsum(terms)[-1]) if len(terms) else 0.0  # cumsum adds left to right, as the reference's loop does


def golden_section_search(f, x_min, x_max, tolerance):
    inv_phi = (math.sqrt(5.0) - 1.0) / 2.0
    steps = int(math.ceil(math.log(tolerance / (x_max - x_min)) / math.log(inv_phi)))
    x_lo = x_min + inv_phi * inv_phi * (x_max - x_min)
    x_hi = x_min + inv_phi * (x_max - x_min)
    f_lo, f_hi = f(x_lo), f(x_hi)
    for _ in range(max(steps, 0)):
        if f_lo < f_hi:
            x_min = x_lo
            x_lo = x_hi
            x_hi = x_min + inv_phi * (x_max - x_min)
            f_lo = f_hi
            f_hi = f(x_hi)
        else:
            x_max = x_hi
            x_hi = x_lo
            x_lo = x_min + inv_phi * inv_phi * (x_max - x_min)
            f_hi = f_lo
            f_lo = f(x_lo)
    return (x_min + x_hi) / 2.0 if f_lo > f_hi else (x_lo + x_max) / 2.0


def _bracket(f, x, quirk):
    factor = 1.3
    ll = f(x)
    left, right = 1.0, 1.0
    rad = f(x - left)
    while rad >= ll and not math.isinf(rad):
        if math.isinf(left * factor):
            break
        left *= factor
        rad = f(x - left)
    rad = f(x + right)
    while rad >= ll and not math.isinf(rad):
        if math.isinf(right * factor):
            break
        right *= factor
        rad = f(x + (left if quirk else right))  # src/fragment_length_dist.cpp:230 (alpha) against :254 (mu)
    return left, right


def fit(counts, skew_normal=True):
    """-> dict(loc, scale, shape, max_length, sample_size, iterations, evaluations, valid)"""
    counts = np.asarray(counts, dtype=np.uint32)
    assert len(counts) and counts[0] == 0
    idx = np.arange(len(counts), dtype=np.float64)
    c = counts.astype(np.float64)
    sample_size = int(counts.astype(np.uint64).sum()) & 0xffffffff
    length_sum = int((np.arange(len(counts), dtype=np.uint64) * counts.astype(np.uint64)).sum())
    out = dict(max_length=len(counts), sample_size=sample_size, iterations=0, evaluations=0)
    if sample_size < 2:
        out.update(loc=float(length_sum), scale=0.0, shape=0.0, valid=False)
        return out
    if not skew_normal:
        loc = length_sum / float(sample_size)
        scale = math.sqrt(_sequential_sum((idx - loc) ** 2 * c) / float(sample_size - 1))
        out.update(loc=loc, scale=scale, shape=0.0, valid=loc >= 0 and scale > 0)
        return out

    k0, k1 = float(sample_size), float(length_sum)
    term = c * idx * idx
    k2, k3 = _sequential_sum(term), _sequential_sum(term * idx)
    m1 = k1 / k0
    m2 = k2 / k0 - m1 * m1
    m3 = k3 / k0 - 3.0 * m1 * m2 - m1 * m1 * m1
    mean, sd = m1, math.sqrt(m2)
    skew = m3 / (sd * sd * sd)
    alpha = sigma = 0.0
    if skew != 0.0 and k0 > 2.0:
        gam = min(abs(skew), 0.9952717464311565) ** (2.0 / 3.0)
        abs_delta = math.sqrt((PI / 2.0) * (gam / (gam + ((4.0 - PI) / 2.0) ** (2.0 / 3.0))))
        abs_alpha = abs_delta / math.sqrt(1.0 - abs_delta * abs_delta)
        alpha = -abs_alpha if skew < 0.0 else abs_alpha
    delta = alpha / math.sqrt(1.0 + alpha * alpha)
    if sd != 0.0 and k0 > 1.0:
        sigma = sd / math.sqrt(1.0 - 2.0 * delta * delta / PI)
    mu = mean - sigma * delta * math.sqrt(2.0 / PI)
    if abs(alpha) > 1000.0 * sigma:
        alpha = (1.0 if alpha > 0.0 else -1.0) * 1000.0 * sigma

    nonzero = np.nonzero(counts)[0]
    x_nz, c_nz = idx[nonzero], c[nonzero]
    evaluations = [0]

    def log_likelihood(m, s, a):
        evaluations[0] += 1
        with np.errstate(over="ignore", invalid="ignore"):  # a bracket far out is -inf, as in the reference
            return _sequential_sum(c_nz * log_skew_normal_pdf(x_nz, m, s, a))

    tol = 1e-4
    prev_mu, prev_alpha = mu + 2.0 * tol, alpha + 2.0 * tol
    iterations = 0
    while iterations < 100 and (abs(prev_mu - mu) >= tol or abs(prev_alpha - alpha) >= tol):
        iterations += 1
        prev_mu, prev_alpha = mu, alpha

        def f_alpha(a):
            return log_likelihood(mu, sigma, a)
        left, right = _bracket(f_alpha, alpha, quirk=True)
        alpha = golden_section_search(f_alpha, alpha - left, alpha + right, tol / 4.0)

        def f_mu(m):
            return log_likelihood(m, sigma, alpha)
        left, right = _bracket(f_mu, mu, quirk=False)
        mu = golden_section_search(f_mu, mu - left, mu + right, tol / 4.0)

        dev = idx - mu
        sigma = math.sqrt(_sequential_sum(c * dev * dev) / k0)

    out.update(loc=mu, scale=sigma, shape=alpha, iterations=iterations, evaluations=evaluations[0], valid=mu >= 0 and sigma > 0)
    return out


@functools.lru_cache(maxsize=None)
def restated_fit(name, skew_normal=True):
    """The restatement's fit of a fixture vector, computed once per session."""
    return fit(count_vectors()[name], skew_normal)


def skew_normal_pdf(x, m, s, a):
    z = (np.asarray(x, dtype=np.float64) - m) / s
    return (2.0 / math.sqrt(2.0 * PI)) * np.exp(-0.5 * z * z) * phi_cdf(a * z) / s


def skew_normal_cdf(x, m, s, a):
    z = (np.asarray(x, dtype=np.float64) - m) / s
    return phi_cdf(z) - 2.0 * owens_t(z, a)


def truncated_mean(m, s, a, c, d):
    """Utils::truncated_skew_normal_expected_value -> (mean, denominator cdf(v) - cdf(u))"""
    u = (np.asarray(c, dtype=np.float64) - m) / s
    v = (np.asarray(d, dtype=np.float64) - m) / s
    beta = math.sqrt(1.0 + a * a)
    delta = a / beta
    val = skew_normal_pdf(u, 0.0, 1.0, a) - skew_normal_pdf(v, 0.0, 1.0, a)
    val = val + (2.0 / math.sqrt(2.0 * PI)) * delta * (phi_cdf(v * beta) - phi_cdf(u * beta))
    denom = skew_normal_cdf(v, 0.0, 1.0, a) - skew_normal_cdf(u, 0.0, 1.0, a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return m + s * (val / denom), denom


def effective_lengths(path_lengths, loc, scale, shape):
    """PathsIndex::effectivePathLength -> (values, denominator of the truncated mean of every length)"""
    from scipy.special import erf
    lengths = np.asarray(path_lengths, dtype=np.float64)
    if double_compare(shape, 0.0):
        def lower_phi(v):
            return np.exp(-0.5 * v ** 2) / math.sqrt(2 * math.acos(-1))

        def upper_phi(v):
            return 0.5 * (1 + erf(v / math.sqrt(2)))
        alpha = (1.0 - loc) / scale
        beta = (lengths - loc) / scale
        denom = upper_phi(beta) - upper_phi(alpha)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = loc + scale * (lower_phi(alpha) - lower_phi(beta)) / denom
    else:
        mean, denom = truncated_mean(loc, scale, shape, 1.0, lengths)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isfinite(mean), np.maximum(1.0, lengths - mean), 1.0)
    out[lengths == 0] = 0.0
    return out, np.asarray(denom, dtype=np.float64)
