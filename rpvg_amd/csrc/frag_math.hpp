// frag_math.hpp — the scalar mathematics of the fragment-length model, written once for the device kernels of
// frag_length.hip and for the sequential host line of tests/cpp/frag_length_dist_check.cpp.
//
// Restates   Utils::Phi / log_Phi / log_normal_pdf / log_skew_normal_pdf           src/utils.hpp:143-220
//            skew_normal_pdf / skew_normal_cdf / truncated_skew_normal_expected_value   src/utils.hpp:222-247
//            Utils::golden_section_search                                           src/utils.hpp:250-294
//            the skew-normal fit of FragmentLengthDist(counts, skew_normal)         src/fragment_length_dist.cpp:60-285
//            PathsIndex::effectivePathLength                                        src/paths_index.cpp:190-229
//
// Owen's T is this project's own: the reflection and the a > 1 identities of Owen (1956) reduce every argument to
// h >= 0, 0 <= a <= 1, where T(h, a) = 1/(2 pi) * int_0^a exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx is integrated with a
// 64-point Gauss-Legendre rule whose nodes are generated when the library is loaded (Newton on P_64).  The upper limit is
// cut where the integrand is below exp(-50) of its scale, so the Gaussian factor spans at most ten standard deviations
// of the rule (error of the rule < 1e-18 there; the factor 1 / (1 + x^2) has its poles at +-i, Bernstein radius 4.6).
//
// The fit is a template over the object that evaluates the sums: one workgroup with a fixed reduction order on the
// device, a plain loop on the host.  Everything else is scalar code that every thread executes alike.
#ifndef RPVG_HIP_FRAG_MATH_HPP
#define RPVG_HIP_FRAG_MATH_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RPVG_FRAG_HD __host__ __device__ inline
#else
#define RPVG_FRAG_HD inline
#endif

namespace rpvg_frag {

constexpr double kPi = 3.141592653589793238462643383279;               // Utils::pi, src/utils.hpp:56
constexpr double kDoublePrecision = 2.220446049250313e-16 * 100;       // Utils::double_precision, src/utils.hpp:81
constexpr double kEpsilon = 2.220446049250313e-16;
constexpr int kGaussLegendrePairs = 32;                                 // a 64-point rule, symmetric about the midpoint

// nodes in (0, 1) of the rule on [-1, 1] and their weights; the other half is the mirror image
struct GaussLegendre {
    double x[kGaussLegendrePairs];
    double w[kGaussLegendrePairs];
};

// Newton iteration on the Legendre polynomial of degree 64 from the Chebyshev guess (host, once per process)
inline GaussLegendre makeGaussLegendre() {
    GaussLegendre gl;
    const int n = 2 * kGaussLegendrePairs;
    for (int i = 0; i < kGaussLegendrePairs; ++i) {
        long double x = std::cos(static_cast<long double>(kPi) * (i + 0.75L) / (n + 0.5L));
        long double dp = 0;
        for (int it = 0; it < 100; ++it) {
            long double p0 = 1, p1 = x;
            for (int k = 2; k <= n; ++k) {
                const long double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
                p0 = p1;
                p1 = p2;
            }
            dp = n * (x * p1 - p0) / (x * x - 1);
            const long double dx = p1 / dp;
            x -= dx;
            if (std::fabs(static_cast<double>(dx)) < 1e-19) break;
        }
        gl.x[i] = static_cast<double>(x);
        gl.w[i] = static_cast<double>(2 / ((1 - x * x) * dp * dp));
    }
    return gl;
}

// Utils::doubleCompare, src/utils.hpp:87-93
RPVG_FRAG_HD bool doubleCompare(const double a, const double b) {
    return (a == b) || (fabs(a - b) < fabs((b < a) ? b : a) * kDoublePrecision);
}

// src/utils.hpp:143-162
RPVG_FRAG_HD double Phi(const double z) {
    const double root_1_2 = sqrt(0.5);
    const double x = z * root_1_2;
    const double a = fabs(x);
    if (a < root_1_2) return 0.5 + 0.5 * erf(x);
    const double y = 0.5 * erfc(a);
    return (x > 0) ? 1.0 - y : y;
}

// src/utils.hpp:165-196
RPVG_FRAG_HD double logPhi(const double z) {
    if (z > 6.0) return -Phi(-z);
    if (z > -20.0) return log(Phi(z));
    const double log_lhs = -0.5 * z * z - log(-z) - 0.5 * log(2 * kPi);
    double last_total = 0, right_hand_side = 1, numerator = 1, denom_factor = 1;
    const double denom_cons = 1.0 / (z * z);
    long sign = 1, i = 0;
    while (fabs(last_total - right_hand_side) > kEpsilon) {
        i += 1;
        last_total = right_hand_side;
        sign = -sign;
        denom_factor *= denom_cons;
        numerator *= 2 * i - 1;
        right_hand_side += sign * numerator * denom_factor;
    }
    return log_lhs + log(right_hand_side);
}

// src/utils.hpp:206-212
RPVG_FRAG_HD double logNormalPdf(const double x, const double m, const double s) {
    const double inv_sqrt_2pi = 0.3989422804014327;
    const double z = (x - m) / s;
    return log(inv_sqrt_2pi) - log(s) - 0.5 * z * z;
}

// src/utils.hpp:214-220
RPVG_FRAG_HD double logSkewNormalPdf(const double x, const double m, const double s, const double a) {
    const double log_const = log(2.0 / sqrt(2.0 * kPi));
    const double z = (x - m) / s;
    return log_const + logPhi(a * z) - log(s) - 0.5 * z * z;
}

// FragmentLengthDist::logProb without the buffer (the buffer holds the same values), src/fragment_length_dist.cpp:385-427
RPVG_FRAG_HD double logProb(const double value, const double loc, const double scale, const double shape) {
    return doubleCompare(shape, 0.0) ? logNormalPdf(value, loc, scale) : logSkewNormalPdf(value, loc, scale, shape);
}

// src/utils.hpp:222-227
RPVG_FRAG_HD double skewNormalPdf(const double x, const double m, const double s, const double a) {
    const double const_factor = 2.0 / (sqrt(2.0 * kPi));
    const double z = (x - m) / s;
    return const_factor * exp(-0.5 * z * z) * Phi(a * z) / s;
}

// T(h, a) for h >= 0 and 0 <= a <= 1
RPVG_FRAG_HD double owensTUnit(const double h, const double a, const GaussLegendre & gl) {
    if (a == 0.0) return 0.0;
    if (h == 0.0) return atan(a) / (2 * kPi);
    const double hh = h * h;
    double upper = a;
    if (hh < 100.0) {  // beyond h = 10 the whole integral is below 1e-22
        const double cut = sqrt(100.0 / hh - 1.0);
        if (cut < upper) upper = cut;
    }
    const double half = 0.5 * upper;
    double sum = 0;
    for (int i = 0; i < kGaussLegendrePairs; ++i) {
        const double lo = half - half * gl.x[i], hi = half + half * gl.x[i];
        const double qlo = 1.0 + lo * lo, qhi = 1.0 + hi * hi;
        sum += gl.w[i] * (exp(-0.5 * hh * qlo) / qlo + exp(-0.5 * hh * qhi) / qhi);
    }
    return sum * half / (2 * kPi);
}

// Owen's T function for any finite h and a
RPVG_FRAG_HD double owensT(double h, double a, const GaussLegendre & gl) {
    const bool negative = a < 0;
    a = fabs(a);
    h = fabs(h);
    double value;
    if (a <= 1.0) {
        value = owensTUnit(h, a, gl);
    } else if (h == 0.0) {
        value = atan(a) / (2 * kPi);
    } else {
        // T(h, a) = (Phi(h) + Phi(ah)) / 2 - Phi(h) Phi(ah) - T(ah, 1/a) for h >= 0, in the form that does not cancel
        const double ah = a * h;
        const double root_1_2 = sqrt(0.5);
        if (ah <= 0.67) {
            value = 0.25 - 0.25 * erf(h * root_1_2) * erf(ah * root_1_2);
        } else {
            const double nh = 0.5 * erfc(h * root_1_2), nah = 0.5 * erfc(ah * root_1_2);
            value = 0.5 * (nh + nah) - nh * nah;
        }
        value -= owensTUnit(ah, 1.0 / a, gl);
    }
    return negative ? -value : value;
}

// src/utils.hpp:229-233
RPVG_FRAG_HD double skewNormalCdf(const double x, const double m, const double s, const double a, const GaussLegendre & gl) {
    const double z = (x - m) / s;
    return Phi(z) - 2.0 * owensT(z, a, gl);
}

// The three terms of truncated_skew_normal_expected_value that belong to one bound, src/utils.hpp:243-245
struct TruncationBound {
    double pdf;       // skew_normal_pdf(u, 0, 1, a)
    double phi_beta;  // Phi(u * beta)
    double cdf;       // skew_normal_cdf(u, 0, 1, a)
};

RPVG_FRAG_HD TruncationBound truncationBound(const double u, const double a, const GaussLegendre & gl) {
    TruncationBound b;
    b.pdf = skewNormalPdf(u, 0.0, 1.0, a);
    b.phi_beta = Phi(u * sqrt(1.0 + a * a));
    b.cdf = skewNormalCdf(u, 0.0, 1.0, a, gl);
    return b;
}

// src/utils.hpp:237-247 with the terms of the lower bound handed in
RPVG_FRAG_HD double truncatedSkewNormalMean(const double m, const double s, const double a, const TruncationBound & lower, const double d,
                                            const GaussLegendre & gl, double * denominator = nullptr) {
    const double v = (d - m) / s;
    const double beta = sqrt(1.0 + a * a);
    const double delta = a / beta;
    const TruncationBound upper = truncationBound(v, a, gl);
    double val = lower.pdf - upper.pdf;
    val += (2.0 / sqrt(2.0 * kPi)) * delta * (upper.phi_beta - lower.phi_beta);
    const double denom = upper.cdf - lower.cdf;
    if (denominator) *denominator = denom;
    val /= denom;
    return m + s * val;
}

RPVG_FRAG_HD double truncatedSkewNormalMean(const double m, const double s, const double a, const double c, const double d, const GaussLegendre & gl) {
    return truncatedSkewNormalMean(m, s, a, truncationBound((c - m) / s, a, gl), d, gl);
}

// PathsIndex::calculateLowerPhi / calculateUpperPhi, src/paths_index.cpp:221-229
RPVG_FRAG_HD double lowerPhi(const double value) { return exp(-0.5 * pow(value, 2)) / sqrt(2 * acos(-1.0)); }
RPVG_FRAG_HD double upperPhi(const double value) { return 0.5 * (1 + erf(value / sqrt(2.0))); }

// What effectivePathLength needs of the lower bound c = 1: computed once for all paths
struct EffectiveLengthLower {
    double lower_phi, upper_phi;  // normal branch: of alpha = (1 - loc) / scale
    TruncationBound bound;        // skew branch: of u = (1 - loc) / scale
};

RPVG_FRAG_HD EffectiveLengthLower effectiveLengthLower(const double loc, const double scale, const double shape, const GaussLegendre & gl) {
    EffectiveLengthLower lower = {};
    if (doubleCompare(shape, 0.0)) {
        const double alpha = (1.0 - loc) / scale;
        lower.lower_phi = lowerPhi(alpha);
        lower.upper_phi = upperPhi(alpha);
    } else {
        lower.bound = truncationBound((1.0 - loc) / scale, shape, gl);
    }
    return lower;
}

// src/paths_index.cpp:190-219
RPVG_FRAG_HD double effectivePathLength(const uint32_t path_length, const double loc, const double scale, const double shape,
                                        const EffectiveLengthLower & lower, const GaussLegendre & gl) {
    if (path_length == 0) return 0;
    double trunc_fragment_length_mean = 0.0;
    if (doubleCompare(shape, 0.0)) {
        const double beta = (path_length - loc) / scale;
        trunc_fragment_length_mean = loc + scale * (lower.lower_phi - lowerPhi(beta)) / (upperPhi(beta) - lower.upper_phi);
    } else {
        trunc_fragment_length_mean = truncatedSkewNormalMean(loc, scale, shape, lower.bound, path_length, gl);
    }
    if (!__builtin_isfinite(trunc_fragment_length_mean)) return 1;
    const double effective_length = path_length - trunc_fragment_length_mean;
    return (1.0 < effective_length) ? effective_length : 1.0;
}

// ---- the fit -----------------------------------------------------------------------------------------------------

struct FitResult {
    double loc, scale, shape;
    uint32_t max_length, sample_size, iterations, evaluations;
    int32_t valid;
};

// Utils::golden_section_search, src/utils.hpp:250-294; f is called with the abscissa
template <typename F>
RPVG_FRAG_HD double goldenSectionSearch(F & f, double x_min, double x_max, const double tolerance) {
    const double inv_phi = (sqrt(5.0) - 1.0) / 2.0;
    // the reference converts to size_t; a ratio that is not a positive number means no step
    const double steps_real = ceil(log(tolerance / (x_max - x_min)) / log(inv_phi));
    const uint64_t steps = (steps_real > 0) ? static_cast<uint64_t>(steps_real) : 0;
    double x_lo = x_min + inv_phi * inv_phi * (x_max - x_min);
    double x_hi = x_min + inv_phi * (x_max - x_min);
    double f_lo = f(x_lo);
    double f_hi = f(x_hi);
    for (uint64_t step = 0; step < steps; ++step) {
        if (f_lo < f_hi) {
            x_min = x_lo;
            x_lo = x_hi;
            x_hi = x_min + inv_phi * (x_max - x_min);
            f_lo = f_hi;
            f_hi = f(x_hi);
        } else {
            x_max = x_hi;
            x_hi = x_lo;
            x_lo = x_min + inv_phi * inv_phi * (x_max - x_min);
            f_hi = f_lo;
            f_lo = f(x_lo);
        }
    }
    if (f_lo > f_hi) return (x_min + x_hi) / 2.0;
    return (x_lo + x_max) / 2.0;
}

// The interval around x that golden_section_search gets, src/fragment_length_dist.cpp:213-231 / :237-255.  The
// right-hand loop of alpha re-evaluates at alpha + LEFT radius (:230); that is the reference's behaviour and is kept.
template <typename F>
RPVG_FRAG_HD void bracket(F & f, const double x, const bool right_loop_uses_left_radius, double * left_radius_out, double * right_radius_out) {
    const double factor = 1.3;
    const double ll = f(x);
    double left_radius = 1.0, right_radius = 1.0;
    double rad_ll = f(x - left_radius);
    while (rad_ll >= ll && !__builtin_isinf(rad_ll)) {
        if (__builtin_isinf(left_radius * factor)) break;
        left_radius *= factor;
        rad_ll = f(x - left_radius);
    }
    rad_ll = f(x + right_radius);
    while (rad_ll >= ll && !__builtin_isinf(rad_ll)) {
        if (__builtin_isinf(right_radius * factor)) break;
        right_radius *= factor;
        rad_ll = f(x + (right_loop_uses_left_radius ? left_radius : right_radius));
    }
    *left_radius_out = left_radius;
    *right_radius_out = right_radius;
}

// FragmentLengthDist(frag_length_counts, skew_normal), src/fragment_length_dist.cpp:60-285.  `sums` provides, over the
// count vector and in one fixed order each:
//   moments(&k0, &k1, &k2, &k3)      sum c, sum c i (exact integers), sum double(c i i), sum double(c i i) * i
//   squaredDeviations(mu)            sum (c * (i - mu)) * (i - mu)
//   variance(loc)                    sum pow(i - loc, 2) * c
//   logLikelihood(mu, sigma, alpha)  sum over c != 0 of c * log_skew_normal_pdf(i, mu, sigma, alpha)
template <typename Sums>
RPVG_FRAG_HD FitResult fitFragmentLengths(Sums & sums, const uint32_t num_counts, const bool skew_normal) {
    FitResult out = {};
    out.max_length = num_counts;

    double k0_sum, k1_sum, k2, k3;
    sums.moments(&k0_sum, &k1_sum, &k2, &k3);
    const uint32_t sample_size = static_cast<uint32_t>(static_cast<uint64_t>(k0_sum));  // a uint32_t in the reference
    const uint64_t frag_length_sum = static_cast<uint64_t>(k1_sum);
    out.sample_size = sample_size;

    if (sample_size < 2) {
        out.loc = static_cast<double>(frag_length_sum);
        out.scale = 0.0;
        out.shape = 0.0;
        out.valid = 0;
        return out;
    }

    if (!skew_normal) {
        out.loc = frag_length_sum / static_cast<double>(sample_size);
        out.scale = sqrt(sums.variance(out.loc) / static_cast<double>(sample_size - 1));
        out.shape = 0.0;
        out.valid = (out.loc >= 0 && out.scale > 0) ? 1 : 0;
        return out;
    }

    const double k0 = sample_size;
    const double k1 = static_cast<double>(frag_length_sum);

    const double m1 = k1 / k0;
    const double m2 = k2 / k0 - m1 * m1;
    const double m3 = k3 / k0 - 3.0 * m1 * m2 - m1 * m1 * m1;

    const double mean = m1;
    const double sd = sqrt(m2);
    const double skew = m3 / (sd * sd * sd);

    double alpha = 0.0, sigma = 0.0, mu = 0.0;
    if (skew != 0.0 && k0 > 2.0) {
        // The cap sits on the edge: with the correctly rounded powers the reference's libm returns, abs_delta at the cap is
        // 1 - 2^-53 and abs_alpha 6.7e7 (clamped to 1000 sigma below); a power that is one unit in the last place larger
        // makes abs_delta 1 and abs_alpha infinite, and the fit starts from NaN.  The device's pow is not correctly
        // rounded, so the two powers of constants are written out; add, divide, multiply and sqrt round as on the host.
        const double max_skew = 0.9952717464311565;
        const double gam_at_max_skew = 0x1.fe62833b58bf1p-1;  // pow(max_skew, 2.0 / 3.0)
        const double skew_scale = 0x1.235366297af7ap-1;       // pow((4.0 - pi) / 2.0, 2.0 / 3.0)
        const double gam = (max_skew < fabs(skew)) ? gam_at_max_skew : pow(fabs(skew), 2.0 / 3.0);  // pow(std::min(abs(skew), max_skew), 2.0 / 3.0)
        const double abs_delta = sqrt((kPi / 2.0) * (gam / (gam + skew_scale)));
        const double abs_alpha = abs_delta / sqrt(1.0 - abs_delta * abs_delta);
        alpha = skew < 0.0 ? -abs_alpha : abs_alpha;
    }
    const double delta = alpha / sqrt(1.0 + alpha * alpha);
    if (sd != 0.0 && k0 > 1.0) sigma = sd / sqrt(1.0 - 2.0 * delta * delta / kPi);
    mu = mean - sigma * delta * sqrt(2.0 / kPi);

    if (fabs(alpha) > 1000.0 * sigma) alpha = (alpha > 0.0 ? 1.0 : -1.0) * 1000.0 * sigma;

    uint32_t evaluations = 0;
    auto alpha_log_likelihood = [&](const double a) {
        ++evaluations;
        return sums.logLikelihood(mu, sigma, a);
    };
    auto mu_log_likelihood = [&](const double m) {
        ++evaluations;
        return sums.logLikelihood(m, sigma, alpha);
    };

    const double tol = 1e-4;
    double prev_mu = mu + 2.0 * tol;
    double prev_alpha = alpha + 2.0 * tol;
    const int max_iters = 100;
    int iter_num = 0;

    while (iter_num < max_iters && (fabs(prev_mu - mu) >= tol || fabs(prev_alpha - alpha) >= tol)) {
        ++iter_num;
        prev_mu = mu;
        prev_alpha = alpha;

        double left_radius, right_radius;
        bracket(alpha_log_likelihood, alpha, true, &left_radius, &right_radius);
        alpha = goldenSectionSearch(alpha_log_likelihood, alpha - left_radius, alpha + right_radius, tol / 4.0);

        bracket(mu_log_likelihood, mu, false, &left_radius, &right_radius);
        mu = goldenSectionSearch(mu_log_likelihood, mu - left_radius, mu + right_radius, tol / 4.0);

        // equation 8 of Azzalini (1985)
        sigma = sqrt(sums.squaredDeviations(mu) / k0);
    }

    out.loc = mu;
    out.scale = sigma;
    out.shape = alpha;
    out.iterations = static_cast<uint32_t>(iter_num);
    out.evaluations = evaluations;
    out.valid = (out.loc >= 0 && out.scale > 0) ? 1 : 0;
    return out;
}

// The sums as the reference's loops compute them: the sequential host line
struct SequentialSums {
    const uint32_t * counts;
    uint32_t n;

    void moments(double * k0, double * k1, double * k2, double * k3) const {
        uint64_t size = 0, sum = 0;
        double s2 = 0, s3 = 0;
        for (uint64_t i = 0; i < n; ++i) {
            size += counts[i];
            sum += i * counts[i];
            double term = static_cast<double>(counts[i] * i * i);
            s2 += term;
            term *= i;
            s3 += term;
        }
        *k0 = static_cast<double>(size);
        *k1 = static_cast<double>(sum);
        *k2 = s2;
        *k3 = s3;
    }
    double squaredDeviations(const double mu) const {
        double total = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const double dev = i - mu;
            total += counts[i] * dev * dev;
        }
        return total;
    }
    double variance(const double loc) const {
        double total = 0;
        for (uint64_t i = 0; i < n; ++i) total += pow(static_cast<double>(i) - loc, 2) * counts[i];
        return total;
    }
    double logLikelihood(const double mu, const double sigma, const double alpha) const {
        double ll = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (counts[i] == 0) continue;
            ll += counts[i] * logSkewNormalPdf(static_cast<double>(i), mu, sigma, alpha);
        }
        return ll;
    }
};

}  // namespace rpvg_frag

#endif
