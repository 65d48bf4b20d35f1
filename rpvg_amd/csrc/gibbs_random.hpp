// Random numbers of the read-count Gibbs samplers (em_sparse.hip: one workgroup per problem; gibbs_grid.hip: the whole GPU
// per problem): the counter-based Philox4x32-10 generator and the binomial and gamma draws on top of it.  The reference's
// mt19937 / libstdc++ distribution streams cannot be reproduced on a GPU: parity is statistical.
#ifndef RPVG_HIP_GIBBS_RANDOM_HPP
#define RPVG_HIP_GIBBS_RANDOM_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

// (internal linkage, as in em_sparse.hip where these came from: each of the two files has its own copy)
namespace {

struct Philox {
    uint32_t key[2];
    uint32_t ctr[4];
    uint32_t out[4];
    int have;

    __device__ __forceinline__ void init(const uint64_t seed, const uint32_t stream_hi, const uint32_t stream_lo) {
        key[0] = static_cast<uint32_t>(seed);
        key[1] = static_cast<uint32_t>(seed >> 32);
        ctr[0] = 0;
        ctr[1] = 0;
        ctr[2] = stream_lo;
        ctr[3] = stream_hi;
        have = 0;
    }

    __device__ __forceinline__ void round(uint32_t (&c)[4], const uint32_t k0, const uint32_t k1) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c[0];
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c[2];
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n1 = static_cast<uint32_t>(p1);
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
        const uint32_t n3 = static_cast<uint32_t>(p0);
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }

    __device__ __forceinline__ void refill() {
        uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
        uint32_t k0 = key[0], k1 = key[1];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            round(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
        if (++ctr[0] == 0) ++ctr[1];
        have = 4;
    }

    __device__ __forceinline__ uint32_t next() {
        if (have == 0) refill();
        return out[--have];
    }

    // uniform in (0, 1)
    __device__ __forceinline__ double uniform() {
        const uint64_t hi = next(), lo = next();
        return (static_cast<double>(((hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    }

    __device__ __forceinline__ double normal() {
        const double u1 = uniform(), u2 = uniform();
        return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    }
};

// Binomial(n, p) by inversion: from 0 when the mean is small, otherwise outwards from the mode (expected
// O(sqrt(n p q)) steps; exact up to floating point).
__device__ uint32_t sampleBinomial(Philox & rng, const uint32_t n, double p) {
    if (n == 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    const bool flip = p > 0.5;
    if (flip) p = 1.0 - p;
    const double q = 1.0 - p, ratio = p / q;
    uint32_t k;
    if (n * p < 16.0) {
        double pmf = exp(n * log(q));
        double u = rng.uniform();
        k = 0;
        while (u > pmf && k < n) {
            u -= pmf;
            pmf *= ratio * (static_cast<double>(n - k) / (k + 1.0));
            ++k;
        }
    } else {
        const uint32_t mode = static_cast<uint32_t>((n + 1.0) * p);
        const double log_pmf_mode = lgamma(n + 1.0) - lgamma(mode + 1.0) - lgamma(n - mode + 1.0) + mode * log(p) + (n - mode) * log(q);
        const double pmf_mode = exp(log_pmf_mode);
        double u = rng.uniform();
        // walk outwards from the mode, alternating sides, until the accumulated mass passes u
        double up = pmf_mode, down = pmf_mode;
        uint32_t ku = mode, kd = mode;
        k = mode;
        if (u > pmf_mode) {
            u -= pmf_mode;
            while (true) {
                bool moved = false;
                if (ku < n) {
                    up *= ratio * (static_cast<double>(n - ku) / (ku + 1.0));
                    ++ku;
                    moved = true;
                    if (u <= up) { k = ku; break; }
                    u -= up;
                }
                if (kd > 0) {
                    down *= (static_cast<double>(kd) / (n - kd + 1.0)) / ratio;
                    --kd;
                    moved = true;
                    if (u <= down) { k = kd; break; }
                    u -= down;
                }
                if (!moved) { k = mode; break; }
            }
        }
    }
    return flip ? n - k : k;
}

// Gamma(shape >= 1, 1) by Marsaglia and Tsang's squeeze method.
__device__ double sampleGamma(Philox & rng, const double shape) {
    const double d = shape - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    while (true) {
        const double x = rng.normal();
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double u = rng.uniform();
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) return d * v;
    }
}

}  // namespace

#endif
