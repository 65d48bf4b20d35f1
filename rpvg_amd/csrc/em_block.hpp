// Block-level primitives (wave = 64) the EM kernels (em_sparse.hip) and the read-count sampler (gibbs_counts.hip) share.
#ifndef RPVG_EM_BLOCK_HPP
#define RPVG_EM_BLOCK_HPP

#include "common.hpp"

namespace {

using rpvg_hip_detail::waveSumF64;

template <typename T>
__device__ __forceinline__ T waveReduceSum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <>
__device__ __forceinline__ double waveReduceSum<double>(double v) {
    return waveSumF64(v);
}

// Sum over the block, result in every thread.  scratch: BLOCK/64 elements.
template <typename T, int BLOCK>
__device__ __forceinline__ T blockReduceSum(T v, T * scratch) {
    v = waveReduceSum(v);
    if (BLOCK == 64) return v;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    T total = scratch[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) total += scratch[w];
    return total;
}

// Exclusive scan of the pair (a, b) over the block; totals to every thread.
// scratch: 2*BLOCK/64 uint32.
template <int BLOCK>
__device__ __forceinline__ void blockExclusiveScanPair(uint32_t & a, uint32_t & b, uint32_t & total_a, uint32_t & total_b,
                                                       uint32_t * scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ta = __shfl_up(ia, d, 64), tb = __shfl_up(ib, d, 64);
        if (lane >= d) {
            ia += ta;
            ib += tb;
        }
    }
    __syncthreads();
    if (lane == 63) {
        scratch[2 * wave] = ia;
        scratch[2 * wave + 1] = ib;
    }
    __syncthreads();
    uint32_t off_a = 0, off_b = 0, ta = 0, tb = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        const uint32_t xa = scratch[2 * w], xb = scratch[2 * w + 1];
        if (w < wave) {
            off_a += xa;
            off_b += xb;
        }
        ta += xa;
        tb += xb;
    }
    a = off_a + ia - a;
    b = off_b + ib - b;
    total_a = ta;
    total_b = tb;
}
}  // namespace

#endif
