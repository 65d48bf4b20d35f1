// Whole-array scans and sorts (hipcub) and small host helpers shared by align_index.hip, path_table.hip, estimates_table.hip,
// gibbs_table.hip and path_cover_grid.hip.  Each scan or sort allocates its temporary storage from the pool and waits for the
// stream before it goes back.
#ifndef RPVG_HIP_DEVICE_ALGOS_HPP
#define RPVG_HIP_DEVICE_ALGOS_HPP

#include <hipcub/hipcub.hpp>

#include "common.hpp"

namespace rpvg_hip_detail {

struct MaxU32 {
    __host__ __device__ __forceinline__ uint32_t operator()(const uint32_t a, const uint32_t b) const { return a > b ? a : b; }
};

inline dim3 gridFor(const uint64_t n, const uint32_t per_block = 256) { return dim3(static_cast<uint32_t>((n + per_block - 1) / per_block)); }

template <typename In, typename Out>
int exclusiveSum(hipStream_t st, const In * in, Out * out, const uint64_t n) {
    if (n == 0) return RPVG_HIP_OK;
    size_t bytes = 0;
    RPVG_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, static_cast<int>(n), st));
    DeviceBuffer<uint8_t> tmp;
    RPVG_HIP_CHECK(tmp.alloc(bytes ? bytes : 1));
    RPVG_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.ptr, bytes, in, out, static_cast<int>(n), st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // tmp goes back to the pool
    return RPVG_HIP_OK;
}

template <typename In, typename Out, typename Op>
int inclusiveScan(hipStream_t st, const In * in, Out * out, const Op op, const uint64_t n) {
    if (n == 0) return RPVG_HIP_OK;
    size_t bytes = 0;
    RPVG_HIP_CHECK(hipcub::DeviceScan::InclusiveScan(nullptr, bytes, in, out, op, static_cast<int>(n), st));
    DeviceBuffer<uint8_t> tmp;
    RPVG_HIP_CHECK(tmp.alloc(bytes ? bytes : 1));
    RPVG_HIP_CHECK(hipcub::DeviceScan::InclusiveScan(tmp.ptr, bytes, in, out, op, static_cast<int>(n), st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

template <typename In, typename Out>
int inclusiveSum(hipStream_t st, const In * in, Out * out, const uint64_t n) {
    if (n == 0) return RPVG_HIP_OK;
    size_t bytes = 0;
    RPVG_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, in, out, static_cast<int>(n), st));
    DeviceBuffer<uint8_t> tmp;
    RPVG_HIP_CHECK(tmp.alloc(bytes ? bytes : 1));
    RPVG_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp.ptr, bytes, in, out, static_cast<int>(n), st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

// out[i] = i for i < n (a template so that only the files that queue it hold the kernel)
template <typename Index>
__global__ void iotaKernel(const uint64_t n, Index * __restrict__ out) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < n) out[i] = static_cast<Index>(i);
}

template <typename Key, typename Value>
int sortPairs(hipStream_t st, const Key * key_in, Key * key_out, const Value * value_in, Value * value_out, const uint64_t n, const int end_bit) {
    if (n == 0) return RPVG_HIP_OK;
    size_t bytes = 0;
    RPVG_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key_in, key_out, value_in, value_out, static_cast<int>(n), 0, end_bit, st));
    DeviceBuffer<uint8_t> tmp;
    RPVG_HIP_CHECK(tmp.alloc(bytes ? bytes : 1));
    RPVG_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.ptr, bytes, key_in, key_out, value_in, value_out, static_cast<int>(n), 0, end_bit, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

template <typename T>
int fetchOne(hipStream_t st, const T * device, T * host) {
    RPVG_HIP_CHECK(hipMemcpyAsync(host, device, sizeof(T), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

template <typename T>
int downloadVector(hipStream_t st, const T * device, const size_t n, std::vector<T> & host) {
    host.assign(n, T());
    if (n) RPVG_HIP_CHECK(hipMemcpyAsync(host.data(), device, n * sizeof(T), hipMemcpyDeviceToHost, st));
    return RPVG_HIP_OK;
}

}  // namespace rpvg_hip_detail

#endif
