// What the two text builders share on the device side (table_text.hip: a row per path; set_text.hip: a row per path group set): the
// resident handle behind rpvg_hip_table_text, the guards around a text, the wavefront's flush of its staging block (flushPlan,
// table_text_plan.hpp), the wave sum and the host's power-of-ten table.  Under hipcc only; everything but the handle has internal
// linkage, so each of the two files holds kernels of its own.
#ifndef RPVG_HIP_TABLE_TEXT_DEVICE_HPP
#define RPVG_HIP_TABLE_TEXT_DEVICE_HPP

#include <mutex>
#include <vector>

#include "table_kit.hpp"
#include "table_text_plan.hpp"
#include "../../include/rpvg_text.h"

struct rpvg_hip_table_text {
    rpvg_hip_ctx * ctx = nullptr;
    uint64_t num_paths = 0, num_rows = 0, num_bytes = 0;
    rpvg_hip_detail::DeviceBuffer<char> block;  // guard, text, guard
    std::vector<uint64_t> h_row_off;
    void * pinned = nullptr;   // the host copy of the text
    ~rpvg_hip_table_text() {
        if (pinned) rpvg_hip_detail::pinnedFree(pinned);
    }
    char * text() const { return block.ptr + 64; }
};

namespace {

constexpr int kBlock = 256;
constexpr uint64_t kGuardBytes = 64;
constexpr unsigned char kGuardPattern = 0xa5;
constexpr uint32_t kMaxWriteBlocks = 1u << 20;

__device__ __forceinline__ uint64_t waveSum(uint64_t v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(static_cast<unsigned long long>(v), d, 64);
    return __shfl(static_cast<unsigned long long>(v), 0, 64);
}

// the wavefront's staging block leaves (table_text_plan.hpp); [lo, hi) and base are uniform
__device__ __forceinline__ void flush(char * stage, char * text, uint64_t & base, uint32_t & lo, uint32_t & hi, const bool last, const uint32_t lane) {
    __syncthreads();  // the step's stores into the block
    const rpvg_table_text::FlushPlan p = rpvg_table_text::flushPlan(lo, hi);
    char * out = text + base;
    if (lane >= lo && lane < p.head_end) out[lane] = stage[lane];
    const uint32_t * words = reinterpret_cast<const uint32_t *>(stage);
    uint32_t * out_words = reinterpret_cast<uint32_t *>(out);
    for (uint32_t w = p.first_word + lane; w < p.end_word; w += 64) out_words[w] = words[w];
    const uint32_t behind = hi - p.tail_begin;  // at most 3
    if (last) {
        if (lane < behind) out[p.tail_begin + lane] = stage[p.tail_begin + lane];
        __syncthreads();  // the block is free for the next row
        return;
    }
    char carried = 0;
    if (lane < behind) carried = stage[p.tail_begin + lane];
    __syncthreads();
    if (lane < behind) stage[p.next_lo + lane] = carried;
    base += p.advance;
    lo = p.next_lo;
    hi = p.next_hi;
}

__global__ __launch_bounds__(128) void guardKernel(char * block, const uint64_t num_bytes) {
    const uint32_t i = threadIdx.x;
    block[i < kGuardBytes ? i : num_bytes + i] = static_cast<char>(kGuardPattern);
}

const uint64_t * pow10Table() {
    static uint64_t words[rpvg_number_text::kPow10Words];
    static std::once_flag once;
    std::call_once(once, [] { rpvg_number_text::buildPow10Table(words, nullptr); });
    return words;
}

}  // namespace

#endif
