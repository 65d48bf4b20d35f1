// What every device table needs (align_index.hip, path_table.hip, estimates_table.hip, gibbs_table.hip, table_text.hip, set_text.hip): one validated flat input,
// one build call, one resident handle, one host view.  Nothing here knows a particular table; a helper is here because at least two
// of the six files call it.
//
// The first part is pure computation in plain C++17 under the RPVG_PLAN_FN convention of the *_plan.hpp files, so a CPU program
// reaches it (tests/cpp/table_kit_check.cpp); the second part, under hipcc only, needs common.hpp.
#ifndef RPVG_HIP_TABLE_KIT_HPP
#define RPVG_HIP_TABLE_KIT_HPP

#include <cstdint>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_hip_detail {

typedef unsigned long long word64;

// ---- the offender word ---------------------------------------------------------------------------------------------------
// A describe or validate kernel reports every offence it meets with one atomicMin on one 64-bit word that starts as kNoBad; the
// host decodes the word that is left and words the message (each builder has its own kReasons).  The word of an offence is
//     kind * 2^62 + index * kWhyRadix + why        with 1 <= why < kWhyRadix, index < 2^58, kind 0 or 1.
// Within one kind the words order by index first and by reason second, whatever the radix (why < radix, so a larger index always
// gives a larger word): the minimum is the smallest offending index and, of its offences, the smallest reason.  With both kinds
// in one word (gibbs_table.hip: kind 0 a cluster, kind 1 a block) every word of kind 0 is below 2^62 and every word of kind 1 is
// not, so an offence of kind 0 comes back whenever there is one, whatever its index, and across kinds the order depends on the
// kind bit alone.  The indices of a table are below 2^31 (a word below 2^35), far from the kind bit and from kNoBad.
constexpr word64 kNoBad = ~0ull;
constexpr word64 kWhyRadix = 16;
constexpr word64 kSecondKind = 1ull << 62;

RPVG_PLAN_FN word64 offenderWord(const uint64_t index, const int why, const bool second_kind = false) {
    return (second_kind ? kSecondKind : 0ull) + static_cast<word64>(index) * kWhyRadix + static_cast<word64>(why);
}

struct Offender {
    bool second_kind;
    uint64_t index;
    int why;  // 0: none of the reasons the caller knows
};

// the offender of a word other than kNoBad; a reason above max_why comes back as 0 (the "" of a kReasons table)
RPVG_PLAN_FN Offender offenderOf(const word64 bad, const int max_why) {
    const bool second_kind = bad >= kSecondKind;
    const word64 word = second_kind ? bad - kSecondKind : bad;
    const int why = static_cast<int>(word % kWhyRadix);
    return Offender{second_kind, static_cast<uint64_t>(word / kWhyRadix), why <= max_why ? why : 0};
}

// the last index i in [0, n) with off[i] <= x (0 when there is none); any contents of `off` leave the result inside [0, n)
RPVG_PLAN_FN uint64_t lastAtMost(const uint64_t * __restrict__ off, const uint64_t n, const uint64_t x) {
    uint64_t lo = 0, hi = n;  // first index with off > x
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

// off[i] .. off[i + 1] of an array of n + 1 offsets that must run from 0 to `total` without decreasing
RPVG_PLAN_FN bool offsetsBad(const uint64_t * __restrict__ off, const uint64_t i, const uint64_t n, const uint64_t total) {
    const uint64_t o0 = off[i], o1 = off[i + 1];
    return o0 > o1 || o1 > total || (i == 0 && o0 != 0) || (i + 1 == n && o1 != total);
}

}  // namespace rpvg_hip_detail

#if defined(__HIPCC__)

#include "common.hpp"

namespace rpvg_hip_detail {

__device__ __forceinline__ void reportOffender(word64 * bad, const uint64_t index, const int why, const bool second_kind = false) {
    atomicMin(bad, offenderWord(index, why, second_kind));
}

// Appends `item` of every lane with a route in [0, ROUTES) to the list of its route (list r lies from r * stride): one integer
// atomic per wavefront and route (tens of thousands of items on one counter took 0.55 ms), the wavefront's items behind one
// another in lane order.  Called by whole wavefronts; a lane without an item passes a route of -1.
template <int ROUTES, typename Stride>
__device__ __forceinline__ void appendToRouteList(const int my_route, const uint32_t item, uint32_t * counters, uint32_t * lists, const Stride stride) {
    for (int route = 0; route < ROUTES; ++route) {
        const word64 with_route = __ballot(my_route == route);
        if (with_route == 0) continue;
        const int lane = threadIdx.x & 63, leader = __ffsll(static_cast<long long>(with_route)) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&counters[route], static_cast<uint32_t>(__popcll(with_route)));
        base = __shfl(base, leader, 64);
        if (my_route == route) {
            const uint32_t at = base + __popcll(with_route & ((1ull << lane) - 1ull));
            if (at < stride) lists[static_cast<uint64_t>(route) * stride + at] = item;
        }
    }
}

// a timed span that is closed on every way out of a function, the error returns included
struct SpanScope {
    rpvg_hip_ctx * ctx;
    int span;
    SpanScope(rpvg_hip_ctx * ctx_in, const int family) : ctx(ctx_in), span(ctx_in->spanBegin(family)) {}
    SpanScope(const SpanScope &) = delete;
    SpanScope & operator=(const SpanScope &) = delete;
    void end() {
        if (ctx) ctx->spanEnd(span);
        ctx = nullptr;
    }
    ~SpanScope() { end(); }
};

// an input array and where it lies: copied with the pack, or the caller's device memory where it is
template <typename T>
struct Source {
    const T * from = nullptr;
    bool on_device = false;
};

template <typename T>
void takeInput(UploadPack & pack, DeviceBuffer<T> & buffer, const Source<T> & source, const size_t n) {
    if (source.on_device) buffer.borrow(const_cast<T *>(source.from), n);
    else pack.add(buffer, source.from, n);
}

// What a describe pass left, in one wait: the offender word and, with num_counters > 0, that many counters.
inline int fetchDescribed(hipStream_t st, const word64 * d_bad, word64 * bad, const uint32_t * d_counters = nullptr, uint32_t * counters = nullptr,
                          const size_t num_counters = 0) {
    RPVG_HIP_CHECK(hipMemcpyAsync(bad, d_bad, sizeof(*bad), hipMemcpyDeviceToHost, st));
    if (num_counters) RPVG_HIP_CHECK(hipMemcpyAsync(counters, d_counters, num_counters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    return RPVG_HIP_OK;
}

// The same for a describe pass that leaves 64-bit words behind its offender word (words[0]; the totals that size the next pass):
// ONE copy of num_words adjacent device words into page-locked memory (a copy into pageable memory is staged by the runtime and
// holds the calling thread), one wait.
inline int fetchDescribedWords(hipStream_t st, const word64 * d_words, word64 * words, const size_t num_words) {
    void * pinned = nullptr;
    if (pinnedAlloc(&pinned, num_words * sizeof(word64)) != hipSuccess) {
        setError("fetchDescribedWords: out of page-locked host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    hipError_t e = hipMemcpyAsync(pinned, d_words, num_words * sizeof(word64), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) std::memcpy(words, pinned, num_words * sizeof(word64));
    pinnedFree(pinned);
    RPVG_HIP_CHECK(e);
    return RPVG_HIP_OK;
}

// The first half of every *_free: nothing queued on the context's stream may still use the handle's blocks.  The caller deletes.
inline void waitAndDelete(rpvg_hip_ctx * ctx) {
    if (!ctx) return;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    (void) hipSetDevice(ctx->device);
    (void) hipStreamSynchronize(ctx->stream);
}

}  // namespace rpvg_hip_detail

#endif  // __HIPCC__

#endif
