// Context, device memory helpers (pools, pinned memory, streams) and kernel timing of
// librpvg_hip.so; the device batch and its makers are batch_upload.hip's.  gfx950 only; no CPU fallback anywhere in this library.

#include "common.hpp"

#include <sys/prctl.h>
#include <time.h>

#include <algorithm>
#include <thread>

#include <map>

namespace rpvg_hip_detail {

static thread_local char g_last_error[1024] = "";

void setError(const char * fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
}

namespace {

struct DevicePool {
    std::map<size_t, std::vector<void *>> free_blocks;  // size class -> cached blocks
    std::map<void *, size_t> live;                      // block -> size class
};

std::mutex g_pool_mutex;
std::map<int, DevicePool> g_pools;
std::map<void *, int> g_block_device;
std::map<int, int> g_device_contexts;

// power-of-two classes below 1 MiB, eight classes per octave above
size_t sizeClass(size_t bytes) {
    if (bytes <= 256) return 256;
    size_t pow2 = 256;
    while (pow2 < bytes) pow2 <<= 1;
    if (pow2 <= (1u << 20)) return pow2;
    const size_t step = pow2 >> 4;  // pow2/2 .. pow2 in 8 steps
    return ((bytes + step - 1) / step) * step;
}

}  // namespace

hipError_t poolAlloc(void ** ptr, size_t bytes) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    const size_t cls = sizeClass(bytes);
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        DevicePool & pool = g_pools[device];
        auto it = pool.free_blocks.find(cls);
        if (it != pool.free_blocks.end() && !it->second.empty()) {
            *ptr = it->second.back();
            it->second.pop_back();
            pool.live[*ptr] = cls;
            return hipSuccess;
        }
    }
    {
        static const bool trace = std::getenv("RPVG_AMD_TRACE") != nullptr;
        if (trace) std::fprintf(stderr, "[rpvg_hip trace] pool miss: device block of %zu bytes\n", cls);
    }
    e = hipMalloc(ptr, cls);
    if (e == hipErrorOutOfMemory) {
        // give cached blocks back to the driver and retry once
        (void) hipGetLastError();
        poolTrim(device);
        e = hipMalloc(ptr, cls);
    }
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    g_pools[device].live[*ptr] = cls;
    g_block_device[*ptr] = device;
    return hipSuccess;
}

void poolFree(void * ptr) {
    if (!ptr) return;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    auto dev_it = g_block_device.find(ptr);
    if (dev_it == g_block_device.end()) {
        (void) hipFree(ptr);
        return;
    }
    DevicePool & pool = g_pools[dev_it->second];
    auto it = pool.live.find(ptr);
    if (it == pool.live.end()) return;
    pool.free_blocks[it->second].push_back(ptr);
    pool.live.erase(it);
}

void poolTrim(int device) {
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    DevicePool & pool = g_pools[device];
    for (auto & cls : pool.free_blocks) {
        for (void * p : cls.second) {
            (void) hipFree(p);
            g_block_device.erase(p);
        }
        cls.second.clear();
    }
}

namespace {
std::mutex g_pinned_mutex;
std::map<size_t, std::vector<void *>> g_pinned_free;  // size class -> cached blocks
std::map<void *, size_t> g_pinned_live;
}  // namespace

hipError_t pinnedAlloc(void ** ptr, size_t bytes) {
    const size_t cls = sizeClass(bytes);
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        auto it = g_pinned_free.find(cls);
        if (it != g_pinned_free.end() && !it->second.empty()) {
            *ptr = it->second.back();
            it->second.pop_back();
            g_pinned_live[*ptr] = cls;
            return hipSuccess;
        }
    }
    {
        static const bool trace = std::getenv("RPVG_AMD_TRACE") != nullptr;
        if (trace) std::fprintf(stderr, "[rpvg_hip trace] pool miss: pinned block of %zu bytes\n", cls);
    }
    const hipError_t e = hipHostMalloc(ptr, cls, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        *ptr = nullptr;
        return e;
    }
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    g_pinned_live[*ptr] = cls;
    return hipSuccess;
}

size_t pinnedCapacity(const void * ptr) {
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    auto it = g_pinned_live.find(const_cast<void *>(ptr));
    return it == g_pinned_live.end() ? 0 : it->second;
}

void pinnedFree(void * ptr) {
    if (!ptr) return;
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    auto it = g_pinned_live.find(ptr);
    if (it == g_pinned_live.end()) return;
    g_pinned_free[it->second].push_back(ptr);
    g_pinned_live.erase(it);
}

void pinnedTrim() {
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (auto & cls : g_pinned_free) {
        for (void * p : cls.second) (void) hipHostFree(p);
        cls.second.clear();
    }
}

bool stagedUploads() {
    static const bool staged = std::getenv("RPVG_HIP_PAGEABLE_UPLOADS") == nullptr;
    return staged;
}

namespace {
std::mutex g_registered_mutex;
std::map<const char *, size_t> g_registered;  // start -> bytes of the ranges registered through the library
}  // namespace

bool hostIsPinned(const void * host, size_t bytes) {
    if (!host || bytes == 0) return false;
    std::lock_guard<std::mutex> lock(g_registered_mutex);
    if (g_registered.empty()) return false;
    const char * p = static_cast<const char *>(host);
    auto it = g_registered.upper_bound(p);
    if (it == g_registered.begin()) return false;
    --it;
    return p >= it->first && p + bytes <= it->first + it->second;
}

void copyToStaging(void * staging, const void * host, size_t bytes) {
    constexpr size_t kChunk = 8u << 20;
    if (bytes < 2 * kChunk) {
        std::memcpy(staging, host, bytes);
        return;
    }
    const size_t threads = std::min<size_t>(8, (bytes + kChunk - 1) / kChunk);
    const size_t share = ((bytes + threads - 1) / threads + 63) & ~size_t(63);
    std::vector<std::thread> workers;
    for (size_t t = 1; t < threads; ++t) {
        const size_t begin = t * share;
        if (begin >= bytes) break;
        workers.emplace_back([=] { std::memcpy(static_cast<char *>(staging) + begin, static_cast<const char *>(host) + begin, std::min(share, bytes - begin)); });
    }
    std::memcpy(staging, host, std::min(share, bytes));
    for (auto & w : workers) w.join();
}

namespace {
struct CopyLane {
    hipStream_t copy_stream;
    hipEvent_t copied;
};
std::mutex g_copy_mutex;
std::map<hipStream_t, CopyLane> g_copy_lanes;
}  // namespace

void registerCopyStream(hipStream_t stream, hipStream_t copy_stream, hipEvent_t copied) {
    std::lock_guard<std::mutex> lock(g_copy_mutex);
    g_copy_lanes[stream] = CopyLane{copy_stream, copied};
}

void forgetCopyStream(hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_copy_mutex);
    g_copy_lanes.erase(stream);
}

hipError_t stagedCopy(void * device_dst, const void * pinned_src, size_t bytes, hipStream_t stream) {
    // (measured on the configs[2] bench: 19.1-19.9 ms per batch with the copy stream against 14.4-15.8 ms with the
    // uploads on their own streams — the event waits between hardware queues cost more than the overlap brings; off
    // unless RPVG_HIP_COPY_STREAM=1)
    static const bool inline_uploads = RPVG_EXPERIMENT_ENV("RPVG_HIP_COPY_STREAM") == nullptr;
    CopyLane lane{nullptr, nullptr};
    if (!inline_uploads) {
        std::lock_guard<std::mutex> lock(g_copy_mutex);
        auto it = g_copy_lanes.find(stream);
        if (it != g_copy_lanes.end()) lane = it->second;
    }
    if (!lane.copy_stream) return hipMemcpyAsync(device_dst, pinned_src, bytes, hipMemcpyHostToDevice, stream);
    hipError_t e = hipMemcpyAsync(device_dst, pinned_src, bytes, hipMemcpyHostToDevice, lane.copy_stream);
    if (e == hipSuccess) e = hipEventRecord(lane.copied, lane.copy_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, lane.copied, 0);
    return e;
}

namespace {

int g_hardware_queues = 4;

__attribute__((constructor)) void askForHardwareQueues() {
    // (8: two host lanes of nine streams over one batch — 12 and 16 measured equal or slower there — and, since round 5, the batch
    // pipeline's four single-lane engines of four streams each: 6.0 ms per configs[2] batch on 8 queues, 6.1 on 6, 6.6 on 4, 7.0 on
    // 10, 5.9 on 12, 8.7 on 16; engines of nine streams each wanted 16 — rpvg_amd/host/batch_pipeline.hpp)
    (void) setenv("GPU_MAX_HW_QUEUES", "8", 0);  // keeps a value the user has set
    const char * env = std::getenv("GPU_MAX_HW_QUEUES");
    g_hardware_queues = env ? std::max(1, std::atoi(env)) : 4;
}

}  // namespace

int hardwareQueues() { return g_hardware_queues; }

}  // namespace rpvg_hip_detail

using namespace rpvg_hip_detail;

namespace rpvg_hip_detail {

namespace {

// how long a wait of the calling thread queries before it starts to nap (rpvg_hip_thread_wait_spin_us)
thread_local uint32_t t_spin_us = 20;

template <typename Query>
hipError_t pollUntilDone(Query query) {
    static const bool spin = std::getenv("RPVG_HIP_SPIN_WAITS") != nullptr;
    if (spin) return hipErrorNotSupported;  // (the caller falls back to the runtime's wait)
    thread_local bool slack_set = false;
    if (!slack_set) {
        (void) prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
        slack_set = true;
    }
    const auto begin = std::chrono::steady_clock::now();
    const auto spin_for = std::chrono::microseconds(t_spin_us);
    while (true) {
        const hipError_t e = query();
        if (e != hipErrorNotReady) return e;
        const auto waited = std::chrono::steady_clock::now() - begin;
        if (waited < spin_for) continue;
        // naps of a twentieth of the time waited so far, 30 to 200 us: a nap is ~15 us of CPU time (timer, two context switches), and
        // a wait of many milliseconds — a round of the device sampler, a large cluster's EM — took hundreds of them (8 ms of system
        // time per configs[4] call); the wait ends at most 5 % late
        const long nap_ns = std::min<long>(200000, std::max<long>(30000, std::chrono::duration_cast<std::chrono::nanoseconds>(waited).count() / 20));
        timespec nap{0, nap_ns};
        (void) nanosleep(&nap, nullptr);
    }
}

}  // namespace

namespace {
__global__ void zeroWordsKernel(uint32_t * __restrict__ words, const size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) words[i] = 0u;
}
}  // namespace

hipError_t zeroAsync(void * ptr, const size_t bytes, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(ptr) & 3u) || (bytes & 3u)) return hipMemsetAsync(ptr, 0, bytes, stream);
    const size_t n = bytes / 4;
    const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((n + 255) / 256, 2048));
    zeroWordsKernel<<<dim3(blocks), dim3(256), 0, stream>>>(static_cast<uint32_t *>(ptr), n);
    return hipGetLastError();
}

hipError_t waitEvent(hipEvent_t event) {
    const hipError_t e = pollUntilDone([event]() { return hipEventQuery(event); });
    return e == hipErrorNotSupported ? hipEventSynchronize(event) : e;
}

hipError_t waitStream(hipStream_t stream) {
    const hipError_t e = pollUntilDone([stream]() { return hipStreamQuery(stream); });
    return e == hipErrorNotSupported ? hipStreamSynchronize(stream) : e;
}

}  // namespace rpvg_hip_detail

hipError_t rpvg_hip_ctx::forkAux() {
    hipError_t e = hipEventRecord(fork_event, stream);
    for (int i = 0; i < aux_count && e == hipSuccess; ++i) e = hipStreamWaitEvent(aux[i], fork_event, 0);
    return e;
}

hipError_t rpvg_hip_ctx::joinAux() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < aux_count && e == hipSuccess; ++i) {
        e = hipEventRecord(join_event[i], aux[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, join_event[i], 0);
    }
    return e;
}

// joinAux() with the submitting thread waiting for the side streams itself: `stream` is not left parked on their events (a
// stream whose next command waits for an event holds its hardware queue until it arrives, and the kernels of other
// streams on that queue — the other lane's — stand behind it)
hipError_t rpvg_hip_ctx::joinAuxOnHost() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < aux_count && e == hipSuccess; ++i) e = hipEventRecord(join_event[i], aux[i]);
    for (int i = 0; i < aux_count && e == hipSuccess; ++i) e = rpvg_hip_detail::waitEvent(join_event[i]);
    for (int i = 0; i < aux_count && e == hipSuccess; ++i) e = hipStreamWaitEvent(stream, join_event[i], 0);  // (the ordering, for the record: they have arrived)
    return e;
}

namespace rpvg_hip_detail {
namespace {
// The clock of the timed intervals: one event per GPU that every span of every context on it is measured against
// (hipEventElapsedTime returns a float: the base is renewed by a statistics reset once it is older than a few
// seconds, so that the intervals of a measurement keep microsecond resolution).
struct DeviceClock {
    hipEvent_t base = nullptr;
    uint64_t id = 0;
    std::chrono::steady_clock::time_point taken;
};
std::mutex g_clock_mutex;
std::map<int, DeviceClock> g_clocks;

// Caller has set the device.  renew_if_old: take a new base when the present one is older than five seconds.
DeviceClock deviceClock(const int device, hipStream_t stream, const bool renew_if_old) {
    std::lock_guard<std::mutex> lock(g_clock_mutex);
    DeviceClock & clock = g_clocks[device];
    const auto now = std::chrono::steady_clock::now();
    if (!clock.base || (renew_if_old && now - clock.taken > std::chrono::seconds(5))) {
        hipEvent_t base = nullptr;
        // (the previous base is not destroyed: spans of other contexts may still be folded against it)
        if (hipEventCreate(&base) == hipSuccess && hipEventRecord(base, stream) == hipSuccess && hipEventSynchronize(base) == hipSuccess) {
            clock.base = base;
            clock.id++;
            clock.taken = now;
        }
    }
    return clock;
}
}  // namespace
}  // namespace rpvg_hip_detail

// The spans cost what they record with: two events each, two marker commands in the stream's queue — eighty per configs[2]
// batch with all of them, between kernels that depend on each other; with several batches in flight that was 0.6 of 4.8 ms per
// batch.  span_level (rpvg_hip_ctx): 2 every family (the contexts of rpvg_hip_create: one batch at a time, the statistics
// bench.py and the tools read), 1 the EM launches only (the contexts of rpvg_hip_create_with_streams and rpvg_hip_create_uploader:
// the batch pipeline — the two events around a batch's copies alone were 0.25 of 3.8 ms per upload), 0 none; RPVG_HIP_SPANS=n when a
// context is made overrides.
int rpvg_hip_ctx::spanBegin(int family, hipStream_t on, int sub) {
    if (span_level <= 0 || (span_level == 1 && family != FAM_EM_KERNEL)) return -1;
    // a caller that never reads the statistics: the spans that are done are folded now and then (nothing waits: a span still
    // running stays), once no span is open — handles are positions in the list
    if (open_spans == 0 && spans.size() >= 1024) foldFinishedSpans();
    TimedSpan s;
    s.family = family;
    s.sub = sub;
    if (hipEventCreate(&s.start) != hipSuccess) return -1;
    if (hipEventCreate(&s.stop) != hipSuccess) {
        (void) hipEventDestroy(s.start);
        return -1;
    }
    if (!on) on = stream;
    (void) hipEventRecord(s.start, on);
    spans.push_back(s);
    span_streams.push_back(on);
    ++open_spans;
    return static_cast<int>(spans.size()) - 1;
}

void rpvg_hip_ctx::spanEnd(int idx) {
    if (idx < 0) return;
    (void) hipEventRecord(spans[idx].stop, span_streams[idx]);
    if (open_spans > 0) --open_spans;
}

// what a finished span adds to the statistics (the caller destroys its events)
void rpvg_hip_ctx::accountSpan(const rpvg_hip_detail::TimedSpan & s, const void * clock_base, const uint64_t clock_id) {
    constexpr size_t kMaxIntervals = 1u << 20;
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.start, s.stop) != hipSuccess) return;
    switch (s.family) {
        case FAM_EM_SPARSE: stats.em_sparse_ms += ms; break;
        case FAM_EM_DENSE: stats.em_dense_ms += ms; break;
        case FAM_LOGLIK: stats.loglik_ms += ms; break;
        case FAM_BUILD: stats.build_ms += ms; break;
        case FAM_H2D: stats.h2d_ms += ms; break;
        case FAM_COLLAPSE: stats.collapse_ms += ms; break;
        case FAM_GIBBS: stats.gibbs_ms += ms; break;
        case FAM_TILE: stats.search_tile_ms += ms; stats.search_tile_launches += 1; break;
        case FAM_EM_KERNEL:
            if (s.sub >= 0 && s.sub < RPVG_HIP_EM_KERNELS) stats.em_kernel[s.sub].ms += ms;
            break;
        default: break;
    }
    float at = 0;
    // (the per-kernel spans lie inside their call's FAM_EM_SPARSE span: not a second interval)
    // (... and the conditionals' FAM_LOGLIK spans inside their sampler's FAM_GIBBS span)
    hipEvent_t base = static_cast<hipEvent_t>(const_cast<void *>(clock_base));
    if (s.family != FAM_EM_KERNEL && s.family != FAM_GIBBS && base && intervals.size() < kMaxIntervals &&
        hipEventElapsedTime(&at, base, s.start) == hipSuccess) {
        intervals.push_back(TimedInterval{static_cast<double>(at), static_cast<double>(at) + ms, s.family, clock_id});
    }
}

void rpvg_hip_ctx::foldFinishedSpans() {
    const DeviceClock clock = deviceClock(device, stream, false);
    size_t kept = 0;
    for (size_t i = 0; i < spans.size(); ++i) {
        if (hipEventQuery(spans[i].stop) == hipSuccess) {
            accountSpan(spans[i], clock.base, clock.id);
            (void) hipEventDestroy(spans[i].start);
            (void) hipEventDestroy(spans[i].stop);
        } else {
            (void) hipGetLastError();
            spans[kept] = spans[i];
            span_streams[kept] = span_streams[i];
            ++kept;
        }
    }
    (void) hipGetLastError();
    spans.resize(kept);
    span_streams.resize(kept);
}

int rpvg_hip_ctx::foldSpans() {
    RPVG_HIP_CHECK(hipStreamSynchronize(stream));
    if (collapse_stream) RPVG_HIP_CHECK(hipStreamSynchronize(collapse_stream));
    const DeviceClock clock = deviceClock(device, stream, false);
    for (auto & s : spans) {
        (void) hipEventSynchronize(s.stop);  // spans on side streams
        accountSpan(s, clock.base, clock.id);
        (void) hipGetLastError();
        (void) hipEventDestroy(s.start);
        (void) hipEventDestroy(s.stop);
    }
    spans.clear();
    span_streams.clear();
    open_spans = 0;
    // union of the intervals on the present clock
    std::vector<std::pair<double, double>> iv;
    for (auto & t : intervals) {
        if (t.clock == clock.id) iv.emplace_back(t.start_ms, t.stop_ms);
    }
    std::sort(iv.begin(), iv.end());
    double busy = 0, cur_s = 0, cur_e = -1;
    for (auto & x : iv) {
        if (cur_e < cur_s || x.first > cur_e) {
            if (cur_e >= cur_s) busy += cur_e - cur_s;
            cur_s = x.first;
            cur_e = x.second;
        } else if (x.second > cur_e) {
            cur_e = x.second;
        }
    }
    if (cur_e >= cur_s) busy += cur_e - cur_s;
    stats.busy_ms = busy;
    return RPVG_HIP_OK;
}

extern "C" {

int rpvg_hip_device_count(int * count) {
    RPVG_REQUIRE(count != nullptr, "rpvg_hip_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        setError("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        *count = 0;
        return RPVG_HIP_ERR_NO_DEVICE;
    }
    *count = n;
    return RPVG_HIP_OK;
}

namespace {
// The context's own stream carries the short kernels that stand between a host lane and its next stage (matrix build,
// row collapse, EM problem set); the long ones — the searches, the EM bins — run on the side streams.  With a higher
// priority the short ones of one lane get their workgroups in between those of the other lane's long kernels
// — the idea; measured 17.4-17.8 ms per configs[2] batch against 15.1-15.9 ms with all streams alike (same box, same
// call), so it is off unless RPVG_HIP_MAIN_PRIORITY=1.
hipError_t createMainStream(hipStream_t * stream, const bool highest_priority) {
    const char * env = RPVG_EXPERIMENT_ENV("RPVG_HIP_MAIN_PRIORITY");  // A/B knob: every context's stream at the highest priority (slower)
    if (!highest_priority && (!env || std::atoi(env) == 0)) return hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) {
        (void) hipGetLastError();
        return hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
    }
    return hipStreamCreateWithPriority(stream, hipStreamNonBlocking, greatest);
}

// The runtime maps its streams onto a pool of GPU_MAX_HW_QUEUES hardware queues per priority (least used first), and the
// commands of streams that share a queue run one after the other.  With several batches in flight (the contexts of few side
// streams: rpvg_hip_create_with_streams) that is where a batch's time went: the main stream — the chain of dependent kernels
// from the matrices to the packed results — shared its queue with other contexts' side streams, whose EM kernels run for a
// millisecond each.  A stream with a CU mask gets a hardware queue of its own, outside the pools; the mask here names every
// CU.  5.7 -> 5.1-5.2 ms per configs[2] batch with four such contexts; the side or collapse streams as well: 14 and 7 ms —
// beyond some twenty hardware queues in the process the device time-slices them (GPU_MAX_HW_QUEUES=10: 8 ms).
// RPVG_HIP_POOLED_MAIN_QUEUE=1: the main stream from the pool, as in the contexts of rpvg_hip_create.
bool ownQueueForMainStream(const bool uploader, const int side_streams) {
    static const bool pooled = std::getenv("RPVG_HIP_POOLED_MAIN_QUEUE") != nullptr && std::atoi(std::getenv("RPVG_HIP_POOLED_MAIN_QUEUE")) != 0;
    return !uploader && side_streams < rpvg_hip_ctx::kAuxStreams && !pooled;
}

hipError_t createOwnQueueStream(hipStream_t * stream, const int num_cus) {
    uint32_t every_cu[32];
    for (uint32_t & word : every_cu) word = 0xffffffffu;
    const uint32_t words = static_cast<uint32_t>(std::min(32, std::max(1, (num_cus + 31) / 32)));  // (256 CUs: eight words; bits past the device's last are ignored)
    hipError_t e = hipExtStreamCreateWithCUMask(stream, words, every_cu);
    if (e != hipSuccess) {  // (a runtime or a partition mode that does not take the mask: a stream of the pool, as everywhere else)
        (void) hipGetLastError();
        e = hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
    }
    return e;
}

int createContext(int device, bool uploader, int side_streams, rpvg_hip_ctx ** ctx_out);
}  // namespace

int rpvg_hip_create(int device, rpvg_hip_ctx ** ctx_out) { return createContext(device, false, rpvg_hip_ctx::kAuxStreams, ctx_out); }

int rpvg_hip_create_uploader(int device, rpvg_hip_ctx ** ctx_out) { return createContext(device, true, 1, ctx_out); }

int rpvg_hip_create_with_streams(int device, int side_streams, rpvg_hip_ctx ** ctx_out) {
    RPVG_REQUIRE(side_streams >= 1 && side_streams <= rpvg_hip_ctx::kAuxStreams, "rpvg_hip_create_with_streams: 1 to %d side streams", rpvg_hip_ctx::kAuxStreams);
    return createContext(device, false, side_streams, ctx_out);
}

namespace {
int createContext(int device, const bool uploader, const int side_streams, rpvg_hip_ctx ** ctx_out) {
    RPVG_REQUIRE(ctx_out != nullptr, "rpvg_hip_create: ctx_out is NULL");
    *ctx_out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        setError("rpvg_hip_create: no HIP device available (%s); this engine has no CPU fallback",
                 e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return RPVG_HIP_ERR_NO_DEVICE;
    }
    RPVG_REQUIRE(device >= 0 && device < n, "rpvg_hip_create: device %d out of range [0, %d)", device, n);
    rpvg_hip_ctx * ctx = new (std::nothrow) rpvg_hip_ctx();
    if (!ctx) {
        setError("rpvg_hip_create: out of host memory");
        return RPVG_HIP_ERR_ALLOC;
    }
    ctx->device = device;
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    {
        const char * env = std::getenv("RPVG_HIP_SPANS");  // (read per context)
        ctx->span_level = env ? std::max(0, std::min(2, std::atoi(env))) : ((uploader || side_streams < rpvg_hip_ctx::kAuxStreams) ? 1 : 2);
    }
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&ctx->props, device)) != hipSuccess ||
        (e = ownQueueForMainStream(uploader, side_streams) ? createOwnQueueStream(&ctx->stream, ctx->props.multiProcessorCount) : createMainStream(&ctx->stream, uploader)) != hipSuccess) {
        setError("rpvg_hip_create: %s", hipGetErrorString(e));
        delete ctx;
        return RPVG_HIP_ERR_RUNTIME;
    }
    // side_streams real side streams; the other entries of aux[] are aliases of them, so that every use site keeps its index
    // (launches that would have had streams of their own then follow one another on the stream they share)
    ctx->aux_count = side_streams;
    for (int i = 0; i < rpvg_hip_ctx::kAuxStreams && e == hipSuccess; ++i) {
        if (i < side_streams) {
            e = hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->join_event[i], hipEventDisableTiming);
        } else {
            ctx->aux[i] = ctx->aux[i % side_streams];
        }
    }
    if (e == hipSuccess) e = createMainStream(&ctx->collapse_stream, RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_PRIORITY") == nullptr || std::atoi(RPVG_EXPERIMENT_ENV("RPVG_HIP_COLLAPSE_PRIORITY")) != 0);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->fork_event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->search_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->copied, hipEventDisableTiming);
    if (e == hipSuccess) {
        registerCopyStream(ctx->stream, ctx->copy_stream, ctx->copied);
        for (int i = 0; i < ctx->aux_count; ++i) registerCopyStream(ctx->aux[i], ctx->copy_stream, ctx->copied);
    }
    if (e != hipSuccess) {
        setError("rpvg_hip_create: %s", hipGetErrorString(e));
        delete ctx;
        return RPVG_HIP_ERR_RUNTIME;
    }
    if (strncmp(ctx->props.gcnArchName, "gfx950", 6) != 0) {
        setError("rpvg_hip_create: device %d is %s; this library is built for gfx950 only", device, ctx->props.gcnArchName);
        (void) hipStreamDestroy(ctx->stream);
        delete ctx;
        return RPVG_HIP_ERR_NO_DEVICE;
    }
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        g_device_contexts[device]++;
    }
    *ctx_out = ctx;
    return RPVG_HIP_OK;
}
}  // namespace

void rpvg_hip_destroy(rpvg_hip_ctx * ctx) {
    if (!ctx) return;
    const bool trace = std::getenv("RPVG_AMD_TRACE_EXIT") != nullptr;
#define RPVG_EXIT_STEP(what) do { if (trace) std::fprintf(stderr, "[exit]   rpvg_hip_destroy: %s\n", what); } while (0)
    RPVG_EXIT_STEP("begin");
    (void) hipSetDevice(ctx->device);
    (void) ctx->foldSpans();
    RPVG_EXIT_STEP("spans folded");
    (void) rpvg_hip_comm_destroy(ctx);
    if (ctx->stream) forgetCopyStream(ctx->stream);
    for (int i = 0; i < ctx->aux_count; ++i) {
        if (ctx->aux[i]) forgetCopyStream(ctx->aux[i]);
    }
    if (ctx->copy_stream) {
        (void) hipStreamSynchronize(ctx->copy_stream);
        (void) hipStreamDestroy(ctx->copy_stream);
    }
    RPVG_EXIT_STEP("copy stream destroyed");
    if (ctx->copied) (void) hipEventDestroy(ctx->copied);
    // Every stream drained, then the pooled streams, and the main stream last: a main stream with a hardware queue of its own
    // (createOwnQueueStream) destroyed in front of the side streams left hipStreamDestroy of the first side stream hanging in one
    // process exit of twenty (tools/r06_exit_hang.sh: the reference-shaped factory binary, whose default engine goes at exit).
    if (ctx->stream) (void) hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < ctx->aux_count; ++i) {
        if (ctx->aux[i]) (void) hipStreamSynchronize(ctx->aux[i]);
    }
    if (ctx->collapse_stream) (void) hipStreamSynchronize(ctx->collapse_stream);
    RPVG_EXIT_STEP("streams drained");
    for (int i = 0; i < ctx->aux_count; ++i) {  // (the entries behind are aliases)
        if (ctx->aux[i]) (void) hipStreamDestroy(ctx->aux[i]);
        RPVG_EXIT_STEP("a side stream destroyed");
        if (ctx->join_event[i]) (void) hipEventDestroy(ctx->join_event[i]);
    }
    if (ctx->collapse_stream) (void) hipStreamDestroy(ctx->collapse_stream);
    RPVG_EXIT_STEP("side and collapse streams destroyed");
    if (ctx->stream) (void) hipStreamDestroy(ctx->stream);
    RPVG_EXIT_STEP("main stream destroyed");
    if (ctx->fork_event) (void) hipEventDestroy(ctx->fork_event);
    for (hipStream_t grid_stream : ctx->grid_stream) {
        if (grid_stream) {
            (void) hipStreamSynchronize(grid_stream);
            (void) hipStreamDestroy(grid_stream);
        }
    }
    if (ctx->grid_ready) (void) hipEventDestroy(ctx->grid_ready);
    searchGateForget(ctx);
    if (ctx->search_done) (void) hipEventDestroy(ctx->search_done);
    bool last = false;
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        last = (--g_device_contexts[ctx->device] <= 0);
    }
    RPVG_EXIT_STEP("events destroyed");
    if (last) {
        poolTrim(ctx->device);
        RPVG_EXIT_STEP("pool trimmed");
        bool any = false;
        {
            std::lock_guard<std::mutex> lock(g_pool_mutex);
            for (auto & kv : g_device_contexts) any = any || kv.second > 0;
        }
        if (!any) pinnedTrim();
        RPVG_EXIT_STEP("pinned blocks trimmed");
    }
    delete ctx;
    RPVG_EXIT_STEP("done");
#undef RPVG_EXIT_STEP
}

const char * rpvg_hip_last_error(void) { return g_last_error; }

int rpvg_hip_subset_em_keep_device(rpvg_hip_ctx * ctx, int32_t keep) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_subset_em_keep_device: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    ctx->keep_subset_block = keep != 0;
    return RPVG_HIP_OK;
}

int rpvg_hip_synchronize(rpvg_hip_ctx * ctx) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_synchronize: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->collapse_stream) RPVG_HIP_CHECK(hipStreamSynchronize(ctx->collapse_stream));
    return RPVG_HIP_OK;
}

int rpvg_hip_device_info(rpvg_hip_ctx * ctx, char * name, uint32_t name_cap, uint32_t * num_cus, uint64_t * mem_bytes) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_device_info: ctx is NULL");
    if (name && name_cap) {
        snprintf(name, name_cap, "%s (%s)", ctx->props.name, ctx->props.gcnArchName);
    }
    if (num_cus) *num_cus = ctx->props.multiProcessorCount;
    if (mem_bytes) *mem_bytes = ctx->props.totalGlobalMem;
    return RPVG_HIP_OK;
}

int rpvg_hip_malloc(rpvg_hip_ctx * ctx, uint64_t bytes, void ** device_ptr_out) {
    RPVG_REQUIRE(ctx != nullptr && device_ptr_out != nullptr, "rpvg_hip_malloc: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(device_ptr_out, bytes);
    if (e != hipSuccess) {
        setError("rpvg_hip_malloc: %llu bytes: %s", static_cast<unsigned long long>(bytes), hipGetErrorString(e));
        return RPVG_HIP_ERR_ALLOC;
    }
    return RPVG_HIP_OK;
}

int rpvg_hip_free(rpvg_hip_ctx * ctx, void * device_ptr) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_free: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    RPVG_HIP_CHECK(hipFree(device_ptr));
    return RPVG_HIP_OK;
}

int rpvg_hip_memcpy_h2d(rpvg_hip_ctx * ctx, void * device_dst, const void * host_src, uint64_t bytes) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_memcpy_h2d: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

int rpvg_hip_memcpy_d2h(rpvg_hip_ctx * ctx, void * host_dst, const void * device_src, uint64_t bytes) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_memcpy_d2h: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_host_register(void * host, uint64_t bytes) {
    RPVG_REQUIRE(host && bytes > 0, "rpvg_hip_host_register: NULL or empty range");
    RPVG_HIP_CHECK(hipHostRegister(host, bytes, hipHostRegisterDefault));
    std::lock_guard<std::mutex> lock(g_registered_mutex);
    g_registered[static_cast<const char *>(host)] = bytes;
    return RPVG_HIP_OK;
}

extern "C" int rpvg_hip_host_unregister(void * host) {
    RPVG_REQUIRE(host, "rpvg_hip_host_unregister: NULL");
    {
        std::lock_guard<std::mutex> lock(g_registered_mutex);
        RPVG_REQUIRE(g_registered.erase(static_cast<const char *>(host)) == 1, "rpvg_hip_host_unregister: the range was not registered here");
    }
    RPVG_HIP_CHECK(hipHostUnregister(host));
    return RPVG_HIP_OK;
}

void rpvg_hip_thread_wait_spin_us(uint32_t microseconds) { t_spin_us = microseconds; }

int rpvg_hip_pinned_alloc(uint64_t bytes, void ** host_out) {
    RPVG_REQUIRE(host_out != nullptr, "rpvg_hip_pinned_alloc: host_out is NULL");
    *host_out = nullptr;
    const hipError_t e = pinnedAlloc(host_out, std::max<uint64_t>(bytes, 8));
    if (e != hipSuccess) {
        setError("rpvg_hip_pinned_alloc: %llu bytes: %s", static_cast<unsigned long long>(bytes), hipGetErrorString(e));
        return RPVG_HIP_ERR_ALLOC;
    }
    return RPVG_HIP_OK;
}

void rpvg_hip_pinned_free(void * host) { pinnedFree(host); }

int rpvg_hip_stats_get(rpvg_hip_ctx * ctx, rpvg_hip_kernel_stats * stats_out) {
    RPVG_REQUIRE(ctx != nullptr && stats_out != nullptr, "rpvg_hip_stats_get: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    int rc = ctx->foldSpans();
    if (rc != RPVG_HIP_OK) return rc;
    *stats_out = ctx->stats;
    return RPVG_HIP_OK;
}

int rpvg_hip_stats_reset(rpvg_hip_ctx * ctx) {
    RPVG_REQUIRE(ctx != nullptr, "rpvg_hip_stats_reset: ctx is NULL");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    int rc = ctx->foldSpans();
    if (rc != RPVG_HIP_OK) return rc;
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->independent_stats = rpvg_hip_independent_stats{};
    ctx->parse_stats = rpvg_hip_parse_stats{};
    ctx->intervals.clear();
    (void) deviceClock(ctx->device, ctx->stream, true);
    return RPVG_HIP_OK;
}

int rpvg_hip_stats_intervals(rpvg_hip_ctx * ctx, uint64_t capacity, double * start_ms, double * stop_ms, int32_t * family,
                             uint64_t * count_out) {
    RPVG_REQUIRE(ctx != nullptr && count_out != nullptr, "rpvg_hip_stats_intervals: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    int rc = ctx->foldSpans();
    if (rc != RPVG_HIP_OK) return rc;
    const DeviceClock clock = deviceClock(ctx->device, ctx->stream, false);
    uint64_t n = 0;
    for (auto & t : ctx->intervals) {
        if (t.clock != clock.id) continue;
        if (n < capacity) {
            if (start_ms) start_ms[n] = t.start_ms;
            if (stop_ms) stop_ms[n] = t.stop_ms;
            if (family) family[n] = t.family;
        }
        ++n;
    }
    *count_out = n;
    return RPVG_HIP_OK;
}

}  // extern "C"
