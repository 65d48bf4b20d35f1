// text_deflate.hip — a text resident on the GPU as the bytes of a .gz file: BGZF members, deflated here (interface include/rpvg_text.h,
// plan text_deflate_plan.hpp).  Only the compressed bytes leave the device; the writers copy them into the file.
//
// Takes over   the gzwrite of <prefix>_gibbs.txt.gz and <prefix>_probs.txt.gz, one host thread over every byte the device had
//              just formatted (src/threaded_output_writer.cpp:8-40, :98: mode "wg")
//
// Chunk        One workgroup of 1024 lanes per chunk of 65 280 bytes, the chunk in LDS (156 KB with its tables: one workgroup per CU).
//   CRC-32     a lane per slice of 64 bytes, zero bytes in front of a short chunk, joined by a tree whose operators are constants.
//   Matches    rounds of 1024 positions.  Every lane hashes the four bytes at its position, reads the table's entry for them (the
//              LAST position with that hash among the rounds before: the table takes a maximum, so the order of the lanes does not
//              reach it), compares in LDS against it and against distances 1 and 2, and keeps the longest match, the nearer on
//              a tie, if it is long enough for its distance (shortestMatchAt: four bytes at distances 1 and 2, six beyond).  Then
//              every lane enters its position (a maximum again).
//   Parse      greedy, by the first wavefront, 64 positions at a time: from the position the last token left off, literals up to
//              the next position with a match, that match, and on behind it.  All uniform work on two ballots.  A token start is a
//              bit in a mask, a match its length and distance in the three bytes of a shadow of the chunk that it covers anyway.
//   Codes      histograms by integer LDS atomics, code lengths, codes, header and the exact size on one lane (the plan's routines),
//              the size against the stored form.
//   Bits       every lane sums the bits of the tokens of its 64 positions, a prefix sum places them, and the lane ORs its codes
//              into the member's slot word by word (a slot is zero before the kernel; an OR commutes).  A stored member is copied.
//   Each member lies in a slot of 65 536 bytes; its size goes to an array.
// Pack         an exclusive sum over the sizes (hipcub) gives member_off; a gather kernel moves the members behind one another
//              into one block between two guards of 64 pattern bytes.
// Determinism  no result depends on which lane or wavefront reaches a table first: the match table keeps maxima, the histograms sums,
//              the slot ORs, and the parse is one wavefront's.  The same bytes give the same members.

#include <memory>
#include <mutex>
#include <vector>

#include "device_algos.hpp"
#include "table_kit.hpp"
#include "table_text_device.hpp"
#include "text_deflate_plan.hpp"
#include "../../include/rpvg_text.h"

using namespace rpvg_hip_detail;
using namespace rpvg_text_deflate;

struct rpvg_hip_text_bgzf {
    rpvg_hip_ctx * ctx = nullptr;
    uint64_t num_members = 0, num_text_bytes = 0, num_bytes = 0, num_stored_members = 0;
    DeviceBuffer<char> block;  // guard, members, guard
    std::vector<uint64_t> h_member_off;
    void * pinned = nullptr;   // the host copy of the members
    ~rpvg_hip_text_bgzf() {
        if (pinned) pinnedFree(pinned);
    }
    char * bytes() const { return block.ptr + kGuardBytes; }
};

namespace {

constexpr int kLanes = 1024;
static_assert(kRound == kLanes, "a lane per position of a round");
constexpr uint32_t kMaskWords = (kChunkBytes + 63) / 64;  // 1020
static_assert(kMaskWords <= kLanes, "a lane per 64 positions");
static_assert(kCrcSlices == kLanes, "a lane per slice");

// the workgroup's LDS (dynamic: above 64 KB)
struct ChunkLds {
    uint32_t chunk[kChunkBytes / 4 + 2];   // two words of zeros behind: a four-byte read may start at the last byte
    uint8_t shadow[kChunkBytes];           // at a match start: length - 3, then distance - 1 in two bytes
    unsigned long long start_mask[kLanes]; // bit: a token starts here
    unsigned long long match_mask[kLanes]; // bit: that token is a match
    union {
        struct {
            uint32_t table[1u << (kHashBits - 1)];  // two 16-bit entries per word: position + 1 of the last such hash, 0: none
            uint16_t round_len[kRound];
        } search;
        struct {  // behind the parse
            uint32_t weight[2 * kNumLitLen];
            uint16_t order[kNumLitLen], parent[2 * kNumLitLen], per_len[16];
            uint32_t cl_hist[kNumCodeLen];
            uint16_t cl_codes[kNumCodeLen];
            uint8_t cl_lens[kNumCodeLen];
        } code;
    } u;
    uint32_t lit_hist[kNumLitLen + 2], dist_hist[kNumDist + 2];
    uint16_t lit_codes[kNumLitLen + 2], dist_codes[kNumDist + 2];
    uint8_t lit_lens[kNumLitLen + 2], dist_lens[kNumDist + 2];
    uint32_t wave_value[kLanes / 64];
    uint32_t carry, crc, stored, header_bits, payload_bytes, hlit, hdist, hclen;
};
static_assert(sizeof(ChunkLds) == 159528 && sizeof(ChunkLds) <= 160 * 1024, "the chunk's LDS fits a CU, once");

// four bytes from byte position p, little-endian
__device__ __forceinline__ uint32_t load4(const uint32_t * words, const uint32_t p) {
    const uint32_t w = p >> 2, shift = (p & 3) * 8;
    const unsigned long long pair = static_cast<unsigned long long>(words[w + 1]) << 32 | words[w];
    return static_cast<uint32_t>(pair >> shift);
}

__device__ __forceinline__ uint32_t byteAt(const uint32_t * words, const uint32_t p) { return (words[p >> 2] >> ((p & 3) * 8)) & 0xff; }

// the bytes that agree from p and from c < p, at most `most`
__device__ __forceinline__ uint32_t matchLength(const uint32_t * words, const uint32_t p, const uint32_t c, const uint32_t most) {
    uint32_t l = 0;
    while (l < most) {
        const uint32_t x = load4(words, p + l) ^ load4(words, c + l);
        if (x) {
            l += static_cast<uint32_t>(__ffs(static_cast<int>(x)) - 1) >> 3;
            break;
        }
        l += 4;
    }
    return l < most ? l : most;
}

// the maximum of a 16-bit entry and `value`, entries in pairs per word
__device__ __forceinline__ void tableMax(uint32_t * table, const uint32_t h, const uint32_t value) {
    uint32_t * word = table + (h >> 1);
    const uint32_t shift = (h & 1) * 16;
    uint32_t old = *word;
    while (((old >> shift) & 0xffff) < value) {
        const uint32_t assumed = old;
        old = atomicCAS(word, assumed, (assumed & ~(0xffffu << shift)) | value << shift);
        if (old == assumed) break;
    }
}

// a lane's bits into the slot: whole words leave by one OR each
struct SlotSink {
    uint32_t * slot;
    uint32_t word;
    uint32_t bits;
    unsigned long long acc;
    __device__ __forceinline__ SlotSink(uint32_t * slot_in, const uint64_t bit) : slot(slot_in), word(static_cast<uint32_t>(bit >> 5)), bits(static_cast<uint32_t>(bit & 31)), acc(0) {}
    __device__ __forceinline__ void put(const uint32_t value, const uint32_t n) {  // n <= 28
        acc |= static_cast<unsigned long long>(value) << bits;
        bits += n;
        if (bits >= 32) {
            atomicOr(slot + word, static_cast<uint32_t>(acc));
            acc >>= 32;
            bits -= 32;
            word += 1;
        }
    }
    __device__ __forceinline__ void finish() {
        if (bits) atomicOr(slot + word, static_cast<uint32_t>(acc));
        bits = 0;
        acc = 0;
    }
};

__device__ __forceinline__ BlockCodes codesOf(ChunkLds & s) {
    BlockCodes codes = {s.lit_lens, s.lit_codes, s.dist_lens, s.dist_codes, s.u.code.cl_hist, s.u.code.cl_lens, s.u.code.cl_codes, s.hlit, s.hdist, s.hclen, s.header_bits};
    return codes;
}

// text: the chunks' bytes, 4-byte aligned, readable up to the next multiple of four.  slots: zero.
__global__ __launch_bounds__(kLanes) void deflateChunkKernel(const char * __restrict__ text, const uint64_t num_bytes, uint32_t * __restrict__ slots,
                                                             uint64_t * __restrict__ member_bytes, word64 * __restrict__ num_stored) {
    extern __shared__ __attribute__((aligned(16))) unsigned char deflate_lds[];
    ChunkLds & s = *reinterpret_cast<ChunkLds *>(deflate_lds);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t chunk = blockIdx.x;
    const uint32_t n = chunkBytes(chunk, num_bytes);
    const uint32_t * in = reinterpret_cast<const uint32_t *>(text + chunkBegin(chunk));
    uint32_t * slot = slots + chunk * (kMaxMemberBytes / 4);

    // ---- the chunk and empty tables
    for (uint32_t w = tid; w < kChunkBytes / 4 + 2; w += kLanes) {
        uint32_t v = 0;
        if (4 * w < n) {
            v = in[w];
            if (4 * w + 4 > n) v &= 0xffffffffu >> (8 * (4 * w + 4 - n));
        }
        s.chunk[w] = v;
    }
    s.start_mask[tid] = 0;
    s.match_mask[tid] = 0;
    for (uint32_t i = tid; i < (1u << (kHashBits - 1)); i += kLanes) s.u.search.table[i] = 0;
    if (tid < kNumLitLen + 2) s.lit_hist[tid] = 0;
    if (tid < kNumDist + 2) s.dist_hist[tid] = 0;
    if (tid == 0) s.carry = 0;
    __syncthreads();

    // ---- CRC-32: slice `tid` of the chunk with kCrcSlices * kCrcSliceBytes - n zero bytes in front
    {
        const uint32_t front = kCrcSlices * kCrcSliceBytes - n;
        uint32_t raw = 0;
        for (uint32_t i = 0; i < kCrcSliceBytes; ++i) {
            const uint32_t v = tid * kCrcSliceBytes + i;
            if (v >= front) raw = crcRawByte(raw, byteAt(s.chunk, v - front));  // (zero bytes in front leave a zero residue)
        }
        uint32_t pow = kCrcSlicePow;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t right = __shfl_down(raw, d, 64);
            raw = crcShift(raw, pow) ^ right;  // meaningful in the lanes that are multiples of 2 d
            pow = crcMul(pow, pow);
        }
        if (lane == 0) s.wave_value[wave] = raw;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (int w = 0; w < kLanes / 64; ++w) all = crcShift(all, pow) ^ s.wave_value[w];  // pow: 64 slices
            s.crc = crcFinish(all, n);
        }
    }

    // ---- matches and the greedy parse, a round of kRound positions at a time
    uint32_t carry = 0;  // the first position no token covers yet (the first wavefront's)
    const uint32_t rounds = (n + kRound - 1) / kRound;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t p = r * kRound + tid;
        uint32_t best = 0, best_dist = 0, h = 0;
        const bool hashed = p + kParseMinMatch <= n;
        if (hashed) {
            const uint32_t four = load4(s.chunk, p);
            h = hashOf(four);
            const uint32_t entry = (s.u.search.table[h >> 1] >> ((h & 1) * 16)) & 0xffff;
            if (p >= s.carry) {  // (a position the last round's tokens cover already starts no token)
                const uint32_t most = n - p < kMaxMatch ? n - p : kMaxMatch;
                for (uint32_t d = 1; d <= 2; ++d) {
                    if (p >= d && load4(s.chunk, p - d) == four) {
                        const uint32_t l = matchLength(s.chunk, p, p - d, most);
                        if (l > best) {
                            best = l;
                            best_dist = d;
                        }
                    }
                }
                if (entry && p - (entry - 1) <= kMaxDist && load4(s.chunk, entry - 1) == four) {
                    const uint32_t l = matchLength(s.chunk, p, entry - 1, most);
                    if (l > best) {
                        best = l;
                        best_dist = p - (entry - 1);
                    }
                }
                if (best < shortestMatchAt(best_dist)) best = 0;
            }
        }
        s.u.search.round_len[tid] = static_cast<uint16_t>(best);
        __syncthreads();
        if (hashed) tableMax(s.u.search.table, h, p + 1);
        if (wave == 0) {
            for (uint32_t sub = 0; sub < kRound / 64; ++sub) {
                const uint32_t base = r * kRound + sub * 64;
                if (base >= n) break;
                const uint32_t len = s.u.search.round_len[sub * 64 + lane];
                const unsigned long long with_match = __ballot(len != 0);
                unsigned long long starts = 0, matches = 0;
                uint32_t cur = carry > base ? carry - base : 0;
                while (cur < 64) {
                    const unsigned long long ahead = with_match >> cur;
                    if (ahead == 0) {  // literals to the end
                        starts |= ~0ull << cur;
                        cur = 64;
                        break;
                    }
                    const uint32_t at = cur + static_cast<uint32_t>(__ffsll(static_cast<long long>(ahead)) - 1);
                    starts |= (~0ull << cur) & (~0ull >> (63 - at));  // literals cur .. at - 1 and the match at `at`
                    matches |= 1ull << at;
                    cur = at + __shfl(len, static_cast<int>(at), 64);
                }
                if (base + cur > carry) carry = base + cur;
                if (n - base < 64) starts &= ~0ull >> (64 - (n - base));
                if (lane == 0) {
                    s.start_mask[base >> 6] = starts;
                    s.match_mask[base >> 6] = matches;
                }
            }
            if (lane == 0) s.carry = carry;
        }
        __syncthreads();
        if (best && ((s.match_mask[p >> 6] >> (p & 63)) & 1)) {
            s.shadow[p] = static_cast<uint8_t>(best - 3);
            s.shadow[p + 1] = static_cast<uint8_t>((best_dist - 1) & 0xff);
            s.shadow[p + 2] = static_cast<uint8_t>((best_dist - 1) >> 8);
        }
    }
    __syncthreads();

    // ---- histograms: the tokens of positions 64 tid .. 64 tid + 63
    const unsigned long long my_starts = s.start_mask[tid], my_matches = s.match_mask[tid];
    for (unsigned long long left = my_starts; left; left &= left - 1) {
        const uint32_t b = static_cast<uint32_t>(__ffsll(static_cast<long long>(left)) - 1), p = tid * 64 + b;
        if ((my_matches >> b) & 1) {
            atomicAdd(&s.lit_hist[lengthCode(s.shadow[p] + 3u)], 1u);
            atomicAdd(&s.dist_hist[distCode((s.shadow[p + 1] | static_cast<uint32_t>(s.shadow[p + 2]) << 8) + 1u)], 1u);
        } else {
            atomicAdd(&s.lit_hist[byteAt(s.chunk, p)], 1u);
        }
    }
    if (tid == 0) atomicAdd(&s.lit_hist[kEndOfBlock], 1u);
    __syncthreads();

    // ---- codes, header and size on one lane
    if (tid == 0) {
        BlockCodes codes = codesOf(s);
        planBlock(s.lit_hist, s.dist_hist, codes, LengthWork{s.u.code.order, s.u.code.weight, s.u.code.parent, s.u.code.per_len});
        const uint32_t dynamic_bytes = static_cast<uint32_t>((blockBits(s.lit_hist, s.dist_hist, codes) + 7) / 8);
        s.stored = storedBytes(n) <= dynamic_bytes ? 1 : 0;
        s.payload_bytes = s.stored ? storedBytes(n) : dynamic_bytes;
        s.hlit = codes.hlit;
        s.hdist = codes.hdist;
        s.hclen = codes.hclen;
        s.header_bits = codes.header_bits;
    }
    __syncthreads();
    const uint32_t payload_bytes = s.payload_bytes, total_bytes = kHeaderBytes + payload_bytes + kTrailerBytes;
    const bool stored = s.stored != 0;

    // ---- the member's frame
    if (tid < kHeaderBytes) reinterpret_cast<unsigned char *>(slot)[tid] = static_cast<unsigned char>(memberHeaderByte(tid, total_bytes));
    else if (tid < kHeaderBytes + kTrailerBytes) reinterpret_cast<unsigned char *>(slot)[payload_bytes + tid] = static_cast<unsigned char>(memberTrailerByte(tid - kHeaderBytes, s.crc, n));
    if (tid == 0) {
        member_bytes[chunk] = total_bytes;
        if (stored) atomicAdd(num_stored, 1ull);
    }

    if (stored) {
        unsigned char * out = reinterpret_cast<unsigned char *>(slot) + kHeaderBytes;
        if (tid < kStoredHeadBytes) out[tid] = static_cast<unsigned char>(storedHeadByte(tid, n));
        for (uint32_t i = tid; i < n; i += kLanes) out[kStoredHeadBytes + i] = static_cast<unsigned char>(byteAt(s.chunk, i));
        return;
    }

    // The frame's bytes and the stream's bits share the words at both ends of the stream: the plain stores above must have reached
    // memory before another lane's OR into such a word.
    __threadfence();
    __syncthreads();

    // ---- the bits of every lane's tokens, placed by a prefix sum
    const BlockCodes codes = codesOf(s);
    uint32_t my_bits = 0;
    for (unsigned long long left = my_starts; left; left &= left - 1) {
        const uint32_t b = static_cast<uint32_t>(__ffsll(static_cast<long long>(left)) - 1), p = tid * 64 + b;
        if ((my_matches >> b) & 1) my_bits += matchBits(codes, s.shadow[p] + 3u, (s.shadow[p + 1] | static_cast<uint32_t>(s.shadow[p + 2]) << 8) + 1u);
        else my_bits += s.lit_lens[byteAt(s.chunk, p)];
    }
    uint32_t before = my_bits;  // inclusive within the wavefront
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(before, d, 64);
        if (lane >= static_cast<uint32_t>(d)) before += up;
    }
    if (lane == 63) s.wave_value[wave] = before;
    __syncthreads();
    uint32_t waves_before = 0, all_bits = 0;
    for (uint32_t w = 0; w < kLanes / 64; ++w) {
        if (w < wave) waves_before += s.wave_value[w];
        all_bits += s.wave_value[w];
    }
    const uint64_t first_bit = 8ull * kHeaderBytes + s.header_bits;
    SlotSink sink(slot, first_bit + waves_before + before - my_bits);
    for (unsigned long long left = my_starts; left; left &= left - 1) {
        const uint32_t b = static_cast<uint32_t>(__ffsll(static_cast<long long>(left)) - 1), p = tid * 64 + b;
        if ((my_matches >> b) & 1) putMatch(sink, codes, s.shadow[p] + 3u, (s.shadow[p + 1] | static_cast<uint32_t>(s.shadow[p + 2]) << 8) + 1u);
        else putLiteral(sink, codes, byteAt(s.chunk, p));
    }
    sink.finish();
    if (tid == kLanes - 1) {  // the header, and the end of block behind the last token
        SlotSink head(slot, 8ull * kHeaderBytes);
        putHeader(head, codes);
        head.finish();
        SlotSink tail(slot, first_bit + all_bits);
        putLiteral(tail, codes, kEndOfBlock);
        tail.finish();
    }
}

// member i from its slot to bytes [member_off[i], member_off[i + 1]) of the packed block
__global__ __launch_bounds__(256) void packMembersKernel(const uint32_t * __restrict__ slots, const uint64_t * __restrict__ member_off, char * __restrict__ out) {
    const uint64_t i = blockIdx.x;
    const unsigned char * from = reinterpret_cast<const unsigned char *>(slots + i * (kMaxMemberBytes / 4));
    const uint64_t begin = member_off[i];
    const uint32_t size = static_cast<uint32_t>(member_off[i + 1] - begin);
    char * to = out + begin;
    // whole words of the destination, the source read as two words and shifted; the ragged ends byte by byte
    const uint32_t head = static_cast<uint32_t>((4 - (reinterpret_cast<uintptr_t>(to) & 3)) & 3);
    const uint32_t lead = head < size ? head : size;
    if (threadIdx.x < lead) to[threadIdx.x] = static_cast<char>(from[threadIdx.x]);
    const uint32_t words = (size - lead) / 4;
    uint32_t * to_words = reinterpret_cast<uint32_t *>(to + lead);
    for (uint32_t w = threadIdx.x; w < words; w += 256) to_words[w] = load4(reinterpret_cast<const uint32_t *>(from), lead + 4 * w);
    const uint32_t done = lead + 4 * words;
    if (threadIdx.x < size - done) to[done + threadIdx.x] = static_cast<char>(from[done + threadIdx.x]);
}

int optInOnce(rpvg_hip_ctx * ctx) {
    static std::once_flag once[64];
    static hipError_t result[64];
    const int device = ctx->device >= 0 && ctx->device < 64 ? ctx->device : 0;
    std::call_once(once[device], [&] {
        result[device] = hipFuncSetAttribute(reinterpret_cast<const void *>(&deflateChunkKernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(sizeof(ChunkLds)));
    });
    RPVG_HIP_CHECK(result[device]);
    return RPVG_HIP_OK;
}

// text: device memory, 4-byte aligned and readable up to the next multiple of four bytes behind num_bytes.  The context's mutex is held.
int buildBgzf(rpvg_hip_ctx * ctx, const char * text, const uint64_t num_bytes, const char * who, rpvg_hip_text_bgzf ** out) {
    std::unique_ptr<rpvg_hip_text_bgzf> bgzf(new (std::nothrow) rpvg_hip_text_bgzf());
    if (!bgzf) {
        setError("%s: out of host memory", who);
        return RPVG_HIP_ERR_ALLOC;
    }
    bgzf->ctx = ctx;
    bgzf->num_text_bytes = num_bytes;
    const uint64_t M = numChunks(num_bytes);
    bgzf->num_members = M;
    bgzf->h_member_off.assign(M + 1, 0);
    if (M == 0) {
        *out = bgzf.release();
        return RPVG_HIP_OK;
    }
    RPVG_REQUIRE(M < (1ull << 31), "%s: a text of %llu bytes has more chunks than a launch takes", who, static_cast<unsigned long long>(num_bytes));
    hipStream_t st = ctx->stream;
    if (const int rc = optInOnce(ctx)) return rc;
    SpanScope span(ctx, FAM_BUILD);
    DeviceBuffer<uint32_t> slots;
    DeviceBuffer<uint64_t> sizes, member_off;
    DeviceBuffer<word64> d_stored;
    if (slots.alloc(M * (kMaxMemberBytes / 4)) != hipSuccess || sizes.alloc(M + 1) != hipSuccess || member_off.alloc(M + 1) != hipSuccess || d_stored.alloc(1) != hipSuccess) {
        (void) hipGetLastError();
        span.end();
        setError("%s: no device memory for the %llu slots of a text of %llu bytes", who, static_cast<unsigned long long>(M), static_cast<unsigned long long>(num_bytes));
        return RPVG_HIP_ERR_ALLOC;
    }
    RPVG_HIP_CHECK(zeroAsync(slots.ptr, M * kMaxMemberBytes, st));
    RPVG_HIP_CHECK(zeroAsync(sizes.ptr, (M + 1) * sizeof(uint64_t), st));
    RPVG_HIP_CHECK(zeroAsync(d_stored.ptr, sizeof(word64), st));
    deflateChunkKernel<<<dim3(static_cast<uint32_t>(M)), dim3(kLanes), sizeof(ChunkLds), st>>>(text, num_bytes, slots.ptr, sizes.ptr, d_stored.ptr);
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 1;
    if (const int rc = exclusiveSum(st, sizes.ptr, member_off.ptr, M + 1)) return rc;
    word64 stored = 0;
    RPVG_HIP_CHECK(hipMemcpyAsync(bgzf->h_member_off.data(), member_off.ptr, (M + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipMemcpyAsync(&stored, d_stored.ptr, sizeof(stored), hipMemcpyDeviceToHost, st));
    RPVG_HIP_CHECK(hipStreamSynchronize(st));
    bgzf->num_bytes = bgzf->h_member_off[M];
    bgzf->num_stored_members = stored;
    const size_t block_bytes = (static_cast<size_t>(bgzf->num_bytes) + 2 * kGuardBytes + 3) & ~size_t(3);
    if (bgzf->block.alloc(block_bytes) != hipSuccess) {
        (void) hipGetLastError();
        (void) hipDeviceSynchronize();
        span.end();
        setError("%s: no device memory for %llu compressed bytes", who, static_cast<unsigned long long>(bgzf->num_bytes));
        return RPVG_HIP_ERR_ALLOC;
    }
    guardKernel<<<dim3(1), dim3(128), 0, st>>>(bgzf->block.ptr, bgzf->num_bytes);
    packMembersKernel<<<dim3(static_cast<uint32_t>(M)), dim3(256), 0, st>>>(slots.ptr, member_off.ptr, bgzf->bytes());
    RPVG_HIP_CHECK(hipGetLastError());
    ctx->stats.build_launches += 2;
    RPVG_HIP_CHECK(hipStreamSynchronize(st));  // the slots go back to the pool
    span.end();
    *out = bgzf.release();
    return RPVG_HIP_OK;
}

}  // namespace

extern "C" {

int rpvg_hip_table_text_bgzf(rpvg_hip_table_text * text, rpvg_hip_text_bgzf ** out) {
    const char * const who = "rpvg_hip_table_text_bgzf";
    RPVG_REQUIRE(text && out, "%s: NULL argument", who);
    *out = nullptr;
    rpvg_hip_ctx * ctx = text->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    return buildBgzf(ctx, text->num_bytes ? text->text() : nullptr, text->num_bytes, who, out);  // (the text's block ends in a guard: readable past its last byte)
}

int rpvg_hip_bytes_bgzf(rpvg_hip_ctx * ctx, const char * bytes, uint64_t n, int32_t on_device, rpvg_hip_text_bgzf ** out) {
    const char * const who = "rpvg_hip_bytes_bgzf";
    RPVG_REQUIRE(ctx && out, "%s: NULL argument", who);
    *out = nullptr;
    RPVG_REQUIRE(n == 0 || bytes, "%s: NULL argument (%llu bytes)", who, static_cast<unsigned long long>(n));
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    DeviceBuffer<char> copy;  // a block of the library's own: aligned, and readable to the next multiple of four
    if (n) {
        if (copy.alloc((static_cast<size_t>(n) + 3) & ~size_t(3)) != hipSuccess) {
            (void) hipGetLastError();
            setError("%s: no device memory for %llu bytes", who, static_cast<unsigned long long>(n));
            return RPVG_HIP_ERR_ALLOC;
        }
        RPVG_HIP_CHECK(hipMemcpyAsync(copy.ptr, bytes, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    }
    const int rc = buildBgzf(ctx, copy.ptr, n, who, out);
    (void) hipStreamSynchronize(ctx->stream);  // the copy goes back to the pool
    return rc;
}

int rpvg_hip_text_bgzf_view(rpvg_hip_text_bgzf * bgzf, rpvg_text_bgzf_view * view_out) {
    RPVG_REQUIRE(bgzf && view_out, "rpvg_hip_text_bgzf_view: NULL argument");
    rpvg_hip_ctx * ctx = bgzf->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    if (!bgzf->pinned && bgzf->num_bytes) {
        RPVG_HIP_CHECK(hipSetDevice(ctx->device));
        if (pinnedAlloc(&bgzf->pinned, bgzf->num_bytes) != hipSuccess) {
            bgzf->pinned = nullptr;
            (void) hipGetLastError();
            setError("rpvg_hip_text_bgzf_view: no page-locked memory for %llu bytes (rpvg_hip_text_bgzf_get takes a range)", static_cast<unsigned long long>(bgzf->num_bytes));
            return RPVG_HIP_ERR_ALLOC;
        }
        RPVG_HIP_CHECK(hipMemcpyAsync(bgzf->pinned, bgzf->bytes(), bgzf->num_bytes, hipMemcpyDeviceToHost, ctx->stream));
        RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    view_out->num_members = bgzf->num_members;
    view_out->num_text_bytes = bgzf->num_text_bytes;
    view_out->num_bytes = bgzf->num_bytes;
    view_out->num_stored_members = bgzf->num_stored_members;
    view_out->member_off = bgzf->h_member_off.data();
    view_out->bytes = static_cast<const char *>(bgzf->pinned);
    return RPVG_HIP_OK;
}

int rpvg_hip_text_bgzf_get(rpvg_hip_text_bgzf * bgzf, uint64_t byte_begin, uint64_t byte_end, char * dst) {
    RPVG_REQUIRE(bgzf, "rpvg_hip_text_bgzf_get: NULL argument");
    RPVG_REQUIRE(byte_begin <= byte_end && byte_end <= bgzf->num_bytes, "rpvg_hip_text_bgzf_get: bytes %llu to %llu of %llu", static_cast<unsigned long long>(byte_begin),
                 static_cast<unsigned long long>(byte_end), static_cast<unsigned long long>(bgzf->num_bytes));
    if (byte_begin == byte_end) return RPVG_HIP_OK;
    RPVG_REQUIRE(dst, "rpvg_hip_text_bgzf_get: NULL argument");
    rpvg_hip_ctx * ctx = bgzf->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    RPVG_HIP_CHECK(hipMemcpyAsync(dst, bgzf->bytes() + byte_begin, byte_end - byte_begin, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPVG_HIP_OK;
}

int rpvg_hip_text_bgzf_guards(rpvg_hip_text_bgzf * bgzf, int32_t * intact_out) {
    RPVG_REQUIRE(bgzf && intact_out, "rpvg_hip_text_bgzf_guards: NULL argument");
    *intact_out = 1;
    if (!bgzf->block.ptr) return RPVG_HIP_OK;  // an empty text has no block
    rpvg_hip_ctx * ctx = bgzf->ctx;
    std::lock_guard<std::mutex> lock(ctx->mutex);
    RPVG_HIP_CHECK(hipSetDevice(ctx->device));
    unsigned char guards[2 * kGuardBytes];
    RPVG_HIP_CHECK(hipMemcpyAsync(guards, bgzf->block.ptr, kGuardBytes, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipMemcpyAsync(guards + kGuardBytes, bgzf->block.ptr + kGuardBytes + bgzf->num_bytes, kGuardBytes, hipMemcpyDeviceToHost, ctx->stream));
    RPVG_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (const unsigned char byte : guards) {
        if (byte != kGuardPattern) *intact_out = 0;
    }
    return RPVG_HIP_OK;
}

void rpvg_hip_text_bgzf_free(rpvg_hip_text_bgzf * bgzf) {
    if (!bgzf) return;
    waitAndDelete(bgzf->ctx);
    delete bgzf;
}

}  // extern "C"
