// text_deflate_plan.hpp — what the host and the device share about a text as BGZF (text_deflate.hip, include/rpvg_text.h): the cut
// of a text into chunks, the bytes around a member, the stored form, RFC 1951's length and distance codes, code lengths from a
// histogram under a bit limit, canonical codes, the dynamic block's header, its exact bit size, CRC-32 with the operators that join
// slices, and the host's framing of its own rows.  Plain C++17 under the RPVG_PLAN_FN convention of the other *_plan.hpp files: a
// CPU program reaches every function (tests/cpp/text_deflate_plan_check.cpp).  No function holds an array of its own: the caller
// hands the work space in, so the device's copy lives in LDS.
//
// Format       BGZF, htslib's blocked gzip: a sequence of gzip members of at most 65 536 bytes, each one raw DEFLATE stream over at
//              most kChunkBytes bytes of the text, with its own size in an extra field.  Any gzip reader reads the members one after
//              the other.
// Member       18 header bytes (memberHeaderByte), one DEFLATE block with BFINAL set, CRC-32 and ISIZE of the chunk.
// Block        BTYPE 10 over literals and matches (length 3 .. 258, distance 1 .. 32 768 inside the chunk), or BTYPE 00 when the
//              stored form (5 + n bytes) is not larger: a member is at most n + 31 bytes.
#ifndef RPVG_HIP_TEXT_DEFLATE_PLAN_HPP
#define RPVG_HIP_TEXT_DEFLATE_PLAN_HPP

#include <cstdint>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string>
#endif

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

namespace rpvg_text_deflate {

constexpr uint32_t kChunkBytes = 65280;      // htslib's 0xff00: a stored chunk still fits a member
constexpr uint32_t kMaxMemberBytes = 65536;  // BSIZE is 16 bits
constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8, kStoredHeadBytes = 5;
constexpr uint32_t kMemberOverhead = kHeaderBytes + kStoredHeadBytes + kTrailerBytes;  // 31
constexpr uint32_t kEofBytes = 28;

constexpr int kNumLitLen = 286, kNumDist = 30, kNumCodeLen = 19, kEndOfBlock = 256;
constexpr int kMaxBits = 15, kMaxCodeLenBits = 7;
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768;

// the parse of text_deflate.hip: rounds of kRound positions, a table of the last position per hash of four bytes
constexpr uint32_t kRound = 1024, kParseMinMatch = 4, kHashBits = 12;
RPVG_PLAN_FN uint32_t hashOf(const uint32_t four) { return (four * 2654435761u) >> (32 - kHashBits); }
// The shortest match the parse takes at a distance.  A match pays a length code, a distance code and up to 13 extra bits of distance
// where a literal of this kind of text pays about four bits: in uniformly random digits four bytes agree somewhere in nearly every
// round, and taking those matches brought a chunk to 0.493 of its size where its literals alone take 0.454.  Six bytes beyond the
// two distances of a run or an alternation measured best of 4 .. 12 on digits, on %.8g cells with names and on rows of integer counts
// (0.454, 0.456, 0.369 of the text against 0.518, 0.508, 0.372 for zlib at level 1 over the same chunks).
constexpr uint32_t kNearDist = 2, kFarMinMatch = 6;
RPVG_PLAN_FN uint32_t shortestMatchAt(const uint32_t dist) { return dist <= kNearDist ? kParseMinMatch : kFarMinMatch; }

// ---- chunks ---------------------------------------------------------------------------------------------------------------------

RPVG_PLAN_FN uint64_t numChunks(const uint64_t num_bytes) { return (num_bytes + kChunkBytes - 1) / kChunkBytes; }
RPVG_PLAN_FN uint64_t chunkBegin(const uint64_t chunk) { return chunk * kChunkBytes; }
RPVG_PLAN_FN uint32_t chunkBytes(const uint64_t chunk, const uint64_t num_bytes) {
    const uint64_t left = num_bytes - chunkBegin(chunk);
    return static_cast<uint32_t>(left < kChunkBytes ? left : kChunkBytes);
}

// ---- the bytes around the DEFLATE stream ----------------------------------------------------------------------------------------

// byte i (0 .. 17) of the header of a member of member_bytes bytes in all
RPVG_PLAN_FN uint32_t memberHeaderByte(const uint32_t i, const uint32_t member_bytes) {
    const uint32_t bsize = member_bytes - 1;
    switch (i) {
        case 0: return 0x1f;
        case 1: return 0x8b;
        case 2: return 8;      // CM: deflate
        case 3: return 4;      // FLG: FEXTRA
        case 9: return 0xff;   // OS: unknown
        case 10: return 6;     // XLEN
        case 12: return 'B';
        case 13: return 'C';
        case 14: return 2;     // SLEN
        case 16: return bsize & 0xff;
        case 17: return bsize >> 8;
        default: return 0;     // MTIME, XFL, the high bytes of XLEN and SLEN
    }
}

// byte i (0 .. 7) of the trailer: CRC-32 and ISIZE, little-endian
RPVG_PLAN_FN uint32_t memberTrailerByte(const uint32_t i, const uint32_t crc, const uint32_t isize) {
    return ((i < 4 ? crc : isize) >> (8 * (i & 3))) & 0xff;
}

// byte i (0 .. 4) in front of the n bytes of a stored block with BFINAL set
RPVG_PLAN_FN uint32_t storedHeadByte(const uint32_t i, const uint32_t n) {
    switch (i) {
        case 0: return 1;  // BFINAL 1, BTYPE 00, padding
        case 1: return n & 0xff;
        case 2: return n >> 8;
        case 3: return ~n & 0xff;
        default: return (~n >> 8) & 0xff;
    }
}

RPVG_PLAN_FN uint32_t storedBytes(const uint32_t n) { return kStoredHeadBytes + n; }

// ---- RFC 1951, 3.2.5: length and distance codes ------------------------------------------------------------------------------------

// length 3 .. 258 -> code 257 .. 285
RPVG_PLAN_FN uint32_t lengthCode(const uint32_t length) {
    const uint32_t l = length - 3;
    if (l < 8) return 257 + l;
    if (l == 255) return 285;
    const uint32_t e = (31 - __builtin_clz(l)) - 2;
    return 261 + 4 * e + ((l >> e) & 3);
}
RPVG_PLAN_FN uint32_t lengthExtraBits(const uint32_t code) { return code < 265 || code == 285 ? 0 : (code - 261) >> 2; }
RPVG_PLAN_FN uint32_t lengthBase(const uint32_t code) {
    if (code < 265) return code - 254;
    if (code == 285) return 258;
    const uint32_t e = lengthExtraBits(code);
    return 3 + ((4 + ((code - 261) & 3)) << e);
}
RPVG_PLAN_FN uint32_t lengthExtraValue(const uint32_t length, const uint32_t code) { return length - lengthBase(code); }

// distance 1 .. 32 768 -> code 0 .. 29
RPVG_PLAN_FN uint32_t distCode(const uint32_t dist) {
    const uint32_t d = dist - 1;
    if (d < 4) return d;
    const uint32_t hb = 31 - __builtin_clz(d);
    return 2 * hb + ((d >> (hb - 1)) & 1);
}
RPVG_PLAN_FN uint32_t distExtraBits(const uint32_t code) { return code < 4 ? 0 : (code >> 1) - 1; }
RPVG_PLAN_FN uint32_t distBase(const uint32_t code) {
    if (code < 4) return code + 1;
    return 1 + ((2 + (code & 1)) << distExtraBits(code));
}
RPVG_PLAN_FN uint32_t distExtraValue(const uint32_t dist, const uint32_t code) { return dist - distBase(code); }

// the order in which the lengths of the code-length code are sent (3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
RPVG_PLAN_FN uint32_t codeLenOrder(const uint32_t i) {
    // five bits per entry, twelve entries in the first word
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return static_cast<uint32_t>((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// ---- code lengths from a histogram ------------------------------------------------------------------------------------------------

// the caller's work space for an alphabet of at most n symbols
struct LengthWork {
    uint16_t * order;    // [n] the used symbols by (count, symbol)
    uint32_t * weight;   // [2 n] the tree's weights, then its depths
    uint16_t * parent;   // [2 n]
    uint16_t * per_len;  // [16] codes per length
};

// Code lengths of at most `limit` bits (limit <= 15) for the symbols with a count: Huffman's tree from the sorted counts by two
// queues, depths above the limit cut to it, and the Kraft sum brought back to one by lengthening, one at a time, a code of the
// longest length below the limit; the lengths then go to the symbols by count, the longest to the rarest.  With two or more used
// symbols the code is complete (Kraft sum exactly one); one used symbol gets length 1; none: all lengths 0.  Returns the number of
// used symbols.  What the cut costs against the unlimited tree is measured in tests/cpp/text_deflate_plan_check.cpp.
RPVG_PLAN_FN uint32_t codeLengths(const uint32_t * hist, const uint32_t n, const uint32_t limit, uint8_t * lens, const LengthWork & work) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        lens[s] = 0;
        if (hist[s] == 0) continue;
        uint32_t at = m++;  // insertion by (count, symbol): symbols arrive in order, so equal counts stay in symbol order
        while (at > 0 && hist[work.order[at - 1]] > hist[s]) {
            work.order[at] = work.order[at - 1];
            --at;
        }
        work.order[at] = static_cast<uint16_t>(s);
    }
    if (m == 0) return 0;
    if (m == 1) {
        lens[work.order[0]] = 1;
        return 1;
    }
    for (uint32_t i = 0; i < m; ++i) work.weight[i] = hist[work.order[i]];
    uint32_t leaf = 0, inner = m, next = m;
    while (next < 2 * m - 1) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool take_leaf = leaf < m && (inner >= next || work.weight[leaf] <= work.weight[inner]);
            const uint32_t node = take_leaf ? leaf++ : inner++;
            sum += work.weight[node];
            work.parent[node] = static_cast<uint16_t>(next);
        }
        work.weight[next++] = sum;
    }
    for (uint32_t l = 0; l <= limit; ++l) work.per_len[l] = 0;
    work.weight[2 * m - 2] = 0;  // depths from the root down: a parent was made after its children
    for (uint32_t node = 2 * m - 2; node-- > 0;) {
        const uint32_t depth = work.weight[work.parent[node]] + 1;
        work.weight[node] = depth;
        if (node < m) work.per_len[depth < limit ? depth : limit] += 1;
    }
    uint32_t total = 0;  // the Kraft sum in units of 2^-limit
    for (uint32_t l = 1; l <= limit; ++l) total += static_cast<uint32_t>(work.per_len[l]) << (limit - l);
    while (total > (1u << limit)) {
        work.per_len[limit] -= 1;
        for (uint32_t l = limit - 1; l > 0; --l) {
            if (work.per_len[l]) {
                work.per_len[l] -= 1;
                work.per_len[l + 1] += 2;
                break;
            }
        }
        total -= 1;
    }
    uint32_t at = 0;
    for (uint32_t l = limit; l > 0; --l) {
        for (uint32_t c = work.per_len[l]; c > 0; --c) lens[work.order[at++]] = static_cast<uint8_t>(l);
    }
    return m;
}

// Canonical codes (3.2.2) from lengths, each with its bits reversed: DEFLATE packs a Huffman code from its most significant bit
// into a stream that fills bytes from the least significant one.  next_code: [16] work space.
RPVG_PLAN_FN void canonicalCodes(const uint8_t * lens, const uint32_t n, uint16_t * codes, uint16_t * next_code) {
    for (uint32_t l = 0; l < 16; ++l) next_code[l] = 0;
    for (uint32_t s = 0; s < n; ++s) next_code[lens[s]] += 1;
    uint32_t code = 0, count = 0;
    next_code[0] = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code = (code + count) << 1;
        count = next_code[l];
        next_code[l] = static_cast<uint16_t>(code);
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s];
        uint32_t reversed = 0;
        if (l) {
            uint32_t c = next_code[l]++;
            for (uint32_t b = 0; b < l; ++b) {
                reversed = reversed << 1 | (c & 1);
                c >>= 1;
            }
        }
        codes[s] = static_cast<uint16_t>(reversed);
    }
}

// ---- the dynamic block ----------------------------------------------------------------------------------------------------------------

// everything a dynamic block's header needs, in the caller's memory
struct BlockCodes {
    uint8_t * lit_lens;     // [286]
    uint16_t * lit_codes;   // [286]
    uint8_t * dist_lens;    // [30]
    uint16_t * dist_codes;  // [30]
    uint32_t * cl_hist;     // [19]
    uint8_t * cl_lens;      // [19]
    uint16_t * cl_codes;    // [19]
    uint32_t hlit, hdist, hclen;
    uint32_t header_bits;   // BFINAL and BTYPE included
};

// Codes for the two histograms (lit_hist[256] must count the end of block) and the header that sends them with the plain
// code-length symbols 0 .. 15.  The decoder's traps: the literal/length code is complete (at least a literal or a match and the end
// of block are used); a distance alphabet with one used code gets length 1, and one without any sends code 0 with length 1.
RPVG_PLAN_FN void planBlock(const uint32_t * lit_hist, const uint32_t * dist_hist, BlockCodes & codes, const LengthWork & work) {
    codeLengths(lit_hist, kNumLitLen, kMaxBits, codes.lit_lens, work);
    if (codeLengths(dist_hist, kNumDist, kMaxBits, codes.dist_lens, work) == 0) codes.dist_lens[0] = 1;
    canonicalCodes(codes.lit_lens, kNumLitLen, codes.lit_codes, work.per_len);
    canonicalCodes(codes.dist_lens, kNumDist, codes.dist_codes, work.per_len);
    codes.hlit = kNumLitLen;
    while (codes.hlit > 257 && codes.lit_lens[codes.hlit - 1] == 0) codes.hlit -= 1;
    codes.hdist = kNumDist;
    while (codes.hdist > 1 && codes.dist_lens[codes.hdist - 1] == 0) codes.hdist -= 1;
    for (uint32_t s = 0; s < static_cast<uint32_t>(kNumCodeLen); ++s) codes.cl_hist[s] = 0;
    for (uint32_t s = 0; s < codes.hlit; ++s) codes.cl_hist[codes.lit_lens[s]] += 1;
    for (uint32_t s = 0; s < codes.hdist; ++s) codes.cl_hist[codes.dist_lens[s]] += 1;
    // (at least 258 lengths that cannot all be equal: a complete code over 257 .. 286 symbols has two lengths or unused symbols)
    codeLengths(codes.cl_hist, kNumCodeLen, kMaxCodeLenBits, codes.cl_lens, work);
    canonicalCodes(codes.cl_lens, kNumCodeLen, codes.cl_codes, work.per_len);
    codes.hclen = kNumCodeLen;
    while (codes.hclen > 4 && codes.cl_lens[codeLenOrder(codes.hclen - 1)] == 0) codes.hclen -= 1;
    codes.header_bits = 3 + 5 + 5 + 4 + 3 * codes.hclen;
    for (uint32_t s = 0; s < 16; ++s) codes.header_bits += codes.cl_hist[s] * codes.cl_lens[s];
}

// the exact size of the block in bits: header, every counted symbol with its extra bits (the end of block is in lit_hist)
RPVG_PLAN_FN uint64_t blockBits(const uint32_t * lit_hist, const uint32_t * dist_hist, const BlockCodes & codes) {
    uint64_t bits = codes.header_bits;
    for (uint32_t s = 0; s < static_cast<uint32_t>(kNumLitLen); ++s) bits += static_cast<uint64_t>(lit_hist[s]) * (codes.lit_lens[s] + (s > 256 ? lengthExtraBits(s) : 0));
    for (uint32_t s = 0; s < static_cast<uint32_t>(kNumDist); ++s) bits += static_cast<uint64_t>(dist_hist[s]) * (codes.dist_lens[s] + distExtraBits(s));
    return bits;
}

// the header into a sink with put(value, bits), bits from the least significant one
template <typename Sink>
RPVG_PLAN_FN void putHeader(Sink & sink, const BlockCodes & codes) {
    sink.put(1 | 2 << 1, 3);  // BFINAL, BTYPE 10
    sink.put(codes.hlit - 257, 5);
    sink.put(codes.hdist - 1, 5);
    sink.put(codes.hclen - 4, 4);
    for (uint32_t i = 0; i < codes.hclen; ++i) sink.put(codes.cl_lens[codeLenOrder(i)], 3);
    for (uint32_t s = 0; s < codes.hlit; ++s) sink.put(codes.cl_codes[codes.lit_lens[s]], codes.cl_lens[codes.lit_lens[s]]);
    for (uint32_t s = 0; s < codes.hdist; ++s) sink.put(codes.cl_codes[codes.dist_lens[s]], codes.cl_lens[codes.dist_lens[s]]);
}

template <typename Sink>
RPVG_PLAN_FN void putLiteral(Sink & sink, const BlockCodes & codes, const uint32_t symbol) {
    sink.put(codes.lit_codes[symbol], codes.lit_lens[symbol]);
}

template <typename Sink>
RPVG_PLAN_FN void putMatch(Sink & sink, const BlockCodes & codes, const uint32_t length, const uint32_t dist) {
    const uint32_t lc = lengthCode(length), dc = distCode(dist);
    sink.put(codes.lit_codes[lc] | lengthExtraValue(length, lc) << codes.lit_lens[lc], codes.lit_lens[lc] + lengthExtraBits(lc));
    sink.put(codes.dist_codes[dc] | distExtraValue(dist, dc) << codes.dist_lens[dc], codes.dist_lens[dc] + distExtraBits(dc));
}

RPVG_PLAN_FN uint32_t matchBits(const BlockCodes & codes, const uint32_t length, const uint32_t dist) {
    const uint32_t lc = lengthCode(length), dc = distCode(dist);
    return codes.lit_lens[lc] + lengthExtraBits(lc) + codes.dist_lens[dc] + distExtraBits(dc);
}

// ---- CRC-32 (the gzip polynomial, reflected) ------------------------------------------------------------------------------------------
// crcRaw is the remainder alone, without the preset and the final inversion: it is linear, zero bytes in front do not change it, and
//     crcRaw(A B) = crcShift(crcRaw(A), bytes of B) ^ crcRaw(B),        crc32(M) = crcFinish(crcRaw(M), bytes of M).
// A product of two residues (crcMul) is zlib's multmodp; x^0 is 0x80000000 in this bit order.

constexpr uint32_t kCrcPoly = 0xedb88320u;

RPVG_PLAN_FN constexpr uint32_t crcRawByte(uint32_t crc, const uint32_t byte) {
    crc ^= byte;
    for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (kCrcPoly & (0u - (crc & 1)));
    return crc;
}

RPVG_PLAN_FN constexpr uint32_t crcMul(const uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1)));
    }
    return p;
}

// x^(8 n): the operator that moves a residue past n bytes
RPVG_PLAN_FN constexpr uint32_t crcPowBytes(uint64_t n) {
    uint32_t result = 1u << 31, base = 1u << 23;  // x^0, x^8
    while (n) {
        if (n & 1) result = crcMul(result, base);
        base = crcMul(base, base);
        n >>= 1;
    }
    return result;
}

RPVG_PLAN_FN constexpr uint32_t crcShift(const uint32_t raw, const uint32_t pow_bytes) { return crcMul(pow_bytes, raw); }
RPVG_PLAN_FN constexpr uint32_t crcFinish(const uint32_t raw, const uint64_t n) { return raw ^ crcMul(crcPowBytes(n), 0xffffffffu) ^ 0xffffffffu; }

// The device's cut: a chunk, zero bytes in front of it up to kCrcSlices * kCrcSliceBytes, is kCrcSlices slices of equal length, so the
// operator between neighbours of each round of the tree is a constant: kCrcSlicePow, squared from round to round.
constexpr uint32_t kCrcSlices = 1024, kCrcSliceBytes = 64;
constexpr uint32_t kCrcSlicePow = crcPowBytes(kCrcSliceBytes);
static_assert(kCrcSlices * kCrcSliceBytes >= kChunkBytes, "the slices cover a chunk");

#if !defined(__HIP_DEVICE_COMPILE__)

inline uint32_t crc32(const void * data, const uint64_t n) {
    const unsigned char * bytes = static_cast<const unsigned char *>(data);
    uint32_t raw = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) raw = crcRawByte(raw, bytes[i]);
    return ~raw;
}

// ---- the host's own members: a writer's header row and `Unknown` row ------------------------------------------------------------------

inline const unsigned char * eofBlock() {
    static const unsigned char block[kEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return block;
}

struct ByteSink {
    std::string * out;
    uint64_t acc = 0;
    uint32_t bits = 0;
    void put(const uint32_t value, const uint32_t n) {
        acc |= static_cast<uint64_t>(value) << bits;
        bits += n;
        while (bits >= 8) {
            out->push_back(static_cast<char>(acc & 0xff));
            acc >>= 8;
            bits -= 8;
        }
    }
    void finish() {
        if (bits) out->push_back(static_cast<char>(acc & 0xff));
        acc = 0;
        bits = 0;
    }
};

// One member of at most kChunkBytes bytes appended to `out`: a dynamic block of literals coded with the routines above (rows of a
// few hundred bytes: there is nothing for matches to find that would repay them), or the stored form when that is not larger.
inline void frameMember(const char * data, const uint32_t n, std::string & out) {
    uint32_t lit_hist[kNumLitLen] = {}, dist_hist[kNumDist] = {}, cl_hist[kNumCodeLen], weight[2 * kNumLitLen];
    uint16_t order[kNumLitLen], parent[2 * kNumLitLen], per_len[16], lit_codes[kNumLitLen], dist_codes[kNumDist], cl_codes[kNumCodeLen];
    uint8_t lit_lens[kNumLitLen], dist_lens[kNumDist], cl_lens[kNumCodeLen];
    for (uint32_t i = 0; i < n; ++i) lit_hist[static_cast<unsigned char>(data[i])] += 1;
    lit_hist[kEndOfBlock] = 1;
    BlockCodes codes = {lit_lens, lit_codes, dist_lens, dist_codes, cl_hist, cl_lens, cl_codes, 0, 0, 0, 0};
    planBlock(lit_hist, dist_hist, codes, LengthWork{order, weight, parent, per_len});
    const uint64_t dynamic_bytes = (blockBits(lit_hist, dist_hist, codes) + 7) / 8;
    const bool stored = storedBytes(n) <= dynamic_bytes;
    const uint32_t member_bytes = kHeaderBytes + static_cast<uint32_t>(stored ? storedBytes(n) : dynamic_bytes) + kTrailerBytes;
    for (uint32_t i = 0; i < kHeaderBytes; ++i) out.push_back(static_cast<char>(memberHeaderByte(i, member_bytes)));
    if (stored) {
        for (uint32_t i = 0; i < kStoredHeadBytes; ++i) out.push_back(static_cast<char>(storedHeadByte(i, n)));
        out.append(data, n);
    } else {
        ByteSink sink{&out};
        putHeader(sink, codes);
        for (uint32_t i = 0; i < n; ++i) putLiteral(sink, codes, static_cast<unsigned char>(data[i]));
        putLiteral(sink, codes, kEndOfBlock);
        sink.finish();
    }
    const uint32_t crc = crc32(data, n);
    for (uint32_t i = 0; i < kTrailerBytes; ++i) out.push_back(static_cast<char>(memberTrailerByte(i, crc, n)));
}

// host-made bytes as members, chunk by chunk; no bytes: no member
inline void frameMembers(const char * data, const uint64_t n, std::string & out) {
    for (uint64_t c = 0; c < numChunks(n); ++c) frameMember(data + chunkBegin(c), chunkBytes(c, n), out);
}

inline void appendEof(std::string & out) { out.append(reinterpret_cast<const char *>(eofBlock()), kEofBytes); }

// ---- the device's member on the host, position by position ---------------------------------------------------------------------------------
// What deflateChunkKernel (text_deflate.hip) computes, written as one loop: the same rounds, the same table of maxima, the same
// candidates and ties, the same greedy parse, the same codes.  The device's members are these bytes; tests hold them to it.
inline void modelMember(const char * data, const uint32_t n, std::string & out, bool * stored_out = nullptr) {
    const unsigned char * bytes = reinterpret_cast<const unsigned char *>(data);
    const auto four_at = [&](const uint32_t p) {  // bytes behind the chunk read as zero
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; ++b) v |= static_cast<uint32_t>(p + b < n ? bytes[p + b] : 0) << (8 * b);
        return v;
    };
    const auto match_length = [&](const uint32_t p, const uint32_t c, const uint32_t most) {
        uint32_t l = 0;
        while (l < most && bytes[p + l] == bytes[c + l]) ++l;
        return l;
    };
    struct Token { uint32_t at, length, dist; };
    uint32_t table[1u << kHashBits] = {};
    uint32_t lit_hist[kNumLitLen] = {}, dist_hist[kNumDist] = {};
    uint32_t carry = 0;
    Token * tokens = new Token[n + 1];
    uint32_t num_tokens = 0;
    for (uint32_t base = 0; base < n; base += kRound) {
        uint32_t best[kRound] = {}, best_dist[kRound] = {};
        const uint32_t round_carry = carry;
        for (uint32_t t = 0; t < kRound; ++t) {
            const uint32_t p = base + t;
            if (p + kParseMinMatch > n || p < round_carry) continue;
            const uint32_t four = four_at(p), entry = table[hashOf(four)], most = n - p < kMaxMatch ? n - p : kMaxMatch;
            for (uint32_t d = 1; d <= 2; ++d) {
                if (p >= d && four_at(p - d) == four) {
                    const uint32_t l = match_length(p, p - d, most);
                    if (l > best[t]) best[t] = l, best_dist[t] = d;
                }
            }
            if (entry && p - (entry - 1) <= kMaxDist && four_at(entry - 1) == four) {
                const uint32_t l = match_length(p, entry - 1, most);
                if (l > best[t]) best[t] = l, best_dist[t] = p - (entry - 1);
            }
            if (best[t] < shortestMatchAt(best_dist[t])) best[t] = 0;
        }
        for (uint32_t t = 0; t < kRound && base + t + kParseMinMatch <= n; ++t) table[hashOf(four_at(base + t))] = base + t + 1;  // ascending: the maximum
        for (uint32_t t = 0; t < kRound && base + t < n; ++t) {
            const uint32_t p = base + t;
            if (p < carry) continue;
            tokens[num_tokens++] = Token{p, best[t], best_dist[t]};
            carry = p + (best[t] ? best[t] : 1);
        }
    }
    for (uint32_t i = 0; i < num_tokens; ++i) {
        if (tokens[i].length) {
            lit_hist[lengthCode(tokens[i].length)] += 1;
            dist_hist[distCode(tokens[i].dist)] += 1;
        } else {
            lit_hist[bytes[tokens[i].at]] += 1;
        }
    }
    lit_hist[kEndOfBlock] = 1;
    uint32_t cl_hist[kNumCodeLen], weight[2 * kNumLitLen];
    uint16_t order[kNumLitLen], parent[2 * kNumLitLen], per_len[16], lit_codes[kNumLitLen], dist_codes[kNumDist], cl_codes[kNumCodeLen];
    uint8_t lit_lens[kNumLitLen], dist_lens[kNumDist], cl_lens[kNumCodeLen];
    BlockCodes codes = {lit_lens, lit_codes, dist_lens, dist_codes, cl_hist, cl_lens, cl_codes, 0, 0, 0, 0};
    planBlock(lit_hist, dist_hist, codes, LengthWork{order, weight, parent, per_len});
    const uint64_t dynamic_bytes = (blockBits(lit_hist, dist_hist, codes) + 7) / 8;
    const bool stored = storedBytes(n) <= dynamic_bytes;
    if (stored_out) *stored_out = stored;
    const uint32_t member_bytes = kHeaderBytes + static_cast<uint32_t>(stored ? storedBytes(n) : dynamic_bytes) + kTrailerBytes;
    for (uint32_t i = 0; i < kHeaderBytes; ++i) out.push_back(static_cast<char>(memberHeaderByte(i, member_bytes)));
    if (stored) {
        for (uint32_t i = 0; i < kStoredHeadBytes; ++i) out.push_back(static_cast<char>(storedHeadByte(i, n)));
        out.append(data, n);
    } else {
        ByteSink sink{&out};
        putHeader(sink, codes);
        for (uint32_t i = 0; i < num_tokens; ++i) {
            if (tokens[i].length) putMatch(sink, codes, tokens[i].length, tokens[i].dist);
            else putLiteral(sink, codes, bytes[tokens[i].at]);
        }
        putLiteral(sink, codes, kEndOfBlock);
        sink.finish();
    }
    delete[] tokens;
    const uint32_t crc = crc32(data, n);
    for (uint32_t i = 0; i < kTrailerBytes; ++i) out.push_back(static_cast<char>(memberTrailerByte(i, crc, n)));
}

inline void modelMembers(const char * data, const uint64_t n, std::string & out, uint64_t * num_stored = nullptr) {
    for (uint64_t c = 0; c < numChunks(n); ++c) {
        bool stored = false;
        modelMember(data + chunkBegin(c), chunkBytes(c, n), out, &stored);
        if (num_stored) *num_stored += stored ? 1 : 0;
    }
}

#endif  // host

}  // namespace rpvg_text_deflate

#endif
