// The plan of the BGZF text (rpvg_amd/csrc/text_deflate_plan.hpp) without a GPU: chunk ranges, CRC-32 and its slice operators against
// zlib, the length and distance codes against RFC 1951's tables, limited code lengths against the unlimited Huffman cost, canonical
// codes against the RFC's example, and whole members — the host framing and the model of the device's member — inflated by zlib.
// Prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <random>
#include <string>
#include <vector>

#include <zlib.h>

#include "text_deflate_plan.hpp"

using namespace rpvg_text_deflate;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++failures > 20) std::exit(1);            \
        }                                                 \
    } while (0)

// RFC 1951, 3.2.5, typed from the document
static const int kRfcLengthBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int kRfcLengthExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int kRfcDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const int kRfcDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const int kRfcCodeLenOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

static void checkChunks() {
    const uint64_t sizes[] = {0, 1, 65279, 65280, 65281, 2 * 65280 + 1};
    const uint64_t chunks[] = {0, 1, 1, 1, 2, 3};
    for (int i = 0; i < 6; ++i) {
        const uint64_t n = sizes[i];
        CHECK(numChunks(n) == chunks[i], "numChunks(%llu)", (unsigned long long) n);
        uint64_t covered = 0;
        for (uint64_t c = 0; c < numChunks(n); ++c) {
            CHECK(chunkBegin(c) == covered, "chunk %llu of %llu begins at %llu", (unsigned long long) c, (unsigned long long) n, (unsigned long long) chunkBegin(c));
            const uint32_t bytes = chunkBytes(c, n);
            CHECK(bytes >= 1 && bytes <= kChunkBytes && (bytes == kChunkBytes || c + 1 == numChunks(n)), "chunk %llu of %llu has %u bytes", (unsigned long long) c, (unsigned long long) n, bytes);
            covered += bytes;
        }
        CHECK(covered == n, "the chunks of %llu cover %llu", (unsigned long long) n, (unsigned long long) covered);
    }
    CHECK(kMemberOverhead == 31 && kChunkBytes + kMemberOverhead <= kMaxMemberBytes, "a stored chunk fits a member");
}

static uint32_t rawOf(const unsigned char * bytes, const size_t n) {
    uint32_t raw = 0;
    for (size_t i = 0; i < n; ++i) raw = crcRawByte(raw, bytes[i]);
    return raw;
}

static void checkCrc(std::mt19937_64 & rng) {
    std::vector<unsigned char> data(kChunkBytes);
    for (auto & b : data) b = static_cast<unsigned char>(rng());
    const size_t sizes[] = {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 65279, 65280};
    for (const size_t n : sizes) {
        const uint32_t want = static_cast<uint32_t>(::crc32(0L, data.data(), static_cast<uInt>(n)));
        CHECK(rpvg_text_deflate::crc32(data.data(), n) == want, "crc32 of %zu bytes", n);
        CHECK(crcFinish(rawOf(data.data(), n), n) == want, "crcFinish of %zu bytes", n);
        // the device's cut: zero bytes in front up to kCrcSlices slices of kCrcSliceBytes, a tree over neighbours
        const size_t front = static_cast<size_t>(kCrcSlices) * kCrcSliceBytes - n;
        std::vector<uint32_t> level(kCrcSlices);
        for (uint32_t t = 0; t < kCrcSlices; ++t) {
            uint32_t raw = 0;
            for (uint32_t i = 0; i < kCrcSliceBytes; ++i) {
                const size_t v = static_cast<size_t>(t) * kCrcSliceBytes + i;
                if (v >= front) raw = crcRawByte(raw, data[v - front]);
            }
            level[t] = raw;
        }
        uint32_t pow = kCrcSlicePow;
        for (size_t width = kCrcSlices; width > 1; width /= 2) {
            for (size_t i = 0; i < width / 2; ++i) level[i] = crcShift(level[2 * i], pow) ^ level[2 * i + 1];
            pow = crcMul(pow, pow);
        }
        CHECK(crcFinish(level[0], n) == want, "the slice tree of %zu bytes", n);
        // two slices of any lengths
        const size_t cut = n / 3;
        CHECK((crcShift(rawOf(data.data(), cut), crcPowBytes(n - cut)) ^ rawOf(data.data() + cut, n - cut)) == rawOf(data.data(), n), "two slices of %zu bytes", n);
    }
    CHECK(kCrcSlicePow == crcPowBytes(64), "the slice operator");
}

static void checkCodeTables() {
    for (int length = 3; length <= 258; ++length) {
        int code = 28;
        while (kRfcLengthBase[code] > length) --code;
        if (length == 258) code = 28;
        else if (code == 28) code = 27;  // 227 .. 257 belong to code 284
        CHECK(lengthCode(length) == 257u + code, "length %d: code %u, the RFC's %d", length, lengthCode(length), 257 + code);
        CHECK(lengthExtraBits(257 + code) == (uint32_t) kRfcLengthExtra[code] && lengthBase(257 + code) == (uint32_t) kRfcLengthBase[code], "length code %d", 257 + code);
        const uint32_t extra = lengthExtraValue(length, 257 + code);
        CHECK(extra < (1u << kRfcLengthExtra[code]) && kRfcLengthBase[code] + extra == (uint32_t) length, "length %d: extra %u", length, extra);
    }
    for (int dist = 1; dist <= 32768; ++dist) {
        int code = 29;
        while (kRfcDistBase[code] > dist) --code;
        CHECK(distCode(dist) == (uint32_t) code, "distance %d: code %u, the RFC's %d", dist, distCode(dist), code);
        CHECK(distExtraBits(code) == (uint32_t) kRfcDistExtra[code] && distBase(code) == (uint32_t) kRfcDistBase[code], "distance code %d", code);
        const uint32_t extra = distExtraValue(dist, code);
        CHECK(extra < (1u << kRfcDistExtra[code]) && kRfcDistBase[code] + extra == (uint32_t) dist, "distance %d: extra %u", dist, extra);
    }
    for (int i = 0; i < 19; ++i) CHECK(codeLenOrder(i) == (uint32_t) kRfcCodeLenOrder[i], "code length order %d", i);
}

// the cost of Huffman's unlimited code, by a heap
static uint64_t unlimitedCost(const std::vector<uint32_t> & hist) {
    std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> heap;
    for (const uint32_t c : hist) {
        if (c) heap.push(c);
    }
    if (heap.size() == 1) return heap.top();
    uint64_t cost = 0;
    while (heap.size() > 1) {
        const uint64_t a = heap.top();
        heap.pop();
        const uint64_t b = heap.top();
        heap.pop();
        cost += a + b;
        heap.push(a + b);
    }
    return cost;
}

static void checkLengths(const char * what, const std::vector<uint32_t> & hist, const uint32_t limit, const bool must_cut) {
    const uint32_t n = static_cast<uint32_t>(hist.size());
    std::vector<uint8_t> lens(n);
    std::vector<uint16_t> order(n), parent(2 * n), per_len(16);
    std::vector<uint32_t> weight(2 * n);
    const uint32_t used = codeLengths(hist.data(), n, limit, lens.data(), LengthWork{order.data(), weight.data(), parent.data(), per_len.data()});
    uint64_t kraft = 0, cost = 0;
    uint32_t counted = 0, longest = 0;
    for (uint32_t s = 0; s < n; ++s) {
        CHECK((lens[s] != 0) == (hist[s] != 0), "%s: symbol %u has count %u and length %u", what, s, hist[s], lens[s]);
        CHECK(lens[s] <= limit, "%s: symbol %u has length %u above %u", what, s, lens[s], limit);
        if (lens[s]) {
            kraft += 1ull << (limit - lens[s]);
            cost += static_cast<uint64_t>(hist[s]) * lens[s];
            counted += 1;
            longest = std::max<uint32_t>(longest, lens[s]);
        }
    }
    CHECK(counted == used, "%s: %u used symbols, %u returned", what, counted, used);
    if (used == 1) CHECK(kraft == 1ull << (limit - 1), "%s: the single code has length 1", what);
    else CHECK(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu", what, (unsigned long long) kraft, 1ull << limit);
    const uint64_t unlimited = unlimitedCost(hist);
    CHECK(cost >= unlimited && cost * 100 <= unlimited * 101, "%s: cost %llu, unlimited %llu", what, (unsigned long long) cost, (unsigned long long) unlimited);
    if (must_cut) CHECK(longest == limit && cost > unlimited, "%s: the limit of %u does not bite: longest %u", what, limit, longest);  // the unlimited tree is deeper
}

static void checkCodeLengths() {
    std::vector<uint32_t> fib(kNumLitLen, 0);
    uint32_t a = 1, b = 1, sum = 0;
    for (int i = 0; i < 22; ++i) {  // 1 1 2 3 5 ... 17711: an unlimited code is 21 bits deep
        fib[40 + 3 * i] = a;
        sum += a;
        const uint32_t next = a + b;
        a = b;
        b = next;
    }
    CHECK(sum == 46367, "the Fibonacci counts sum to %u", sum);
    checkLengths("Fibonacci over 22 symbols", fib, kMaxBits, true);
    checkLengths("all 286 symbols once", std::vector<uint32_t>(kNumLitLen, 1), kMaxBits, false);
    std::vector<uint32_t> two(kNumLitLen, 0);
    two[48] = 7;
    two[256] = 1;
    checkLengths("one symbol and the end of block", two, kMaxBits, false);
    two[256] = 0;
    two[9] = 1000;
    checkLengths("two symbols", two, kMaxBits, false);
    std::vector<uint32_t> one(kNumDist, 0);
    one[5] = 3;
    checkLengths("one distance", one, kMaxBits, false);
    // A code-length histogram whose unlimited code is 10 bits deep: the lengths of a text block (most symbols unused, the used ones
    // between 2 and 9 bits, a tail of rare lengths).  The head is heavy, as it is wherever most of 316 symbols are unused, so the
    // cut to 7 bits costs far less than one percent: the optimum for these counts is within it, and the routine must be too.
    std::vector<uint32_t> cl(kNumCodeLen, 0);
    const uint32_t cl_counts[11] = {1, 1, 2, 4, 8, 16, 32, 64, 128, 3000, 9000};
    for (int i = 0; i < 11; ++i) cl[i] = cl_counts[i];
    checkLengths("a code-length histogram deeper than 7 bits", cl, kMaxCodeLenBits, true);
}

static void checkCanonical() {
    // RFC 1951, 3.2.2: the alphabet ABCDEFGH with lengths (3, 3, 3, 3, 3, 2, 4, 4) has the codes 010 011 100 101 110 00 1110 1111
    const uint8_t lens[8] = {3, 3, 3, 3, 3, 2, 4, 4};
    const uint32_t want[8] = {2, 3, 4, 5, 6, 0, 14, 15};
    uint16_t codes[8], next_code[16];
    canonicalCodes(lens, 8, codes, next_code);
    for (int s = 0; s < 8; ++s) {
        uint32_t reversed = 0;
        for (int bit = 0; bit < lens[s]; ++bit) reversed |= ((want[s] >> bit) & 1) << (lens[s] - 1 - bit);
        CHECK(codes[s] == reversed, "symbol %d: code %u reversed, want %u", s, codes[s], reversed);
    }
}

// every member of `framed` by the rules of the format, its text inflated by zlib
static std::string inflateMembers(const std::string & framed, const char * what, uint64_t * stored = nullptr) {
    std::string text;
    size_t at = 0;
    while (at < framed.size()) {
        CHECK(framed.size() - at >= kHeaderBytes + kTrailerBytes, "%s: a member of %zu bytes", what, framed.size() - at);
        const unsigned char * m = reinterpret_cast<const unsigned char *>(framed.data()) + at;
        const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        CHECK(std::memcmp(m, head, 16) == 0, "%s: header at %zu", what, at);
        const size_t size = (m[16] | m[17] << 8) + 1u;
        CHECK(size <= kMaxMemberBytes && at + size <= framed.size(), "%s: BSIZE at %zu", what, at);
        if (at + size > framed.size()) return text;
        if (stored && (m[18] & 6) == 0) *stored += 1;
        std::vector<unsigned char> chunk(kChunkBytes + 1);
        z_stream z;
        std::memset(&z, 0, sizeof(z));
        CHECK(inflateInit2(&z, -15) == Z_OK, "inflateInit2");
        z.next_in = const_cast<unsigned char *>(m) + kHeaderBytes;
        z.avail_in = static_cast<uInt>(size - kHeaderBytes - kTrailerBytes);
        z.next_out = chunk.data();
        z.avail_out = static_cast<uInt>(chunk.size());
        const int rc = inflate(&z, Z_FINISH);
        CHECK(rc == Z_STREAM_END && z.avail_in == 0, "%s: inflate of the member at %zu gave %d (%s), %u bytes left", what, at, rc, z.msg ? z.msg : "", z.avail_in);
        const size_t n = z.total_out;
        inflateEnd(&z);
        CHECK(n <= kChunkBytes && size <= n + kMemberOverhead, "%s: a member of %zu bytes for %zu", what, size, n);
        const unsigned char * t = m + size - kTrailerBytes;
        const uint32_t crc = t[0] | t[1] << 8 | t[2] << 16 | static_cast<uint32_t>(t[3]) << 24, isize = t[4] | t[5] << 8 | t[6] << 16 | static_cast<uint32_t>(t[7]) << 24;
        CHECK(crc == static_cast<uint32_t>(::crc32(0L, chunk.data(), static_cast<uInt>(n))) && isize == n, "%s: trailer of the member at %zu", what, at);
        text.append(reinterpret_cast<const char *>(chunk.data()), n);
        at += size;
    }
    return text;
}

static void checkMembers(std::mt19937_64 & rng) {
    std::vector<std::pair<const char *, std::string>> texts;
    texts.emplace_back("a header row", "Name\tClusterID\tLength\tEffectiveLength\tReadCount\tTPM\n");
    texts.emplace_back("one byte", "x");
    texts.emplace_back("an Unknown row", "Unknown\t0\t0\t0\t12345.5\t0\n");
    std::string digits(2 * kChunkBytes + 1, '0'), random(kChunkBytes + 700, '\0'), repeated(kChunkBytes, 'a'), period(70000, '0'), rows;
    for (auto & c : digits) c = "0123456789\t"[rng() % 11];
    for (auto & c : random) c = static_cast<char>(rng());
    for (size_t i = 0; i < period.size(); ++i) period[i] = "0\t"[i % 2];
    for (int r = 0; r < 3000; ++r) {
        rows += "transcript_" + std::to_string(rng() % 50) + "_hap" + std::to_string(r % 7) + "\t" + std::to_string(r / 40);
        for (int c = 0; c < 12; ++c) rows += "\t" + std::to_string((rng() % 1000) / 8.0).substr(0, 7);
        rows += "\n";
    }
    std::string far = random.substr(0, 300);  // 300 bytes again 32 768 and 32 769 bytes later, and across the end of a chunk
    far.resize(32768, 'q');
    for (size_t i = 300; i < far.size(); ++i) far[i] = static_cast<char>(rng());
    far += random.substr(0, 300);
    far.resize(2 * 32768 + 1, 'r');
    far += random.substr(0, 300);
    far.resize(kChunkBytes - 150, 's');
    far += random.substr(0, 300);
    texts.emplace_back("digits and tabs", digits);
    texts.emplace_back("random bytes", random);
    texts.emplace_back("one byte repeated", repeated);
    texts.emplace_back("period two", period);
    texts.emplace_back("rows", rows);
    texts.emplace_back("far repeats", far);
    for (const size_t n : {size_t(2), size_t(3), size_t(4), size_t(5), size_t(257), size_t(258), size_t(259), size_t(260), size_t(1023), size_t(1024), size_t(1025), size_t(1027)}) {
        texts.emplace_back("a short run", std::string(n, 'z'));
        texts.emplace_back("short digits", digits.substr(0, n));
    }
    for (const auto & named : texts) {
        const std::string & text = named.second;
        std::string framed, model;
        frameMembers(text.data(), text.size(), framed);
        CHECK(inflateMembers(framed, named.first) == text, "%s: the host framing does not give the text back", named.first);
        uint64_t stored = 0, seen_stored = 0;
        modelMembers(text.data(), text.size(), model, &stored);
        CHECK(inflateMembers(model, named.first, &seen_stored) == text, "%s: the model's members do not give the text back", named.first);
        CHECK(stored == seen_stored, "%s: %llu stored members, %llu counted", named.first, (unsigned long long) stored, (unsigned long long) seen_stored);
        if (named.second.size() == kChunkBytes && named.second[0] == 'a') CHECK(model.size() <= 1024, "one byte repeated: %zu bytes", model.size());
        if (&named.second == &texts[3].second) CHECK(model.size() <= text.size() / 2, "digits and tabs: %zu of %zu bytes", model.size(), text.size());
        if (&named.second == &texts[4].second) CHECK(stored == 2 && model.size() == text.size() + 2 * kMemberOverhead, "random bytes: %llu stored", (unsigned long long) stored);
    }
    std::string none;
    frameMembers(nullptr, 0, none);
    modelMembers(nullptr, 0, none);
    CHECK(none.empty(), "no bytes, no member");
    appendEof(none);
    CHECK(none.size() == kEofBytes && inflateMembers(none, "the end-of-file block").empty(), "the end-of-file block");
}

int main() {
    std::mt19937_64 rng(20240611);
    checkChunks();
    checkCrc(rng);
    checkCodeTables();
    checkCodeLengths();
    checkCanonical();
    checkMembers(rng);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
