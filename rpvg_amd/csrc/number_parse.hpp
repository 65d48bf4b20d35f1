// Decimal text as a double and as an unsigned integer, for the kernels of rows_parse.hip and for the CPU
// (tests/cpp/number_parse_check.cpp holds parseDouble to glibc's strtod bit for bit): the inverse of number_text.hpp, plain C++17
// under the RPVG_PLAN_FN convention of the *_plan.hpp files, no HIP.
//
// Takes over   std::stod / std::stoul on the cells of the --write-probs dump      rpvg_amd/host/io/cluster_io.cpp:135-251
//
// Token        [-] digits [. digits] [(e|E) [+|-] digits]   with at least one digit in front of the exponent ("1.", ".5" and "00012.5"
//              are tokens), or one of the four words "%g" prints: inf, -inf, nan, -nan.  Anything else is kMalformed: an empty token,
//              a '+' in front, hex, a space, bytes behind the number.  The significant digits are those from the first non-zero digit
//              to the last digit written (trailing zeros count, leading zeros do not); more than 19 of them are kTooLong.
//
// parseDouble  A token of at most 19 significant digits is w 10^q with an integer w < 10^19 < 2^64.  Its double is the CORRECTLY
//              rounded one (ties to even): what glibc's strtod and Python's float() return, for every exponent, subnormals, the
//              underflow to +-0 and -0 included.
//                1. w = 0: +-0.  q < -342: w 10^q < 10^-323 < 2^-1075, half the smallest subnormal: +-0.  q > 308: kOverflow.
//                2. w64 = w shifted to the top of 64 bits (by lz).  With 10^q = T 2^E of the table (T in [2^127, 2^128), truncated),
//                   U = the top 128 bits of w64 T leaves the exact value V = w64 10^q / 2^(E + 64) inside [U, U + 2): less than one
//                   unit for the bits of w64 T_lo dropped, less than one for the truncation of T.  A unit is 2^(E + 64 - lz).
//                3. U has its top bit at 126 or 127; that places the value's binary exponent b and the exponent e2 = max(b - 52,
//                   -1074) of the result's last place.  U = m 2^s + fraction with s = e2 - (E + 64 - lz) >= 74.
//                   fraction > half: up (V >= U).  fraction + 2 <= half: down (V < U + 2).  Here the 128-bit product HAS decided,
//                   whatever the place of V inside [U, U + 2): also when V crosses a power of two above U (then the fraction is
//                   all ones and m + 1 = 2^53 is that power).
//                4. Otherwise — an exact tie, or a token within 2^(1 - s) relative of the middle of two doubles — the sign of
//                   w 10^q - (2 m + 1) 2^(e2 - 1) decides, as integers: compareExact(w, -e2, q, m) of number_text.hpp.  A tie goes
//                   to the even m.  *exact says that the token went this way.
//                   The words: for q < 0 the larger side is at most (2 m + 1) 5^-q < 2^54 5^342 < 2^849 or w 2^(q + 1 - e2) within a
//                   factor of four of it; for q >= 0 it is w 5^q < 2^64 5^308 < 2^780 or (2 m + 1) 2^(e2 - 1 - q) of the same size.  Both
//                   are below the 896 bits of kExactWords (RPVG_NUMBER_TEXT_CHECKED traps on a carry out of them).
//                5. m = 2^53 after an "up" is 2^52 one exponent above; a biased exponent of 2047 is kOverflow (so is a value whose U
//                   alone lies at or above 2^1024, before any rounding).  A subnormal m = 2^52 is the smallest normal by its encoding.
//              No array is indexed by a run-time value but the table and the bytes; multiword loops have constant length.
#ifndef RPVG_HIP_NUMBER_PARSE_HPP
#define RPVG_HIP_NUMBER_PARSE_HPP

#include "number_text.hpp"

namespace rpvg_number_parse {

using rpvg_number_text::u128;

enum Status { kOk = 0, kOverflow = 1, kTooLong = 2, kMalformed = 3 };

constexpr int kMaxDigits = 19;
constexpr int kExponentClamp = 100000;  // beyond any q that matters; keeps the sum of the exponent and the digits' shift in an int

struct Parsed {
    double value;
    int status;
    bool exact;  // decided by compareExact
};

RPVG_PLAN_FN double fromBits(const uint64_t bits) {
    double v;
    __builtin_memcpy(&v, &bits, sizeof(v));
    return v;
}

RPVG_PLAN_FN bool isDigit(const char c) { return c >= '0' && c <= '9'; }

// digits only, at most 19 of them (the host reader's marker check): *value < 10^19
RPVG_PLAN_FN int parseU64(const char * __restrict__ bytes, const uint64_t n, uint64_t * value) {
    *value = 0;
    if (n == 0) return kMalformed;
    uint64_t v = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!isDigit(bytes[i])) return kMalformed;
        if (i < static_cast<uint64_t>(kMaxDigits)) v = v * 10u + static_cast<uint64_t>(bytes[i] - '0');
    }
    if (n > static_cast<uint64_t>(kMaxDigits)) return kTooLong;
    *value = v;
    return kOk;
}

// w 10^q, w in [1, 10^19), as the bits of the correctly rounded double without its sign; kOverflow: it rounds to infinity
RPVG_PLAN_FN int roundDecimal(const uint64_t w, const int q, const uint64_t * __restrict__ pow10, uint64_t * bits, bool * exact) {
    *bits = 0;
    if (q < rpvg_number_text::kMinPow10) return kOk;  // below 2^-1075
    if (q > 308) return kOverflow;
    const int lz = __builtin_clzll(w);
    const uint64_t w64 = w << lz;
    const int at = 2 * (q - rpvg_number_text::kMinPow10);
    const uint64_t hi = pow10[at], lo = pow10[at + 1];
    const u128 U = static_cast<u128>(w64) * hi + ((static_cast<u128>(w64) * lo) >> 64);
    const int unit = rpvg_number_text::pow10BinaryExponent(q) + 64 - lz;  // V = value / 2^unit
    const int b = unit + ((U >> 127) ? 127 : 126);                         // 2^b <= U 2^unit < 2^(b + 1)
    if (b >= 1024) return kOverflow;
    const int e2 = b - 52 < -1074 ? -1074 : b - 52;
    const int s = e2 - unit;  // >= 74
    uint64_t m;
    bool up;
    if (s >= 129) {  // V < 2^128 + 1 <= half, but for the last two values of U at s = 129
        m = 0;
        if (s == 129 && U >= ~static_cast<u128>(1)) {
            *exact = true;
            up = rpvg_number_text::compareExact(w, -e2, q, 0) > 0;  // (a tie stays at the even 0)
        } else {
            up = false;
        }
    } else {
        const u128 fraction = s == 128 ? U : U & ((static_cast<u128>(1) << s) - 1);
        const u128 half = static_cast<u128>(1) << (s - 1);
        m = s == 128 ? 0 : static_cast<uint64_t>(U >> s);
        if (fraction > half) up = true;
        else if (fraction + 2 <= half) up = false;
        else {
            const int sign = rpvg_number_text::compareExact(w, -e2, q, m);
            *exact = true;
            up = sign > 0 || (sign == 0 && (m & 1u));
        }
    }
    m += up ? 1u : 0u;
    int exponent = e2;
    if (m == (1ull << 53)) {
        m = 1ull << 52;
        ++exponent;
    }
    // normal: m in [2^52, 2^53), biased = exponent + 1075; a subnormal has exponent -1074 and m < 2^52, and its bits are m
    if (m < (1ull << 52)) {
        *bits = m;
        return kOk;
    }
    const int biased = exponent + 1075;
    if (biased >= 2047) return kOverflow;
    *bits = (static_cast<uint64_t>(biased) << 52) | (m & ((1ull << 52) - 1));
    return kOk;
}

RPVG_PLAN_FN Parsed parseDouble(const char * __restrict__ bytes, const uint64_t n, const uint64_t * __restrict__ pow10) {
    Parsed r;
    r.value = 0;
    r.status = kMalformed;
    r.exact = false;
    uint64_t i = 0;
    bool negative = false;
    if (i < n && bytes[i] == '-') {
        negative = true;
        ++i;
    }
    const uint64_t sign_bit = negative ? 1ull << 63 : 0;
    if (n - i == 3) {
        const char a = bytes[i], b = bytes[i + 1], c = bytes[i + 2];
        if (a == 'i' && b == 'n' && c == 'f') {
            r.value = fromBits(sign_bit | 0x7ff0000000000000ull);
            r.status = kOk;
            return r;
        }
        if (a == 'n' && b == 'a' && c == 'n') {
            r.value = fromBits(sign_bit | 0x7ff8000000000000ull);
            r.status = kOk;
            return r;
        }
    }
    uint64_t w = 0;
    int significant = 0;    // digits from the first non-zero one
    int64_t shift = 0;      // digits behind the point
    uint64_t digits = 0;    // digits of either side
    bool point = false, too_long = false;
    for (; i < n; ++i) {
        const char c = bytes[i];
        if (c == '.') {
            if (point) return r;
            point = true;
            continue;
        }
        if (!isDigit(c)) break;
        ++digits;
        if (point && shift < kExponentClamp) ++shift;
        else if (point) too_long = true;  // (a hundred thousand digits behind the point)
        if (significant > 0 || c != '0') {
            if (significant < kMaxDigits) w = w * 10u + static_cast<uint64_t>(c - '0');
            else too_long = true;
            ++significant;
            if (significant > kMaxDigits) significant = kMaxDigits + 1;
        }
    }
    if (digits == 0) return r;
    int64_t exponent = 0;
    if (i < n) {
        if (bytes[i] != 'e' && bytes[i] != 'E') return r;
        ++i;
        bool exponent_negative = false;
        if (i < n && (bytes[i] == '-' || bytes[i] == '+')) {
            exponent_negative = bytes[i] == '-';
            ++i;
        }
        if (i == n) return r;
        for (; i < n; ++i) {
            if (!isDigit(bytes[i])) return r;
            if (exponent < kExponentClamp) exponent = exponent * 10 + (bytes[i] - '0');
        }
        if (exponent_negative) exponent = -exponent;
    }
    if (too_long) {
        r.status = kTooLong;
        return r;
    }
    if (w == 0) {
        r.value = fromBits(sign_bit);
        r.status = kOk;
        return r;
    }
    int64_t q = exponent - shift;
    if (q < -kExponentClamp) q = -kExponentClamp;
    uint64_t bits = 0;
    r.status = roundDecimal(w, static_cast<int>(q), pow10, &bits, &r.exact);
    if (r.status == kOk) r.value = fromBits(sign_bit | bits);
    return r;
}

}  // namespace rpvg_number_parse

#endif
