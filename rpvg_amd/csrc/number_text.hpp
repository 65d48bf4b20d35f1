// A double as the text of printf("%.*g") and an unsigned integer as decimal text, for the kernels of table_text.hip and for the CPU
// (tests/cpp/number_text_check.cpp holds formatG to glibc byte for byte): plain C++17 under the RPVG_PLAN_FN convention of the
// *_plan.hpp files, no HIP.
//
// Takes over   the stream insertions of a double at setprecision(8) in the default float field, i.e. "%.8g"
//              src/threaded_output_writer.cpp:6, :160-201, :295-322, :358-411
//
// formatG      The value is rounded CORRECTLY to `precision` significant digits (the exact binary value, ties to even), for every bit
//              pattern and every precision 1 .. 17:
//                1. v = m64 * 2^e with the significand shifted to the top of 64 bits; k = floor((e + 63) log10 2) is the decimal
//                   exponent of v or one below it.
//                2. v * 10^q for q = precision - 1 - k is the 64 x 128-bit product with the truncated power of ten of the table
//                   (10^q = T * 2^E, T in [2^127, 2^128), 683 entries of 16 bytes made exactly by buildPow10Table on the host).  The
//                   top 128 bits U of the product leave the exact value inside [U, U + 2) units (one unit for the bits of m64 * T_lo
//                   dropped, less than one for the truncation of T); they split into the integer I of `precision` digits and a
//                   fraction of at least 64 bits.  I >= 10^precision: k was one below, once more with q - 1.
//                3. fraction + 2 <= half: down.  fraction > half: up.  Otherwise (an exact tie, or a double within 2^-60 relative of
//                   one) the sign of m 2^(e2+1) 10^q - (2 I + 1) decides, as integers of 28 words (compareExact: at most 864 bits);
//                   a tie goes to the even I.  `exact` says that the cell went that way, `tie` that it was one.
//                4. A carry to 10^precision is 10^(precision-1) one decade up; the notation is chosen from the exponent after that.
//              Digits come out by division by constants of a value scaled to 17 digits; no array is indexed by a run-time value (the
//              28 words of compareExact are walked by loops of constant length).
#ifndef RPVG_HIP_NUMBER_TEXT_HPP
#define RPVG_HIP_NUMBER_TEXT_HPP

#include <cstdint>

#ifndef RPVG_PLAN_FN
#if defined(__HIPCC__)
#define RPVG_PLAN_FN __host__ __device__ inline
#else
#define RPVG_PLAN_FN inline
#endif
#endif

#include <vector>

// the loops over the words of the exact comparison have constant lengths: unrolled, the words are registers on the device
#if defined(__clang__)
#define RPVG_NUMBER_TEXT_UNROLL _Pragma("unroll")
#else
#define RPVG_NUMBER_TEXT_UNROLL
#endif

namespace rpvg_number_text {

typedef unsigned __int128 u128;

constexpr int kMinPrecision = 1, kMaxPrecision = 17;
constexpr int kMaxCellBytes = 24;                     // -1.2345678901234567e-308
constexpr int kMinPow10 = -342, kMaxPow10 = 340;      // formatG: q = precision - 1 - k, k in -324 .. 308, and q - 1 (-309 .. 340);
                                                      // parseDouble (number_parse.hpp): 19 digits at the smallest subnormal, q >= -342
constexpr int kPow10Entries = kMaxPow10 - kMinPow10 + 1;
constexpr int kPow10Words = 2 * kPow10Entries;        // entry i: 10^(kMinPow10 + i) as words[2 i] (high) and words[2 i + 1] (low)
constexpr int kExactWords = 28;                       // of 32 bits

// floor(e log10 2) for |e| <= 1200 and floor(q log2 10) for |q| <= 400 (tests/cpp/number_text_check.cpp walks both ranges)
RPVG_PLAN_FN int floorLog10Pow2(const int e) { return static_cast<int>((static_cast<int64_t>(e) * 78913) >> 18); }
RPVG_PLAN_FN int floorLog2Pow10(const int q) { return static_cast<int>((static_cast<int64_t>(q) * 1741647) >> 19); }
// E of 10^q = T * 2^E
RPVG_PLAN_FN int pow10BinaryExponent(const int q) { return floorLog2Pow10(q) + 1 - 128; }

// 10^n, n in 0 .. 19
RPVG_PLAN_FN uint64_t tenTo(const int n) {
    uint64_t r = 1;
    for (int i = 0; i < n; ++i) r *= 10u;
    return r;
}

enum Kind { kFinite = 0, kZero = 1, kInf = 2, kNan = 3 };

struct Decimal {
    uint64_t digits;  // kFinite: the `precision` digits, in [10^(precision-1), 10^precision)
    int exponent;     // kFinite: the decimal exponent of the first digit
    int kind;
    bool negative;
    bool exact;       // the rounding was decided by compareExact
    bool tie;         // ... and was a tie
    bool rounded_up;  // the digits are one above the truncated ones (a tie that went up had odd digits, one that stayed had even)
};

// ---- the exact comparison ---------------------------------------------------------------------------------------------------

RPVG_PLAN_FN void mulSmall(uint32_t (&w)[kExactWords], const uint32_t f) {
    uint64_t carry = 0;
    RPVG_NUMBER_TEXT_UNROLL
    for (int i = 0; i < kExactWords; ++i) {
        const uint64_t t = static_cast<uint64_t>(w[i]) * f + carry;
        w[i] = static_cast<uint32_t>(t);
        carry = t >> 32;
    }
#if defined(RPVG_NUMBER_TEXT_CHECKED)
    if (carry != 0) __builtin_trap();
#endif
}

RPVG_PLAN_FN void mulPow5(uint32_t (&w)[kExactWords], int n) {
    for (; n >= 13; n -= 13) mulSmall(w, 1220703125u);  // 5^13
    uint32_t f = 1;
    for (; n > 0; --n) f *= 5u;
    mulSmall(w, f);
}

RPVG_PLAN_FN void mulPow2(uint32_t (&w)[kExactWords], int n) {
    for (; n >= 31; n -= 31) mulSmall(w, 1u << 31);
    mulSmall(w, 1u << n);
}

// the sign of m 2^(e2 + 1) 10^q - (2 I + 1): twice the distance of m 2^e2 10^q from I + 1/2
RPVG_PLAN_FN int compareExact(const uint64_t m, const int e2, const int q, const uint64_t I) {
    uint32_t a[kExactWords], b[kExactWords];
    RPVG_NUMBER_TEXT_UNROLL
    for (int i = 0; i < kExactWords; ++i) a[i] = b[i] = 0;
    const uint64_t odd = 2 * I + 1;
    a[0] = static_cast<uint32_t>(m);
    a[1] = static_cast<uint32_t>(m >> 32);
    b[0] = static_cast<uint32_t>(odd);
    b[1] = static_cast<uint32_t>(odd >> 32);
    int shift = e2 + 1;  // of a against b
    if (q >= 0) {
        mulPow5(a, q);
        shift += q;
    } else {
        mulPow5(b, -q);
        shift += q;
    }
    if (shift >= 0) mulPow2(a, shift);
    else mulPow2(b, -shift);
    int sign = 0;
    RPVG_NUMBER_TEXT_UNROLL
    for (int i = kExactWords - 1; i >= 0; --i) {
        if (sign == 0 && a[i] != b[i]) sign = a[i] > b[i] ? 1 : -1;
    }
    return sign;
}

// ---- value -> digits and exponent ------------------------------------------------------------------------------------------

RPVG_PLAN_FN uint64_t bitsOf(const double v) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, sizeof(bits));
    return bits;
}

// I and the fraction of m64 2^e 10^q (step 2 above); *frac_bits: the width of the fraction, 64 .. 127
RPVG_PLAN_FN uint64_t scaledBy(const uint64_t m64, const int e, const int q, const uint64_t * __restrict__ pow10, u128 * frac, int * frac_bits) {
    const int at = 2 * (q - kMinPow10);
    const uint64_t hi = pow10[at], lo = pow10[at + 1];
    const u128 top = static_cast<u128>(m64) * hi + ((static_cast<u128>(m64) * lo) >> 64);
    int s = -(e + pow10BinaryExponent(q)) - 64;
    s = s < 64 ? 64 : (s > 127 ? 127 : s);  // (it is inside already: the integer has at most 61 bits and the value is at least 1 - 2^-60)
    *frac_bits = s;
    *frac = top & ((static_cast<u128>(1) << s) - 1);
    return static_cast<uint64_t>(top >> s);
}

RPVG_PLAN_FN Decimal decompose(const double v, const int precision, const uint64_t * __restrict__ pow10) {
    const uint64_t bits = bitsOf(v);
    Decimal d;
    d.digits = 0;
    d.exponent = 0;
    d.negative = (bits >> 63) != 0;
    d.exact = d.tie = d.rounded_up = false;
    const int biased = static_cast<int>((bits >> 52) & 0x7ff);
    const uint64_t fraction = bits & ((1ull << 52) - 1);
    if (biased == 0x7ff) {
        d.kind = fraction ? kNan : kInf;
        return d;
    }
    if (biased == 0 && fraction == 0) {
        d.kind = kZero;
        return d;
    }
    d.kind = kFinite;
    const uint64_t m = biased ? fraction | (1ull << 52) : fraction;
    const int e2 = biased ? biased - 1075 : -1074;
    const int lz = __builtin_clzll(m);
    const uint64_t m64 = m << lz;
    const int e = e2 - lz;
    int k = floorLog10Pow2(e + 63);
    const uint64_t limit = tenTo(precision);
    u128 frac;
    int frac_bits;
    uint64_t I = scaledBy(m64, e, precision - 1 - k, pow10, &frac, &frac_bits);
    if (I >= limit) {
        ++k;
        I = scaledBy(m64, e, precision - 1 - k, pow10, &frac, &frac_bits);
    }
    const u128 half = static_cast<u128>(1) << (frac_bits - 1);
    bool up;
    if (frac + 2 <= half) up = false;
    else if (frac > half) up = true;
    else {
        const int sign = compareExact(m, e2, precision - 1 - k, I);
        d.exact = true;
        d.tie = sign == 0;
        up = sign > 0 || (sign == 0 && (I & 1u));
    }
    d.rounded_up = up;
    uint64_t D = I + (up ? 1u : 0u);
    if (D >= limit) {
        D = limit / 10u;
        ++k;
    }
    d.digits = D;
    d.exponent = k;
    return d;
}

// ---- digits -> text -----------------------------------------------------------------------------------------------------------

// put(j, digit) for the 8 digits of x < 10^8, the first as j = first
template <typename Put>
RPVG_PLAN_FN void eightDigits(const uint32_t x, const int first, Put put) {
    const uint32_t a = x / 10000u, b = x % 10000u;
    const uint32_t a0 = a / 100u, a1 = a % 100u, b0 = b / 100u, b1 = b % 100u;
    put(first + 0, a0 / 10u);
    put(first + 1, a0 % 10u);
    put(first + 2, a1 / 10u);
    put(first + 3, a1 % 10u);
    put(first + 4, b0 / 10u);
    put(first + 5, b0 % 10u);
    put(first + 6, b1 / 10u);
    put(first + 7, b1 % 10u);
}

// put(j, digit) for the 17 digits of x < 10^17, the most significant as j = 0
template <typename Put>
RPVG_PLAN_FN void seventeenDigits(const uint64_t x, Put put) {
    const uint64_t rest = x % 10000000000000000ull;
    put(0, static_cast<uint32_t>(x / 10000000000000000ull));
    eightDigits(static_cast<uint32_t>(rest / 100000000ull), 1, put);
    eightDigits(static_cast<uint32_t>(rest % 100000000ull), 9, put);
}

// The text of a decomposed value; kStore = false: its length alone (out is not touched).
template <bool kStore>
RPVG_PLAN_FN int textOf(const Decimal & d, const int precision, char * out) {
    int n = 0;
    if (d.negative) {
        if (kStore) out[0] = '-';
        n = 1;
    }
    if (d.kind != kFinite) {
        if (d.kind == kZero) {
            if (kStore) out[n] = '0';
            return n + 1;
        }
        if (kStore) {
            out[n] = d.kind == kInf ? 'i' : 'n';
            out[n + 1] = d.kind == kInf ? 'n' : 'a';
            out[n + 2] = d.kind == kInf ? 'f' : 'n';
        }
        return n + 3;
    }
    const uint64_t scaled = d.digits * tenTo(kMaxPrecision - precision);  // 17 digits, the text's digits first
    int nd = 1;                                                          // without the trailing zeros
    seventeenDigits(scaled, [&](const int j, const uint32_t digit) {
        if (digit) nd = j + 1;
    });
    const int X = d.exponent;
    if (X >= -4 && X < precision) {
        if (X >= 0) {
            const int whole = nd > X + 1 ? nd : X + 1;  // digits printed (the zeros up to the point are digits of `scaled` too)
            if (kStore) {
                seventeenDigits(scaled, [&](const int j, const uint32_t digit) {
                    if (j < whole) out[n + j + (j > X ? 1 : 0)] = static_cast<char>('0' + digit);
                });
                if (nd > X + 1) out[n + X + 1] = '.';
            }
            return n + whole + (nd > X + 1 ? 1 : 0);
        }
        const int zeros = -X - 1;  // 0 .. 3
        if (kStore) {
            out[n] = '0';
            out[n + 1] = '.';
            for (int i = 0; i < 3; ++i) {
                if (i < zeros) out[n + 2 + i] = '0';
            }
            seventeenDigits(scaled, [&](const int j, const uint32_t digit) {
                if (j < nd) out[n + 2 + zeros + j] = static_cast<char>('0' + digit);
            });
        }
        return n + 2 + zeros + nd;
    }
    if (kStore) {
        seventeenDigits(scaled, [&](const int j, const uint32_t digit) {
            if (j < nd) out[n + j + (j > 0 ? 1 : 0)] = static_cast<char>('0' + digit);
        });
        if (nd > 1) out[n + 1] = '.';
    }
    n += nd + (nd > 1 ? 1 : 0);
    uint32_t magnitude = static_cast<uint32_t>(X < 0 ? -X : X);
    if (kStore) {
        out[n] = 'e';
        out[n + 1] = X < 0 ? '-' : '+';
    }
    n += 2;
    if (magnitude >= 100u) {
        if (kStore) out[n] = static_cast<char>('0' + magnitude / 100u);
        magnitude %= 100u;
        n += 1;
    }
    if (kStore) {
        out[n] = static_cast<char>('0' + magnitude / 10u);
        out[n + 1] = static_cast<char>('0' + magnitude % 10u);
    }
    return n + 2;
}

// what snprintf(out, n, "%.*g", precision, v) writes, without the terminator: at most kMaxCellBytes bytes; returns their number
RPVG_PLAN_FN int formatG(const double v, const int precision, char * out, const uint64_t * __restrict__ pow10) {
    return textOf<true>(decompose(v, precision, pow10), precision, out);
}

RPVG_PLAN_FN int decimalDigits(const uint32_t x) {
    int n = 1;
    if (x >= 10u) n = 2;
    if (x >= 100u) n = 3;
    if (x >= 1000u) n = 4;
    if (x >= 10000u) n = 5;
    if (x >= 100000u) n = 6;
    if (x >= 1000000u) n = 7;
    if (x >= 10000000u) n = 8;
    if (x >= 100000000u) n = 9;
    if (x >= 1000000000u) n = 10;
    return n;
}

// x in decimal: at most 10 bytes, no terminator; returns their number
RPVG_PLAN_FN int formatU32(const uint32_t x, char * out) {
    const int n = decimalDigits(x), skipped = 10 - n;
    const uint32_t high = x / 100000000u;  // two digits
    const auto put = [&](const int j, const uint32_t digit) {
        if (j >= skipped) out[j - skipped] = static_cast<char>('0' + digit);
    };
    put(0, high / 10u);
    put(1, high % 10u);
    eightDigits(x % 100000000u, 2, put);
    return n;
}

RPVG_PLAN_FN int decimalDigits64(const uint64_t x) {
    if (x <= 0xffffffffull) return decimalDigits(static_cast<uint32_t>(x));
    int n = 10;
    uint64_t power = 10000000000ull;  // 10^10 .. 10^19 < 2^64
    for (int i = 10; i <= 19; ++i) {
        if (x >= power) n = i + 1;
        if (i < 19) power *= 10u;
    }
    return n;
}

// x in decimal: at most 20 bytes, no terminator; returns their number
RPVG_PLAN_FN int formatU64(const uint64_t x, char * out) {
    const int n = decimalDigits64(x), skipped = 20 - n;
    const uint32_t high = static_cast<uint32_t>(x / 10000000000000000ull);  // four digits
    const uint64_t rest = x % 10000000000000000ull;
    const auto put = [&](const int j, const uint32_t digit) {
        if (j >= skipped) out[j - skipped] = static_cast<char>('0' + digit);
    };
    put(0, high / 1000u);
    put(1, high / 100u % 10u);
    put(2, high / 10u % 10u);
    put(3, high % 10u);
    eightDigits(static_cast<uint32_t>(rest / 100000000ull), 4, put);
    eightDigits(static_cast<uint32_t>(rest % 100000000ull), 12, put);
    return n;
}

// ---- the table of powers of ten (host) ----------------------------------------------------------------------------------------

namespace big {

typedef std::vector<uint32_t> Number;  // little endian, no leading zero words (zero: empty)

inline void trim(Number & a) {
    while (!a.empty() && a.back() == 0) a.pop_back();
}

inline void mulSmall(Number & a, const uint32_t f) {
    uint64_t carry = 0;
    for (auto & word : a) {
        const uint64_t t = static_cast<uint64_t>(word) * f + carry;
        word = static_cast<uint32_t>(t);
        carry = t >> 32;
    }
    if (carry) a.push_back(static_cast<uint32_t>(carry));
}

inline int bitLength(const Number & a) { return a.empty() ? 0 : 32 * static_cast<int>(a.size()) - __builtin_clz(a.back()); }

inline bool bitAt(const Number & a, const int i) {
    const size_t word = static_cast<size_t>(i) / 32;
    return i >= 0 && word < a.size() && ((a[word] >> (i % 32)) & 1u);
}

inline bool notBelow(const Number & a, const Number & b) {
    if (a.size() != b.size()) return a.size() > b.size();
    for (size_t i = a.size(); i-- > 0;) {
        if (a[i] != b[i]) return a[i] > b[i];
    }
    return true;
}

inline void subtract(Number & a, const Number & b) {  // a >= b
    int64_t borrow = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        int64_t t = static_cast<int64_t>(a[i]) - (i < b.size() ? b[i] : 0) - borrow;
        borrow = t < 0 ? 1 : 0;
        if (t < 0) t += (1ll << 32);
        a[i] = static_cast<uint32_t>(t);
    }
    trim(a);
}

inline void doubleAndAdd(Number & a, const bool bit) {
    uint32_t carry = bit ? 1u : 0u;
    for (auto & word : a) {
        const uint32_t next = word >> 31;
        word = (word << 1) | carry;
        carry = next;
    }
    if (carry) a.push_back(carry);
}

}  // namespace big

// words [kPow10Words]: every 10^q, q = kMinPow10 .. kMaxPow10, as the 128 bits T = floor(10^q / 2^E) with T in [2^127, 2^128);
// exponents [kPow10Entries] (may be NULL): the E, which the kernels compute as pow10BinaryExponent(q)
inline void buildPow10Table(uint64_t * words, int * exponents) {
    for (int q = kMinPow10; q <= kMaxPow10; ++q) {
        big::Number power(1, 1u);
        for (int i = 0; i < (q < 0 ? -q : q); ++i) big::mulSmall(power, 10u);
        const int bits = big::bitLength(power);
        u128 T = 0;
        int E = 0;
        if (q >= 0) {  // the top 128 bits of 10^q
            for (int i = 0; i < 128; ++i) T = (T << 1) | (big::bitAt(power, bits - 1 - i) ? 1u : 0u);
            E = bits - 128;
        } else {  // floor(2^(127 + bits) / 10^-q) by long division: below 2^128, as 10^-q is above 2^(bits - 1)
            big::Number rest;
            for (int step = 0; step <= 127 + bits; ++step) {
                big::doubleAndAdd(rest, step == 0);
                const bool fits = big::notBelow(rest, power);
                if (fits) big::subtract(rest, power);
                T = (T << 1) | (fits ? 1u : 0u);
            }
            E = -(127 + bits);
        }
        words[2 * (q - kMinPow10)] = static_cast<uint64_t>(T >> 64);
        words[2 * (q - kMinPow10) + 1] = static_cast<uint64_t>(T);
        if (exponents) exponents[q - kMinPow10] = E;
    }
}

}  // namespace rpvg_number_text

#endif
