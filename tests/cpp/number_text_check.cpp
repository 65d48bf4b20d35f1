// formatG and formatU32 of rpvg_amd/csrc/number_text.hpp against glibc's snprintf, byte for byte and length for length; the table of
// powers of ten against long double.  Prints the first mismatch as bit pattern, precision and both texts; "ok" and the counts otherwise.
// Built with -fsanitize=address,undefined by tests/test_number_text.py.
#define RPVG_NUMBER_TEXT_CHECKED 1
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "number_text.hpp"

using namespace rpvg_number_text;

namespace {

std::vector<uint64_t> table(kPow10Words);
uint64_t compared = 0, exact_cells = 0, odd_ties = 0, even_ties = 0;

double fromBits(const uint64_t bits) {
    double v;
    std::memcpy(&v, &bits, sizeof(v));
    return v;
}

// splitmix64
uint64_t state = 0x243f6a8885a308d3ull;
uint64_t nextWord() {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

void check(const double v, const int precision) {
    char want[64], got[64];
    const int want_length = std::snprintf(want, sizeof(want), "%.*g", precision, v);
    std::memset(got, '#', sizeof(got));
    const Decimal d = decompose(v, precision, table.data());
    const int length_alone = textOf<false>(d, precision, nullptr);
    const int got_length = formatG(v, precision, got + 8, table.data());
    ++compared;
    exact_cells += d.exact;
    odd_ties += d.tie && d.rounded_up;   // a tie goes up from odd digits alone
    even_ties += d.tie && !d.rounded_up;
    bool intact = true;
    for (int i = 0; i < 8; ++i) intact = intact && got[i] == '#' && got[8 + kMaxCellBytes + i] == '#';
    if (got_length != want_length || length_alone != want_length || got_length > kMaxCellBytes || std::memcmp(got + 8, want, want_length) != 0 ||
        got[8 + got_length] != '#' || !intact) {
        std::printf("mismatch: bits %016" PRIx64 " precision %d: glibc \"%s\" (%d), formatG \"%.*s\" (%d, length alone %d)\n", bitsOf(v), precision, want,
                    want_length, got_length > 0 && got_length < 40 ? got_length : 0, got + 8, got_length, length_alone);
        std::exit(1);
    }
}

void checkWithNeighbours(const double v, const int precision) {
    check(v, precision);
    check(std::nextafter(v, INFINITY), precision);
    check(std::nextafter(v, -INFINITY), precision);
    check(-v, precision);
}

void require(const bool condition, const char * what) {
    if (!condition) {
        std::printf("failed: %s\n", what);
        std::exit(1);
    }
}

void checkTable() {
    std::vector<int> exponents(kPow10Entries);
    buildPow10Table(table.data(), exponents.data());
    for (int q = kMinPow10; q <= kMaxPow10; ++q) {
        const int i = q - kMinPow10;
        require(exponents[i] == pow10BinaryExponent(q), "pow10BinaryExponent is the table's exponent");
        require((table[2 * i] >> 63) == 1, "a table entry is normalised");
        // the high word against long double (64 bits of significand, powl good to a few units of them)
        const long double high = std::ldexp(powl(10.0L, static_cast<long double>(q)), -exponents[i] - 64);
        const long double difference = high - static_cast<long double>(table[2 * i]);
        if (!(difference > -16.0L && difference < 16.0L)) {
            std::printf("table entry 10^%d: high word %016" PRIx64 " is %Lg away from long double\n", q, table[2 * i], difference);
            std::exit(1);
        }
    }
    // the exact entries: 10^q below 2^128 is its own top bits
    for (int q = 0; q <= 38; ++q) {
        u128 power = 1;
        for (int i = 0; i < q; ++i) power *= 10u;
        while (!(power >> 127)) power <<= 1;
        require(table[2 * (q - kMinPow10)] == static_cast<uint64_t>(power >> 64) && table[2 * (q - kMinPow10) + 1] == static_cast<uint64_t>(power), "an exact power of ten");
    }
    // a second construction of the negative powers: T 10^n <= 2^(127 + bits) < (T + 1) 10^n
    for (int q = kMinPow10; q < 0; ++q) {
        const int i = q - kMinPow10;
        big::Number low = {static_cast<uint32_t>(table[2 * i + 1]), static_cast<uint32_t>(table[2 * i + 1] >> 32), static_cast<uint32_t>(table[2 * i]),
                           static_cast<uint32_t>(table[2 * i] >> 32)};
        big::Number above = low, power(1, 1u);
        for (int n = 0; n < -q; ++n) {
            big::mulSmall(low, 10u);
            big::mulSmall(power, 10u);
        }
        above = low;
        {  // above = (T + 1) 10^n = low + 10^n
            uint64_t carry = 0;
            for (size_t w = 0; w < above.size() || carry; ++w) {
                if (w == above.size()) above.push_back(0);
                const uint64_t t = static_cast<uint64_t>(above[w]) + (w < power.size() ? power[w] : 0) + carry;
                above[w] = static_cast<uint32_t>(t);
                carry = t >> 32;
            }
        }
        big::Number two(1, 1u);
        for (int b = 0; b < -exponents[i]; ++b) big::doubleAndAdd(two, false);
        require(big::notBelow(two, low) && !big::notBelow(two, above), "a negative power of ten is the floor of the quotient");
    }
    for (int e = -1200; e <= 1200; ++e) {
        require(floorLog10Pow2(e) == static_cast<int>(std::floor(static_cast<long double>(e) * log10l(2.0L))), "floorLog10Pow2");
    }
    for (int q = -400; q <= 400; ++q) {
        require(floorLog2Pow10(q) == static_cast<int>(std::floor(static_cast<long double>(q) * log2l(10.0L))), "floorLog2Pow10");
    }
}

void expect(const double v, const int precision, const char * text) {
    char got[32];
    const int n = formatG(v, precision, got, table.data());
    if (std::string(got, n) != text) {
        std::printf("expected \"%s\" for bits %016" PRIx64 " at precision %d, formatG gave \"%.*s\"\n", text, bitsOf(v), precision, n, got);
        std::exit(1);
    }
    check(v, precision);
}

void checkU32(const uint32_t x) {
    char want[32], got[32];
    const int want_length = std::snprintf(want, sizeof(want), "%u", x);
    std::memset(got, '#', sizeof(got));
    const int got_length = formatU32(x, got);
    if (got_length != want_length || std::memcmp(got, want, want_length) != 0 || got[got_length] != '#') {
        std::printf("mismatch: formatU32(%u) gave \"%.*s\"\n", x, got_length, got);
        std::exit(1);
    }
}

}  // namespace

int main(int argc, char ** argv) {
    // the numbers of random patterns; the arguments scale them down for a quick look, the test runs the defaults
    const uint64_t random_at_8 = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
    const uint64_t random_elsewhere = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1000000ull;
    const int tie_strings = argc > 3 ? std::atoi(argv[3]) : 2000;
    checkTable();

    // the contract's examples
    expect(123456785.0, 8, "1.2345678e+08");
    expect(123456795.0, 8, "1.234568e+08");
    expect(99999999.5, 8, "1e+08");
    expect(0.0000999999995, 8, "9.9999999e-05");                      // (the double nearest that literal lies below the tie ...
    expect(std::nextafter(0.0000999999995, 1.0), 8, "0.0001");        // ... and its upper neighbour above it: the carry moves the notation)
    expect(1e-5, 8, "1e-05");
    expect(fromBits(2024), 8, "9.9998887e-321");
    expect(0.0, 8, "0");
    expect(-0.0, 8, "-0");
    expect(INFINITY, 8, "inf");
    expect(-INFINITY, 8, "-inf");
    expect(fromBits(0x7ff8000000000000ull), 8, "nan");
    expect(fromBits(0xfff8000000000000ull), 8, "-nan");
    expect(1.99999995, 8, "2");
    expect(9.9999999e+99, 8, "9.9999999e+99");
    expect(9.99999995e+99, 8, "1e+100");
    expect(0.00099999999, 8, "0.00099999999");
    expect(0.000999999995, 8, "0.001");
    expect(-1.2345678901234567e-308, 17, "-1.2345678901234567e-308");
    expect(-1.2345678e-308, 8, "-1.2345678e-308");

    for (int precision = kMinPrecision; precision <= kMaxPrecision; ++precision) {
        const double specials[] = {0.0, -0.0, INFINITY, -INFINITY, fromBits(0x7ff8000000000000ull), fromBits(0xfff8000000000000ull),
                                   fromBits(0x7ff0000000000001ull), fromBits(0xffffffffffffffffull), fromBits(1), fromBits(0x000fffffffffffffull),
                                   DBL_MIN, DBL_MAX, -DBL_MAX, -DBL_MIN, -fromBits(1)};
        for (const double v : specials) check(v, precision);
        for (int e = -1074; e <= 1023; ++e) checkWithNeighbours(std::ldexp(1.0, e), precision);
        for (int k = -323; k <= 308; ++k) {
            char text[16];
            std::snprintf(text, sizeof(text), "1e%d", k);
            checkWithNeighbours(std::strtod(text, nullptr), precision);
        }
        // the notation boundary from both sides at X = -5, -4, precision - 1, precision, and the carries across it
        for (const int X : {-5, -4, precision - 1, precision}) {
            char text[64];
            std::snprintf(text, sizeof(text), "1e%d", X);
            checkWithNeighbours(std::strtod(text, nullptr), precision);
            const std::string nines(static_cast<size_t>(precision), '9');
            for (const char * behind : {"", "4", "5", "49999999999999999999", "50000000000000000001", "9"}) {
                std::snprintf(text, sizeof(text), "%c.%s%se%d", nines[0], nines.c_str() + 1, behind, X - 1);
                checkWithNeighbours(std::strtod(text, nullptr), precision);
                std::snprintf(text, sizeof(text), "%c.%s%se%d", nines[0], nines.c_str() + 1, behind, X);
                checkWithNeighbours(std::strtod(text, nullptr), precision);
            }
        }
    }

    // the ties and near-ties: (D + 1/2) 10^q for random strings D of `precision` digits and every q in range
    for (const int precision : {8, 17}) {
        const uint64_t low = tenTo(precision - 1);
        for (int i = 0; i < tie_strings; ++i) {
            const uint64_t D = low + nextWord() % (9 * low);
            for (int q = -324 - precision; q <= 309 - precision; ++q) {
                char text[64];
                std::snprintf(text, sizeof(text), "%" PRIu64 "5e%d", D, q - 1);
                const double v = std::strtod(text, nullptr);
                if (v == 0.0 || std::isinf(v)) continue;
                check(v, precision);
                check(std::nextafter(v, INFINITY), precision);
                check(std::nextafter(v, -INFINITY), precision);
            }
        }
    }
    for (uint64_t n = 10000000; n < 10000064; ++n) check(static_cast<double>(n) + 0.5, 8);
    require(odd_ties > 0 && even_ties > 0, "exact ties with odd and with even digits were met");
    const uint64_t exact_before_random = exact_cells;

    for (uint64_t i = 0; i < random_at_8; ++i) check(fromBits(nextWord()), 8);
    for (const int precision : {1, 6, 17}) {
        for (uint64_t i = 0; i < random_elsewhere; ++i) check(fromBits(nextWord()), precision);
    }

    checkU32(0);
    checkU32(9);
    checkU32(10);
    checkU32(UINT32_MAX);
    checkU32(UINT32_MAX - 1);
    for (uint64_t power = 1; power <= 1000000000ull; power *= 10) {
        checkU32(static_cast<uint32_t>(power - 1));
        checkU32(static_cast<uint32_t>(power));
        checkU32(static_cast<uint32_t>(power + 1));
    }

    std::printf("ok %" PRIu64 " compared, %" PRIu64 " by the exact comparison (%" PRIu64 " before the random patterns), ties: %" PRIu64 " from odd digits, %" PRIu64 " from even\n",
                compared, exact_cells, exact_before_random, odd_ties, even_ties);
    return 0;
}
