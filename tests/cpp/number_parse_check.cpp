// parseDouble and parseU64 of rpvg_amd/csrc/number_parse.hpp against glibc's strtod, bit for bit (tests/test_number_parse.py builds
// and runs this under the sanitizers with RPVG_NUMBER_TEXT_CHECKED defined): every "%.{p}g" text, p = 1 .. 17, of 10^7 random bit
// patterns; the 17-, 18- and 19-digit decimals below and above the middle of 10^6 random adjacent pairs of doubles (from glibc's exact
// "%.60Le" of the middle, which a long double holds exactly); exact ties; both ends of the range; the malformed forms.
// Prints "ok <compared> compared, <exact> by the exact comparison, <ties> ties among them".
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "number_parse.hpp"

using namespace rpvg_number_parse;

namespace {

std::vector<uint64_t> table(rpvg_number_text::kPow10Words);
std::atomic<uint64_t> failures{0};
thread_local uint64_t compared = 0, by_exact = 0;  // summed when a worker ends
std::atomic<uint64_t> all_compared{0}, all_by_exact{0};

void workerEnds() {
    all_compared.fetch_add(compared);
    all_by_exact.fetch_add(by_exact);
    compared = by_exact = 0;
}

uint64_t bitsOf(const double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

void fail(const char * what, const std::string & token) {
    if (failures.fetch_add(1) < 20) std::fprintf(stderr, "FAILED: %s: \"%s\"\n", what, token.c_str());
}

// the token against strtod; returns whether the exact comparison decided it
bool againstStrtod(const std::string & token) {
    const Parsed p = parseDouble(token.data(), token.size(), table.data());
    char * end = nullptr;
    const double ref = std::strtod(token.c_str(), &end);
    ++compared;
    if (*end != 0) {
        fail("strtod left bytes", token);
        return false;
    }
    if (std::isinf(ref) && token.find("inf") == std::string::npos) {
        if (p.status != kOverflow) fail("expected the overflow status", token);
    } else if (p.status != kOk || (bitsOf(p.value) != bitsOf(ref) && !(std::isnan(ref) && std::isnan(p.value) && std::signbit(ref) == std::signbit(p.value)))) {
        fail("differs from strtod", token);
    }
    if (p.exact) ++by_exact;
    return p.exact;
}

void expectValue(const std::string & token, const double value) {
    againstStrtod(token);
    const Parsed p = parseDouble(token.data(), token.size(), table.data());
    if (p.status != kOk || bitsOf(p.value) != bitsOf(value)) fail("not the expected double", token);
}

void expectStatus(const std::string & token, const int status) {
    const Parsed p = parseDouble(token.data(), token.size(), table.data());
    ++compared;
    if (p.status != status) fail("not the expected status", token);
}

struct Random {
    uint64_t s;
    uint64_t next() {  // splitmix64
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
};

double fromBits(const uint64_t b) {
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
}

void randomPatterns(const uint64_t seed, const uint64_t count) {
    Random rng{seed};
    char text[64];
    for (uint64_t i = 0; i < count; ++i) {
        uint64_t bits = rng.next();
        if (i % 16 == 0) bits &= ~(0x7ffull << 52);  // a subnormal
        const double v = fromBits(bits);
        for (int p = 1; p <= 17; ++p) {
            std::snprintf(text, sizeof(text), "%.*g", p, v);
            againstStrtod(text);
        }
    }
    workerEnds();
}

// the D-digit decimals below and above the middle of a and its successor
void midpointBrackets(const uint64_t seed, const uint64_t count) {
    Random rng{seed};
    char text[128];
    for (uint64_t i = 0; i < count; ++i) {
        uint64_t bits = rng.next() & ~(1ull << 63);
        if (i % 16 == 0) bits &= ~(0x7ffull << 52);
        if (((bits >> 52) & 0x7ff) == 0x7ff || bits + 1 == (0x7ffull << 52)) continue;
        const double a = fromBits(bits), b = fromBits(bits + 1);
        const long double mid = static_cast<long double>(a) + (static_cast<long double>(b) - static_cast<long double>(a)) / 2;
        std::snprintf(text, sizeof(text), "%.60Le", mid);  // d.ddd...e+-XXXX, exact but for the 61st digit
        std::string digits(1, text[0]);
        digits.append(text + 2, 60);
        const int exponent = std::atoi(std::strchr(text, 'e') + 1);
        for (int D = 17; D <= 19; ++D) {
            const std::string rest = digits.substr(D);
            if (rest.find_first_not_of('0') == std::string::npos || rest.find_first_not_of('9') == std::string::npos) continue;  // (a tie, or a carry the print may have made)
            const unsigned long long w = std::strtoull(digits.substr(0, D).c_str(), nullptr, 10);
            if (w + 1 >= 10000000000000000000ull) continue;
            const std::string below = std::to_string(w) + "e" + std::to_string(exponent - (D - 1));
            const std::string above = std::to_string(w + 1) + "e" + std::to_string(exponent - (D - 1));
            expectValue(below, a);
            expectValue(above, b);
        }
    }
    workerEnds();
}

}  // namespace

int main(int argc, char ** argv) {
    const uint64_t patterns = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000;  // (a smaller number for a quick look)
    rpvg_number_text::buildPow10Table(table.data(), nullptr);

    // parseU64 at every digit count
    for (int n = 1; n <= 21; ++n) {
        const std::string token(static_cast<size_t>(n), '9');
        uint64_t value = 1;
        const int status = parseU64(token.data(), token.size(), &value);
        if (n <= 19 ? (status != kOk || value != std::strtoull(token.c_str(), nullptr, 10)) : status != kTooLong) fail("parseU64", token);
    }
    for (const char * bad : {"", "+1", "-1", "1 ", " 1", "12a", "0x10", "1.0", "1e3"}) {
        uint64_t value = 0;
        if (parseU64(bad, std::strlen(bad), &value) != kMalformed) fail("parseU64 took a malformed token", bad);
    }
    {
        uint64_t value = 0;
        if (parseU64("0000000000000000042", 19, &value) != kOk || value != 42) fail("parseU64", "0000000000000000042");
        if (parseU64("4294967296", 10, &value) != kOk || value != 4294967296ull) fail("parseU64", "4294967296");
    }

    // exact ties, which the exact comparison must decide
    uint64_t ties = 0;
    const auto tie = [&](const std::string & token, const double value) {
        const Parsed p = parseDouble(token.data(), token.size(), table.data());
        if (!p.exact) fail("a tie that the product decided", token);
        expectValue(token, value);
        ++ties;
    };
    tie("9007199254740993", 9007199254740992.0);
    tie("9007199254740995", 9007199254740996.0);
    tie("4611686018427388416", 4611686018427387904.0);
    for (uint64_t j = 0; j < 100000; ++j) {  // the odd integers above 2^53: half way between two doubles of spacing 2
        const uint64_t x = (1ull << 53) + 1 + 2 * j;
        tie(std::to_string(x), static_cast<double>((x & 2) ? x + 1 : x - 1));
    }
    for (uint64_t j = 0; j < 100000; ++j) {  // 19 digits: spacing 1024 above 2^62
        const uint64_t x = (1ull << 62) + 512 + 1024 * j;
        tie(std::to_string(x), static_cast<double>((j & 1) ? x + 512 : x - 512));
    }

    // the large end
    expectValue("1.7976931348623158e308", 1.7976931348623157e308);
    expectStatus("1.7976931348623159e308", kOverflow);
    expectStatus("1e309", kOverflow);
    expectStatus("-1e400", kOverflow);
    expectStatus("9999999999999999999e308", kOverflow);
    expectStatus("1e99999999999999999999", kOverflow);
    expectValue("179769313486231570e291", 1.7976931348623157e308);
    // the small end
    expectValue("2.4703282292062327e-324", 0.0);
    expectValue("2.4703282292062328e-324", 4.9406564584124654e-324);
    expectValue("4.9406564584124654e-324", 4.9406564584124654e-324);
    expectValue("2.2250738585072011e-308", 2.2250738585072009e-308);
    expectValue("2.2250738585072014e-308", 2.2250738585072014e-308);
    expectValue("2470328229206232720e-342", 0.0);
    expectValue("2470328229206232721e-342", 4.9406564584124654e-324);
    expectValue("9999999999999999999e-343", 0.0);
    expectValue("9999999999999999999e-342", 4.9406564584124654e-324 * 2);
    expectValue("1e-400", 0.0);
    expectValue("-1e-400", -0.0);
    expectValue("1e-99999999999999999999", 0.0);
    // forms
    expectValue("-0", -0.0);
    expectValue("0.000", 0.0);
    expectValue("0e999", 0.0);
    expectValue("1e23", 1e23);
    expectValue("00012.5", 12.5);
    expectValue("5E-1", 0.5);
    expectValue("1.", 1.0);
    expectValue(".5", 0.5);
    expectValue("1e+2", 100.0);
    againstStrtod("0.00000000000000000000000000001234567890123456789");
    expectValue("inf", HUGE_VAL);
    expectValue("-inf", -HUGE_VAL);
    againstStrtod("nan");
    againstStrtod("-nan");
    expectStatus("12345678901234567890", kTooLong);
    expectStatus("1.2345678901234567890", kTooLong);
    expectStatus("1000000000000000000000", kTooLong);
    expectStatus("0.12345678901234567891e5", kTooLong);
    for (const char * bad : {"", "-", "+1", "+inf", "0x1p3", "0x10", "1.5abc", "1.5 ", " 1.5", "1 5", "1e", "1e+", "1e-", "e5", ".", "-.", ".e5", "1..2", "1.2.3", "1e5.0", "1e5e5", "Inf", "INF", "NaN",
                             "infinity", "nan(1)", "--1", "1-", "1,5", "1\t", "in", "na", "1f", "1d5"}) {
        expectStatus(bad, kMalformed);
    }

    const unsigned workers = 16;
    {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < workers; ++t) pool.emplace_back(randomPatterns, 1000 + t, patterns / workers + 1);
        for (auto & th : pool) th.join();
    }
    {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < workers; ++t) pool.emplace_back(midpointBrackets, 5000 + t, patterns / 9 / workers + 1);
        for (auto & th : pool) th.join();
    }

    workerEnds();
    if (failures.load()) {
        std::printf("FAILED %llu\n", static_cast<unsigned long long>(failures.load()));
        return 1;
    }
    std::printf("ok %llu compared, %llu by the exact comparison, %llu ties among them\n", static_cast<unsigned long long>(all_compared.load()),
                static_cast<unsigned long long>(all_by_exact.load()), static_cast<unsigned long long>(ties));
    return 0;
}
