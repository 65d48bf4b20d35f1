// The index logic of the subset selection (rpvg_amd/csrc/subset_select_plan.hpp) executed on host arrays the way the kernels
// execute it — the threads of a step one after the other, a step's results visible only to the next step — against a plain
// quadratic model: leaders, a leader's members in pair order (through sums whose order shows in the last bit), and the rank of
// the retained lists.  Plain C++17; built with -fsanitize=address,undefined.  Prints "ok".
#include "subset_select_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

using namespace rpvg_select;
typedef std::vector<uint32_t> List;
typedef std::function<unsigned long long(const List &)> HashFn;

static unsigned long long fnv(const List & list) {
    unsigned long long h = 1469598103934665603ull;
    for (const uint32_t path : list) h = (h ^ path) * 1099511628211ull;
    return h;
}

struct Result {
    std::vector<uint32_t> leader;   // per selected
    std::vector<double> weight;     // per selected: the sum over its members where it leads, 0 elsewhere
    std::vector<uint32_t> ranked;   // the retained leaders in the order of their lists
};

// the quadratic model: what selectPathSubsetIndices and an ordered map of the lists give
static Result model(const std::vector<List> & lists, const std::vector<double> & value, const std::vector<bool> & retained_if_leader) {
    const uint32_t n = static_cast<uint32_t>(lists.size());
    Result r;
    r.leader.resize(n);
    r.weight.assign(n, 0.0);
    for (uint32_t s = 0; s < n; ++s) {
        r.leader[s] = s;
        for (uint32_t t = 0; t < s; ++t) {
            if (lists[t] == lists[s]) {
                r.leader[s] = t;
                break;
            }
        }
    }
    for (uint32_t s = 0; s < n; ++s) {
        if (r.leader[s] != s) continue;
        double w = 0;
        for (uint32_t t = s; t < n; ++t) {
            if (r.leader[t] == s) w += value[t];
        }
        r.weight[s] = w;
        if (retained_if_leader[s]) r.ranked.push_back(s);
    }
    std::sort(r.ranked.begin(), r.ranked.end(), [&](const uint32_t x, const uint32_t y) { return lists[x] < lists[y]; });
    return r;
}

static uint64_t g_list_comparisons = 0;

// the key of a list as the kernel builds it: keyElements(bits) fields, the elements the list does not have as missing
static unsigned long long keyOf(const List & list, const uint32_t bits) {
    unsigned long long key = 0;
    for (uint32_t i = 0; i < keyElements(bits); ++i) key = keyAppend(key, bits, i < list.size(), i < list.size() ? list[i] : 12345u);
    return key;
}
static uint32_t maxPath(const std::vector<List> & lists) {
    uint32_t max_path = 0;
    for (const List & list : lists) {
        for (const uint32_t path : list) max_path = std::max(max_path, path);
    }
    return max_path;
}

// the network over `order`, stage by stage, pair by pair
template <class Before>
static void network(std::vector<uint32_t> & order, Before before) {
    const uint32_t padded = static_cast<uint32_t>(order.size());
    REQUIRE(padded >= 1 && (padded & (padded - 1)) == 0);
    for (uint32_t size = 2; size <= padded; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            std::vector<bool> touched(padded, false);
            for (uint32_t p = 0; p < sortStagePairs(padded); ++p) {
                const uint32_t low = pairLow(p, stride);
                REQUIRE((low & stride) == 0 && (low | stride) < padded && !touched[low] && !touched[low | stride]);  // the pairs of a stage are disjoint
                touched[low] = touched[low | stride] = true;
                compareExchange(order.data(), p, size, stride, before);
            }
        }
    }
}

// the steps of selectSubsetsOfMatrix behind the staging
static Result plan(const std::vector<List> & lists, const std::vector<double> & value, const std::vector<bool> & retained_if_leader, const HashFn & hash_of) {
    const uint32_t n = static_cast<uint32_t>(lists.size());
    std::vector<unsigned long long> hash(n + 1);  // (+ 1: data() of an empty vector may be null)
    std::vector<uint32_t> length(n + 1);
    for (uint32_t s = 0; s < n; ++s) {
        hash[s] = hash_of(lists[s]);
        length[s] = static_cast<uint32_t>(lists[s].size());
    }
    const uint32_t padded = paddedSize(n);
    REQUIRE(padded >= n && padded >= 1 && (padded & (padded - 1)) == 0 && (padded == 1 || padded / 2 < n));
    std::vector<uint32_t> sorted(padded, kPadding);
    for (uint32_t s = 0; s < n; ++s) sorted[s] = n - 1 - s;  // (any order going in)
    network(sorted, [&](const uint32_t x, const uint32_t y) { return groupBefore(hash.data(), length.data(), x, y); });
    for (uint32_t p = 0; p < padded; ++p) REQUIRE((p < n) == (sorted[p] != kPadding));
    for (uint32_t p = 1; p < n; ++p) REQUIRE(groupBefore(hash.data(), length.data(), sorted[p - 1], sorted[p]));
    std::vector<uint32_t> head(n + 1), next(n + 1);
    for (uint32_t p = 0; p < n; ++p) head[p] = isRunHead(sorted.data(), hash.data(), length.data(), p) ? p : 0u;
    for (uint32_t d = 1; d < n; d <<= 1) {
        for (uint32_t p = 0; p < n; ++p) next[p] = scanStep(head.data(), p, d);
        head = next;
    }
    for (uint32_t p = 0; p < n; ++p) {  // head[p]: the first position of p's run
        uint32_t h = p;
        while (h > 0 && hash[sorted[h - 1]] == hash[sorted[p]] && length[sorted[h - 1]] == length[sorted[p]]) --h;
        REQUIRE(head[p] == h);
    }
    Result r;
    r.leader.assign(n, kPadding);
    r.weight.assign(n, 0.0);
    for (uint32_t p = 0; p < n; ++p) {
        r.leader[sorted[p]] = leaderAt(sorted.data(), head.data(), p, [&](const uint32_t t, const uint32_t s) {
            REQUIRE(t < s && hash[t] == hash[s] && length[t] == length[s]);  // only candidates of the run, only earlier ones
            ++g_list_comparisons;
            return lists[t] == lists[s];
        });
    }
    std::vector<uint32_t> order;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t s = sorted[p];
        if (r.leader[s] != s) continue;
        r.weight[s] = memberSum(sorted.data(), head.data(), r.leader.data(), value.data(), p, n);
        if (retained_if_leader[s]) order.push_back(s);
    }
    const uint32_t n_ret = static_cast<uint32_t>(order.size());
    std::vector<unsigned long long> key(n + 1, 0);
    const uint32_t bits = keyElementBits(maxPath(lists));
    REQUIRE(bits >= 1 && bits <= 33 && keyElements(bits) >= 1 && keyElements(bits) * bits <= 64);
    for (const uint32_t s : order) key[s] = keyOf(lists[s], bits);
    order.resize(paddedSize(n_ret), kPadding);
    network(order, [&](const uint32_t x, const uint32_t y) {
        return rankBefore(key.data(), x, y, [&](const uint32_t u, const uint32_t v) {
            REQUIRE(key[u] == key[v]);  // the lists are compared between equal keys only
            ++g_list_comparisons;
            return lists[u] < lists[v];
        });
    });
    for (uint32_t i = n_ret; i < order.size(); ++i) REQUIRE(order[i] == kPadding);
    order.resize(n_ret);
    r.ranked = order;
    return r;
}

static void check(const std::vector<List> & lists, std::mt19937_64 & rng, const HashFn & hash_of = fnv) {
    const uint32_t n = static_cast<uint32_t>(lists.size());
    // values whose sum depends on the order of the additions in the last bits
    std::vector<double> value(n);
    std::uniform_real_distribution<double> mantissa(1.0, 2.0);
    std::uniform_int_distribution<int> exponent(-30, 0);
    for (double & v : value) v = std::ldexp(mantissa(rng), exponent(rng));
    std::vector<bool> retained(n);
    for (uint32_t s = 0; s < n; ++s) retained[s] = (rng() % 8) != 0;
    const Result want = model(lists, value, retained), got = plan(lists, value, retained, hash_of);
    REQUIRE(got.leader == want.leader);
    REQUIRE(got.weight == want.weight);  // equal to the bit: the members were added in pair order
    REQUIRE(got.ranked == want.ranked);
}

static List randomList(std::mt19937_64 & rng, const uint32_t max_length, const uint32_t alphabet) {
    List list(rng() % (max_length + 1));
    for (uint32_t & path : list) path = static_cast<uint32_t>(rng() % alphabet);
    std::sort(list.begin(), list.end());  // ascending with repetition, as a merged walk gives them
    return list;
}

int main() {
    std::mt19937_64 rng(20240607);
    // the network's pairs
    REQUIRE(paddedSize(0) == 1 && paddedSize(1) == 1 && paddedSize(2) == 2 && paddedSize(3) == 4 && paddedSize(1024) == 1024 && paddedSize(1025) == 2048);
    // the key never decreases along the order of the lists, at every width of its fields; lists that fit into it differ in it
    REQUIRE(keyElementBits(0) == 1 && keyElementBits(1) == 2 && keyElementBits(2) == 2 && keyElementBits(3) == 3 && keyElementBits(39) == 6 &&
            keyElementBits(62) == 6 && keyElementBits(63) == 7 && keyElementBits(0xfffffffeu) == 32 && keyElementBits(0xffffffffu) == 33);
    REQUIRE(keyElements(1) == 64 && keyElements(6) == 10 && keyElements(32) == 2 && keyElements(33) == 1);
    for (const uint32_t max_path : {0u, 1u, 2u, 3u, 6u, 7u, 39u, 1000u, 65534u, 65535u, 0x7fffffffu, 0xfffffffeu, 0xffffffffu}) {
        const uint32_t bits = keyElementBits(max_path);
        REQUIRE((max_path + 1ull) >> bits == 0 && (max_path + 1ull) >> (bits - 1) != 0);
        for (int round = 0; round < 4000; ++round) {
            List x = randomList(rng, 2 * keyElements(bits) < 12 ? 12 : 70, 3), y = randomList(rng, 2 * keyElements(bits) < 12 ? 12 : 70, 3);
            for (uint32_t & path : x) path = path == 2 ? max_path : std::min(path, max_path);
            for (uint32_t & path : y) path = path == 2 ? max_path : std::min(path, max_path);
            std::sort(x.begin(), x.end());
            std::sort(y.begin(), y.end());
            const unsigned long long kx = keyOf(x, bits), ky = keyOf(y, bits);
            if (x < y) REQUIRE(kx <= ky);
            if (kx < ky) REQUIRE(x < y);
            if (x.size() <= keyElements(bits) && y.size() <= keyElements(bits)) REQUIRE((kx == ky) == (x == y));
        }
    }
    // no selected diplotype, one, two
    check({}, rng);
    check({List{3, 4, 4}}, rng);
    check({List{}}, rng);
    check({List{3, 4}, List{3, 4}}, rng);
    check({List{3, 4}, List{3}}, rng);
    // random lists: every count around the sizes of the network, few and many identical lists
    for (const uint32_t n : {2u, 3u, 4u, 5u, 7u, 8u, 9u, 31u, 33u, 63u, 64u, 65u, 127u, 129u, 255u, 256u, 257u, 511u, 513u, 946u, 1023u, 1024u}) {
        for (const uint32_t alphabet : {2u, 5u, 1000u}) {
            for (const uint32_t max_length : {3u, 12u}) {
                std::vector<List> lists(n);
                for (List & list : lists) list = randomList(rng, max_length, alphabet);
                check(lists, rng);
            }
        }
    }
    // equal hashes with different lists: one hash for all, a hash of the length alone, a hash of the last element alone
    for (const uint32_t n : {6u, 64u, 200u}) {
        std::vector<List> lists(n);
        for (List & list : lists) list = randomList(rng, 4, 3);
        check(lists, rng, [](const List &) { return 42ull; });
        check(lists, rng, [](const List & list) { return static_cast<unsigned long long>(list.size()); });
        check(lists, rng, [](const List & list) { return list.empty() ? 7ull : static_cast<unsigned long long>(list.back()); });
    }
    // equal leading keys with a difference in the tail, and lists that are prefixes of others
    {
        std::vector<List> lists;
        for (uint32_t tail = 0; tail < 40; ++tail) {
            List list{5, 9};
            for (uint32_t i = 0; i < tail % 7; ++i) list.push_back(9 + i);
            list.push_back(20 + (tail * 13) % 11);
            lists.push_back(list);
        }
        for (uint32_t length = 0; length <= 12; ++length) lists.push_back(List(length, 5));  // every one a prefix of the next
        for (uint32_t length = 0; length <= 12; ++length) {
            List list;
            for (uint32_t i = 0; i < length; ++i) list.push_back(5 + i);
            lists.push_back(list);
        }
        lists.push_back(List{0});
        lists.push_back(List{0, 0});
        lists.push_back(List{0xffffffffu});
        lists.push_back(List{0xffffffffu, 0xffffffffu});
        lists.push_back(List{0xffffffffu, 0xffffffffu, 0});
        for (int round = 0; round < 20; ++round) {
            std::shuffle(lists.begin(), lists.end(), rng);
            check(lists, rng);
        }
    }
    // all selected diplotypes identical: one leader, every other compared with it once, no comparison in the rank
    for (const uint32_t n : {2u, 65u, 1024u}) {
        const uint64_t before = g_list_comparisons;
        check(std::vector<List>(n, List{1, 2, 2, 8}), rng);
        REQUIRE(g_list_comparisons - before == n - 1);
    }
    // all different in the first two elements: the lists are never walked
    {
        std::vector<List> lists;
        for (uint32_t i = 0; i < 300; ++i) lists.push_back(List{i / 20, i / 20 + i % 20, 1000, 1001});
        std::shuffle(lists.begin(), lists.end(), rng);
        const uint64_t before = g_list_comparisons;
        check(lists, rng);
        REQUIRE(g_list_comparisons == before);
    }
    std::printf("ok\n");
    return 0;
}
