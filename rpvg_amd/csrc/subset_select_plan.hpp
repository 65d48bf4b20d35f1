// The index logic of the subset selection (subset_em.hip, selectSubsetsOfMatrix) as plain functions: the selected diplotypes
// grouped by (hash, length) of their path lists with one sort of their indices, every group confirmed by list comparisons, the
// first member in pair order as its leader, a leader's members in ascending pair order, and the order of the retained lists —
// plain C++17, so that a CPU test runs the same steps on host arrays against a quadratic model
// (tests/cpp/subset_select_check.cpp).  The kernels call these on arrays in LDS; nothing here knows a HIP type.
//
// The steps, each over all positions p (or pairs of a network stage) with a barrier between two of them:
//   sort      `sorted` = the selected 0 .. n - 1 in the order of groupBefore: (hash, length, index) ascending, so that the
//             candidates of a group lie in one run and in pair order (sortStagePairs .. compareExchange, padding last)
//   heads     head[p] = isRunHead(p) ? p : 0, then scanStep with d = 1, 2, 4 .. < n: the position at which p's run begins
//   leaders   leader[sorted[p]] = leaderAt(p): the first member of the run with the identical list (equal hashes need not
//             mean equal lists: the comparison decides), itself when there is none in front of it
//   weights   a leader adds up memberSum(p): its own members only, in ascending pair order
//   rank      the retained leaders in the order of rankBefore: a 64-bit key of the leading elements of the list
//             (keyElementBits, keyElements, keyAppend), the list comparison only between equal keys; the lists of distinct
//             leaders differ, so the order is strict and total and any correct sort gives the same slots
#ifndef RPVG_SUBSET_SELECT_PLAN_HPP
#define RPVG_SUBSET_SELECT_PLAN_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define RPVG_SELECT_FN __host__ __device__ inline
#else
#define RPVG_SELECT_FN inline
#endif

namespace rpvg_select {

constexpr uint32_t kPadding = 0xffffffffu;  // an index behind every selected one: sorts last in both orders

// slots of the bitonic network over n indices: the smallest power of two >= n (1 for n = 0)
RPVG_SELECT_FN uint32_t paddedSize(const uint32_t n) {
    uint32_t padded = 1;
    while (padded < n) padded <<= 1;
    return padded;
}

// Stage (size, stride) of the network over `padded` slots, size = 2, 4 .. padded, stride = size / 2 .. 1, has padded / 2
// disjoint pairs: pair p is (low, low | stride) and ends ascending where bit `size` of low is clear.
RPVG_SELECT_FN uint32_t sortStagePairs(const uint32_t padded) { return padded >> 1; }
RPVG_SELECT_FN uint32_t pairLow(const uint32_t p, const uint32_t stride) { return ((p & ~(stride - 1)) << 1) | (p & (stride - 1)); }
RPVG_SELECT_FN bool pairAscending(const uint32_t low, const uint32_t size) { return (low & size) == 0; }
// pair p of stage (size, stride) on the index array; before(x, y): x sorts strictly before y (padding included)
template <class Before>
RPVG_SELECT_FN void compareExchange(uint32_t * order, const uint32_t p, const uint32_t size, const uint32_t stride, Before before) {
    const uint32_t low = pairLow(p, stride), high = low | stride;
    const uint32_t x = order[low], y = order[high];
    if (before(y, x) == pairAscending(low, size)) {
        order[low] = y;
        order[high] = x;
    }
}

// ---- groups ------------------------------------------------------------------------------------------------------------------
RPVG_SELECT_FN bool groupBefore(const unsigned long long * hash, const uint32_t * length, const uint32_t x, const uint32_t y) {
    if (x == kPadding || y == kPadding) return x != kPadding;
    if (hash[x] != hash[y]) return hash[x] < hash[y];
    if (length[x] != length[y]) return length[x] < length[y];
    return x < y;
}
RPVG_SELECT_FN bool isRunHead(const uint32_t * sorted, const unsigned long long * hash, const uint32_t * length, const uint32_t p) {
    if (p == 0) return true;
    const uint32_t s = sorted[p], t = sorted[p - 1];
    return hash[s] != hash[t] || length[s] != length[t];
}
// one round of the running maximum over head[]: what position p holds after the round with distance d
RPVG_SELECT_FN uint32_t scanStep(const uint32_t * head, const uint32_t p, const uint32_t d) {
    const uint32_t own = head[p];
    if (p < d) return own;
    const uint32_t other = head[p - d];
    return other > own ? other : own;
}
// the leader of the selected diplotype at position p; same_list(t, s): the lists of t and s are identical
template <class SameList>
RPVG_SELECT_FN uint32_t leaderAt(const uint32_t * sorted, const uint32_t * head, const uint32_t p, SameList same_list) {
    const uint32_t s = sorted[p];
    for (uint32_t q = head[p]; q < p; ++q) {
        if (same_list(sorted[q], s)) return sorted[q];
    }
    return s;
}
// the sum over the members of the leader at position p, in ascending pair order (the run is in pair order); value by index
template <class Value>
RPVG_SELECT_FN Value memberSum(const uint32_t * sorted, const uint32_t * head, const uint32_t * leader, const Value * value,
                               const uint32_t p, const uint32_t n) {
    const uint32_t s = sorted[p], h = head[p];
    Value sum = 0;
    for (uint32_t q = p; q < n && head[q] == h; ++q) {
        const uint32_t t = sorted[q];
        if (leader[t] == s) sum += value[t];
    }
    return sum;
}

// ---- rank of the retained lists ----------------------------------------------------------------------------------------------
// The leading elements of a list as one word: keyElements(bits) fields of `bits` bits, the first element in the highest field, an
// element e as e + 1 and a missing one as 0, where `bits` holds the largest path of the matrix's lists plus one.  The word never
// decreases in the lexicographic order of the lists (a missing element is the smallest there is), so different keys decide and
// equal keys leave it to the lists; a list of at most keyElements(bits) elements is told apart by its key alone.  (40 paths in a
// cluster: 6 bits, ten elements.)
RPVG_SELECT_FN uint32_t keyElementBits(const uint32_t max_path) {
    uint32_t bits = 1;
    while ((max_path + 1ull) >> bits) ++bits;
    return bits;  // 1 .. 33
}
RPVG_SELECT_FN uint32_t keyElements(const uint32_t bits) { return 64 / bits; }  // 1 .. 64
// the key with one more field behind it: element e, or a missing one
RPVG_SELECT_FN unsigned long long keyAppend(const unsigned long long key, const uint32_t bits, const bool present, const uint32_t e) {
    return (key << bits) | (present ? e + 1ull : 0ull);
}
// list_before(x, y): the list of x is lexicographically smaller than that of y
template <class ListBefore>
RPVG_SELECT_FN bool rankBefore(const unsigned long long * key, const uint32_t x, const uint32_t y, ListBefore list_before) {
    if (x == kPadding || y == kPadding) return x != kPadding;
    if (key[x] != key[y]) return key[x] < key[y];
    return list_before(x, y);
}

}  // namespace rpvg_select

#endif
