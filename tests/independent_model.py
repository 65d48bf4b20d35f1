"""Plain-Python model of what rpvg_hip_nested_independent_subset_em (rpvg_amd/csrc/subset_independent.hip) does between the
posteriors and the EM: std::mt19937 as the standard defines it, libstdc++'s generate_canonical<double, 53> and
std::discrete_distribution (bits/random.tcc, GCC 11), the draws of sampleGroupPathIndices, the samples of a cluster as sorted path
lists, and the weight of a subset as a chain of additions (rpvg_amd/host/path_abundance_estimator.cpp, the independent branch of
estimateClusters).  Python floats are IEEE doubles: every sum, quotient and comparison is the host's.  Test-only."""
import bisect
import math

from tests import nested_full_model

N, M_SHIFT = 624, 397


class Mt19937:
    """std::mt19937(seed): 32-bit Mersenne twister ([rand.predef]); its 10 000th output from the default seed 5489 is 4123659995."""

    def __init__(self, seed=5489):
        x = [seed & 0xFFFFFFFF]
        for i in range(1, N):
            x.append((1812433253 * (x[-1] ^ (x[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.x, self.p = x, N
        self.taken = 0
        self.window = list(x)  # the 624 state words before the next output: regenerating from them gives it

    def _twist(self):
        x = self.x
        for k in range(N):
            y = (x[k] & 0x80000000) | (x[(k + 1) % N] & 0x7FFFFFFF)
            x[k] = x[(k + M_SHIFT) % N] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.p = 0

    def __call__(self):
        if self.p >= N:
            self._twist()
        y = self.x[self.p]
        self.p += 1
        self.taken += 1
        self.window.append(y)
        del self.window[0]
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y

    def copy(self):
        other = Mt19937.__new__(Mt19937)
        other.x, other.p, other.taken, other.window = list(self.x), self.p, self.taken, list(self.window)
        return other

    def next_words(self, n=N):
        """The next n outputs; the generator stays where it is."""
        ahead = self.copy()
        return [ahead() for _ in range(n)]

    def discard(self, n):
        for _ in range(n):
            self()

    def state_before_next(self):
        """The 624 state words whose regeneration gives the next output: the untempered last 624 outputs (the recurrence is a
        sliding window over the stream)."""
        return list(self.window)


def canonical(rng):
    """std::generate_canonical<double, 53>(std::mt19937): two words, the first one the low part."""
    total = float(rng())
    total += float(rng()) * 4294967296.0
    ret = total / 18446744073709551616.0
    return 0.9999999999999999 if ret >= 1.0 else ret


def partial_sums(weights):
    """std::discrete_distribution's construction: None for fewer than two weights."""
    if len(weights) < 2:
        return None
    total = 0.0
    for w in weights:
        total += float(w)
    cp, run = [], 0.0
    for w in weights:
        run += float(w) / total
        cp.append(run)
    cp[-1] = 1.0
    return cp


def draw_sets(weights, samples, rng):
    """`samples` set indices from the distribution over `weights`, draw for draw; a distribution of one set draws nothing."""
    cp = partial_sums(weights)
    if cp is None:
        return [0] * samples
    return [bisect.bisect_left(cp, canonical(rng)) for _ in range(samples)]


def num_samples(min_hap_prob):
    return int(math.floor(1 / min_hap_prob))


def weight_of(count, samples):
    w, step = 0.0, 1 / float(samples)
    for _ in range(count):
        w += step
    return w


def cluster(transcripts, min_hap_prob, rng):
    """transcripts: [(paths of the columns, member tuples of the sets, posteriors)] in findPathGroups order.  Returns
    (draws[slot][transcript], [(sorted path list, weight, sample count)] in lexicographic order of the lists).  The generator is
    moved as the host's is."""
    S = num_samples(min_hap_prob)
    draws = [[0] * len(transcripts) for _ in range(S)]
    lists = [[] for _ in range(S)]
    for t, (paths, members, posteriors) in enumerate(transcripts):
        for slot, index in enumerate(draw_sets(posteriors, S, rng)):
            draws[slot][t] = index
            lists[slot].extend(paths[c] for c in sorted(members[index]))
    counts = {}
    for sample in lists:
        key = tuple(sorted(sample))
        counts[key] = counts.get(key, 0) + 1
    out = []
    for key in sorted(counts):
        w = weight_of(counts[key], S)
        if w < min_hap_prob:
            continue
        out.append((list(key), w, counts[key]))
    return draws, out


merge = nested_full_model.merge
all_sets = nested_full_model.all_sets
