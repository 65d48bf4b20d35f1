"""Plain-Python model of the estimates table (include/rpvg_table.h, rpvg_amd/csrc/estimates_table.hip): Python floats and loops,
restating the table's semantics line by line.

A batch is a list of clusters, each a dict:
    num_paths    N
    sets         [tuple of cluster-local paths ...]   PathClusterEstimates::path_group_sets
    posteriors   [float per set]
    abundances   [float per member in (set, member) order], or [] (`haplotypes`)
    noise_count  float
    eff          [float per path]                      PathInfo::effective_length

table(clusters, ploidy) returns the arrays of rpvg_estimates_table_view as numpy float64 arrays and its scalars as floats; every
sum is `acc = acc + x` from 0.0 in the stated order, every quotient one division.  with_tpm(table, denominator) adds the second step.
"""
import numpy as np


class InvalidEstimates(ValueError):
    def __init__(self, cluster, why):
        super().__init__(f"cluster {cluster}: {why}")
        self.cluster = cluster


def table(clusters, ploidy):
    haplotype_prob, read_count, transcript_count, member_tc, cluster_tc = [], [], [], [], []
    for k, c in enumerate(clusters):
        n = c["num_paths"]
        members = [p for s in c["sets"] for p in s]
        if any(p >= n for p in members):
            raise InvalidEstimates(k, "a member is not below the number of paths")
        if len(c["abundances"]) not in (0, len(members)):                       # one per member, or none
            raise InvalidEstimates(k, "the abundances are neither one per member nor none")
        has = len(c["abundances"]) > 0
        prob, count = [0.0] * n, [0.0] * n                                       # start from 0.0
        part = 0.0
        a = 0
        for s, post in zip(c["sets"], c["posteriors"]):                          # sets ascending
            for j, p in enumerate(s):                                            # member positions ascending
                if j == 0 or s[j] != s[j - 1]:                                   # the adjacent-duplicate rule, literally
                    prob[p] = prob[p] + post
                ab = c["abundances"][a] if has else None
                if has:
                    count[p] = count[p] + ab                                     # at every position (a homozygous path twice)
                e = c["eff"][p]
                if has and e > 0:
                    member_tc.append(ab / e)
                    part = part + ab / e                                         # clusterTranscriptCount: eff > 0 only
                else:
                    member_tc.append(0.0)
                a += 1
        haplotype_prob.extend(prob)
        read_count.extend(count)
        transcript_count.extend(count[p] / c["eff"][p] if c["eff"][p] > 0 else 0.0 for p in range(n))
        cluster_tc.append(part)
    total = noise_total = share_total = 0.0
    for k, c in enumerate(clusters):                                             # ascending cluster order
        total = total + cluster_tc[k]
        noise_total = noise_total + c["noise_count"]
        share_total = share_total + c["noise_count"] / float(ploidy)
    f = lambda x: np.asarray(x, dtype=np.float64)
    return dict(haplotype_prob=f(haplotype_prob), read_count=f(read_count), transcript_count=f(transcript_count),
                member_transcript_count=f(member_tc), cluster_transcript_count=f(cluster_tc), total_transcript_count=total,
                noise_count_total=noise_total, noise_count_share_total=share_total)


def with_tpm(t, denominator):
    """The second step: count / denominator * 1e6, the division first (numpy: 0 / 0 is NaN, x / 0 infinite, no exception)."""
    out = dict(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.float64(denominator)
        out["tpm"] = (t["transcript_count"] / d) * np.float64(1e6)
        out["member_tpm"] = (t["member_transcript_count"] / d) * np.float64(1e6)
    return out


def total_single_chain(clusters):
    """totalTranscriptCount (src/main.cpp:1029-1057): ONE running sum over all members of all clusters."""
    total, n = 0.0, 0
    for c in clusters:
        a = 0
        for s in c["sets"]:
            for p in s:
                if c["abundances"] and c["eff"][p] > 0:
                    total = total + c["abundances"][a] / c["eff"][p]
                    n += 1
                a += 1
    return total, n


def flatten(clusters):
    """The arrays of rpvg_estimates_flat by name (numpy, the ABI's types)."""
    set_off, member_off, members, posteriors, abund_off, abundances, noise, path_off, eff = [0], [0], [], [], [0], [], [], [0], []
    for c in clusters:
        for s, post in zip(c["sets"], c["posteriors"]):
            members.extend(s)
            member_off.append(len(members))
            posteriors.append(post)
        set_off.append(len(posteriors))
        abundances.extend(c["abundances"])
        abund_off.append(len(abundances))
        noise.append(c["noise_count"])
        assert len(c["eff"]) == c["num_paths"]
        eff.extend(c["eff"])
        path_off.append(len(eff))
    u64, u32, f64 = np.uint64, np.uint32, np.float64
    return dict(set_off=np.asarray(set_off, u64), member_off=np.asarray(member_off, u64), members=np.asarray(members, u32),
                posteriors=np.asarray(posteriors, f64), abund_off=np.asarray(abund_off, u64), abundances=np.asarray(abundances, f64),
                noise_count=np.asarray(noise, f64), cluster_path_off=np.asarray(path_off, u64), path_effective_length=np.asarray(eff, f64))


def from_estimates(batch, estimates):
    """Clusters of the model from a ClusterBatch and the ClusterEstimates of a run."""
    out = []
    for k, e in enumerate(estimates):
        p0, p1 = int(batch.cluster_path_off[k]), int(batch.cluster_path_off[k + 1])
        out.append(dict(num_paths=p1 - p0, sets=[tuple(int(p) for p in s) for s in e.path_group_sets], posteriors=[float(x) for x in e.posteriors],
                        abundances=[float(x) for x in e.abundances], noise_count=float(e.noise_count),
                        eff=[float(x) for x in batch.path_effective_length[p0:p1]]))
    return out


def route_of(limits, paths, members):
    """rpvg_amd/csrc/estimates_plan.hpp: 0 one wavefront, 1 one workgroup, 2 global memory."""
    if paths <= limits.wave_paths and members <= limits.wave_members:
        return 0
    if paths <= limits.lds_paths and members <= limits.lds_members:
        return 1
    return 2


def clusters_by_route(limits, clusters):
    out = [0, 0, 0]
    for c in clusters:
        out[route_of(limits, c["num_paths"], sum(len(s) for s in c["sets"]))] += 1
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------

def hand_case():
    """One cluster of three paths, sets {0,0} {0,1} {2} {1,0,1}, dyadic posteriors and abundances, path 1 with effective length 0:
    every expected value written out from the writer's lines (src/threaded_output_writer.cpp:346-432).
      haplotype_prob  path 0: {0,0} counts once 0.5, {0,1} 0.25, {1,0,1} position 1 (0 != 1) 0.0625           = 0.8125
                      path 1: {0,1} position 1 0.25, {1,0,1} positions 0 and 2 (unsorted: twice) 2 x 0.0625   = 0.375
                      path 2: {2} 0.125
      read_count      path 0: 1 + 2 + 4 + 0.25 = 7.25; path 1: 8 + 0.5 + 0.125 = 8.625; path 2: 16
      transcripts     path 0: 7.25 / 2 = 3.625; path 1: effective length 0 -> 0; path 2: 16 / 4 = 4
      members         1/2 2/2 4/2 0 16/4 0 0.25/2 0
      cluster         0.5 + 1 + 2 + 4 + 0.125 = 7.625 (the members of path 1 are left out)
    """
    cluster = dict(num_paths=3, sets=[(0, 0), (0, 1), (2,), (1, 0, 1)], posteriors=[0.5, 0.25, 0.125, 0.0625],
                   abundances=[1.0, 2.0, 4.0, 8.0, 16.0, 0.5, 0.25, 0.125], noise_count=3.0, eff=[2.0, 0.0, 4.0])
    expected = dict(haplotype_prob=[0.8125, 0.375, 0.125], read_count=[7.25, 8.625, 16.0], transcript_count=[3.625, 0.0, 4.0],
                    member_transcript_count=[0.5, 1.0, 2.0, 0.0, 4.0, 0.0, 0.125, 0.0], cluster_transcript_count=[7.625],
                    total_transcript_count=7.625, noise_count_total=3.0, noise_count_share_total=1.5)
    # with a denominator of 8: 3.625 / 8 * 1e6, 0, 4 / 8 * 1e6; members x / 8 * 1e6
    expected_tpm = dict(tpm=[453125.0, 0.0, 500000.0], member_tpm=[62500.0, 125000.0, 250000.0, 0.0, 500000.0, 0.0, 15625.0, 0.0])
    return [cluster], 2, expected, 8.0, expected_tpm


def sequential_sum(values):
    acc = 0.0
    for v in values:
        acc = acc + v
    return acc


def reversed_sum(values):
    return sequential_sum(list(values)[::-1])


def pairwise_sum(values):
    """A balanced tree: halves added separately, then together."""
    values = list(values)
    if len(values) == 1:
        return values[0]
    half = len(values) // 2
    return pairwise_sum(values[:half]) + pairwise_sum(values[half:])


def three_sums_differ(values):
    return len({sequential_sum(values), reversed_sum(values), pairwise_sum(values)}) == 3


def three_sum_cases(seed, n, size=4):
    """n lists of `size` values in (0, 1000) whose sequential, reversed and pairwise sums are three different doubles: the
    abundances (and, scaled, posteriors) of a path with `size` memberships."""
    assert size >= 3
    out, s = [], seed
    while len(out) < n:
        rng = np.random.default_rng(s)
        for _ in range(256):
            values = [float(x) for x in rng.uniform(0.001, 1000.0, size=size)]
            if three_sums_differ(values):
                out.append(values)
        s += 1
    return out[:n]


def order_cluster(values_list, num_paths, gap, rng, ploidy=2):
    """A cluster in which path i (i < len(values_list)) has the memberships values_list[i] as abundances, and values / 4096 as
    posteriors, `gap` sets of other paths between two of them (so that they lie in different chunks of 64 members), every set
    {path, filler} with the filler path above the cases' paths and different from the path."""
    cases = len(values_list)
    assert num_paths > cases + 1
    sets, posteriors, abundances = [], [], []
    rounds = max(len(v) for v in values_list)
    for r in range(rounds):
        for i, values in enumerate(values_list):
            if r < len(values):
                filler = cases + int(rng.integers(0, num_paths - cases))
                sets.append((i, filler))
                posteriors.append(values[r] / 4096.0)
                abundances.extend([values[r], float(rng.uniform(0.5, 50.0))])
        for _ in range(gap):
            a, b = (cases + int(x) for x in rng.integers(0, num_paths - cases, size=2))
            sets.append((a, b))
            posteriors.append(float(rng.uniform(0.0, 0.01)))
            abundances.extend(float(x) for x in rng.uniform(0.5, 50.0, size=2))
    eff = [float(x) for x in rng.uniform(50.0, 8000.0, size=num_paths)]
    return dict(num_paths=num_paths, sets=sets, posteriors=posteriors, abundances=abundances, noise_count=float(rng.uniform(0, 30)), eff=eff)


def random_cluster(rng, num_paths, num_sets, ploidy=2, with_abundances=True, eff_zero_share=0.0):
    """Sets of 1 .. ploidy paths, sorted (so homozygous sets have adjacent duplicates), random doubles."""
    sets = []
    for _ in range(num_sets):
        size = int(rng.integers(1, ploidy + 1))
        sets.append(tuple(sorted(int(x) for x in rng.integers(0, num_paths, size=size))))
    members = sum(len(s) for s in sets)
    eff = [float(x) for x in rng.uniform(50.0, 8000.0, size=num_paths)]
    for p in range(num_paths):
        if rng.uniform() < eff_zero_share:
            eff[p] = 0.0 if p % 2 else -float(rng.uniform(1.0, 10.0))
    return dict(num_paths=num_paths, sets=sets, posteriors=[float(x) for x in rng.uniform(0.0, 1.0, size=num_sets)],
                abundances=[float(x) for x in rng.uniform(0.0, 500.0, size=members)] if with_abundances else [],
                noise_count=float(rng.uniform(0.0, 40.0)), eff=eff)


def cluster_with(rng, num_paths, num_members, ploidy=2):
    """Exactly num_members members over num_paths paths (sets of `ploidy`, the last one shorter)."""
    sets, left = [], num_members
    while left > 0:
        size = min(ploidy, left)
        sets.append(tuple(sorted(int(x) for x in rng.integers(0, max(num_paths, 1), size=size))))
        left -= size
    c = random_cluster(rng, num_paths, 0, ploidy)
    c["sets"] = sets
    c["posteriors"] = [float(x) for x in rng.uniform(0.0, 1.0, size=len(sets))]
    c["abundances"] = [float(x) for x in rng.uniform(0.0, 500.0, size=num_members)]
    return c
