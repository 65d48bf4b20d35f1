"""A plain-Python restatement of the resident-estimates gather (include/rpvg_table.h, rpvg_estimates_part -> rpvg_estimates_flat): from
the views of the nested calls as include/rpvg_hip.h documents them to the flat arrays, and the refusals in their reporting order.
Nothing here is shared with rpvg_amd/csrc/estimates_gather_plan.hpp; tests/test_resident_estimates_model.py pins it to the hand case
tests/cpp/estimates_gather_plan_check.cpp writes out.

A part is a dict: width (0: the diploid form), unit_cluster [U], subset_off [U+1], path_off [S+1], set_count [U], cluster_noise_count
[U], set_posterior [L], set_abundance [L, 2 or width], and set_first / set_second [L] (width 0) or set_size [L] / set_member [L, width].
"""
import numpy as np

NO = 0xFFFFFFFF
MAX_WIDTH = 8
BAD_UNIT_CLUSTER, BAD_DUPLICATE, BAD_SUBSET_OFF, BAD_PATH_OFF, BAD_SET_COUNT, BAD_SET_SIZE, BAD_MEMBER = range(1, 8)
BAD_WIDTH = "width"


class Refused(Exception):
    def __init__(self, part, unit, why):
        super().__init__(f"part {part}, unit {unit}: {why}")
        self.part, self.unit, self.why = part, unit, why


def cells(width):
    return 2 if width == 0 else width


def _offsets_bad(off, i, n, total):
    o0, o1 = int(off[i]), int(off[i + 1])
    return o0 > o1 or o1 > total or (i == 0 and o0 != 0) or (i + 1 == n and o1 != total)


def _slot(part, slot):
    """(members, abundances) of a slot, or the offence of its size"""
    if part["width"] == 0:
        size = 1 if int(part["set_second"][slot]) == NO else 2
        members = [int(part["set_first"][slot]), int(part["set_second"][slot])][:size]
    else:
        size = int(part["set_size"][slot])
        if not 1 <= size <= part["width"]:
            return None, None
        members = [int(x) for x in part["set_member"][slot][:size]]
    return members, [float(x) for x in part["set_abundance"][slot][:size]]


def _unit_offence(part, u, K, cluster_path_off, listed):
    c = int(part["unit_cluster"][u])
    U, S, L = len(part["unit_cluster"]), len(part["path_off"]) - 1, int(part.get("num_slots", len(part["set_posterior"])))
    if c >= K:
        return BAD_UNIT_CLUSTER
    if listed[c] > 1:
        return BAD_DUPLICATE
    if _offsets_bad(part["subset_off"], u, U, S):
        return BAD_SUBSET_OFF
    s0, s1 = int(part["subset_off"][u]), int(part["subset_off"][u + 1])
    if any(_offsets_bad(part["path_off"], s, S, L) for s in range(s0, s1)):
        return BAD_PATH_OFF
    first = int(part["path_off"][s0])
    slots = int(part["path_off"][s1]) - first if s1 > s0 else 0
    count = int(part["set_count"][u])
    if count > slots:
        return BAD_SET_COUNT
    sets = [_slot(part, first + q) for q in range(count)]
    if any(members is None for members, _ in sets):
        return BAD_SET_SIZE
    paths = int(cluster_path_off[c + 1]) - int(cluster_path_off[c])
    if any(m >= paths for members, _ in sets for m in members):
        return BAD_MEMBER
    return 0


def gather(cluster_path_off, totals, parts):
    """The flat arrays (a dict of numpy arrays, without the batch's two) of the K = len(totals) clusters, or Refused with the smallest
    offending (part, unit)."""
    K = len(totals)
    for p, part in enumerate(parts):
        if part["width"] > MAX_WIDTH:
            raise Refused(p, None, BAD_WIDTH)
    listed = [0] * K
    for part in parts:
        for c in part["unit_cluster"]:
            if int(c) < K:
                listed[int(c)] += 1
    owner = {}
    for p, part in enumerate(parts):
        for u in range(len(part["unit_cluster"])):
            why = _unit_offence(part, u, K, cluster_path_off, listed)
            if why:
                raise Refused(p, u, why)
            owner[int(part["unit_cluster"][u])] = (part, u)
    set_off, member_off, abund_off, members, posteriors, abundances, noise = [0], [0], [0], [], [], [], []
    for k in range(K):
        if k in owner:
            part, u = owner[k]
            s0, s1 = int(part["subset_off"][u]), int(part["subset_off"][u + 1])
            first = int(part["path_off"][s0])
            for q in range(int(part["set_count"][u])):
                m, a = _slot(part, first + q)
                members.extend(m)
                abundances.extend(a)
                member_off.append(len(members))
                posteriors.append(float(part["set_posterior"][first + q]))
            noise.append(float(part["cluster_noise_count"][u]) if s1 > s0 else float(totals[k]))
        else:
            noise.append(float(totals[k]))
        set_off.append(len(posteriors))
        abund_off.append(len(abundances))
    return dict(set_off=np.array(set_off, np.uint64), member_off=np.array(member_off, np.uint64), members=np.array(members, np.uint32),
                posteriors=np.array(posteriors, np.float64), abund_off=np.array(abund_off, np.uint64),
                abundances=np.array(abundances, np.float64), noise_count=np.array(noise, np.float64))


FLAT_NAMES = ("set_off", "member_off", "members", "posteriors", "abund_off", "abundances", "noise_count")


def make_part(rng, width, clusters, sets_per_cluster, path_counts, no_subsets=()):
    """A valid part: unit i is clusters[i] with sets_per_cluster[i] sets (sizes cycling through 1 .. width, or one and two members
    mixed at width 0), one to three subsets whose lists leave a few slots unused; units listed in no_subsets have no subset."""
    w = cells(width)
    subset_off, path_off, set_count, noise = [0], [0], [], []
    first, second, size, member, posterior, abundance = [], [], [], [], [], []
    for i, (c, n) in enumerate(zip(clusters, sets_per_cluster)):
        paths = int(path_counts[c])
        if i in no_subsets:
            assert n == 0
            subset_off.append(subset_off[-1])
            set_count.append(0)
            noise.append(-3.0)
            continue
        subsets = int(rng.integers(1, 4))
        slots = n + int(rng.integers(0, 3))
        cuts = sorted(int(x) for x in rng.integers(0, slots + 1, size=subsets - 1))
        unit_first = path_off[-1]
        for end in cuts + [slots]:
            path_off.append(unit_first + end)
        subset_off.append(subset_off[-1] + subsets)
        set_count.append(n)
        noise.append(float(rng.random() * 5))
        for q in range(slots):
            used = q < n
            k = 0
            if used:
                k = (q % width) + 1 if width else 1 + (q + i) % 2
            cell = [int(rng.integers(0, paths)) if j < k else NO for j in range(w)]
            if width == 0:
                first.append(cell[0] if used else 12345)
                second.append(cell[1] if used else 54321)
            else:
                size.append(k if used else 77)
                member.append(cell)
            posterior.append(float(rng.random()))
            abundance.append([float(rng.random() * 100) if j < k else 0.0 for j in range(w)])
    L = path_off[-1]
    part = dict(width=width, unit_cluster=np.array(clusters, np.uint32), subset_off=np.array(subset_off, np.uint64),
                path_off=np.array(path_off, np.uint64), set_count=np.array(set_count, np.uint32),
                cluster_noise_count=np.array(noise, np.float64), set_posterior=np.array(posterior, np.float64),
                set_abundance=np.array(abundance, np.float64).reshape(L, w))
    if width == 0:
        part.update(set_first=np.array(first, np.uint32), set_second=np.array(second, np.uint32))
    else:
        part.update(set_size=np.array(size, np.uint32), set_member=np.array(member, np.uint32).reshape(L, w))
    return part


def part_of_view(view, unit_cluster, width):
    """The part of a nested call's host view (the dicts rpvg_amd returns: rpvg_hip_subset_em_view with width 0,
    rpvg_hip_subset_em_sets_view / _independent_view with their group size)."""
    part = dict(width=width, unit_cluster=np.asarray(unit_cluster, np.uint32))
    for name in ("subset_off", "path_off", "set_count", "cluster_noise_count", "set_posterior", "set_abundance"):
        part[name] = view[name]
    for name in (("set_first", "set_second") if width == 0 else ("set_size", "set_member")):
        part[name] = view[name]
    return part


def hand_case():
    """(cluster_path_off, totals, parts, expected flat arrays as lists): the case of tests/cpp/estimates_gather_plan_check.cpp."""
    a = dict(width=0, unit_cluster=[2, 0], subset_off=[0, 2, 2], path_off=[0, 2, 5], set_count=[3, 0], cluster_noise_count=[7.0, 8.0],
             set_first=[1, 0, 3, 9, 9], set_second=[NO, 2, 3, 9, 9], set_posterior=[0.5, 0.25, 0.125, -1.0, -1.0],
             set_abundance=[[1.5, 99.0], [2.5, 3.5], [4.5, 5.5], [-1.0, -1.0], [-1.0, -1.0]])
    b = dict(width=3, unit_cluster=[3], subset_off=[0, 1], path_off=[0, 4], set_count=[2], cluster_noise_count=[0.75],
             set_size=[1, 3, 7, 7], set_member=[[0, NO, NO], [0, 0, 0], [5, 5, 5], [5, 5, 5]], set_posterior=[0.0625, 0.03125, -1.0, -1.0],
             set_abundance=[[6.5, 0.0, 0.0], [7.5, 8.5, 9.5], [-1.0] * 3, [-1.0] * 3])
    expected = dict(set_off=[0, 0, 0, 3, 5], member_off=[0, 1, 3, 5, 6, 9], members=[1, 0, 2, 3, 3, 0, 0, 0, 0],
                    posteriors=[0.5, 0.25, 0.125, 0.0625, 0.03125], abund_off=[0, 0, 0, 5, 9],
                    abundances=[1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5], noise_count=[10.0, 20.0, 7.0, 0.75])
    return [0, 3, 5, 9, 10], [10.0, 20.0, 30.0, 40.0], [typed(a), typed(b)], expected


_DTYPES = dict(unit_cluster=np.uint32, subset_off=np.uint64, path_off=np.uint64, set_count=np.uint32, cluster_noise_count=np.float64,
               set_first=np.uint32, set_second=np.uint32, set_size=np.uint32, set_member=np.uint32, set_posterior=np.float64,
               set_abundance=np.float64)


def typed(part):
    """The arrays of a hand-written part as numpy arrays of the ABI's types."""
    return {name: (np.array(value, _DTYPES[name]) if name in _DTYPES else value) for name, value in part.items()}
