"""Plain-Python model of the set text (include/rpvg_text.h, rpvg_hip_estimates_set_text): the rows the two writers print whose row
is a path group set — JointHaplotypeAbundanceEstimatesWriter (JOINT) and JointHaplotypeEstimatesWriter (POSTERIOR),
rpvg_amd/host/io/estimates_writers.cpp — every double by tests/table_text_model.fmt.  The cases of tests/test_hip_set_text.py."""
import numpy as np

from tests.table_text_model import fmt, join

JOINT, POSTERIOR = 2, 3


def _raw(name):
    return name.encode() if isinstance(name, str) else bytes(name)


def set_text(kind, flat, member_tpm, names, cluster_ids, ploidy, min_posterior, precision=8):
    """flat: the arrays of rpvg_estimates_flat by name; member_tpm [M] (JOINT; None for POSTERIOR) -> (text, row_off [S + 1]).
    A set that is not printed is an empty row."""
    rows = []
    for k in range(len(cluster_ids)):
        p0 = int(flat["cluster_path_off"][k])
        s0, s1 = int(flat["set_off"][k]), int(flat["set_off"][k + 1])
        first_member = int(flat["member_off"][s0]) if s1 > s0 else 0
        for s in range(s0, s1):
            p = float(flat["posteriors"][s])
            if not (not (p < min_posterior)):                      # printed iff not (p < min_posterior): the writers' test, literally
                rows.append(b"")
                continue
            m0, m1 = int(flat["member_off"][s]), int(flat["member_off"][s + 1])
            n = m1 - m0
            assert 1 <= n <= ploidy
            row = b"".join(_raw(names[p0 + int(flat["members"][m])]) + b"\t" for m in range(m0, m1)) + b".\t" * (ploidy - n)
            row += str(int(cluster_ids[k])).encode() + b"\t" + fmt(p, precision).encode()
            if kind == JOINT:
                a0 = int(flat["abund_off"][k])
                for m in range(m0, m1):
                    row += b"\t" + fmt(flat["abundances"][a0 + m - first_member], precision).encode() + b"\t" + fmt(member_tpm[m], precision).encode()
                row += b"\t0\t0" * (ploidy - n)
            rows.append(row + b"\n")
    return join(rows)


def header(kind, ploidy):
    """The header row of the writer."""
    text = "".join(f"Name_{i + 1}\t" for i in range(ploidy)) + "ClusterID\tHaplotypingProbability"
    if kind == JOINT:
        text += "".join(f"\tReadCount_{i + 1}\tTPM_{i + 1}" for i in range(ploidy))
    return text.encode() + b"\n"


# ---- cases --------------------------------------------------------------------------------------------------------------------------

NAME_LENGTHS = [0, 1, 3, 4, 5, 26, 27, 255]


def cluster_of_sets(sets, posteriors, num_paths, rng, with_abundances=True, abundances=None):
    """A cluster of tests/estimates_table_model: effective lengths > 0, one abundance per member (or none)."""
    members = sum(len(s) for s in sets)
    if abundances is None:
        abundances = [0.0 if i % 7 == 3 else float(x) for i, x in enumerate(rng.gamma(0.8, 30.0, size=members))] if with_abundances else []
    return dict(num_paths=num_paths, sets=[tuple(s) for s in sets], posteriors=[float(p) for p in posteriors], abundances=list(abundances),
                noise_count=float(rng.random()), eff=[float(x) for x in rng.gamma(2.0, 400.0, size=num_paths)])


def every_size_cluster(ploidy, num_paths, rng, with_abundances=True):
    """Sets of every size 1 .. ploidy (so every pad count occurs), members unsorted and repeated: {a, a, ..}, {b, a, ..}."""
    assert num_paths >= 2
    sets = []
    for n in range(1, ploidy + 1):
        sets.append([int(x) for x in rng.integers(0, num_paths, size=n)])     # unsorted
        sets.append([num_paths - 1] * n)                                       # {a, a, ...}
        sets.append(([1, 0] * n)[:n])                                          # {b, a, ...}
    posteriors = rng.random(len(sets))
    return cluster_of_sets(sets, posteriors, num_paths, rng, with_abundances)


def hand_ploidy_2():
    """One cluster (ClusterID 7) of three paths at ploidy 2: a heterozygous, a homozygous and a one-member set, min_posterior 0.01:
    the fourth set lies below it."""
    flat = dict(cluster_path_off=[0, 3], set_off=[0, 4], member_off=[0, 2, 4, 5, 7], members=[0, 1, 2, 2, 1, 1, 0], posteriors=[0.5, 0.25, 0.125, 0.001],
                abund_off=[0, 7], abundances=[10.0, 2.5, 3.0, 3.0, 1e-5, 4.0, 5.0])
    member_tpm = [250000.0, 0.125, 99999999.5, 1.0, 0.0, 7.0, 8.0]
    names, ids = ["hapA", "hapB", "c"], [7]
    joint = (b"hapA\thapB\t7\t0.5\t10\t250000\t2.5\t0.125\n" + b"c\tc\t7\t0.25\t3\t1e+08\t3\t1\n" + b"hapB\t.\t7\t0.125\t1e-05\t0\t0\t0\n")
    posterior = b"hapA\thapB\t7\t0.5\n" + b"c\tc\t7\t0.25\n" + b"hapB\t.\t7\t0.125\n"
    return flat, member_tpm, names, ids, 0.01, joint, posterior


def hand_ploidy_3():
    """Two clusters (ClusterIDs 4 and 9; the first without sets) at ploidy 3: a one-member set with two pads and a full set."""
    flat = dict(cluster_path_off=[0, 1, 3], set_off=[0, 0, 2], member_off=[0, 1, 4], members=[1, 0, 1, 0], posteriors=[1.0, 0.3333333333333333],
                abund_off=[0, 0, 4], abundances=[1.5, 2.0, 0.0, 123456785.0])
    member_tpm = [1e6, 0.5, 0.0, 1e-7]
    names, ids = ["unused", "x", "yy"], [4, 9]
    joint = b"yy\t.\t.\t9\t1\t1.5\t1000000\t0\t0\t0\t0\n" + b"x\tyy\tx\t9\t0.33333333\t2\t0.5\t0\t0\t1.2345678e+08\t1e-07\n"
    posterior = b"yy\t.\t.\t9\t1\n" + b"x\tyy\tx\t9\t0.33333333\n"
    return flat, member_tpm, names, ids, 0.0, joint, posterior
