"""The plain-Python model of the polyploid one-call route (tests/nested_full_model.py) pinned to a hand-written case and to the numpy
oracle, and the host-side plan of the call (rpvg_amd/csrc/subset_full_plan.hpp) walked by a program of its own under AddressSanitizer
and UBSan.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from tests import nested_full_model as model, small_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranks_are_the_lexicographic_order():
    for g, G in ((1, 5), (3, 4), (6, 3), (8, 2), (4, 1)):
        sets = model.all_sets(G, g)
        assert len(sets) == model.set_count(G, g)
        assert [model.members_of_rank(G, g, r) for r in range(len(sets))] == sets
    assert model.set_count(0, 3) == 0 and model.set_count(30, 6) == math.comb(35, 6)


def test_hand_written_case():
    """Two transcripts x two HSTs, four haplotype columns A B C D, group size 3: {A, A, B} and {A, C, D} expand to the same list."""
    columns = [[0, 2], [1, 3], [0, 3], [1, 2]]
    gid = [0, 0, 1, 1]
    sets = model.all_sets(4, 3)
    post = [0.0] * len(sets)
    post[sets.index((0, 0, 1))] = 0.25       # A A B -> 0 0 1 2 2 3
    post[sets.index((0, 2, 3))] = 0.125      # A C D -> 0 0 1 2 2 3
    post[sets.index((1, 1, 1))] = 0.5        # B B B -> 1 1 1 3 3 3
    post[sets.index((0, 1, 2))] = 0.0005     # below the threshold
    post[sets.index((3, 3, 3))] = 0.1245
    ranks, kept, total = model.retain(post, 1e-3)
    assert [sets[r] for r in ranks] == [(0, 0, 1), (0, 2, 3), (1, 1, 1), (3, 3, 3)]
    assert kept == [0.25, 0.125, 0.5, 0.1245] and total == ((0.25 + 0.125) + 0.5) + 0.1245
    subs = model.subsets(ranks, kept, total, columns, 3, 1e-3)
    assert [s[0] for s in subs] == [[0, 0, 1, 2, 2, 3], [1, 1, 1, 2, 2, 2], [1, 1, 1, 3, 3, 3]]
    assert [s[1] for s in subs] == [(0.25 + 0.125) / total, 0.1245 / total, 0.5 / total]
    # EM results by hand: abundances of the distinct paths, noise
    solutions = [([0, 1, 2, 3], [8.0, 3.0, 6.0, 2.0], 1.0), ([1, 2], [12.0, 7.0], 1.0), ([1, 3], [10.0, 9.0], 1.0)]
    merged, noise = model.merge(subs, solutions, gid, 20.0)
    w0, w1, w2 = (s[1] for s in subs)
    assert [m[0] for m in merged] == [(0, 0, 1), (1, 1, 1), (2, 2, 2), (2, 2, 3), (3, 3, 3)]
    by_key = {m[0]: m for m in merged}
    assert by_key[(0, 0, 1)][1] == w0 and by_key[(0, 0, 1)][2] == [8.0 * w0 / 2, 8.0 * w0 / 2, 3.0 * w0 / 1]
    assert by_key[(1, 1, 1)][1] == w1 + w2
    assert by_key[(1, 1, 1)][2] == [12.0 * w1 / 3 + 10.0 * w2 / 3] * 3
    assert by_key[(2, 2, 2)][2] == [7.0 * w1 / 3] * 3 and by_key[(3, 3, 3)][2] == [9.0 * w2 / 3] * 3
    assert by_key[(2, 2, 3)][2] == [6.0 * w0 / 2, 6.0 * w0 / 2, 2.0 * w0 / 1]
    assert noise == ((1.0 * w0 + 1.0 * w1) + 1.0 * w2) + (1 - ((w0 + w1) + w2)) * 20.0


def _model_estimate(paths, rows, g, min_hap_prob=1e-3, prob_precision=1e-8):
    """estimate_haplotype_transcripts with the model between the posteriors and the estimates."""
    groups, mult = np_oracle.source_groups(paths)
    G, noise, counts = np_oracle.grouped_matrix(rows, groups)
    Gn = np_oracle.add_noise_and_normalize(G, noise)
    Gn, gcounts = np_oracle.read_collapse(Gn, counts, prob_precision)
    sets, post = np_oracle.posteriors_full(Gn[:, :-1].copy(), Gn[:, -1].copy(), gcounts, mult, g)
    assert sets == model.all_sets(len(groups), g)
    ranks, kept, total = model.retain(post, min_hap_prob)
    subs = model.subsets(ranks, kept, total, groups, g, min_hap_prob)
    solutions = []
    for U, _ in subs:
        distinct = sorted(set(U))
        P, pn, pc = np_oracle.dense_matrix(rows, len(paths), distinct)
        Pn, pc = np_oracle.read_collapse(np_oracle.add_noise_and_normalize(P, pn), pc, prob_precision)
        ab, nc, _, _ = np_oracle.em(Pn, pc)
        solutions.append((distinct, ab, nc))
    return model.merge(subs, solutions, [p["group_id"] for p in paths], float(sum(r[0] for r in rows)))


@pytest.mark.parametrize("g", [1, 3, 6])
def test_model_against_the_numpy_oracle(g):
    rng = np.random.default_rng(9300 + g)
    multiplicities = set()
    for _ in range(4):
        cl = small_cases.make_cluster(rng, 2, (2, 2), n_haps=int(rng.integers(3, 7)), n_reads=40)
        want = np_oracle.estimate_haplotype_transcripts(cl["paths"], cl["rows"], ploidy=g)
        merged, noise = _model_estimate(cl["paths"], cl["rows"], g)
        assert [m[0] for m in merged] == sorted(want["keyed"])
        for key, posterior, abundances in merged:
            assert small_cases.rel_close(posterior, want["keyed"][key][0], rel=1e-12, floor=1e-300)
            assert small_cases.rel_close(abundances, want["keyed"][key][1], rel=1e-12, floor=1e-300)
            multiplicities.update(key.count(p) for p in key)
        assert small_cases.rel_close(noise, want["noise"], rel=1e-12, floor=1e-300)
    if g >= 3:
        assert max(multiplicities) >= 3


def test_plan_under_the_sanitizers():
    """tests/cpp/subset_full_plan_check.cpp: unranking against explicit enumeration for group sizes 1 .. 8 over 1 .. 12 columns, the
    last rank of a problem at the set bound, slots, the launch cuts either side of 2^27 sets, every host-side refusal and the packed
    layout, as a program of its own built with AddressSanitizer and UBSan."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "subset_full_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "subset_full_plan_check.cpp"), "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"


def test_the_stats_struct_carries_the_new_counters():
    from rpvg_amd import hip
    names = [n for n, _ in hip.CKernelStats._fields_]
    assert names[-3:] == ["nested_full_calls", "nested_full_sets", "nested_full_retained"]
    assert "rpvg_hip_nested_full_subset_em" in hip.EXPORTS and "rpvg_hip_subset_em_get_sets" in hip.EXPORTS
    assert hip.CSubsetEmSetsView._fields_[1][0] == "group_size"
