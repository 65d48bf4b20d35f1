"""The table of EM size-bin edges (tests/em_bin_cases.py) checked without a GPU: every case lands in the bin it names by
the Python restatement of emBinOf, every named boundary has a case on each side, one unit apart, and the kept rows of
every case are pairwise farther apart than prob_precision.  The C++ rule itself (rpvg_amd/csrc/em_plan.hpp) is compiled with g++
and held to the same restatement, shape by shape, and its plan of a solve to expectations at the sizes where a decision flips."""
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle
from tests import em_bin_cases as ebc


@pytest.mark.parametrize("case", ebc.CASES, ids=lambda c: c.name)
def test_case_lands_in_its_bin(case):
    C, rows, entries = case.shape()
    assert ebc.em_bin(C, rows, entries) == case.bin, (case.name, C, rows, entries)
    assert len(case.cluster().count) >= rows


def test_every_boundary_has_a_case_on_each_side():
    for name, (what, last_low, low, high) in ebc.BOUNDARIES.items():
        lo, hi = ebc.BY_NAME[low], ebc.BY_NAME[high]
        assert ebc.quantity(lo, what) == last_low, (name, low)
        assert ebc.quantity(hi, what) == last_low + 1, (name, high)
        print(f"{name:32s} {low:>16s} bin {lo.bin:2d} | {high:<16s} bin {hi.bin:2d}")
    # every bin edge changes the bin (or, for the mid-size line, the mid-size verdict; for the column map, the fill route)
    for name, (what, _, low, high) in ebc.BOUNDARIES.items():
        lo, hi = ebc.BY_NAME[low], ebc.BY_NAME[high]
        if what == "cluster_paths":
            assert lo.cluster().n_paths <= ebc.LDS_MAP_PATHS < hi.cluster().n_paths
        elif name.startswith("mid-size"):
            assert not ebc.is_mid(*lo.shape()) and ebc.is_mid(*hi.shape())
        else:
            assert lo.bin != hi.bin, name
    # every one of the twelve bins, and the grid's dense sub-route, has a case
    assert {c.bin for c in ebc.CASES} == set(range(12))
    assert any(c.bin == ebc.GRID_BIN and ebc.dense_rule(*c.shape()) for c in ebc.CASES)
    assert any(c.bin == ebc.GRID_BIN and not ebc.dense_rule(*c.shape()) for c in ebc.CASES)


def test_mid_size_move_takes_eight_problems_and_not_nine():
    mids = [ebc.BY_NAME[n].shape() for n in ebc.MID_COUNT_CASES]
    assert all(ebc.is_mid(*s) for s in mids)
    assert ebc.routes(mids[:8]) == [ebc.GRID_BIN] * 8
    assert ebc.routes(mids) == [ebc.STREAMED_BIN] * 9
    # a lone problem one unit below the grid threshold is a mid-size one: it takes the grid all the same
    assert ebc.routes([ebc.BY_NAME["grid_csr_lo"].shape()]) == [ebc.GRID_BIN]
    assert ebc.routes([ebc.BY_NAME["mid_work_lo"].shape()]) == [ebc.STREAMED_BIN]


def test_rule_restatement_at_the_byte_limits():
    """The LDS formulas at the limits the issue names: the grid keeps C <= 3993 in LDS, the wide bin starts at C = 3993,
    four wavefronts take C = 1174 .. 3992."""
    assert ebc.grid_lds_bytes(3993) <= ebc.LDS_LIMIT < ebc.grid_lds_bytes(3994)
    assert ebc.lds_bytes(3992, 0, 0, 256, False) <= ebc.LDS_LIMIT < ebc.lds_bytes(3993, 0, 0, 256, False)
    assert ebc.lds_bytes(1173, 0, 0, 1024, False) <= ebc.LDS_LIMIT < ebc.lds_bytes(1174, 0, 0, 1024, False)
    # the nested model's restatement (subset_em.hip: device route up to 3991 cluster paths)
    nested_ok = lambda paths: 8 * (5 * (paths + 1) + 6) <= ebc.LDS_LIMIT
    assert nested_ok(3991) and not nested_ok(3992)
    assert ebc.em_bin(3992, 10, 10) == 2 and ebc.em_bin(3993, 10, 10) == 10


@pytest.mark.parametrize("case", ebc.CASES, ids=lambda c: c.name)
def test_kept_rows_are_pairwise_apart(case):
    """The noise column of the normalised matrix alone separates every two kept rows by more than prob_precision."""
    cl = case.cluster()
    cols = case.cols()
    rows = cl.rows()
    P, noise, counts = np_oracle.dense_matrix(rows, cl.n_paths, cols)
    kept = P.sum(axis=1) > 0
    assert int(kept.sum()) == case.shape()[1]
    Pn = np_oracle.add_noise_and_normalize(P, noise)
    z = np.sort(Pn[kept, -1])
    assert len(z) < 2 or float(np.min(np.diff(z))) > ebc.PROB_PRECISION
    assert np.all(Pn[kept, :-1][Pn[kept, :-1] > 0] >= ebc.PROB_PRECISION)
    # rows ascend inside themselves, and every probability is at least prob_precision (the upload's invariants)
    off = cl.ent_off.astype(np.int64)
    for r in range(min(len(cl.count), 2000)):
        p = cl.ent_prob[off[r]:off[r + 1]]
        assert np.all(np.diff(p) >= 0) and np.all(p >= ebc.PROB_PRECISION)
        assert len(set(cl.ent_path[off[r]:off[r + 1]].tolist())) == len(p)


def test_fillers_are_mixed_sizes_of_their_bin():
    for b in (0, 1, 7) + ebc.REGISTER_BINS:
        fs = ebc.fillers(b)
        assert [ebc.em_bin(*f.shape()) for f in fs] == [b] * len(fs)
        assert len({f.shape() for f in fs}) == len(fs)   # sizes mixed


@pytest.mark.parametrize("cus", [256, 304, 80])
def test_fill_workgroups_switch_maps_between_subsets_of_one_cluster(cus):
    """The map-cache call puts four subset problems of one cluster on each of four fill workgroups, one after the other."""
    clusters, problems = ebc.map_cache_call(cus)
    seqs = ebc.fill_sequences([len(clusters[k].count) for k, _ in problems], cus)
    assert len(seqs) == ebc.FILL_WORKGROUPS_PER_CU * cus
    assert ebc.map_switches(clusters, problems, cus) == 4 * (ebc.MAP_LANE_PROBLEMS - 1)
    lanes = [seq for seq in seqs if any(problems[p][0] != 2 for p in seq)]
    assert len(lanes) == 4 and all(len({problems[p][0] for p in seq}) == 1 for seq in lanes)
    # the grid-stride restated on a small list: problem 0 has five segments, the others one; G = min(10, 8)
    assert ebc.fill_sequences([5000, 1, 1, 1, 1, 1], 1) == [[0, 4], [0, 5], [0], [0], [0], [1], [2], [3]]


def _em_plan_check():
    """tests/cpp/em_plan_check.cpp compiled against rpvg_amd/csrc/em_plan.hpp alone: plain C++17, no GPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "em_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "rpvg_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "em_plan_check.cpp"), "-o", binary])
    return binary


def test_em_plan_decisions_at_their_edges():
    """The plan of a solve — grid gate, mid-size move, fused look, grids per CU, LDS per variant, the launch tables with their
    streams for one and five register launches —, the sampler's route and the storage layout, at the sizes where each flips."""
    assert subprocess.run([_em_plan_check()], capture_output=True, text=True, check=True).stdout.strip() == "ok"


def test_cpp_rule_equals_the_python_restatement():
    """emBinOf, the mid-size predicate, emDenseRule, the route inside a call and the statistics slots of em_plan.hpp — the code
    the device and the host run — against em_bin, is_mid, dense_rule, routes and expected_stats, for the shape of every case,
    the fillers of every bin, the eight and the nine mid-size problems in one call, and the byte limits of the LDS formulas."""
    calls = [[c.shape()] for c in ebc.CASES]
    calls += [[f.shape() for f in ebc.fillers(b)] for b in (0, 1, 7) + ebc.REGISTER_BINS]
    mids = [ebc.BY_NAME[n].shape() for n in ebc.MID_COUNT_CASES]
    calls += [mids[:8], mids]
    calls += [[(C, 10, 10)] for C in (1173, 1174, 3992, 3993, 3994)]
    calls += [[(C, 4096, ebc.GRID_MIN_WORK - 4096)] for C in (3993, 3994)]
    calls.append([s for call in calls for s in call])   # and everything in one call (more than eight mid-size problems: none moves)
    text = "".join("".join(f"{C} {rows} {entries}\n" for C, rows, entries in call) + "-\n" for call in calls)
    out = subprocess.run([_em_plan_check(), "shapes"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    at = 0
    for call in calls:
        got = [tuple(int(x) for x in out[at + i].split()) for i in range(len(call))]
        assert out[at + len(call)] == "-"
        at += len(call) + 1
        want_routes = ebc.routes(call)
        for s, g, route in zip(call, got, want_routes):
            assert g[:4] == (ebc.em_bin(*s), int(ebc.is_mid(*s)), int(ebc.dense_rule(*s)), route), (s, g)
        for launches, column in ((1, 4), (5, 5)):
            slots = {}
            for g in got:
                slots[g[column]] = slots.get(g[column], 0) + 1
            want_slots, want_dense = ebc.expected_stats(call, launches)
            assert slots == want_slots, (call[:3], launches)
            assert sum(1 for g in got if g[3] == ebc.GRID_BIN and g[2]) == want_dense
    assert at == len(out) - 1 and out[-1] == ""
