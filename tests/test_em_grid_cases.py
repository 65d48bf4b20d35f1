"""The table of the whole-GPU EM's edges (tests/em_grid_cases.py) checked without a GPU: the table covers every target it
names at 256 CUs by the Python restatement of the launch plans, the restatement equals the C++ plans (rpvg_amd/csrc/em_plan.hpp,
compiled with g++ under the address and undefined-behaviour sanitizers as a program of its own: tests/cpp/em_grid_plan_check.cpp),
the long-double model reproduces the oracle's iteration counts with a decision gap above 1e-6, the oracle's distance from the
model is what the table records (the GPU tests' bound is 64 x its maximum), and the model's known answers."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import em_grid_cases as egc


def _lanes(c):
    return c.launch_shape()["lanes"]


def _csr():
    return [c for c in egc.CASES if not egc.dense_rule(*c.shape())]


def _dense():
    return [c for c in egc.CASES if egc.dense_rule(*c.shape())]


def test_every_case_takes_the_route_it_names_within_the_size_limit():
    for c in egc.CASES:
        C, rows, entries = c.shape()
        assert ("dense" if egc.dense_rule(C, rows, entries) else "csr") == c.route, c.name
        assert c.name.startswith(c.route + "_")
        assert 40 * C <= 156 * 1024   # the grid bin holds its vectors in LDS (emBinOf)
        if c.name != "csr_cap_l1":
            assert rows <= 5200 and entries <= 500_000, c.name
    # the one case beyond: 2 workgroups per CU of 256 rows and more each — no smaller problem reaches that cap at 256 CUs
    C, rows, entries = egc.BY_NAME["csr_cap_l1"].shape()
    assert egc.csr_launch_shape(C, 2 * egc.CUS * 256 - 256, entries)["grid"] < 2 * egc.CUS


def test_csr_lanes_on_both_sides_of_every_mean_row_length():
    by = {n: egc.BY_NAME[n] for n in ("csr_lanes1_hi", "csr_lanes4_lo", "csr_lanes4_hi", "csr_lanes16_lo", "csr_lanes16_hi", "csr_lanes64_lo")}
    assert [_lanes(c) for c in by.values()] == [1, 4, 4, 16, 16, 64]
    for lo, hi, mean in (("csr_lanes1_hi", "csr_lanes4_lo", 6), ("csr_lanes4_hi", "csr_lanes16_lo", 24), ("csr_lanes16_hi", "csr_lanes64_lo", 96)):
        (C0, r0, e0), (C1, r1, e1) = by[lo].shape(), by[hi].shape()
        assert (C0, r0) == (C1, r1) and e0 + 1 == e1 == mean * r1   # one entry apart, the high side exactly on the mean
    # at 96 entries per row the dense rule needs fewer than 147 columns: the 64-lane cases are wider (restated, not assumed)
    assert egc.dense_rule(146, 300, 28800) and not egc.dense_rule(147, 300, 28800)
    assert all(c.shape()[0] >= 150 for c in _csr() if _lanes(c) == 64)
    assert {_lanes(c) for c in _csr()} == {1, 4, 16, 64}


def test_csr_rows_blocks_and_trips():
    shapes = {c.name: (c.shape(), c.launch_shape()) for c in _csr()}
    for rows, grid in ((1, 1), (3, 1), (255, 1), (256, 1), (257, 2)):
        (C, r, e), s = shapes[f"csr_rows{rows}"]
        assert r == rows and s["lanes"] == 1 and s["grid"] == grid
    (C, r, e), s = shapes["csr_last_block_1"]
    assert egc.block_rows(s, r)[-1] == 1 and s["grid"] > 1
    (C, r, e), s = shapes["csr_c2049"]
    assert egc.block_rows(s, r)[-1] == 1
    (C, r, e), s = shapes["csr_remainder_l16"]
    assert r % s["grid"] != 0 and 1 < egc.block_rows(s, r)[-1] < s["rows_per_block"]
    # a workgroup's rows against the rows it holds at once (256 / LANES) and the rows of a trip (4 x 256 / LANES): for every
    # LANES a workgroup with more rows than slots whose count is no multiple of a trip — and, under 64 lanes, several trips
    for name, lanes in (("csr_trips_l1", 1), ("csr_trips_l4", 4), ("csr_trips_l16", 16), ("csr_trips_l64", 64), ("csr_cap_l1", 1)):
        (C, r, e), s = shapes[name]
        slots = egc.GRID_BLOCK // lanes
        assert s["lanes"] == lanes and s["rows_per_block"] > slots and s["rows_per_block"] % (egc.GRID_UNROLL * slots) != 0, name
    assert shapes["csr_trips_l64"][1]["rows_per_block"] == 25 and shapes["csr_long_trips_l64"][1]["rows_per_block"] == 50   # 2 and 4 trips of 16
    assert shapes["csr_long_trips_l64"][1]["lds"] > 64 * 1024   # (the opt-in to more than 64 KB of dynamic LDS)
    # every LANES also with a short workgroup: fewer rows than slots
    for lanes in (1, 4, 16, 64):
        assert any(s["lanes"] == lanes and min(egc.block_rows(s, r)) < egc.GRID_BLOCK // lanes for (C, r, e), s in shapes.values()), lanes


def test_csr_mixed_rows():
    for name, lanes, short, long_ in (("csr_mixed_l64", 64, 1, 300), ("csr_mixed_l1", 1, 2, 200)):
        c = egc.BY_NAME[name]
        k = np.diff(c.cluster().ent_off.astype(np.int64))
        assert _lanes(c) == lanes and k.min() == short and k.max() == long_
    assert int((np.diff(egc.BY_NAME["csr_mixed_l1"].cluster().ent_off.astype(np.int64)) == 200).sum()) == 1


def test_columns_partial_counts_and_caps():
    csr_cols = {c.shape()[0] for c in egc.CASES if "columns" in c.tags and c.route == "csr"}
    assert csr_cols == {15, 16, 17, 63, 64, 65}
    # two columns are one path: 16 B per row of the dense copy against 20 B and more of the CSR — always the dense route
    assert all(egc.dense_rule(2, rows, entries) for rows in (1, 300, 5000) for entries in (0, rows, 1 << 30))
    assert egc.BY_NAME["dense_cols2"].shape()[0] == 2
    assert [egc.csr_launch_shape(C, 300, 600)["partial_ld"] for C in (63, 64, 65)] == [64, 64, 128]
    assert [egc.csr_launch_shape(C, 300, 600)["update_grid"] for C in (15, 16, 17)] == [1, 1, 2]
    partials = {c.launch_shape()["grid"] for c in egc.CASES if "partials" in c.tags}
    assert partials >= {63, 64, 65, 192, 193, 256, 257} and 1 in {c.launch_shape()["grid"] for c in _csr()}
    l1, l64 = egc.BY_NAME["csr_cap_l1"], egc.BY_NAME["csr_cap_l64"]
    assert (_lanes(l1), l1.launch_shape()["grid"]) == (1, 2 * egc.CUS) and (_lanes(l64), l64.launch_shape()["grid"]) == (64, 4 * egc.CUS)
    # ... reached as caps: the rows ask for more workgroups
    assert -(-l1.shape()[1] // 256) > 2 * egc.CUS and -(-l64.shape()[1] // 4) > 4 * egc.CUS
    # the update kernel's four-loads-at-a-time loop (b + 3 x 64 < partials) runs from 193 partials on
    assert all(c.launch_shape()["chunk_its"] == 32 for c in _csr())


def test_dense_route_zero_mass_collapsed_and_counts():
    dense = {c.name: (c.shape(), c.launch_shape()) for c in _dense()}
    want = {"dense_c128": (128, 0, 1), "dense_c129": (129, 0, 2), "dense_c256": (256, 0, 2), "dense_c257": (257, 1, 1), "dense_c2048": (2048, 1, 4)}
    for name, (C, wide, nchunk) in want.items():
        (c, r, e), s = dense[name]
        assert (c, s["wide"], s["nchunk"]) == (C, wide, nchunk) and e == r * (C - 1), name
    c2049 = egc.BY_NAME["csr_c2049"]
    C, r, e = c2049.shape()
    assert C == 2049 and e == r * 2048 and c2049.route == "csr" and _lanes(c2049) == 64
    assert egc.dense_rule(2048, r, r * 2047) and not egc.dense_rule(2049, r, e)
    for route in ("csr", "dense"):
        zero = [c for c in egc.CASES if "zero_mass" in c.tags and c.route == route]
        assert any(c.columns is None and c.zero_mass() > 0 for c in zero), route       # path-less rows
        assert any(c.columns is not None and c.zero_mass() > 0 for c in zero), route   # rows that touch none of the subset
        coll = [c for c in egc.CASES if c.collapse and c.route == route]
        assert coll and all(len(c.inputs()[1]) < c.shape()[1] for c in coll), route     # rows merged (their counts too)
        big = [c for c in egc.CASES if "counts" in c.tags and c.route == route]
        assert big and all(sorted(set((x.cluster().count >= 1_000_000).tolist())) == [False, True] and
                           set(x.cluster().count[x.cluster().count < 1_000_000].tolist()) == {1} for x in big), route
    assert all(c.zero_mass() == 0 for c in egc.CASES if "zero_mass" not in c.tags)
    assert set(egc.BUDGET_CASES) <= set(egc.BY_NAME) and {egc.BY_NAME[n].route for n in egc.BUDGET_CASES} == {"csr", "dense"}
    # the budgets straddle both chunk sizes and two chunks in flight
    assert {egc.DENSE_CHUNK_ITS - 1, egc.DENSE_CHUNK_ITS, egc.DENSE_CHUNK_ITS + 1, 31, 32, 33, 64, 65, 1} == set(egc.CHUNK_BUDGETS)


# ---- the restatement against the C++ plan --------------------------------------------------------------------------------
def _em_grid_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "em_grid_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "em_grid_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_plans_at_their_edges():
    done = subprocess.run([_em_grid_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]


@pytest.mark.parametrize("cus", [256, 304, 80, 1])
def test_cpp_plans_equal_the_python_restatement(cus):
    shapes = [c.shape() for c in egc.CASES]
    shapes += [(C, R, R * (C - 1)) for C in egc.RAW_COLUMNS for R in egc.RAW_ROWS]
    shapes += [(C, R, R * (C - 1)) for C in egc.RAW_CAP_COLUMNS for R in egc.RAW_CAP_ROWS]
    rng = np.random.default_rng(5)
    for _ in range(2000):
        C, rows = int(rng.integers(2, 4000)), int(2 ** rng.uniform(0, 21))
        shapes.append((C, rows, int(rows * 2 ** rng.uniform(0, 8))))
    text = "".join(f"{C} {rows} {entries}\n" for C, rows, entries in shapes)
    done = subprocess.run([_em_grid_plan_check(), "shapes", str(cus)], input=text, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.strip().split("\n")
    assert len(lines) == len(shapes)
    csr_keys = ("lanes", "grid", "rows_per_block", "partial_ld", "update_grid", "lds", "chunk_its")
    dense_keys = ("wide", "nchunk", "grid", "partial_ld", "reduce_slices", "chunk_its")
    for (C, rows, entries), line in zip(shapes, lines):
        f = line.split()
        assert int(f[0]) == int(egc.dense_rule(C, rows, entries)), (C, rows, entries)
        want = egc.csr_launch_shape(C, rows, entries, cus)
        assert f[1] == "csr" and [int(x) for x in f[2:9]] == [want[k] for k in csr_keys], (C, rows, entries, line)
        if C <= egc.DENSE_MAX_COLS:
            want = egc.dense_launch_shape(C, rows, cus)
            assert f[9] == "dense" and [int(x) for x in f[10:16]] == [want[k] for k in dense_keys], (C, rows, entries, line)
        else:
            assert len(f) == 9


# ---- the model ----------------------------------------------------------------------------------------------------------
def _oracle(case, max_em_its, max_rel_em_conv=1e-3):
    Pn, counts = case.inputs()
    ab, nz, total, its, _ = pyoracle.em_dense(Pn, counts, max_em_its, max_rel_em_conv)
    return ab, nz, total, its


@pytest.mark.parametrize("case", egc.CASES, ids=lambda c: c.name)
def test_model_reproduces_the_oracle_and_the_oracle_stays_within_its_recorded_distance(case):
    """Iteration counts equal (to convergence, or to the case's cap), a decision gap above 1e-6 — no verdict of the stop rule
    hangs on the last digits —, and the oracle's distance from the model at every budget the GPU tests use within what
    ORACLE_DISTANCE records for the case."""
    model = case.model()
    ab, nz, total, its = _oracle(case, case.max_em_its)
    got = model.run(case.max_em_its)
    assert got.iterations == its and float(got.total) == total
    if its < case.max_em_its:
        assert its >= egc.MIN_EM_CONV_ITS
    else:
        assert case.max_em_its == egc.HEAVY_CAP and case.shape()[2] >= 90_000   # (only the large cases are capped)
    assert got.gap > 1e-6, got.gap
    worst = egc.distance(ab, nz, got)
    print(f"{case.name:20s} iterations {its:5d} gap {got.gap:.2e} distance {worst:.2e}", end="")
    for budget in (egc.FIXED_BUDGET,) + (egc.CHUNK_BUDGETS if case.name in egc.BUDGET_CASES else ()):
        ab, nz, total, its = _oracle(case, budget, 0.0)
        assert its == budget    # (max_rel_em_conv = 0: no ten iterations without a changed bit inside the budget)
        fixed = model.run(budget, 0.0)
        assert fixed.iterations == budget and fixed.gap > 1e-6
        d = egc.distance(ab, nz, fixed)
        print(f" {budget}:{d:.2e}", end="")
        worst = max(worst, d)
    print()
    assert worst <= egc.ORACLE_DISTANCE[case.name], (worst, egc.ORACLE_DISTANCE[case.name])


def test_the_kernel_bound_is_64_times_the_largest_oracle_distance():
    assert set(egc.ORACLE_DISTANCE) == set(egc.BY_NAME)
    assert egc.MAX_ORACLE_DISTANCE == max(egc.ORACLE_DISTANCE.values())
    assert egc.KERNEL_REL == 64 * egc.MAX_ORACLE_DISTANCE and egc.KERNEL_REL < 1e-11


def test_model_known_answers():
    LD = egc.LD
    # one row (p, z) from equal starts: a_j is proportional to P_j^n after n iterations
    one = egc.EmModel(np.array([[0.75, 0.25]]), np.array([8.0]))
    r = one.run(1, 0.0)
    assert r.iterations == 1 and abs(r.abundances[0] - LD(6)) < 1e-17 and abs(r.noise_count - LD(2)) < 1e-17 and r.total == 8
    r = one.run(3, 0.0)
    assert r.iterations == 3 and abs(r.abundances[0] - LD(8) * 27 / 28) < 1e-17 and abs(r.noise_count - LD(8) / 28) < 1e-17
    r = one.run()   # the noise, about 3^-n, changes by a factor of 3 per iteration while it is live: below 1e-8 from n = 17 on
    assert r.iterations == 26 and abs(r.abundances[0] - LD(8) / (1 + LD(3) ** -26)) < 1e-17
    # all mass on noise: no row touches the path — its abundance is 0 after one iteration (a violation: the noise went
    # from 1/2 to 1), the counts are Z, and the next ten iterations change nothing
    none = egc.EmModel(np.array([[0.0, 0.3], [0.0, 1.0]]), np.array([5.0, 2.0]))
    assert none.Z == 7 and len(none.count) == 0
    r = none.run()
    assert r.iterations == 11 and r.abundances[0] == 0 and not r.live[0] and abs(r.noise_count - LD(7)) < 1e-17
    # max_em_its = 1 on two rows: a' = a0 sum_i c_i P_ij / (a0 sum_k P_ik) / T = sum_i c_i P_ij / T for rows that sum to 1
    P = np.array([[0.5, 0.25, 0.25], [0.0, 0.5, 0.5]])
    r = egc.EmModel(P, np.array([3.0, 1.0])).run(1)
    assert r.iterations == 1 and np.allclose(r.abundances.astype(float), [1.5, 1.25], rtol=1e-15) and abs(float(r.noise_count) - 1.25) < 1e-15
    # the start vector is 1 / float(C), widened: visible where the rows do not sum to 1
    r = egc.EmModel(np.array([[0.5, 0.2]]), np.array([1.0])).iterate(0)
    assert r[0] == LD(np.float64(np.float32(0.5)))
    assert egc.EmModel(np.ones((1, 3)) / 3, np.ones(1)).iterate(0)[0] == LD(np.float64(np.float32(1) / np.float32(3)))
    # a count-0 row takes no part, whatever it holds
    a = egc.EmModel(np.array([[0.5, 0.5], [0.9, 0.1]]), np.array([4.0, 0.0])).run(3, 0.0)
    b = egc.EmModel(np.array([[0.5, 0.5]]), np.array([4.0])).run(3, 0.0)
    assert np.array_equal(a.abundances, b.abundances) and a.noise_count == b.noise_count
    # the stop rule: a violation resets the count of converged iterations; the gap is that of the deciding comparison
    slow = egc.BY_NAME["csr_rows3"].model().run()
    assert slow.iterations > 10 and 0 < slow.gap < float("inf")
