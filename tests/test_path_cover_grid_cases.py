"""CPU checks of the minimum path cover's whole-GPU route: the decision margin of every case of
tests/path_cover_grid_cases.py in the plain-Python model, what each kind of case is there for, and the route rule
(rpvg_amd/csrc/cover_plan.hpp) walked by a program of its own under AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

import pytest

from rpvg_amd import hip
from tests import path_cover_cases as pcc
from tests import path_cover_grid_cases as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", grid.CASES + [grid.THRESHOLD_CASE], ids=lambda c: c.name)
def test_every_case_has_the_margin(case):
    m = case.model()
    print(case.name, "margin", m.margin, "cover", len(m.cover))
    assert m.margin >= pcc.MIN_MARGIN, (case.name, m.margin)


@pytest.mark.parametrize("case", [c for c in grid.CASES if c.kind in ("grid_wide", "grid_tall")] + [grid.THRESHOLD_CASE], ids=lambda c: c.name)
def test_the_cover_of_a_planted_case_is_the_planted_paths(case):
    cl = case.cluster()
    assert case.model().cover == pcc.wide_planted(cl.n_paths)
    if case.kind == "grid_tall":   # a planted column is a chain of exactly L terms
        chain = int(case.name.rsplit("_", 1)[1])
        cols = pcc.columns(cl)
        assert [len(cols[j]) for j in pcc.wide_planted(cl.n_paths)] == [chain] * 8


def test_the_widest_workgroup_cluster_plus_one_path_is_the_first_wide_case():
    n = grid.WIDE_PATHS[0]
    assert n == pcc.MAX_PATHS + 1 == grid.MAX_WORKGROUP_PATHS + 1
    # the planted path n - 1 is index 9 600, the first the workgroup route cannot hold
    assert pcc.MAX_PATHS in grid.BY_NAME[f"grid_wide_{n}"].model().cover


def test_long_covers_end_either_side_of_a_look_at_the_control_record():
    lengths = [len(c.model().cover) for c in grid.CASES if c.kind == "grid_long_cover"]
    assert lengths == [grid.CHUNK - 1, grid.CHUNK, grid.CHUNK + 1, 2 * grid.CHUNK + 1]
    for c in grid.CASES:
        if c.kind == "grid_long_cover":
            assert sorted(c.model().order) == c.model().cover and c.model().order != c.model().cover   # (chosen in a random order)


@pytest.mark.parametrize("case", grid.TWIN_CASES, ids=lambda c: c.name)
def test_twins_sit_at_the_edges_of_the_pick_kernel_and_the_model_keeps_the_first(case):
    first, second = case.twins
    assert grid.twin_ok(case.cluster(), first, second)
    assert pcc.twin_classes(case.cluster())[second] == first
    tile, block = grid.PICK_TILE, grid.PICK_BLOCK
    where = {"last_thread_and_first_of_the_next_workgroup": first // tile + 1 == second // tile and first % tile == tile - 1 and second % tile == 0,
             "end_of_a_stride_and_the_next_workgroup": first // tile < second // tile and first % block == block - 1 and second % tile == 0,
             "second_and_third_workgroup": first // tile == 1 and second // tile == 2,
             "first_and_last_workgroup": first // tile == 0 and second // tile == (grid.TWIN_PATHS - 1) // tile,
             "both_on_one_thread": first // tile == second // tile and first % block == second % block}
    assert where[case.name[len("grid_twins_"):]]


def test_the_threshold_cluster_is_narrow_and_its_work_is_what_the_plan_counts():
    cl = grid.THRESHOLD_CASE.cluster()
    assert cl.n_paths <= grid.MAX_WORKGROUP_PATHS and len(cl.rows) == grid.THRESHOLD_ROWS
    batch = pcc.batch_of([cl])
    assert grid.work_of(cl) == batch.num_rows + len(batch.path_idx)   # rows + entries of the uploaded batch
    # R terms of one sign per weight: R * 2^-53 relative, two orders of magnitude below the margin up to 10^5 rows
    assert grid.THRESHOLD_ROWS * 2.0 ** -53 < 1e-2 * pcc.MIN_MARGIN and 1e5 * 2.0 ** -53 < 2e-2 * pcc.MIN_MARGIN


def test_random_small_clusters_are_small_and_fixed():
    assert len(grid.RANDOM_SEEDS) == 200
    for seed in grid.RANDOM_SEEDS[:20]:
        cl = grid.random_small_cluster(seed)
        assert 2 <= cl.n_paths <= 40 and 1 <= len(cl.rows) <= 300
    assert grid.random_small_cluster(8200).rows == grid.random_small_cluster(8200).rows


def test_route_rule_under_the_sanitizers():
    """tests/cpp/cover_plan_check.cpp: the route at limit - 1, limit and limit + 1 paths, at threshold - 1 and threshold, at the three
    special threshold values, at one path and at the 31-bit edges, as a program of its own built with AddressSanitizer and UBSan;
    the plan's numbers are the library's."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "cover_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "cover_plan_check.cpp"),
                           "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
    plan = [int(x) for x in subprocess.run([binary, "limits"], capture_output=True, text=True, check=True).stdout.split()]
    lim = hip.cover_limits()
    assert plan == [lim.workgroup_max_paths, lim.chunk_rounds, lim.default_grid_min_work, lim.grid_max_rows, lim.grid_max_entries, lim.pick_block,
                    lim.pick_per_thread, lim.pick_max_blocks, lim.strike_block, lim.strike_max_blocks, lim.hist_max_paths]
    assert lim.workgroup_max_paths == pcc.MAX_PATHS and lim.grid_max_rows == lim.grid_max_entries == 2 ** 31 - 1
