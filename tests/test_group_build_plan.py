"""The plan of the group matrix build (rpvg_amd/csrc/group_build_plan.hpp) checked without a GPU: tests/cpp/group_build_plan_check.cpp
compares refusals (code and text), the per-matrix arrays, the route and the work items of every matrix, the `~0` sentinels, the
totals, the grid, block and LDS of every launch and the upload's byte figure with the formulas buildGroups carried before, written
out literally, over a grid of shapes and at the edges of each formula, for the three kinds of columns and every setting of the
switches, and checks that every matrix sits in exactly one route with its chunks in order and that the offsets are disjoint,
ordered and add up.  Built against group_build_plan.hpp alone, with the address and undefined-behaviour sanitizers, as a program
of its own."""
import os
import subprocess


def _group_build_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "group_build_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "group_build_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_plan_restates_the_build_and_every_matrix_has_one_route():
    done = subprocess.run([_group_build_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
