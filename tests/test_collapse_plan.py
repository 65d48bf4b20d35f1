"""The plan of the row collapse (rpvg_amd/csrc/collapse_plan.hpp) checked without a GPU: tests/cpp/collapse_plan_check.cpp
compares refusals, route, the layout of the info block, every buffer count, the radix sort's bits, the merge rounds and the grid
and block of every launch with the formulas the launch code carried before, written out literally, over a grid of shapes and
at the edges of each formula, and checks that the info block's regions are disjoint, ordered and add up.  Built against
collapse_plan.hpp and segment_sort_plan.hpp alone, with the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _collapse_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "collapse_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "collapse_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_plan_restates_the_launch_code_and_the_info_block_is_well_formed():
    done = subprocess.run([_collapse_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
