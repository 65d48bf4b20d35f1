"""The plan of the read rows (rpvg_amd/csrc/rows_plan.hpp) checked without a GPU: tests/cpp/rows_plan_check.cpp compares every
refusal of the alignment upload (code and text), the cluster of every read, the output columns, the split of the reads between the
two row kernels and the upload's byte figure, the lists and the launch sequence of the row sort at the edges of its tiers, alone
and mixed, and the launch shapes of the row kernels and the pack with the arithmetic the entry points carried before, written out
literally; and replays the planned launches on the host, with the kernels' guards restated, as a sorting network: every cluster of
a call ends sorted and a permutation of its input.  Built against rows_plan.hpp and include/rpvg_rows.h alone, with the address
and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _rows_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "rows_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "rows_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_plan_restates_the_upload_and_the_sort_and_its_launches_sort_every_cluster():
    done = subprocess.run([_rows_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
