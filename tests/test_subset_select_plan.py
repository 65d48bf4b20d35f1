"""The index logic of the subset selection (rpvg_amd/csrc/subset_select_plan.hpp) checked without a GPU:
tests/cpp/subset_select_check.cpp runs the steps the kernels run — the sort of the selected diplotypes by (hash, length, index),
the runs' first positions, the leaders, the members' sums, the key of the leading elements and the rank of the retained lists —
on host arrays against a quadratic model: random lists around every size of the network, equal hashes with different lists,
equal leading keys with a difference in the tail, lists that are prefixes of others, one selected diplotype, all identical.
Built with the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _subset_select_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "subset_select_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "subset_select_check.cpp"),
                           "-o", binary])
    return binary


def test_leaders_members_and_ranks_equal_the_quadratic_model():
    done = subprocess.run([_subset_select_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
