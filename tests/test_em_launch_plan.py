"""The merged EM launches of a solve's plan (rpvg_amd/csrc/em_plan.hpp: EmSolveKnobs::merged_launches) checked without a GPU:
tests/cpp/em_launch_plan_check.cpp pins the tables for three and six side streams, with and without problems of more than 16
columns and of a problem too wide for LDS, the 256-thread launches (bin 2 on the main stream, bin 1 on a side stream) on both sides
of 40 KB of streamed vectors, the roles of every launch with their grids, and the tables of default-constructed knobs.  Built
against em_plan.hpp alone, with the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _em_launch_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "em_launch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "em_launch_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_merged_launch_tables_roles_and_default_tables():
    done = subprocess.run([_em_launch_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
