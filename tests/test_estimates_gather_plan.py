"""The plan of the resident-estimates gather (rpvg_amd/csrc/estimates_gather_plan.hpp) checked without a GPU:
tests/cpp/estimates_gather_plan_check.cpp holds the size rule of a set slot in both forms, gatherModel on a hand-written case of both
forms with every output array written out, and every refusal with the smallest offending (part, unit) reported when two are planted;
its parts live in memory exactly as long as their sizes say.  Built against the plan header alone, with the address and
undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _estimates_gather_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "estimates_gather_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "estimates_gather_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_model_hand_case_and_every_refusal():
    done = subprocess.run([_estimates_gather_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", (done.stdout + done.stderr)[-2000:]
