"""The plan of the rows text (rpvg_amd/csrc/rows_text_plan.hpp) checked without a GPU: tests/cpp/rows_text_plan_check.cpp compares
rowBytes and rowWrite with lines built by snprintf, bare and ranked, at 8, 12 and 17 digits, walks the kernels' wavefront (blockWalk:
the code the measure and the write kernel run) lane by lane with a counter behind every byte of the text at every residue of its
start modulo 4 — names up to 4 000 bytes, a row of 1 000 indices, lines that end inside, at and just behind a step of 64 cells,
skipped clusters — and holds formatU64 to snprintf("%llu") at every digit count.  Built against the plan header alone, with the
address and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _rows_text_plan_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "rows_text_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "rows_text_plan_check.cpp"),
                           "-o", binary])
    return binary


def test_lines_and_the_wavefront_walk_store_every_byte_once():
    done = subprocess.run([_rows_text_plan_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", (done.stdout + done.stderr)[-2000:]
