"""The schedule of the row collapse's segment sort (rpvg_amd/csrc/segment_sort_plan.hpp) checked without a GPU:
tests/cpp/segment_sort_check.cpp runs it on host arrays — lanes and wavefronts simulated, in-lane, in-wavefront and
across-wavefront stages taken as the header says — for every size class, lengths around every class boundary and the chunk
length, random, sorted, reversed and organ-pipe orders, words that differ in one half only and 0xFF..FE next to the padding, and
the merge rounds with their two buffers for 1 .. 9 and 2^k +- 1 chunks, against std::sort.  Built with the address and
undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _segment_sort_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "segment_sort_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "segment_sort_check.cpp"),
                           "-o", binary])
    return binary


def test_schedule_sorts_every_size_class_and_the_rounds_end_in_the_right_buffer():
    done = subprocess.run([_segment_sort_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
