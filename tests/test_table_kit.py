"""The pure part of what the device tables share (rpvg_amd/csrc/table_kit.hpp) checked without a GPU: tests/cpp/table_kit_check.cpp
round-trips the offender word for every reason in use at the indices 0, 1 and 2^31 - 1, checks that the minimum of two words is the
smaller index and then the smaller reason, that every cluster-kind word is below every block-kind word and that a reason out of range
decodes to 0; holds lastAtMost inside [0, n) on ascending, constant, descending and random contents and to a linear search on ascending
ones; and holds offsetsBad to its four clauses written out.  Built against table_kit.hpp alone, with the address and
undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess


def _table_kit_check():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "table_kit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rpvg_amd", "csrc"), os.path.join(root, "tests", "cpp", "table_kit_check.cpp"),
                           "-o", binary])
    return binary


def test_offender_word_last_at_most_and_offsets_test():
    done = subprocess.run([_table_kit_check()], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
