"""CPU checks of the table text (include/rpvg_text.h): the plain-Python model of tests/table_text_model.py against rows written out
by hand for each of the three files, the row descriptor and the write kernel's wavefront walked on the CPU under the sanitizers
(tests/cpp/table_text_plan_check.cpp), and the conditions the cases of tests/test_hip_table_text.py rest on."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import table_text_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(name, extra=()):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rpvg_amd", "host")] + list(extra) + [os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", binary])
    run = subprocess.run([binary], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_hand_case_of_the_gibbs_file():
    table, cluster_path_off, names, ids, text, row_off = M.hand_gibbs()
    got, off = M.gibbs_text(table, cluster_path_off, names, ids)
    assert got == text and off.tolist() == row_off


def test_hand_case_of_the_two_estimates_files():
    flat, table, names, lengths, ids, per_path, haplotype = M.hand_estimates()
    assert M.estimates_text(M.PER_PATH, flat, table, names, lengths, ids)[0] == per_path
    got, off = M.estimates_text(M.HAPLOTYPE, flat, table, names, lengths, ids)
    assert got == haplotype and off.tolist() == [0, len(haplotype.splitlines(True)[0]), len(haplotype)]
    flat["members"] = [1, 0]
    with pytest.raises(ValueError, match="cluster 0"):
        M.estimates_text(M.PER_PATH, flat, table, names, lengths, ids)


def test_the_format_of_the_contract():
    for v, text in ((123456785.0, "1.2345678e+08"), (123456795.0, "1.234568e+08"), (99999999.5, "1e+08"), (float(np.nextafter(0.0000999999995, 1.0)), "0.0001"),
                    (0.0000999999995, "9.9999999e-05"), (1e-5, "1e-05"), (M.from_bits(2024), "9.9998887e-321"), (-0.0, "-0"), (M.NAN, "nan"), (M.NEG_NAN, "-nan"),
                    (float("-inf"), "-inf"), (5e-324, "4.9406565e-324")):
        assert M.fmt(v) == text
    assert M.fmt(-1.2345678901234567e-308, 17) == "-1.2345678901234567e-308"


def test_the_descriptor_and_the_wavefront_walk():
    build_and_run("table_text_plan_check")


def test_add_text_writes_the_bytes_of_add_table_under_the_sanitizers(tmp_path):
    """tests/cpp/table_text_writers_check.cpp: the three writers' addText() fed with the host line against their addTable()."""
    host = os.path.join(ROOT, "rpvg_amd", "host")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "table_text_writers_check")
    sources = [os.path.join(ROOT, "tests", "cpp", "table_text_writers_check.cpp"), os.path.join(host, "io", "estimates_writers.cpp"),
               os.path.join(host, "io", "cluster_io.cpp"), os.path.join(host, "read_path_probabilities.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-sign-compare", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + host, "-I" + os.path.join(ROOT, "rpvg_amd", "csrc")]
                          + sources + ["-o", binary, "-lz"])
    run = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
    rows = open(tmp_path / "haplotype_text.txt", "rb").read().splitlines()
    assert rows[1] == b"tx_a\t7\t1000\t812.25\t1\t12\t1000000" and rows[2] == b"\t7\t20\t1e-07\t0.33333333\t1e+08\t0.125" and len(rows) == 7


def test_what_the_device_cases_rely_on():
    """The tie cells are ties of both parities, the names have the stated lengths and the longest cells are the longest."""
    assert [M.is_tie(v, 8) for v in M.TIES_8] == [(True, 0), (True, 1), (True, 0), (True, 1), (True, 1)]
    assert all(M.is_tie(v, 17)[0] for v in M.TIES_17) and {M.is_tie(v, 17)[1] for v in M.TIES_17} == {0, 1}
    assert not any(M.is_tie(v, 8)[0] for v in (0.0000999999995, 1.99999995, 9.99999995e+99, 0.000999999995))
    assert [M.fmt(v) for v in M.CARRIES] == ["0.0001", "9.9999999e-05", "2", "1e+100", "0.001", "100000", "1e+09"]
    assert [len(n) for n in M.names_of_lengths(M.NAME_LENGTHS)] == [0, 1, 3, 4, 5, 255]
    assert len(M.fmt(M.LONGEST[0], 8)) == 15 and len(M.fmt(M.LONGEST[1], 17)) == 24
    assert all(len(M.fmt(v, p)) <= 24 for v in M.HARD_CELLS + [-v for v in M.HARD_CELLS] for p in (8, 17))
    assert sum(1 for v in M.HARD_CELLS if math.isfinite(v) and v != 0 and M.is_tie(v, 8)[0]) >= 3
