"""formatG and formatU32 of rpvg_amd/csrc/number_text.hpp, the cell of the table text: tests/cpp/number_text_check.cpp compares them
with glibc's snprintf byte for byte over the edges of the format (every precision 1 .. 17), ties and near-ties, carries across the
notation boundary and 1.3 * 10^7 random bit patterns, under the sanitizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_format_g_is_glibc_byte_for_byte():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "number_text_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "number_text_check.cpp"), "-o", binary])
    run = subprocess.run([binary], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
    compared, exact, odd, even = (int(x) for x in re.match(r"ok (\d+) compared, (\d+) by the exact comparison .* ties: (\d+) from odd digits, (\d+) from even", run.stdout).groups())
    assert compared >= 13_000_000 + 2 * 3 * 2000 * 500 and exact >= odd + even and odd > 0 and even > 0
