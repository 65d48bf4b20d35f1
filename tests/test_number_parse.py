"""parseDouble and parseU64 of rpvg_amd/csrc/number_parse.hpp, the cell of the rows parse: tests/cpp/number_parse_check.cpp compares
parseDouble with glibc's strtod bit for bit over 1.7 * 10^8 "%.{p}g" texts of random bit patterns, the 17- to 19-digit decimals on
either side of the middle of 10^6 adjacent pairs of doubles, exact ties, both ends of the range and every malformed form, under the
sanitizers and with the overflow trap of the exact comparison's words compiled in.  The brackets of a middle are checked here, on
a sample, with Python's exact fractions: float() sends them to the lower and the upper neighbour."""
import os
import random
import re
import struct
import subprocess
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_double_is_strtod_bit_for_bit():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "number_parse_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-pthread", "-DRPVG_NUMBER_TEXT_CHECKED", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "number_parse_check.cpp"), "-o", binary])
    run = subprocess.run([binary], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
    compared, exact, ties = (int(x) for x in re.match(r"ok (\d+) compared, (\d+) by the exact comparison, (\d+) ties among them", run.stdout).groups())
    # 17 texts of 10^7 patterns, two brackets at three lengths of most of 10^6 pairs, and every tie went the slow way
    assert compared >= 17 * 10_000_000 + 2 * 3 * 900_000 and ties >= 200_003 and exact >= ties


def test_brackets_of_a_middle_go_to_the_neighbours():
    """The construction of the C++ check, on a sample, with exact arithmetic: the D-digit floor and ceiling of the middle of two
    adjacent doubles are decimals that float() sends to the lower and to the upper one."""
    rng = random.Random(7)
    checked = 0
    for _ in range(2000):
        bits = rng.getrandbits(63)
        if (bits >> 52) >= 0x7fe:
            continue
        a, b = (struct.unpack("<d", struct.pack("<Q", x))[0] for x in (bits, bits + 1))
        middle = (Fraction(a) + Fraction(b)) / 2
        if middle == 0:
            continue
        k = len(str(middle.numerator)) - len(str(middle.denominator))  # the decimal exponent, or one above it
        for D in (17, 18, 19):
            q = k - (D - 1)  # w = floor(middle / 10^q) has D digits
            w = 0
            while not 10 ** (D - 1) <= w < 10 ** D:
                q += 1 if w >= 10 ** D else (-1 if w else 0)
                scaled = middle / Fraction(10) ** q
                w = scaled.numerator // scaled.denominator
            if Fraction(w) == scaled or w + 1 >= 10 ** 19:
                continue
            assert float(f"{w}e{q}") == a and float(f"{w + 1}e{q}") == b
            checked += 1
    assert checked > 5000
