"""The functions of rpvg_amd/csrc/rows_parse_plan.hpp under ASan + UBSan (tests/cpp/rows_parse_plan_check.cpp): every text of
tests/rows_parse_cases.py, accepted and refused, through the kernels' per-byte functions with every array and the text itself in heap
blocks of exactly their sizes.  The totals, the bytes of the names, the exact tokens and the refusal (line, reason) are the model's."""
import os
import subprocess

from tests import rows_parse_cases as cases
from tests import rows_parse_model as P
from tests.test_rows_parse_model import ACCEPTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_under_the_sanitizers(tmp_path):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "rows_parse_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-DRPVG_NUMBER_TEXT_CHECKED", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "rpvg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rows_parse_plan_check.cpp"), "-o", binary])
    # truncations of a valid text too: every prefix ends a line, a field or a token somewhere
    whole = cases.STRUCTURE["names with commas and colons"] + b"# 1 2\nx,1,2\n7 0.5 0.25:0 0.5:0,0\n"
    texts = list(ACCEPTED.values()) + list(cases.REFUSALS) + [whole[:n] for n in range(len(whole))]
    with open(tmp_path / "texts", "wb") as f:
        for text in texts:
            f.write(b"%d\n" % len(text) + text)
    run = subprocess.run([binary, str(tmp_path / "texts")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(texts)
    for text, line in zip(texts, lines):
        try:
            flat = P.parse(text)
        except P.Refused as refused:
            assert line == f"refused {refused.line} {refused.why}", text
            continue
        want = [len(flat["has_rank_key"]), len(flat["path_length"]), len(flat["row_count"]), len(flat["grp_prob"]), len(flat["path_idx"]), len(flat["name_bytes"])]
        assert line.split()[:7] == ["ok"] + [str(x) for x in want], text
    assert int(lines[list(ACCEPTED).index("hard tokens")].split()[7]) == 2 * len(cases.SLOW)
