"""CPU checks of the set text (include/rpvg_text.h, rpvg_hip_estimates_set_text): the plain-Python model of tests/set_text_model.py
against rows written out by hand for both kinds and against the bytes the writers' addEstimates() write, the set row descriptor
and the write kernel's wavefront walked on the CPU under the sanitizers (tests/cpp/set_text_plan_check.cpp), the writers' addText()
and addTable() (tests/cpp/set_text_writers_check.cpp), and the conditions the cases of tests/test_hip_set_text.py rest on."""
import math
import os
import subprocess

import numpy as np

from tests import set_text_model as S
from tests import table_text_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build(name, sources, extra=()):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, name)
    host = os.path.join(ROOT, "rpvg_amd", "host")
    subprocess.check_call(SANITIZE + ["-I" + os.path.join(ROOT, "rpvg_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), "-I" + host] + list(extra) + sources + ["-o", binary, "-lz"])
    return binary


def test_hand_rows_at_ploidy_2():
    """A heterozygous, a homozygous and a one-member set; a set below min_posterior has no bytes."""
    flat, member_tpm, names, ids, min_posterior, joint, posterior = S.hand_ploidy_2()
    got, off = S.set_text(S.JOINT, flat, member_tpm, names, ids, 2, min_posterior)
    rows = joint.splitlines(True)
    assert got == joint and off.tolist() == [0, len(rows[0]), len(rows[0]) + len(rows[1]), len(joint), len(joint)]
    got, off = S.set_text(S.POSTERIOR, flat, None, names, ids, 2, min_posterior)
    assert got == posterior and int(off[-1]) == len(posterior) and off[3] == off[4]


def test_hand_rows_at_ploidy_3():
    """Two pads behind a one-member set, names and pairs; a cluster without sets."""
    flat, member_tpm, names, ids, min_posterior, joint, posterior = S.hand_ploidy_3()
    assert S.set_text(S.JOINT, flat, member_tpm, names, ids, 3, min_posterior)[0] == joint
    assert S.set_text(S.POSTERIOR, flat, None, names, ids, 3, min_posterior)[0] == posterior


def test_the_filter_of_the_model():
    """Printed iff not (p < min_posterior): the threshold itself, either zero and both NaNs are printed, one ulp below is not."""
    flat = dict(cluster_path_off=[0, 1], set_off=[0, 7], member_off=list(range(8)), members=[0] * 7,
                posteriors=[0.25, float(np.nextafter(0.25, 0.0)), 0.0, -0.0, M.NAN, M.NEG_NAN, 1.0])
    text, off = S.set_text(S.POSTERIOR, flat, None, ["n"], [3], 1, 0.25)
    assert text == b"n\t3\t0.25\nn\t3\tnan\nn\t3\t-nan\nn\t3\t1\n" and np.diff(off.astype(np.int64)).tolist() == [9, 0, 0, 0, 8, 9, 6]
    text, off = S.set_text(S.POSTERIOR, flat, None, ["n"], [3], 1, 0.0)
    assert text == b"n\t3\t0.25\nn\t3\t0.25\nn\t3\t0\nn\t3\t-0\nn\t3\tnan\nn\t3\t-nan\nn\t3\t1\n"


def test_the_descriptor_and_the_wavefront_walk():
    binary = build("set_text_plan_check", [os.path.join(ROOT, "tests", "cpp", "set_text_plan_check.cpp")])
    run = subprocess.run([binary], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_the_writers_under_the_sanitizers_and_the_model_against_add_estimates(tmp_path):
    """tests/cpp/set_text_writers_check.cpp; then the model against the files addEstimates() and addTable() wrote there: the rows
    behind the header are the model's bytes for the same estimates (which the program derives from the ploidy as written below)."""
    host = os.path.join(ROOT, "rpvg_amd", "host")
    sources = [os.path.join(ROOT, "tests", "cpp", "set_text_writers_check.cpp"), os.path.join(host, "io", "estimates_writers.cpp"),
               os.path.join(host, "io", "cluster_io.cpp"), os.path.join(host, "read_path_probabilities.cpp")]
    binary = build("set_text_writers_check", sources, extra=["-Wno-sign-compare"])
    run = subprocess.run([binary, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
    hard = [1.5, 0.0, 123456785.0, 2.5e-10, 99999999.5, 10000000.5, -0.0, 1e22, 1.0 / 3.0]
    names, ids, paths_of = ["tx_a", "", "hap|3", "x", "n" * 300], [7, 8, 4000000000], [3, 0, 2]
    for ploidy in (1, 2, 3):
        salt, clusters = ploidy, []
        for k, paths in enumerate(paths_of):
            sets, posteriors, abundances = [], [], []
            for n in range(1, ploidy + 1 if paths else 1):
                for variant in range(3):
                    sets.append([paths - 1 - (j + n) % paths if variant == 0 else (paths - 1 if variant == 1 else (1 if j % 2 == 0 else 0)) for j in range(n)])
                    salt += 1
                    posteriors.append(0.001 if salt % 5 == 0 else 0.125 * (1 + salt % 7))
                    abundances += [hard[(salt + j) % len(hard)] for j in range(n)]
            clusters.append(dict(sets=sets, posteriors=posteriors, abundances=abundances, num_paths=paths))
        clusters[0]["posteriors"][0:3] = [M.NAN, 0.125, float(np.nextafter(0.125, 0.0))]
        clusters[2]["posteriors"][-1] = M.NEG_NAN
        flat = dict(cluster_path_off=np.cumsum([0] + paths_of), set_off=np.cumsum([0] + [len(c["sets"]) for c in clusters]),
                    member_off=np.cumsum([0] + [len(s) for c in clusters for s in c["sets"]]), members=[p for c in clusters for s in c["sets"] for p in s],
                    posteriors=[p for c in clusters for p in c["posteriors"]], abund_off=np.cumsum([0] + [len(c["abundances"]) for c in clusters]),
                    abundances=[a for c in clusters for a in c["abundances"]])
        member_tpm = [hard[(m * 5 + ploidy) % len(hard)] * (1.0 if m % 2 == 0 else 3.25) for m in range(len(flat["members"]))]
        want = open(tmp_path / f"posterior_estimates{ploidy}.txt", "rb").read()
        text, off = S.set_text(S.POSTERIOR, flat, None, names, ids, ploidy, 0.125)
        assert want == S.header(S.POSTERIOR, ploidy) + text and off[3] == off[2] and off[1] > off[0] and off[2] > off[1]
        want = open(tmp_path / f"joint_table{ploidy}.txt", "rb").read()
        text, _ = S.set_text(S.JOINT, flat, member_tpm, names, ids, ploidy, 0.125)
        assert want.startswith(S.header(S.JOINT, ploidy) + text + b"Unknown\t") and want.count(b"\n") == text.count(b"\n") + 2


def test_what_the_device_cases_rely_on():
    """The names have the stated lengths, the every-size cluster holds every set size with unsorted and repeated members, and the hard
    cells hold ties of both parities, a carry that lengthens a cell, -0.0, a subnormal, inf and the longest cell."""
    assert [len(n) for n in M.names_of_lengths(S.NAME_LENGTHS)] == [0, 1, 3, 4, 5, 26, 27, 255]
    rng = np.random.default_rng(1)
    for ploidy in (1, 2, 3, 8):
        c = S.every_size_cluster(ploidy, 5, rng)
        assert {len(s) for s in c["sets"]} == set(range(1, ploidy + 1)) and len(c["abundances"]) == sum(len(s) for s in c["sets"])
        if ploidy >= 2:
            assert any(s[0] == s[1] for s in c["sets"] if len(s) >= 2) and any(s[0] > s[1] for s in c["sets"] if len(s) >= 2)
    assert {M.is_tie(v, 8) for v in M.TIES_8} == {(True, 0), (True, 1)} and {M.is_tie(v, 17)[1] for v in M.TIES_17} == {0, 1}
    assert M.fmt(99999999.5) == "1e+08" and M.fmt(0.000999999995) == "0.001" and M.fmt(1.99999995) == "2"   # carries
    assert M.fmt(9.99999995e+99) == "1e+100" and len(M.fmt(9.99999995e+99)) > len(M.fmt(1e+99))               # a carry that lengthens the cell
    assert M.fmt(-0.0) == "-0" and M.fmt(5e-324) == "4.9406565e-324" and M.fmt(math.inf) == "inf"
    assert len(M.fmt(M.LONGEST[0], 8)) == 15 and len(M.fmt(M.LONGEST[1], 17)) == 24
