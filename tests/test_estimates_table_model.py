"""The plain-Python model of the estimates table (tests/estimates_table_model.py) pinned to a case written out by hand from the
writer's lines and held against the existing writers, the conditions the cases of tests/test_hip_estimates_table.py rest on, and
the two host pieces that need no GPU — the route rule (rpvg_amd/csrc/estimates_plan.hpp) and the writers' addTable()
(rpvg_amd/host/io/estimates_writers.cpp) — under the sanitizers.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import estimates_table_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fmt(x):
    """std::setprecision(8) with default float formatting."""
    return "%.8g" % x


def test_hand_case_sets_00_01_2_101():
    """src/threaded_output_writer.cpp:346-432 by hand: a homozygous set counts once for the probability and twice for the read
    count, the unsorted {1,0,1} counts path 1 twice, a path of effective length 0 has no transcripts and is left out of the
    cluster's count."""
    clusters, ploidy, expected, denominator, expected_tpm = M.hand_case()
    got = M.table(clusters, ploidy)
    for name, want in expected.items():
        if isinstance(want, list):
            assert got[name].tolist() == want, name
        else:
            assert got[name] == want, name
    with_tpm = M.with_tpm(got, denominator)
    for name, want in expected_tpm.items():
        assert with_tpm[name].tolist() == want, name
    assert M.total_single_chain(clusters) == (7.625, 5)
    flat = M.flatten(clusters)
    assert flat["set_off"].tolist() == [0, 4] and flat["member_off"].tolist() == [0, 2, 4, 5, 8] and flat["abund_off"].tolist() == [0, 8]
    assert flat["members"].tolist() == [0, 0, 0, 1, 2, 1, 0, 1] and flat["cluster_path_off"].tolist() == [0, 3]


def test_a_cluster_without_abundances_and_invalid_counts():
    clusters, ploidy, expected, _, _ = M.hand_case()
    bare = dict(clusters[0], abundances=[])
    got = M.table([bare, clusters[0]], 4)
    assert got["haplotype_prob"].tolist() == expected["haplotype_prob"] * 2
    assert got["read_count"].tolist() == [0.0] * 3 + expected["read_count"]
    assert got["member_transcript_count"].tolist() == [0.0] * 8 + expected["member_transcript_count"]
    assert got["cluster_transcript_count"].tolist() == [0.0, 7.625] and got["noise_count_share_total"] == 1.5
    with pytest.raises(M.InvalidEstimates) as err:
        M.table([clusters[0], dict(clusters[0], abundances=clusters[0]["abundances"][:-1])], 2)
    assert err.value.cluster == 1
    with pytest.raises(M.InvalidEstimates):
        M.table([dict(clusters[0], sets=[(0, 3)], posteriors=[1.0], abundances=[1.0, 1.0])], 2)


def test_zero_denominator_gives_nan_where_the_count_is_zero_and_infinity_elsewhere():
    clusters, ploidy, _, _, _ = M.hand_case()
    t = M.with_tpm(M.table(clusters, ploidy), 0.0)
    assert [math.isnan(x) for x in t["tpm"]] == [False, True, False] and t["tpm"][0] == math.inf
    assert [math.isnan(x) for x in t["member_tpm"]] == [False, False, False, True, False, True, False, True]


def test_order_cases_tell_the_orders_apart():
    """The cases of the device test: a path with four memberships whose sequential, reversed and pairwise (tree) sums are three
    different doubles.  About one random list of four in a hundred qualifies (sums that differ do so by a unit in the last place,
    and three different values need two differences that do not cancel), so the cases are searched for and the property is asserted
    for each."""
    cases = M.three_sum_cases(7, 24)
    assert len(cases) == 24
    for values in cases:
        assert len(values) >= 3
        sums = {M.sequential_sum(values), M.reversed_sum(values), M.pairwise_sum(values)}
        assert len(sums) == 3, values
    rng = np.random.default_rng(1)
    share = sum(M.three_sums_differ([float(x) for x in rng.uniform(0.001, 1000.0, size=4)]) for _ in range(2000)) / 2000
    print("share of random lists of four with three different sums:", share)
    assert 0.002 < share < 0.05   # a binomial count with a mean near 20 of 2 000
    # in a cluster built around them the model's read count of the case's path is the sequential sum, and its memberships lie
    # more than 64 members apart
    cluster = M.order_cluster(cases[:5], num_paths=40, gap=40, rng=np.random.default_rng(2))
    t = M.table([cluster], 2)
    members = [p for s in cluster["sets"] for p in s]
    for i, values in enumerate(cases[:5]):
        assert t["read_count"][i] == M.sequential_sum(values)
        assert t["read_count"][i] != M.reversed_sum(values) and t["read_count"][i] != M.pairwise_sum(values)
        assert t["haplotype_prob"][i] == M.sequential_sum([v / 4096.0 for v in values])
        at = [m for m, p in enumerate(members) if p == i]
        assert len(at) == 4 and all(b - a > 64 for a, b in zip(at, at[1:]))


def test_the_cluster_sums_differ_from_the_single_chain_within_the_derived_bound():
    """total_transcript_count adds per cluster, then the clusters; totalTranscriptCount is one chain.  Both are sums of the same n
    non-negative terms, each within (n - 1) 2^-53 relative of the exact sum to first order: they differ by at most 2 (n - 1) 2^-53."""
    rng = np.random.default_rng(5)
    clusters = [M.random_cluster(rng, int(rng.integers(1, 30)), int(rng.integers(0, 40))) for _ in range(60)]
    t = M.table(clusters, 2)
    single, n = M.total_single_chain(clusters)
    assert n > 1000 and abs(t["total_transcript_count"] - single) <= 2 * (n - 1) * 2.0 ** -53 * single
    assert t["total_transcript_count"] == M.sequential_sum(t["cluster_transcript_count"].tolist())


@pytest.mark.parametrize("model", ["haplotype-transcripts", "transcripts"])
def test_existing_writers_print_the_model(tmp_path, model):
    """For a small_cases batch the text addEstimates() writes parses to the model's values at the 8 digits it prints."""
    from oracle import pyoracle
    from rpvg_amd import io as rio
    from rpvg_amd.batch import ClusterBatch, make_params
    from tests import small_cases
    orig = ClusterBatch.from_clusters(small_cases.make_batch_clusters(777, n_clusters=8, with_empty=False))
    probs, info = str(tmp_path / "probs.txt.gz"), str(tmp_path / "info.tsv")
    rio.write_batch_files(orig, probs, info)
    batch = rio.read_batch_files(probs, info)
    params = make_params()
    prefix = str(tmp_path / "out")
    with pyoracle.RawRun(model, params, batch, 2) as run:
        rio.write_estimates(probs, info, model, params, run.view, prefix, unaligned_read_count=0)
        clusters = M.from_estimates(batch, run.estimates)
    t = M.table(clusters, 2)
    single, _ = M.total_single_chain(clusters)   # the writers' denominator (src/main.cpp:1029-1057)
    t = M.with_tpm(t, single)
    lines = [line.split("\t") for line in open(prefix + ".txt").read().splitlines()]
    g = m = 0
    if model == "transcripts":
        for k, c in enumerate(clusters):
            for j in range(c["num_paths"]):
                assert lines[1 + g][4:] == [fmt(t["read_count"][g]), fmt(t["tpm"][g])], (k, j)
                assert t["tpm"][g] == t["member_tpm"][g]   # set i is {i}
                g += 1
        assert lines[1 + g][4] == fmt(t["noise_count_total"])
        return
    for k, c in enumerate(clusters):
        for j in range(c["num_paths"]):
            assert lines[1 + g][4:] == [fmt(t["haplotype_prob"][g]), fmt(t["read_count"][g]), fmt(t["tpm"][g])], (k, j)
            g += 1
    assert lines[1 + g][5] == fmt(t["noise_count_total"])
    joint = [line.split("\t") for line in open(prefix + "_joint.txt").read().splitlines()]
    row, m = 1, 0
    for k, c in enumerate(clusters):
        a = 0
        for s, post in zip(c["sets"], c["posteriors"]):
            if post >= params.prob_precision:
                want = []
                for i in range(len(s)):
                    want += [fmt(c["abundances"][a + i]), fmt(t["member_tpm"][m + i])]
                assert joint[row][4:4 + 2 * len(s)] == want, (k, s)
                row += 1
            a += len(s)
            m += len(s)
    assert joint[row][4] == fmt(t["noise_count_share_total"]) == joint[row][6]


def _sanitized(name, sources, includes):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-sign-compare", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + ["-I" + i for i in includes] + sources + ["-o", binary, "-lz"])
    return binary


def test_route_rule_under_the_sanitizers():
    """tests/cpp/estimates_plan_check.cpp: the route at limit - 1, limit and limit + 1 for paths and for members, at 0 paths, 0 members
    and the 32-bit edges, as a program of its own built with AddressSanitizer and UBSan."""
    binary = _sanitized("estimates_plan_check", [os.path.join(ROOT, "tests", "cpp", "estimates_plan_check.cpp")], [os.path.join(ROOT, "rpvg_amd", "csrc")])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
    wave_paths, wave_members, lds_paths, lds_members, wave_bytes, lds_bytes = (int(x) for x in subprocess.run([binary, "limits"], capture_output=True,
                                                                                                           text=True, check=True).stdout.split())
    assert wave_paths <= lds_paths and wave_members <= lds_members and lds_bytes <= 64 * 1024 and wave_bytes < lds_bytes


def test_add_table_writes_the_bytes_of_add_estimates_under_the_sanitizers(tmp_path):
    """tests/cpp/estimates_writers_check.cpp: the three writers, ploidy 1, 2 and 3, identical bytes; a set {1} at position 0 makes
    AbundanceEstimatesWriter::addTable throw."""
    host = os.path.join(ROOT, "rpvg_amd", "host")
    binary = _sanitized("estimates_writers_check", [os.path.join(ROOT, "tests", "cpp", "estimates_writers_check.cpp"), os.path.join(host, "io", "estimates_writers.cpp"),
                                                   os.path.join(host, "io", "cluster_io.cpp"), os.path.join(host, "read_path_probabilities.cpp")], [host])
    assert subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, check=True).stdout.strip() == "ok"
