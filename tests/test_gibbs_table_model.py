"""CPU checks of the Gibbs samples table (include/rpvg_samples.h): the plain-Python model of tests/gibbs_table_model.py against a
case written out by hand from the writer's lines and against ReadCountGibbsSamplesWriter itself, the writer's addTable() against its
addSamples() and the decisions of the plan under the sanitizers, and the conditions the cases of tests/test_hip_gibbs_table.py
rest on."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from rpvg_amd.gibbs_table import FlatGibbs, limits
from tests import gibbs_table_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_case_blocks_02_empty_12():
    """rpvg_amd/host/io/estimates_writers.cpp:487-583 by hand: path 1 is listed only through the third block, the block without
    samples shifts no column, the fourth column is the tail, and the cluster without blocks adds its total_count to every column."""
    clusters, N, expected = M.hand_case()
    got = M.table(clusters, N)
    assert got["samples"].tolist() == expected["samples"]
    assert got["listed"].tolist() == expected["listed"]
    assert got["noise_counts"].tolist() == expected["noise_counts"]
    flat = FlatGibbs(**M.flatten(clusters, N))
    assert flat.sizes() == dict(num_clusters=2, num_blocks=3, num_paths=5, num_gibbs_samples=4, num_path_ids=5, num_noise_samples=3,
                                num_abundance_samples=6)
    assert flat.gibbs_off.tolist() == [0, 3, 3] and flat.gibbs_noise_off.tolist() == [0, 2, 2, 3] and flat.gibbs_abund_off.tolist() == [0, 4, 4, 6]
    assert M.text(clusters, N, ["a", "b", "c", "d", "e"], [7, 9], 2).splitlines()[1:] == [
        "a\t7\t10\t11\t0\t0", "b\t7\t0\t0\t20.5\t0", "c\t7\t30\t31\t32.5\t0", "Unknown\t0\t10.5\t11.5\t13.25\t109"]


def test_every_scatter_case_has_distinct_non_zero_sources():
    """A cell read from the wrong place, or left unwritten, cannot compare equal."""
    cases = M.scatter_cases(limits())
    assert set(cases) >= {"widths_and_counts", "tails", "one_sample", "many_blocks", "odd_clusters", "single_cluster", "empty_batch", "route_limits"}
    for name, (clusters, N) in cases.items():
        values = M.source_values(clusters)
        assert all(v != 0.0 for v in values) and len(set(values)) == len(values), name
        assert all(sum(len(b["noise"]) for b in c["blocks"]) <= N for c in clusters), name
        if name != "empty_batch":
            assert len(values) > 0, name
    lim = limits()
    widths = {len(b["ids"]) for c in cases["widths_and_counts"][0] for b in c["blocks"]}
    counts = {len(b["noise"]) for c in cases["widths_and_counts"][0] for b in c["blocks"]}
    assert widths >= {1, 2, 31, 32, 33, 63, 64, 65} and counts >= {1, 63, 64, 65, lim.sample_tile - 1, lim.sample_tile + 1}
    tails, N = cases["tails"]
    sums = [sum(len(b["noise"]) for b in c["blocks"]) for c in tails]
    assert sums[:3] == [N, N - 1, 0] and len(tails[2]["blocks"]) == 2
    assert cases["one_sample"][1] == 1 and len(cases["many_blocks"][0][0]["blocks"]) == 200


@pytest.mark.parametrize("K", [1, 2, 64, 65, 257])
def test_noise_cases_tell_the_orders_apart(K):
    """For three clusters and more some column's chain differs in its last bits from the reversed chain and from a pairwise sum, so a
    tree on the device cannot pass.  With one or two clusters a column has at most two addends after the 0.0 and every order gives
    the same double (a + b is b + a): those cases check the loop's ends, not its order."""
    clusters, N, seed = M.noise_case(K)
    assert len(clusters) == K and seed < 50
    values = [x for c in clusters for b in c["blocks"] for x in b["noise"]] + [c["total_count"] for c in clusters]
    assert min(values) >= 1e-3 and max(values) <= 1e9 and (K < 64 or (min(values) < 1e-1 and max(values) > 1e7))
    if K >= 3:
        assert M.order_matters(clusters, N)
        got = M.table(clusters, N)["noise_counts"]
        differing = [s for s in range(N) if got[s] != M.reversed_sum(M.column_addends(clusters, N, s)) and got[s] != M.pairwise_sum(M.column_addends(clusters, N, s))]
        assert differing and all(got[s] == M.sequential_sum(M.column_addends(clusters, N, s)) for s in range(N))
    else:
        assert not M.order_matters(clusters, N)


def _sanitized(name, sources, includes):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-sign-compare", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + ["-I" + i for i in includes] + sources + ["-o", binary, "-lz"])
    return binary


def test_plan_decisions_under_the_sanitizers():
    """tests/cpp/gibbs_table_plan_check.cpp: the route at limit - 1, limit and limit + 1 for paths and for columns, at 0 paths, 0 blocks
    and the 32-bit edges, as a program of its own built with AddressSanitizer and UBSan; its limits are the library's."""
    binary = _sanitized("gibbs_table_plan_check", [os.path.join(ROOT, "tests", "cpp", "gibbs_table_plan_check.cpp")], [os.path.join(ROOT, "rpvg_amd", "csrc")])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
    plan = [int(x) for x in subprocess.run([binary, "limits"], capture_output=True, text=True, check=True).stdout.split()]
    lim = limits()
    assert plan == [lim.resident_paths, lim.resident_columns, lim.sample_tile, lim.global_paths, lim.resident_lds_bytes]


def _read_containers(filename):
    clusters, names, ids = [], [], []
    for line in open(filename):
        word, _, rest = line.rstrip("\n").partition(" ")
        if word == "cluster":
            cluster_id, num_paths, total = rest.split()
            clusters.append(dict(num_paths=int(num_paths), total_count=float(total), blocks=[]))
            ids.append(int(cluster_id))
        elif word == "path":
            names.append(rest)
        elif word == "block":
            c, n = (int(x) for x in rest.split())
            clusters[-1]["blocks"].append(dict(c=c, n=n))
        elif word == "ids":
            clusters[-1]["blocks"][-1]["ids"] = [int(x) for x in rest.split()]
        elif word == "noise":
            clusters[-1]["blocks"][-1]["noise"] = [float(x) for x in rest.split()]
        elif word == "abund":
            block = clusters[-1]["blocks"][-1]
            flat = [float(x) for x in rest.split()]
            assert len(flat) == block["c"] * block["n"] and len(block["ids"]) == block["c"] and len(block["noise"]) == block["n"]
            block["abund"] = [flat[s * block["c"]:(s + 1) * block["c"]] for s in range(block["n"])]
    return clusters, names, ids


def test_add_table_writes_the_bytes_of_add_samples_under_the_sanitizers(tmp_path):
    """tests/cpp/gibbs_writer_check.cpp: identical file bytes for one table per writer, the rows identical and the noise totals in
    another order for two.  The file of the one-table case is also the model's text: every number as `%.8g`."""
    host = os.path.join(ROOT, "rpvg_amd", "host")
    binary = _sanitized("gibbs_writer_check", [os.path.join(ROOT, "tests", "cpp", "gibbs_writer_check.cpp"), os.path.join(host, "io", "estimates_writers.cpp"),
                                              os.path.join(host, "io", "cluster_io.cpp"), os.path.join(host, "read_path_probabilities.cpp")], [host])
    assert subprocess.run([binary, str(tmp_path)], capture_output=True, text=True, check=True).stdout.strip() == "ok"
    clusters, names, ids = _read_containers(tmp_path / "one_table_containers.txt")
    assert len(clusters) == 23 and any(len(b["noise"]) == 0 for c in clusters for b in c["blocks"]) and any(not c["blocks"] for c in clusters)
    written = gzip.open(tmp_path / "one_table.txt.gz", "rt").read()
    assert written == M.text(clusters, 11, names, ids, unaligned_read_count=11)
    assert len(written.splitlines()) > 30
