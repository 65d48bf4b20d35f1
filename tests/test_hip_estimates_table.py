"""The estimates table on the GPU (rpvg_amd/csrc/estimates_table.hip, include/rpvg_table.h) against the plain-Python model of
tests/estimates_table_model.py, which tests/test_estimates_table_model.py pins to a case written out from the writer's lines and
holds against the existing writers.  Every array of the view and every scalar is compared byte for byte."""
import struct

import numpy as np
import pytest

from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import ClusterBatch, make_params
from rpvg_amd.estimates_table import (ROUTE_GLOBAL, ROUTE_LDS, ROUTE_WAVE, EstimatesTable, FlatEstimates, HarnessTable, limits,
                                      write_from_containers)
from tests import estimates_table_model as M
from tests import small_cases

pytestmark = pytest.mark.gpu

ARRAYS = ("haplotype_prob", "read_count", "transcript_count", "member_transcript_count", "cluster_transcript_count")
SCALARS = ("total_transcript_count", "noise_count_total", "noise_count_share_total")
TPM_ARRAYS = ("tpm", "member_tpm")


def bits(x):
    return struct.pack("<d", x)


def assert_same(got, want, names=ARRAYS, scalars=SCALARS):
    for name in names:
        assert got[name].dtype == np.float64 and got[name].shape == want[name].shape, name
        if got[name].tobytes() != want[name].tobytes():
            at = int(np.flatnonzero(got[name].view(np.uint64) != want[name].view(np.uint64))[0])
            raise AssertionError(f"{name}[{at}]: {got[name][at]!r} != {want[name][at]!r}")
    for name in scalars:
        assert bits(got[name]) == bits(want[name]), (name, got[name], want[name])


def flat_of(clusters):
    return FlatEstimates(**M.flatten(clusters))


def check(ctx, clusters, ploidy=2, routes=None):
    """Builds the table of the model's clusters on the device and holds view, scalars and TPMs (for the table's own total) to the
    model.  Returns the device's view."""
    want = M.table(clusters, ploidy)
    table = EstimatesTable.build(ctx, None, flat_of(clusters), ploidy)
    try:
        got = table.view()
        assert_same(got, want)
        assert not got["has_tpm"] and not got["tpm"].any() and not got["member_tpm"].any() and got["ploidy"] == ploidy
        assert got["clusters_by_route"] == M.clusters_by_route(limits(), clusters)
        if routes is not None:
            assert got["clusters_by_route"] == routes
        if want["total_transcript_count"] > 0:
            table.tpm(want["total_transcript_count"])
            got = table.view()
            assert got["has_tpm"] and bits(got["tpm_denominator"]) == bits(want["total_transcript_count"])
            assert_same(got, M.with_tpm(want, want["total_transcript_count"]), ARRAYS + TPM_ARRAYS)
        return got
    finally:
        table.free()


def test_limits_are_those_of_the_plan():
    lim = limits()
    assert (lim.wave_paths, lim.wave_members, lim.lds_paths, lim.lds_members) == (64, 256, 4096, 8192)
    assert lim.wave_lds_bytes == 4 * (64 + 256 + 1) and lim.lds_bytes == 4 * (4096 + 8192 + 4) <= 64 * 1024


def test_hand_case(hip_ctx):
    clusters, ploidy, expected, denominator, expected_tpm = M.hand_case()
    got = check(hip_ctx, clusters, ploidy, routes=[1, 0, 0])
    assert got["haplotype_prob"].tolist() == expected["haplotype_prob"] and got["read_count"].tolist() == expected["read_count"]
    table = EstimatesTable.build(hip_ctx, None, flat_of(clusters), ploidy)
    table.tpm(denominator)
    got = table.view()
    table.free()
    assert got["tpm"].tolist() == expected_tpm["tpm"] and got["member_tpm"].tolist() == expected_tpm["member_tpm"]


def test_wavefront_edges(hip_ctx):
    rng = np.random.default_rng(11)
    clusters = [M.cluster_with(rng, n, 120) for n in (63, 64, 65)]          # paths either side of a wavefront
    clusters += [M.cluster_with(rng, 9, m) for m in (63, 64, 65, 127, 128, 129)]  # members either side of a chunk of the placement
    clusters.append(dict(num_paths=1, sets=[(0,)], posteriors=[0.75], abundances=[12.5], noise_count=2.0, eff=[333.0]))  # one path in one set
    clusters.append(M.cluster_with(rng, 64, 64, ploidy=1))
    check(hip_ctx, clusters)


def test_empty_pieces(hip_ctx):
    rng = np.random.default_rng(12)
    no_sets = dict(num_paths=4, sets=[], posteriors=[], abundances=[], noise_count=5.0, eff=[100.0, 200.0, 0.0, 50.0])
    unused = M.cluster_with(rng, 30, 20)
    unused["sets"] = [tuple(min(p, 9) for p in s) for s in unused["sets"]]      # paths 10 .. 29 appear in no set
    bare = M.random_cluster(rng, 12, 25, with_abundances=False)                 # `haplotypes`: sets and posteriors, no abundances
    bare_mid = M.random_cluster(rng, 100, 300, with_abundances=False)           # ... on the workgroup route
    no_paths = dict(num_paths=0, sets=[], posteriors=[], abundances=[], noise_count=1.0, eff=[])
    clusters = [M.random_cluster(rng, 7, 10), no_sets, bare, unused, no_paths, bare_mid, M.random_cluster(rng, 5, 6), no_sets]
    got = check(hip_ctx, clusters)
    assert got["cluster_transcript_count"][1] == 0.0 and not got["read_count"][7 + 4:7 + 4 + 12].any()
    check(hip_ctx, [no_sets])
    check(hip_ctx, [no_paths, no_paths])
    # a cluster of the global route in a batch without any member: nothing to sort, every row zero
    wide = dict(num_paths=limits().lds_paths + 1, sets=[], posteriors=[], abundances=[], noise_count=2.5, eff=[75.0] * (limits().lds_paths + 1))
    got = check(hip_ctx, [wide, no_sets], routes=[1, 0, 1])
    assert not got["haplotype_prob"].any() and got["noise_count_total"] == 7.5


def test_empty_batch(hip_ctx):
    got = check(hip_ctx, [], routes=[0, 0, 0])
    assert all(got[name].size == 0 for name in ARRAYS + TPM_ARRAYS) and all(got[name] == 0.0 for name in SCALARS)


def test_either_side_of_every_route_limit(hip_ctx):
    lim = limits()
    rng = np.random.default_rng(13)
    clusters, routes = [], [0, 0, 0]

    def add(paths, members, route):
        clusters.append(M.cluster_with(rng, paths, members))
        routes[route] += 1

    for d, route in ((-1, ROUTE_WAVE), (0, ROUTE_WAVE), (1, ROUTE_LDS)):
        add(lim.wave_paths + d, 100, route)
        add(10, lim.wave_members + d, route)
    add(lim.wave_paths, lim.wave_members, ROUTE_WAVE)
    for d, route in ((-1, ROUTE_LDS), (0, ROUTE_LDS), (1, ROUTE_GLOBAL)):
        add(lim.lds_paths + d, 300, route)
        add(100, lim.lds_members + d, route)
    add(lim.lds_paths, lim.lds_members, ROUTE_LDS)
    add(lim.lds_paths + 1, lim.lds_members + 1, ROUTE_GLOBAL)
    add(3, 4, ROUTE_WAVE)   # a small cluster behind the large ones
    check(hip_ctx, clusters, routes=routes)


def test_order_of_additions_on_every_route(hip_ctx):
    """Paths with four memberships, in different chunks of 64 members, whose sequential, reversed and pairwise sums are three
    different doubles (searched for; tests/test_estimates_table_model.py asserts the property): a kernel that adds in another
    order, or as a tree, gives another double."""
    lim = limits()
    cases = M.three_sum_cases(7, 24)
    rng = np.random.default_rng(14)
    wave = M.order_cluster(cases[:2], num_paths=40, gap=20, rng=rng)
    mid = M.order_cluster(cases[2:12], num_paths=500, gap=40, rng=rng)
    large = M.order_cluster(cases[12:24], num_paths=lim.lds_paths + 10, gap=40, rng=rng)
    got = check(hip_ctx, [wave, mid, large], routes=[1, 1, 1])
    first = [0, wave["num_paths"], wave["num_paths"] + mid["num_paths"]]
    for g0, used in zip(first, (cases[:2], cases[2:12], cases[12:24])):
        for i, values in enumerate(used):
            assert got["read_count"][g0 + i] == M.sequential_sum(values)
            assert got["read_count"][g0 + i] not in (M.reversed_sum(values), M.pairwise_sum(values))
    # the same clusters in another order of the batch: the cluster sums keep their values, the total changes its order
    check(hip_ctx, [large, wave, mid, wave], routes=[2, 1, 1])


@pytest.mark.parametrize("ploidy", [2, 3, 8])
def test_duplicate_rule(hip_ctx, ploidy):
    """{a,a}, {a,a,b,b,b} and the unsorted {a,b,a}: a member counts for the probability unless it repeats its predecessor."""
    a, b = 2, 5
    sets = [(a, a), (a, a, b, b, b), (a, b, a), (b,), (b, a)]
    members = sum(len(s) for s in sets)
    cluster = dict(num_paths=7, sets=sets, posteriors=[0.5, 0.25, 0.125, 0.0625, 0.03125],
                   abundances=[float(2 ** i) for i in range(members)], noise_count=7.0, eff=[10.0, 20.0, 4.0, 40.0, 50.0, 8.0, 70.0])
    got = check(hip_ctx, [cluster], ploidy)
    assert got["haplotype_prob"][a] == 0.5 + 0.25 + 0.125 + 0.125 + 0.03125      # {a,b,a} counts a twice
    assert got["haplotype_prob"][b] == 0.25 + 0.125 + 0.0625 + 0.03125
    assert got["noise_count_share_total"] == 7.0 / ploidy


def test_zero_and_negative_effective_lengths(hip_ctx):
    lim = limits()
    rng = np.random.default_rng(15)
    clusters = [M.random_cluster(rng, 20, 60, eff_zero_share=0.4), M.random_cluster(rng, 300, 900, eff_zero_share=0.4),
                M.random_cluster(rng, lim.lds_paths + 3, 600, eff_zero_share=0.4)]
    got = check(hip_ctx, clusters, routes=[1, 1, 1])
    eff = np.concatenate([c["eff"] for c in clusters])
    assert (eff <= 0).sum() > 100 and not got["transcript_count"][eff <= 0].any() and got["read_count"][eff <= 0].any()


@pytest.mark.parametrize("ploidy", [1, 2, 8])
def test_ploidy_shares(hip_ctx, ploidy):
    rng = np.random.default_rng(16)
    clusters = [M.random_cluster(rng, 6, 9, ploidy=ploidy) for _ in range(150)]   # three rounds of the totals' wavefront
    got = check(hip_ctx, clusters, ploidy)
    assert got["noise_count_share_total"] == M.sequential_sum([c["noise_count"] / float(ploidy) for c in clusters])


def test_device_pointers(hip_ctx):
    """on_device = 1: the arrays are read where they lie on the GPU; the result is that of the host-pointer call."""
    lim = limits()
    rng = np.random.default_rng(17)
    clusters = [M.random_cluster(rng, 30, 50), M.random_cluster(rng, 200, 700), M.random_cluster(rng, 5, 3, with_abundances=False),
                M.cluster_with(rng, 50, lim.lds_members + 7)]
    flat = flat_of(clusters)
    host = EstimatesTable.build(hip_ctx, None, flat, 2)
    pointers = {}
    try:
        for name in ("set_off", "member_off", "members", "posteriors", "abund_off", "abundances", "noise_count", "cluster_path_off",
                     "path_effective_length"):
            a = getattr(flat, name)
            pointers[name] = hip_ctx.malloc(max(a.nbytes, 8))
            if a.nbytes:
                hip_ctx.h2d(pointers[name], a)
        device = EstimatesTable.build_flat(hip_ctx, flat.as_c(device_pointers=pointers), 2)
        try:
            want = host.view()
            assert_same(device.view(), want)
            assert device.view()["clusters_by_route"] == want["clusters_by_route"] == [2, 1, 1]
            assert_same(want, M.table(clusters, 2))
        finally:
            device.free()
    finally:
        host.free()
        for p in pointers.values():
            hip_ctx.free(p)


def test_invalid_input_names_the_cluster(hip_ctx):
    rng = np.random.default_rng(18)
    clusters = [M.random_cluster(rng, 8, 12) for _ in range(5)]

    def refused(flat, cluster, **sizes):
        with pytest.raises(hip.EngineError) as err:
            EstimatesTable.build_flat(hip_ctx, flat.as_c(**sizes), 2)
        assert "(-3)" in str(err.value) and f"cluster {cluster}:" in str(err.value), str(err.value)   # RPVG_HIP_ERR_INVALID

    flat = flat_of(clusters)
    s = int(flat.set_off[2]) + 3
    flat.member_off[s] = flat.member_off[s - 1] - 1          # decreasing member_off inside cluster 2
    refused(flat, 2)
    flat = flat_of(clusters)
    flat.members[int(flat.member_off[int(flat.set_off[3])])] = 8   # a member equal to the path count of cluster 3
    refused(flat, 3)
    short = [dict(c) for c in clusters]
    short[1]["abundances"] = short[1]["abundances"][:-1]     # members - 1 abundances in cluster 1
    refused(flat_of(short), 1)
    flat = flat_of(clusters)
    refused(flat, 4, num_members=len(flat.members) - 1)      # member_off ends beyond the array
    flat = flat_of(clusters)
    for k in (3, 1):
        flat.members[int(flat.member_off[int(flat.set_off[k])])] = 8   # the same offence in clusters 3 and 1: the smaller one is named
    refused(flat, 1)
    flat = flat_of(clusters)
    s = int(flat.set_off[2]) + 3
    flat.member_off[s] = flat.member_off[s - 1] - 1          # decreasing member_off inside cluster 2 (the smaller reason) ...
    flat.members[int(flat.member_off[int(flat.set_off[1])])] = 8   # ... and a member beyond its paths in cluster 1: the cluster decides
    refused(flat, 1)
    with pytest.raises(hip.EngineError):
        EstimatesTable.build(hip_ctx, None, flat_of(clusters), 0)
    check(hip_ctx, clusters)                                   # the context is usable afterwards


def test_zero_denominator(hip_ctx):
    """0 / 0 is NaN with a sign that differs between x86 and the GPU: positions are compared, not bytes."""
    rng = np.random.default_rng(19)
    clusters = [M.random_cluster(rng, 10, 14, eff_zero_share=0.3), M.random_cluster(rng, 6, 8, with_abundances=False)]
    want = M.with_tpm(M.table(clusters, 2), 0.0)
    table = EstimatesTable.build(hip_ctx, None, flat_of(clusters), 2)
    table.tpm(0.0)
    got = table.view()
    table.free()
    for name in TPM_ARRAYS:
        assert np.isnan(want[name]).any() and np.isinf(want[name]).any()
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
        assert np.array_equal(got[name][~np.isnan(want[name])], want[name][~np.isnan(want[name])]), name
    assert_same(got, want)


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("model", ["haplotype-transcripts", "transcripts"])
def test_end_to_end(engine, tmp_path, model):
    """Engine.run on a small_cases batch with default parameters: the table of its estimates is the model's, the files written from
    the table with its own total as the denominator are those of the existing writers byte for byte, and the total is the sum of the
    clusters' counts, within the derived bound of the single chain of totalTranscriptCount."""
    batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(4242, n_clusters=8, with_empty=True))
    params = make_params()
    prepared = engine.prepare(batch)
    try:
        estimates, _ = engine.run(model, params, prepared)
        clusters = M.from_estimates(batch, estimates)
        want = M.table(clusters, params.ploidy)
        table = EstimatesTable.build(engine, batch, estimates, params.ploidy)
        got = table.view()
        table.free()
        assert_same(got, want)
        total = got["total_transcript_count"]
        assert total > 0 and total == M.sequential_sum(want["cluster_transcript_count"].tolist())
        single = write_from_containers(prepared, "", params.ploidy, "")[0]
        model_single, n = M.total_single_chain(clusters)
        assert bits(single) == bits(model_single) and n > 10
        assert abs(total - single) <= 2 * (n - 1) * 2.0 ** -53 * single
        harness = HarnessTable(engine, prepared, params.ploidy)
        try:
            assert_same(harness.view(), want)
            harness.tpm(total)
            assert_same(harness.view(), M.with_tpm(want, total), ARRAYS + TPM_ARRAYS)
            writers = ("haplotype", "joint") + (("abundance",) if model == "transcripts" else ())
            for writer in writers:
                from_table, from_containers = str(tmp_path / f"table_{writer}"), str(tmp_path / f"containers_{writer}")
                harness.write(writer, from_table, params.prob_precision, unaligned_read_count=9)
                write_from_containers(prepared, writer, params.ploidy, from_containers, denominator=total, min_posterior=params.prob_precision,
                                      unaligned_read_count=9)
                suffix = "_joint.txt" if writer == "joint" else ".txt"
                text = open(from_containers + suffix, "rb").read()
                assert len(text.splitlines()) >= 2 and open(from_table + suffix, "rb").read() == text, writer
            if model != "transcripts":
                with pytest.raises(hip.EngineError, match="set i is not"):   # AbundanceEstimatesWriter asserts one set {i} per path
                    harness.write("abundance", str(tmp_path / "refused"))
        finally:
            harness.free()
    finally:
        prepared.free()
