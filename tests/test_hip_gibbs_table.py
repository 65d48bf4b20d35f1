"""The Gibbs samples table on the GPU (rpvg_amd/csrc/gibbs_table.hip, include/rpvg_samples.h) against the plain-Python model of
tests/gibbs_table_model.py, which tests/test_gibbs_table_model.py pins to a case written out from the writer's lines and holds
against ReadCountGibbsSamplesWriter.  Samples, listed and noise_counts are compared byte for byte: there is no tolerance."""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.batch import ClusterBatch
from rpvg_amd.gibbs_table import ROUTE_GLOBAL, ROUTE_RESIDENT, FlatGibbs, GibbsSamples, GibbsTable, limits
from tests import gibbs_table_model as M
from tests import large_cases

pytestmark = pytest.mark.gpu

ARRAYS = ("samples", "listed", "noise_counts")


def assert_same(got, want):
    for name in ARRAYS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        if got[name].tobytes() != want[name].tobytes():
            bits = np.uint64 if got[name].dtype == np.float64 else np.uint8
            at = np.argwhere(got[name].view(bits) != want[name].view(bits))[0]
            raise AssertionError(f"{name}{at.tolist()}: {got[name][tuple(at)]!r} != {want[name][tuple(at)]!r}")


def flat_of(clusters, N):
    return FlatGibbs(**M.flatten(clusters, N))


def check(ctx, clusters, N, routes=None):
    """Builds the table of the model's clusters on the device and holds the view to the model.  Returns the device's view."""
    want = M.table(clusters, N)
    table = GibbsTable.build(ctx, flat_of(clusters, N))
    try:
        got = table.view()
    finally:
        table.free()
    assert_same(got, want)
    assert got["clusters_by_route"] == M.clusters_by_route(limits(), clusters)
    if routes is not None:
        assert got["clusters_by_route"] == routes
    assert got["cluster_path_off"].tolist() == M.flatten(clusters, N)["cluster_path_off"]
    return got


@pytest.fixture(scope="module")
def cases():
    return M.scatter_cases(limits())


def test_limits_are_those_of_the_plan():
    lim = limits()
    assert (lim.resident_paths, lim.resident_columns, lim.sample_tile, lim.global_paths) == (1024, 64, 64, 256)
    assert lim.resident_lds_bytes == 8 * 64 * 65 <= 64 * 1024


def test_hand_case(hip_ctx):
    clusters, N, expected = M.hand_case()
    got = check(hip_ctx, clusters, N, routes=[2, 0])
    assert got["samples"].tolist() == expected["samples"] and got["listed"].tolist() == expected["listed"]
    assert got["noise_counts"].tolist() == expected["noise_counts"]


@pytest.mark.parametrize("name", ["widths_and_counts", "tails", "one_sample", "many_blocks", "odd_clusters", "single_cluster", "empty_batch"])
def test_scatter_cases(hip_ctx, cases, name):
    clusters, N = cases[name]
    got = check(hip_ctx, clusters, N)
    if name == "tails":
        assert not got["listed"][18:27].any() and got["listed"][:18].any()        # all blocks empty: nothing listed
        assert got["noise_counts"][N - 1] == M.sequential_sum(M.column_addends(clusters, N, N - 1))
    if name == "odd_clusters":
        assert 2 + 2 <= got["listed"].sum() <= 3 + 2 and got["samples"].shape == (302, N)  # most paths of the second cluster unlisted
    if name == "empty_batch":
        assert got["samples"].shape == (0, N) and got["noise_counts"].tolist() == [0.0] * N and got["clusters_by_route"] == [0, 0]
    if name == "widths_and_counts":
        wide = sum(1 for c in clusters if len(c["blocks"][0]["ids"]) > limits().resident_columns)                   # the width of 65
        assert wide >= 4 and got["clusters_by_route"] == [len(clusters) - wide, wide]


def test_either_side_of_every_route_limit(hip_ctx, cases):
    lim = limits()
    clusters, N = cases["route_limits"]
    want_routes = [ROUTE_RESIDENT, ROUTE_RESIDENT, ROUTE_RESIDENT, ROUTE_RESIDENT, ROUTE_GLOBAL, ROUTE_GLOBAL,   # paths - 1, columns - 1, at, at, + 1, + 1
                   ROUTE_RESIDENT, ROUTE_GLOBAL, ROUTE_GLOBAL, ROUTE_RESIDENT]
    assert [M.route_of(lim, c) for c in clusters] == want_routes
    check(hip_ctx, clusters, N, routes=[want_routes.count(ROUTE_RESIDENT), want_routes.count(ROUTE_GLOBAL)])


def test_negative_zero_and_a_subnormal_arrive_as_they_are(hip_ctx):
    values, rng = M.Values(), np.random.default_rng(3)
    clusters = [M.make_cluster(values, rng, 8, [(3, 5)]), M.make_cluster(values, rng, 70, [(66, 3)])]   # one per route
    for cluster in clusters:
        cluster["blocks"][0]["abund"][1][0] = -0.0
        cluster["blocks"][0]["abund"][2][1] = 5e-324
    got = check(hip_ctx, clusters, 6, routes=[1, 1])
    words = got["samples"].view(np.uint64)
    assert (words == 0x8000000000000000).sum() == 2 and (words == 1).sum() == 2


@pytest.mark.parametrize("K", [1, 2, 64, 65, 257])
def test_noise_chains_add_in_cluster_order(hip_ctx, K):
    """Magnitudes from 1e-3 to 1e9; for K >= 3 some column's chain differs from the reversed chain and from a pairwise sum (searched
    for; tests/test_gibbs_table_model.py asserts the property): a kernel that adds in another order, or as a tree, gives another double."""
    clusters, N, _ = M.noise_case(K)
    got = check(hip_ctx, clusters, N)
    for s in range(N):
        assert got["noise_counts"][s] == M.sequential_sum(M.column_addends(clusters, N, s))


def test_rows_of_a_range_equal_the_view(hip_ctx, cases):
    clusters, N = cases["tails"]
    table = GibbsTable.build(hip_ctx, flat_of(clusters, N))
    try:
        view = table.view()
        P = view["samples"].shape[0]
        for first, count in ((0, 5), (P // 2, 7), (P - 3, 3), (P, 0), (0, P)):
            assert table.rows(first, count, N).tobytes() == view["samples"][first:first + count].tobytes()
        with pytest.raises(hip.EngineError, match=r"\(-3\)"):
            table.rows(P - 1, 2, N)
    finally:
        table.free()


def test_device_pointers_and_two_builds(hip_ctx, cases):
    """on_device = 1: the arrays are read where they lie on the GPU; the result is that of the host-pointer call, twice."""
    clusters, N = cases["route_limits"]
    flat = flat_of(clusters, N)
    host = GibbsTable.build(hip_ctx, flat)
    pointers = {}
    try:
        for name in ("gibbs_off", "gibbs_path_off", "gibbs_path", "gibbs_noise_off", "gibbs_noise", "gibbs_abund_off", "gibbs_abund",
                     "cluster_path_off", "total_count"):
            a = getattr(flat, name)
            pointers[name] = hip_ctx.malloc(max(a.nbytes, 8))
            if a.nbytes:
                hip_ctx.h2d(pointers[name], a)
        want = host.view()
        for _ in range(2):
            device = GibbsTable.build_flat(hip_ctx, flat.as_c(device_pointers=pointers))
            try:
                got = device.view()
                assert_same(got, want)
                assert got["clusters_by_route"] == want["clusters_by_route"] and got["cluster_path_off"].tolist() == want["cluster_path_off"].tolist()
            finally:
                device.free()
        assert_same(want, M.table(clusters, N))
    finally:
        host.free()
        for p in pointers.values():
            hip_ctx.free(p)


def test_invalid_input_names_the_cluster_or_block(hip_ctx):
    values, rng = M.Values(), np.random.default_rng(4)
    clusters = [M.make_cluster(values, rng, 8, [(3, 2), (4, 3), (2, 1)]) for _ in range(5)]   # blocks 3k .. 3k + 2 of cluster k
    N = 6

    def refused(flat, what, **sizes):
        with pytest.raises(hip.EngineError) as err:
            GibbsTable.build_flat(hip_ctx, flat.as_c(**sizes))
        assert "(-3)" in str(err.value) and f"{what}:" in str(err.value), str(err.value)   # RPVG_HIP_ERR_INVALID

    flat = flat_of(clusters, N)
    flat.gibbs_off[3] = flat.gibbs_off[2] - 1                    # gibbs_off decreases at the end of cluster 2
    refused(flat, "cluster 2")
    flat = flat_of(clusters, N)
    refused(flat, "cluster 4", num_blocks=len(flat.gibbs_path_off) - 2)   # gibbs_off ends beyond the stated number of blocks
    flat = flat_of(clusters, N)
    flat.cluster_path_off[2] = flat.cluster_path_off[1] - 1      # cluster_path_off decreases at the end of cluster 1
    refused(flat, "cluster 1")
    flat = flat_of(clusters, N)
    flat.gibbs_path_off[8] = flat.gibbs_path_off[7] - 1          # gibbs_path_off decreases at the end of block 7
    refused(flat, "block 7")
    flat = flat_of(clusters, N)
    refused(flat, "block 14", num_noise_samples=len(flat.gibbs_noise) - 1)       # gibbs_noise_off ends beyond the stated size
    flat = flat_of(clusters, N)
    refused(flat, "block 14", num_abundance_samples=len(flat.gibbs_abund) - 1)   # gibbs_abund_off ends beyond the stated size
    short = [dict(c, blocks=[dict(b) for b in c["blocks"]]) for c in clusters]
    short[1]["blocks"][1]["abund"] = short[1]["blocks"][1]["abund"][:-1]         # samples - 1 rows of abundance samples in block 4
    refused(flat_of(short, N), "block 4")
    flat = flat_of(clusters, N)
    at = int(flat.gibbs_path_off[10])
    flat.gibbs_path[at + 1] = flat.gibbs_path[at]                # equal ids in block 10
    refused(flat, "block 10")
    flat = flat_of(clusters, N)
    flat.gibbs_path[int(flat.gibbs_path_off[12]) - 1] = 8        # an id equal to the path count, last of block 11
    refused(flat, "block 11")
    refused(flat_of(clusters, 5), "cluster 0")                   # S_k = 6 > N = 5 in every cluster
    flat = flat_of(clusters, N)
    flat.gibbs_off[4] = flat.gibbs_off[3] - 1                    # gibbs_off decreases at the end of cluster 3 (the smaller reason) ...
    flat.cluster_path_off[2] = flat.cluster_path_off[1] - 1      # ... and cluster_path_off at the end of cluster 1: the cluster decides
    refused(flat, "cluster 1")
    flat = flat_of(clusters, N)
    at = int(flat.gibbs_path_off[10])
    flat.gibbs_path[at + 1] = flat.gibbs_path[at]                # equal ids in block 10 (cluster 3) ...
    flat.gibbs_path_off[5] = flat.gibbs_path_off[4] - 1          # ... and gibbs_path_off decreases at the end of block 4 (cluster 1)
    refused(flat, "block 4")
    flat = flat_of(clusters, N)
    at = int(flat.gibbs_path_off[1])
    flat.gibbs_path[at + 1] = flat.gibbs_path[at]                # equal ids in block 1 (cluster 0) ...
    flat.cluster_path_off[4] = flat.cluster_path_off[3] - 1      # ... and a cluster offence behind it: a cluster comes before every block
    refused(flat, "cluster 3")
    with pytest.raises(hip.EngineError, match=r"\(-3\).*num_gibbs_samples is 0"):
        GibbsTable.build(hip_ctx, flat_of(clusters, 0))
    check(hip_ctx, clusters, N)                                  # the context is usable afterwards


def _columns(b):
    return [list(range(int(b.cluster_path_off[k + 1] - b.cluster_path_off[k]))) for k in range(b.num_clusters)]


def _resident_against_downloaded(ctx, batch, problems_of, num_samples, seeds, thin, N, grid_problems):
    """The sampler's samples left on the device equal those it downloads, and the table built from the handle equals the table
    built from the downloaded arrays.  problems_of: the cluster of every problem (non-decreasing); a problem takes all paths."""
    dev = ctx.upload(batch)
    try:
        columns = [_columns(batch)[k] for k in problems_of]
        abund, noise, total, _ = ctx.em_solve(dev, problems_of, columns)
        ctx.reset_stats()
        got = ctx.gibbs_read_counts(dev, problems_of, columns, abund, noise, num_samples, seeds, thin)
        assert ctx.stats()["gibbs_count_grid_problems"] == grid_problems
        handle = GibbsSamples.draw(ctx, dev, problems_of, columns, abund, noise, num_samples, seeds, thin)
        try:
            noise_samples, abund_samples = handle.get()
            assert noise_samples.tobytes() == np.concatenate([g[0] for g in got]).tobytes() and noise_samples.size == sum(num_samples)
            assert abund_samples.tobytes() == np.concatenate([g[1].reshape(-1) for g in got]).tobytes()
            K = batch.num_clusters
            cluster_total = [float(total[problems_of.index(k)]) if k in problems_of else 3.25 for k in range(K)]
            clusters = [dict(num_paths=len(_columns(batch)[k]), total_count=cluster_total[k],
                             blocks=[dict(ids=columns[p], noise=got[p][0].tolist(), abund=got[p][1].tolist())
                                     for p in range(len(problems_of)) if problems_of[p] == k]) for k in range(K)]
            from_arrays = GibbsTable.build(ctx, flat_of(clusters, N))
            from_handle = GibbsTable.build_resident(ctx, handle, batch.cluster_path_off, cluster_total, N)
            try:
                want = from_arrays.view()
                assert_same(from_handle.view(), want)
                assert_same(want, M.table(clusters, N))
                assert want["listed"].any() and want["samples"].any()
            finally:
                from_arrays.free()
                from_handle.free()
        finally:
            handle.free()
    finally:
        dev.free()


def test_resident_samples_one_workgroup(hip_ctx, monkeypatch):
    """The two-problem one-workgroup case of tests/test_hip_gibbs_counts_draws.py, with a third problem without samples."""
    monkeypatch.delenv("RPVG_HIP_EM_GRID_MIN_WORK", raising=False)
    tall = large_cases.cluster_batch(300, 12, 3, seed=31, noise_only_frac=0.02, max_count=400)
    wide = large_cases.cluster_batch(40, 300, 3, seed=32, noise_only_frac=0.1)
    batch = ClusterBatch.concat([tall, wide])
    _resident_against_downloaded(hip_ctx, batch, [0, 1, 1], [4, 4, 0], [77, 78, 79], 2, 9, grid_problems=0)


def test_resident_samples_whole_gpu_route(hip_ctx, monkeypatch):
    monkeypatch.setenv("RPVG_HIP_EM_GRID_MIN_WORK", "1000")
    batch = large_cases.cluster_batch(600, 40, 3, seed=31, noise_only_frac=0.01, max_count=400)
    _resident_against_downloaded(hip_ctx, batch, [0], [4], [77], 2, 4, grid_problems=1)


def test_resident_refusals_and_the_empty_handle(hip_ctx, monkeypatch):
    monkeypatch.delenv("RPVG_HIP_EM_GRID_MIN_WORK", raising=False)
    tall = large_cases.cluster_batch(300, 12, 3, seed=31, noise_only_frac=0.02, max_count=400)
    batch = ClusterBatch.concat([tall, tall])
    dev = hip_ctx.upload(batch)
    try:
        columns = _columns(batch)
        abund, noise, total, _ = hip_ctx.em_solve(dev, [0, 1], columns)
        empty = GibbsSamples.draw(hip_ctx, dev, [0, 1], columns, abund, noise, [0, 0], [1, 2], 2)   # no sample: an empty handle
        try:
            assert empty.get()[0].size == 0
            table = GibbsTable.build_resident(hip_ctx, empty, batch.cluster_path_off, [5.0, 6.0], 3)
            got = table.view()
            table.free()
            assert not got["samples"].any() and not got["listed"].any() and got["noise_counts"].tolist() == [11.0] * 3
        finally:
            empty.free()
        backwards = GibbsSamples.draw(hip_ctx, dev, [1, 0], [columns[1], columns[0]], [abund[1], abund[0]], [noise[1], noise[0]], [2, 2], [1, 2], 2)
        try:
            with pytest.raises(hip.EngineError, match=r"\(-3\).*problem 1"):
                GibbsTable.build_resident(hip_ctx, backwards, batch.cluster_path_off, [5.0, 6.0], 3)
        finally:
            backwards.free()
    finally:
        dev.free()


@pytest.mark.parametrize("model", ["haplotype-transcripts", "transcripts"])
def test_end_to_end(tmp_path, model):
    """Engine.run with -n 6 on a small_cases batch: the table of its samples is the model's and the host loop's, and the file
    written from the table is the file of the writer's addSamples(), byte for byte."""
    import gzip

    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import make_params
    from rpvg_amd.gibbs_table import HarnessGibbsTable, from_containers
    from tests import small_cases

    N = 6
    batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(4242, n_clusters=8, with_empty=True))
    params = make_params(num_gibbs_samples=N)
    engine = eng_mod.Engine(0)
    try:
        prepared = engine.prepare(batch)
        try:
            estimates, _ = engine.run(model, params, prepared)
            clusters = [dict(num_paths=int(batch.cluster_path_off[k + 1] - batch.cluster_path_off[k]), total_count=float(e.total_count),
                             blocks=[dict(ids=[int(p) for p in ids], noise=[float(x) for x in ns], abund=np.asarray(ab).reshape(len(ns), len(ids)).tolist())
                                     for ids, ns, ab in e.gibbs_samples]) for k, e in enumerate(estimates)]
            assert sum(len(c["blocks"]) for c in clusters) >= 4
            want = M.table(clusters, N)
            table = GibbsTable.build(engine, FlatGibbs.from_estimates(batch, estimates, N))
            got = table.view()
            table.free()
            assert_same(got, want)
            assert want["listed"].any() and want["samples"].any()
            host = from_containers(prepared, N, int(batch.cluster_path_off[-1]), prefix=str(tmp_path / "containers"), unaligned_read_count=9)
            assert_same(host, want)
            harness = HarnessGibbsTable(engine, prepared, N)
            try:
                assert_same(harness.view(), want)
                harness.write(str(tmp_path / "table"), unaligned_read_count=9)
            finally:
                harness.free()
            text = gzip.open(tmp_path / "containers.txt.gz", "rb").read()
            assert len(text.splitlines()) >= 3 and gzip.open(tmp_path / "table.txt.gz", "rb").read() == text
            assert open(tmp_path / "table.txt.gz", "rb").read() == open(tmp_path / "containers.txt.gz", "rb").read()
        finally:
            prepared.free()
    finally:
        engine.close()
