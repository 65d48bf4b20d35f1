"""The path table on the GPU (rpvg_amd/csrc/path_table.hip, include/rpvg_index.h) against the plain-Python model of
tests/path_table_model.py, which tests/test_path_table_model.py pins to a case written out from the reference's lines.
Every comparison is exact: integers, and doubles byte for byte."""
import dataclasses

import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.index import DevicePathTable, FragmentLists, IndexParams, PathTable, build_index, name_groups_limits
from rpvg_amd.rows import AlignmentBatch, RowParams
from tests import align_index_model as IM
from tests import path_table_model as M
from tests import small_cases

pytestmark = pytest.mark.gpu


# ---- an index with clusters of given sizes -----------------------------------------------------------------------------------

def blocks_case(sizes, lists_per_block=None):
    """(params, lists, extra_sets): consecutive id blocks of the given sizes, each one cluster (joined by an extra set); block b
    is touched by lists_per_block[b] distinct lists (default: one, every fourth block none — those rank last)."""
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    lists, extra = [], []
    for b, n in enumerate(sizes):
        ids = list(range(starts[b], starts[b + 1]))
        if n > 1:
            extra.append(ids)
        touched = (0 if b % 4 == 3 else 1) if lists_per_block is None else lists_per_block[b]
        for t in range(touched):
            lists.append(IM.mk([(10 + t, 50, 100 + t, [ids[0]]), (9, 50, 101, [ids[-1]])], 1, 40, -3 - t))
    return IM.default_params(int(starts[-1])), lists, extra


def device_table(ctx, table):
    """The model's table (tests/path_table_model.py: dict of lists) made resident."""
    off = ids = None
    if table["source_ids"] is not None:
        off = np.concatenate([[0], np.cumsum([len(s) for s in table["source_ids"]])]).astype(np.uint64)
        ids = [s for per_path in table["source_ids"] for s in per_path]
    return DevicePathTable(ctx, PathTable(table["group_id"], table["source_count"], table["length"], table["effective_length"], off, ids,
                                          table["name_id"]))


def model_view(clusters, table):
    path_group, cluster_group_off = M.name_groups(clusters, table["name_id"])
    flat = [c for collapsed in M.collapsed_paths(clusters, table) for c in collapsed]
    return dict(path_group=np.asarray(path_group, dtype=np.uint32), cluster_group_off=np.asarray(cluster_group_off, dtype=np.uint64),
                group_first_path=np.asarray([c["first_path"] for c in flat], dtype=np.uint32),
                group_name_id=np.asarray([c["name_id"] for c in flat], dtype=np.uint32),
                group_group_id=np.asarray([c["group_id"] for c in flat], dtype=np.uint32),
                group_source_count=np.asarray([c["source_count"] for c in flat], dtype=np.uint32),
                group_length=np.asarray([c["length"] for c in flat], dtype=np.uint32),
                group_effective_length=np.asarray([c["effective_length"] for c in flat], dtype=np.float64))


def assert_same(got, want):
    assert set(got) == set(want)
    for name, w in want.items():
        assert got[name].dtype == w.dtype and got[name].shape == w.shape and got[name].tobytes() == w.tobytes(), name


def check_groups(ctx, sizes, table, lists_per_block=None):
    """Builds the index of blocks_case, forms the groups on the device and holds every array to the model.  Returns the device's view."""
    params, lists, extra = blocks_case(sizes, lists_per_block)
    want_index = IM.run_model(params, [lists], extra)
    clusters = M.cluster_lists(want_index["arrays"])
    assert sorted(len(c) for c in clusters) == sorted(sizes)
    index = build_index(ctx, IndexParams(**params), [FragmentLists.from_lists(lists)], extra)
    dev = device_table(ctx, table)
    try:
        assert np.array_equal(index.view().cluster_paths, want_index["arrays"]["cluster_paths"])
        groups = index.name_groups(dev)
        got = groups.view()
        groups.free()
        assert_same(got, model_view(clusters, table))
        return got
    finally:
        dev.free()
        index.free()


def names_for(sizes, per_block):
    """name ids by global path: per_block(b, n, first global id) -> n ids."""
    out, start = [], 0
    for b, n in enumerate(sizes):
        ids = per_block(b, n, start)
        assert len(ids) == n
        out.extend(int(x) for x in ids)
        start += n
    return out


# ---- name groups and collapsed paths -----------------------------------------------------------------------------------------

def test_small_clusters(hip_ctx):
    rng = np.random.default_rng(1)
    sizes = [1, 1, 2, 2, 63, 64, 65, 3, 3, 1, 5, 64, 64]

    def per_block(b, n, start):
        if b == 2:
            return [77, 77]                                   # two paths, one name
        if b == 3:
            return [5, 4]                                     # two paths, two names, ids descending
        if b == 7:
            return [900, 800, 900]                            # the same ids as block 8: one id in two clusters
        if b == 8:
            return [800, 900, 800]
        if b == 11:
            return [123456] * n                               # all names equal
        if b == 12:
            return list(range(5000 + n, 5000, -1))            # all names different, ids descending along the cluster
        if n >= 3:
            return M.non_monotone_names(rng, n, max(2, n // 3))
        return [1000 + start]
    names = names_for(sizes, per_block)
    got = check_groups(hip_ctx, sizes, M.make_table(sum(sizes), name_id=names, seed=2))
    assert int(got["cluster_group_off"][-1]) < sum(sizes)


def test_either_side_of_the_route_limits(hip_ctx):
    limits = name_groups_limits()
    assert (limits.wave_paths, limits.lds_paths) == (64, 4096)
    rng = np.random.default_rng(3)
    sizes = [limits.wave_paths - 1, limits.wave_paths, limits.wave_paths + 1, limits.lds_paths - 1, limits.lds_paths, limits.lds_paths + 1, 7]
    names = names_for(sizes, lambda b, n, start: M.non_monotone_names(rng, n, max(2, n // 4)))
    check_groups(hip_ctx, sizes, M.make_table(sum(sizes), name_id=names, seed=4))
    # all names equal and all names different on the two larger routes
    sizes = [300, 300, limits.lds_paths + 5, limits.lds_paths + 5]
    names = names_for(sizes, lambda b, n, start: [9] * n if b % 2 == 0 else list(range(start + n + 100, start + 100, -1)))
    check_groups(hip_ctx, sizes, M.make_table(sum(sizes), name_id=names, seed=5))


def test_a_b_a_with_the_repeat_far_away(hip_ctx):
    limits = name_groups_limits()
    sizes = [200, 1500, limits.lds_paths + 2000]
    repeat_at = {0: 130, 1: 1400, 2: limits.lds_paths + 1500}   # another wavefront, another part of the sort, another workgroup's tile

    def per_block(b, n, start):
        ids = list(range(10 ** 6 + start + n, 10 ** 6 + start, -1))  # all different, descending
        ids[repeat_at[b]] = ids[0]
        return ids
    got = check_groups(hip_ctx, sizes, M.make_table(sum(sizes), name_id=names_for(sizes, per_block), seed=6))
    assert int(got["cluster_group_off"][-1]) == sum(sizes) - 3


def test_untouched_clusters_rank_last(hip_ctx):
    sizes = [3, 4, 70, 2, 5]
    rng = np.random.default_rng(7)
    names = names_for(sizes, lambda b, n, start: M.non_monotone_names(rng, n, 2) if n >= 3 else [4, 4])
    params, lists, extra = blocks_case(sizes, [2, 0, 0, 3, 0])
    order = [len(c) for c in M.cluster_lists(IM.run_model(params, [lists], extra)["arrays"])]
    assert order == [2, 3, 5, 70, 4]  # the clusters no list touches come last, the larger PathClusters index first
    check_groups(hip_ctx, sizes, M.make_table(sum(sizes), name_id=names, seed=8), [2, 0, 0, 3, 0])


def test_no_clusters_no_paths(hip_ctx):
    got = check_groups(hip_ctx, [], M.make_table(0, name_id=[]))
    assert got["cluster_group_off"].tolist() == [0] and got["path_group"].size == 0


def test_a_group_of_700_members(hip_ctx):
    rng = np.random.default_rng(9)
    names = [11 if i % 2 == 0 or i >= 200 else 1000 + i for i in range(800)]    # 700 members (the reference's largest group: 648), and 100 singletons
    assert names.count(11) == 700
    table = M.make_table(800, name_id=names, source_count=[int(x) for x in rng.integers(1, 5000, size=800)], seed=10)
    got = check_groups(hip_ctx, [800], table)
    assert int(got["group_source_count"][0]) == sum(table["source_count"][i] for i in range(800) if names[i] == 11)


def test_rounding_is_half_away_from_zero(hip_ctx):
    lengths = [(1, 2), (2, 3), (3, 4), (4, 5), (7, 8), (0, 1), (2, 2), (0xfffffffe, 0xffffffff)]
    sizes = [2] * len(lengths)
    table = M.make_table(2 * len(lengths), name_id=[i // 2 for i in range(2 * len(lengths))], source_count=[1] * (2 * len(lengths)),
                         length=[x for pair in lengths for x in pair], seed=11)
    got = check_groups(hip_ctx, sizes, table, [1] * len(sizes))
    assert sorted(got["group_length"].tolist()) == sorted([2, 3, 4, 5, 8, 1, 2, 0xffffffff])
    # weighted: (5 * 1 + 6 * 3) / 4 = 5.75 -> 6; (10 * 3 + 11 * 3) / 6 = 10.5 -> 11; (10 * 1 + 13 * 1 + 13 * 2) / 4 = 12.25 -> 12
    table = M.make_table(7, name_id=[1, 1, 2, 2, 3, 3, 3], source_count=[1, 3, 3, 3, 1, 1, 2], length=[5, 6, 10, 11, 10, 13, 13], seed=12)
    got = check_groups(hip_ctx, [2, 2, 3], table, [1, 1, 1])
    assert sorted(got["group_length"].tolist()) == [6, 11, 12]


def test_effective_lengths_are_the_sequential_unfused_sum(hip_ctx):
    cases = M.three_sum_cases(90, 24)
    assert cases[0] == M.THREE_SUM_TRIPLE
    sizes = [3] * len(cases)
    eff = [e for c in cases for e in c[0]]
    counts = [n for c in cases for n in c[1]]
    table = M.make_table(3 * len(cases), name_id=[500 - i // 3 for i in range(3 * len(cases))], effective_length=eff, source_count=counts, seed=13)
    got = check_groups(hip_ctx, sizes, table, [1] * len(sizes))
    sequential = sorted(M.sequential_sum(*c) / float(sum(c[1])) for c in cases)
    assert sorted(got["group_effective_length"].tolist()) == sequential
    assert sequential != sorted(M.reversed_sum(*c) / float(sum(c[1])) for c in cases)
    assert sequential != sorted(M.fused_sum(*c) / float(sum(c[1])) for c in cases)


def test_zero_source_count_and_overflow_are_refused(hip_ctx):
    sizes = [3, 4, 70]
    params, lists, extra = blocks_case(sizes, [3, 2, 1])
    clusters = M.cluster_lists(IM.run_model(params, [lists], extra)["arrays"])
    names = names_for(sizes, lambda b, n, start: [(start + i) // 2 for i in range(n)])
    good = M.make_table(77, name_id=names, seed=14)
    zero = dict(good, source_count=list(good["source_count"]))
    zero["source_count"][5] = 0
    over = dict(good, source_count=list(good["source_count"]))
    over["source_count"][40] = 0xffffffff
    over["source_count"][41] = 1
    index = build_index(hip_ctx, IndexParams(**params), [FragmentLists.from_lists(lists)], extra)
    try:
        for bad in (zero, over):
            with pytest.raises(M.InvalidGroup):
                M.collapsed_paths(clusters, bad)
            cluster, group = M.first_invalid_group(clusters, bad)
            dev = device_table(hip_ctx, bad)
            with pytest.raises(hip.EngineError) as err:
                index.name_groups(dev)
            assert "(-3)" in str(err.value) and f"group {group} of cluster {cluster} " in str(err.value)
            dev.free()
        dev = device_table(hip_ctx, good)   # the context and the index still work
        groups = index.name_groups(dev)
        assert_same(groups.view(), model_view(clusters, good))
        groups.free()
        no_names = device_table(hip_ctx, dict(good, name_id=None))
        with pytest.raises(hip.EngineError):
            index.name_groups(no_names)
        no_names.free()
        dev.free()
    finally:
        index.free()


def test_two_runs_give_the_same_bytes(hip_ctx):
    limits = name_groups_limits()
    rng = np.random.default_rng(15)
    sizes = [40, 500, limits.lds_paths + 100, 64, 9]
    names = names_for(sizes, lambda b, n, start: M.non_monotone_names(rng, n, max(2, n // 5)))
    table = M.make_table(sum(sizes), name_id=names, seed=16)
    a = check_groups(hip_ctx, sizes, table)
    b = check_groups(hip_ctx, sizes, table)
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)


# ---- a stream of a few hundred lists over sixty paths ------------------------------------------------------------------------

def stream_case():
    lists = IM.random_stream(71, num_paths=60, num_lists=400, num_templates=120, long_lists=1, max_frag_length=600, join_prob=0.0)
    scaled = {}  # noise scores on the scale of the row construction: noise probabilities 0.03 .. 0.6
    for ls in lists:
        if id(ls) not in scaled:
            scaled[id(ls)] = dict(ls, noise_score=-500000 * (1 + (-ls["noise_score"]) % 7))
    lists = [scaled[id(ls)] for ls in lists]
    params = IM.default_params(60)
    rng = np.random.default_rng(72)
    effective_length = [float(x) for x in rng.uniform(300.0, 3000.0, size=60)]
    extra = [[0, 59], [20, 21, 22]]
    return lists, params, effective_length, extra


def frag_table():
    v = np.arange(65536, dtype=np.float64)
    return -0.5 * ((v - 300.0) / 50.0) ** 2 - np.log(50.0 * np.sqrt(2 * np.pi))


def source_tables(effective_length):
    """The tables of the path-side tests over sixty paths: haplotypes 0 .. 39, transcripts of three consecutive paths."""
    rng = np.random.default_rng(73)
    base = dict(group_id=[(p // 3) % 7 for p in range(60)], source_count=[1 + p % 4 for p in range(60)], length=[400 + 37 * p for p in range(60)],
                effective_length=effective_length, name_id=[500 + 13 * ((p * 7) % 10) for p in range(60)])  # ten names, each on every tenth path
    mixed = [sorted(int(x) for x in rng.choice(40, size=int(rng.integers(1, 6)), replace=False)) for _ in range(60)]
    mixed[0] = [3]                                        # the first path of the table: one source
    mixed[7] = []                                         # a path without sources
    mixed[30] = list(range(100, 400))                     # a path with 300 sources (longer than a wavefront)
    mixed[59] = [0, 39]                                   # the last path of the table
    # several haplotypes with identical path lists (multiplicity > 1): haplotypes 50 .. 55 ride on the paths of haplotype 3
    shared = [sorted(s + ([50, 51, 52, 53, 54, 55] if 3 in s else [])) for s in mixed]
    return {"mixed": dict(base, source_ids=mixed), "shared": dict(base, source_ids=shared), "none": dict(base, source_ids=None)}


def baseline_batch(rows, clusters, table):
    """The downloaded rows with the table permuted on the host: what a caller hands to rpvg_hip_batch_upload."""
    group_id, off, ids = M.path_side(clusters, table)
    P = len(group_id)
    order = [p for c in clusters for p in c]
    return dataclasses.replace(rows, path_group_id=np.asarray(group_id, dtype=np.uint32),
                               path_source_count=np.asarray([table["source_count"][p] for p in order], dtype=np.uint32),
                               path_source_off=np.asarray(off if off is not None else [0] * (P + 1), dtype=np.uint64),
                               source_id=np.asarray(ids if ids is not None else [], dtype=np.uint32),
                               path_effective_length=np.asarray([table["effective_length"][p] for p in order], dtype=np.float64))


def test_rows_from_the_collapsed_index_equal_rows_from_the_uploaded_model_output(hip_ctx):
    lists, params, effective_length, extra = stream_case()
    want = IM.run_model(params, [lists], extra)
    clusters = M.cluster_lists(want["arrays"])
    table = source_tables(effective_length)["none"]
    assert len(clusters) >= 4 and not M.is_monotone([table["name_id"][p] for p in clusters[0]])
    path_group, cluster_group_off = M.name_groups(clusters, table["name_id"])
    model_clusters = IM.model_clusters(want, effective_length)
    at = 0
    for cl, paths in zip(model_clusters, clusters):
        for info, p in zip(cl["paths"], paths):
            info["source_count"] = table["source_count"][p]
            info["group"] = path_group[at]
            at += 1
    index = build_index(hip_ctx, IndexParams(**params), [FragmentLists.from_lists(c) for c in IM.chunked(lists, 150)], extra)
    dev = device_table(hip_ctx, table)
    row_params = RowParams(frag_length_log_prob=frag_table())
    try:
        groups = index.name_groups(dev)
        from_index = index.alignments_collapsed(dev, groups)
        host = AlignmentBatch.from_clusters(model_clusters)
        assert host.cluster_group_off.tolist() == cluster_group_off
        uploaded = hip_ctx.upload_alignments(host)
        a = from_index.build_rows(row_params).download()[0]
        b = uploaded.build_rows(row_params).download()[0]
        assert a.num_clusters == b.num_clusters == want["num_clusters"] and int(a.cluster_row_off[-1]) > 50
        assert a.cluster_path_off.tolist() == cluster_group_off
        for name in ("cluster_row_off", "cluster_path_off", "row_count", "row_noise", "row_grp_off", "grp_prob", "grp_idx_off", "path_idx"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        from_index.free()
        uploaded.free()
        groups.free()
    finally:
        dev.free()
        index.free()


@pytest.mark.parametrize("which", ["mixed", "shared", "none"])
def test_path_side_equals_the_upload_of_the_permuted_table(hip_ctx, which):
    lists, params, effective_length, extra = stream_case()
    want = IM.run_model(params, [lists], extra)
    clusters = M.cluster_lists(want["arrays"])
    table = source_tables(effective_length)[which]
    index = build_index(hip_ctx, IndexParams(**params), [FragmentLists.from_lists(c) for c in IM.chunked(lists, 150)], extra)
    dev = device_table(hip_ctx, table)
    try:
        alignments = index.alignments(effective_length)
        rows = alignments.build_rows(RowParams(frag_length_log_prob=frag_table()))
        host_rows = rows.download()[0]
        baseline = hip_ctx.upload(baseline_batch(host_rows, clusters, table))
        batch = rows.to_batch(index, dev)
        assert batch.has_source_columns() == baseline.has_source_columns() == (which != "none")
        assert batch.path_group_ids().tolist() == M.path_side(clusters, table)[0]
        assert np.array_equal(batch.cluster_totals(), baseline.cluster_totals()) and batch.cluster_totals().sum() == len(lists)
        if which != "none":
            assert np.array_equal(batch.path_group_ids(), baseline.path_group_ids())
            multiplicities = []
            for k in range(len(clusters)):
                assert batch.source_columns(k) == baseline.source_columns(k), k
                multiplicities += batch.source_columns(k)[0]
            # every haplotype of a cluster is in exactly one of its columns
            assert sum(multiplicities) == sum(len({s for p in c for s in table["source_ids"][p]}) for c in clusters)
            assert 300 in multiplicities                                       # the 300 haplotypes of path 30 alone
            assert which != "shared" or any(7 <= m < 300 for m in multiplicities)  # haplotypes 3 and 50 .. 55 carry one list
        assert small_cases.same_device_rows(batch, baseline)
        plain = rows.to_batch()   # without a table: as before, no path side
        assert not plain.has_source_columns() and small_cases.same_device_rows(plain, baseline)
        with pytest.raises(hip.EngineError):
            plain.cluster_totals()
        for b in (plain, batch, baseline):
            b.free()
        rows.free()
        alignments.free()
    finally:
        dev.free()
        index.free()


def test_bad_tables_are_refused(hip_ctx):
    lists, params, effective_length, extra = stream_case()
    table = source_tables(effective_length)["mixed"]
    off = np.concatenate([[0], np.cumsum([len(s) for s in table["source_ids"]])]).astype(np.uint64)
    ids = np.asarray([s for per_path in table["source_ids"] for s in per_path], dtype=np.uint32)

    def upload(offsets, table_ids=ids):
        return DevicePathTable(hip_ctx, PathTable(table["group_id"], table["source_count"], table["length"], table["effective_length"], offsets,
                                                  table_ids, table["name_id"]))
    broken = off.copy()
    broken[20], broken[21] = off[21], off[20]        # source_off[21] < source_off[20]; path 19 is still in order
    assert off[20] < off[21]
    with pytest.raises(hip.EngineError) as err:
        upload(broken)
    assert "(-3)" in str(err.value) and "path 20:" in str(err.value)
    with pytest.raises(hip.EngineError) as err:
        upload(off, ids[:-1])                        # the offsets end beyond the ids
    assert "(-3)" in str(err.value) and "path 59:" in str(err.value)
    short = off.copy()
    short[-1] -= 1                                   # the offsets end before the ids do
    with pytest.raises(hip.EngineError) as err:
        upload(short)
    assert "(-3)" in str(err.value) and "path 59:" in str(err.value)
    upload(off).free()                               # the context still works
    # a table of another size than the index
    index = build_index(hip_ctx, IndexParams(**IM.default_params(61)), [FragmentLists.from_lists(lists)], extra)
    dev = upload(off)
    try:
        with pytest.raises(hip.EngineError):
            index.name_groups(dev)
    finally:
        dev.free()
        index.free()


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def python_table(table):
    off = ids = None
    if table["source_ids"] is not None:
        off = np.concatenate([[0], np.cumsum([len(s) for s in table["source_ids"]])]).astype(np.uint64)
        ids = [s for per_path in table["source_ids"] for s in per_path]
    return PathTable(table["group_id"], table["source_count"], table["length"], table["effective_length"], off, ids, table["name_id"])


def assert_same_estimates(got, ref, exact=True):
    bit_equal = True
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.total_count == r.total_count
        gk, rk = g.keyed(), r.keyed()
        assert set(gk) == set(rk)
        for key in rk:
            same = gk[key][0] == rk[key][0] and np.array_equal(np.asarray(gk[key][1]), np.asarray(rk[key][1]))
            bit_equal = bit_equal and same
            if exact:
                assert same, key
            else:
                assert small_cases.rel_close(gk[key][0], rk[key][0], rel=1e-6) and small_cases.rel_close(gk[key][1], rk[key][1], rel=1e-6), key
    return bit_equal


def test_haplotype_transcripts_from_fragments_with_the_table(hip_ctx):
    """`-i haplotype-transcripts` on the batch prepared from fragments with a path table.  The batch has its haplotype columns, and
    the run equals, bit for bit, the run on the uploaded baseline: the same rows downloaded and the table permuted on the host,
    through rpvg_hip_batch_upload.  Against the table-less prepare_from_fragments, which groups on the host, the group sets are
    identical and the values within 1e-6.  (Single end: the rows need no density table, so the rows built here through the
    context and those the harness builds are the same kernels on the same input.)"""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import ClusterBatch, make_params
    lists, params, effective_length, extra = stream_case()
    params = dict(params, is_single_end=True)
    want = IM.run_model(params, [lists], extra)
    clusters = M.cluster_lists(want["arrays"])
    # transcripts of three consecutive paths; a haplotype carries at most one path of a transcript (the estimator refuses anything
    # else, as the reference asserts); haplotypes 12 .. 14 carry the path list of haplotype 0 (multiplicity 4)
    sources = [[h for h in range(12) if h % 3 == p % 3 and (h + p // 3) % 4 != 0] for p in range(60)]
    sources = [ids + [12, 13, 14] if 0 in ids else ids for ids in sources]
    table = dict(source_tables(effective_length)["none"], group_id=[p // 3 for p in range(60)], source_count=[len(ids) for ids in sources],
                 source_ids=sources)
    chunks = [FragmentLists.from_lists(c) for c in IM.chunked(lists, 130)]
    index = build_index(hip_ctx, IndexParams(**params), chunks, extra)
    try:
        alignments = index.alignments(effective_length)
        rows = alignments.build_rows(RowParams(is_single_end=True, min_noise_prob=1e-4, prob_precision=1e-8))
        host_rows = rows.download()[0]
        rows.free()
        alignments.free()
    finally:
        index.free()
    global_paths = ClusterBatch.from_clusters([dict(paths=[dict(group_id=table["group_id"][p], source_count=table["source_count"][p],
                                                                source_ids=table["source_ids"][p], effective_length=table["effective_length"][p])
                                                           for p in range(60)], rows=[])])
    e = eng_mod.Engine(0)
    try:
        kw = dict(extra_sets=extra, min_noise_prob=1e-4, prob_precision=1e-8)
        with_table = e.prepare_from_fragments(chunks, IndexParams(**params), path_table=python_table(table), **kw)
        assert with_table.has_source_columns
        assert np.array_equal(with_table.cluster_paths, want["arrays"]["cluster_paths"])
        without = e.prepare_from_fragments(chunks, IndexParams(**params), global_paths, **kw)
        assert not without.has_source_columns
        baseline = e.prepare(baseline_batch(host_rows, clusters, table))
        assert baseline.has_source_columns
        got, _ = e.run("haplotype-transcripts", make_params(), with_table)
        ref, _ = e.run("haplotype-transcripts", make_params(), baseline)
        host_grouped, _ = e.run("haplotype-transcripts", make_params(), without)
    finally:
        e.close()
    assert len(got) == want["num_clusters"] and sum(g.total_count for g in got) == len(lists)
    assert_same_estimates(got, ref, exact=True)
    bit_equal = assert_same_estimates(got, host_grouped, exact=False)
    print("with the table against the table-less route:", "bit-equal" if bit_equal else "within 1e-6, not bit-equal")


def test_transcripts_with_collapsed_names(hip_ctx):
    """`-i transcripts --path-info`: prepare_from_fragments(collapse_names=True) against the batch uploaded from the model's collapsed
    clusters: rows of the uploaded model output (the model's groups and source counts), collapsed paths of the model.  Single end,
    as above."""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import make_params
    lists, params, effective_length, extra = stream_case()
    params = dict(params, is_single_end=True)
    want = IM.run_model(params, [lists], extra)
    clusters = M.cluster_lists(want["arrays"])
    table = source_tables(effective_length)["none"]
    path_group, _ = M.name_groups(clusters, table["name_id"])
    collapsed = M.collapsed_paths(clusters, table)
    model_clusters = IM.model_clusters(want, effective_length)
    at = 0
    for cl, paths in zip(model_clusters, clusters):
        for info, p in zip(cl["paths"], paths):
            info["source_count"] = table["source_count"][p]
            info["group"] = path_group[at]
            at += 1
    uploaded = hip_ctx.upload_alignments(AlignmentBatch.from_clusters(model_clusters))
    rows = uploaded.build_rows(RowParams(is_single_end=True, min_noise_prob=1e-4, prob_precision=1e-8))
    host_rows = rows.download()[0]
    rows.free()
    uploaded.free()
    flat = [c for cl in collapsed for c in cl]
    assert host_rows.cluster_path_off.tolist() == np.concatenate([[0], np.cumsum([len(cl) for cl in collapsed])]).tolist()
    baseline_host = dataclasses.replace(host_rows, path_group_id=np.asarray([c["group_id"] for c in flat], dtype=np.uint32),
                                        path_source_count=np.asarray([c["source_count"] for c in flat], dtype=np.uint32),
                                        path_source_off=np.zeros(len(flat) + 1, dtype=np.uint64), source_id=np.zeros(0, dtype=np.uint32),
                                        path_effective_length=np.asarray([c["effective_length"] for c in flat], dtype=np.float64))
    chunks = [FragmentLists.from_lists(c) for c in IM.chunked(lists, 130)]
    e = eng_mod.Engine(0)
    try:
        from_fragments = e.prepare_from_fragments(chunks, IndexParams(**params), path_table=python_table(table), collapse_names=True,
                                                  extra_sets=extra, min_noise_prob=1e-4, prob_precision=1e-8)
        baseline = e.prepare(baseline_host)
        got, _ = e.run("transcripts", make_params(), from_fragments)
        ref, _ = e.run("transcripts", make_params(), baseline)
    finally:
        e.close()
    assert len(got) == want["num_clusters"] and sum(g.total_count for g in got) == len(lists)
    assert [len(g.abundances) for g in got] == [len(cl) for cl in collapsed]
    assert_same_estimates(got, ref, exact=True)
