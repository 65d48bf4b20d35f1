"""The alignment-path index on the GPU (rpvg_amd/csrc/align_index.hip, include/rpvg_index.h) against the plain-Python model of
tests/align_index_model.py, which tests/test_align_index_model.py pins to a case written out from the reference's lines.
Every comparison is exact: integers, byte for byte."""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.index import AlignmentIndex, FragmentLists, IndexParams, build_index
from rpvg_amd.rows import AlignmentBatch, RowParams
from tests import align_index_model as M

pytestmark = pytest.mark.gpu


def device_params(params, hash_bits=0):
    return IndexParams(hash_bits=hash_bits, **params)


def run_device(ctx, params, chunks, extra_sets=None, hash_bits=0):
    """(arrays by name, frag_counts, info) of the device for the stream `chunks` (sequences of list dicts)."""
    index = build_index(ctx, device_params(params, hash_bits), [FragmentLists.from_lists(c) for c in chunks], extra_sets)
    try:
        return index.view().arrays(), index.frag_counts(), index.info
    finally:
        index.free()


def assert_equals_model(got, want):
    arrays, counts, info = got
    assert (info.num_lists, info.num_distinct, info.num_clusters) == (want["num_lists"], want["num_distinct"], want["num_clusters"])
    assert counts.dtype == np.uint32 and np.array_equal(counts, want["frag_counts"])
    assert set(arrays) == set(want["arrays"])
    for name, w in want["arrays"].items():
        assert arrays[name].dtype == w.dtype and arrays[name].shape == w.shape and np.array_equal(arrays[name], w), name


def check(ctx, params, chunks, extra_sets=None, hash_bits=0):
    want = M.run_model(params, chunks, extra_sets or ())
    got = run_device(ctx, params, chunks, extra_sets, hash_bits)
    assert_equals_model(got, want)
    return got, want


def same_bytes(a, b):
    return set(a) == set(b) and all(a[n].tobytes() == b[n].tobytes() for n in a)


# ---- the hand-written case ---------------------------------------------------------------------------------------

def test_hand_case(hip_ctx):
    params, lists = M.hand_case()
    check(hip_ctx, params, [lists])
    check(hip_ctx, params, [lists], extra_sets=[[2, 4]])


# ---- lists that differ in exactly one field stay distinct ------------------------------------------------------------

def one_field_stream(seed=11, num_paths=300, num_bases=320):
    """Base lists over a few hundred paths, each followed somewhere in the stream by copies that differ from it in exactly one
    field (lists of two alignments or more, so that nothing is normalised away), plus the pair [a | b c] / [a b | c]."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(num_bases):
        p0 = int(rng.integers(0, num_paths - 8))
        ids = [sorted(int(x) for x in rng.choice(np.arange(p0, p0 + 8), size=int(rng.integers(2, 5)), replace=False)) for _ in range(int(rng.integers(2, 4)))]
        aligns = [(int(rng.integers(10, 200)), int(rng.integers(40, 250)), int(rng.integers(1, 600)), i) for i in ids]
        base = M.mk(aligns, 1, 40, -7)
        lists.append(base)

        def variant(**kw):
            v = M.mk(base["aligns"], base["is_simple"], base["min_mapq"], base["noise_score"])
            v.update(kw)
            return v

        def with_align(j, s=0, a=0, f=0):
            al = [tuple(x) for x in base["aligns"]]
            al[j] = (al[j][0] + s, al[j][1] + a, al[j][2] + f, al[j][3])
            return variant(aligns=[(x[0], x[1], x[2], list(x[3])) for x in al])

        j = int(rng.integers(0, len(aligns)))
        other_id = [p for p in range(p0, p0 + 8) if p not in aligns[j][3]][0]
        swapped = sorted(aligns[j][3][1:] + [other_id])
        lists += [variant(is_simple=0), variant(min_mapq=41), variant(noise_score=-8), with_align(j, s=1), with_align(j, a=1), with_align(j, f=1),
                  variant(aligns=[(x[0], x[1], x[2], list(swapped if k == j else x[3])) for k, x in enumerate(aligns)]),
                  variant(aligns=[(x[0], x[1], x[2], list(x[3])) for x in aligns[:-1]] if len(aligns) > 2 else
                          [(x[0], x[1], x[2], list(x[3])) for x in aligns] + [(aligns[0][0], aligns[0][1], aligns[0][2], list(aligns[0][3]))])]
    # the same flattened ids with the alignment boundary moved
    lists.append(M.mk([(50, 100, 200, [1]), (50, 100, 200, [2, 3])]))
    lists.append(M.mk([(50, 100, 200, [1, 2]), (50, 100, 200, [3])]))
    order = rng.permutation(len(lists))
    return [lists[int(i)] for i in order] + [lists[int(i)] for i in order[:200]]  # and some true repeats


def test_one_field_differences_stay_distinct(hip_ctx):
    lists = one_field_stream()
    params = M.default_params(300)
    (arrays, _, info), want = check(hip_ctx, params, [lists])
    distinct = len({repr(ls) for ls in lists})
    assert 2000 < distinct == info.num_distinct < len(lists)  # nothing is normalised here: every variant is a list of its own
    assert int(arrays["read_count"].sum()) == len(lists)


# ---- normalisation against the histogram --------------------------------------------------------------------------------

def test_one_alignment_lists_merge_and_are_counted_at_their_own_lengths(hip_ctx):
    params = M.default_params(20, max_frag_length=500, pre_frag_loc=123)
    lists = [M.mk([(10 + i, 50 + i, 100 + 3 * i, [4, 7])], 1, 30, -2) for i in range(40)] + [M.mk([(1, 1, 123, [4, 7])], 1, 30, -2)]
    (arrays, counts, info), _ = check(hip_ctx, params, [lists])
    assert info.num_distinct == 1 and arrays["read_count"].tolist() == [41]
    assert (arrays["align_score_sum"].tolist(), arrays["align_length"].tolist(), arrays["align_frag_length"].tolist()) == ([1], [1], [123])
    assert counts.sum() == 41 and all(counts[100 + 3 * i] == 1 for i in range(40)) and counts[123] == 1


# ---- the histogram gate ------------------------------------------------------------------------------------------------

def test_histogram_gate(hip_ctx):
    params = M.default_params(10, max_frag_length=64)
    lists = [M.mk([(5, 5, 17, [1])], 1, 29), M.mk([(5, 5, 17, [1])], 1, 30), M.mk([(5, 5, 18, [1])], 0, 60), M.mk([(5, 5, 18, [1])], 1, 60),
             M.mk([(5, 5, 64, [2])], 1, 255),                                  # the maximum lands in the last bin
             M.mk([(5, 5, 65, [2])], 1, 29), M.mk([(5, 5, 0, [2])], 0, 60),     # uncounted lists may have any length
             M.mk([(5, 5, 30000, [2]), (5, 5, 0, [3])], 0, 60)]
    (_, counts, _), _ = check(hip_ctx, params, [lists])
    want = np.zeros(65, dtype=np.uint32)
    want[[17, 18, 64]] = 1
    assert np.array_equal(counts, want)
    (_, counts, _), _ = check(hip_ctx, dict(params, is_single_end=True), [lists + [M.mk([(5, 5, 65, [2])], 1, 60), M.mk([(5, 5, 0, [2])], 1, 60)]])
    assert not counts.any()  # single end: nothing is counted, nothing is checked
    # the global-atomics route: more bins than the workgroup histogram holds
    check(hip_ctx, dict(params, max_frag_length=65535), [lists + [M.mk([(5, 5, 65535, [2])], 1, 60)]])


@pytest.mark.parametrize("bad", [
    M.mk([(5, 5, 65, [2])], 1, 60), M.mk([(5, 5, 0, [2])], 1, 30),                                  # counted: above the maximum, zero
    M.mk([]), M.mk([(5, 5, 9, [])]), M.mk([(5, 5, 9, [3, 3])]), M.mk([(5, 5, 9, [4, 3])]), M.mk([(5, 5, 9, [10])]),
    M.mk([(5, 5, 9, [1])], noise_score=1)], ids=["above_max", "zero", "no_alignments", "no_paths", "repeated_id", "descending_ids", "id_out_of_range", "positive_noise"])
def test_invalid_chunks_are_refused_and_change_nothing(hip_ctx, bad):
    params = M.default_params(10, max_frag_length=64)
    good = M.random_stream(5, num_paths=10, num_lists=60, num_templates=20, max_frag_length=64)
    index = AlignmentIndex(hip_ctx, device_params(params))
    try:
        index.add(FragmentLists.from_lists(good[:30]))
        with pytest.raises(hip.EngineError) as err:
            index.add(FragmentLists.from_lists(good[30:33] + [bad] + good[33:36]))
        assert "(-3)" in str(err.value) and "list 3 of the chunk (33 of the stream)" in str(err.value)
        index.add(FragmentLists.from_lists(good[30:]))  # the context and the index still work
        index.finish()
        assert_equals_model((index.view().arrays(), index.frag_counts(), index.info), M.run_model(params, [good]))
    finally:
        index.free()


def test_bad_offsets_and_parameters_are_refused(hip_ctx):
    params = M.default_params(10, max_frag_length=64)
    with pytest.raises(hip.EngineError):
        AlignmentIndex(hip_ctx, IndexParams(num_paths=10, max_frag_length=65536))
    good = FragmentLists.from_lists(M.random_stream(6, num_paths=10, num_lists=20, num_templates=8, max_frag_length=64))
    index = AlignmentIndex(hip_ctx, device_params(params))
    try:
        for field, at in (("list_align_off", 5), ("align_path_off", 3)):
            broken = FragmentLists(**{n: getattr(good, n).copy() for n in FragmentLists._DTYPES})
            off = getattr(broken, field)
            off[at] = off[at + 1] + 1 if at + 2 < len(off) else off[at]  # not monotone
            with pytest.raises(hip.EngineError) as err:
                index.add(broken)
            assert "(-3)" in str(err.value)
        index.add(good)
        info = index.finish()
        assert info.num_lists == 20
        with pytest.raises(hip.EngineError):
            index.add(good)  # finished
    finally:
        index.free()


# ---- long lists, a long duplicate run --------------------------------------------------------------------------------

def test_long_lists(hip_ctx):
    lists = M.random_stream(21, num_paths=200, num_lists=3000, num_templates=400, long_lists=12)
    entries = [sum(len(a[3]) for a in ls["aligns"]) for ls in lists]
    assert max(entries) > 64 and sum(16 < e <= 64 for e in entries) > 10
    check(hip_ctx, M.default_params(200), [lists])


def test_long_duplicate_run_across_workgroups(hip_ctx):
    others = M.random_stream(22, num_paths=150, num_lists=5000, num_templates=900)
    repeated = M.mk([(33, 120, 240, [7, 9]), (31, 120, 250, [8])], 1, 60, -4)
    lists = []
    for o in others:
        lists += [repeated, o]
    (arrays, _, info), _ = check(hip_ctx, M.default_params(150), [lists])
    assert info.num_lists == 10000 and int(arrays["read_count"].max()) >= 5000


# ---- chunking, hash width ----------------------------------------------------------------------------------------------

def test_chunk_invariance(hip_ctx):
    lists = M.random_stream(31, num_paths=90, num_lists=400, num_templates=120, long_lists=2)
    params = M.default_params(90)
    (whole, whole_counts, _), _ = check(hip_ctx, params, [lists])
    for chunks in (M.chunked(lists, 1), M.chunked(lists, 7), [[], lists[:150], [], [], lists[150:], []]):
        arrays, counts, info = run_device(hip_ctx, params, chunks)
        assert same_bytes(arrays, whole) and np.array_equal(counts, whole_counts) and info.num_lists == 400
    big = M.random_stream(32, num_paths=400, num_lists=3500, num_templates=700)
    (whole, whole_counts, _), _ = check(hip_ctx, M.default_params(400), [big])
    arrays, counts, _ = run_device(hip_ctx, M.default_params(400), M.chunked(big, 1000))
    assert same_bytes(arrays, whole) and np.array_equal(counts, whole_counts)


def test_forced_collisions_give_the_same_index(hip_ctx):
    lists = M.random_stream(41, num_paths=120, num_lists=1500, num_templates=300, long_lists=3)
    params = M.default_params(120)
    (full, full_counts, full_info), want = check(hip_ctx, params, [lists], hash_bits=64)
    for bits in (1, 4):
        arrays, counts, info = run_device(hip_ctx, params, [lists], hash_bits=bits)
        assert same_bytes(arrays, full) and np.array_equal(counts, full_counts)
        # at most 2^bits runs: every distinct list but the run heads is found by the collision path, with all its repeats
        assert info.num_collision_lists >= 1500 - int(full["read_count"].max()) * (1 << bits) > 0
        assert info.num_distinct == full_info.num_distinct == want["num_distinct"]
    assert full_info.num_collision_lists == 0  # 300 templates in 64 bits (a collision there is a 1e-15 event)


# ---- cluster edges -----------------------------------------------------------------------------------------------------

def test_empty_stream_and_cluster_edges(hip_ctx):
    params = M.default_params(7)
    (arrays, counts, info), _ = check(hip_ctx, params, [])
    assert info.num_clusters == 7 and arrays["rank_cluster"].tolist() == [6, 5, 4, 3, 2, 1, 0] and not counts.any()
    assert arrays["cluster_paths"].tolist() == [6, 5, 4, 3, 2, 1, 0] and arrays["cluster_read_off"].tolist() == [0] * 8
    check(hip_ctx, params, [[], []], extra_sets=[[1, 5], [5, 3]])
    # clusters without a list, ties on the number of lists (the larger index first), sets that join two clusters with lists
    lists = [M.mk([(9, 9, 9, [0])]), M.mk([(9, 9, 9, [2]), (8, 9, 9, [2])]), M.mk([(9, 9, 9, [4])]), M.mk([(9, 9, 9, [4])], 0),
             M.mk([(9, 9, 9, [6])]), M.mk([(9, 9, 9, [0])])]
    (arrays, _, _), _ = check(hip_ctx, params, [lists])
    assert arrays["rank_cluster"].tolist() == [4, 6, 2, 0, 5, 3, 1]
    (arrays, _, info), _ = check(hip_ctx, params, [lists], extra_sets=[[0, 6], [1, 3]])
    assert info.num_clusters == 5 and arrays["rank_cluster"].tolist() == [3, 0, 2, 4, 1]
    assert arrays["first_occurrence"].tolist() == [2, 3, 0, 4, 1]


def test_old_entry_point_gives_the_same_clusters(hip_ctx):
    lists = M.random_stream(51, num_paths=500, num_lists=2500, num_templates=600)
    extra = [[3, 250], [499, 0, 17]]
    (arrays, _, info), want = check(hip_ctx, M.default_params(500), [lists], extra_sets=extra)
    sets = [[p for a in ls["aligns"] for p in a[3]] for ls in lists] + extra
    path_to_cluster, members = hip_ctx.path_clusters(500, sets)
    assert np.array_equal(path_to_cluster, arrays["path_to_cluster"]) and len(members) == info.num_clusters
    assert members == want["clusters"]


# ---- a larger stream: the multi-block routes of sort and scan -----------------------------------------------------------

def test_larger_stream(hip_ctx):
    lists = M.random_stream(61, num_paths=20000, num_lists=200000, num_templates=25000, long_lists=4)
    (_, _, info), _ = check(hip_ctx, M.default_params(20000), M.chunked(lists, 64000))
    assert info.num_distinct > 20000 and info.num_clusters > 1000


# ---- end to end: rows, one estimator run ---------------------------------------------------------------------------------

def end_to_end_case():
    lists = M.random_stream(71, num_paths=60, num_lists=4000, num_templates=500, long_lists=3, max_frag_length=600)
    scaled = {}  # noise scores on the scale of the row construction (Utils::noise_score_log_base = 1e-6): noise probabilities 0.03 .. 0.6
    for ls in lists:
        if id(ls) not in scaled:
            scaled[id(ls)] = dict(ls, noise_score=-500000 * (1 + (-ls["noise_score"]) % 7))
    lists = [scaled[id(ls)] for ls in lists]
    params = M.default_params(60)
    rng = np.random.default_rng(72)
    effective_length = rng.uniform(300.0, 3000.0, size=60)
    return lists, params, effective_length


def frag_table():
    v = np.arange(65536, dtype=np.float64)
    return -0.5 * ((v - 300.0) / 50.0) ** 2 - np.log(50.0 * np.sqrt(2 * np.pi))


def test_rows_from_the_index_equal_rows_from_the_uploaded_model_output(hip_ctx):
    lists, params, effective_length = end_to_end_case()
    want = M.run_model(params, [lists])
    index = build_index(hip_ctx, device_params(params), [FragmentLists.from_lists(c) for c in M.chunked(lists, 1500)])
    row_params = RowParams(frag_length_log_prob=frag_table())
    try:
        from_index = index.alignments(effective_length)
        uploaded = hip_ctx.upload_alignments(AlignmentBatch.from_clusters(M.model_clusters(want, effective_length)))
        a = from_index.build_rows(row_params).download()[0]
        b = uploaded.build_rows(row_params).download()[0]
        assert a.num_clusters == b.num_clusters == want["num_clusters"] and int(a.cluster_row_off[-1]) > 100
        for name in ("cluster_row_off", "cluster_path_off", "row_count", "row_noise", "row_grp_off", "grp_prob", "grp_idx_off", "path_idx"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        # the effective lengths can be replaced on the result as on an uploaded batch: lengths in the order of cluster_paths
        lengths = (np.arange(60, dtype=np.uint32) * 37 + 400)[want["arrays"]["cluster_paths"]]
        assert np.array_equal(from_index.set_effective_lengths(lengths, 300.0, 50.0, 0.0), uploaded.set_effective_lengths(lengths, 300.0, 50.0, 0.0))
        a = from_index.build_rows(row_params).download()[0]
        b = uploaded.build_rows(row_params).download()[0]
        assert a.grp_prob.tobytes() == b.grp_prob.tobytes() and a.row_noise.tobytes() == b.row_noise.tobytes()
        from_index.free()
        uploaded.free()
    finally:
        index.free()


def test_estimates_through_prepare_from_fragments_equal_prepare_from_alignments(hip_ctx):
    """One `-i haplotype-transcripts` run on the batch the harness prepares from the stream of fragments against the same run on the
    batch it prepares from the model's distinct lists: the same clusters in the same order, the same bits."""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import ClusterBatch, make_params
    lists, params, effective_length = end_to_end_case()
    want = M.run_model(params, [lists], extra_sets=[[0, 59]])

    def path(p):  # every path its own haplotype, transcripts of three consecutive paths
        return dict(group_id=(p // 3) % 2, source_count=1, source_ids=[p], effective_length=float(effective_length[p]))

    global_paths = ClusterBatch.from_clusters([dict(paths=[path(p) for p in range(60)], rows=[])])
    a = want["arrays"]
    ordered_paths = ClusterBatch.from_clusters([dict(paths=[path(int(p)) for p in a["cluster_paths"][int(a["cluster_path_off"][r]):int(a["cluster_path_off"][r + 1])]],
                                                     rows=[]) for r in range(want["num_clusters"])])
    e = eng_mod.Engine(0)
    try:
        from_fragments = e.prepare_from_fragments([FragmentLists.from_lists(c) for c in M.chunked(lists, 1300)], device_params(params), global_paths,
                                                  extra_sets=[[0, 59]], frag=(300.0, 50.0, 0.0, 10), min_noise_prob=1e-4)
        info = from_fragments.index_info
        assert (info.num_lists, info.num_distinct, info.num_clusters) == (want["num_lists"], want["num_distinct"], want["num_clusters"])
        assert np.array_equal(from_fragments.frag_counts, want["frag_counts"])
        assert np.array_equal(from_fragments.cluster_paths, a["cluster_paths"]) and np.array_equal(from_fragments.cluster_path_off, a["cluster_path_off"])
        from_alignments = e.prepare_from_alignments(AlignmentBatch.from_clusters(M.model_clusters(want, effective_length)), ordered_paths,
                                                    frag=(300.0, 50.0, 0.0, 10), min_noise_prob=1e-4)
        got, _ = e.run("haplotype-transcripts", make_params(), from_fragments)
        ref, _ = e.run("haplotype-transcripts", make_params(), from_alignments)
    finally:
        e.close()
    assert len(got) == len(ref) == want["num_clusters"] and sum(g.total_count for g in got) == len(lists)
    for g, r in zip(got, ref):
        assert g.total_count == r.total_count
        gk, rk = g.keyed(), r.keyed()
        assert set(gk) == set(rk)
        for key in rk:
            assert gk[key][0] == rk[key][0]
            assert np.array_equal(np.asarray(gk[key][1]), np.asarray(rk[key][1]))
