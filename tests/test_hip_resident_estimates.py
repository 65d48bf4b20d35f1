"""Resident estimates on the GPU (rpvg_amd/csrc/estimates_gather.hip, include/rpvg_table.h): hand-made parts in host and in device
memory against the plain-Python model of tests/resident_estimates_model.py at the edges of the scatter's step, the special units
and batches, every refusal with a valid gather behind it, the three nested calls with their device block kept against the model
applied to the call's own host view, and the estimator's resident route against Engine.run and the container route.  Every array is
compared byte for byte."""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd import resident_estimates as res
from rpvg_amd.batch import ClusterBatch
from tests import resident_estimates_model as R
from tests import small_cases

pytestmark = pytest.mark.gpu

STEP_EDGES = (0, 1, 63, 64, 65, 128, 129)   # sets of a cluster either side of the scatter's step of 64


def _cluster(num_paths, reads):
    """A cluster of num_paths single-haplotype paths of one transcript with `reads` reads on path 0 (0: a cluster without rows)."""
    paths = [dict(group_id=0, source_ids=[p], source_count=1, effective_length=100.0 + p) for p in range(num_paths)]
    return dict(paths=paths, rows=[small_cases.finish_row(reads, 0.01, {0: 0.004})] if reads else [])


class _Batch:
    """K clusters of the given path counts on the device: cluster k has 3 k + 2 reads."""

    def __init__(self, ctx, path_counts):
        self.ctx = ctx
        self.host = ClusterBatch.from_clusters([_cluster(n, 3 * k + 2) for k, n in enumerate(path_counts)])
        self.dev = ctx.upload(self.host)
        self.cluster_path_off = np.concatenate([[0], np.cumsum(path_counts)]).astype(np.uint64)
        self.totals = self.dev.cluster_totals() if len(path_counts) else np.zeros(0)
        self.eff = np.arange(int(self.cluster_path_off[-1]), dtype=np.float64) * 0.5 + 17.25

    def free(self):
        self.dev.free()


class _DeviceArrays:
    """The arrays of model parts copied to device memory by hand (on_device = 1)."""

    def __init__(self, ctx):
        self.ctx, self.pointers = ctx, []

    def put(self, array):
        a = np.ascontiguousarray(array)
        if a.size == 0:
            return 0
        pointer = self.ctx.malloc(a.nbytes)
        self.pointers.append(pointer)
        self.ctx.h2d(pointer, a)
        return pointer

    def part(self, p):
        names = [name for name, _ in res._PART_ARRAYS if name in p]
        return res.EstimatesPart.from_device(p["width"], p["unit_cluster"], len(p["path_off"]) - 1, len(p["set_posterior"]),
                                             **{name: self.put(np.asarray(p[name], dtype=dict(res._PART_ARRAYS)[name])) for name in names})

    def free(self):
        for pointer in self.pointers:
            self.ctx.free(pointer)
        self.pointers = []


def _host_part(p):
    return res.EstimatesPart.from_arrays(p["width"], p["unit_cluster"], **{name: p[name] for name, _ in res._PART_ARRAYS if name in p})


def _same(got, want, batch):
    """got: a FlatEstimates of rpvg_hip_flat_estimates_get; want: the model's arrays."""
    for name in R.FLAT_NAMES:
        a, b = getattr(got, name), want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            at = int(np.flatnonzero(a != b)[0]) if (a != b).any() else -1
            raise AssertionError(f"{name}[{at}]: {a[at]!r} != {b[at]!r}")
    assert got.cluster_path_off.tobytes() == batch.cluster_path_off.tobytes()
    assert got.path_effective_length.tobytes() == batch.eff.tobytes()


def _gather(ctx, batch, parts, on_device):
    """The gather of model parts, from host memory or from device memory: (FlatEstimates, sizes of the device view)."""
    arrays = _DeviceArrays(ctx)
    try:
        c_parts = [arrays.part(p) if on_device else _host_part(p) for p in parts]
        est = res.gather(ctx, batch.dev, c_parts, batch.eff)
        try:
            view = est.view()
            sizes = (int(view.num_clusters), int(view.num_sets), int(view.num_members), int(view.num_abundances), int(view.num_paths), int(view.on_device))
            return est.get(), sizes
        finally:
            est.free()
    finally:
        arrays.free()


def _check(ctx, batch, parts, on_device):
    want = R.gather(batch.cluster_path_off, batch.totals, parts)
    got, sizes = _gather(ctx, batch, parts, on_device)
    _same(got, want, batch)
    S, M = len(want["posteriors"]), len(want["members"])
    assert sizes == (len(batch.totals), S, M, M, len(batch.eff), 1)
    return got


@pytest.fixture(scope="module")
def edge_batch(hip_ctx):
    rng = np.random.default_rng(31)
    b = _Batch(hip_ctx, [int(x) for x in rng.integers(1, 12, size=len(STEP_EDGES) + 2)])
    yield b
    b.free()


@pytest.mark.parametrize("on_device", (0, 1))
def test_hand_case(hip_ctx, on_device):
    cluster_path_off, totals, parts, expected = R.hand_case()
    batch = _Batch(hip_ctx, np.diff(cluster_path_off).tolist())
    try:
        batch.totals = batch.dev.cluster_totals()
        assert batch.totals.tolist() == [2.0, 5.0, 8.0, 11.0]
        got, _ = _gather(hip_ctx, batch, parts, on_device)
        for name in R.FLAT_NAMES:
            want = expected[name] if name != "noise_count" else [2.0, 5.0, 7.0, 0.75]   # the batch's own totals for clusters 0 and 1
            assert getattr(got, name).tolist() == want, name
    finally:
        batch.free()


@pytest.mark.parametrize("on_device", (0, 1))
@pytest.mark.parametrize("width", (0, 1, 3, 8))
def test_step_edges_in_every_form(hip_ctx, edge_batch, width, on_device):
    """0, 1, 63, 64, 65, 128 and 129 sets per cluster; width 0 mixes single and double sets, the others every size 1 .. width."""
    rng = np.random.default_rng(100 + width)
    K = len(edge_batch.totals)
    clusters = [int(c) for c in rng.permutation(K)[:len(STEP_EDGES)]]
    part = R.make_part(rng, width, clusters, list(STEP_EDGES), np.diff(edge_batch.cluster_path_off))
    got = _check(hip_ctx, edge_batch, [part], on_device)
    sizes = set(np.diff(got.member_off).tolist())
    assert sizes == ({1, 2} if width == 0 else set(range(1, width + 1)))
    assert sorted(np.diff(got.set_off).tolist()) == sorted(list(STEP_EDGES) + [0, 0])


@pytest.mark.parametrize("on_device", (0, 1))
def test_special_units_and_interleaved_parts(hip_ctx, edge_batch, on_device):
    rng = np.random.default_rng(41)
    counts = np.diff(edge_batch.cluster_path_off)
    # a unit without subsets (its noise is the cluster's total), clusters 4 and 7 in no unit, parts of three widths whose clusters interleave
    a = R.make_part(rng, 0, [6, 0, 3], [70, 0, 5], counts, no_subsets=(1,))
    b = R.make_part(rng, 5, [1, 8], [9, 130], counts)
    c = R.make_part(rng, 2, [5, 2], [64, 1], counts)
    got = _check(hip_ctx, edge_batch, [a, b], on_device)
    assert got.noise_count[0] == edge_batch.totals[0] and got.noise_count[4] == edge_batch.totals[4] and got.noise_count[6] == a["cluster_noise_count"][0]
    got = _check(hip_ctx, edge_batch, [a, b, c], on_device)
    assert np.diff(got.set_off).tolist() == [0, 9, 1, 5, 0, 64, 70, 0, 130]
    _check(hip_ctx, edge_batch, [c, R.make_part(rng, 8, [], [], counts), a], on_device)   # a part without units in the middle


def test_empty_batches_and_no_parts(hip_ctx, edge_batch):
    got = _check(hip_ctx, edge_batch, [], 0)                      # zero parts: every cluster without sets, its total as noise
    assert got.noise_count.tobytes() == edge_batch.totals.tobytes() and got.member_off.tolist() == [0]
    rng = np.random.default_rng(43)
    for counts in ([], [4]):                                      # K = 0 and K = 1
        batch = _Batch(hip_ctx, counts)
        try:
            _check(hip_ctx, batch, [], 0)
            if counts:
                for on_device in (0, 1):
                    _check(hip_ctx, batch, [R.make_part(rng, 3, [0], [65], counts)], on_device)
        finally:
            batch.free()


def test_two_builds_give_the_same_bytes(hip_ctx, edge_batch):
    rng = np.random.default_rng(44)
    counts = np.diff(edge_batch.cluster_path_off)
    parts = [R.make_part(rng, 0, [2, 7, 4], [129, 64, 33], counts), R.make_part(rng, 8, [0, 5], [65, 127], counts)]
    first, _ = _gather(hip_ctx, edge_batch, parts, 1)
    second, _ = _gather(hip_ctx, edge_batch, parts, 1)
    for name in R.FLAT_NAMES:
        assert getattr(first, name).tobytes() == getattr(second, name).tobytes(), name


def _refusal_cases(counts):
    """(name, parts, part, unit, why) of the model: one case per refusal, built from valid parts."""
    rng = np.random.default_rng(45)

    def parts():
        r = np.random.default_rng(46)
        return [R.make_part(r, 0, [6, 0, 3], [70, 0, 5], counts, no_subsets=(1,)), R.make_part(r, 3, [1, 8], [9, 130], counts)]

    cases = []

    def case(name, change):
        p = parts()
        change(p)
        cases.append((name, p))

    def planted(name, index, value, part=1):
        def change(p):
            p[part][name][index] = value
        return change

    case("unit_cluster beyond K", planted("unit_cluster", 1, len(counts)))
    case("a cluster listed twice", planted("unit_cluster", 0, 3))
    case("subset_off decreases", planted("subset_off", 1, 1 << 40))
    case("path_off beyond L", lambda p: p[1]["path_off"].__setitem__(int(p[1]["subset_off"][1]), 1 << 33))
    case("set_count beyond the slots", planted("set_count", 1, 134))
    case("set_count of a unit without subsets", planted("set_count", 1, 1, part=0))
    case("set size 0", planted("set_size", 3, 0))
    case("set size beyond the width", planted("set_size", int(rng.integers(0, 9)), 4))
    case("member beyond the cluster's paths", lambda p: p[1]["set_member"].__setitem__((2, 0), int(counts[1])))
    case("second path beyond the cluster's paths", lambda p: p[0]["set_second"].__setitem__(1, int(counts[6])))

    def two(p):
        p[1]["set_size"][int(p[1]["path_off"][int(p[1]["subset_off"][1])]) + 100] = 9   # unit 1 of part 1 ...
        p[0]["set_first"][int(p[0]["path_off"][int(p[0]["subset_off"][2])]) + 1] = 1 << 20  # ... and unit 2 of part 0: the smaller
    case("two offenders", two)
    return cases


@pytest.mark.parametrize("on_device", (0, 1))
def test_refusals_name_the_smallest_offender_and_leave_a_usable_context(hip_ctx, edge_batch, on_device):
    counts = np.diff(edge_batch.cluster_path_off)
    valid = [R.make_part(np.random.default_rng(47), 3, [1, 8], [9, 130], counts)]
    for name, parts in _refusal_cases(counts):
        with pytest.raises(R.Refused) as modelled:
            R.gather(edge_batch.cluster_path_off, edge_batch.totals, parts)
        m = modelled.value
        with pytest.raises(hip.EngineError, match=rf"\(-3\).*part {m.part}, unit {m.unit}: ") as refused:
            _gather(hip_ctx, edge_batch, parts, on_device)
        reasons = {R.BAD_UNIT_CLUSTER: "unit_cluster", R.BAD_DUPLICATE: "two units", R.BAD_SUBSET_OFF: "subset_off", R.BAD_PATH_OFF: "path_off",
                   R.BAD_SET_COUNT: "set_count", R.BAD_SET_SIZE: "set size", R.BAD_MEMBER: "member"}
        assert reasons[m.why] in str(refused.value), (name, str(refused.value))
        _check(hip_ctx, edge_batch, valid, on_device)


def test_width_and_batch_refusals(hip_ctx, edge_batch):
    counts = np.diff(edge_batch.cluster_path_off)
    rng = np.random.default_rng(48)
    valid = [R.make_part(rng, 2, [1, 8], [9, 130], counts)]
    wide = R.make_part(rng, 8, [2], [3], counts)
    wide["width"] = 9
    with pytest.raises(hip.EngineError, match=r"\(-3\).*part 1: a width of 9"):
        _gather(hip_ctx, edge_batch, [valid[0], wide], 0)
    _check(hip_ctx, edge_batch, valid, 0)
    # a batch made from rows on the device without a table has no cluster totals
    from rpvg_amd.rows import AlignmentBatch
    from tests.test_hip_rows import make_alignment_clusters, params
    alignments = hip_ctx.upload_alignments(AlignmentBatch.from_clusters(make_alignment_clusters(801, n_clusters=2, reads_per_cluster=20)))
    try:
        rows = alignments.build_rows(params(min_noise=1e-4), True)
        try:
            bare = rows.to_batch()
            try:
                with pytest.raises(hip.EngineError, match=r"\(-3\).*no cluster totals"):
                    res.gather(hip_ctx, bare, [], np.ones(bare.num_paths))
            finally:
                bare.free()
        finally:
            rows.free()
    finally:
        alignments.free()
    _check(hip_ctx, edge_batch, valid, 0)


# ---- the three nested calls with their block kept ---------------------------------------------------------------------------------

def _flat_of_view(batch_host, totals, view, unit_cluster, width):
    return R.gather(batch_host.cluster_path_off, totals, [R.part_of_view(view, unit_cluster, width)])


def _check_kept(ctx, dev, host, view, part, unit_cluster, width):
    """The part from the kept block gives the flat arrays of the model applied to the call's own host view."""
    totals = dev.cluster_totals()
    want = _flat_of_view(host, totals, view, unit_cluster, width)
    est = res.gather(ctx, dev, [part], host.path_effective_length)
    try:
        got = est.get()
    finally:
        est.free()
    for name in R.FLAT_NAMES:
        assert getattr(got, name).tobytes() == want[name].tobytes(), name
    assert len(want["posteriors"]) > 0 and int(part.c.on_device) == 1 and int(part.c.width) == width
    return got


def _same_views(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        if isinstance(a[name], np.ndarray):
            assert a[name].tobytes() == b[name].tobytes(), name
        elif name != "draws":
            assert a[name] == b[name], name


def _not_kept(handle):
    part = res.CEstimatesPart()
    assert hip.lib().rpvg_hip_subset_em_part(handle, hip.C.byref(part)) == -5
    assert b"did not keep" in hip.lib().rpvg_hip_last_error()
    hip.lib().rpvg_hip_subset_em_free(handle)


def test_diploid_call_kept(hip_ctx):
    from oracle import np_oracle
    clusters = small_cases.make_batch_clusters(9301, n_clusters=5, with_empty=False)
    host = ClusterBatch.from_clusters(clusters)
    dev = hip_ctx.upload(host)
    sg = [np_oracle.source_groups(cl["paths"]) for cl in clusters]
    units = list(range(len(clusters)))[::-1]   # the matrices in another order than the clusters
    counts = [c for k in units for c in sg[k][1]]

    def matrices():   # (fresh for every call: the diploid search finishes the row collapse of the matrices it is given)
        return hip_ctx.groups(dev, units, [sg[k][0] for k in units], True, collapse_precision=1e-8)

    dg = matrices()
    try:
        plain, handle = res.nested_subset_em(dg, counts, 1e-3, 1e-3, collapse_precision=1e-8)
        assert plain["set_count"] is not None
        _not_kept(handle)
        dg.free()
        dg = matrices()
        view, part = res.nested_subset_em_kept(dg, units, counts, 1e-3, 1e-3, collapse_precision=1e-8)
        try:
            _same_views(view, plain)
            got = _check_kept(hip_ctx, dev, host, view, part, units, 0)
            assert set(np.diff(got.member_off).tolist()) <= {1, 2}
        finally:
            part.free()
    finally:
        dg.free()
        dev.free()


def test_part_refuses_a_call_that_did_no_merge(hip_ctx):
    """A batch uploaded without path_group_id: the diploid call leaves the merge to its caller, keeps its block when asked, and
    rpvg_hip_subset_em_part refuses the result; the kept block goes back with the result."""
    from oracle import np_oracle
    clusters = small_cases.make_batch_clusters(9302, n_clusters=3, with_empty=False)
    host = ClusterBatch.from_clusters(clusters)
    segments = hip.PinnedSegments(host, with_paths=False)
    dev = hip_ctx.upload_segments(host, segments)
    sg = [np_oracle.source_groups(cl["paths"]) for cl in clusters]
    units = list(range(len(clusters)))
    dg = hip_ctx.groups(dev, units, [sg[k][0] for k in units], True, collapse_precision=1e-8)
    try:
        view, handle = res.nested_subset_em(dg, [c for k in units for c in sg[k][1]], 1e-3, 1e-3, collapse_precision=1e-8, keep=True)
        try:
            assert view["set_count"] is None and int(view["subset_off"][-1]) > 0
            assert int(hip.lib().rpvg_hip_subset_em_kept_bytes(handle)) > 0
            part = res.CEstimatesPart()
            assert hip.lib().rpvg_hip_subset_em_part(handle, hip.C.byref(part)) == -5
            assert b"did no merge" in hip.lib().rpvg_hip_last_error() and not part.subset_off
        finally:
            hip.lib().rpvg_hip_subset_em_free(handle)
    finally:
        dg.free()
        dev.free()
        segments.free()


@pytest.mark.parametrize("group_size", (3, 5))
def test_full_call_kept(hip_ctx, group_size):
    from tests.test_hip_nested_full import PRECISION, _Case, _recombinant_clusters
    case = _Case(hip_ctx, _recombinant_clusters())
    units = list(range(len(case.clusters)))
    try:
        plain, handle = case.dg.nested_full_subset_em(group_size, case.log_freq, case.min_hap_prob, collapse_precision=PRECISION, keep_handle=True)
        _not_kept(handle)
        view, part = res.nested_full_subset_em_kept(case.dg, units, group_size, case.log_freq, case.min_hap_prob, collapse_precision=PRECISION)
        try:
            _same_views(view, plain)
            got = _check_kept(hip_ctx, case.dev, case.batch, view, part, units, group_size)
            assert max(np.diff(got.member_off).tolist()) <= group_size
        finally:
            part.free()
    finally:
        case.free()


def test_independent_call_kept(hip_ctx):
    from tests.test_hip_independent import PRECISION, _Case, _interleaved, _single_path
    case = _Case(hip_ctx, _single_path() + _interleaved())
    try:
        words = [rng.next_words() for rng in case.generators(7)]
        flat = [c for counts in case.counts for c in counts]
        kwargs = dict(column_counts=flat, collapse_precision=PRECISION)
        plain, handle = case.dg.nested_independent_subset_em(case.matrix_off, 2, 1e-3, words, keep_handle=True, **kwargs)
        _not_kept(handle)
        view, part = res.nested_independent_subset_em_kept(case.dg, case.units, case.matrix_off, 2, 1e-3, words, **kwargs)
        try:
            _same_views(view, plain)
            _check_kept(hip_ctx, case.dev, case.batch, view, part, case.units, 2)
        finally:
            part.free()
    finally:
        case.free()


# ---- the estimator's resident route -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from rpvg_amd import engine as eng_mod
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _tables_equal(a, b):
    for name in ("haplotype_prob", "read_count", "transcript_count", "tpm", "member_transcript_count", "member_tpm", "cluster_transcript_count"):
        assert a[name].tobytes() == b[name].tobytes(), name
    for name in ("total_transcript_count", "noise_count_total", "noise_count_share_total", "tpm_denominator"):
        assert np.float64(a[name]).tobytes() == np.float64(b[name]).tobytes(), name
    assert a["has_tpm"] == b["has_tpm"] and a["ploidy"] == b["ploidy"] and a["clusters_by_route"] == b["clusters_by_route"]


def test_run_resident_equals_the_container_route(engine, tmp_path):
    """A default haplotype-transcripts batch with a cluster without rows and enough clusters for two lanes: the resident estimates
    against Engine.run -> FlatEstimates.from_estimates, the table built from them against the table from the containers, and the
    per-path text, the joint set text and their BGZF members against those of the existing route; the two result files written from
    the resident table (the writers print sets from its lazily fetched host copy) against those of the container table."""
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import FlatEstimates, HarnessTable
    from rpvg_amd.table_text import HAPLOTYPE, JOINT, HarnessTableText
    clusters = small_cases.make_batch_clusters(9311, n_clusters=80, max_reads=60, with_empty=True)
    assert any(not cl["rows"] for cl in clusters) and sum(1 for cl in clusters if cl["rows"]) >= 64   # more than one lane takes part
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params()
    prepared = engine.prepare(batch)
    try:
        resident = res.run_resident(engine, "haplotype-transcripts", params, prepared)
        assert resident is not None
        try:
            got = resident.get()
            estimates, _ = engine.run("haplotype-transcripts", params, prepared)
            want = FlatEstimates.from_estimates(batch, estimates)
            for name, _ in want._FIELDS:
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
            assert len(want.posteriors) > 100
            ours, theirs = resident.table(engine, prepared, params.ploidy), HarnessTable(engine, prepared, params.ploidy)
            try:
                _tables_equal(ours.view(), theirs.view())
                denominator = theirs.view()["total_transcript_count"]
                ours.tpm(denominator)
                theirs.tpm(denominator)
                _tables_equal(ours.view(), theirs.view())
                for writer, suffix in (("haplotype", ".txt"), ("joint", "_joint.txt")):
                    ours.write(writer, str(tmp_path / "resident"), params.prob_precision)
                    theirs.write(writer, str(tmp_path / "containers"), params.prob_precision)
                    written = open(str(tmp_path / "resident") + suffix, "rb").read()
                    assert written == open(str(tmp_path / "containers") + suffix, "rb").read() and len(written) > 1000, writer
                for kind in (HAPLOTYPE, JOINT):   # the two files of a haplotype-transcripts result
                    a = HarnessTableText(engine, ours, kind=kind, ploidy=params.ploidy, min_posterior=params.prob_precision)
                    b = HarnessTableText(engine, theirs, kind=kind, ploidy=params.ploidy, min_posterior=params.prob_precision)
                    try:
                        va, vb = a.view(), b.view()
                        assert va["bytes"] == vb["bytes"] and va["row_off"].tobytes() == vb["row_off"].tobytes() and va["num_bytes"] > 0
                        za, zb = a.bgzf(), b.bgzf()
                        for name in za:
                            if name.endswith("_seconds"):
                                continue
                            same = za[name].tobytes() == zb[name].tobytes() if isinstance(za[name], np.ndarray) else za[name] == zb[name]
                            assert same, (kind, name)
                    finally:
                        a.free()
                        b.free()
            finally:
                ours.free()
                theirs.free()
        finally:
            resident.free()
    finally:
        prepared.free()


def test_run_resident_is_not_taken_elsewhere_and_leaves_the_engine_alone(engine):
    """-n 10, a ploidy the route does not cover and another model return "not taken"; Engine.run behind them gives what it gave."""
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import FlatEstimates
    clusters = small_cases.make_batch_clusters(9312, n_clusters=6, with_empty=False)
    batch = ClusterBatch.from_clusters(clusters)
    prepared = engine.prepare(batch)
    try:
        before, _ = engine.run("haplotype-transcripts", make_params(), prepared)
        want = FlatEstimates.from_estimates(batch, before)
        assert res.run_resident(engine, "haplotype-transcripts", make_params(num_gibbs_samples=10), prepared) is None
        assert res.run_resident(engine, "haplotype-transcripts", make_params(ploidy=3), prepared) is None
        assert res.run_resident(engine, "transcripts", make_params(), prepared) is None
        after, _ = engine.run("haplotype-transcripts", make_params(), prepared)
        got = FlatEstimates.from_estimates(batch, after)
        for name, _ in want._FIELDS:
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
        resident = res.run_resident(engine, "haplotype-transcripts", make_params(), prepared)   # few clusters: one lane
        assert resident is not None
        try:
            flat = resident.get()
            for name, _ in want._FIELDS:
                assert getattr(flat, name).tobytes() == getattr(want, name).tobytes(), name
        finally:
            resident.free()
    finally:
        prepared.free()


def test_run_resident_at_ploidy_5(engine):
    """The polyploid collapsed route (rpvg_hip_nested_full_subset_em with its block kept) against Engine.run on the same batch, the
    table included."""
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import FlatEstimates, HarnessTable
    from tests.test_hip_nested_full import _recombinant_clusters
    from tests.test_hip_polyploid import _small_clusters
    clusters = _small_clusters(9505, 5, max_paths=10) + _recombinant_clusters()
    clusters.insert(2, dict(paths=clusters[0]["paths"], rows=[]))   # a cluster without rows
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=5)
    prepared = engine.prepare(batch)
    try:
        resident = res.run_resident(engine, "haplotype-transcripts", params, prepared)
        assert resident is not None
        try:
            got = resident.get()
            estimates, _ = engine.run("haplotype-transcripts", params, prepared)
            want = FlatEstimates.from_estimates(batch, estimates)
            for name, _ in want._FIELDS:
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
            assert int(np.diff(want.member_off).max()) > 2 and want.set_off[2] == want.set_off[3]
            ours, theirs = resident.table(engine, prepared, params.ploidy), HarnessTable(engine, prepared, params.ploidy)
            try:
                _tables_equal(ours.view(), theirs.view())
            finally:
                ours.free()
                theirs.free()
        finally:
            resident.free()
    finally:
        prepared.free()
