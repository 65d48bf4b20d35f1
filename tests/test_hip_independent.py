"""Independent haplotype inference in one device call: rpvg_hip_nested_independent_subset_em (rpvg_amd/csrc/subset_independent.hip) —
posteriors, distributions, draws, path subsets, EM and the posterior-weighted merge with the cluster as the unit — against the
plain-Python model of tests/independent_model.py fed with the device's own posteriors (rpvg_hip_bounded_pair_posteriors at group
size 2, rpvg_hip_group_full_posteriors otherwise), bit for bit; and through the estimator at ploidy 2, 5 and 8 against the separate
route (RPVG_HIP_NO_DEVICE_SUBSETS=1), bit for bit with the generators, and against the oracle."""
import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import ClusterBatch, make_params
from tests import independent_model as model, small_cases
from tests.test_hip_models import _compare
from tests.test_hip_polyploid import _bits, _small_clusters

pytestmark = pytest.mark.gpu

PRECISION = 1e-8
DEFAULT = 1e-3


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _path(gid, length=100.0, count=1):
    return dict(group_id=gid, source_ids=list(range(count)), source_count=count, effective_length=length)


def _transcripts(cluster):
    """findPathGroups: the paths of every transcript ascending, transcripts in the order their first path appears."""
    order, by_gid = [], {}
    for p, path in enumerate(cluster["paths"]):
        if path["group_id"] not in by_gid:
            by_gid[path["group_id"]] = []
            order.append(path["group_id"])
        by_gid[path["group_id"]].append(p)
    return [by_gid[g] for g in order]


class _Case:
    """Clusters on the device, one matrix per transcript with one column per path; the call's view per (group size, min_hap_prob,
    seed) next to the model fed with the device's own posteriors."""

    def __init__(self, ctx, clusters):
        self.ctx, self.clusters = ctx, clusters
        self.batch = ClusterBatch.from_clusters(clusters)
        self.dev = ctx.upload(self.batch)
        # the units of the call: the clusters that have reads (a cluster without any has no matrix: rpvg_hip_groups_build refuses it,
        # and the estimators never get there, src/path_abundance_estimator.cpp:20-22)
        self.units = [c for c, cl in enumerate(clusters) if cl["rows"]]
        self.transcripts = [_transcripts(clusters[c]) for c in self.units]
        self.matrix_off = np.concatenate([[0], np.cumsum([len(t) for t in self.transcripts])]).astype(np.uint32)
        self.mat_cluster = [c for c, t in zip(self.units, self.transcripts) for _ in t]
        self.mat_paths = [paths for t in self.transcripts for paths in t]
        self.counts = [[clusters[c]["paths"][p]["source_count"] for p in paths] for c, t in zip(self.units, self.transcripts) for paths in t]
        self.log_freq = [np_oracle.log_freqs(c) for c in self.counts]
        self.gid = [[p["group_id"] for p in clusters[c]["paths"]] for c in self.units]
        self.total = [float(sum(r[0] for r in clusters[c]["rows"])) for c in self.units]
        self.dg = ctx.groups(self.dev, self.mat_cluster, [[[p] for p in paths] for paths in self.mat_paths], True, collapse_precision=PRECISION)
        self.posteriors = {}

    def generators(self, seed):
        return [model.Mt19937(seed + k) for k in range(len(self.units))]

    def call(self, g, min_hap_prob=DEFAULT, seed=7, keep_draws=True, dg=None, matrix_off=None):
        words = [rng.next_words() for rng in self.generators(seed)]
        flat = [c for counts in self.counts for c in counts]
        return (dg or self.dg).nested_independent_subset_em(self.matrix_off if matrix_off is None else matrix_off, g, min_hap_prob, words,
                                                            column_counts=flat if g == 2 else None, log_freq=self.log_freq if g != 2 else None,
                                                            collapse_precision=PRECISION, keep_draws=keep_draws)

    def sets(self, g, min_hap_prob):
        """Per matrix (member tuples, posteriors) as the device computes them."""
        key = (g, min_hap_prob if g == 2 else None)
        if key not in self.posteriors:
            if g == 2:
                flat = [c for counts in self.counts for c in counts]
                self.posteriors[key] = [([tuple(sorted(pair)) for pair in pairs], [float(x) for x in post])
                                        for pairs, post in self.dg.bounded_pair_posteriors(flat, min_hap_prob)]
            else:
                post = self.dg.full_posteriors(list(range(len(self.mat_paths))), g, self.log_freq, [len(p) for p in self.mat_paths])
                self.posteriors[key] = [(model.all_sets(len(paths), g), [float(x) for x in p]) for paths, p in zip(self.mat_paths, post)]
        return self.posteriors[key]

    def modelled(self, g, min_hap_prob=DEFAULT, seed=7):
        """Per cluster (draws, subsets, words consumed, generator)."""
        sets, out = self.sets(g, min_hap_prob), []
        for k, rng in enumerate(self.generators(seed)):
            m0, m1 = int(self.matrix_off[k]), int(self.matrix_off[k + 1])
            draws, subsets = model.cluster([(self.mat_paths[m], sets[m][0], sets[m][1]) for m in range(m0, m1)], min_hap_prob, rng)
            out.append((draws, subsets, rng.taken, rng))
        return out

    def free(self):
        self.dg.free()
        self.dev.free()


def _check(case, g, min_hap_prob=DEFAULT, seed=7):
    """Draws, subsets, counts, weights, words, generator states, merged sets and noise against the model, bit for bit."""
    v, want = case.call(g, min_hap_prob, seed), case.modelled(g, min_hap_prob, seed)
    S = model.num_samples(min_hap_prob)
    assert v["num_samples"] == S and v["group_size"] == g and v["num_clusters"] == len(case.units)
    for k, (draws, subsets, taken, rng) in enumerate(want):
        T = len(case.transcripts[k])
        assert v["draws"][k].tolist() == draws, (k, g)
        assert int(v["words_consumed"][k]) == taken
        if taken >= 624:
            assert v["generator_state"][k].tolist() == rng.state_before_next(), k
        s0, s1 = int(v["subset_off"][k]), int(v["subset_off"][k + 1])
        assert s1 - s0 == len(subsets), (k, s1 - s0, len(subsets))
        got_subs, solutions = [], []
        for i, (paths, w, count) in enumerate(subsets):
            s = s0 + i
            got = [int(x) for x in v["path"][int(v["path_off"][s]):int(v["path_off"][s + 1])]]
            cols = [int(x) for x in v["col_path"][int(v["col_off"][s]):int(v["col_off"][s + 1])]]
            assert got == paths and len(paths) == T * g and cols == sorted(set(paths))
            assert float(v["weight"][s]) == w and int(v["sample_count"][s]) == count
            assert float(v["total_count"][s]) == case.total[k]
            got_subs.append((got, w))
            solutions.append((cols, v["abundances"][int(v["col_off"][s]):int(v["col_off"][s + 1])], float(v["noise_count"][s])))
        assert sum(c for _, _, c in subsets) == S
        merged, noise = model.merge(got_subs, solutions, case.gid[k], case.total[k])
        assert int(v["set_count"][k]) == len(merged)
        assert float(v["cluster_noise_count"][k]) == noise
        q0 = int(v["path_off"][s0])
        for q, (key, posterior, abundances) in enumerate(merged):
            size = int(v["set_size"][q0 + q])
            assert size == len(key) == g and tuple(int(x) for x in v["set_member"][q0 + q][:size]) == key
            assert float(v["set_posterior"][q0 + q]) == posterior
            assert [float(x) for x in v["set_abundance"][q0 + q][:size]] == abundances
    return v, want


@pytest.fixture(scope="module")
def cases(hip_ctx):
    made = {}

    def get(name, make):
        if name not in made:
            made[name] = _Case(hip_ctx, make())
        return made[name]

    yield get
    for case in made.values():
        case.free()


def _single_path():
    return [dict(paths=[_path(0)], rows=[small_cases.finish_row(3, 0.01, {0: 0.004}), small_cases.finish_row(2, 0.1, {0: 0.002})])]


def test_single_path_draws_nothing(cases):
    case = cases("single", _single_path)
    v, _ = _check(case, 2)
    assert int(v["words_consumed"][0]) == 0 and not v["generator_state"][0].any()
    assert int(v["subset_off"][1]) == 1 and int(v["sample_count"][0]) == 1000
    assert float(v["weight"][0]) == 1.0000000000000007          # a thousand additions of 0.001
    assert v["path"].tolist() == [0, 0] and v["col_path"].tolist() == [0]
    noise = float(v["noise_count"][0]) * float(v["weight"][0]) + (1 - float(v["weight"][0])) * 5.0
    assert 1 - float(v["weight"][0]) < 0 and float(v["cluster_noise_count"][0]) == noise   # the negative hair, unclamped
    assert int(v["set_count"][0]) == 1 and v["set_member"][0].tolist() == [0, 0]


def _rows(rng, paths_of_transcripts, n):
    rows = []
    for _ in range(n):
        paths = paths_of_transcripts[int(rng.integers(len(paths_of_transcripts)))]
        lik = {int(p): float(rng.uniform(0.001, 0.004)) for p in paths if rng.random() < 0.8}
        rows.append(small_cases.finish_row(int(rng.integers(1, 4)), float(rng.choice([1e-3, 0.1])), lik) if lik else (1, 1.0, []))
    return small_cases.sort_and_merge(rows)


def _interleaved():
    rng = np.random.default_rng(9701)
    return [dict(paths=[_path(0, 100.0), _path(1, 150.0), _path(0, 120.0), _path(1, 90.0)], rows=_rows(rng, [[0, 2], [1, 3]], 30))]


def test_interleaved_transcripts_sort_and_order(cases):
    case = cases("interleaved", _interleaved)
    assert case.transcripts == [[[0, 2], [1, 3]]]
    v, want = _check(case, 2)
    lists = [v["path"][int(v["path_off"][s]):int(v["path_off"][s + 1])].tolist() for s in range(int(v["subset_off"][1]))]
    assert len(lists) > 1 and lists == sorted(lists) and all(l == sorted(l) for l in lists)
    assert any(any(p in (1, 3) for p in l[:3]) and any(p in (0, 2) for p in l[1:]) for l in lists)   # the two transcripts' paths interleave


def _quiet_then_drawing():
    rng = np.random.default_rng(9702)
    return [dict(paths=[_path(0), _path(1, 150.0), _path(1, 120.0)], rows=_rows(rng, [[0], [1, 2]], 20))]


def test_a_transcript_that_draws_nothing_takes_no_words(cases):
    case = cases("quiet", _quiet_then_drawing)
    v, want = _check(case, 2)
    assert int(v["words_consumed"][0]) == 2 * 1000 * 1
    assert not v["draws"][0][:, 0].any() and v["draws"][0][:, 1].any()
    # the second transcript starts at word 0: its draws are those of a cluster that holds it alone
    rng = case.generators(7)[0]
    sets = case.sets(2, DEFAULT)
    assert v["draws"][0][:, 1].tolist() == model.draw_sets(sets[1][1], 1000, rng)


def _block_clusters():
    """One and three transcripts of three paths that every read fits equally well: the three heterozygous pairs tie for the best
    likelihood, so each transcript keeps at least two pairs — and draws — even at min_hap_prob 0.5."""
    one = dict(paths=[_path(0), _path(0), _path(0)], rows=[small_cases.finish_row(2, 0.01, {0: 0.004, 1: 0.004, 2: 0.004})])
    three = dict(paths=[_path(0), _path(1), _path(0), _path(2), _path(1), _path(2), _path(0), _path(1), _path(2)],
                 rows=small_cases.sort_and_merge([small_cases.finish_row(2, 0.01, {0: 0.004, 2: 0.004, 6: 0.004}),
                                                  small_cases.finish_row(3, 0.01, {1: 0.004, 4: 0.004, 7: 0.004}),
                                                  small_cases.finish_row(4, 0.01, {3: 0.004, 5: 0.004, 8: 0.004})]))
    return [one, three]


@pytest.mark.parametrize("min_hap_prob", [0.5, 1 / 312, 1 / 313])
def test_words_and_states_around_a_block(cases, min_hap_prob):
    """S = 2, exactly one block of 624 words per drawing transcript, and one draw into the next block; one and three drawing transcripts."""
    case = cases("blocks", _block_clusters)
    v, want = _check(case, 2, min_hap_prob, seed=31)
    S = model.num_samples(min_hap_prob)
    assert [int(x) for x in v["words_consumed"]] == [2 * S, 6 * S]
    assert S in (2, 312, 313)


def _late_losers():
    """A transcript of three paths: half of the reads fit path 0 alone, the other half paths 1 and 2.  The search keeps {1, 1} and
    {1, 2} before the running maximum passes them by more than min_hap_prob (the numpy oracle keeps (1,1) (1,2) (1,0) (2,0) with
    posteriors 0 0 0.5996 0.4004): the late losers stay listed with posterior 0 and are weights of the distribution."""
    rows = [small_cases.finish_row(20, 1e-4, {0: 0.004}), small_cases.finish_row(20, 1e-4, {1: 0.004, 2: 0.0039}),
            small_cases.finish_row(2, 1e-4, {2: 0.004, 1: 0.0038})]
    return [dict(paths=[_path(0, 100.0, 3), _path(0, 100.0, 2), _path(0, 100.0, 2)], rows=small_cases.sort_and_merge(rows))]


def test_kept_pairs_with_posterior_zero(cases):
    case = cases("late", _late_losers)
    v, want = _check(case, 2)
    members, post = case.sets(2, DEFAULT)[0]
    assert len(post) == 4 and post[0] == 0.0 and post[1] == 0.0 and post[2] > 0 and post[3] > 0
    drawn = set(int(x) for x in v["draws"][0][:, 0])
    assert drawn == {2, 3}                     # a set of posterior 0 is never drawn, and the zeros in front shift no index
    assert int(v["words_consumed"][0]) == 2000


def _forty_flat():
    paths, rows = [], []
    for t in range(40):
        paths += [_path(t, 100.0), _path(t, 100.0)]
        rows.append(small_cases.finish_row(2, 0.01, {2 * t: 0.004, 2 * t + 1: 0.004}))
    return [dict(paths=paths, rows=small_cases.sort_and_merge(rows))]


def test_forty_flat_transcripts_give_distinct_samples(cases):
    case = cases("flat", _forty_flat)
    v, want = _check(case, 2)
    assert int(v["subset_off"][1]) > 512
    assert int(v["words_consumed"][0]) == 2 * 1000 * 40


def _mixed():
    return small_cases.make_batch_clusters(9704, n_clusters=8)   # ... and the two empty ones behind them: ten


@pytest.mark.parametrize("g", [1, 2, 3, 4, 5, 6, 7, 8])
def test_mixed_clusters_equal_the_model(cases, g):
    case = cases("mixed", _mixed)
    assert len(case.clusters) == 10 and len(case.units) == 9   # (the read-less cluster is no unit; the all-noise one is)
    v, want = _check(case, g, seed=100 + g)
    assert int(v["subset_off"][-1]) >= 9 and int(v["words_consumed"].sum()) > 624


def test_two_runs_give_the_same_bytes(cases):
    case = cases("mixed", _mixed)
    for g in (2, 6):
        a, b = case.call(g, seed=5), case.call(g, seed=5)
        for name in a:
            if isinstance(a[name], np.ndarray):
                used = int(a["path_off"][-1]) if name in ("set_size", "set_member", "set_posterior", "set_abundance") else None
                x, y = (r[name] for r in (a, b))
                if used is not None:   # (the set slots of a cluster end at its set_count: compare what is used)
                    for k in range(a["num_clusters"]):
                        q, n = int(a["path_off"][int(a["subset_off"][k])]), int(a["set_count"][k])
                        assert x[q:q + n].tobytes() == y[q:q + n].tobytes(), name
                else:
                    assert x.tobytes() == y.tobytes(), name
        assert all(np.array_equal(p, q) for p, q in zip(a["draws"], b["draws"]))


def test_refusals_leave_the_context_usable(cases, hip_ctx, monkeypatch):
    case = cases("mixed", _mixed)
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
    before = case.call(2, seed=5, keep_draws=False)
    calls = hip_ctx.independent_stats()["calls_completed"]
    for g in (0, 9):
        with pytest.raises(hip.EngineError, match=r"\(-5\).*group size"):
            case.call(g)
    for p in (1 / 2000, 1.5):
        with pytest.raises(hip.EngineError, match=r"\(-5\).*min_hap_prob"):
            case.call(2, p)
    monkeypatch.setenv("RPVG_HIP_NO_DEVICE_SUBSETS", "1")
    with pytest.raises(hip.EngineError, match=r"\(-5\).*RPVG_HIP_NO_DEVICE_SUBSETS"):
        case.call(2)
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS")
    # a transcript with more than 65 536 sets: twelve paths at group size 8 have 75 582
    wide = _Case(hip_ctx, [dict(paths=[_path(0) for _ in range(12)], rows=[small_cases.finish_row(1, 0.01, {0: 0.004, 5: 0.002})])])
    with pytest.raises(hip.EngineError, match=r"\(-5\).*65536 sets"):
        wide.call(8)
    assert int(wide.call(7)["subset_off"][-1]) >= 1      # 31 824 sets: taken
    wide.free()
    # a cluster too wide for LDS-resident EM vectors
    many = _Case(hip_ctx, [dict(paths=[_path(0) for _ in range(4000)], rows=[small_cases.finish_row(1, 0.01, {0: 0.004, 3999: 0.002})])])
    with pytest.raises(hip.EngineError, match=r"\(-5\).*too wide"):
        many.call(1)
    many.free()
    # a batch uploaded without the transcripts of its paths
    bare = ClusterBatch.from_clusters(case.clusters)
    as_c = bare.as_c

    def without_group_ids(*args, **kwargs):
        c = as_c(*args, **kwargs)
        c.path_group_id = None
        return c

    bare.as_c = without_group_ids
    dev = hip_ctx.upload(bare)
    dg = hip_ctx.groups(dev, case.mat_cluster, [[[p] for p in paths] for paths in case.mat_paths], True, collapse_precision=PRECISION)
    with pytest.raises(hip.EngineError, match=r"\(-5\).*path_group_id"):
        case.call(2, dg=dg)
    dg.free()
    dev.free()
    # the matrices of one unit on two clusters; a unit whose columns miss a path of its cluster
    off = case.matrix_off.copy()
    off[1] = off[2]
    if off[0] < off[1] and case.mat_cluster[int(off[0])] != case.mat_cluster[int(off[1]) - 1]:
        with pytest.raises(hip.EngineError, match=r"\(-3\).*not of one cluster"):
            case.call(2, matrix_off=off)
    short = [[[p] for p in paths] for paths in case.mat_paths]
    dropped = next(m for m, cols in enumerate(short) if len(cols) > 1)
    short[dropped] = short[dropped][:-1]
    dg = hip_ctx.groups(case.dev, case.mat_cluster, short, True, collapse_precision=PRECISION)
    counts = case.counts
    case.counts = [c[:-1] if m == dropped else c for m, c in enumerate(counts)]
    try:
        with pytest.raises(hip.EngineError, match=r"\(-3\).*do not partition"):
            case.call(2, dg=dg)
    finally:
        case.counts = counts
        dg.free()
    # nothing counted, and the context serves the next call with the same bytes
    assert hip_ctx.independent_stats()["calls_completed"] == calls + 1   # (wide.call(7))
    after = case.call(2, seed=5, keep_draws=False)
    for name in ("weight", "path", "col_path", "abundances", "sample_count", "words_consumed", "generator_state", "cluster_noise_count"):
        assert before[name].tobytes() == after[name].tobytes(), name


# ---- through the estimator ------------------------------------------------------------------------------------------------

def _estimator_batch(ploidy):
    if ploidy == 2:
        return ClusterBatch.from_clusters(small_cases.make_batch_clusters(681, n_clusters=10))
    return ClusterBatch.from_clusters(_small_clusters(9800 + ploidy, 5, max_paths=8))


def _same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.path_group_sets == y.path_group_sets, k
        assert np.asarray(x.posteriors).tobytes() == np.asarray(y.posteriors).tobytes(), k
        assert np.asarray(x.abundances).tobytes() == np.asarray(y.abundances).tobytes(), k
        assert x.noise_count == y.noise_count and x.total_count == y.total_count, k
        assert list(x.em_iters) == list(y.em_iters) and x.em_cols == y.em_cols, k


@pytest.mark.parametrize("ploidy", [2, 5, 8])
def test_estimator_routes_agree_bit_for_bit(engine, monkeypatch, ploidy):
    batch = _estimator_batch(ploidy)
    params = make_params(ploidy=ploidy, ind_hap_inference=1, rng_seed=7)
    K = batch.num_clusters
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
    engine.reset_stats()
    got, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    stats = engine.independent_stats()
    assert stats["calls_completed"] > 0 and stats["subsets"] > 0
    next_device = engine.generators_after("haplotype-transcripts", params, engine.prepare(batch), K)
    single, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch, per_cluster=True))
    team, _ = engine.run_team("haplotype-transcripts", params, engine.prepare(batch, per_cluster=True), 4)
    monkeypatch.setenv("RPVG_HIP_NO_DEVICE_SUBSETS", "1")
    engine.reset_stats()
    separate, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert engine.independent_stats() == {"calls_completed": 0, "draws": 0, "subsets": 0}
    next_separate = engine.generators_after("haplotype-transcripts", params, engine.prepare(batch), K)
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS")
    _same_bits(got, separate)
    _same_bits(single, separate)
    _same_bits(team, separate)
    assert next_device == next_separate
    again, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert _bits(got) == _bits(again)
    if ploidy == 2:
        ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 1)
        _compare(got, ref)


def test_other_settings_stay_on_their_routes(engine, monkeypatch):
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
    batch = ClusterBatch.from_clusters(_small_clusters(9803, 4, max_paths=6))
    for params in (make_params(ploidy=3, ind_hap_inference=1, rng_seed=7), make_params(ind_hap_inference=1, use_hap_gibbs=1, rng_seed=7)):
        engine.reset_stats()
        engine.run("haplotype-transcripts", params, engine.prepare(batch))
        assert engine.independent_stats()["calls_completed"] == 0
