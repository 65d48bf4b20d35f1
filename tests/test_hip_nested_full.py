"""The polyploid one-call route on the GPU: rpvg_hip_nested_full_subset_em (rpvg_amd/csrc/subset_full.hip) — full enumeration,
retained sets, path subsets, EM and the posterior-weighted merge for group sizes 1 and 3 .. 8 — against the enumeration's own
posteriors (rpvg_hip_group_full_posteriors), the plain-Python model of tests/nested_full_model.py bit for bit, rpvg_hip_em_solve,
and through the estimator at ploidy 5, 6 and 8 against the separate-calls route (RPVG_HIP_NO_DEVICE_SUBSETS=1) and the oracle."""
import itertools
import math

import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import ClusterBatch, make_params
from tests import fuzz_parity, nested_full_model as model, small_cases
from tests.test_hip_polyploid import _bits, _small_clusters

pytestmark = pytest.mark.gpu

MIN_HAP_PROB = 1e-3
PRECISION = 1e-8
RECOMBINANT_SEEDS = (9401, 9402, 9404, 9405)   # two transcripts x two HSTs over eight haplotypes: four haplotype columns each
GROUP_SIZES = (1, 3, 4, 5, 6, 8)


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _recombinant_clusters():
    return [small_cases.make_cluster(np.random.default_rng(seed), 2, (2, 2), n_haps=8, n_reads=6, empty_read_frac=0.0) for seed in RECOMBINANT_SEEDS]


def _abi_clusters():
    """The four recombinant clusters, a one-column matrix and a one-row matrix (as test_hip_polyploid._abi_matrices)."""
    rng = np.random.default_rng(7101)
    return _recombinant_clusters() + [
        small_cases.make_cluster(rng, 1, [1], n_haps=1, n_reads=40),
        dict(paths=[dict(group_id=0, source_ids=[0], source_count=1, effective_length=100.0),
                    dict(group_id=0, source_ids=[1], source_count=1, effective_length=150.0),
                    dict(group_id=0, source_ids=[2], source_count=1, effective_length=120.0)],
             rows=[small_cases.finish_row(3, 0.01, {0: 0.004, 1: 0.002, 2: 0.0035})])]


class _Case:
    """Clusters on the device with their haplotype-column matrices, and per group size the call's view next to the posteriors of
    rpvg_hip_group_full_posteriors on the same matrices (computed once, shared by the tests)."""

    def __init__(self, ctx, clusters, min_hap_prob=MIN_HAP_PROB):
        self.ctx, self.clusters, self.min_hap_prob = ctx, clusters, min_hap_prob
        self.batch = ClusterBatch.from_clusters(clusters)
        self.dev = ctx.upload(self.batch)
        sg = [np_oracle.source_groups(cl["paths"]) for cl in clusters]
        self.columns = [g for g, _ in sg]
        self.log_freq = [np_oracle.log_freqs(mult) for _, mult in sg]
        self.gid = [[p["group_id"] for p in cl["paths"]] for cl in clusters]
        self.dg = ctx.groups(self.dev, list(range(len(clusters))), self.columns, True, collapse_precision=PRECISION)
        self.views, self.posteriors = {}, {}

    def view(self, g):
        if g not in self.views:
            self.views[g] = self.dg.nested_full_subset_em(g, self.log_freq, self.min_hap_prob, collapse_precision=PRECISION)
        return self.views[g]

    def full(self, g):
        if g not in self.posteriors:
            self.posteriors[g] = self.dg.full_posteriors(list(range(len(self.clusters))), g, self.log_freq, [len(c) for c in self.columns])
        return self.posteriors[g]

    def free(self):
        self.dg.free()
        self.dev.free()


class _Cases:
    def __init__(self, ctx):
        self.ctx, self.made = ctx, {}

    def get(self, name, make):
        if name not in self.made:
            self.made[name] = _Case(self.ctx, make())
        return self.made[name]


@pytest.fixture(scope="module")
def cases(hip_ctx):
    """The shared cases of the module; freed before the session's context goes."""
    c = _Cases(hip_ctx)
    yield c
    for case in c.made.values():
        case.free()


def _check_retained(case, g):
    v, post = case.view(g), case.full(g)
    assert v["group_size"] == g and v["num_matrices"] == len(case.clusters)
    for m, p in enumerate(post):
        a, b = int(v["retained_off"][m]), int(v["retained_off"][m + 1])
        want = np.nonzero(p >= case.min_hap_prob)[0]
        assert np.array_equal(v["retained_rank"][a:b], want.astype(np.uint64))
        assert v["retained_posterior"][a:b].tobytes() == p[want].tobytes()
    return v, post


def _check_subsets_and_merge(case, g):
    """subset_off, path, col_path and weight against the model fed with the device's posteriors; set_* and cluster_noise_count against
    the model fed with the call's own weights and EM results.  Returns (retained sets, subsets, largest multiplicity in a key)."""
    v, post = case.view(g), case.full(g)
    retained, n_subsets, top = 0, 0, 0
    for m, p in enumerate(post):
        ranks, kept, total = model.retain(p, case.min_hap_prob)
        subs = model.subsets(ranks, kept, total, case.columns[m], g, case.min_hap_prob)
        s0, s1 = int(v["subset_off"][m]), int(v["subset_off"][m + 1])
        assert s1 - s0 == len(subs)
        retained += len(ranks)
        n_subsets += len(subs)
        got_subs, solutions = [], []
        for i, (paths, w) in enumerate(subs):
            s = s0 + i
            got_paths = [int(x) for x in v["path"][int(v["path_off"][s]):int(v["path_off"][s + 1])]]
            cols = [int(x) for x in v["col_path"][int(v["col_off"][s]):int(v["col_off"][s + 1])]]
            assert got_paths == paths and cols == sorted(set(paths))
            assert float(v["weight"][s]) == w, (m, i, float(v["weight"][s]), w)
            got_subs.append((got_paths, float(v["weight"][s])))
            solutions.append((cols, v["abundances"][int(v["col_off"][s]):int(v["col_off"][s + 1])], float(v["noise_count"][s])))
            assert float(v["total_count"][s]) == float(sum(r[0] for r in case.clusters[m]["rows"]))
        merged, noise = model.merge(got_subs, solutions, case.gid[m], float(sum(r[0] for r in case.clusters[m]["rows"])))
        assert int(v["set_count"][m]) == (len(merged) if subs else 0)
        if not subs:
            continue
        assert float(v["cluster_noise_count"][m]) == noise
        q0 = int(v["path_off"][s0])
        for q, (key, posterior, abundances) in enumerate(merged):
            size = int(v["set_size"][q0 + q])
            assert size == len(key) and tuple(int(x) for x in v["set_member"][q0 + q][:size]) == key
            assert all(int(x) == 0xFFFFFFFF for x in v["set_member"][q0 + q][size:])
            assert float(v["set_posterior"][q0 + q]) == posterior
            assert [float(x) for x in v["set_abundance"][q0 + q][:size]] == abundances
            assert all(float(x) == 0.0 for x in v["set_abundance"][q0 + q][size:])
            top = max(top, max(key.count(p) for p in key))
    return retained, n_subsets, top


@pytest.mark.parametrize("g", GROUP_SIZES)
def test_retained_sets_are_the_enumerations(cases, g):
    case = cases.get("abi", _abi_clusters)
    v, post = _check_retained(case, g)
    for m, p in enumerate(post):
        G = len(case.columns[m])
        sets = list(itertools.combinations_with_replacement(range(G), g))
        assert len(p) == len(sets) == math.comb(G + g - 1, g)
        a, b = int(v["retained_off"][m]), int(v["retained_off"][m + 1])
        assert [model.members_of_rank(G, g, int(r)) for r in v["retained_rank"][a:b]] == [sets[int(r)] for r in v["retained_rank"][a:b]]
    assert int(v["retained_off"][-1]) > 0


@pytest.mark.parametrize("g", GROUP_SIZES)
def test_subsets_weights_and_merge_equal_the_model(cases, g):
    case = cases.get("abi", _abi_clusters)
    retained, n_subsets, top = _check_subsets_and_merge(case, g)
    assert n_subsets > 0
    if g in (3, 4, 6):
        assert retained > n_subsets   # some matrix merges two retained sets into one subset
    if g >= 3:
        assert top >= 3               # a key holds a path three times or more: the division by the multiplicity is not exact


@pytest.mark.parametrize("g", GROUP_SIZES)
def test_em_results_are_those_of_em_solve(cases, g):
    hip_ctx = cases.ctx
    case = cases.get("abi", _abi_clusters)
    v = case.view(g)
    S = int(v["subset_off"][-1])
    clusters = [m for m in range(len(case.clusters)) for _ in range(int(v["subset_off"][m + 1] - v["subset_off"][m]))]
    cols = [[int(x) for x in v["col_path"][int(v["col_off"][s]):int(v["col_off"][s + 1])]] for s in range(S)]
    abund, noise, total, iters = hip_ctx.em_solve(case.dev, clusters, cols, collapse_precision=PRECISION)
    assert [int(x) for x in iters] == [int(x) for x in v["iterations"]]
    assert small_cases.rel_close(noise, v["noise_count"], rel=1e-12, floor=1e-300)
    assert np.array_equal(total, v["total_count"])
    for s in range(S):
        assert small_cases.rel_close(abund[s], v["abundances"][int(v["col_off"][s]):int(v["col_off"][s + 1])], rel=1e-12, floor=1e-300)


def _many_cluster():
    return [small_cases.make_cluster(np.random.default_rng(9410), 1, (36,), n_haps=36, n_reads=2, empty_read_frac=0.0)]


def _empty_cluster():
    return [small_cases.make_cluster(np.random.default_rng(9420), 1, (36,), n_haps=36, n_reads=2, empty_read_frac=1.0)]


def test_many_retained_sets(cases):
    case = cases.get("many", _many_cluster)
    v, post = _check_retained(case, 3)
    assert len(post[0]) == 8436
    retained, n_subsets, _ = _check_subsets_and_merge(case, 3)
    assert retained == int(v["retained_off"][-1]) == 631 and n_subsets == 631


def test_a_threshold_below_the_slots_is_refused(cases):
    case = cases.get("many", _many_cluster)
    with pytest.raises(hip.EngineError, match=r"\(-5\).*min_hap_prob"):
        case.dg.nested_full_subset_em(3, case.log_freq, 1.0 / 2048, collapse_precision=PRECISION)
    again = case.dg.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB, collapse_precision=PRECISION)
    assert again["retained_rank"].tobytes() == case.view(3)["retained_rank"].tobytes()


def test_a_first_call_that_outgrows_its_capacities_is_tried_once_more():
    """A context's first call reserves eight subsets' worth of every cluster's rows; 631 subsets of a two-row cluster do not fit, the call
    learns what it needs from its own header and selects, expands and solves once more from the retained sets it holds (the
    enumeration runs once).  The result is that of a call that fitted, bit for bit; the second attempt shows in the kernels
    behind the enumeration (more build launches than the call after it, which fits, and the same enumeration launches)."""
    ctx = hip.Context(0)
    try:
        case = _Case(ctx, _many_cluster())
        ctx.synchronize()
        before = ctx.stats()
        first = case.dg.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB, collapse_precision=PRECISION)
        middle = ctx.stats()
        second = case.dg.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB, collapse_precision=PRECISION)
        after = ctx.stats()
        assert int(first["subset_off"][-1]) == 631 and after["nested_full_calls"] == 2
        assert middle["build_launches"] - before["build_launches"] > after["build_launches"] - middle["build_launches"]       # two attempts
        assert middle["loglik_launches"] - before["loglik_launches"] == after["loglik_launches"] - middle["loglik_launches"]  # one enumeration
        used = int(first["set_count"][0])
        assert used == int(second["set_count"][0]) > 0
        for name in first:
            if isinstance(first[name], np.ndarray):
                a, b = (x[name][:used] if name in ("set_size", "set_member", "set_posterior", "set_abundance") else x[name] for x in (first, second))
                assert a.tobytes() == b.tobytes(), name
        case.free()
    finally:
        ctx.close()


def test_nothing_retained(cases):
    hip_ctx = cases.ctx
    case = cases.get("empty", _empty_cluster)
    v, post = _check_retained(case, 3)
    assert len(post[0]) == 8436 and int(v["retained_off"][-1]) == 0
    assert int(v["set_count"][0]) == 0 and int(v["subset_off"][-1]) == 0 and len(v["iterations"]) == 0
    # between two ordinary matrices: their results are what they are without it
    ordinary = _recombinant_clusters()[:2]
    both = _Case(hip_ctx, [ordinary[0]] + _empty_cluster() + [ordinary[1]])
    alone = _Case(hip_ctx, ordinary)
    w, a = both.view(3), alone.view(3)
    assert int(w["set_count"][1]) == 0 and int(w["subset_off"][1]) == int(w["subset_off"][2])
    for name in ("weight", "path", "col_path", "abundances", "noise_count", "iterations", "retained_rank", "retained_posterior"):
        assert w[name].tobytes() == a[name].tobytes(), name
    assert [int(x) for x in w["set_count"]] == [int(a["set_count"][0]), 0, int(a["set_count"][1])]
    assert w["cluster_noise_count"][[0, 2]].tobytes() == a["cluster_noise_count"].tobytes()
    for m_w, m_a in ((0, 0), (2, 1)):
        qw, qa, n = int(w["path_off"][int(w["subset_off"][m_w])]), int(a["path_off"][int(a["subset_off"][m_a])]), int(a["set_count"][m_a])
        for name in ("set_size", "set_member", "set_posterior", "set_abundance"):
            assert w[name][qw:qw + n].tobytes() == a[name][qa:qa + n].tobytes(), name


def test_nothing_retained_through_the_estimator(engine):
    batch = ClusterBatch.from_clusters(_empty_cluster())
    engine.reset_stats()
    got, _ = engine.run("haplotype-transcripts", make_params(ploidy=5), engine.prepare(batch))
    stats = engine.stats()
    assert stats["nested_full_calls"] == 1 and stats["nested_full_sets"] == 658008 and stats["nested_full_retained"] == 0
    assert got[0].noise_count == got[0].total_count > 0 and len(got[0].path_group_sets) == 0


def test_chunk_boundary(hip_ctx):
    """Two problems of group size 8 over 33 columns: 76 904 685 sets each, together past the 2^27 sets of a launch.  One call
    against two calls of one problem each, bit for bit; no posterior is downloaded.  (The smallest shape that crosses the cut.)"""
    clusters = [small_cases.make_cluster(np.random.default_rng(9430 + i), 1, (33,), n_haps=33, n_reads=2, empty_read_frac=0.0) for i in range(2)]
    assert all(len(cl["rows"]) <= 2 for cl in clusters)
    both = _Case(hip_ctx, clusters)
    assert [len(c) for c in both.columns] == [33, 33] and math.comb(40, 8) == 76904685 and 2 * 76904685 > 2 ** 27
    hip_ctx.reset_stats()
    w = both.view(8)
    assert hip_ctx.stats()["nested_full_sets"] == 2 * 76904685
    singles = [_Case(hip_ctx, [cl]).view(8) for cl in clusters]
    for name in ("weight", "path", "col_path", "abundances", "noise_count", "iterations", "retained_rank", "retained_posterior", "set_count",
                 "cluster_noise_count"):
        assert w[name].tobytes() == b"".join(s[name].tobytes() for s in singles), name
    for m, s in enumerate(singles):
        q, n = int(w["path_off"][int(w["subset_off"][m])]), int(s["set_count"][0])
        for name in ("set_size", "set_member", "set_posterior", "set_abundance"):
            assert w[name][q:q + n].tobytes() == s[name][:n].tobytes(), name


def _estimator_batch(ploidy):
    return ClusterBatch.from_clusters(_small_clusters(9500 + ploidy, 5, max_paths=10 if ploidy < 8 else 8) + _recombinant_clusters())


@pytest.mark.parametrize("ploidy", [5, 6, 8])
def test_estimator_takes_the_one_call_route(engine, monkeypatch, ploidy):
    batch = _estimator_batch(ploidy)
    params = make_params(ploidy=ploidy)
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
    engine.reset_stats()
    got, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    stats = engine.stats()
    assert stats["nested_full_calls"] > 0 and stats["nested_full_sets"] > 0   # (no posterior download: the sets stayed on the device)
    monkeypatch.setenv("RPVG_HIP_NO_DEVICE_SUBSETS", "1")
    engine.reset_stats()
    separate, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert engine.stats()["nested_full_calls"] == 0
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS")
    for a, b in zip(got, separate):
        assert a.path_group_sets == b.path_group_sets
        assert np.array_equal(a.posteriors, b.posteriors)
        assert list(a.em_iters) == list(b.em_iters) and a.em_cols == b.em_cols and a.total_count == b.total_count
        assert small_cases.rel_close(a.abundances, b.abundances, rel=1e-12, floor=1e-300)
        assert small_cases.rel_close(a.noise_count, b.noise_count, rel=1e-12, floor=1e-300)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 8)
    assert fuzz_parity.compare(got, ref) == []


def test_routes_agree_and_repeat_at_ploidy_6(engine, monkeypatch):
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS", raising=False)
    batch = ClusterBatch.from_clusters(_small_clusters(7601, 10))
    params = make_params(ploidy=6)
    calls = []
    engine.reset_stats()
    whole, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    calls.append(engine.stats()["nested_full_calls"])
    engine.reset_stats()
    single, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch, per_cluster=True))
    calls.append(engine.stats()["nested_full_calls"])
    engine.reset_stats()
    team, _ = engine.run_team("haplotype-transcripts", params, engine.prepare(batch, per_cluster=True), 8)
    calls.append(engine.stats()["nested_full_calls"])
    assert all(c > 0 for c in calls), calls
    for other in (single, team):
        for a, b in zip(whole, other):
            assert a.path_group_sets == b.path_group_sets
            assert small_cases.rel_close(a.posteriors, b.posteriors, rel=1e-12, floor=1e-15)
            assert small_cases.rel_close(a.abundances, b.abundances, rel=1e-12, floor=1e-15)
            assert a.total_count == b.total_count
    again, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert _bits(whole) == _bits(again)


def test_refusals(cases):
    hip_ctx = cases.ctx
    case = cases.get("abi", _abi_clusters)
    for g in (2, 9, 0):
        with pytest.raises(hip.EngineError, match=r"\(-5\).*group size " + str(g)):
            case.dg.nested_full_subset_em(g, case.log_freq, MIN_HAP_PROB)
    # a batch uploaded without the transcripts of its paths
    bare = ClusterBatch.from_clusters(_abi_clusters())
    as_c = bare.as_c

    def without_group_ids(*args, **kwargs):
        c = as_c(*args, **kwargs)
        c.path_group_id = None
        return c

    bare.as_c = without_group_ids
    dev = hip_ctx.upload(bare)
    dg = hip_ctx.groups(dev, list(range(len(case.clusters))), case.columns, True, collapse_precision=PRECISION)
    with pytest.raises(hip.EngineError, match=r"\(-5\).*path_group_id"):
        dg.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB)
    # matrices built on another batch
    other = hip_ctx.upload(ClusterBatch.from_clusters(_abi_clusters()))
    stray = hip.DeviceGroups.__new__(hip.DeviceGroups)
    stray.ctx, stray.batch, stray.handle = hip_ctx, other, case.dg.handle
    try:
        with pytest.raises(hip.EngineError, match=r"\(-3\).*another batch"):
            stray.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB)
    finally:
        stray.handle = None   # (case.dg owns the matrices)
    # the context still serves the next call
    again = case.dg.nested_full_subset_em(3, case.log_freq, MIN_HAP_PROB, collapse_precision=PRECISION)
    assert again["weight"].tobytes() == case.view(3)["weight"].tobytes()
