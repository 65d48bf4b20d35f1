"""Polyploid haplotype inference (ploidy 1 .. 8) on the GPU, against numpy and the CPU oracle.

Full enumeration of every multiset of `ploidy` columns runs on the device from ploidy 5 on (rpvg_hip_group_full_posteriors:
the sets are enumerated from their lexicographic ranks, evaluated and normalised there); --use-hap-gibbs drives the
host sampler with device conditionals up to width 8.  Ploidy 1, 3 and 4 keep the request route
(rpvg_hip_group_loglik), which the new entry point is checked against here."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import engine as eng_mod, hip, io as rio
from rpvg_amd.batch import ClusterBatch, make_params
from tests import fuzz_parity, small_cases
from tests.test_hip_models import _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _small_clusters(seed, n_clusters, max_paths=10, max_reads=300):
    """Clusters of at most max_paths paths (haplotypes: one column per path) and haplotypes (haplotype-transcripts: one
    column per distinct haplotype), small enough for the oracle's full enumeration at ploidy 8."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_clusters):
        T = int(rng.integers(1, 3))
        hst = [int(rng.integers(1, 4)) for _ in range(T)]
        while sum(hst) > max_paths:
            hst[int(np.argmax(hst))] -= 1
        out.append(small_cases.make_cluster(rng, T, hst, n_haps=int(rng.integers(2, 7)), n_reads=int(rng.integers(20, max_reads))))
    return out


def _bits(estimates):
    return [(e.path_group_sets, e.posteriors.tobytes(), np.asarray(e.abundances).tobytes(), e.noise_count, e.total_count) for e in estimates]


# ---- the C ABI ------------------------------------------------------------------------------------------------

def _abi_matrices(hip_ctx, normalise):
    """Device group matrices of a few clusters, a single-column one and a one-row one, and their numpy twins."""
    rng = np.random.default_rng(7101)
    clusters = [small_cases.make_cluster(rng, 2, [3, 2], n_haps=5, n_reads=120),
                small_cases.make_cluster(rng, 1, [4], n_haps=6, n_reads=200),
                small_cases.make_cluster(rng, 1, [1], n_haps=1, n_reads=40),
                dict(paths=[dict(group_id=0, source_ids=[0], source_count=1, effective_length=100.0),
                            dict(group_id=0, source_ids=[1], source_count=1, effective_length=150.0),
                            dict(group_id=0, source_ids=[2], source_count=1, effective_length=120.0)],
                     rows=[small_cases.finish_row(3, 0.01, {0: 0.004, 1: 0.002, 2: 0.0035})])]
    batch = ClusterBatch.from_clusters(clusters)
    dev = hip_ctx.upload(batch)
    groups = [np_oracle.source_groups(cl["paths"])[0] if normalise else [[p] for p in range(len(cl["paths"]))] for cl in clusters]
    dg = hip_ctx.groups(dev, list(range(len(clusters))), groups, normalise)
    twins = []
    for cl, g in zip(clusters, groups):
        M, noise, counts = np_oracle.grouped_matrix(cl["rows"], g)
        if normalise:
            M = np_oracle.add_noise_and_normalize(M, noise)[:, :-1]
        path_counts = [int(x) for x in rng.integers(1, 4, size=len(g))]
        twins.append((M, noise, counts, path_counts))
    return dev, dg, twins


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("g", [1, 3, 4, 5, 6, 8])
def test_full_posteriors_match_numpy(hip_ctx, g, normalise):
    dev, dg, twins = _abi_matrices(hip_ctx, normalise)
    num_cols = [t[0].shape[1] for t in twins]
    assert 1 in num_cols and any(t[0].shape[0] == 1 for t in twins)
    got = dg.full_posteriors(list(range(len(twins))), g, [np_oracle.log_freqs(t[3]) for t in twins], num_cols)
    for (M, noise, counts, path_counts), post in zip(twins, got):
        G = M.shape[1]
        sets, want = np_oracle.posteriors_full(M, noise, counts, path_counts, g)
        assert len(post) == math.comb(G + g - 1, g) == len(sets)
        assert sets == list(itertools.combinations_with_replacement(range(G), g))  # the rank order the ABI promises
        assert small_cases.rel_close(post, want, rel=1e-9, floor=1e-12)
        assert abs(post.sum() - 1.0) < 1e-12
    # the set count of the header's helper
    assert hip.lib().rpvg_hip_full_set_count(40, 6) == math.comb(45, 6)


@pytest.mark.parametrize("g", [3, 4])
def test_full_posteriors_equal_the_request_route(hip_ctx, g):
    """The new entry point against rpvg_hip_group_loglik on host-enumerated members (the route ploidy 3 and 4 keep)."""
    dev, dg, twins = _abi_matrices(hip_ctx, False)
    num_cols = [t[0].shape[1] for t in twins]
    got = dg.full_posteriors(list(range(len(twins))), g, [np_oracle.log_freqs(t[3]) for t in twins], num_cols)
    for m, ((M, noise, counts, path_counts), post) in enumerate(zip(twins, got)):
        sets = list(itertools.combinations_with_replacement(range(M.shape[1]), g))
        ll = dg.loglik([m] * len(sets), [list(s) for s in sets], float(g))
        lf = np_oracle.log_freqs(path_counts)
        logp = []
        lse = np_oracle.LOWEST
        for s, x in zip(sets, ll):
            v = float(x)
            for k in s:
                v += lf[k]
            v += math.log(np_oracle.num_permutations(s))
            logp.append(v)
            lse = np_oracle.add_log(lse, v)
        want_log = np.array(logp) - lse
        keep = post > 1e-300
        scale = max(1.0, float(np.abs(ll).max()))
        assert np.all(np.abs(np.log(post[keep]) - want_log[keep]) <= 1e-12 * scale)


# ---- the estimators against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("ploidy", [5, 6, 8])
def test_haplotypes_full_enumeration_matches_oracle(engine, ploidy):
    clusters = _small_clusters(7200 + ploidy, 6, max_paths=10 if ploidy < 8 else 8)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=ploidy)
    ref, _ = pyoracle.run("haplotypes", params, batch, 8)
    got, _ = engine.run("haplotypes", params, engine.prepare(batch))
    for g, r in zip(got, ref):
        assert g.path_group_sets == r.path_group_sets
    _compare(got, ref)


@pytest.mark.parametrize("ind", [0, 1])
@pytest.mark.parametrize("ploidy", [5, 6, 8])
def test_haplotype_transcripts_match_oracle(engine, ploidy, ind):
    clusters = _small_clusters(7300 + ploidy + 10 * ind, 6)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=ploidy, ind_hap_inference=ind, rng_seed=5)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 8)
    got, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert fuzz_parity.compare(got, ref) == []


@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
@pytest.mark.parametrize("ploidy", [5, 6])
def test_gibbs_polyploid_follows_the_reference_stream(engine, model, ploidy):
    """--use-hap-gibbs at ploidy 5 and 6: chains on the host with the reference's generator, conditionals of width up to 8
    on the device; draw for draw the oracle's sets and counts."""
    clusters = _small_clusters(7400 + ploidy, 5, max_reads=200)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(use_hap_gibbs=1, ploidy=ploidy, rng_seed=13)
    ref, _ = pyoracle.run(model, params, batch, 1)
    got, _ = engine.run(model, params, engine.prepare(batch))
    _compare(got, ref)
    for g, r in zip(got, ref):
        if model == "haplotypes":
            assert g.path_group_sets == r.path_group_sets  # first-seen order of the sampled sets


def test_read_count_samples_at_ploidy_6_conserve_mass_and_repeat(engine):
    clusters = _small_clusters(7501, 6)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=6, num_gibbs_samples=2, rng_seed=3)
    got, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    for g in got:
        if g.total_count > 0 and len(g.abundances):
            assert abs(float(np.sum(g.abundances)) + g.noise_count - g.total_count) <= 1e-9 * g.total_count
    again, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    assert _bits(got) == _bits(again)


@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
def test_routes_agree_at_ploidy_6(engine, model):
    """Batch run, per-cluster estimate() and estimate() from an OpenMP team of 8 (the call combiner)."""
    clusters = _small_clusters(7601, 10)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=6)
    whole, _ = engine.run(model, params, engine.prepare(batch))
    single, _ = engine.run(model, params, engine.prepare(batch, per_cluster=True))
    team, _ = engine.run_team(model, params, engine.prepare(batch, per_cluster=True), 8)
    for other in (single, team):
        for a, b in zip(whole, other):
            assert a.path_group_sets == b.path_group_sets
            assert small_cases.rel_close(a.posteriors, b.posteriors, rel=1e-12, floor=1e-15)
            assert small_cases.rel_close(a.abundances, b.abundances, rel=1e-12, floor=1e-15)
            assert a.total_count == b.total_count


def test_replay_command_line_ploidy_6(tmp_path):
    clusters = _small_clusters(7701, 8)
    batch = ClusterBatch.from_clusters(clusters)
    probs, info = str(tmp_path / "run_probs.txt.gz"), str(tmp_path / "info.tsv.gz")
    rio.write_batch_files(batch, probs, info)
    exe = os.path.join(ROOT, "rpvg_amd", "host", "rpvg_amd_replay")
    prefix = str(tmp_path / "cli")
    out = subprocess.run([exe, "-p", probs, "-f", info, "-i", "haplotypes", "-y", "6", "-o", prefix], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    params = make_params(ploidy=6)
    cpu_prefix = str(tmp_path / "cpu")
    with pyoracle.RawRun("haplotypes", params, rio.read_batch_files(probs, info, parse_haplotype_ids=False), 8) as run:
        rio.write_estimates(probs, info, "haplotypes", params, run.view, cpu_prefix)
    lines = {}
    for name, p in (("gpu", prefix), ("cpu", cpu_prefix)):
        text = open(p + ".txt").read().splitlines()
        assert text[0].split("\t")[:6] == [f"Name_{i}" for i in range(1, 7)]
        lines[name] = (text[0], {tuple(f[:7]): [float(x) for x in f[7:]] for f in (line.split("\t") for line in text[1:])})
    assert lines["gpu"][0] == lines["cpu"][0]
    gpu, cpu = lines["gpu"][1], lines["cpu"][1]
    assert set(gpu) == set(cpu) and len(gpu) > 0
    for key in cpu:
        assert small_cases.rel_close(gpu[key], cpu[key], rel=1e-5, floor=1e-6), (key, gpu[key], cpu[key])


# ---- limits -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
def test_ploidy_above_8_is_an_error_naming_the_limit(engine, model):
    clusters = _small_clusters(7801, 2)
    prep = engine.prepare(ClusterBatch.from_clusters(clusters))
    with pytest.raises(hip.EngineError, match=r"ploidy.*\b9\b.*\b8\b"):
        engine.run(model, make_params(ploidy=9), prep)


def test_ploidy_8_over_the_set_bound_names_the_cluster(engine):
    rng = np.random.default_rng(7802)
    clusters = [small_cases.make_cluster(rng, 1, [3], n_haps=3, n_reads=30),
                small_cases.make_cluster(rng, 1, [200], n_haps=200, n_reads=60)]
    prep = engine.prepare(ClusterBatch.from_clusters(clusters))
    with pytest.raises(hip.EngineError, match=r"cluster 1\b.*--use-hap-gibbs"):
        engine.run("haplotypes", make_params(ploidy=8), prep)


@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
def test_ploidy_6_repeats_to_the_bit(engine, model):
    clusters = _small_clusters(7206, 6)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(ploidy=6)
    first, _ = engine.run(model, params, engine.prepare(batch))
    second, _ = engine.run(model, params, engine.prepare(batch))
    assert _bits(first) == _bits(second)
