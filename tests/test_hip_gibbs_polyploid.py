"""The Gibbs sampler of haplotype sets at ploidy 3 .. 8 on the device (rpvg_hip_group_gibbs_polyploid): draw for draw
against a sequential Python model of the reference's sampler through the C ABI, the estimators against the CPU oracle,
the fallbacks to the host-driven sampler, repeatability, and a cluster that full enumeration refuses.

The device adds the other members of a conditional to a row's noise in ascending column order, the reference in the slot
order of whichever chain misses its memo first: a row's base can differ in its last bit.  The ABI test asserts on its own
inputs that this moves no draw (the model is run both ways); the seeds below pass that precondition."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import ClusterBatch, make_params
from tests import fuzz_parity, small_cases
from tests.test_hip_kernels import _gibbs_model, _mt19937_words, _mt_temper
from tests.test_hip_models import _compare
from tests.test_hip_polyploid import _bits, _small_clusters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _assert_on_the_device(engine):
    """The span of the device sampler was opened (it is opened nowhere else) AND the device calls returned their sets: a call
    that gives up on the way has a span too, and the host-driven sampler behind it would pass the comparisons."""
    stats = engine.stats()
    assert stats["gibbs_ms"] > 0
    assert stats["gibbs_calls_completed"] >= 1


# ---- the C ABI, draw for draw ---------------------------------------------------------------------------------

@pytest.mark.parametrize("group_size", [3, 4, 5, 8])
def test_device_sampler_follows_a_python_model_draw_for_draw(hip_ctx, group_size):
    """The layout of test_device_gibbs_sampler_follows_a_python_model_draw_for_draw (test_hip_kernels.py): several matrices,
    one generator serving two problems, one single-column matrix, generators starting at stream offsets 0, 100, 623, 624,
    1000.  The model takes its conditionals from rpvg_hip_group_conditionals (pinned by item 21 of docs/design/parity.md,
    tests/test_hip_set_loglik.py) and is run twice per problem — the others
    handed over in slot order (the reference) and sorted ascending (the device): both must give the same sets, counts and
    words, or the seed sits on a last-bit tie and is a bad input (none of the committed seeds does)."""
    rng = np.random.default_rng(8100 + group_size)
    shapes_of_clusters = [[5, 4] if group_size < 8 else [4, 4], [3, 3], [4], [6, 2], [2, 1], [5], [3]]  # (at most 8 columns at group size 8)
    clusters = [small_cases.make_cluster(rng, len(hst), hst, n_haps=int(rng.integers(2, 7)), n_reads=int(rng.integers(20, 200)))
                for hst in shapes_of_clusters]
    batch = ClusterBatch.from_clusters(clusters)
    dev = hip_ctx.upload(batch)
    mats = list(range(len(clusters)))
    groups = [[[p] for p in range(len(cl["paths"]))] for cl in clusters]
    groups[-1] = [list(range(len(clusters[-1]["paths"])))]  # one column: every path of the cluster
    num_cols = [len(g) for g in groups]
    assert max(num_cols) >= 8 and num_cols[-1] == 1
    dg = hip_ctx.groups(dev, mats, groups, False)
    rng = np.random.default_rng(5)
    log_freq = [np.log(rng.integers(1, 5, size=G) / 7.0) for G in num_cols]
    generator_problems = [[0], [1, 2], [3], [4], [5], [6]]
    seeds = [(21, 0), (22, 100), (23, 623), (24, 624), (25, 7), (26, 1000)]

    def conditional_of(m, ascending):
        cache = {}

        def conditional(others):
            handed = tuple(sorted(others)) if ascending else tuple(others)
            if handed not in cache:
                got = dg.conditionals([m], [list(handed)], group_size, float(group_size), num_cols)[0]
                cache[handed] = [float(x) + float(y) for x, y in zip(got, log_freq[m])]
            return cache[handed]
        return conditional

    want, want_words, streams, shapes = {}, [], [], {}
    for problems, (seed, skip) in zip(generator_problems, seeds):
        words = _mt19937_words(seed, skip, 400000)
        taken = 0
        for m in problems:
            order, counts, used, shape = _gibbs_model(num_cols[m], group_size, conditional_of(m, True), words[taken:])
            in_slot_order = _gibbs_model(num_cols[m], group_size, conditional_of(m, False), words[taken:])
            assert in_slot_order == (order, counts, used, shape), f"problem {m}: the order of the others moves a draw (a bad seed)"
            want[m] = (order, counts)
            shapes[m] = shape
            taken += used
        assert taken + 624 <= len(words)
        want_words.append(taken)
        streams.append(words)
    got, words_consumed, state, (rounds, conditionals) = dg.gibbs_polyploid(
        mats, group_size, [shapes[m][0] for m in mats], [shapes[m][1] for m in mats], [shapes[m][2] for m in mats], log_freq,
        generator_problems, [s[:624] for s in streams])
    assert [int(w) for w in words_consumed] == want_words
    for m in mats:
        assert got[m][0] == want[m][0], f"sets of problem {m}"
        assert got[m][1] == want[m][1], f"counts of problem {m}"
        assert sum(got[m][1]) == shapes[m][0] * shapes[m][2]
        assert all(len(s) == group_size and list(s) == sorted(s) for s in got[m][0])
    assert got[6][0] == [(0,) * group_size]
    assert rounds >= 1 and conditionals >= sum(1 for G in num_cols if G >= 2)  # (one column: nothing to evaluate)
    for g, taken in enumerate(want_words):
        if taken >= 624:
            assert [_mt_temper(int(x)) for x in state[g]] == streams[g][taken - 624:taken]


def test_device_sampler_reports_what_it_does_not_take(hip_ctx):
    """Group sizes 2 and 9 belong to other routes, a problem with more columns than the packed key holds (256 at group
    size 8: 8 bits per member, all-ones reserved) is 'unsupported' with the bound in the message, a matrix that does not
    exist is an invalid argument and a call without problems is an empty result."""
    paths = [dict(group_id=0, source_ids=[p], source_count=1, effective_length=100.0 + p) for p in range(256)]
    rows = small_cases.sort_and_merge([small_cases.finish_row(2, 0.01, {p: 0.001 * (1 + (p * (r + 3)) % 7) for p in range(r, 256, r + 2)})
                                       for r in range(5)])
    clusters = [dict(paths=paths, rows=rows)] + small_cases.make_batch_clusters(813, n_clusters=1, with_empty=False)
    batch = ClusterBatch.from_clusters(clusters)
    dev = hip_ctx.upload(batch)
    groups = [[[p] for p in range(len(cl["paths"]))] for cl in clusters]
    dg = hip_ctx.groups(dev, [0, 1], groups, False)
    log_freq = [np.zeros(len(g)) for g in groups]
    words = [_mt19937_words(5, 0, 624)]
    with pytest.raises(hip.EngineError, match=r"256 columns.*at most 255\b.*group size 8"):
        dg.gibbs_polyploid([0], 8, [10], [50], [100], log_freq[:1], [[0]], words)
    for group_size in (2, 9):
        with pytest.raises(hip.EngineError, match=rf"group size {group_size}\b"):
            dg.gibbs_polyploid([1], group_size, [10], [50], [100], log_freq[1:], [[0]], words)
    with pytest.raises(hip.EngineError, match=r"matrix 7\b"):
        dg.gibbs_polyploid([7], 4, [10], [50], [100], log_freq[1:], [[0]], words)
    got, consumed, _, (rounds, conditionals) = dg.gibbs_polyploid([], 4, [], [], [], [], [], np.zeros((0, 624), np.uint32))
    assert got == [] and len(consumed) == 0 and rounds == 0 and conditionals == 0
    # the wide problem is fine where the key has room for it: 256 columns at group size 7 (9 bits per member)
    got, consumed, _, _ = dg.gibbs_polyploid([0], 7, [3], [2], [4], log_freq[:1], [[0]], words)
    assert sum(got[0][1]) == 12 and int(consumed[0]) >= 3 * 7 + 2 * 3 * 6 * 7
    assert all(len(s) == 7 and list(s) == sorted(s) and s[-1] < 256 for s in got[0][0])


# ---- the estimators against the oracle ------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
@pytest.mark.parametrize("ploidy", [3, 4, 6, 8])
def test_estimators_follow_the_reference_stream_on_the_device(engine, model, ploidy):
    clusters = _small_clusters(8200 + ploidy, 5, max_paths=10 if ploidy < 8 else 8, max_reads=200)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(use_hap_gibbs=1, ploidy=ploidy, rng_seed=13)
    ref, _ = pyoracle.run(model, params, batch, 1)
    engine.reset_stats()
    got, _ = engine.run(model, params, engine.prepare(batch))
    _assert_on_the_device(engine)
    _compare(got, ref)
    assert fuzz_parity.compare(got, ref) == []
    if model == "haplotypes":
        for g, r in zip(got, ref):
            assert g.path_group_sets == r.path_group_sets  # first-seen order of the sampled sets


@pytest.mark.parametrize("ploidy", [3, 6])
def test_the_generator_is_left_where_the_reference_leaves_it(engine, ploidy):
    """--ind-hap-inference draws its subsets from the cluster's generator behind the sampler's chains."""
    clusters = _small_clusters(8300 + ploidy, 5, max_reads=200)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(use_hap_gibbs=1, ploidy=ploidy, ind_hap_inference=1, rng_seed=17)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 1)
    engine.reset_stats()
    got, _ = engine.run("haplotype-transcripts", params, engine.prepare(batch))
    _assert_on_the_device(engine)
    assert fuzz_parity.compare(got, ref) == []


# ---- fallbacks ------------------------------------------------------------------------------------------------

def test_without_room_for_the_distributions_the_host_driven_sampler_takes_the_call(engine):
    clusters = _small_clusters(8401, 5, max_reads=200)
    batch = ClusterBatch.from_clusters(clusters)
    for model in ("haplotypes", "haplotype-transcripts"):
        params = make_params(use_hap_gibbs=1, ploidy=4, rng_seed=11)
        ref, _ = pyoracle.run(model, params, batch, 1)
        os.environ["RPVG_HIP_GIBBS_BYTES"] = "64"
        try:
            engine.reset_stats()
            got, _ = engine.run(model, params, engine.prepare(batch))
            assert engine.stats()["gibbs_calls_completed"] == 0  # (the device gave the call up: the host-driven sampler ran)
        finally:
            del os.environ["RPVG_HIP_GIBBS_BYTES"]
        _compare(got, ref)
        engine.reset_stats()
        again, _ = engine.run(model, params, engine.prepare(batch))
        _assert_on_the_device(engine)
        _compare(again, ref)


# ---- repeatability, and the two routes ------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["haplotypes", "haplotype-transcripts"])
def test_ploidy_6_repeats_to_the_bit(engine, model):
    clusters = _small_clusters(8501, 6)
    batch = ClusterBatch.from_clusters(clusters)
    params = make_params(use_hap_gibbs=1, ploidy=6, rng_seed=3)
    first, _ = engine.run(model, params, engine.prepare(batch))
    second, _ = engine.run(model, params, engine.prepare(batch))
    assert _bits(first) == _bits(second)


_HOST_ROUTE_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from rpvg_amd import engine as eng_mod
from rpvg_amd.batch import ClusterBatch, make_params
from tests.test_hip_polyploid import _small_clusters
batch = ClusterBatch.from_clusters(_small_clusters(int(sys.argv[2]), int(sys.argv[3])))
e = eng_mod.Engine(0)
e.reset_stats()
got, _ = e.run("haplotypes", make_params(use_hap_gibbs=1, ploidy=5, rng_seed=29), e.prepare(batch))
span, completed = e.stats()["gibbs_ms"], e.stats()["gibbs_calls_completed"]
e.close()
print(json.dumps(dict(gibbs_ms=span, completed=completed, estimates=[[[list(s) for s in g.path_group_sets], [float(x) for x in g.posteriors]] for g in got])))
"""


def test_the_device_route_equals_the_host_driven_route_at_ploidy_5(engine):
    """RPVG_AMD_HOST_GIBBS (read once per process: a child has it) runs the chains on the host with the others of a
    conditional added in slot order; the same sets in the same order, and the same counts."""
    seed, n = 8601, 5
    env = dict(os.environ, RPVG_AMD_HOST_GIBBS="1")
    child = subprocess.run([sys.executable, "-c", _HOST_ROUTE_CHILD, ROOT, str(seed), str(n)], capture_output=True, text=True, env=env,
                           timeout=600)
    assert child.returncode == 0, child.stderr
    host = json.loads(child.stdout.strip().splitlines()[-1])
    assert host["gibbs_ms"] == 0 and host["completed"] == 0  # (the child did take the host-driven route)
    clusters = _small_clusters(seed, n)
    batch = ClusterBatch.from_clusters(clusters)
    engine.reset_stats()
    got, _ = engine.run("haplotypes", make_params(use_hap_gibbs=1, ploidy=5, rng_seed=29), engine.prepare(batch))
    _assert_on_the_device(engine)
    assert len(got) == len(host["estimates"]) == n
    for cl, g, (sets, posteriors) in zip(clusters, got, host["estimates"]):
        assert [list(s) for s in g.path_group_sets] == sets
        G = len(cl["paths"])
        samples = (10 + int(math.floor(0.01 * 5 * G + 0.5))) * (100 + int(math.floor(0.05 * 5 * G + 0.5)))
        assert [round(float(x) * samples) for x in g.posteriors] == [round(x * samples) for x in posteriors]


# ---- a cluster full enumeration sends here ----------------------------------------------------------------------

def test_the_cluster_over_the_set_bound_at_ploidy_8_runs_on_the_device(engine):
    """The clusters of test_ploidy_8_over_the_set_bound_names_the_cluster (test_hip_polyploid.py): 200 columns at ploidy 8
    fit the 8-bit key.  Not compared with the oracle (tens of thousands of conditionals in reference order)."""
    rng = np.random.default_rng(7802)
    clusters = [small_cases.make_cluster(rng, 1, [3], n_haps=3, n_reads=30),
                small_cases.make_cluster(rng, 1, [200], n_haps=200, n_reads=60)]
    prep = engine.prepare(ClusterBatch.from_clusters(clusters))
    engine.reset_stats()
    got, _ = engine.run("haplotypes", make_params(use_hap_gibbs=1, ploidy=8, rng_seed=7), prep)
    _assert_on_the_device(engine)
    wide = got[1]
    chains, its = 10 + round(0.01 * 8 * 200), 100 + round(0.05 * 8 * 200)
    assert abs(float(np.sum(wide.posteriors)) - 1.0) <= 1e-12
    assert len(wide.path_group_sets) >= 1
    for s in wide.path_group_sets:
        assert len(s) == 8 and list(s) == sorted(s) and 0 <= s[0] and s[-1] < 200
    counts = [float(x) * chains * its for x in wide.posteriors]
    assert all(abs(c - round(c)) <= 1e-6 for c in counts)
    assert sum(round(c) for c in counts) == chains * its
