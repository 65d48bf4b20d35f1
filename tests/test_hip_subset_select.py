"""The select kernels of `-i haplotype-transcripts` on the device (rpvg_amd/csrc/subset_em.hip: subsetSelectSmallKernel, one
wavefront per matrix up to 64 kept pairs, and subsetSelectWideKernel behind it) at the shapes where their paths part: both sides
of the small / wide cut, a selection near the 1 024 the wide kernel holds, diplotypes that share a path list (leaders with
members), column lists past the LDS cache, and more wide matrices than the wide launch has workgroups.

Every case is compared three ways: against the host-driven route (RPVG_HIP_NO_DEVICE_SUBSETS=1: the same path subsets, posteriors
equal to the bit, the same EM columns and iteration counts — the assertions of
tests/test_hip_models.py::test_device_subset_path_equals_the_separate_calls), against the oracle (that file's _compare), and
against a second run of itself, bit for bit.

What a case needs of its clusters (kept pairs, selected diplotypes, subsets) is asserted from the oracle alone: the matrix of the
numpy model (oracle/np_oracle.py), the bounded search of the C++ oracle on it, the oracle's estimates.  The seeds were chosen on
the CPU so that these hold, and none puts a posterior within 0.5 % of min_hap_prob (the knife edge of docs/design/parity.md)."""
import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import engine as eng_mod
from rpvg_amd.batch import ClusterBatch, make_params
from tests import small_cases
from tests.test_hip_models import _compare

pytestmark = pytest.mark.gpu

MIN_HAP_PROB = 0.001   # make_params() default
SMALL_SELECTED = 64    # kSmallSelected: more kept pairs than this go to the wide kernel
WIDE_CACHED_PATHS = 6144   # kWideCachedPaths, kSmallCachedPaths: column list entries the kernels copy into LDS
SMALL_CACHED_PATHS = 1024
WIDE_GRID = 128        # workgroups of the wide launch


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.Engine(0)
    yield e
    e.close()


def _facts(cluster):
    """What the selection of one cluster works on, from the oracle: columns and the entries of their path lists, the pairs the
    bounded search keeps, the diplotypes at or above min_hap_prob, their distinct merged path lists, and how close (relative) a
    posterior comes to min_hap_prob."""
    paths, rows = cluster["paths"], cluster["rows"]
    groups, mult = np_oracle.source_groups(paths)
    G, noise, counts = np_oracle.grouped_matrix(rows, groups)
    Gn = np_oracle.add_noise_and_normalize(G, noise)
    Gn, gcounts = np_oracle.read_collapse(Gn, counts, 1e-8)
    sets, post = pyoracle.group_posteriors(Gn[:, :-1].copy(), Gn[:, -1].copy(), gcounts, mult, 2, bounded=True, min_rel_lik=MIN_HAP_PROB)
    selected = [s for s, p in zip(sets, post) if p >= MIN_HAP_PROB]
    lists = set(tuple(sorted(p for g in s for p in groups[g])) for s in selected)
    return dict(columns=len(groups), entries=sum(len(g) for g in groups), kept=len(sets), selected=len(selected), lists=len(lists),
                margin=min((abs(p - MIN_HAP_PROB) / MIN_HAP_PROB for p in post), default=1.0))


def _cluster(seed, n_transcripts, hst, n_haps, n_reads):
    return small_cases.make_cluster(np.random.default_rng(seed), n_transcripts, hst, n_haps=n_haps, n_reads=n_reads, empty_read_frac=0.0)


def _same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.path_group_sets == y.path_group_sets, k
        assert np.array_equal(x.posteriors, y.posteriors) and np.array_equal(x.abundances, y.abundances), k
        assert x.noise_count == y.noise_count and x.total_count == y.total_count, k
        assert list(x.em_cols) == list(y.em_cols) and list(x.em_iters) == list(y.em_iters), k


def _three_ways(engine, monkeypatch, clusters):
    """The device route against the host-driven one, the oracle and itself; returns the oracle's estimates."""
    batch = ClusterBatch.from_clusters(clusters)
    prep = engine.prepare(batch)
    params = make_params()
    fused, _ = engine.run("haplotype-transcripts", params, prep)
    again, _ = engine.run("haplotype-transcripts", params, prep)
    monkeypatch.setenv("RPVG_HIP_NO_DEVICE_SUBSETS", "1")
    separate, _ = engine.run("haplotype-transcripts", params, prep)
    monkeypatch.delenv("RPVG_HIP_NO_DEVICE_SUBSETS")
    for k, (f, s) in enumerate(zip(fused, separate)):
        fk, sk = f.keyed(), s.keyed()
        assert set(fk) == set(sk), k
        for key in sk:
            assert fk[key][0] == sk[key][0], (k, key)  # posteriors: sums of subset weights in the same order
            assert small_cases.rel_close(fk[key][1], sk[key][1], rel=1e-12, floor=1e-300), (k, key)
        assert list(f.em_cols) == list(s.em_cols) and list(f.em_iters) == list(s.em_iters), k
        assert f.total_count == s.total_count and abs(f.noise_count - s.noise_count) <= 1e-12 * max(1.0, s.total_count)
    ref, _ = pyoracle.run("haplotype-transcripts", params, batch, 4)
    _compare(fused, ref)
    _same_bits(fused, again)
    return ref


def test_both_sides_of_the_small_wide_cut(engine, monkeypatch):
    """64 kept pairs: the last matrix of the one-wave kernel, every slot of its LDS arrays in use; 65: the first of the wide one."""
    at_cut, past_cut, past_cut_two_rows = _cluster(9001, 1, (64,), 64, 1), _cluster(9006, 1, (65,), 65, 1), _cluster(9000, 1, (33,), 33, 1)
    facts = [_facts(c) for c in (at_cut, past_cut, past_cut_two_rows)]
    assert [f["kept"] for f in facts] == [SMALL_SELECTED, SMALL_SELECTED + 1, SMALL_SELECTED + 1], facts
    assert [f["selected"] for f in facts] == [64, 65, 65] and min(f["margin"] for f in facts) > 0.005, facts
    clusters = small_cases.make_batch_clusters(9100, n_clusters=5, with_empty=True) + [at_cut, past_cut, past_cut_two_rows]
    ref = _three_ways(engine, monkeypatch, clusters)
    assert [len(r.em_iters) for r in ref[-3:]] == [64, 65, 65]


@pytest.mark.parametrize("columns,seed,selected", [(36, 9415, 632), (44, 9435, 947)])
def test_selection_near_the_cap(engine, monkeypatch, columns, seed, selected):
    """A flat posterior: nearly every heterozygous diplotype of 36 / 44 haplotype columns passes min_hap_prob (of the 990 pairs of
    44 columns all but the homozygous ones), so the groups are sorted at 1 024 slots, and the retained subsets as well."""
    rng = np.random.default_rng(seed)
    cluster = small_cases.make_cluster(rng, 1, (columns,), n_haps=columns, n_reads=int(rng.integers(1, 4)), empty_read_frac=0.0)
    f = _facts(cluster)
    assert f["selected"] == selected and f["kept"] == columns * (columns + 1) // 2 and f["margin"] > 0.005, f
    ref = _three_ways(engine, monkeypatch, small_cases.make_batch_clusters(9101, n_clusters=3, with_empty=False) + [cluster])
    most_subsets = max(len(r.em_iters) for r in ref)
    assert most_subsets > 512, most_subsets  # the sorts run at 1 024 slots


def _shared_lists(seed, hst, n_haps):
    rng = np.random.default_rng(seed)
    return small_cases.make_cluster(rng, 3, hst, n_haps=n_haps, n_reads=int(rng.integers(1, 4)), empty_read_frac=0.0)


def test_diplotypes_that_share_a_path_list(engine, monkeypatch):
    """Several transcripts of two or three HSTs: different pairs of haplotype columns carry the same paths between them, so a
    subset has a leader and members whose posteriors are added in pair order — in the one-wave kernel (the first three clusters) and in
    the wide one (the last two)."""
    clusters = [_shared_lists(seed, (2, 2, 3), 12) for seed in (9628, 9633, 9638)] + [_shared_lists(seed, (3, 3, 3), 30) for seed in (9676, 9683)]
    facts = [_facts(c) for c in clusters]
    assert max(f["kept"] for f in facts[:3]) <= SMALL_SELECTED < min(f["kept"] for f in facts[3:]), facts
    assert min(f["margin"] for f in facts) > 0.005, facts
    ref = _three_ways(engine, monkeypatch, clusters)
    fewer = [len(r.em_iters) < f["selected"] for r, f in zip(ref, facts)]
    assert any(fewer[:3]) and any(fewer[3:]), (fewer, facts)  # some cluster has fewer subsets than selected diplotypes


def test_column_lists_past_the_lds_cache(engine, monkeypatch):
    """100 transcripts of two HSTs, 64 haplotypes that carry one HST of each: the column lists have 6 400 entries, the wide kernel
    walks them in device memory, and the lists of all diplotypes begin alike, so the rank falls back on whole comparisons.  The
    second cluster does the same to the one-wave kernel (1 200 entries, few kept pairs)."""
    rng = np.random.default_rng(9712)
    wide = small_cases.make_cluster(rng, 100, (2,) * 100, n_haps=64, n_reads=2, empty_read_frac=0.0)
    rng = np.random.default_rng(9713)
    small = small_cases.make_cluster(rng, 40, (2,) * 40, n_haps=30, n_reads=60, empty_read_frac=0.0)
    fw, fs = _facts(wide), _facts(small)
    assert fw["entries"] > WIDE_CACHED_PATHS and fw["kept"] > SMALL_SELECTED and fw["selected"] > 100 and fw["margin"] > 0.005, fw
    assert fs["entries"] > SMALL_CACHED_PATHS and 1 < fs["kept"] <= SMALL_SELECTED and fs["selected"] > 1 and fs["margin"] > 0.005, fs
    _three_ways(engine, monkeypatch, [wide, small])


def test_more_wide_matrices_than_workgroups(engine, monkeypatch):
    """140 matrices of 65 columns, every one with more than 64 kept pairs: the wide launch has 128 workgroups, so twelve of them
    take a second matrix through the same LDS."""
    rng = np.random.default_rng(9801)
    wide = [small_cases.make_cluster(rng, 1, (65,), n_haps=65, n_reads=1, empty_read_frac=0.0) for _ in range(140)]
    facts = [_facts(c) for c in wide]
    assert sum(f["kept"] > SMALL_SELECTED for f in facts) > WIDE_GRID and min(f["margin"] for f in facts) > 0.005
    _three_ways(engine, monkeypatch, small_cases.make_batch_clusters(9102, n_clusters=4, with_empty=True) + wide)
