"""rpvg_hip_min_path_cover at its edges (tests/path_cover_cases.py) against the plain-Python model of the reference's
weighted minimum path cover.

Every case has a decision margin of at least 1e-9 (asserted on the CPU, tests/test_path_cover_cases.py), far above what
the order of the weight sums and the device's log can move, so the device must return the model's cover exactly — the
index lists.  Between twin paths only bit-equal weights give the reference's answer, the lower index: the twin cases are
drawn so that a kernel adding a path's terms in the order of the rows' entry lists returns the higher one.  No case is
skipped, masked or loosened here.
"""
import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import make_params
from tests import path_cover_cases as pcc
from tests.test_hip_models import _compare

pytestmark = pytest.mark.gpu

INDEX = {c.name: i for i, c in enumerate(pcc.CASES)}


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case, uploaded as one batch."""
    dev = hip_ctx.upload(pcc.batch_of([c.cluster() for c in pcc.CASES]))
    yield dev
    dev.free()


_ALONE = {}


def _alone(hip_ctx, table, case):
    """The cover of a case in a call of its own (computed once)."""
    if case.name not in _ALONE:
        _ALONE[case.name] = hip_ctx.min_path_cover(table, [INDEX[case.name]])[0]
    return _ALONE[case.name]


@pytest.mark.parametrize("case", pcc.CASES, ids=lambda c: c.name)
def test_case_equals_the_model(hip_ctx, table, case):
    assert _alone(hip_ctx, table, case) == case.model().cover, case.name


@pytest.mark.parametrize("case", pcc.TWIN_CASES, ids=lambda c: c.name)
def test_twins_take_the_first_index(hip_ctx, table, case):
    first, second = case.twins
    got = hip_ctx.min_path_cover(table, [INDEX[case.name]])[0]
    assert first in got and second not in got, (case.name, got)


def test_three_calls_give_the_same_lists(hip_ctx, table):
    cases = [c for c in pcc.CASES if c.kind == "twins_many_wavefronts"]
    assert len(cases) >= 2
    listed = [INDEX[c.name] for c in cases]
    calls = [hip_ctx.min_path_cover(table, listed) for _ in range(3)]
    assert calls[0] == calls[1] == calls[2] == [c.model().cover for c in cases]


def test_several_in_one_call_equal_each_cluster_alone(hip_ctx, table):
    base, listings = pcc.several_in_one_call()
    for name, (listed, extra) in listings.items():
        got = hip_ctx.min_path_cover(table, [INDEX[base[k].name] for k in listed], extra=extra)
        assert len(got) == len(listed)
        for k, cover in zip(listed, got):
            assert cover == _alone(hip_ctx, table, base[k]) == base[k].model().cover, (name, base[k].name)


def test_a_cluster_of_9601_paths_is_refused_before_anything_is_launched(hip_ctx):
    small = pcc.BY_NAME["noise_one"].cluster()
    rows = [(3, 0.1, [(0.2, [0]), (0.3, [pcc.MAX_PATHS])]), (2, 0.05, [(0.4, [17])])]
    dev = hip_ctx.upload(pcc.batch_of([small, pcc.Cluster(pcc.MAX_PATHS + 1, rows)]))
    try:
        for listed in ([1], [0, 1]):
            hip_ctx.reset_stats()
            with pytest.raises(hip.EngineError, match=str(pcc.MAX_PATHS + 1)):
                hip_ctx.min_path_cover(dev, listed)
            assert hip_ctx.stats()["build_launches"] == 0
        assert hip_ctx.min_path_cover(dev, [0]) == [pcc.BY_NAME["noise_one"].model().cover]
    finally:
        dev.free()


def test_strains_on_the_edge_clusters_matches_the_oracle():
    """Engine.run("strains") — cover, partial matrix, collapse, EM — on the twin clusters, the noise-one rows, a cluster
    with nothing to cover and the one-path clusters: group sets identical, EM iteration counts exact, 1e-6 (_compare of
    tests/test_hip_models.py).  A cluster with nothing to cover keeps the all-zero estimates of
    src/path_abundance_estimator.cpp:219 (:254 skips the rest)."""
    cases = pcc.TWIN_CASES + [pcc.BY_NAME[n] for n in ("noise_one", "nothing_to_cover", "single_path", "single_path_noise_one")]
    batch = pcc.batch_of([c.cluster() for c in cases])
    ref, _ = pyoracle.run("strains", make_params(), batch, 2)
    eng = eng_mod.Engine(0)
    try:
        got, _ = eng.run("strains", make_params(), eng.prepare(batch))
    finally:
        eng.close()
    for case, g, r in zip(cases, got, ref):
        cover = case.model().cover
        assert g.em_cols == r.em_cols == ([tuple(cover)] if cover else []), case.name
    _compare(got, ref)
    nothing = got[[c.name for c in cases].index("nothing_to_cover")]
    assert nothing.total_count == 0 and nothing.noise_count == 0 and not np.any(nothing.abundances)
