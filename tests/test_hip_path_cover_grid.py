"""rpvg_hip_min_path_cover_any: the minimum path cover of clusters of any size — the whole-GPU route (path_cover_grid.hip) at its
edges, both routes on one input, and `-i strains` on clusters the workgroup route cannot hold.

Every case of tests/path_cover_cases.py and of tests/path_cover_grid_cases.py has a decision margin of at least 1e-9 (asserted
on the CPU: tests/test_path_cover_cases.py, tests/test_path_cover_grid_cases.py), far above what a chain of at most 4 096
additions of one sign and the device's log can move, so the device must return the model's cover AND the model's order of
choices exactly — the index lists.  Between twins only bit-equal weights give the lower index.  Both routes add a path's weight
up in the same order, so on ANY input they return the same cover: the random clusters need no margin.  No case is skipped,
masked or loosened here.
"""
import pytest

from oracle import pyoracle
from rpvg_amd import engine as eng_mod, hip
from rpvg_amd.batch import make_params
from tests import path_cover_cases as pcc
from tests import path_cover_grid_cases as grid
from tests.test_hip_models import _compare

pytestmark = pytest.mark.gpu

ALL_CASES = pcc.CASES + grid.CASES
INDEX = {c.name: i for i, c in enumerate(ALL_CASES)}
EVERYTHING = 1              # grid_min_work: every cluster of at least two paths over the whole GPU
NEVER = hip.GRID_NEVER      # ... every cluster that fits on the workgroup route


@pytest.fixture(scope="module")
def table(hip_ctx):
    """Every case, old and new, uploaded as one batch."""
    dev = hip_ctx.upload(pcc.batch_of([c.cluster() for c in ALL_CASES]))
    yield dev
    dev.free()


_ALONE = {}


def _alone(hip_ctx, table, case):
    """(cover, order, whole-GPU problems counted, rounds counted) of a case in a call of its own on the whole-GPU route (computed once)."""
    if case.name not in _ALONE:
        hip_ctx.reset_stats()
        covers, orders = hip_ctx.min_path_cover_any(table, [INDEX[case.name]], grid_min_work=EVERYTHING, order=True)
        s = hip_ctx.stats()
        _ALONE[case.name] = (covers[0], orders[0], s["cover_grid_problems"], s["cover_grid_rounds"])
    return _ALONE[case.name]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_on_the_grid_route_equals_the_model_cover_and_order(hip_ctx, table, case):
    cover, order, problems, rounds = _alone(hip_ctx, table, case)
    m = case.model()
    assert cover == m.cover, case.name
    if case.cluster().n_paths == 1:   # never the whole GPU: the cover is {0}
        assert (order, problems, rounds) == (None, 0, 0)
    else:
        assert order == m.order, case.name
        assert (problems, rounds) == (1, len(m.cover))


@pytest.mark.parametrize("case", pcc.TWIN_CASES + grid.TWIN_CASES, ids=lambda c: c.name)
def test_twins_take_the_first_index_on_the_grid_route(hip_ctx, table, case):
    first, second = case.twins
    got = _alone(hip_ctx, table, case)[0]
    assert first in got and second not in got, (case.name, got)


def test_both_routes_agree_on_200_random_clusters(hip_ctx):
    clusters = [grid.random_small_cluster(s) for s in grid.RANDOM_SEEDS]
    dev = hip_ctx.upload(pcc.batch_of(clusters))
    try:
        listed = list(range(len(clusters)))
        hip_ctx.reset_stats()
        on_grid = hip_ctx.min_path_cover_any(dev, listed, grid_min_work=EVERYTHING)
        assert hip_ctx.stats()["cover_grid_problems"] == len(clusters)
        hip_ctx.reset_stats()
        on_workgroups = hip_ctx.min_path_cover_any(dev, listed, grid_min_work=NEVER)
        assert hip_ctx.stats()["cover_grid_problems"] == 0
        assert on_workgroups == hip_ctx.min_path_cover(dev, listed)
        different = [(s, a, b) for s, a, b in zip(grid.RANDOM_SEEDS, on_grid, on_workgroups) if a != b]
        assert not different, different[:3]
    finally:
        dev.free()


def test_three_calls_give_the_same_lists_and_orders(hip_ctx, table):
    cases = [c for c in ALL_CASES if c.kind in ("twins_many_wavefronts", "grid_long_cover", "grid_twins")]
    listed = [INDEX[c.name] for c in cases]
    calls = [hip_ctx.min_path_cover_any(table, listed, grid_min_work=EVERYTHING, order=True) for _ in range(3)]
    assert calls[0] == calls[1] == calls[2]
    assert calls[0][0] == [c.model().cover for c in cases] and calls[0][1] == [c.model().order for c in cases]


def test_several_in_one_call_split_between_the_routes_equal_each_cluster_alone(hip_ctx, table):
    base, listings = pcc.several_in_one_call()
    works = sorted(grid.work_of(c.cluster()) for c in base if c.cluster().n_paths > 1)
    threshold = works[len(works) // 2]   # half of the clusters over the whole GPU, half side by side on workgroups
    for name, (listed, extra) in listings.items():
        hip_ctx.reset_stats()
        covers, orders = hip_ctx.min_path_cover_any(table, [INDEX[base[k].name] for k in listed], extra=extra, grid_min_work=threshold, order=True)
        on_grid = [k for k in listed if base[k].cluster().n_paths > 1 and grid.work_of(base[k].cluster()) >= threshold]
        assert 0 < len(on_grid) < len(listed), name
        assert hip_ctx.stats()["cover_grid_problems"] == len(on_grid)
        assert len(covers) == len(listed)
        for k, cover, order in zip(listed, covers, orders):
            m = base[k].model()
            assert cover == _alone(hip_ctx, table, base[k])[0] == m.cover, (name, base[k].name)
            assert order == (m.order if k in on_grid else None), (name, base[k].name)
    twice = [k for k in listings["one cluster twice"][0] if listings["one cluster twice"][0].count(k) == 2]
    assert twice and grid.work_of(base[twice[0]].cluster()) >= threshold   # the cluster listed twice runs twice over the whole GPU


def _strains(batch):
    ref, _ = pyoracle.run("strains", make_params(), batch, pyoracle.max_threads())
    eng = eng_mod.Engine(0)
    try:
        eng.reset_stats()
        got, _ = eng.run("strains", make_params(), eng.prepare(batch))
        stats = eng.stats()
    finally:
        eng.close()
    return got, ref, stats


def test_strains_on_clusters_wider_than_the_workgroup_route(hip_ctx):
    """A 9 601-path and a 65 537-path cluster next to a small one: the default threshold sends the two over the whole GPU, and
    Engine.run("strains") — cover, partial matrix, collapse, EM — equals the oracle: group sets and EM iteration counts exactly,
    values by _compare of tests/test_hip_models.py.  (rpvg_hip_min_path_cover refuses this batch.)"""
    cases = [pcc.BY_NAME["noise_one"], grid.BY_NAME[f"grid_wide_{grid.WIDE_PATHS[0]}"], grid.BY_NAME[f"grid_wide_{grid.WIDE_PATHS[-1]}"]]
    assert [c.cluster().n_paths for c in cases][1:] == [9601, 65537]
    batch = pcc.batch_of([c.cluster() for c in cases])
    dev = hip_ctx.upload(batch)
    try:
        hip_ctx.reset_stats()
        covers, orders = hip_ctx.min_path_cover_any(dev, [0, 1, 2], order=True)
        assert covers == [c.model().cover for c in cases]
        assert orders[1:] == [c.model().order for c in cases[1:]]
        assert orders[0] is None and hip_ctx.stats()["cover_grid_problems"] == 2   # (the small one stays on its workgroup)
        with pytest.raises(hip.EngineError, match="9601|65537"):
            hip_ctx.min_path_cover(dev, [0, 1, 2])
    finally:
        dev.free()
    got, ref, stats = _strains(batch)
    for case, g, r in zip(cases, got, ref):
        assert g.em_cols == r.em_cols == [tuple(case.model().cover)], case.name
    _compare(got, ref)
    assert stats["cover_grid_problems"] >= 2


def test_a_cluster_at_the_work_threshold_takes_the_grid_route(hip_ctx):
    """Narrower than the workgroup route's limit, so only its work (rows + entries) decides.  The library's default threshold is
    read from the plan; where the plan says "width only" (the measured table gave no size at which the whole GPU is twice as
    fast for every cover length) the cluster's own work is passed as the threshold: at it the whole GPU, one above it a
    workgroup.  The planted columns have 4 096 rows (32 768 rows in all, with the default at 2^16): 4 096 * 2^-53 ~ 4.5e-13
    relative on a weight, three orders of magnitude below the margin (asserted on the CPU); with R rows per weight the bound
    R * 2^-53 still lies two orders of magnitude below 1e-9 up to 10^5 rows."""
    case = grid.THRESHOLD_CASE
    cl, m = case.cluster(), case.model()
    work, default = grid.work_of(cl), int(grid.LIMITS.default_grid_min_work)
    batch = pcc.batch_of([cl])
    dev = hip_ctx.upload(batch)
    try:
        if default != grid.WIDTH_ONLY:
            assert default <= work < 2 * default
        for threshold, problems in ((0, 0 if default == grid.WIDTH_ONLY else 1), (work, 1), (work + 1, 0), (NEVER, 0)):
            hip_ctx.reset_stats()
            covers, orders = hip_ctx.min_path_cover_any(dev, [0], grid_min_work=threshold, order=True)
            assert hip_ctx.stats()["cover_grid_problems"] == problems, threshold
            assert covers == [m.cover], threshold
            assert orders == [m.order if problems else None], threshold
    finally:
        dev.free()
    got, ref, stats = _strains(batch)
    assert got[0].em_cols == ref[0].em_cols == [tuple(m.cover)]
    _compare(got, ref)
    assert stats["cover_grid_problems"] == (0 if default == grid.WIDTH_ONLY else 1)
