"""The minimum-path-cover cases (tests/path_cover_cases.py) checked without a GPU: the model against the oracle's greedy
cover and its `strains` run, the decision margin of every case, and that the twin cases do separate a kernel that adds a
path's terms in row order from one that adds them in the order of the rows' entry lists."""
import math

import numpy as np
import pytest

from oracle import pyoracle
from rpvg_amd.batch import make_params
from tests import path_cover_cases as pcc


@pytest.mark.parametrize("case", pcc.CASES, ids=lambda c: c.name)
def test_model_equals_the_oracle_cover_on_row_order_weights(case):
    """pyoracle.min_path_cover on the dense cover matrix, the weights added up in row order as the oracle's `strains`
    estimator adds them (oracle/rpvg_oracle.cpp:750-762)."""
    cl = case.cluster()
    got = pyoracle.min_path_cover(pcc.dense_cover(cl), pcc.read_counts(cl), pcc.row_order_weights(cl))
    assert got == case.model().cover, case.name


def test_oracle_strains_run_solves_its_em_on_exactly_the_model_cover():
    ref, _ = pyoracle.run("strains", make_params(max_em_its=20), pcc.batch_of([c.cluster() for c in pcc.CASES]), pyoracle.max_threads())
    for case, est in zip(pcc.CASES, ref):
        cover = case.model().cover
        assert est.em_cols == ([tuple(cover)] if cover else []), case.name


@pytest.mark.parametrize("case", pcc.CASES, ids=lambda c: c.name)
def test_margin_condition_and_row_invariants(case):
    m = case.model()
    print(f"{case.name:40s} cover of {len(m.cover):3d}, margin {m.margin:.3e}")
    assert m.margin >= pcc.MIN_MARGIN, (case.name, m.margin)
    cl = case.cluster()
    assert len(cl.rows) <= 4096 and 1 <= cl.n_paths <= pcc.MAX_PATHS   # the margin's derivation: at most 4096 terms per weight
    for count, noise, groups in cl.rows:
        assert 0.0 < noise <= 1.0 and count >= 1 and len(groups) >= 1
        probs = [p for p, _ in groups]
        assert all(0.0 < p < 1.0 for p in probs) and all(a < b for a, b in zip(probs, probs[1:]))
        members = [j for _, ms in groups for j in ms]
        assert len(set(members)) == len(members) and all(0 <= j < cl.n_paths for j in members)


@pytest.mark.parametrize("case", pcc.TWIN_CASES, ids=lambda c: c.name)
def test_twin_cases_separate_row_order_from_entry_list_order(case):
    """Twins by the definition; bit-equal weights in row order and the first twin in the cover; bit-DIFFERENT weights in
    the emulated order of a thread per row with LDS atomics, the second twin's the smaller, and the cover a kernel with
    those weights returns holds the second twin instead — so the device tests of these cases cannot pass by accident."""
    cl = case.cluster()
    first, second = case.twins
    classes = pcc.twin_classes(cl)
    assert first < second and classes[second] == classes[first] == first
    m = case.model()
    assert first in m.cover and second not in m.cover
    exact, by_row, by_entry = pcc.exact_weights(cl), pcc.row_order_weights(cl), pcc.parent_order_weights(cl)
    assert exact[first] == exact[second] and by_row[first] == by_row[second]
    assert by_entry[second] < by_entry[first]
    assert abs(by_entry[first] - by_entry[second]) <= 1e-12 * exact[first]    # (the last bits only)
    emulated = pcc.cover_model(cl, weights=by_entry)
    assert second in emulated.cover and first not in emulated.cover
    assert [j for j in emulated.cover if j != second] == [j for j in m.cover if j != first]
    assert pcc.twin_seed_ok(cl, first, second)


def test_twin_cases_are_the_ones_the_issue_lists():
    kinds = {}
    for c in pcc.TWIN_CASES:
        kinds.setdefault(c.kind, []).append(c)
    one = kinds["twins_one_wavefront"]
    assert len([c for c in one if "_asc_" in c.name]) >= 8 and len([c for c in one if "_desc_" in c.name]) >= 8
    assert all(len(c.cluster().rows) == 48 and 3 <= c.cluster().n_paths <= 6 for c in one)
    assert all(len(c.cluster().rows) == 300 for c in kinds["twins_many_wavefronts"])
    assert {"_asc_", "_desc_"} == {t for c in kinds["twins_many_wavefronts"] for t in ("_asc_", "_desc_") if t in c.name}
    assert [c.twins for c in kinds["twins_across_the_reduction"]] == [(0, 256), (63, 64), (255, 256), (5, 300), (257, 513)]
    for c in kinds["twins_across_the_reduction"]:
        assert c.cluster().n_paths == 600
        assert c.twins[0] in c.model().order      # the pair is the best choice of one round: the tie decides the cover
    # the descending variant does list the second twin in front of the first
    desc = next(c for c in one if "_desc_" in c.name).cluster()
    assert any(ms[0] == 2 and ms[-1] == 0 for _, _, groups in desc.rows for _, ms in groups if len(ms) > 1)


def test_the_references_own_vector_goes_through_the_model():
    """src/tests/path_abundance_estimator_test.cpp:8-28."""
    cover = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 1]])
    col_rows = [[int(r) for r in np.nonzero(cover[:, j])[0]] for j in range(3)]
    assert pcc.greedy_cover(3, col_rows, [1, 3, 1, 5], [1.0, 1.0, 1.0])[0] == [0, 1]
    assert pcc.greedy_cover(3, col_rows, [1, 3, 1, 5], [1.0, 1.0, 0.01])[0] == [0, 1, 2]
    assert pcc.greedy_cover(1, [[0, 1]], [1, 1], [1.0])[0] == [0]


def test_wide_and_long_covers_are_what_the_cases_plant():
    for n in (255, 256, 257, 4096, 4097, 9600):
        case = pcc.BY_NAME[f"wide_{n}"]
        cl = case.cluster()
        planted = pcc.wide_planted(n)
        assert cl.n_paths == n and len(cl.rows) == 64
        assert case.model().cover == planted and len(planted) <= 8
        assert planted[0] == 0 and planted[-1] == n - 1 and (n <= 256 or {255, 256} <= set(planted))
    m = pcc.BY_NAME["long_cover"].model()
    assert m.cover == list(range(600)) and len(m.order) == 600
    descents = sum(a > b for a, b in zip(m.order, m.order[1:]))
    assert 200 < descents < 400, descents   # the rounds choose the paths in an order far from ascending


def test_noise_one_rows_count_nothing():
    cl = pcc.BY_NAME["noise_one"].cluster()
    counts = pcc.read_counts(cl)
    for (count, noise, groups), c in zip(cl.rows, counts):
        holds_winner = any(pcc.NOISE_ONE_WINNER in ms for _, ms in groups)
        assert holds_winner == (noise in pcc.NOISE_ONE) == (c == 0)
        assert noise in pcc.NOISE_ONE + pcc.NOISE_NOT_ONE and (c == 0 or c == count)
    assert {noise for _, noise, _ in cl.rows} == set(pcc.NOISE_ONE + pcc.NOISE_NOT_ONE)
    assert 1.0 - 1e-14 < 1.0 and pyoracle.lib().rpvg_oracle_double_compare(1.0 - 1e-14, 1.0) == 1
    assert pyoracle.lib().rpvg_oracle_double_compare(1.0 - 4e-14, 1.0) == 0
    m = pcc.BY_NAME["noise_one"].model()
    assert pcc.NOISE_ONE_WINNER not in m.cover and len(m.cover) >= 1
    assert pcc.cover_model(cl, noise_rule=False).order[0] == pcc.NOISE_ONE_WINNER   # it would win if its rows counted
    nothing = pcc.BY_NAME["nothing_to_cover"]
    assert nothing.cluster().n_paths > 1 and set(pcc.read_counts(nothing.cluster())) == {0} and nothing.model().cover == []
    assert pcc.BY_NAME["single_path"].model().cover == [0] and pcc.BY_NAME["single_path_noise_one"].model().cover == [0]
    assert set(pcc.read_counts(pcc.BY_NAME["single_path_noise_one"].cluster())) == {0}


def test_listings_of_several_in_one_call():
    base, listings = pcc.several_in_one_call()
    assert {c.kind for c in base} == {c.kind for c in pcc.CASES}
    perm, _ = listings["permutation"]
    assert sorted(perm) == list(range(len(base))) and perm != sorted(perm)
    sub, _ = listings["subset"]
    assert 1 < len(set(sub)) == len(sub) < len(base)
    dup, _ = listings["one cluster twice"]
    twice = [k for k in set(dup) if dup.count(k) == 2]
    assert len(twice) == 1 and base[twice[0]].name == "long_cover"
    everything, extra = listings["larger output ranges"]
    assert everything == list(range(len(base))) and max(extra) > 0 and min(extra) == 0
    assert math.isinf(pcc.BY_NAME["single_path"].model().margin)
