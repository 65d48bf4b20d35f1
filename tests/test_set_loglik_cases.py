"""The cases of the set log-likelihoods (tests/set_loglik_cases.py) checked without a GPU: the conditions under which the device
tests (tests/test_hip_set_loglik.py) can neither pass nor fail by accident, asserted on the long-double model and the FP64
reference alone — the reference agrees with the model and sets the tolerance, every posterior is a normal double, every row and
every requested column moves some output far above the tolerance, three wrong models miss by as much — and that the cases put
the row classes, the strides, the segments and the folds where their names say."""
import math

import numpy as np
import pytest

from oracle import np_oracle
from rpvg_amd import hip
from tests import set_loglik_cases as slc

SET_CASES = slc.cases_of("sets")
FULL_CASES = slc.cases_of("full")


@pytest.mark.parametrize("case", SET_CASES, ids=lambda c: c.name)
def test_conditions_of_the_set_sums(case):
    ref = case.reference()
    M, noise, counts, _ = case.matrix()
    outs = slc.outputs_of(case)
    assert M.shape == (case.R, case.G) and len(ref.model) == len(outs) == len(ref.oracle) and case.empty == 0
    terms = slc.output_terms(case)
    rows = np.max(np.abs(terms), axis=1)
    columns = slc.column_bites(case)
    print(f"{case.name:32s} {case.R:5d} x {case.G:2d}, {len(outs):4d} outputs: max |ll| {ref.max_abs_ll:9.1f}, oracle {ref.oracle_deviation:.1e}, "
          f"tol {ref.tol:.1e}, row bite {rows.min():.1e}, column bite {min(columns.values(), default=math.inf):.1e}")

    # (a) the FP64 reference agrees with the model: R additions of terms of one sign and a logarithm per term, (R + 8) 2^-52 max |ll|
    assert np.all(np.isfinite(ref.oracle)) and np.all(np.isfinite(ref.model.astype(np.float64)))
    assert ref.oracle_deviation <= (case.R + 8) * 2.0 ** -52 * ref.max_abs_ll
    assert ref.tol == max(8 * ref.oracle_deviation, 2.0 ** -50 * ref.max_abs_ll) > 0
    assert np.allclose(terms.sum(axis=0), ref.oracle, rtol=1e-12, atol=0)      # (the terms are those of the outputs)

    # (c) every row bites — no case here has rows of noise 1 without entries: none is exempt —, and every column an output names
    assert np.all(rows >= slc.BITE * ref.tol)
    named = {m for members, _, _ in outs for m in members} - {slc.NO_MEMBER}
    assert named == set(range(case.G))      # (a case that keeps its member lists to some columns still has every column a candidate)
    assert set(columns) == (named if case.G > 1 else set()) and all(b >= slc.BITE * ref.tol for b in columns.values())

    # (d) a row class left out misses
    perm, fast_end, mid_end = slc.device_rows(counts, noise)
    for a, b in ((0, fast_end), (fast_end, mid_end), (mid_end, case.R)):
        if b > a:
            assert np.max(np.abs(terms[perm[a:b]].sum(axis=0))) >= slc.BITE * ref.tol

    # (e) the class sizes are the ones the case names
    assert case.ends == (fast_end, mid_end)


@pytest.mark.parametrize("case", FULL_CASES, ids=lambda c: c.name)
def test_conditions_of_the_enumeration(case):
    ref = case.reference()
    M, noise, counts, mult = case.matrix()
    assert case.full and set(ref.full) == set(case.full)
    for g, full in ref.full.items():
        sets = len(full.sets)
        assert sets == math.comb(case.G + g - 1, g) and full.sets == slc.multisets(case.G, g)
        spread = float(full.log_posterior.max() - full.log_posterior.min())
        print(f"{case.name:32s} {case.R:5d} x {case.G:3d} sets of {g}: {sets:5d} sets, spread {spread:7.1f}, oracle {full.oracle_deviation:.1e} "
              f"(normaliser {full.oracle_best:.1e}), tol {full.tol:.1e}")

        # (a) the reference agrees with the model; its normaliser folds add_log over the sets one by one: an ulp of the running value each
        bar = (case.R + 8 + 2 * g) * 2.0 ** -52 * full.max_abs_ll
        assert full.oracle_deviation <= bar and full.oracle_best <= bar + sets * 2.0 ** -52 * full.max_abs_ll
        assert full.tol == max(8 * full.oracle_deviation, 2.0 ** -50 * full.max_abs_ll) > 0
        assert abs(float(full.oracle_posteriors.sum()) - 1) < 1e-9
        assert abs(float(np.sum(np.exp(full.log_posterior))) - 1) < 1e-15 * sets

        # (b) every posterior is a normal double — but in the underflow case, where every set lies on one side, well off the brink
        if case.underflow:
            assert spread > slc.UNDERFLOW and 0 < int(np.sum(~full.kept)) < sets
            assert not np.any((full.log_posterior < -slc.MAX_SPREAD) & (full.log_posterior >= -slc.UNDERFLOW - 40))
            assert np.all(full.oracle_posteriors[~full.kept] == 0) and math.exp(-slc.UNDERFLOW) == 0.0
        else:
            assert spread <= slc.MAX_SPREAD and np.all(full.kept)
            assert math.exp(-(slc.MAX_SPREAD + math.log(sets))) > 1e10 * np.finfo(np.float64).tiny
        assert np.all(full.oracle_posteriors[full.kept] > 1e-290)

        # (c) every row moves one set against another (one column: a single set of posterior 1 whatever the rows — its sum is held
        # through rpvg_hip_group_loglik by the cases of the "sets" route), and every column differs from its neighbour
        if case.G > 1:
            idx = np.array(full.sets)
            x = noise[:, None] + sum(M[:, idx[:, w]] for w in range(g)) / g
            terms = counts[:, None] * np.log(x)
            assert np.all(terms.max(axis=1) - terms.min(axis=1) >= slc.BITE * full.tol)
            single = full.ll[[slc.rank_of_members(case.G, (a,) * g) for a in range(case.G)]]
            assert np.all(np.abs(np.diff(single.astype(np.float64))) >= slc.BITE * full.tol)


def test_the_enumerations_stand_on_their_edges():
    shapes = [(c.G, g) for c in FULL_CASES for g in c.full]
    assert set(slc.FULL_SHAPES) <= set(shapes)
    # a wave walks the candidates last .. G - 1 of its prefix in blocks of four: every remainder of G - last, for whole blocks and none
    assert {(G - last) % slc.CANDIDATES for G, g in slc.FULL_SHAPES for last in range(G)} == {0, 1, 2, 3}
    assert {(G - last) % slc.CANDIDATES for G, g in slc.FULL_SHAPES if g > 1 and G > slc.CANDIDATES for last in range(G)} == {0, 1, 2, 3}
    counts = {shape: math.comb(shape[0] + shape[1] - 1, shape[1]) for shape in slc.FULL_SHAPES}
    assert counts[(12, 5)] == 4368 and counts[(8, 8)] == 6435 and counts[(23, 3)] == 2300 and max(counts.values()) == 6435
    # one thread per set, one set short of it and one over
    assert [counts[(G, 1)] - slc.NORMALISE_THREADS for G in (255, 256, 257)] == [-1, 0, 1]
    assert any(counts[s] > 2 * slc.NORMALISE_THREADS and counts[s] % slc.NORMALISE_THREADS for s in counts)
    assert max(c.R for c in FULL_CASES if "sets" not in c.routes and not c.underflow) <= 70
    assert sorted(c.ends[0] for c in FULL_CASES if "sets" in c.routes) == [slc.MULTI_SEGMENT - 1, slc.MULTI_SEGMENT, slc.MULTI_SEGMENT + 1]


@pytest.mark.parametrize("G,g", [s for s in slc.FULL_SHAPES if s[0] < 255] + [(255, 2), (3, 8), (7, 1)])
def test_rank_and_members_as_restated(G, g):
    sets = slc.multisets(G, g)
    step = max(1, len(sets) // 700)
    picked = list(range(0, len(sets), step)) + [len(sets) - 1]
    assert [slc.members_of_rank(G, g, r) for r in picked] == [sets[r] for r in picked]
    assert [slc.rank_of_members(G, sets[r]) for r in picked] == picked
    # the prefixes of the kernel's waves: the sets of one prefix are consecutive, last member from the prefix's largest on
    if g > 1:
        for p, prefix in enumerate(slc.multisets(G, g - 1)[:50]):
            assert slc.members_of_rank(G, g - 1, p) == prefix
            first = slc.rank_of_members(G, prefix + (prefix[-1],))
            assert [sets[first + k] for k in range(G - prefix[-1])] == [prefix + (k,) for k in range(prefix[-1], G)]


def test_full_set_count_is_the_binomial():
    count = hip.lib().rpvg_hip_full_set_count
    for G in list(range(0, 14)) + [23, 40, 255, 256, 257, 1000]:
        for g in range(1, 9):
            want = math.comb(G + g - 1, g) if G else 0
            assert int(count(G, g)) == (want if want < 2 ** 64 else 2 ** 64 - 1), (G, g)
    assert all(int(count(G, g)) == len(slc.multisets(G, g)) for G, g in slc.FULL_SHAPES if G < 255)


def test_row_cases_put_the_edges_where_their_names_say():
    def ends(name):
        _, noise, counts, _ = slc.BY_NAME[name].matrix()
        perm, fast_end, mid_end = slc.device_rows(counts, noise)
        return fast_end, mid_end, counts[perm], noise[perm]

    for n in slc.LOGLIK_COUNT_1:
        fast_end, mid_end, counts, _ = ends(f"loglik_count_1_rows_{n}")
        assert fast_end == n and mid_end == n + 2 and len(counts) == n + 5 and slc.BY_NAME[f"loglik_count_1_rows_{n}"].G == 3
    for n in slc.MULTI_COUNT_1:
        fast_end, mid_end, counts, _ = ends(f"multi_count_1_rows_{n}")
        assert fast_end == n and mid_end == n + 2 and len(counts) == n + 5 and slc.BY_NAME[f"multi_count_1_rows_{n}"].G == 5
    # either side of a lane stride (64), of the four chains (192 | 256) and of a segment
    assert {64, 192, 256, slc.LOGLIK_SEGMENT} <= {n for n in slc.LOGLIK_COUNT_1} and slc.LOGLIK_SEGMENT == 7680
    assert all({e - 1, e, e + 1} <= set(slc.LOGLIK_COUNT_1) for e in (64, 192, 256, slc.LOGLIK_SEGMENT))
    assert all({e - 1, e, e + 1} <= set(slc.MULTI_COUNT_1) for e in (64, slc.MULTI_SEGMENT)) and slc.MULTI_SEGMENT == 1920
    assert 2 * slc.MULTI_SEGMENT + 1 in slc.MULTI_COUNT_1
    for c in range(2, slc.MID_MAX_COUNT + 1):
        for n in slc.MID_ROWS[1:]:
            fast_end, mid_end, counts, _ = ends(f"count_{c}_rows_{n}")
            assert mid_end - fast_end == n and set(counts[fast_end:mid_end]) == {float(c)} and fast_end == 5 and len(counts) == mid_end + 3
    fast_end, mid_end, counts, _ = ends("counts_2_to_8_rows_0")
    assert fast_end == mid_end == 5 < len(counts)
    fast_end, mid_end, counts, _ = ends("counts_8_and_9")
    assert set(counts[fast_end:mid_end]) == {8.0} and set(counts[mid_end:]) == {9.0} and counts[mid_end - 1] == 8 and counts[mid_end] == 9
    for n in slc.LOG_ROWS:      # either side of the two accumulators' stride: 64 | 128
        fast_end, mid_end, counts, _ = ends(f"log_rows_{n}")
        assert len(counts) - mid_end == n and (fast_end, mid_end) == (4, 6)
    assert all({e - 1, e, e + 1} <= set(slc.LOG_ROWS) for e in (64, 128))
    fast_end, mid_end, counts, noise = ends("only_log_rows_below_the_floor")
    assert fast_end == mid_end == 0 and np.all(noise == slc.SUB_FLOOR) and np.nextafter(slc.SUB_FLOOR, 1.0) == slc.FLOOR == 2.0 ** -30
    assert sorted(set(counts)) == [1.0, 8.0]      # counts that would be products at noise 2^-30
    fast_end, mid_end, counts, _ = ends("no_log_rows")
    assert 0 < fast_end < mid_end == len(counts)
    fast_end, mid_end, counts, _ = ends("no_count_1_rows")
    assert 0 == fast_end < mid_end < len(counts)
    assert ends("one_row")[:2] == (1, 1) and slc.BY_NAME["one_row"].R == 1
    assert ends("one_log_row")[:2] == (0, 0) and slc.BY_NAME["one_log_row"].R == 1
    assert ends("two_rows")[:2] == (1, 2) and slc.BY_NAME["two_rows"].R == 2
    for G in slc.CONDITIONAL_COLUMNS:
        assert slc.BY_NAME[f"columns_{G}"].G == G
    assert {G % slc.CANDIDATES for G in slc.CONDITIONAL_COLUMNS} == {0, 1, 2, 3} and 65 in slc.CONDITIONAL_COLUMNS
    assert max(c.R * c.G for c in slc.CASES) == slc.FOLD_BOUND_ROWS * 3 + 40 * 3


def test_fold_cases_multiply_the_most_factors_between_two_folds():
    """The loop of sumCountLogs restated: in a partial segment of 7 616 rows every lane has 29 rounds of four rows and three rows
    left, which all go to chain 0 — 32 factors between two folds, the most the loop allows for any class size; with columns 0 and
    1 zero there and noise exactly 2^-30 the product reaches 2^-960."""
    case = slc.BY_NAME["loglik_fold_bound"]
    M, noise, counts, _ = case.matrix()
    perm, fast_end, mid_end = slc.device_rows(counts, noise)
    assert fast_end == slc.FOLD_BOUND_ROWS == slc.LOGLIK_SEGMENT + 7616 and slc.loglik_chain_factors(fast_end) == slc.FOLD_FACTORS - 1 + 3 == 32
    assert max(slc.loglik_chain_factors(n) for n in list(range(0, 2 * slc.LOGLIK_SEGMENT + 2, 64)) + [7553, 7615, 7617, 7679, 7681]) == 32
    assert slc.loglik_chain_factors(slc.LOGLIK_SEGMENT) == slc.FOLD_FACTORS and 32 * 30 < 1022
    assert np.all(noise[perm[:fast_end]] == slc.FLOOR) and not np.any(M[perm[:fast_end]][:, [0, 1]]) and np.any(M[perm[:fast_end], 2] > 0)
    assert case.columns == (0, 1) and all(set(m) <= {0, 1, slc.NO_MEMBER} for w in slc.WIDTHS for m, _ in slc.loglik_requests(case, w))

    case = slc.BY_NAME["multi_fold_bound"]
    M, noise, counts, _ = case.matrix()
    perm, fast_end, mid_end = slc.device_rows(counts, noise)
    assert fast_end == slc.MULTI_SEGMENT and slc.multi_chain_factors(fast_end) == slc.FOLD_FACTORS
    assert max(slc.multi_chain_factors(n) for n in range(0, 4000)) == slc.FOLD_FACTORS
    assert np.all(noise[perm[:fast_end]] == slc.FLOOR) and not np.any(M[perm[:fast_end]])
    M, noise, counts, _ = slc.BY_NAME["multi_fold_run"].matrix()
    perm, fast_end, mid_end = slc.device_rows(counts, noise)
    assert fast_end == 2 * slc.MULTI_SEGMENT + 1 and np.all(noise[perm[:fast_end]] == slc.FLOOR) and not np.any(M[perm[:fast_end]])


@pytest.mark.parametrize("name,stride", [("loglik_fold_bound", 256), ("loglik_fold_bound", 64), ("multi_fold_run", 64)])
def test_a_product_that_is_not_folded_misses(name, stride):
    """(d) a product of 35 factors of 2^-30 has left the normal numbers (2^-1050) and the 36th makes it 0: a chain that is never
    folded — one per lane (stride 64) or four (stride 256) — gives minus infinity on the cases that name it, and still the right
    sum where a lane meets fewer than 35 rows."""
    case = slc.BY_NAME[name]
    assert ("fold_loglik" if name.startswith("loglik") else "fold_multi") in case.wrong
    ref = case.reference()
    M, noise, counts, _ = case.matrix()
    perm, fast_end, _ = slc.device_rows(counts, noise)
    outs = slc.outputs_of(case)
    assert 2.0 ** (-30 * 35) < np.finfo(np.float64).tiny and 2.0 ** (-30 * 36) == 0.0 and fast_end // stride > 35
    for j in (0, len(outs) - 1):
        members, g, rowmax = outs[j]
        x = slc._arguments(M, noise, members, g, rowmax, np.float64)[perm]
        wrong = slc.unfolded_sum(counts[perm], x, fast_end, stride)
        assert not abs(wrong - float(ref.model[j])) < slc.BITE * ref.tol
    small = slc.BY_NAME["loglik_count_1_rows_257"]
    M, noise, counts, _ = small.matrix()
    perm, fast_end, _ = slc.device_rows(counts, noise)
    members, g, rowmax = slc.outputs_of(small)[0]
    x = slc._arguments(M, noise, members, g, rowmax, np.float64)[perm]
    assert abs(slc.unfolded_sum(counts[perm], x, fast_end, stride) - float(small.reference().model[0])) <= small.reference().tol


def test_a_clamp_that_reads_the_last_column_for_a_live_candidate_misses():
    """(d) on every case that names it: the columns whose last block of four has more than one live candidate."""
    named = [c for c in SET_CASES if "clamp" in c.wrong]
    assert sorted(c.G for c in named) == [G for G in slc.CONDITIONAL_COLUMNS if (G - 1) % slc.CANDIDATES] == [2, 3, 4, 7, 8]
    for case in named:
        ref = case.reference()
        for w in slc.WIDTHS:
            for cond in ref.conditionals(case, w):
                wrong = slc.clamp_reads_last_column(cond)
                assert np.max(np.abs(wrong - cond)) >= slc.BITE * ref.tol, (case.name, w)
    for case in SET_CASES:      # (elsewhere the last block has one live candidate, column G - 1 itself: nothing to misread)
        if case.name.startswith("columns_") and "clamp" not in case.wrong:
            cond = case.reference().conditionals(case, 2)[0]
            assert np.array_equal(slc.clamp_reads_last_column(cond), cond)


def test_requests_are_the_ones_the_kernels_need():
    for case in SET_CASES:
        cols = set(case.columns if case.columns is not None else range(case.G))
        for w in slc.WIDTHS:
            reqs = slc.loglik_requests(case, w)
            members = [m for m, _ in reqs]
            assert all(len(m) == w for m in members) and {r for _, r in reqs} == {0, 1}
            assert any(len(set(m)) == 1 for m in members) and (members[0][::-1] in members)
            assert all(set(m) - {slc.NO_MEMBER} <= cols for m in members)
            slots = {m.index(slc.NO_MEMBER) for m in members if slc.NO_MEMBER in m}
            assert slots == ({0, w // 2, w - 1} if w in (2, 5, 8) else set())
            assert all(len(o) == w - 1 and set(o) <= cols for o in slc.conditional_requests(case, w))
    # the same members in two slot orders are two different sums only in the last bits
    case = slc.BY_NAME["columns_9"]
    ref = case.reference()
    got = ref.loglik(case, 5)
    assert abs(float(got[0] - got[1])) <= ref.tol and slc.loglik_requests(case, 5)[0][0] != slc.loglik_requests(case, 5)[1][0]


def test_the_batch_holds_the_matrices_of_the_cases():
    picked = [slc.BY_NAME[n] for n in ("columns_5", "multi_fold_bound", "multi_count_1_rows_1920", "only_log_rows_below_the_floor", "full_underflow", "one_row")]
    batch = slc.batch_of(picked)
    for k, case in enumerate(picked):
        cl = batch.cluster(k)
        M, noise, counts, mult = case.matrix()
        got, got_noise, got_counts = np_oracle.grouped_matrix(cl["rows"], [[p] for p in range(case.G)])
        assert np.array_equal(got, M) and np.array_equal(got_noise, noise) and np.array_equal(got_counts, counts)
        assert [p["source_count"] for p in cl["paths"]] == list(mult)
