"""The samplers' own conditional kernels draw for draw at their shapes: rpvg_hip_group_gibbs (group sizes 1 and 2) and
rpvg_hip_group_gibbs_polyploid (group size 3) on problems that reach the numbers of gibbsConditionalTileKernel (64 candidate
columns x 64 staged rows), gibbsConditionalKernel (turns of 8 | 4 | 2 | 1 work items, set by 256 | 512 | 1 024 rows),
gibbsDistributionKernel (stretches of ceil(G / 64) columns per lane) and the collect kernel (kRankInLds = 2 048 sets ordered by
first appearance in LDS).

Nothing here comes from the device: the sequential Python model of the reference's sampler (_gibbs_model of
tests/test_hip_kernels.py) takes its conditionals from the long-double model of tests/set_loglik_cases.py rounded to FP64, plus
the log frequencies — the expected sets, counts and words are known before the GPU runs.  The device forms the log-sum-exp as
max + log sum and the partial sums by lane stretches, so its partial sums differ from the model's chain in the last bits, and its
conditionals from the model's by at most the tolerances of tests/test_hip_set_loglik.py, about 1e-12; every draw of the model
therefore keeps a relative distance of at least 1e-9 from every partial sum — three orders above both —, asserted before the
sampler is called.  The seeds were chosen to meet it; no draw is skipped.
"""
import bisect

import numpy as np
import pytest

from tests import set_loglik_cases as slc
from tests.test_hip_kernels import _gibbs_model, _mt19937_words, _mt_temper

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
RANK_IN_LDS = 2048      # kRankInLds (gibbs_chains.hip)


class _Problem:
    """What slc.batch_of asks of a case."""
    def __init__(self, name, G, R, seed, peak=None, flat=False):
        self.name, self.G, self.R = name, G, R
        rng = np.random.default_rng(seed)
        M, noise, counts = slc.draw_rows(rng, G, (("mix", R),))
        if flat:      # every cell there and within a few per cent of its neighbours': no column stands out
            M = (1.0 - noise)[:, None] / G * rng.uniform(0.97, 1.03, size=(R, G))
        if peak is not None:
            M[:, peak[0]] = np.maximum(M[:, peak[0]], (1.0 - noise) / G) * peak[1]
        self._matrix = (M, noise, counts, np.ones(G, dtype=np.uint32))
        self.log_freq = np.log(rng.integers(1, 5, size=G) / 7.0)

    def matrix(self):
        return self._matrix

    def conditional(self, group_size, ascending):
        """others -> log-likelihood + log frequency of every candidate column: the long-double model rounded to FP64."""
        M, noise, counts, _ = self._matrix
        cache = {}

        def conditional(others):
            handed = tuple(sorted(others)) if ascending else tuple(others)
            if handed not in cache:
                ll = slc.conditionals_model(M, noise, counts, handed, group_size).astype(np.float64)
                cache[handed] = [float(x) + float(y) for x, y in zip(ll, self.log_freq)]
            return cache[handed]
        return conditional


def _margin(draws):
    """The smallest relative distance of a draw's u from a partial sum of its distribution."""
    smallest = np.inf
    arrays = {}
    for cp, u in draws:
        if id(cp) not in arrays:
            arrays[id(cp)] = (cp, np.array(cp))
        a = arrays[id(cp)][1]
        k = bisect.bisect_left(cp, u)
        for c in a[max(0, k - 1):k + 1]:
            smallest = min(smallest, abs(u - c) / max(u, c))
    return smallest


def _expect(problems, group_size, generator_problems, seeds, slot_order_too=False):
    """The model over every generator's stream: per problem (sets in order of first appearance, counts), the words every generator
    gives, the streams, the (chains, burn, its) of every problem and the smallest margin of any draw."""
    want, want_words, streams, shapes, margin = {}, [], [], {}, np.inf
    for members, (seed, skip) in zip(generator_problems, seeds):
        words = _mt19937_words(seed, skip, 200000)
        taken = 0
        for m in members:
            draws = []
            order, counts, used, shape = _gibbs_model(problems[m].G, group_size, problems[m].conditional(group_size, True), words[taken:], draws)
            if slot_order_too:      # the others in slot order (the reference) and ascending (the device) give the same draws
                assert _gibbs_model(problems[m].G, group_size, problems[m].conditional(group_size, False), words[taken:]) == (order, counts, used, shape)
            margin = min(margin, _margin(draws))
            want[m], shapes[m] = (order, counts), shape
            taken += used
        assert taken + 624 <= len(words)
        want_words.append(taken)
        streams.append(words)
    return want, want_words, streams, shapes, margin


def _run_and_compare(hip_ctx, problems, group_size, generator_problems, entry, expected):
    want, want_words, streams, shapes, margin = expected
    assert margin >= MARGIN, f"a draw of the model lies within {margin:.1e} of a partial sum: another seed"
    dev = hip_ctx.upload(slc.batch_of(problems))
    try:
        mats = list(range(len(problems)))
        dg = hip_ctx.groups(dev, mats, [[[p] for p in range(pr.G)] for pr in problems], False)
        try:
            def run():
                return getattr(dg, entry)(mats, group_size, [shapes[m][0] for m in mats], [shapes[m][1] for m in mats], [shapes[m][2] for m in mats],
                                          [pr.log_freq for pr in problems], generator_problems, [s[:624] for s in streams])
            got, words_consumed, state, (rounds, conditionals) = run()
            again = run()
        finally:
            dg.free()
    finally:
        dev.free()
    assert [int(w) for w in words_consumed] == want_words
    for m in mats:
        where = f"problem {m} ({problems[m].name}: {problems[m].G} columns, {problems[m].R} rows)"
        assert got[m][0] == want[m][0], f"sets of {where}"
        assert got[m][1] == want[m][1], f"counts of {where}"
        assert sum(got[m][1]) == shapes[m][0] * shapes[m][2]
    for g, taken in enumerate(want_words):
        assert taken >= 624 and [_mt_temper(int(x)) for x in state[g]] == streams[g][taken - 624:taken]
    assert again[0] == got and np.array_equal(again[1], words_consumed) and np.array_equal(again[2], state)
    print(f"{entry} at group size {group_size}: {len(problems)} problems, {sum(len(want[m][0]) for m in mats)} sets, {rounds} rounds, "
          f"{conditionals} conditionals, smallest margin {margin:.1e}")


# (columns, rows): the tile kernel's 64 candidates and 64 staged rows and one more of each; stretches of 1 | 2 | 3 columns per lane
# (64 | 65 .. 128 | 129); turns of 8 | 4 | 2 | 1 items (rows up to 256 | 512 | 1 024 | more)
SHAPES = ((64, 64), (65, 65), (128, 257), (129, 513), (66, 1025))
SEEDS = {1: [(31, 0), (32, 623), (33, 624), (34, 0), (35, 623), (36, 624)], 2: [(41, 0), (42, 623), (43, 624), (44, 0), (45, 623), (46, 624)]}


@pytest.mark.parametrize("group_size", [1, 2])
def test_sampler_follows_the_model_at_the_shapes_of_its_kernels(hip_ctx, group_size):
    problems = [_Problem(f"shape_{G}x{R}", G, R, 71000 + G + R) for G, R in SHAPES]
    problems.append(_Problem("peaked_70x300", 70, 300, 71900, peak=(37, 1.6)))
    problems.append(_Problem("flat_96x2", 96, 2, 71901, flat=True))
    assert [(-(-p.G // 64)) for p in problems[:5]] == [1, 2, 2, 3, 2] and [p.R > 256 for p in problems[:5]] == [False, False, True, True, True]
    generator_problems = [[0], [1, 2], [3], [4], [5], [6]]      # one generator serves two problems
    expected = _expect(problems, group_size, generator_problems, SEEDS[group_size])
    want = expected[0]
    # the chains of the peaked problem sit on the mode; those of the flat one draw off it all the time
    assert max(want[5][1]) > 0.9 * sum(want[5][1]) and set(want[5][0][int(np.argmax(want[5][1]))]) == {37}
    assert len(want[6][0]) > (40 if group_size == 1 else 400) and max(want[6][1]) < 0.1 * sum(want[6][1])
    _run_and_compare(hip_ctx, problems, group_size, generator_problems, "gibbs", expected)


def test_sets_come_in_order_of_first_appearance_either_side_of_the_lds_ranking(hip_ctx):
    """Two flat problems of about 400 columns at group size 2: the model samples fewer than 2 048 distinct sets for one (its
    weight lies on 40 columns: the log frequencies of the others are log 1e-7) and more for the other — the order of first appearance is formed in LDS for one and not for the
    other, and must be the same order either way."""
    narrow = _Problem("flat_390x2_over_40_columns", 390, 2, 72001, flat=True)
    narrow.log_freq[40:] = np.log(1e-7)
    problems = [_Problem("flat_400x2", 400, 2, 72000, flat=True), narrow]
    generator_problems, seeds = [[0], [1]], [(51, 624), (52, 0)]
    expected = _expect(problems, 2, generator_problems, seeds)
    want = expected[0]
    assert len(want[0][0]) > RANK_IN_LDS > len(want[1][0]) > 500, (len(want[0][0]), len(want[1][0]))
    _run_and_compare(hip_ctx, problems, 2, generator_problems, "gibbs", expected)


def test_polyploid_sampler_follows_the_model_at_the_shapes_of_its_kernels(hip_ctx):
    problems = [_Problem("shape_65x65", 65, 65, 73065, peak=(11, 1.15)), _Problem("shape_129x513", 129, 513, 73129)]
    generator_problems, seeds = [[0, 1]], [(61, 623)]
    expected = _expect(problems, 3, generator_problems, seeds, slot_order_too=True)
    _run_and_compare(hip_ctx, problems, 3, generator_problems, "gibbs_polyploid", expected)
