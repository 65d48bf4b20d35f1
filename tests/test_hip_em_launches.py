"""The merged EM launches of rpvg_hip_em_solve — the register bins and bin 0 in one launch of 64 threads, bins 7, 3 and 10 in one of
1 024 (planEmSolve, rpvg_amd/csrc/em_plan.hpp); bins 1 and 2 keep a launch each — against the same solve with
RPVG_HIP_EM_SEPARATE_LAUNCHES=1 (a launch per kernel variant, read per call): abundances, noise counts and iteration counts
bit-equal, the statistics' problems per slot what emBinOf assigns (tests/em_bin_cases.py restates it).

The problems are those of tests/em_bin_cases.py's builders, a few hundred rows at most.  What decides the plan of a solve is its
widest problem, so there are two sets:
  narrow   at most 1 000 columns: the wave launch with all six roles, bin 1, the 1 024-thread launch with bins 7 and 3
  wide     with problems of 1 174 and of 3 993 columns: bin 2 (a problem reaches it only from 1 174 columns on), and the
           1 024-thread launch with its third role, bin 10

Bin 10 keeps its vectors in global memory and adds into them with atomics in the order the wavefronts arrive (emSparseProblem):
two runs of ONE build differ in the last bits there, so its problems are compared as tests/test_hip_em_bins.py compares them
(iterations equal, values within 1e-12); every other bin bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import np_oracle, pyoracle
from rpvg_amd import hip
from tests import em_bin_cases as ebc, small_cases

pytestmark = pytest.mark.gpu

REL = 1e-7          # tests/test_hip_em_bins.py
MAX_ITS = 200       # one cap per call
SWITCH = "RPVG_HIP_EM_SEPARATE_LAUNCHES"
WAVE_BINS = (6, 4, 5, 8, 9, 0)


def _cases():
    """name -> case, bin by bin: two sizes of every register bin and of bin 0 (the fillers), and one or two of the others."""
    cases = {}
    for b in WAVE_BINS:
        fs = ebc.fillers(b)
        cases[f"b{b}_small"], cases[f"b{b}_large"] = fs[0], fs[-1]
    # 33 columns and 300 rows: 10 KB resident; 1 000 columns: the vectors of sixteen wavefronts are 133 KB — resident with 300
    # rows (146 KB), streamed with 450 (156 KB)
    cases["b1_a"] = ebc._case("launch_b1_a", 1, 9901, 32, 300, 300)
    cases["b1_b"] = ebc._case("launch_b1_b", 1, 9902, 32, 420, 500)
    cases["b7"] = ebc._case("launch_b7", 7, 9903, 999, 300, 600)
    cases["b3"] = ebc._case("launch_b3", 3, 9904, 999, 450, 900)
    cases["b3_p1172"] = ebc.BY_NAME["streamed_p1172"]
    cases["b2"] = ebc.BY_NAME["streamed_p1173"]
    cases["b10"] = ebc.BY_NAME["streamed_p3992"]
    return cases


CASES = _cases()
NARROW = [n for n in CASES if n not in ("b3_p1172", "b2", "b10")]
WIDE = list(CASES)
NAMES = list(CASES)


def test_cases_are_in_their_bins_and_in_their_sets():
    for name, c in CASES.items():
        assert ebc.em_bin(*c.shape()) == c.bin, (name, c.shape())
        assert c.shape()[1] <= 450
    assert {CASES[n].bin for n in NARROW} == set(WAVE_BINS) | {1, 7, 3}
    assert max(CASES[n].shape()[0] for n in NARROW) < 3993       # two roles in the 1 024-thread launch
    assert {CASES[n].bin for n in WIDE} == set(WAVE_BINS) | {1, 2, 7, 3, 10}


def _batch(names):
    return ebc.batch_of([CASES[n].cluster() for n in names])


@pytest.fixture(scope="module")
def dev(hip_ctx):
    d = hip_ctx.upload(_batch(NAMES))
    yield d
    d.free()


class _StreamsContext(hip.Context):
    """A context with `side_streams` real side streams (rpvg_hip_create_with_streams: the contexts of the batch pipeline have 3)."""

    def __init__(self, side_streams):
        self.handle = C.c_void_p()
        hip._check(hip.lib().rpvg_hip_create_with_streams(C.c_int(0), C.c_int(side_streams), C.byref(self.handle)), "rpvg_hip_create_with_streams")


def _slot_problems(stats):
    return {i: int(stats["em_kernel"][hip.em_kernel_name(i)]["problems"]) for i in range(hip.EM_KERNELS)}


def _solve(ctx, dev, names, index):
    return ctx.em_solve(dev, [index[n] for n in names], [CASES[n].cols() for n in names], max_em_its=MAX_ITS)


def _both(ctx, dev, names, monkeypatch, index=None):
    """The call with merged launches and with a launch per variant; the merged one's statistics."""
    index = index or {n: i for i, n in enumerate(NAMES)}
    monkeypatch.delenv(SWITCH, raising=False)
    ctx.reset_stats()
    merged = _solve(ctx, dev, names, index)
    stats = ctx.stats()
    monkeypatch.setenv(SWITCH, "1")
    ctx.reset_stats()
    separate = _solve(ctx, dev, names, index)
    separate_stats = ctx.stats()
    monkeypatch.delenv(SWITCH)
    return merged, separate, stats, separate_stats


def _assert_same(names, x, y):
    for j, n in enumerate(names):
        if CASES[n].bin == 10:   # (global atomics: see the module's text)
            assert small_cases.rel_close(x[0][j], y[0][j], rel=1e-12, floor=1e-300), n
            assert abs(x[1][j] - y[1][j]) <= 1e-12 * max(1.0, x[2][j]), n
        else:
            assert np.array_equal(x[0][j], y[0][j]), n
            assert x[1][j] == y[1][j], n
        assert x[2][j] == y[2][j] and x[3][j] == y[3][j], n
    if not any(CASES[n].bin == 10 for n in names):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[3], y[3])


def _assert_slots(names, stats):
    want, _ = ebc.expected_stats([CASES[n].shape() for n in names])
    assert _slot_problems(stats) == {i: want.get(i, 0) for i in range(hip.EM_KERNELS)}


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        c = CASES[name]
        P, noise, counts = np_oracle.dense_matrix(c.cluster().rows(), c.cluster().n_paths, c.cols())
        ab, nc, tot, its, _ = pyoracle.em_dense(np_oracle.add_noise_and_normalize(P, noise), counts, MAX_ITS)
        _ORACLE[name] = (ab, nc, tot, its)
    return _ORACLE[name]


@pytest.mark.parametrize("names", [NARROW, WIDE], ids=["narrow", "wide"])
def test_every_role_populated_at_once(hip_ctx, dev, monkeypatch, names):
    """(a) every bin of every launch of the plan has problems, three of each in a shuffled order; also against the oracle."""
    order = [names[j] for j in np.random.default_rng(5).permutation(len(names) * 3) % len(names)]
    merged, separate, stats, separate_stats = _both(hip_ctx, dev, order, monkeypatch)
    _assert_same(order, merged, separate)
    _assert_slots(order, stats)
    _assert_slots(order, separate_stats)
    # the switch is what it says: bin 0's own launch has a device time of its own, the wave launch's goes to the register slot
    name0, name_reg = hip.em_kernel_name(0), hip.em_kernel_name(ebc.REGISTER_SLOT)
    assert stats["em_kernel"][name0]["ms"] == 0 and stats["em_kernel"][name_reg]["ms"] > 0
    assert separate_stats["em_kernel"][name0]["ms"] > 0
    for j, n in enumerate(order):
        want_ab, want_nz, want_tot, want_its = _oracle(n)
        assert merged[2][j] == want_tot and int(merged[3][j]) == want_its, n
        assert small_cases.rel_close(merged[0][j], want_ab, rel=REL), n
        assert abs(merged[1][j] - want_nz) <= REL * max(1.0, want_tot), n


SINGLE_ROLES = [("wave-16", ["b6_large", "b6_small"]), ("wave-16", ["b4_large", "b4_small"]), ("wave-16", ["b5_large", "b5_small"]),
                ("wave-32", ["b8_large", "b8_small"]), ("wave-32", ["b9_large", "b9_small"]), ("wave-32", ["b0_large", "b0_small"]),
                ("256", ["b1_a", "b1_b"]), ("1024", ["b7"]), ("1024", ["b3"]), ("1024-p1172", ["b3_p1172"]), ("1024-wide", ["b10"]),
                ("256-own", ["b2"])]


@pytest.mark.parametrize("launch,names", SINGLE_ROLES, ids=[f"{l}:bin{CASES[n[0]].bin}" for l, n in SINGLE_ROLES])
def test_one_role_populated_the_others_empty(hip_ctx, dev, monkeypatch, launch, names):
    """(b) a call whose problems are all of one bin: the workgroups of every other role of its launch, and of the other
    launches, find their bins empty and fall through the guard.  Register bins 4 to 6 alone: the wave launch has four roles, else
    six.  "256", "256-own": bins 1 and 2, a launch each, next to the merged launches with every role empty.  "1024-wide": the third role
    of the 1 024-thread launch alone — the plan of a call follows its widest problem, and a problem that gives the launch its
    third role is one of bin 10, so bins 7 and 3 alone under three roles cannot be built."""
    call = names * 2
    merged, separate, stats, _ = _both(hip_ctx, dev, call, monkeypatch)
    _assert_same(call, merged, separate)
    _assert_slots(call, stats)
    slot = ebc.REGISTER_SLOT if CASES[names[0]].bin in ebc.REGISTER_BINS else CASES[names[0]].bin
    assert _slot_problems(stats)[slot] == len(call)


def test_more_problems_than_workgroups_in_every_role(hip_ctx, dev, monkeypatch):
    """(c) every role of the narrow set's launches gets more problems than it has workgroups — two per CU, one for the 1 024
    threads — so every persistent workgroup draws again from its own bin's cursor, a large problem first and smaller ones behind
    it in the same LDS.  (Problems of a call may share a cluster: nothing more is uploaded.)"""
    _, cus, _ = hip_ctx.info()
    call = []
    for b in WAVE_BINS:
        call += [f"b{b}_small", f"b{b}_large"] * (cus + 8)
    call += ["b1_a", "b1_b"] * (cus + 8)
    call += ["b7"] * (cus + 8) + ["b3"] * (cus + 8)
    call = [call[j] for j in np.random.default_rng(6).permutation(len(call))]
    bins = [CASES[n].bin for n in call]
    assert all(bins.count(b) > 2 * cus for b in WAVE_BINS + (1,)) and all(bins.count(b) > cus for b in (7, 3))
    merged, separate, stats, _ = _both(hip_ctx, dev, call, monkeypatch)
    _assert_same(call, merged, separate)
    _assert_slots(call, stats)
    # every copy of a problem has the result of the first
    first = {}
    for j, n in enumerate(call):
        k = first.setdefault(n, j)
        assert np.array_equal(merged[0][j], merged[0][k]) and merged[1][j] == merged[1][k] and merged[3][j] == merged[3][k], n


@pytest.mark.parametrize("side_streams", [3, 6])
def test_contexts_of_three_and_of_six_side_streams(hip_ctx, dev, monkeypatch, side_streams):
    """(d) with three side streams every launch of a side stream has one of its own (bin 2's is on the main stream); with six as well.  Both
    against the separate launches on the same context (three side streams: chains of two) and against the session's context."""
    order = [NARROW[j] for j in np.random.default_rng(7).permutation(len(NARROW) * 2) % len(NARROW)]
    monkeypatch.delenv(SWITCH, raising=False)
    want = _solve(hip_ctx, dev, order, {n: i for i, n in enumerate(NAMES)})
    ctx = _StreamsContext(side_streams)
    try:
        own = ctx.upload(_batch(NARROW))
        try:
            merged, separate, stats, _ = _both(ctx, own, order, monkeypatch, index={n: i for i, n in enumerate(NARROW)})
        finally:
            own.free()
    finally:
        ctx.close()
    _assert_same(order, merged, separate)
    _assert_same(order, merged, want)
    _assert_slots(order, stats)
