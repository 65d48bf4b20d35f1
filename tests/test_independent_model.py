"""The plain-Python model of the independent one-call route (tests/independent_model.py) pinned to the standard's check value and to a
hand-written cluster, and the host side of the call — the plan (rpvg_amd/csrc/subset_independent_plan.hpp) and the distribution
and draw of rpvg_amd/csrc/gibbs_streams.hpp against libstdc++ — as programs of their own under AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

import pytest

from tests import independent_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_check_value():
    """[rand.predef]: the 10 000th consecutive invocation of a default-constructed mt19937 produces 4123659995."""
    rng = model.Mt19937()
    rng.discard(9999)
    assert rng() == 4123659995
    assert rng.taken == 10000
    # next_words leaves the generator where it is; the state words are the untempered last 624 outputs
    ahead = rng.next_words(3)
    assert [rng(), rng(), rng()] == ahead
    again = model.Mt19937()
    again.x, again.p = rng.state_before_next(), model.N  # (as seeding from a sequence that hands these out)
    assert again.next_words(700) == rng.next_words(700)


def test_distribution_construction():
    assert model.partial_sums([]) is None and model.partial_sums([1.0]) is None
    assert model.partial_sums([0.25, 0.75]) == [0.25, 1.0]
    total = ((0.1 + 0.2) + 0.3) + 0.4
    assert model.partial_sums([0.1, 0.2, 0.3, 0.4]) == [0.1 / total, 0.1 / total + 0.2 / total, (0.1 / total + 0.2 / total) + 0.3 / total, 1.0]
    # trailing zeros (the late losers of the bounded search): the partial sums stay where they are, the last one is 1.0
    cp = model.partial_sums([0.5, 0.5, 0.0, 0.0])
    assert cp == [0.5, 1.0, 1.0, 1.0]
    rng = model.Mt19937(1)
    assert set(model.draw_sets([0.5, 0.5, 0.0, 0.0], 200, rng)) == {0, 1} and rng.taken == 400
    rng = model.Mt19937(1)
    assert model.draw_sets([1.0], 200, rng) == [0] * 200 and rng.taken == 0


def test_weights_are_chains_of_additions():
    assert model.num_samples(0.5) == 2 and model.num_samples(1 / 312) == 312 and model.num_samples(1 / 313) == 313
    assert model.num_samples(0.001) == 1000 and model.num_samples(1 / 1024) == 1024
    assert model.weight_of(1000, 1000) == 1.0000000000000007
    assert model.weight_of(3, 4) == 0.75 and model.weight_of(0, 4) == 0.0


def test_hand_written_cluster():
    """Two transcripts at group size 2, min_hap_prob 0.25 (four samples), std::mt19937(4).  Transcript 0 has the paths 0 and 2 and
    the sets {0,0} {0,1} {1,1} with posteriors 0.5 0.25 0.25; transcript 1 the paths 1 and 3 and the sets {0,0} {0,1} at 0.5 each.
    libstdc++ draws 2 0 2 1 for the first and then 1 0 0 1 for the second, and the generator's next output is 1086550967."""
    rng = model.Mt19937(4)
    transcripts = [([0, 2], [(0, 0), (0, 1), (1, 1)], [0.5, 0.25, 0.25]), ([1, 3], [(0, 0), (0, 1)], [0.5, 0.5])]
    draws, subsets = model.cluster(transcripts, 0.25, rng)
    assert draws == [[2, 1], [0, 0], [2, 0], [1, 1]]
    assert rng.taken == 16
    assert rng() == 1086550967
    # slot 0: 2 2 + 1 3; slot 1: 0 0 + 1 1; slot 2: 2 2 + 1 1; slot 3: 0 2 + 1 3 — the transcripts' paths interleave
    assert subsets == [([0, 0, 1, 1], 0.25, 1), ([0, 1, 2, 3], 0.25, 1), ([1, 1, 2, 2], 0.25, 1), ([1, 2, 2, 3], 0.25, 1)]
    # seed 7 draws 0 0 2 0 and 0 0 0 0: three samples are one subset, whose weight is (0.25 + 0.25) + 0.25
    rng = model.Mt19937(7)
    draws, subsets = model.cluster(transcripts, 0.25, rng)
    assert draws == [[0, 0], [0, 0], [2, 0], [0, 0]]
    assert subsets == [([0, 0, 1, 1], 0.75, 3), ([1, 1, 2, 2], 0.25, 1)]
    assert rng() == 1152936666
    # a transcript of one set draws nothing: the second one starts at word 0
    rng = model.Mt19937(4)
    draws, subsets = model.cluster([([4], [(0, 0)], [1.0])] + transcripts[:1], 0.25, rng)
    assert draws == [[0, 2], [0, 0], [0, 2], [0, 1]] and rng.taken == 8
    assert subsets == [([0, 0, 4, 4], 0.25, 1), ([0, 2, 4, 4], 0.25, 1), ([2, 2, 4, 4], 0.5, 2)]


def _build_and_run(name, include):
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I" + include, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"


def test_plan_under_the_sanitizers():
    """tests/cpp/subset_independent_plan_check.cpp: S for min_hap_prob 0.5, 1/312, 1/313, 0.001 and 1/1024, the weight table against a
    literal loop, word counts and capacities either side of a block of 624 words, every host-side refusal."""
    _build_and_run("subset_independent_plan_check", os.path.join(ROOT, "rpvg_amd", "csrc"))


def test_distribution_and_draw_against_libstdcxx_under_the_sanitizers():
    """tests/cpp/independent_draws_check.cpp: the header's distribution and draw against std::discrete_distribution<uint32_t> on a
    std::mt19937 — one weight, two, trailing zeros, a zero in the middle, 65 536 weights, 300 decades; indices and generator positions."""
    _build_and_run("independent_draws_check", os.path.join(ROOT, "rpvg_amd", "csrc"))


def test_the_binding_mirrors_the_header():
    from rpvg_amd import hip
    for name in ("rpvg_hip_nested_independent_subset_em", "rpvg_hip_subset_em_get_independent", "rpvg_hip_independent_draws_get",
                 "rpvg_hip_independent_limits", "rpvg_hip_independent_stats_get"):
        assert name in hip.EXPORTS
    assert [n for n, _ in hip.CSubsetEmIndependentView._fields_][:3] == ["num_clusters", "group_size", "num_samples"]
    assert [n for n, _ in hip.CSubsetEmIndependentView._fields_][-3:] == ["sample_count", "words_consumed", "generator_state"]
    assert [n for n, _ in hip.CIndependentStats._fields_] == ["calls_completed", "draws", "subsets"]
    # the existing stats struct is untouched
    assert [n for n, _ in hip.CKernelStats._fields_][-3:] == ["nested_full_calls", "nested_full_sets", "nested_full_retained"]
    if os.path.exists(hip.LIB_PATH):
        limits = hip.independent_limits()
        assert (limits.max_group_size, limits.max_samples, limits.max_transcript_sets, limits.words_per_draw, limits.state_words) == (8, 1024, 65536, 2, 624)
