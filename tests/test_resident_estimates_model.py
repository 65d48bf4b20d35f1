"""The plain-Python model of the resident-estimates gather (tests/resident_estimates_model.py) pinned to the hand case that
tests/cpp/estimates_gather_plan_check.cpp writes out for gatherModel, to the refusals in their reporting order, and to the Python
flattening of decoded estimates (FlatEstimates.from_estimates) on generated parts."""
import numpy as np
import pytest

from tests import resident_estimates_model as R


def test_hand_case_array_for_array():
    cluster_path_off, totals, parts, expected = R.hand_case()
    got = R.gather(cluster_path_off, totals, parts)
    assert sorted(got) == sorted(R.FLAT_NAMES)
    for name in R.FLAT_NAMES:
        assert got[name].tolist() == expected[name], name
    assert got["members"].dtype == np.uint32 and got["set_off"].dtype == np.uint64 and got["abundances"].dtype == np.float64
    assert [int(got["member_off"][int(s)]) for s in got["set_off"]] == got["abund_off"].tolist()


def test_no_part_and_no_cluster():
    cluster_path_off, totals, _, _ = R.hand_case()
    got = R.gather(cluster_path_off, totals, [])
    assert got["set_off"].tolist() == [0] * 5 and got["noise_count"].tolist() == totals and got["member_off"].tolist() == [0]
    got = R.gather([0], [], [])
    assert got["set_off"].tolist() == [0] and got["abund_off"].tolist() == [0] and got["noise_count"].size == 0


def _refusal(change):
    cluster_path_off, totals, parts, _ = R.hand_case()
    change(parts)
    with pytest.raises(R.Refused) as err:
        R.gather(cluster_path_off, totals, parts)
    return err.value.part, err.value.unit, err.value.why


def _set(part, name, index, value):
    def change(parts):
        parts[part][name][index] = value
    return change


def test_refusals_name_the_smallest_offender_and_its_first_offence():
    assert _refusal(_set(1, "unit_cluster", 0, 4)) == (1, 0, R.BAD_UNIT_CLUSTER)
    assert _refusal(_set(1, "unit_cluster", 0, 0)) == (0, 1, R.BAD_DUPLICATE)   # the first of the two units
    assert _refusal(_set(0, "subset_off", 1, 3)) == (0, 0, R.BAD_SUBSET_OFF)
    assert _refusal(_set(0, "subset_off", 2, 1)) == (0, 1, R.BAD_SUBSET_OFF)
    assert _refusal(_set(0, "path_off", 1, 6)) == (0, 0, R.BAD_PATH_OFF)
    assert _refusal(_set(1, "path_off", 0, 1)) == (1, 0, R.BAD_PATH_OFF)
    assert _refusal(_set(0, "set_count", 0, 6)) == (0, 0, R.BAD_SET_COUNT)
    assert _refusal(_set(0, "set_count", 1, 1)) == (0, 1, R.BAD_SET_COUNT)      # a unit without subsets has no slot
    assert _refusal(_set(1, "set_size", 1, 4)) == (1, 0, R.BAD_SET_SIZE)
    assert _refusal(_set(1, "set_size", 0, 0)) == (1, 0, R.BAD_SET_SIZE)
    assert _refusal(_set(0, "set_second", 1, 4)) == (0, 0, R.BAD_MEMBER)
    assert _refusal(_set(1, "set_member", (1, 1), 1)) == (1, 0, R.BAD_MEMBER)

    def two(parts):
        parts[1]["set_member"][1, 1] = 1
        parts[1]["set_size"][0] = 9      # a bad size anywhere in the unit comes before a bad member
    assert _refusal(two) == (1, 0, R.BAD_SET_SIZE)

    def two_units(parts):
        two(parts)
        parts[0]["set_first"][2] = 4
    assert _refusal(two_units) == (0, 0, R.BAD_MEMBER)

    def wide(parts):
        parts[1]["width"] = 9
    assert _refusal(wide) == (1, None, R.BAD_WIDTH)
    # what lies beyond set_count or beyond a set's size is not looked at
    cluster_path_off, totals, parts, expected = R.hand_case()
    parts[1]["set_size"][3] = 0
    parts[1]["set_member"][0, 1] = 7
    assert R.gather(cluster_path_off, totals, parts)["members"].tolist() == expected["members"]


def test_generated_parts_flatten_like_the_containers():
    """The model against the container route: the sets of every cluster as lists, flattened by FlatEstimates.from_estimates."""
    from types import SimpleNamespace

    from rpvg_amd.estimates_table import FlatEstimates
    rng = np.random.default_rng(5)
    path_counts = [3, 5, 2, 9, 4, 6, 1]
    cluster_path_off = np.concatenate([[0], np.cumsum(path_counts)]).astype(np.uint64)
    totals = [float(10 * (k + 1)) for k in range(len(path_counts))]
    parts = [R.make_part(rng, 0, [4, 0, 6], [5, 0, 2], path_counts, no_subsets=(1,)), R.make_part(rng, 3, [5, 1], [7, 3], path_counts),
             R.make_part(rng, 8, [3], [17], path_counts)]
    got = R.gather(cluster_path_off, totals, parts)
    estimates = []
    for k in range(len(path_counts)):
        e = SimpleNamespace(path_group_sets=[], posteriors=[], abundances=[], noise_count=totals[k])
        for part in parts:
            for u, c in enumerate(part["unit_cluster"]):
                if int(c) != k:
                    continue
                s0, s1 = int(part["subset_off"][u]), int(part["subset_off"][u + 1])
                first = int(part["path_off"][s0])
                for slot in range(first, first + int(part["set_count"][u])):
                    if part["width"] == 0:
                        n = 1 if int(part["set_second"][slot]) == R.NO else 2
                        e.path_group_sets.append([int(part["set_first"][slot]), int(part["set_second"][slot])][:n])
                    else:
                        n = int(part["set_size"][slot])
                        e.path_group_sets.append([int(x) for x in part["set_member"][slot, :n]])
                    e.posteriors.append(part["set_posterior"][slot])
                    e.abundances.extend(part["set_abundance"][slot, :n])
                if s1 > s0:
                    e.noise_count = part["cluster_noise_count"][u]
        estimates.append(e)
    batch = SimpleNamespace(cluster_path_off=cluster_path_off, path_effective_length=np.ones(int(cluster_path_off[-1])))
    want = FlatEstimates.from_estimates(batch, estimates)
    for name in R.FLAT_NAMES:
        assert got[name].tobytes() == getattr(want, name).tobytes(), name
    assert got["set_off"][-1] == 5 + 2 + 7 + 3 + 17 and len(set(np.diff(got["member_off"]).tolist())) == 8
