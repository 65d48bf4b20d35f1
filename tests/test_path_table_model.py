"""The plain-Python model of the path table (tests/path_table_model.py) pinned to a case written out by hand from the
reference's lines, the conditions the cases of tests/test_hip_path_table.py rest on, and the host side of the table
(rpvg_amd/host/path_table.cpp) under the sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import align_index_model as IM
from tests import path_table_model as M


def test_hand_case_names_a_b_a_c_b():
    """src/main.cpp:853-887: emplace(name, size) over the paths in order numbers a name at its first appearance;
    :909-951: the first member brings name and group_id, counts and length * count add up, round() and the division close."""
    clusters, table, groups, collapsed = M.hand_case()
    path_group, cluster_group_off = M.name_groups(clusters, table["name_id"])
    assert path_group == groups == [0, 1, 0, 2, 1] and cluster_group_off == [0, 3]
    assert M.collapsed_paths(clusters, table) == [collapsed]


def test_round_is_half_away_from_zero():
    """:946 `round(path.length / double(source_count))` is C's round."""
    assert [M.c_round(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 3.5, 2.4999999999999996)] == [0, 0, 1, 2, 3, 4, 2]
    t = M.make_table(2, name_id=[5, 5], length=[1, 2], source_count=[1, 1])
    assert M.collapsed_paths([[0, 1]], t)[0][0]["length"] == 2          # 1.5 -> 2
    t = M.make_table(2, name_id=[5, 5], length=[2, 3], source_count=[1, 1])
    assert M.collapsed_paths([[0, 1]], t)[0][0]["length"] == 3          # 2.5 -> 3 (half-even would give 2)
    t = M.make_table(3, name_id=[5, 5, 5], length=[2, 3, 4], source_count=[1, 2, 1])
    assert M.collapsed_paths([[0, 1, 2]], t)[0][0]["length"] == 3       # 12 / 4


def test_same_name_in_two_clusters_makes_two_groups_and_ids_do_not_order_groups():
    names = [9, 4, 9, 4, 1, 9]
    path_group, off = M.name_groups([[0, 1, 2], [3, 4, 5]], names)
    assert path_group == [0, 1, 0, 0, 1, 2] and off == [0, 2, 5]
    descending = [50, 40, 40, 30, 50, 10]
    assert M.name_groups([list(range(6))], descending)[0] == [0, 1, 1, 2, 0, 3]


def test_three_sums_of_the_recorded_triple_differ():
    eff, counts = M.THREE_SUM_TRIPLE
    assert eff == (3443.520070245456, 4568.900641887635, 852.3741444655479) and counts == (418, 633, 776)
    sums = (M.sequential_sum(eff, counts), M.reversed_sum(eff, counts), M.fused_sum(eff, counts))
    assert len(set(sums)) == 3
    # the model's collapsed effective length is the sequential, unfused sum over the total count
    t = M.make_table(3, name_id=[1, 1, 1], effective_length=eff, source_count=counts)
    assert M.collapsed_paths([[0, 1, 2]], t)[0][0]["effective_length"] == sums[0] / float(sum(counts))


def test_random_triples_tell_the_sums_apart():
    """Any two of the three sums differ for about a quarter of random triples (effective lengths 50 .. 8000, counts below 900).
    All three differ at once for far fewer, about one triple in 250: sums that differ do so by one unit in the last place, so three
    different values need the two differences to point in opposite directions or one of them to be two units.  (The figure of a
    quarter for the three-way condition does not hold for this distribution; 8 of these 2 000 triples qualify.)  The cases of the
    device test are therefore searched for, and every one has three different sums and a group of three members."""
    triples = M.random_triples(5, 2000)
    sums = [(M.sequential_sum(*t), M.reversed_sum(*t), M.fused_sum(*t)) for t in triples]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        share = sum(s[i] != s[j] for s in sums) / len(sums)
        print("share of random triples whose sums", i, j, "differ:", share)
        assert 0.15 < share < 0.35
    all_three = sum(len(set(s)) == 3 for s in sums)
    print("triples with three different sums:", all_three, "of", len(sums))
    # a binomial count with mean 8: between 2 and 20 in all but one draw in ten thousand
    assert 2 <= all_three <= 20
    cases = M.three_sum_cases(90, 40)
    assert len(cases) == 40 and cases[0] == M.THREE_SUM_TRIPLE and all(len(e) >= 3 and M.three_sums_differ(e, c) for e, c in cases)


def test_first_appearance_cases_are_not_monotone():
    rng = np.random.default_rng(3)
    for n, names in ((3, 2), (5, 3), (63, 9), (64, 64), (65, 20), (700, 7)):
        ids = M.non_monotone_names(rng, n, names)
        assert len(ids) == n and not M.is_monotone(ids)
        groups = M.name_groups([list(range(n))], ids)[0]
        seen = []
        for g in groups:  # groups are numbered 0, 1, 2 ... at their first appearance
            if g not in seen:
                assert g == len(seen)
                seen.append(g)
    assert M.is_monotone([3, 3, 5]) and M.is_monotone([7, 2, 2]) and not M.is_monotone([1, 3, 2])


def test_refused_groups():
    t = M.make_table(3, name_id=[1, 2, 1], source_count=[4, 0, 4])
    with pytest.raises(M.InvalidGroup) as err:
        M.collapsed_paths([[0, 1, 2]], t)
    assert (err.value.cluster, err.value.group) == (0, 1) and M.first_invalid_group([[0, 1, 2]], t) == (0, 1)
    t = M.make_table(4, name_id=[1, 2, 2, 3], source_count=[1, 0xffffffff, 1, 1])
    with pytest.raises(M.InvalidGroup) as err:
        M.collapsed_paths([[0], [1, 2, 3]], t)
    assert (err.value.cluster, err.value.group) == (1, 0) and M.first_invalid_group([[0], [1, 2, 3]], t) == (1, 0)
    t = M.make_table(2, name_id=[2, 2], source_count=[0xffffffff - 1, 1])   # the largest sum that fits
    assert M.collapsed_paths([[0, 1]], t)[0][0]["source_count"] == 0xffffffff


def test_path_side_follows_the_clusters_of_the_index_model():
    params, lists = IM.hand_case()
    index = IM.run_model(params, [lists])
    clusters = M.cluster_lists(index["arrays"])
    assert sorted(p for c in clusters for p in c) == list(range(6))
    sources = [[p, p + 10] if p % 2 else [] for p in range(6)]
    t = M.make_table(6, source_ids=sources, group_id=[10 * p for p in range(6)])
    group_id, off, ids = M.path_side(clusters, t)
    order = [p for c in clusters for p in c]
    assert group_id == [10 * p for p in order] and off[-1] == len(ids) == 6
    assert [ids[off[i]:off[i + 1]] for i in range(6)] == [sources[p] for p in order]
    assert M.path_side(clusters, M.make_table(6))[1:] == (None, None)


def test_host_table_under_the_sanitizers():
    """tests/cpp/path_table_check.cpp: PathTable::fromPathInfos and the unflattening of the groups view (rpvg_amd/host/path_table.cpp,
    which needs no engine), as a program of its own built with AddressSanitizer and UBSan."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "path_table_check")
    host = os.path.join(root, "rpvg_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + host,  # the runtimes inside the program: no order of libraries to keep
                           os.path.join(root, "tests", "cpp", "path_table_check.cpp"), os.path.join(host, "path_table.cpp"), "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
