"""The Python model of the alignment-path index (tests/align_index_model.py) — what tests/test_hip_align_index.py holds the device
to — against one case worked out by hand from the reference's lines, and against itself under re-chunking.  No GPU."""
import os
import subprocess

import numpy as np

from tests import align_index_model as M


def test_model_equals_the_case_written_out_by_hand():
    params, lists = M.hand_case()
    got = M.run_model(params, [lists])
    # src/main.cpp:213-216: lists 0, 2 and 4 are counted, at their ORIGINAL lengths 7, 9 and 10 (mapq 29 and !is_simple are not)
    want_counts = np.zeros(11, dtype=np.uint32)
    want_counts[[7, 9, 10]] = 1
    assert np.array_equal(got["frag_counts"], want_counts)
    assert (got["num_lists"], got["num_distinct"], got["num_clusters"]) == (6, 4, 4)
    # PathClusters: {0, 1} (list 1), {2}, {3} (no list), {4, 5}: numbered by ascending smallest id
    assert got["clusters"] == [[0, 1], [2], [3], [4, 5]]
    # :811-827: (lists, index) descending = (2, 3), (1, 1), (1, 0), (0, 2)
    want = dict(
        rank_cluster=[3, 1, 0, 2],
        path_to_cluster=[0, 0, 1, 2, 3, 3],
        cluster_paths=[4, 5, 2, 0, 1, 3],
        cluster_path_off=[0, 2, 3, 5, 6],
        cluster_read_off=[0, 2, 3, 4, 4],
        # cluster {4, 5}: list 0 (twice, with list 2) then list 3; cluster {2}: list 4; cluster {0, 1}: list 1 (twice, with list 5)
        first_occurrence=[0, 3, 4, 1],
        read_count=[2, 1, 1, 2],
        read_min_mapq=[40, 40, 60, 29],
        read_noise_score=[-3, -3, 0, -3],
        read_align_off=[0, 1, 2, 3, 5],
        align_score_sum=[1, 1, 1, 8, 7],       # :218-224: one alignment -> score 1, length 1, the prior's location
        align_length=[1, 1, 1, 40, 40],
        align_frag_length=[5, 5, 5, 6, 6],
        align_path_off=[0, 2, 4, 5, 6, 7],
        align_path_idx=[0, 1, 0, 1, 0, 0, 1],  # :855-857: positions in the cluster's ascending member list
    )
    assert set(want) == set(got["arrays"])
    for name, values in want.items():
        assert got["arrays"][name].tolist() == values, name
        assert got["arrays"][name].dtype == M.DTYPES[name]


def test_model_single_end_counts_nothing():
    params, lists = M.hand_case()
    got = M.run_model(dict(params, is_single_end=True), [lists])
    assert not got["frag_counts"].any() and got["num_distinct"] == 4


def test_model_is_invariant_under_rechunking():
    lists = M.random_stream(3, num_paths=120, num_lists=900, num_templates=150, long_lists=3)
    params = M.default_params(120)
    whole = M.run_model(params, [lists])
    assert 1 < whole["num_distinct"] < 900 and whole["num_clusters"] > 1
    for chunks in (M.chunked(lists, 1), M.chunked(lists, 7), [[], lists[:400], [], [], lists[400:], []]):
        got = M.run_model(params, chunks)
        assert np.array_equal(got["frag_counts"], whole["frag_counts"])
        for name in whole["arrays"]:
            assert got["arrays"][name].tobytes() == whole["arrays"][name].tobytes(), name


def test_model_extra_sets_join_clusters_and_invalid_chunks_change_nothing():
    params, lists = M.hand_case()
    got = M.run_model(params, [lists], extra_sets=[[2, 4]])
    assert got["clusters"] == [[0, 1], [2, 4, 5], [3]]
    assert got["arrays"]["rank_cluster"].tolist() == [1, 0, 2]
    model = M.IndexModel(**params)
    model.add(lists[:3])
    for bad in (M.mk([]), M.mk([(1, 1, 1, [])]), M.mk([(1, 1, 1, [3, 3])]), M.mk([(1, 1, 1, [6])]), M.mk([(1, 1, 1, [0])], noise_score=1),
                M.mk([(1, 1, 0, [0])]), M.mk([(1, 1, 11, [0])])):
        try:
            model.add([lists[3], bad])
            raise AssertionError("accepted")
        except M.InvalidList as err:
            assert err.index == 1
    model.add([M.mk([(1, 1, 11, [0])], min_mapq=29), M.mk([(1, 1, 0, [0])], is_simple=0)])  # uncounted: any length
    model.add(lists[3:])
    ref = M.IndexModel(**params)
    ref.add(lists[:3] + [M.mk([(1, 1, 11, [0])], min_mapq=29), M.mk([(1, 1, 0, [0])], is_simple=0)] + lists[3:])
    a, b = model.finish(), ref.finish()
    assert all(a["arrays"][n].tobytes() == b["arrays"][n].tobytes() for n in a["arrays"]) and np.array_equal(a["frag_counts"], b["frag_counts"])


def test_host_flattening_under_the_sanitizers():
    """tests/cpp/align_index_flatten_check.cpp: the loop body of AlignmentPathsIndex::add up to the device call (rpvg_amd/host/
    fragment_lists.cpp, which needs no engine), as a program of its own built with AddressSanitizer and UBSan."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    binary = os.path.join(out_dir, "align_index_flatten_check")
    host = os.path.join(root, "rpvg_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + host,  # the runtimes inside the program: no order of libraries to keep

                           os.path.join(root, "tests", "cpp", "align_index_flatten_check.cpp"), os.path.join(host, "fragment_lists.cpp"), "-o", binary])
    assert subprocess.run([binary], capture_output=True, text=True, check=True).stdout.strip() == "ok"
