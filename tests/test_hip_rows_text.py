"""The --write-probs dump on the GPU (rpvg_amd/csrc/rows_text.hip; rpvg_hip_rows_text and rpvg_hip_read_rows_text of
include/rpvg_hip.h) against the plain-Python model of tests/rows_text_model.py, which tests/test_rows_text_model.py pins to
hand-written lines and to the file writeProbabilityClusters writes.  Every byte and every row_off is compared: there is no
tolerance."""
import math

import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.table_text import Labels, RowsInput, TableText
from tests import rows_text_model as R
from tests import table_text_model as M

pytestmark = pytest.mark.gpu

U32_MAX, U64_MAX = 4294967295, 18446744073709551615
NAME_LENGTHS = [0, 1, 3, 4, 5, 26, 27, 255]


def assert_text(text, want_bytes, want_off):
    """The view of a device text against the model's bytes and offsets; the guards around the text on the device are intact."""
    got = text.view()
    assert got["row_off"].tolist() == [int(x) for x in want_off]
    assert got["num_bytes"] == len(want_bytes) and got["num_rows"] == int(np.count_nonzero(np.diff(np.asarray(want_off, dtype=np.int64))))
    if got["bytes"] != want_bytes:
        at = next(i for i in range(min(len(want_bytes), len(got["bytes"]))) if got["bytes"][i] != want_bytes[i])
        raise AssertionError(f"byte {at}: {got['bytes'][max(at - 30, 0):at + 30]!r} != {want_bytes[max(at - 30, 0):at + 30]!r}")
    assert text.guards_intact()
    return got


def path_side(clusters, name_lengths=(3,), seed=0):
    """(names, lengths, effective lengths) of the paths of the clusters"""
    P = sum(c["num_paths"] for c in clusters)
    rng = np.random.default_rng(seed)
    names = M.names_of_lengths([name_lengths[i % len(name_lengths)] for i in range(P)], seed=seed)
    return names, [int(x) for x in rng.integers(0, 100000, size=P)], [float(x) for x in rng.gamma(2.0, 400.0, size=P)]


def check(ctx, clusters, names, lengths, eff, prob_precision=1e-8, lists=None, index=None):
    flat = R.flatten(clusters)
    want_bytes, want_off = R.rows_text(flat, names, lengths, eff, prob_precision, lists, index)
    assert len(want_off) == 2 * len(clusters) + len(flat["row_count"]) + 1
    text = TableText.rows(ctx, RowsInput.of(flat, eff, lists, index), Labels.of(names, list(range(len(clusters))), lengths), prob_precision)
    try:
        return assert_text(text, want_bytes, want_off)
    finally:
        text.free()


# ---- the shapes of a row line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ranked", [False, True])
def test_rows_of_no_one_and_two_groups_and_groups_of_every_size(hip_ctx, ranked):
    """Rows of 0, 1 and 2 groups; groups of 0, 1, 63, 64 and 65 members; read counts 0, 9, 10 and 2^32 - 1; rank keys 0 and 2^64 - 1."""
    rng = np.random.default_rng(1)
    members = lambda n: [int(x) for x in rng.integers(0, 70, size=n)]
    rows = [(0, 0.5, []), (9, 0.25, [(0.5, [])]), (10, 1e-9, [(0.125, [69])]), (U32_MAX, 1.0, [(0.1, members(63)), (0.2, members(64))]),
            (1, 0.3, [(0.3, members(65)), (0.4, [])]), (7, 0.9, [(0.5, []), (0.6, [0, 1])])]
    clusters = [dict(num_paths=70, rows=rows), dict(num_paths=1, rows=[(3, 0.75, [(0.25, [0])])])]
    names, lengths, eff = path_side(clusters)
    got = check(hip_ctx, clusters, names, lengths, eff, lists=[0, U64_MAX] if ranked else None, index=[U64_MAX, 0] if ranked else None)
    assert got["num_rows"] == 4 + 7 and b"\n0 0.5\n9 0.25 0.5:\n10 1e-09 0.125:69\n4294967295 1 0.1:" in got["bytes"]
    assert got["bytes"].startswith(b"# 0 18446744073709551615\n" if ranked else b"#\n") and (b"\n# 18446744073709551615 0\n" in got["bytes"]) == ranked


def test_rows_of_61_to_67_and_129_cells(hip_ctx):
    """Rows that end inside, at and just behind a wavefront's 64 cells, at every position of the row in its block: each width at 70
    different offsets."""
    rng = np.random.default_rng(2)
    rows = []
    for shift in range(70):
        rows += [R.row_of_cells(n, rng, 5) for n in (61, 62, 63, 64, 65, 66, 67, 129)] + [R.row_of_cells(2 + shift % 3, rng, 5)]
    clusters = [dict(num_paths=5, rows=rows)]
    names, lengths, eff = path_side(clusters)
    got = check(hip_ctx, clusters, names, lengths, eff)
    assert got["num_rows"] == 2 + len(rows) and {int(x) % 4 for x in got["row_off"][:-1]} == {0, 1, 2, 3}


def test_a_row_longer_than_the_staging_block_and_64_longest_cells(hip_ctx):
    """One row of 3000 indices (its text exceeds a staging block many times) and, at 17 digits, rows of 64 groups without members whose
    probabilities are the longest cell: 63 * 26 + 27 bytes in 64 cells, the most a block holds, ending at every residue of 64."""
    rng = np.random.default_rng(3)
    rows = [(1, 0.5, [(0.5, [int(x) for x in rng.integers(0, 100000, size=3000)])])]
    for _ in range(64):
        rows += [(1, 0.5, [(0.5, [])]), (1, 0.5, [(M.LONGEST[1], [])] * 64)]
    clusters = [dict(num_paths=100000, rows=rows)]
    names, lengths, eff = path_side(clusters, (1,))
    got = check(hip_ctx, clusters, names, lengths, eff, prob_precision=1e-17)
    assert int(got["row_off"][3] - got["row_off"][2]) > 4 * 1668


# ---- the path line --------------------------------------------------------------------------------------------------------------------

def test_path_lines_of_1_2_64_65_and_300_paths(hip_ctx):
    """Names of 0, 1, 3, 4, 5, 26, 27 and 255 bytes; the lines start at every residue modulo 4."""
    clusters = [dict(num_paths=n, rows=[(n, 0.5, [(0.5, [n - 1])])]) for n in (1, 2, 64, 65, 300)]
    names, lengths, eff = path_side(clusters, NAME_LENGTHS, seed=4)
    assert {len(n) for n in names} == set(NAME_LENGTHS)
    got = check(hip_ctx, clusters, names, lengths, eff)
    assert got["num_rows"] == 15
    # different name lengths in front shift every line: all residues with the next case's names
    residues = {int(x) % 4 for x in got["row_off"][:-1]}
    for rotate in range(1, 4):
        got = check(hip_ctx, clusters, names[rotate:] + names[:rotate], lengths, eff)
        residues |= {int(x) % 4 for x in got["row_off"][:-1]}
    assert residues == {0, 1, 2, 3}


def test_a_cluster_of_100001_paths(hip_ctx):
    """A row that lists index 100 000; the path line is 300 003 cells."""
    clusters = [dict(num_paths=2, rows=[(1, 0.5, [(0.5, [1])])]), dict(num_paths=100001, rows=[(2, 0.25, [(0.75, [0, 100000])]), (1, 0.5, [])])]
    names, lengths, eff = path_side(clusters, (0, 1, 5, 9), seed=5)
    got = check(hip_ctx, clusters, names, lengths, eff)
    assert b" 0.75:0,100000\n" in got["bytes"] and R.num_cells(R.flatten(clusters)) > 300000


# ---- skipped clusters ------------------------------------------------------------------------------------------------------------------

def test_skipped_clusters(hip_ctx):
    """A cluster without rows and one without paths have no bytes: first, last, adjacent, all of them, and no cluster at all."""
    full = lambda n: dict(num_paths=n, rows=[(1, 0.5, [(0.5, [n - 1])]), (2, 0.25, [])])
    no_rows, no_paths, neither = dict(num_paths=2, rows=[]), dict(num_paths=0, rows=[(1, 0.5, [])]), dict(num_paths=0, rows=[])
    for clusters, printed in (([no_rows, full(2), no_paths, neither, no_rows, full(3), full(1), no_paths], 3), ([full(1), no_rows, full(2)], 2),
                              ([no_rows, no_paths, neither], 0), ([no_paths], 0), ([neither], 0), ([], 0)):
        names, lengths, eff = path_side(clusters, (2, 5))
        K = len(clusters)
        for ranked in (False, True):
            got = check(hip_ctx, clusters, names, lengths, eff, lists=list(range(K)) if ranked else None, index=list(range(K, 2 * K)) if ranked else None)
            assert got["num_rows"] == 4 * printed and got["bytes"].count(b"#") == printed
    assert got["num_bytes"] == 0 and got["row_off"].tolist() == [0]


# ---- hard cells -----------------------------------------------------------------------------------------------------------------------

TIES_12 = [100000000000.5, 100000000001.5]   # even and odd at 12 digits


@pytest.mark.parametrize("prob_precision, digits", [(1e-8, 8), (1e-12, 12), (1e-17, 17)])
def test_hard_cells_as_noise_probability_and_effective_length(hip_ctx, prob_precision, digits):
    """Ties of both parities, the carry 1.99999995, -0.0, a subnormal, inf, both NaNs and the longest cell in the three columns of
    doubles; the effective length is printed at 8 digits whatever the precision."""
    assert R.digits_of(prob_precision) == digits
    ties = {8: M.TIES_8, 12: TIES_12, 17: M.TIES_17}[digits]
    assert {M.is_tie(v, digits)[1] for v in ties if M.is_tie(v, digits)[0]} == {0, 1}
    hard = ties + M.TIES_8 + M.CARRIES + M.SPECIALS + M.LONGEST
    rows = [(i, hard[i], [(hard[(i + 3) % len(hard)], [i]), (hard[(i + 7) % len(hard)], [])]) for i in range(len(hard))]
    clusters = [dict(num_paths=len(hard), rows=rows)]
    names, lengths, _ = path_side(clusters)
    hip_ctx.reset_stats()
    got = check(hip_ctx, clusters, names, lengths, hard, prob_precision)
    row_cells = [r[1] for r in rows] + [g[0] for r in rows for g in r[2]]
    num_ties = sum(1 for v in row_cells if math.isfinite(v) and v != 0 and M.is_tie(v, digits)[0]) + sum(1 for v in hard if math.isfinite(v) and v != 0 and M.is_tie(v, 8)[0])
    assert num_ties >= 3 * 2 + 5 and hip_ctx.stats()["text_exact_cells"] >= num_ties
    assert b",1.2345678e+08 " in got["bytes"] and b",-1.2345678e-308" in got["bytes"] and b",-nan" in got["bytes"] and b",-0 " in got["bytes"]
    assert (b" " + M.fmt(1.99999995, digits).encode() + b" ") in got["bytes"] and M.fmt(1.99999995, 8) == "2"
    assert max(len(M.fmt(v, digits)) for v in row_cells) == {8: 15, 12: 19, 17: 24}[digits]
    for special in (b" -0 ", b" inf ", b" -inf ", b" nan ", b" -nan ", b" 4.9406564584124654e-324 " if digits == 17 else b" 4.9406565e-324 " if digits == 8 else b" 4.94065645841e-324 "):
        assert special in got["bytes"]


def test_exact_cells_are_counted_for_ties_alone(hip_ctx):
    clusters = [dict(num_paths=2, rows=[(1, 0.5, [(0.25, [0])]), (1, 0.75, [])]), dict(num_paths=1, rows=[])]
    names, lengths, _ = path_side(clusters)
    hip_ctx.reset_stats()
    check(hip_ctx, clusters, names, lengths, [1.0, 2.0, 10000000.5])      # (the tie belongs to a cluster that is not printed)
    assert hip_ctx.stats()["text_exact_cells"] == 0
    clusters[0]["rows"] = [(1, 10000000.5, [(123456785.0, [0])]), (1, 0.75, [])]
    check(hip_ctx, clusters, names, lengths, [10000001.5, 2.0, 3.0])
    assert hip_ctx.stats()["text_exact_cells"] == 3


# ---- equal bytes across routes --------------------------------------------------------------------------------------------------------

def test_device_arrays_two_builds_and_ranges(hip_ctx):
    """Host arrays against device arrays (labels too), two builds, and rpvg_hip_table_text_get on ranges that split a line."""
    rng = np.random.default_rng(13)
    clusters = [dict(num_paths=9, rows=[R.row_of_cells(int(n), rng, 9, count=int(n)) for n in rng.integers(2, 40, size=60)]), dict(num_paths=0, rows=[]),
                dict(num_paths=70, rows=[R.row_of_cells(int(n), rng, 70) for n in rng.integers(2, 150, size=30)])]
    names, lengths, eff = path_side(clusters, NAME_LENGTHS, seed=13)
    flat = R.flatten(clusters)
    lists, index = [5, 6, 7], [0, U64_MAX, 9]
    want_bytes, want_off = R.rows_text(flat, names, lengths, eff, 1e-12, lists, index)
    rows, labels = RowsInput.of(flat, eff, lists, index), Labels.of(names, [1, 2, 3], lengths)
    pointers, label_pointers = {}, {}
    try:
        for source, into in ((rows, pointers), (labels, label_pointers)):
            for name, _ in source._FIELDS:
                a = getattr(source, name)
                into[name] = hip_ctx.malloc(max(a.nbytes, 8))
                if a.nbytes:
                    hip_ctx.h2d(into[name], a)
        for rows_c, labels_c in ((rows, labels), (rows, labels), (rows.as_c(device_pointers=pointers), labels.as_c(device_pointers=label_pointers)),
                                 (rows, labels.as_c(device_pointers=label_pointers)), (rows.as_c(device_pointers=pointers), labels)):
            text = TableText.rows(hip_ctx, rows_c, labels_c, 1e-12)
            try:
                assert_text(text, want_bytes, want_off)
                n = len(want_bytes)
                inside = int(want_off[2]) + 1   # inside the first row line
                for begin, end in ((0, n), (1, n - 1), (7, 7), (n, n), (inside, inside + 1), (inside, n - 2)):
                    assert text.bytes(begin, end) == want_bytes[begin:end]
                with pytest.raises(hip.EngineError, match=r"\(-3\)"):
                    text.bytes(1, n + 1)
            finally:
                text.free()
    finally:
        for p in list(pointers.values()) + list(label_pointers.values()):
            hip_ctx.free(p)


# ---- the resident route ---------------------------------------------------------------------------------------------------------------

def cluster_keys(batch):
    """The clusters of a batch that have rows and paths, each as (structure, values) of its rows, in an order of the structures."""
    out = []
    for k in range(batch.num_clusters):
        rows = batch.cluster(k)["rows"]
        if rows and int(batch.cluster_path_off[k + 1]) > int(batch.cluster_path_off[k]):
            out.append(([(int(r[0]), [list(map(int, g[1])) for g in r[2]]) for r in rows], [v for r in rows for v in [r[1]] + [g[0] for g in r[2]]]))
    return sorted(out, key=lambda c: repr(c[0]))


@pytest.mark.parametrize("merge, collapse", [(True, False), (False, False), (True, True)])
def test_resident_rows(hip_ctx, tmp_path, merge, collapse):
    """rpvg_hip_read_rows_text on the rows of rpvg_hip_read_rows_build: equal to rpvg_hip_rows_text on the arrays of the rows' view and
    to the file write_batch_files writes from that view; read back, the file gives the rows again; the rows still convert."""
    from rpvg_amd import io as io_mod
    from rpvg_amd.rows import AlignmentBatch
    from tests.test_hip_rows import make_alignment_clusters, params

    batch = AlignmentBatch.from_clusters(make_alignment_clusters(811 if collapse else 801, n_clusters=4, reads_per_cluster=120, collapse=collapse))
    dev = hip_ctx.upload_alignments(batch)
    try:
        rows = dev.build_rows(params(min_noise=1e-4), merge)
        try:
            sizes = hip.CClusterBatch()
            hip._check(hip.lib().rpvg_hip_read_rows_sizes(hip_ctx.handle, rows.handle, hip.C.byref(sizes)), "rpvg_hip_read_rows_sizes")
            K = int(sizes.num_clusters)
            cpo = [int(sizes.cluster_path_off[k]) for k in range(K + 1)]
            P = cpo[K]
            assert collapse == (P < len(batch.path_effective_length))
            rng = np.random.default_rng(5)
            eff = np.array([float(x) for x in rng.integers(1, 5000, size=P)]) + 0.25
            names = [f"c{k}_p{j}" for k in range(K) for j in range(cpo[k + 1] - cpo[k])]            # clustersFromBatch's
            lengths = [int(e) + 50 for e in eff]
            labels = Labels.of(names, list(range(K)), lengths)
            lists, index = list(range(100, 100 + K)), list(range(K))
            texts = {}
            for ranked in (False, True):
                text = rows.text(labels, eff, 1e-8, lists if ranked else None, index if ranked else None)   # before any download
                try:
                    texts[ranked] = text.view()
                    assert text.guards_intact()
                finally:
                    text.free()
            view, _, _ = rows.download()
            view.path_effective_length = eff
            for ranked in (False, True):
                keys = (lists, index) if ranked else (None, None)
                got = check(hip_ctx, [dict(num_paths=cpo[k + 1] - cpo[k], rows=view.cluster(k)["rows"]) for k in range(K)], names, lengths, eff, 1e-8, *keys)
                assert got["bytes"] == texts[ranked]["bytes"] and got["row_off"].tolist() == texts[ranked]["row_off"].tolist() and got["num_rows"] > 2 * K
                probs, info = str(tmp_path / f"probs_{ranked}.txt"), str(tmp_path / f"info_{ranked}.tsv")
                io_mod.write_batch_files(view, probs, info, 1e-8, *keys)
                assert open(probs, "rb").read() == got["bytes"]
            back = io_mod.read_batch_files(probs, info)
            want, read = cluster_keys(view), cluster_keys(back)
            assert [c[0] for c in read] == [c[0] for c in want]
            for (_, a), (_, b) in zip(read, want):
                assert np.allclose(a, b, rtol=1e-7, atol=0)
            device_batch = rows.to_batch()      # the rows are still there
            device_batch.free()
        finally:
            rows.free()
    finally:
        dev.free()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_a_usable_context(hip_ctx):
    rng = np.random.default_rng(14)
    good = [dict(num_paths=3, rows=[R.row_of_cells(6, rng, 3), (1, 0.5, [(0.5, [2, 0])])]), dict(num_paths=2, rows=[(2, 0.25, [(0.125, [1]), (0.25, [0])])])]
    names, lengths, eff = path_side(good, (4, 5, 6))
    labels = Labels.of(names, [0, 1], lengths)
    flat = R.flatten(good)

    def refused(match, changed=None, with_labels=None, prob_precision=1e-8, lists=None, index=None, with_eff=None):
        arrays = {k: v.copy() for k, v in flat.items()}
        for key, (at, value) in (changed or {}).items():
            arrays[key][at] = value
        with pytest.raises(hip.EngineError, match=match):
            TableText.rows(hip_ctx, RowsInput.of(arrays, eff if with_eff is None else with_eff, lists, index), with_labels or labels, prob_precision)

    refused(r"\(-3\).*position 0: cluster_row_off", dict(cluster_row_off=(1, 5)))
    refused(r"\(-3\).*position 1: cluster_row_off", dict(cluster_row_off=(2, 2)))
    refused(r"\(-3\).*position 0: cluster_path_off", dict(cluster_path_off=(1, 6)))
    refused(r"\(-3\).*position 0: row_grp_off", dict(row_grp_off=(0, 1)))
    refused(r"\(-3\).*position 1: row_grp_off", dict(row_grp_off=(2, int(flat["row_grp_off"][1]) - 1)))
    refused(r"\(-3\).*position 0: grp_idx_off", dict(grp_idx_off=(1, 100)))
    refused(r"\(-3\).*position \d+: grp_idx_off", dict(grp_idx_off=(len(flat["grp_idx_off"]) - 1, len(flat["path_idx"]) - 1)))
    descending = Labels.of(names, [0, 1], lengths)
    descending.name_off[2] = descending.name_off[1] - 1
    refused(r"\(-3\).*position 1: name_off", with_labels=descending)
    refused(r"\(-3\).*row 1: a path_idx that is not below", dict(path_idx=(len(flat["path_idx"]) - 4, 3)))     # 3 paths: index 3
    refused(r"\(-3\).*row 2: a path_idx that is not below", dict(path_idx=(len(flat["path_idx"]) - 1, 2)))     # 2 paths: index 2
    refused(r"\(-3\).*one rank-key array without the other", lists=[1, 2])
    refused(r"\(-3\).*one rank-key array without the other", index=[1, 2])
    refused(r"\(-3\).*labels of 4 paths", with_labels=Labels.of(names[:4], [0, 1], lengths[:4]))
    refused(r"\(-3\).*in 1 clusters", with_labels=Labels.of(names, [0], lengths))
    refused(r"\(-3\).*path_length", with_labels=Labels.of(names, [0, 1]))
    refused(r"\(-3\).*labels of 5 paths.*rows have 4", with_eff=eff[:4])
    for precision in (0.0, 1.0, -1e-8, float("nan")):
        refused(r"\(-3\).*prob_precision outside \(0, 1\)", prob_precision=precision)
    refused(r"\(-3\).*more than 17 digits", prob_precision=1e-18)
    check(hip_ctx, good, names, lengths, eff)                               # the context is usable afterwards
    check(hip_ctx, good, names, lengths, eff, 1e-17, [1, 2], [3, 4])


# ---- the host class and the harness ----------------------------------------------------------------------------------------------------

def test_the_host_class_from_arrays_and_from_resident_rows(tmp_path):
    """HarnessTableText(kind=ROWS) through TableText::rows of rpvg_amd/host/table_text.hpp, from flat arrays and from rows resident
    on the engine's context: each text is the model's and the host line's, write() puts it into the file as it is, and the parent's
    route (rpvg_hip_read_rows_view, one ReadPathProbabilities per row, writeProbabilityClusters into a stream) has its length."""
    import types

    from rpvg_amd import engine as eng_mod
    from rpvg_amd.rows import AlignmentBatch
    from rpvg_amd.table_text import ROWS, HarnessTableText
    from tests.test_hip_rows import make_alignment_clusters, params

    engine = eng_mod.Engine(0)
    try:
        on_engine = types.SimpleNamespace(handle=engine._ctx())
        dev = hip.DeviceAlignments(on_engine, AlignmentBatch.from_clusters(make_alignment_clusters(802, n_clusters=3, reads_per_cluster=80)))
        try:
            rows = dev.build_rows(params(min_noise=1e-4), True)
            try:
                sizes = hip.CClusterBatch()
                hip._check(hip.lib().rpvg_hip_read_rows_sizes(on_engine.handle, rows.handle, hip.C.byref(sizes)), "rpvg_hip_read_rows_sizes")
                K = int(sizes.num_clusters)
                cpo = [int(sizes.cluster_path_off[k]) for k in range(K + 1)]
                eff = np.arange(cpo[K], dtype=np.float64) * 1.5 + 10.125
                names = [f"c{k}_p{j}" for k in range(K) for j in range(cpo[k + 1] - cpo[k])]
                lengths = [int(e) + 50 for e in eff]
                labels = Labels.of(names, list(range(K)), lengths)
                lists, index = list(range(7, 7 + K)), list(range(K))
                resident = HarnessTableText(engine, rows.handle, kind=ROWS, labels=labels, prob_precision=1e-12, effective_lengths=eff, num_align_lists=lists,
                                            cluster_index=index)
                try:
                    got = resident.view()
                    view, _, _ = rows.download()
                    flat = {name: getattr(view, name) for name, _ in RowsInput._FIELDS[:8]}
                    want_bytes, want_off = R.rows_text(flat, names, lengths, eff, 1e-12, lists, index)
                    assert got["bytes"] == want_bytes and got["row_off"].tolist() == want_off.tolist() and got["num_rows"] > 2 * K
                    line = resident.host_line(len(want_off) - 1)
                    assert line["equal"] and line["bytes"] == want_bytes and line["row_off"].tolist() == want_off.tolist()
                    resident.write(str(tmp_path / "resident.txt"))
                    assert open(tmp_path / "resident.txt", "rb").read() == want_bytes
                    resident.parent_route()
                finally:
                    resident.free()
                arrays = HarnessTableText(engine, RowsInput.of(flat, eff, lists, index), kind=ROWS, labels=labels, prob_precision=1e-12)
                try:
                    assert arrays.view()["bytes"] == want_bytes and arrays.host_line(len(want_off) - 1)["equal"]
                    arrays.write(str(tmp_path / "arrays.txt.gz"))
                    import gzip
                    assert gzip.open(tmp_path / "arrays.txt.gz", "rb").read() == want_bytes
                    arrays.parent_route()
                finally:
                    arrays.free()
            finally:
                rows.free()
        finally:
            dev.free()
    finally:
        engine.close()
