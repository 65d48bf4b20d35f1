"""The table text on the GPU (rpvg_amd/csrc/table_text.hip, include/rpvg_text.h) against the plain-Python model of
tests/table_text_model.py, which tests/test_table_text_model.py pins to hand-written rows and whose number format
tests/cpp/number_text_check.cpp holds to glibc.  Every byte and every row_off is compared: there is no tolerance."""
import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.batch import ClusterBatch
from rpvg_amd.estimates_table import EstimatesTable, FlatEstimates
from rpvg_amd.gibbs_table import FlatGibbs, GibbsSamples, GibbsTable
from rpvg_amd.table_text import HAPLOTYPE, PER_PATH, Labels, TableText
from tests import estimates_table_model as EM
from tests import gibbs_table_model as GM
from tests import large_cases
from tests import table_text_model as M

pytestmark = pytest.mark.gpu


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


def gibbs_table_of(ctx, listed_rows, N):
    clusters = M.gibbs_clusters(listed_rows, N)
    return GibbsTable.build(ctx, FlatGibbs(**GM.flatten(clusters, N))), GM.table(clusters, N), GM.flatten(clusters, N)["cluster_path_off"]


def check_gibbs(ctx, listed_rows, N, names, cluster_ids, precision=8):
    table, want_table, cluster_path_off = gibbs_table_of(ctx, listed_rows, N)
    try:
        want_bytes, want_off = M.gibbs_text(want_table, cluster_path_off, names, cluster_ids, precision)
        text = TableText.gibbs(ctx, table, Labels.of(names, cluster_ids), precision)
        try:
            return assert_text(text, want_bytes, want_off)
        finally:
            text.free()
    finally:
        table.free()


def rows_of(rng, counts, N, unlisted=()):
    """counts: paths per cluster; unlisted: batch-wide paths without a row."""
    rows, g = [], 0
    for n in counts:
        rows.append([None if g + i in unlisted else M.sample_values(rng, N) for i in range(n)])
        g += n
    return rows


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 128, 129])
def test_samples_per_row(hip_ctx, N):
    """Either side of the wavefront's step of 64 cells (the ClusterID is the first cell: 63 samples fill a step)."""
    rng = np.random.default_rng(N)
    rows = rows_of(rng, [3, 2], N, unlisted={1})
    check_gibbs(hip_ctx, rows, N, M.names_of_lengths([7, 2, 0, 11, 5]), [1, 4000000000])


def test_names_of_every_length_and_rows_at_every_alignment(hip_ctx):
    lengths = M.NAME_LENGTHS + M.NAME_LENGTHS[::-1]
    rng = np.random.default_rng(5)
    got = check_gibbs(hip_ctx, rows_of(rng, [5, 7], 3), 3, M.names_of_lengths(lengths), [12, 345])
    assert {int(x) % 4 for x in got["row_off"][:-1]} == {0, 1, 2, 3}


def test_edges_of_the_table(hip_ctx):
    rng = np.random.default_rng(6)
    # the first and the last row unlisted, two adjacent unlisted rows, a cluster without paths
    rows = rows_of(rng, [4, 0, 5], 5, unlisted={0, 2, 3, 8})
    got = check_gibbs(hip_ctx, rows, 5, M.names_of_lengths([3] * 9), [1, 2, 3])
    assert got["num_rows"] == 5
    # no listed row at all
    got = check_gibbs(hip_ctx, rows_of(rng, [2, 1], 4, unlisted={0, 1, 2}), 4, M.names_of_lengths([3] * 3), [1, 2])
    assert got["num_bytes"] == 0 and got["bytes"] == b"" and got["row_off"].tolist() == [0, 0, 0, 0]
    # no path at all
    got = check_gibbs(hip_ctx, [], 4, [], [])
    assert got["num_bytes"] == 0 and got["row_off"].tolist() == [0]


@pytest.mark.parametrize("precision", [8, 17])
def test_hard_cells(hip_ctx, precision):
    """Ties of both parities, carries that change the notation, -0.0, a subnormal, inf, both NaNs and the longest cell: one table
    printed at precision 8 and again at 17."""
    cells = M.HARD_CELLS
    N = len(cells)
    rows = [[cells, cells[::-1]], [[-v for v in cells]]]
    hip_ctx.reset_stats()
    got = check_gibbs(hip_ctx, rows, N, ["ties", "seit", "negated"], [1, 2], precision)
    ties = 3 * sum(1 for v in cells if np.isfinite(v) and v != 0 and M.is_tie(v, precision)[0])   # three rows hold every cell once
    assert ties >= 9 and hip_ctx.stats()["text_exact_cells"] >= ties                                # (counted by the measure pass alone)
    longest = max(len(M.fmt(v, precision)) for v in cells)
    assert longest == (15 if precision == 8 else 24) and b"-nan" in got["bytes"] and b"\tnan" in got["bytes"]


def test_exact_cells_are_counted_for_ties_alone(hip_ctx):
    rng = np.random.default_rng(8)
    hip_ctx.reset_stats()
    check_gibbs(hip_ctx, [[[float(x) for x in rng.integers(0, 1000, size=70)] for _ in range(3)]], 70, ["a", "b", "c"], [1])
    assert hip_ctx.stats()["text_exact_cells"] == 0
    check_gibbs(hip_ctx, [[[10000000.5, 10000001.5, 3.0]]], 3, ["a"], [1])
    assert hip_ctx.stats()["text_exact_cells"] == 2


def test_two_builds_and_device_labels_give_the_same_bytes(hip_ctx):
    rng = np.random.default_rng(9)
    names, ids = M.names_of_lengths([4, 0, 9, 1, 30, 2]), [5, 6]
    table, want_table, cpo = gibbs_table_of(hip_ctx, rows_of(rng, [2, 4], 66, unlisted={3}), 66)
    labels = Labels.of(names, ids)
    pointers = {}
    try:
        want_bytes, want_off = M.gibbs_text(want_table, cpo, names, ids)
        for name, _ in labels._FIELDS:
            a = getattr(labels, name)
            pointers[name] = hip_ctx.malloc(max(a.nbytes, 8))
            if a.nbytes:
                hip_ctx.h2d(pointers[name], a)
        device_labels = labels.as_c(device_pointers=pointers)
        for source in (labels, labels, device_labels):
            text = TableText.gibbs(hip_ctx, table, source)
            try:
                assert_text(text, want_bytes, want_off)
            finally:
                text.free()
    finally:
        table.free()
        for p in pointers.values():
            hip_ctx.free(p)


def test_get_of_ranges_equals_the_view(hip_ctx):
    rng = np.random.default_rng(10)
    table, _, _ = gibbs_table_of(hip_ctx, rows_of(rng, [3], 9), 9)
    text = TableText.gibbs(hip_ctx, table, Labels.of(["x", "yy", "zzz"], [1]))
    try:
        whole = text.view()["bytes"]
        n = len(whole)
        cell = whole.index(b"\t", 3)   # inside the first row
        for begin, end in ((0, n), (1, n - 1), (7, 7), (n, n), (cell + 1, cell + 2)):
            assert text.bytes(begin, end) == whole[begin:end]
        with pytest.raises(hip.EngineError, match=r"\(-3\)"):
            text.bytes(1, n + 1)
        with pytest.raises(hip.EngineError, match=r"\(-3\)"):
            text.bytes(5, 4)
    finally:
        text.free()
        table.free()


def test_refusals_leave_a_usable_context(hip_ctx):
    rng = np.random.default_rng(11)
    names, ids = M.names_of_lengths([4, 5, 6]), [7, 8]
    table, want_table, cpo = gibbs_table_of(hip_ctx, rows_of(rng, [2, 1], 4), 4)
    try:
        labels = Labels.of(names, ids)
        for precision in (0, 18):
            with pytest.raises(hip.EngineError, match=r"\(-3\).*precision"):
                TableText.gibbs(hip_ctx, table, labels, precision)
        descending = Labels.of(names, ids)
        descending.name_off[2] = descending.name_off[1] - 1
        with pytest.raises(hip.EngineError, match=r"\(-3\).*path 1: name_off"):
            TableText.gibbs(hip_ctx, table, descending)
        short = Labels.of(names, ids)
        with pytest.raises(hip.EngineError, match=r"\(-3\).*path 2: name_off"):
            TableText.gibbs(hip_ctx, table, short.as_c(num_name_bytes=len(short.name_bytes) - 1))
        with pytest.raises(hip.EngineError, match=r"\(-3\).*labels of 2 paths"):
            TableText.gibbs(hip_ctx, table, Labels.of(names[:2], ids))
        with pytest.raises(hip.EngineError, match=r"\(-3\).*in 1 clusters"):
            TableText.gibbs(hip_ctx, table, Labels.of(names, ids[:1]))
        want_bytes, want_off = M.gibbs_text(want_table, cpo, names, ids)
        text = TableText.gibbs(hip_ctx, table, labels)   # the context is usable afterwards
        try:
            assert_text(text, want_bytes, want_off)
        finally:
            text.free()
    finally:
        table.free()


# ---- the estimates files -----------------------------------------------------------------------------------------------------------

def per_path_cluster(rng, n, eff):
    return dict(num_paths=n, sets=[(i,) for i in range(n)], posteriors=[1.0] * n, abundances=[0.0 if i % 5 == 1 else float(x) for i, x in enumerate(rng.gamma(0.8, 30.0, size=n))],
                noise_count=float(rng.random()), eff=eff)


def estimates_case():
    """1, 2 and 70 paths per cluster, an empty cluster between them; effective lengths that print in fixed and in exponent notation,
    a zero abundance (a zero TPM) in every cluster of more than one path."""
    rng = np.random.default_rng(12)
    clusters = [per_path_cluster(rng, 1, [812.25]), per_path_cluster(rng, 2, [1e-7, 123456789.0]), per_path_cluster(rng, 0, []),
                per_path_cluster(rng, 70, [float(x) for x in rng.gamma(2.0, 400.0, size=70)])]
    P = sum(c["num_paths"] for c in clusters)
    names = M.names_of_lengths([(3 * i) % 14 for i in range(P)], seed=3)
    lengths = [int(x) for x in rng.integers(1, 2 ** 32, size=P)]
    return clusters, names, lengths, [3, 1, 4, 1000000]


def check_estimates(ctx, clusters, names, lengths, ids, kind, precision=8):
    flat = FlatEstimates(**EM.flatten(clusters))
    model = EM.table(clusters, 2)
    model = EM.with_tpm(model, model["total_transcript_count"])
    table = EstimatesTable.build(ctx, None, flat, 2)
    try:
        table.tpm(model["total_transcript_count"])
        want_bytes, want_off = M.estimates_text(kind, EM.flatten(clusters), model, names, lengths, ids, precision)
        text = TableText.estimates(ctx, table, flat.as_c(), Labels.of(names, ids, lengths), kind, precision)
        try:
            return assert_text(text, want_bytes, want_off)
        finally:
            text.free()
    finally:
        table.free()


@pytest.mark.parametrize("kind", [PER_PATH, HAPLOTYPE])
@pytest.mark.parametrize("precision", [8, 17])
def test_estimates_rows(hip_ctx, kind, precision):
    clusters, names, lengths, ids = estimates_case()
    got = check_estimates(hip_ctx, clusters, names, lengths, ids, kind, precision)
    assert b"\t812.25\t" in got["bytes"] and b"\t0\n" in got["bytes"] and got["num_rows"] == 73
    assert (b"\t1e-07\t" if precision == 8 else b"\t9.9999999999999995e-08\t") in got["bytes"]


def test_estimates_from_device_arrays(hip_ctx):
    clusters, names, lengths, ids = estimates_case()
    flat = FlatEstimates(**EM.flatten(clusters))
    model = EM.table(clusters, 2)
    model = EM.with_tpm(model, model["total_transcript_count"])
    pointers = {}
    table = EstimatesTable.build(hip_ctx, None, flat, 2)
    try:
        table.tpm(model["total_transcript_count"])
        for name, _ in flat._FIELDS:
            a = getattr(flat, name)
            pointers[name] = hip_ctx.malloc(max(a.nbytes, 8))
            if a.nbytes:
                hip_ctx.h2d(pointers[name], a)
        for kind in (PER_PATH, HAPLOTYPE):
            want_bytes, want_off = M.estimates_text(kind, EM.flatten(clusters), model, names, lengths, ids)
            text = TableText.estimates(hip_ctx, table, flat.as_c(device_pointers=pointers), Labels.of(names, ids, lengths), kind)
            try:
                assert_text(text, want_bytes, want_off)
            finally:
                text.free()
    finally:
        table.free()
        for p in pointers.values():
            hip_ctx.free(p)


def test_estimates_refusals(hip_ctx):
    clusters, names, lengths, ids = estimates_case()
    rng = np.random.default_rng(13)
    pairs = dict(num_paths=2, sets=[(0, 1), (1, 1)], posteriors=[0.75, 0.25], abundances=[1.0, 2.0, 3.0, 4.0], noise_count=0.5, eff=[100.0, 200.0])
    swapped = per_path_cluster(rng, 3, [10.0, 20.0, 30.0])
    swapped["sets"] = [(0,), (2,), (1,)]
    for wrong, at in ((pairs, 1), (swapped, 3)):
        broken = list(clusters)
        broken[at] = wrong
        P = sum(c["num_paths"] for c in broken)
        broken_names, broken_lengths = M.names_of_lengths([4] * P), [100] * P
        with pytest.raises(ValueError, match=f"cluster {at}"):
            M.estimates_text(PER_PATH, EM.flatten(broken), None, broken_names, broken_lengths, ids)
        flat = FlatEstimates(**EM.flatten(broken))
        table = EstimatesTable.build(hip_ctx, None, flat, 2)
        try:
            table.tpm(1.0)
            with pytest.raises(hip.EngineError, match=rf"\(-3\).*cluster {at}: "):
                TableText.estimates(hip_ctx, table, flat.as_c(), Labels.of(broken_names, ids, broken_lengths), PER_PATH)
        finally:
            table.free()
        check_estimates(hip_ctx, broken, broken_names, broken_lengths, ids, HAPLOTYPE)   # the same estimates print as haplotype rows
    flat = FlatEstimates(**EM.flatten(clusters))
    table = EstimatesTable.build(hip_ctx, None, flat, 2)
    try:
        labels = Labels.of(names, ids, lengths)
        with pytest.raises(hip.EngineError, match=r"\(-3\).*no TPMs"):
            TableText.estimates(hip_ctx, table, flat.as_c(), labels, HAPLOTYPE)
        table.tpm(1.0)
        with pytest.raises(hip.EngineError, match=r"\(-3\).*precision"):
            TableText.estimates(hip_ctx, table, flat.as_c(), labels, HAPLOTYPE, 18)
        with pytest.raises(hip.EngineError, match=r"\(-3\).*no such kind"):
            TableText.estimates(hip_ctx, table, flat.as_c(), labels, 2)
        with pytest.raises(hip.EngineError, match=r"\(-3\).*path_length"):
            TableText.estimates(hip_ctx, table, flat.as_c(), Labels.of(names, ids), HAPLOTYPE)
        other = FlatEstimates(**EM.flatten(clusters[:2]))
        with pytest.raises(hip.EngineError, match=r"\(-3\).*not that of the estimates"):
            TableText.estimates(hip_ctx, table, other.as_c(), labels, HAPLOTYPE)
    finally:
        table.free()
    check_estimates(hip_ctx, clusters, names, lengths, ids, PER_PATH)   # the context is usable afterwards


# ---- the sampler's resident handle ---------------------------------------------------------------------------------------------------

def test_text_of_the_resident_handle_equals_the_text_of_the_arrays(hip_ctx, monkeypatch):
    """The one-workgroup case of tests/test_hip_gibbs_table.py: the table built from the sampler's handle and the table built from
    the downloaded samples print the same bytes, the model's."""
    monkeypatch.delenv("RPVG_HIP_EM_GRID_MIN_WORK", raising=False)
    tall = large_cases.cluster_batch(300, 12, 3, seed=31, noise_only_frac=0.02, max_count=400)
    wide = large_cases.cluster_batch(40, 300, 3, seed=32, noise_only_frac=0.1)
    batch = ClusterBatch.concat([tall, wide])
    problems_of, num_samples, seeds, thin, N = [0, 1, 1], [4, 4, 0], [77, 78, 79], 2, 9
    all_columns = [list(range(int(batch.cluster_path_off[k + 1] - batch.cluster_path_off[k]))) for k in range(batch.num_clusters)]
    columns = [all_columns[k] for k in problems_of]
    dev = hip_ctx.upload(batch)
    try:
        abund, noise, total, _ = hip_ctx.em_solve(dev, problems_of, columns)
        got = hip_ctx.gibbs_read_counts(dev, problems_of, columns, abund, noise, num_samples, seeds, thin)
        handle = GibbsSamples.draw(hip_ctx, dev, problems_of, columns, abund, noise, num_samples, seeds, thin)
        try:
            K = batch.num_clusters
            cluster_total = [float(total[problems_of.index(k)]) for k in range(K)]
            clusters = [dict(num_paths=len(all_columns[k]), total_count=cluster_total[k],
                             blocks=[dict(ids=columns[p], noise=got[p][0].tolist(), abund=got[p][1].tolist()) for p in range(len(problems_of)) if problems_of[p] == k])
                        for k in range(K)]
            P = int(batch.cluster_path_off[-1])
            names, ids = M.names_of_lengths([(5 * i) % 9 for i in range(P)], seed=4), [10, 20]
            want_bytes, want_off = M.gibbs_text(GM.table(clusters, N), batch.cluster_path_off, names, ids)
            assert len(want_bytes) > 0
            from_arrays = GibbsTable.build(hip_ctx, FlatGibbs(**GM.flatten(clusters, N)))
            from_handle = GibbsTable.build_resident(hip_ctx, handle, batch.cluster_path_off, cluster_total, N)
            try:
                for table in (from_arrays, from_handle):
                    text = TableText.gibbs(hip_ctx, table, Labels.of(names, ids))
                    try:
                        assert_text(text, want_bytes, want_off)
                    finally:
                        text.free()
            finally:
                from_arrays.free()
                from_handle.free()
        finally:
            handle.free()
    finally:
        dev.free()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def test_end_to_end(tmp_path):
    """Engine.run of haplotype-transcripts with -n 3 on the small_cases batch of the tables' own end-to-end tests, one batch per
    writer: the Gibbs file and the per-path haplotype file written through addText() are the files of addSamples() and
    addEstimates(), byte for byte, and each text is the host line's."""
    import gzip

    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import make_params
    from rpvg_amd.estimates_table import HarnessTable, write_from_containers
    from rpvg_amd.gibbs_table import HarnessGibbsTable, from_containers
    from rpvg_amd.table_text import HarnessTableText
    from tests import small_cases

    N = 3
    batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(4242, n_clusters=8, with_empty=True))
    P = int(batch.cluster_path_off[-1])
    params = make_params(num_gibbs_samples=N)
    engine = eng_mod.Engine(0)
    try:
        prepared = engine.prepare(batch)
        try:
            engine.run("haplotype-transcripts", params, prepared)
            from_containers(prepared, N, P, prefix=str(tmp_path / "containers_gibbs"), unaligned_read_count=9, table=False)
            gibbs = HarnessGibbsTable(engine, prepared, N)
            try:
                text = HarnessTableText(engine, gibbs)
                try:
                    got, line = text.view(), text.host_line(P)
                    assert got["num_rows"] >= 2 and got["bytes"] == line["bytes"] and got["row_off"].tolist() == line["row_off"].tolist()
                    text.write(str(tmp_path / "text_gibbs"), num_gibbs_samples=N, unaligned_read_count=9)
                finally:
                    text.free()
            finally:
                gibbs.free()
            want = gzip.open(tmp_path / "containers_gibbs.txt.gz", "rb").read()
            assert got["bytes"] in want and gzip.open(tmp_path / "text_gibbs.txt.gz", "rb").read() == want
            total = write_from_containers(prepared, "", params.ploidy, "")[0]
            write_from_containers(prepared, "haplotype", params.ploidy, str(tmp_path / "containers_haplotype"), denominator=total,
                                  min_posterior=params.prob_precision, unaligned_read_count=9)
            table = HarnessTable(engine, prepared, params.ploidy)
            try:
                table.tpm(total)
                text = HarnessTableText(engine, table, kind=HAPLOTYPE)
                try:
                    got, line = text.view(), text.host_line(P)
                    assert got["num_rows"] == P and got["bytes"] == line["bytes"] and got["row_off"].tolist() == line["row_off"].tolist()
                    text.write(str(tmp_path / "text_haplotype"), unaligned_read_count=9)
                finally:
                    text.free()
                with pytest.raises(hip.EngineError, match=r"\(-3\).*cluster 0: not one set"):   # haplotype sets are pairs: no per-path abundance rows
                    HarnessTableText(engine, table, kind=PER_PATH)
            finally:
                table.free()
            want = open(tmp_path / "containers_haplotype.txt", "rb").read()
            assert len(want.splitlines()) == P + 2 and got["bytes"] in want and open(tmp_path / "text_haplotype.txt", "rb").read() == want
        finally:
            prepared.free()
    finally:
        engine.close()
