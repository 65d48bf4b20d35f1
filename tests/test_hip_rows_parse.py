"""The --write-probs dump read on the GPU (rpvg_amd/csrc/rows_parse.hip; rpvg_hip_text_rows, rpvg_hip_table_text_rows and the
rpvg_hip_parsed_dump_* of include/rpvg_hip.h) against the plain-Python model of tests/rows_parse_model.py, which
tests/test_rows_parse_model.py pins to hand-written texts, to readProbabilityClusters and to the writer's model.  Every array, the
names and cluster_path_off are compared byte for byte: there is no tolerance.  The texts are those of tests/rows_parse_cases.py."""
import gzip

import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.table_text import Labels, RowsInput, TableText, harness_parse, harness_parse_file, host_line_parse, parse_rows
from tests import rows_parse_cases as cases
from tests import rows_parse_model as P
from tests import rows_text_model as R

pytestmark = pytest.mark.gpu


def arrays_of(ctx, dump) -> dict:
    return {**dump.rows_view(ctx), **dump.view()}


def check(ctx, text, prob_precision=1e-8):
    """The parse of host bytes against the model's; returns the model's arrays."""
    want = P.parse(text)
    dump = parse_rows(ctx, text, prob_precision=prob_precision)
    try:
        assert P.same(arrays_of(ctx, dump), want) == []
    finally:
        dump.free()
    return want


@pytest.mark.parametrize("prob_precision", [1e-8, 1e-12, 1e-17])
def test_shapes_of_the_rows_text_bare_and_ranked_markers_mixed(hip_ctx, prob_precision):
    want = check(hip_ctx, cases.shapes(prob_precision), prob_precision)
    assert set(want["has_rank_key"].tolist()) == {0, 1} and want["row_count"].max() == cases.U32_MAX and len(want["cluster_row_off"]) == 2 + 5 + 20 + 1 + 1


def test_every_residue(hip_ctx):
    """The first name grows from 1 to 130 bytes: every later token starts at every offset of a 64-byte unit and straddles it."""
    for n in range(1, 131):
        want = check(hip_ctx, cases.residue(n))
        assert int(want["name_off"][1]) == n


def test_long_names_rows_and_cells(hip_ctx):
    """A 4000-byte name, 1000 indices in one group, rows of 70 and 129 groups, 64 rows of the longest cells back to back."""
    rng = np.random.default_rng(3)
    want = check(hip_ctx, cases.text_of([dict(num_paths=2, rows=[(1, 0.5, [(0.5, [1])])])], names=[b"x" * 4000, b"y"]))
    assert want["name_off"].tolist() == [0, 4000, 4001]
    want = check(hip_ctx, cases.text_of([dict(num_paths=100000, rows=[(1, 0.5, [(0.5, [int(x) for x in rng.integers(0, 100000, size=1000)])])])], name_lengths=(1,)))
    assert want["grp_idx_off"].tolist() == [0, 1000]
    for groups in (70, 129):
        row = (1, 0.5, sorted((float(p), [int(rng.integers(0, 5))]) for p in rng.random(groups)))
        want = check(hip_ctx, cases.text_of([dict(num_paths=5, rows=[(2, 0.25, []), row, (3, 1.0, [(0.5, [4])])])], 1e-12), 1e-12)
        assert want["row_grp_off"].tolist() == [0, 0, groups, groups + 1]
    want = check(hip_ctx, cases.long_cells(), 1e-17)
    assert len(want["row_count"]) == 64 and len(want["grp_prob"]) == 64 * 64


@pytest.mark.parametrize("name", list(cases.STRUCTURE))
def test_structure(hip_ctx, name):
    want = check(hip_ctx, cases.STRUCTURE[name])
    if name in ("empty text", "only empty lines"):
        assert want["cluster_row_off"].tolist() == [0]
    if name == "no paths: marker then marker":
        assert want["cluster_path_off"].tolist() == [0, 0, 1, 1, 1] and want["has_rank_key"].tolist() == [0, 0, 1, 1]
    if name == "paths and no rows":
        assert want["cluster_row_off"].tolist() == [0, 0, 1, 1] and want["cluster_path_off"].tolist() == [0, 2, 3, 4]


@pytest.mark.parametrize("name", list(cases.GROUP_ORDER))
def test_group_order(hip_ctx, name):
    """The groups leave in the order of the model's sorted(); the text differs from its own re-print (tests/test_rows_parse_model.py),
    so an identity would fail here."""
    text = cases.GROUP_ORDER[name]
    want = check(hip_ctx, text)
    assert P.print_back(want) != text


def test_hard_tokens_and_the_counter(hip_ctx):
    """The hard tokens of tests/cpp/number_parse_check.cpp as effective lengths, probabilities and noise cells.  rpvg_hip_parse_stats
    counts the four exact ties, twice each (docs/design/kernels-rows-clusters.md: only a token within 2^-73 relative of the middle of
    two doubles goes the slow way), and nothing of a text without one."""
    hip_ctx.reset_stats()
    check(hip_ctx, cases.shapes(1e-17), 1e-17)
    assert hip_ctx.parse_stats()["exact_tokens"] == 0
    want = check(hip_ctx, cases.hard_token_text(), 1e-17)
    assert hip_ctx.parse_stats()["exact_tokens"] == 2 * len(cases.SLOW)
    assert want["path_effective_length"][4] == 1.7976931348623157e308 and want["row_noise"][0] == 5e-324
    last = len(cases.HARD_NOISE) - 1  # ...445e-1 lies above the middle of 1 - 2^-53 and 1, ...444e-1 below it
    assert want["row_noise"][last] == 1.0 - 2.0 ** -53 and want["row_noise"][last - 1] == 1.0


def test_a_megabyte_and_two_parses_from_host_and_device_memory(hip_ctx):
    """About 70 000 lines and 1 MB, so every scan runs more than one tile; the same text from device memory; two parses give equal
    bytes."""
    text = cases.big_text()
    assert text.count(b"\n") > 65000 and len(text) > 900000
    want = check(hip_ctx, text)
    pointer = hip_ctx.malloc(len(text))
    try:
        hip_ctx.h2d(pointer, np.frombuffer(text, dtype=np.uint8))
        views = []
        for _ in range(2):
            dump = parse_rows(hip_ctx, None, device_pointer=pointer, num_bytes=len(text))
            try:
                views.append(arrays_of(hip_ctx, dump))
            finally:
                dump.free()
        assert P.same(views[0], want) == [] and P.same(views[1], views[0]) == []
    finally:
        hip_ctx.free(pointer)


@pytest.mark.parametrize("prob_precision", [1e-8, 1e-17])
def test_text_in_text_out_and_the_batch(hip_ctx, prob_precision):
    """A text resident on the GPU -> rpvg_hip_table_text_rows -> rpvg_hip_read_rows_text with the dump's device labels: the model's print
    of the model's parse.  rpvg_hip_read_rows_to_batch on the parsed rows: the batch whose rows are the arrays."""
    clusters = cases.random_clusters(31, 300)
    n = sum(c["num_paths"] for c in clusters)
    rng = np.random.default_rng(32)
    names, lengths, eff = [b"q%d" % i for i in range(n)], [int(x) for x in rng.integers(0, 100000, size=n)], [float(x) for x in rng.gamma(2.0, 400.0, size=n)]
    K = len(clusters)
    lists, index = list(range(100, 100 + K)), list(range(K))
    first = TableText.rows(hip_ctx, RowsInput.of(R.flatten(clusters), eff, lists, index), Labels.of(names, list(range(K)), lengths), prob_precision)
    try:
        text = first.view()["bytes"]
        want = P.parse(text)
        dump = first.parse(prob_precision)
        try:
            assert P.same(arrays_of(hip_ctx, dump), want) == []
            again = dump.text(hip_ctx, prob_precision)
            try:
                assert again.view()["bytes"] == P.print_back(want, prob_precision) and again.guards_intact()
                if prob_precision == 1e-17:
                    assert again.view()["bytes"] == text
            finally:
                again.free()
            batch = dump.to_batch(hip_ctx)
            try:
                got = batch.rows()
                sizes = np.diff(want["grp_idx_off"].astype(np.int64))
                row_of_group = np.repeat(np.arange(len(want["row_count"])), np.diff(want["row_grp_off"].astype(np.int64)))
                ent_off = np.zeros(len(want["row_count"]) + 1, dtype=np.uint64)
                np.add.at(ent_off, row_of_group + 1, sizes.astype(np.uint64))
                assert got["row_ent_off"].tolist() == np.cumsum(ent_off).tolist()
                assert got["ent_path"].tobytes() == want["path_idx"].tobytes() and got["ent_prob"].tobytes() == np.repeat(want["grp_prob"], sizes).tobytes()
                assert got["row_noise"].tobytes() == want["row_noise"].tobytes() and got["row_count"].tolist() == want["row_count"].tolist()
            finally:
                batch.free()
        finally:
            dump.free()
    finally:
        first.free()


@pytest.mark.parametrize("text", list(cases.REFUSALS))
def test_refusals(hip_ctx, text):
    """The line and the reason are the model's (of two offending lines the smaller, of two reasons on it the smaller), the status
    is RPVG_HIP_ERR_INVALID, and a valid parse on the same context follows."""
    line, why = cases.REFUSALS[text]
    with pytest.raises(hip.EngineError, match=r"\(-3\)") as refused:
        parse_rows(hip_ctx, text)
    assert f"line {line}: {P.REASONS[why]}" in str(refused.value)
    check(hip_ctx, cases.STRUCTURE["one cluster"])


def test_refused_before_anything_is_queued(hip_ctx):
    for prob_precision in (0.0, 1.0, 1e-18):
        with pytest.raises(hip.EngineError, match=r"\(-3\)"):
            parse_rows(hip_ctx, b"#\n", prob_precision=prob_precision)
    with pytest.raises(hip.EngineError, match="2\\^31 - 1"):
        parse_rows(hip_ctx, None, device_pointer=8, num_bytes=2 ** 31 - 1)


@pytest.mark.parametrize("suffix", [".txt", ".txt.gz"])
def test_the_host_class_on_a_written_file(tmp_path, suffix):
    """readProbabilityClustersDevice and readProbabilityClusters, flattened, on a file of write_batch_files, plain and gzipped; the
    device parse through rpvg_amd::ParsedDump against the host line on its text."""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd import io as io_mod
    from rpvg_amd.batch import ClusterBatch
    from tests import small_cases

    batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(77, n_clusters=40, with_empty=True))
    probs = str(tmp_path / ("probs" + suffix))
    io_mod.write_batch_files(batch, probs, str(tmp_path / "info.tsv"), 1e-12, num_align_lists=list(range(5, 5 + batch.num_clusters)), cluster_index=list(range(batch.num_clusters)))
    engine = eng_mod.Engine(0)
    try:
        device, host = harness_parse_file(engine, probs, 1e-12, True), harness_parse_file(None, probs, 1e-12, False)
        assert P.same(device, host) == [] and len(host["row_count"]) > 0
        text = (gzip.open(probs) if suffix.endswith(".gz") else open(probs, "rb")).read()
        assert P.same(harness_parse(engine, text, 1e-12), host_line_parse(text, 1e-12)) == [] and P.same(device, P.parse(text)) == []
    finally:
        engine.close()
