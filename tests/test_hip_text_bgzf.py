"""A text as BGZF on the GPU (rpvg_amd/csrc/text_deflate.hip, include/rpvg_text.h) against the reader's model of
tests/bgzf_model.py, which tests/test_bgzf_model.py pins to zlib: every member is held to the format, the members inflate to the
input byte for byte, and the bytes are those of the host's model of the kernel (rpvg_amd/csrc/text_deflate_plan.hpp: modelMembers,
which tests/cpp/text_deflate_plan_check.cpp holds to zlib's inflate).  The bounds on sizes follow from the format or from zlib on
the same chunks: Huffman coding alone brings uniformly random digits and tabs to 0.454 of their size and fixed codes to 0.70, so
0.50 shows dynamic codes; zlib needs 80 to 416 bytes for a chunk of one byte, so 1 024 shows matches of full length."""
import gzip

import numpy as np
import pytest

from rpvg_amd import hip
from rpvg_amd.estimates_table import EstimatesTable, FlatEstimates
from rpvg_amd.gibbs_table import FlatGibbs, GibbsTable
from rpvg_amd.table_text import HAPLOTYPE, JOINT, PER_PATH, ROWS, BgzfText, HarnessTableText, Labels, RowsInput, TableText, bgzf_bytes, bgzf_model
from tests import bgzf_model as B
from tests import estimates_table_model as EM
from tests import gibbs_table_model as GM
from tests import rows_text_model as R
from tests import set_text_model as S
from tests import table_text_model as M

pytestmark = pytest.mark.gpu

CHUNK = B.CHUNK_BYTES
SIZES = [0, 1, 2, 3, 4, 257, 258, 259, 260, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def fibonacci_chunk():
    """The plan check's counts over 22 symbols, 46 367 bytes, shuffled: an unlimited code would be 21 bits deep."""
    counts, a, b = [], 1, 1
    for _ in range(22):
        counts.append(a)
        a, b = b, a + b
    data = np.repeat(np.arange(40, 40 + 3 * 22, 3, dtype=np.uint8), counts)
    np.random.default_rng(22).shuffle(data)
    assert len(data) == 46367
    return data.tobytes()


def far_repeats():
    """One chunk of random digits and tabs (random filler that still takes a dynamic block) with 300 of its bytes again 32 768 bytes
    later, the longest distance there is, and another 300 again 32 769 bytes later, one too far: no match may reach those."""
    rng = np.random.default_rng(300)
    text = bytearray(np.frombuffer(b"0123456789\t", dtype=np.uint8)[rng.integers(0, 11, size=CHUNK)].tobytes())
    text[32768:32768 + 300] = text[0:300]
    text[400 + 32769:400 + 32769 + 300] = text[400:700]
    return bytes(text)


def straddling_repeat():
    """The same 300 bytes at the start and across byte 65 280: a match that would run past the end of its chunk."""
    rng = np.random.default_rng(301)
    piece = rng.integers(48, 58, size=300, dtype=np.uint8).tobytes()
    text = bytearray(rng.integers(97, 123, size=CHUNK + 400, dtype=np.uint8).tobytes())
    text[100:400] = piece
    text[CHUNK - 150:CHUNK + 150] = piece
    text[CHUNK + 150:CHUNK + 400] = piece[:250]
    return bytes(text)


def contents():
    rng = np.random.default_rng(77)
    longest = max(SIZES)
    scalable = {
        "one byte": b"7" * longest,
        "period two": b"0\t" * (longest // 2 + 1),
        "period three": b"0.\t" * (longest // 3 + 1),
        "all byte values": bytes(range(256)) * (longest // 256 + 1),
        "random bytes": rng.integers(0, 256, size=longest, dtype=np.uint8).tobytes(),
        "digits and tabs": np.frombuffer(b"0123456789\t", dtype=np.uint8)[rng.integers(0, 11, size=longest)].tobytes(),
    }
    cases = [(name, data[:n]) for name, data in scalable.items() for n in SIZES]
    cases += [("Fibonacci counts", fibonacci_chunk()), ("far repeats", far_repeats()), ("straddling repeat", straddling_repeat())]
    return cases


CASES = contents()
NAMES = sorted({name for name, _ in CASES}, key=[name for name, _ in CASES].index)


def check_members(bgzf, data):
    """The members of a BgzfText against the reader's model, the input and the host's model of the kernel; returns (view, walk)."""
    got = bgzf.view()
    walked = B.members(got["bytes"])
    assert b"".join(t for _, _, t in walked) == data
    assert got["num_members"] == len(walked) == (len(data) + CHUNK - 1) // CHUNK and got["num_text_bytes"] == len(data) and got["num_bytes"] == len(got["bytes"])
    assert got["member_off"].tolist() == [at for at, _, _ in walked] + [len(got["bytes"])]
    for i, (_, member, text) in enumerate(walked):
        assert text == data[i * CHUNK:(i + 1) * CHUNK] and len(member) <= len(text) + 31
        assert B.first_block_type(member) in (0, 2)
    assert got["num_stored_members"] == sum(B.first_block_type(m) == 0 for _, m, _ in walked)
    want = bgzf_model(data)
    if got["bytes"] != want["bytes"]:
        at = next((i for i in range(min(len(want["bytes"]), len(got["bytes"]))) if got["bytes"][i] != want["bytes"][i]), None)
        raise AssertionError(f"{len(got['bytes'])} bytes, the host's model {len(want['bytes'])}; they differ from byte {at}")
    assert got["num_stored_members"] == want["num_stored_members"]
    assert bgzf.guards_intact()
    return got, walked


@pytest.mark.parametrize("name", NAMES)
def test_contents_at_every_size(hip_ctx, name):
    for case, data in CASES:
        if case != name:
            continue
        bgzf = bgzf_bytes(hip_ctx, data)
        try:
            got, walked = check_members(bgzf, data)
        finally:
            bgzf.free()
        print(f"{name}: {len(data)} bytes -> {got['num_bytes']} in {got['num_members']} members, {got['num_stored_members']} stored")
        full = [(m, t) for _, m, t in walked if len(t) == CHUNK]
        if name == "random bytes":   # nothing to gain: every chunk of a few hundred bytes or more is stored
            assert all(B.first_block_type(m) == 0 and len(m) == len(t) + 31 for _, m, t in walked if len(t) >= 257)
            assert got["num_stored_members"] >= sum(len(t) >= 257 for _, _, t in walked)
        if name == "one byte":
            assert all(len(m) <= 1024 and B.first_block_type(m) == 2 for m, _ in full)
        if name == "digits and tabs":
            assert all(len(m) <= 0.50 * CHUNK and B.first_block_type(m) == 2 for m, _ in full)


def test_two_builds_and_host_and_device_memory_give_the_same_bytes(hip_ctx):
    data = next(d for name, d in CASES if name == "digits and tabs" and len(d) == 2 * CHUNK + 1)[:CHUNK + 4001] + far_repeats()[:40000]
    pointer = hip_ctx.malloc(len(data) + 8)
    try:
        hip_ctx.h2d(pointer, np.frombuffer(b"\xee" + data, dtype=np.uint8))   # an odd address: the library takes any
        builds = [bgzf_bytes(hip_ctx, data), bgzf_bytes(hip_ctx, data), bgzf_bytes(hip_ctx, None, device_pointer=pointer + 1, num_bytes=len(data))]
        try:
            views = [check_members(b, data)[0] for b in builds]
            assert views[0]["bytes"] == views[1]["bytes"] == views[2]["bytes"]
            assert views[0]["member_off"].tolist() == views[1]["member_off"].tolist() == views[2]["member_off"].tolist()
        finally:
            for b in builds:
                b.free()
    finally:
        hip_ctx.free(pointer)


def test_ranges_that_split_a_member_and_a_header(hip_ctx):
    data = next(d for name, d in CASES if name == "period three" and len(d) == 2 * CHUNK + 1)
    bgzf = bgzf_bytes(hip_ctx, data)
    try:
        got, _ = check_members(bgzf, data)
        n, second = got["num_bytes"], int(got["member_off"][1])
        for begin, end in ((0, n), (1, n - 1), (7, 7), (n, n), (second - 5, second + 9), (second + 3, second + 4), (second + 17, n - 2), (0, 18)):
            assert bgzf.bytes(begin, end) == got["bytes"][begin:end]
    finally:
        bgzf.free()


def test_refusals_leave_a_usable_context(hip_ctx):
    data = b"Name\tClusterID\n" * 500

    def valid_build():
        bgzf = bgzf_bytes(hip_ctx, data)
        try:
            check_members(bgzf, data)
        finally:
            bgzf.free()

    bgzf = bgzf_bytes(hip_ctx, data)
    try:
        n = bgzf.view()["num_bytes"]
        for begin, end in ((0, n + 1), (n + 1, n + 1), (5, 4), (n, 0)):   # outside the bytes, reversed
            with pytest.raises(hip.EngineError, match=r"\(-3\).*rpvg_hip_text_bgzf_get: bytes"):
                bgzf.bytes(begin, end)
            valid_build()
    finally:
        bgzf.free()
    freed = bgzf   # its handle is gone: a NULL handle reaches the library
    for call in (freed.view, lambda: freed.bytes(0, 1), freed.guards_intact, lambda: TableText(None).bgzf(), lambda: BgzfText(None).view()):
        with pytest.raises(hip.EngineError, match=r"\(-3\).*NULL argument"):
            call()
        valid_build()
    with pytest.raises(hip.EngineError, match=r"\(-3\).*rpvg_hip_bytes_bgzf: NULL argument"):
        bgzf_bytes(hip_ctx, None, num_bytes=5)
    valid_build()
    empty = bgzf_bytes(hip_ctx, None, num_bytes=0)   # no bytes: not an error
    try:
        got = empty.view()
        assert (got["num_members"], got["num_bytes"], got["num_text_bytes"], got["bytes"], got["member_off"].tolist()) == (0, 0, 0, b"", [0]) and empty.guards_intact()
    finally:
        empty.free()


# ---- through the layers: the texts of the five builders ------------------------------------------------------------------------------------

def check_text(text):
    """A resident text of any builder: its members give its bytes back."""
    plain = text.view()["bytes"]
    bgzf = text.bgzf()
    try:
        check_members(bgzf, plain)
        assert text.view()["bytes"] == plain and text.guards_intact()   # the text stays as it is
    finally:
        bgzf.free()
    return plain


def test_a_gibbs_text(hip_ctx):
    rng = np.random.default_rng(64)
    N = 65
    rows = [[None if g == 1 else M.sample_values(rng, N) for g in range(3)], [M.sample_values(rng, N) for _ in range(2)]]
    clusters = M.gibbs_clusters(rows, N)
    table = GibbsTable.build(hip_ctx, FlatGibbs(**GM.flatten(clusters, N)))
    try:
        text = TableText.gibbs(hip_ctx, table, Labels.of(M.names_of_lengths([7, 2, 0, 11, 5]), [1, 4000000000]))
        try:
            assert check_text(text).count(b"\n") == 4
        finally:
            text.free()
    finally:
        table.free()


def per_path_cluster(rng, n, eff):
    return dict(num_paths=n, sets=[(i,) for i in range(n)], posteriors=[1.0] * n, abundances=[0.0 if i % 5 == 1 else float(x) for i, x in enumerate(rng.gamma(0.8, 30.0, size=n))],
                noise_count=float(rng.random()), eff=eff)


@pytest.mark.parametrize("kind", [PER_PATH, HAPLOTYPE])
def test_an_estimates_text(hip_ctx, kind):
    rng = np.random.default_rng(12)
    clusters = [per_path_cluster(rng, 1, [812.25]), per_path_cluster(rng, 2, [1e-7, 123456789.0]), per_path_cluster(rng, 0, []),
                per_path_cluster(rng, 70, [float(x) for x in rng.gamma(2.0, 400.0, size=70)])]
    P = sum(c["num_paths"] for c in clusters)
    names, lengths = M.names_of_lengths([(3 * i) % 14 for i in range(P)], seed=3), [int(x) for x in rng.integers(1, 2 ** 32, size=P)]
    flat = FlatEstimates(**EM.flatten(clusters))
    model = EM.table(clusters, 2)
    table = EstimatesTable.build(hip_ctx, None, flat, 2)
    try:
        table.tpm(model["total_transcript_count"])
        text = TableText.estimates(hip_ctx, table, flat.as_c(), Labels.of(names, [3, 1, 4, 1000000], lengths), kind)
        try:
            assert len(check_text(text)) > 0
        finally:
            text.free()
    finally:
        table.free()


def test_a_set_text(hip_ctx):
    rng = np.random.default_rng(103)
    clusters = [S.every_size_cluster(3, 9, rng), S.cluster_of_sets([], [], 0, rng), S.every_size_cluster(3, 8, rng)]
    P = sum(c["num_paths"] for c in clusters)
    names = M.names_of_lengths([S.NAME_LENGTHS[i % len(S.NAME_LENGTHS)] for i in range(P)], seed=0)
    flat = FlatEstimates(**EM.flatten(clusters))
    table = EstimatesTable.build(hip_ctx, None, flat, 3)
    try:
        table.tpm(1.0)
        text = TableText.sets(hip_ctx, table, flat.as_c(), Labels.of(names, [3, 1, 12]), JOINT, 3, 0.0)
        try:
            assert check_text(text).count(b"\n") == sum(len(c["sets"]) for c in clusters)
        finally:
            text.free()
    finally:
        table.free()


def rows_case():
    rng = np.random.default_rng(13)
    clusters = [dict(num_paths=9, rows=[R.row_of_cells(int(n), rng, 9, count=int(n)) for n in rng.integers(2, 40, size=60)]), dict(num_paths=0, rows=[]),
                dict(num_paths=70, rows=[R.row_of_cells(int(n), rng, 70) for n in rng.integers(2, 150, size=30)])]
    P = sum(c["num_paths"] for c in clusters)
    names = M.names_of_lengths([(5 * i) % 23 for i in range(P)], seed=13)
    lengths, eff = [int(x) for x in rng.integers(0, 100000, size=P)], [float(x) for x in rng.gamma(2.0, 400.0, size=P)]
    return R.flatten(clusters), names, lengths, eff, [5, 6, 7], [0, 2 ** 64 - 1, 9]


def test_a_rows_text(hip_ctx):
    flat, names, lengths, eff, lists, index = rows_case()
    want_bytes, _ = R.rows_text(flat, names, lengths, eff, 1e-12, lists, index)
    text = TableText.rows(hip_ctx, RowsInput.of(flat, eff, lists, index), Labels.of(names, [1, 2, 3], lengths), 1e-12)
    try:
        assert check_text(text) == want_bytes
    finally:
        text.free()


def test_the_files_of_the_writers(tmp_path):
    """HarnessTableText.write(compressed=True): the --write-probs dump through writeProbabilityClustersBgzf and the Gibbs file through
    ReadCountGibbsSamplesWriter::addCompressedText end in the end-of-file block, are nothing but members, and gzip reads from them the
    bytes it reads from the files the same writers write without it; the estimates files have no such route."""
    from rpvg_amd import engine as eng_mod
    from rpvg_amd.batch import ClusterBatch, make_params
    from rpvg_amd.gibbs_table import HarnessGibbsTable
    from tests import small_cases

    def check_files(compressed, plain):
        data = open(compressed, "rb").read()
        assert data.endswith(B.EOF_BLOCK) and B.members(data)[-1][2] == b""
        assert gzip.open(compressed, "rb").read() == gzip.open(plain, "rb").read() == B.text_of(data)
        return data

    engine = eng_mod.Engine(0)
    try:
        flat, names, lengths, eff, lists, index = rows_case()
        dump = HarnessTableText(engine, RowsInput.of(flat, eff, lists, index), kind=ROWS, labels=Labels.of(names, [1, 2, 3], lengths), prob_precision=1e-12)
        try:
            dump.write(str(tmp_path / "probs_plain.txt.gz"))
            dump.write(str(tmp_path / "probs_bgzf.txt.gz"), compressed=True)
            members = dump.bgzf()
            assert check_files(tmp_path / "probs_bgzf.txt.gz", tmp_path / "probs_plain.txt.gz") == members["bytes"] + B.EOF_BLOCK
            assert members["num_text_bytes"] == dump.view()["num_bytes"] and B.text_of(members["bytes"]) == dump.view()["bytes"]
        finally:
            dump.free()
        N = 3
        batch = ClusterBatch.from_clusters(small_cases.make_batch_clusters(4242, n_clusters=8, with_empty=True))
        prepared = engine.prepare(batch)
        try:
            engine.run("haplotype-transcripts", make_params(num_gibbs_samples=N), prepared)
            gibbs = HarnessGibbsTable(engine, prepared, N)
            try:
                text = HarnessTableText(engine, gibbs)
                try:
                    text.write(str(tmp_path / "plain_gibbs"), num_gibbs_samples=N, unaligned_read_count=9)
                    text.write(str(tmp_path / "bgzf_gibbs"), num_gibbs_samples=N, unaligned_read_count=9, compressed=True)
                    rows = text.view()["bytes"]
                finally:
                    text.free()
            finally:
                gibbs.free()
            walked = B.members(check_files(tmp_path / "bgzf_gibbs.txt.gz", tmp_path / "plain_gibbs.txt.gz"))
            assert walked[0][2].startswith(b"Name\tClusterID") and walked[0][2].count(b"\n") == 1    # the header row, framed on the host
            assert b"".join(t for _, _, t in walked[1:-2]) == rows and len(rows) > 0                   # the device's members
            assert walked[-2][2].startswith(b"Unknown\t0\t") and walked[-2][2].count(b"\n") == 1      # the Unknown row, framed on the host
        finally:
            prepared.free()
    finally:
        engine.close()
