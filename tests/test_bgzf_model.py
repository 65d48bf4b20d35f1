"""tests/bgzf_model.py pinned without a GPU (and, through it, the host's model of the GPU's member): to a file this test builds with zlib and struct, to the 28 bytes of BGZF's end-of-file
block, and to one deliberately broken member for every check of the walk, each of which the walk must refuse."""
import gzip
import itertools
import struct
import zlib

import pytest

from tests import bgzf_model as B


def member_of(text: bytes, level: int = 6, stored: bool = False) -> bytes:
    if stored:
        payload = b"\x01" + struct.pack("<HH", len(text), len(text) ^ 0xffff) + text
    else:
        deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = deflater.compress(text) + deflater.flush()
    size = 18 + len(payload) + 8
    return B.HEADER + struct.pack("<H", size - 1) + payload + struct.pack("<II", zlib.crc32(text), len(text))


TEXTS = [b"Name\tClusterID\n", bytes(range(256)) * 255, b"0\t" * 1000, b"x"]


def test_the_walk_reads_a_file_built_with_zlib():
    data = b"".join(member_of(t, level) for t, level in zip(TEXTS, (6, 1, 9, 6))) + member_of(b"stored bytes", stored=True) + B.EOF_BLOCK
    walked = B.members(data)
    assert [t for _, _, t in walked] == TEXTS + [b"stored bytes", b""]
    assert [at for at, _, _ in walked] == [0] + list(itertools.accumulate(len(m) for _, m, _ in walked))[:-1]
    assert B.text_of(data) == b"".join(TEXTS) + b"stored bytes" == gzip.decompress(data)
    assert len(TEXTS[1]) == B.CHUNK_BYTES
    assert [B.first_block_type(m) for _, m, _ in walked[3:5]] == [1, 0] and B.first_block_type(walked[1][1]) == 2
    assert B.members(b"") == []


def test_the_end_of_file_block():
    assert len(B.EOF_BLOCK) == 28 and gzip.decompress(B.EOF_BLOCK) == b""
    assert B.members(B.EOF_BLOCK) == [(0, B.EOF_BLOCK, b"")]
    assert B.EOF_BLOCK == member_of(b"", stored=False)[:18] + b"\x03\x00" + bytes(8)


def broken_members():
    good = member_of(b"0123456789\t" * 50)
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14, 15):
        yield f"header byte {i}", good[:i] + bytes([good[i] ^ 0x40]) + good[i + 1:]
    yield "BSIZE too small", good[:16] + struct.pack("<H", len(good) - 2) + good[18:]
    yield "BSIZE past the end", good[:16] + struct.pack("<H", len(good)) + good[18:]
    yield "a stream that ends early", good[:16] + struct.pack("<H", len(good) + 3) + good[18:-8] + b"\0\0\0\0" + good[-8:]
    yield "a stream that is cut", good[:16] + struct.pack("<H", len(good) - 5) + good[18:-12] + good[-8:]
    yield "a wrong CRC", good[:-8] + bytes([good[-8] ^ 1]) + good[-7:]
    yield "a wrong ISIZE", good[:-4] + bytes([good[-4] ^ 1]) + good[-3:]
    yield "bytes behind the last member", good + b"\x1f\x8b"
    yield "garbage in front", b"\0" + good
    big = bytes(range(256)) * 256  # 65 536 bytes of text in one member of legal size
    yield "more text than a chunk", member_of(big, 9)


@pytest.mark.parametrize("what,data", list(broken_members()), ids=[w for w, _ in broken_members()])
def test_the_walk_refuses(what, data):
    with pytest.raises(B.BgzfError):
        B.members(data)


def test_the_host_model_of_the_kernel_writes_members_the_walk_reads():
    """rpvg_amd.table_text.bgzf_model (rpvg_amd/csrc/text_deflate_plan.hpp: modelMembers), the bytes tests/test_hip_text_bgzf.py holds the
    GPU to: rows of names and numbers over a chunk's edge, a run, and bytes nothing can be gained on."""
    import random

    from rpvg_amd.table_text import bgzf_model

    rng = random.Random(5)
    rows = b"".join(b"transcript_%d_hap%d\t%d" % (rng.randrange(40), r % 5, r // 30) + b"".join(b"\t%.8g" % rng.gammavariate(0.8, 30.0) for _ in range(9)) + b"\n" for r in range(900))
    noise = bytes(rng.randrange(256) for _ in range(3000))
    assert len(rows) > B.CHUNK_BYTES
    for data, stored in ((rows, 0), (b"0" * 70000, 0), (noise, 1), (b"x", 1), (b"", 0)):
        got = bgzf_model(data)
        walked = B.members(got["bytes"])
        assert B.text_of(got["bytes"]) == data and [len(t) for _, _, t in walked] == [len(data[at:at + B.CHUNK_BYTES]) for at in range(0, len(data), B.CHUNK_BYTES)]
        assert got["num_stored_members"] == stored == sum(B.first_block_type(m) == 0 for _, m, _ in walked)
        assert all(len(m) <= len(t) + 31 for _, m, t in walked)
    assert len(bgzf_model(rows)["bytes"]) < 0.5 * len(rows) and len(bgzf_model(b"0" * B.CHUNK_BYTES)["bytes"]) <= 1024
