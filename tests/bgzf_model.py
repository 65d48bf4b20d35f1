"""BGZF as a reader sees it, in plain Python: the walk over the members of a byte string that holds every member to the format the
GPU's members promise (include/rpvg_text.h, rpvg_amd/csrc/text_deflate_plan.hpp).  tests/test_bgzf_model.py pins it to a file built
with zlib and struct, to the end-of-file constant and to one broken member per check."""
import struct
import zlib

CHUNK_BYTES = 65280
MAX_MEMBER_BYTES = 65536
HEADER = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00])  # then BSIZE
EOF_BLOCK = bytes([0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00, 0x03, 0x00,
                   0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00])


class BgzfError(ValueError):
    pass


def members(data: bytes):
    """[(offset, member bytes, inflated bytes), ...] of a byte string that is nothing but BGZF members; BgzfError otherwise."""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 26:
            raise BgzfError(f"{len(data) - at} bytes behind the last member at {at}")
        for i, want in enumerate(HEADER):
            if data[at + i] != want:
                raise BgzfError(f"member at {at}: header byte {i} is {data[at + i]:#x}, not {want:#x}")
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        if size > MAX_MEMBER_BYTES or size < 26 or at + size > len(data):
            raise BgzfError(f"member at {at}: BSIZE + 1 = {size} with {len(data) - at} bytes left")
        member = data[at:at + size]
        inflater = zlib.decompressobj(-15)
        try:
            text = inflater.decompress(member[18:size - 8])
        except zlib.error as e:
            raise BgzfError(f"member at {at}: {e}")
        if not inflater.eof or inflater.unused_data:
            raise BgzfError(f"member at {at}: the stream ends {'early' if inflater.unused_data else 'late'}")
        if len(text) > CHUNK_BYTES:
            raise BgzfError(f"member at {at}: {len(text)} bytes of text")
        crc, isize = struct.unpack_from("<II", member, size - 8)
        if crc != zlib.crc32(text) or isize != len(text):
            raise BgzfError(f"member at {at}: trailer ({crc:#x}, {isize}) for ({zlib.crc32(text):#x}, {len(text)})")
        out.append((at, member, text))
        at += size
    return out


def text_of(data: bytes) -> bytes:
    return b"".join(text for _, _, text in members(data))


def first_block_type(member: bytes) -> int:
    """BTYPE of the first block of a member: 0 stored, 1 fixed codes, 2 dynamic codes."""
    return (member[18] >> 1) & 3
