"""Patch the inflated bytes of a BAM in place and cut them into the same
blocks again: the patched file's records keep their virtual offsets (as long
as no block_size changes).  Shared by the tests that break single fields."""
import struct
import zlib

import orc


def recompress(stream, u: bytes) -> bytes:
    """The stream's blocks re-cut from new inflated bytes u (zlib level 5):
    a valid BGZF file carrying whatever records u holds."""
    out = bytearray()
    for b in stream.blocks:
        a, n = int(b["ustart"]), int(b["isize"])
        raw = bytes(u[a:a + n])
        co = zlib.compressobj(5, zlib.DEFLATED, -15)
        c = co.compress(raw) + co.flush()
        total = 18 + len(c) + 8
        out += bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", total - 1)
        out += c + struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, n)
    return bytes(out)


def patched(data, rec, offset, fmt, value):
    """data with struct.pack(fmt, value) written at byte `offset` of record `rec`."""
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, r = s.decode_all()
    u = bytearray(s.data)
    struct.pack_into(fmt, u, int(r["offset"][rec]) + offset, value)
    return recompress(s, bytes(u))
