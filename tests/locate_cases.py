"""Inputs for the anchored BGZF locate (k_bgzf_anchor_walk, k_bgzf_link,
k_bgzf_seg_emit under Pipeline::locate_range) and a pure-Python model of it.

The locate cuts a range [lo, hi) whose lo is a block start into segments of S
bytes, finds one anchor per segment (the first header match whose successor
matches too; lo itself for segment 0), walks BSIZE from every anchor to its
segment's end, and checks that each walk's exit is the next non-empty
segment's anchor.  It either produces the table the serial walk from lo would
produce or declines, and the full scan then locates the range.

A case is a small file (tens to hundreds of KB, deterministic) aimed at one
way this can go wrong, with the path it must take at each segment size:
"anchored", or "declined" for a stated reason:
  header  a walk step stands on bytes that are not a block header
  link    a walk's exit is not the next non-empty segment's anchor
  tail    the chain ends neither at hi nor at a cut block under `partial`
  cap     more blocks than the candidate capacity
test_locate_cases.py proves these from the model (no GPU); test_gpu_locate.py
runs the cases on the GPU.  Builders: hbam.synth (a BAM's inflated stream),
plain zlib, and tests/golden/test.bam.
"""
import collections
import functools
import os
import struct
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAGIC = b"\x1f\x8b\x08\x04"
S_SMALL, S_MID, S_DEFAULT = 4096, 65536, 512 << 10  # S_DEFAULT: kLocateSegBytes (hbam_pipeline.h)
SIZES = (S_SMALL, S_MID, S_DEFAULT)
MAX_STORED = 65536 - 18 - 8 - 5  # payload of a stored block of the maximum compressed size

# name; file bytes; bam (else plain BGZF); expect: S -> "anchored" | reason; cap_limit (0: the library's own)
Case = collections.namedtuple("Case", "name data bam expect cap_limit")


# ----------------------------------------------------------------- blocks ----

def block(raw, level=5, sub=b"BC"):
    """One BGZF block holding raw (level 0: one stored DEFLATE block, written
    here so that its size does not depend on the zlib at hand)."""
    if level == 0:
        c = b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        c = co.compress(raw) + co.flush()
    total = 18 + len(c) + 8
    assert total <= 65536
    return (MAGIC + b"\0\0\0\0\0\xff\x06\0" + sub + b"\x02\0" + struct.pack("<H", total - 1) + c +
            struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw)))


EMPTY = block(b"")  # the 28-byte ISIZE-0 block (the EOF marker)


def block_starts(data):
    """The serial BSIZE walk over a whole file."""
    p, out = 0, []
    while p < len(data):
        out.append(p)
        p += struct.unpack_from("<H", data, p + 16)[0] + 1
    assert p == len(data)
    return out


@functools.lru_cache(maxsize=None)
def bam_stream(n_records=3000):
    """The inflated stream (header + records) of a synthetic BAM."""
    from hbam import synth
    data, _ = synth.make_bam(n_records, threads=1)
    out = []
    for p in block_starts(data):
        bs = struct.unpack_from("<H", data, p + 16)[0] + 1
        out.append(zlib.decompressobj(-15).decompress(data[p + 18:p + bs - 8]))
    return b"".join(out)


class Builder:
    """A BGZF file cut from a payload, block by block."""

    def __init__(self, payload):
        self.payload, self.at, self.out = payload, 0, bytearray()

    def take(self, n):
        raw = self.payload[self.at:self.at + n]
        assert len(raw) == n, "payload exhausted"
        self.at += n
        return raw

    def z(self, n, level=5, sub=b"BC"):
        self.out += block(self.take(n), level, sub)
        return self

    def z_until(self, offset, n=12000, level=5):
        """Compressed blocks of n bytes while the file is shorter than offset."""
        while len(self.out) < offset:
            self.z(n, level)
        return self

    def align(self, offset):
        """A stored block sized so that the next block starts at offset."""
        n = offset - len(self.out) - 31
        assert 0 <= n <= MAX_STORED, n
        self.out += block(self.take(n), 0)
        assert len(self.out) == offset
        return self

    def raw(self, b):
        self.out += b
        return self

    def finish(self, n=30000, eof=True):
        while self.at < len(self.payload):
            self.z(min(n, len(self.payload) - self.at))
        if eof:
            self.out += EMPTY
        return bytes(self.out)


# ------------------------------------------------------------------ model ----

def header_at(d, p, hi):
    """The scan's 16-byte header test at p plus a BSIZE that holds a block:
    the total block size, or 0."""
    if p + 18 > hi or d[p:p + 4] != MAGIC or d[p + 10:p + 16] != b"\x06\0BC\x02\0":
        return 0
    total = struct.unpack_from("<H", d, p + 16)[0] + 1
    return total if total >= 26 else 0


def model(d, lo, hi, partial, S, cap):
    """The anchored locate of [lo, hi): ("anchored", block starts) with a block
    cut by hi as the last start (as the scan emits it), or ("declined",
    reasons).  S == 0: ("scan", None)."""
    if S == 0 or hi <= lo:
        return "scan", None
    nseg = (hi - lo + S - 1) // S
    reasons, segs = set(), []
    for j in range(nseg):
        s0 = lo + j * S
        end = min(s0 + S, hi)
        a = lo if j == 0 else None
        p = s0 - 1
        while a is None:  # anchor: the first match whose successor matches or lies at or past hi
            p = d.find(MAGIC, p + 1, min(end + 3, hi))
            if p < 0 or p >= end:
                break
            t = header_at(d, p, hi)
            if t and (p + t >= hi or header_at(d, p + t, hi)):
                a = p
        if a is None:
            continue
        p, starts = a, []
        while p < end:
            t = header_at(d, p, hi)
            if not t:
                reasons.add("tail" if p + 18 > hi else "header")
                break
            starts.append(p)
            p += t
            if p > hi:
                if not partial:
                    reasons.add("tail")
                break
        segs.append((a, p, starts))
    for (_, e, _), (a, _, _) in zip(segs, segs[1:]):
        if e != a:
            reasons.add("link")
    if segs[-1][1] < hi:
        reasons.add("tail")
    table = [p for _, _, st in segs for p in st]
    if len(table) > cap:
        reasons.add("cap")
    return ("declined", reasons) if reasons else ("anchored", table)


def library_cap(length, cap_limit=0):
    """locate_range's candidate capacity for a range of `length` bytes."""
    cap = min(length // 1024 + 4096, 0x7FFFFFFF)
    return min(cap, cap_limit) if cap_limit else cap


# ------------------------------------------------------------------ cases ----

def _all(path):
    return {s: path for s in SIZES}


def test_bam():
    return open(os.path.join(GOLDEN, "test.bam"), "rb").read()


def _golden():
    return [Case("test_bam", test_bam(), True, _all("anchored"), 0)]


def _boundary():
    """A block start exactly at a segment boundary of both small sizes, one
    byte before one and one byte after one."""
    b = Builder(bam_stream())
    b.z_until(20000).align(65536).z(12000)            # a start at 16 * 4096 = 65536
    b.z_until(90000).align(2 * 65536 - 1).z(12000)    # one byte before 131072
    b.z_until(150000).align(3 * 65536 + 1).z(12000)   # one byte after 196608
    return [Case("boundary", b.finish(), True, _all("anchored"), 0)]


def _max_blocks():
    """Blocks of the maximum compressed size: at S = 4 KiB fifteen consecutive
    segments in each hold no block start."""
    b = Builder(bam_stream())
    b.z(9000)
    for _ in range(3):
        b.z(MAX_STORED, 0)
    return [Case("max_blocks", b.finish(), True, _all("anchored"), 0)]


def _empties():
    """ISIZE-0 blocks: the EOF block (every case), one mid-file, a run of 200;
    the run with the capacity forced below it declines."""
    mid = Builder(bam_stream()).z(30000).z(30000).raw(EMPTY).z(30000).finish()
    run = Builder(bam_stream()).z(30000).z(30000).raw(EMPTY * 200).z(30000).finish()
    return [Case("empty_mid", mid, True, _all("anchored"), 0),
            Case("empty_run", run, True, _all("anchored"), 0),
            Case("empty_run_cap", run, True, _all("cap"), 64)]


def _decoy():
    """A stored block whose payload holds two complete BGZF blocks.  The first
    decoy header is the first header match after the 4 KiB boundary at 8192
    (the stored block starts 100 bytes before it) and its successor is the
    second decoy, so it becomes the segment's anchor; the second decoy runs
    past the segment's end, so the decoy walk leaves its segment cleanly and
    only the link check can tell.  Larger segments hold the whole file."""
    rng_bytes = bytes((i * 37 + 11) % 251 if (i * 37 + 11) % 251 != 0x1F else 7 for i in range(60000))
    d1 = block(b"decoy one")
    d2 = block(rng_bytes[:4200], 0)
    b = Builder(rng_bytes)
    b.z(3000).align(8192 - 100)
    r0 = len(b.out)
    inner = rng_bytes[:8192 + 5 - (r0 + 23)] + d1 + d2 + rng_bytes[:300]
    b.raw(block(inner, 0))
    assert b.out[8197:8201] == MAGIC and b.out.find(MAGIC, 8192) == 8197
    assert 8197 + len(d1) + len(d2) > 8192 + 4096
    b.z(5000).z(5000)
    return [Case("decoy", b.finish(n=5000), False, {S_SMALL: "link", S_MID: "anchored", S_DEFAULT: "anchored"}, 0)]


def _other_subfield():
    """A block whose extra subfield is not BC (XLEN 6 still): the serial walk
    reads it, the scan's header test does not match it.  At 4 KiB it is the
    first block of its segment (the search skips it: the link breaks); in
    larger segments a walk steps on it."""
    b = Builder(bam_stream())
    b.z(30000).z(30000).z(30000, sub=b"XY").z(30000)
    return [Case("other_subfield", b.finish(), True, {S_SMALL: "link", S_MID: "header", S_DEFAULT: "header"}, 0)]


def truncated():
    """A BAM cut in the middle of a block (past its first 64 KiB)."""
    data = Builder(bam_stream()).finish()
    starts = block_starts(data)
    k = max(i for i, p in enumerate(starts) if p < len(data) * 2 // 3)
    return data[:starts[k] + 5000]


def windowed():
    """A BAM of several 64 KiB windows."""
    from hbam import synth
    return synth.make_bam(3000, threads=1)[0]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for f in (_golden, _boundary, _max_blocks, _empties, _decoy, _other_subfield):
        out += f()
    return out
