"""Inflate phase A's two kernels: the lean instance (k_inflate_huff: one
DEFLATE block per round from prebuilt tables, only the round's window of
compressed bits staged) and the fallback (k_huff_fallback: the full body) it
hands every other block to.

Each case builds BGZF blocks from Python's zlib (raw deflate) or hbam.synth,
compares the inflated bytes / the first failing block and its error code with
zlib driven as [htsjdk] BlockGunzipper drives it (one inflate, ISIZE bytes of
room) and with the oracle, and checks through inflate_path_counts() which
kernel decoded the blocks.  The counts are per block and decode round: a BGZF
block of two DEFLATE blocks takes two rounds."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import hbam
import orc
from conftest import ROOT
from hbam import synth
from test_gpu_parity import assert_same_records

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CHUNK_BLOCKS = 65536  # hbam_pipeline.cpp HBAM_INFLATE_CHUNK: blocks per inflate chunk


def bgzf(cdata, payload, isize=None):
    """One BGZF block around raw-deflate bytes."""
    assert len(cdata) + 26 <= 65536
    hdr = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", len(cdata) + 25)
    return hdr + cdata + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload) if isize is None else isize)


def deflate(parts, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush=zlib.Z_BLOCK, zdict=None):
    """Raw deflate of the parts, the DEFLATE block closed after each one
    (`flush`); returns (cdata, [bytes written when each part was flushed])."""
    kw = {} if zdict is None else {"zdict": zdict}
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy, **kw)
    out, marks = b"", []
    for i, p in enumerate(parts):
        out += c.compress(p)
        if i + 1 < len(parts):
            out += c.flush(flush)
            marks.append(len(out))
    return out + c.flush(zlib.Z_FINISH), marks


def letters(rng, n, k=64, lo=32):
    """n bytes drawn evenly from k values: Huffman-compressible, no matches to speak of."""
    return bytes(rng.integers(lo, lo + k, n, dtype=np.uint8))


def texty(rng, n):
    """n bytes with plenty of matches (words of a small vocabulary)."""
    words = [letters(rng, int(rng.integers(3, 12)), 26, 97) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))] + b" "
    return bytes(out[:n])


def gunzip_block(cdata, isize):
    """(status, bytes) of [htsjdk] BlockGunzipper on one block, by zlib."""
    if isize == 0:
        return hbam.OK, b""
    try:
        out = zlib.decompressobj(-15).decompress(cdata, isize)
    except zlib.error:
        return hbam.E_IO, None
    return (hbam.OK, out) if len(out) == isize else (hbam.E_FORMAT, None)


def expected(data):
    """(status, inflated bytes | offset of the first failing block), by zlib."""
    p, out = 0, []
    while p < len(data):
        csize = struct.unpack_from("<H", data, p + 16)[0] + 1
        isize = struct.unpack_from("<I", data, p + csize - 4)[0]
        rc, b = gunzip_block(data[p + 18:p + csize - 8], isize)
        if rc != hbam.OK:
            return rc, p
        out.append(b)
        p += csize
    return hbam.OK, b"".join(out)


def oracle_status(data):
    try:
        orc.Stream(data, check_crc=False, parse_header=False)
        return hbam.OK
    except orc.OracleError as e:
        return e.code


def run(data):
    """(status, bytes | failing offset, (lean, fallback, resident)) on the GPU."""
    with hbam.BamFile(data, bam=False) as f:
        n = int(sum(int(x) for x in f.blocks()["isize"]))
        try:
            got = f.read_inflated(0, n)
        except hbam.HbamError as e:
            m = re.search(r"at offset (\d+)", str(e))
            return e.code, int(m.group(1)) if m else None, f.inflate_path_counts()
        return hbam.OK, got, f.inflate_path_counts()


def check(data, want=None):
    """The GPU result equals zlib's (and the oracle's status); returns the path counts."""
    want = expected(data) if want is None else want
    assert oracle_status(data) == want[0]
    rc, got, counts = run(data)
    assert rc == want[0]
    assert got == want[1]
    return counts


def nonempty(data):
    s = orc.Stream(data, parse_header=False)
    return int(np.count_nonzero(s.blocks["isize"]))


# ---- 1. ordinary data
RESIDENT_CHILD = r"""
import sys
sys.path[:0] = sys.argv[1:3]
import hbam
from hbam import synth
d, _ = synth.make_bam(2000, level=5)
with hbam.BamFile(d, bam=False) as f:
    f.read_inflated(0, int(sum(int(x) for x in f.blocks()["isize"])))
    print(*f.inflate_path_counts())
"""


def test_lean_instance_is_resident_five_per_cu():
    """The runtime's occupancy answer, asked in a child process that loads
    only libhbam.  In the test process other modules import torch, whose own
    copy of the HIP / HSA runtime is then loaded beside libhbam's; once the
    device is initialised with both mapped, the answer is computed from the
    other copy's device properties and reads 4 for the same kernel (measured:
    hbam, then torch, then the first HIP call)."""
    out = subprocess.run([sys.executable, "-c", RESIDENT_CHILD, os.path.join(ROOT, "hadoop-bam_amd"),
                          os.path.join(ROOT, "oracle")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lean, fb, resident = (int(v) for v in out.stdout.split()[-3:])
    assert lean > 0 and fb == 0
    assert resident >= 5


def test_ordinary_reads_run_lean():
    d, _ = synth.make_bam(2000, level=5)
    lean, fb, _ = check(d)
    assert fb == 0
    assert lean >= nonempty(d)
    s = orc.Stream(d)
    rc, want = s.decode_all()
    assert rc == 0
    with hbam.BamFile(d) as f:
        assert_same_records(f.decode_all(), want)
        assert f.inflate_path_counts()[1] == 0


# ---- 2. three or four DEFLATE blocks per BGZF block
def test_third_header_goes_to_the_fallback():
    rng = np.random.default_rng(2)
    blocks = []
    for _ in range(3):
        p = letters(rng, 65280)  # 65,280 literals: four DEFLATE blocks of <= 16,383 symbols
        blocks.append(bgzf(deflate([p])[0], p))
    data = b"".join(blocks) + EOF_BLOCK
    lean, fb, _ = check(data)
    assert lean == 3  # round 0; round 1 ends at a third header and is redone by the fallback
    assert fb == 3


# ---- 3. stored, fixed-Huffman, empty, tiny and single-code blocks
def small_kinds(rng):
    a, b = letters(rng, 3000), texty(rng, 5000)
    return [
        ("stored", bgzf(deflate([a], level=0)[0], a)),
        ("fixed", bgzf(deflate([b], strategy=zlib.Z_FIXED)[0], b)),
        ("empty", bgzf(deflate([b""])[0], b"")),
        ("one byte", bgzf(deflate([b"x"])[0], b"x")),
        ("forty bytes", bgzf(deflate([b[:40]])[0], b[:40])),
        # a dynamic block, then a final one far shorter than one slice per lane
        ("short final", bgzf(deflate([b, b"zq"])[0], b + b"zq")),
        ("single code", bgzf(deflate([b"A" * 30000])[0], b"A" * 30000)),
        ("single code + tail", bgzf(deflate([b"A" * 20000, b"B" * 3])[0], b"A" * 20000 + b"BBB")),
    ]


@pytest.mark.parametrize("k", range(8))
def test_small_kinds_alone(k):
    name, blk = small_kinds(np.random.default_rng(3))[k]
    lean, fb, _ = check(blk + EOF_BLOCK)
    if name in ("stored", "fixed"):
        assert (lean, fb) == (0, 1)
    if name == "empty":
        assert (lean, fb) == (0, 0)


# ---- 4. a round window larger than the lean stage
def test_window_larger_than_the_stage_falls_back():
    rng = np.random.default_rng(4)
    p = letters(rng, 32000, 200, 20)
    q = texty(rng, 4000)
    c1, _ = deflate([p], mem=9)
    assert len(c1) > 28 * 1024  # more than the lean instance can stage
    lean, fb, _ = check(bgzf(c1, p) + EOF_BLOCK)
    assert (lean, fb) == (0, 1)
    c2, _ = deflate([p, q], mem=9)
    lean, fb, _ = check(bgzf(c2, p + q) + EOF_BLOCK)
    assert fb >= 1


# ---- 5. mixed files
def mixed_blocks(rng, big):
    out = [b for _, b in small_kinds(rng)]
    a, t = letters(rng, 6000), texty(rng, 6000)
    out.append(bgzf(deflate([t])[0], t))  # one dynamic block: lean
    out.append(bgzf(deflate([a, t])[0], a + t))  # two: lean, lean
    out.append(bgzf(deflate([a, t, a[:2000]])[0], a + t + a[:2000]))  # three: the third header falls back
    if big:
        p = letters(rng, 65280)
        out.append(bgzf(deflate([p])[0], p))
        p = letters(rng, 32000, 200, 20)
        out.append(bgzf(deflate([p], mem=9)[0], p))
        d, _ = synth.make_bam(1200, level=5, eof_block=False)
        out.append(d)
    return out


def test_mixed_file_one_chunk():
    rng = np.random.default_rng(5)
    kinds = mixed_blocks(rng, True)
    order = [int(i) for i in rng.permutation(len(kinds) * 3) % len(kinds)]
    data = b"".join(kinds[i] for i in order) + EOF_BLOCK
    lean, fb, _ = check(data)
    assert lean > 0 and fb > 0
    assert lean + fb >= nonempty(data)
    with hbam.BamFile(data, bam=False) as f:
        n = int(sum(int(x) for x in f.blocks()["isize"]))
        f.read_inflated(0, n)
        assert 0 < f.inflate_token_count() <= n


def test_mixed_file_two_chunks():
    """More blocks than one inflate chunk holds: the two chunks use the two
    hand-over lists (chunk parity) and overlap."""
    rng = np.random.default_rng(6)
    kinds = mixed_blocks(rng, False)
    tiny = [bgzf(deflate([bytes([65 + i])])[0], bytes([65 + i])) for i in range(8)]
    unit = []
    for i in range(60):
        unit.append(tiny[i % 8])
        if i % 6 == 0:
            unit.append(kinds[(i // 6) % len(kinds)])
    reps = CHUNK_BLOCKS // len(unit) + 2
    data = b"".join(unit) * reps + b"".join(kinds) + EOF_BLOCK
    rc_u, out_u = expected(b"".join(unit))
    rc_k, out_k = expected(b"".join(kinds))
    assert rc_u == rc_k == hbam.OK
    want = (hbam.OK, out_u * reps + out_k)
    rc, got, (lean, fb, _) = run(data)
    nblk = len(unit) * reps + len(kinds)
    assert nblk > CHUNK_BLOCKS
    assert rc == hbam.OK
    assert got == want[1]
    assert lean > 0 and fb > 0
    assert lean + fb >= nblk - reps - 1  # every block but the empty ones took a round


# ---- 6. lookahead edges
def test_full_output_then_nonfinal_eob_and_empty_final_block():
    rng = np.random.default_rng(7)
    t = texty(rng, 9000)
    # zlib's Z_FULL_FLUSH / Z_FINISH tail: ISIZE bytes are out before a
    # non-final end-of-block, an empty stored block and an empty final block
    c, _ = deflate([t, b""], flush=zlib.Z_FULL_FLUSH)
    lean, fb, _ = check(bgzf(c, t) + EOF_BLOCK)
    assert (lean, fb) == (0, 1)
    a = letters(rng, 9000)
    c, _ = deflate([a, t, b""], flush=zlib.Z_FULL_FLUSH)
    check(bgzf(c, a + t) + EOF_BLOCK)


@pytest.mark.parametrize("cut", [1, 2, 3, 100, 4500])
def test_full_output_then_more_symbols(cut):
    """ISIZE smaller than the stream's output: what follows the full output is
    not the end-of-block; zlib's lookahead decides."""
    t = texty(np.random.default_rng(8), 9000)
    c, _ = deflate([t])
    check(bgzf(c, t, isize=len(t) - cut) + EOF_BLOCK)


@pytest.mark.parametrize("x", [0x01, 0x10, 0x80, 0xff])
def test_full_output_then_garbage_bits(x):
    t = texty(np.random.default_rng(9), 9000)
    c = bytearray(deflate([t])[0])
    c[-1] ^= x  # the end-of-block code and the padding after it
    c2 = bytearray(c)
    c2[-2] ^= x
    for cd in (bytes(c), bytes(c2)):
        check(bgzf(cd, t) + EOF_BLOCK)


# ---- 7. errors in the first and in the second DEFLATE block
def two_block_stream(rng):
    a, t = letters(rng, 9000), texty(rng, 9000)
    c, marks = deflate([a, t])
    return a + t, c, marks[0]


def good_neighbours(rng):
    t = texty(rng, 5000)
    return bgzf(deflate([t])[0], t)


@pytest.mark.parametrize("second", [False, True])
def test_truncated_cdata(second):
    rng = np.random.default_rng(10)
    p, c, mark = two_block_stream(rng)
    ok = good_neighbours(rng)
    for k in ((mark + 40, mark + 1000, len(c) - 2) if second else (40, mark // 2, mark - 40)):
        data = ok + bgzf(c[:k], p) + ok + EOF_BLOCK
        want = expected(data)
        assert want == (hbam.E_FORMAT, len(ok))
        check(data, want)
    if second:  # cut inside the last byte's padding, or inside the end-of-block code: as zlib decides
        check(ok + bgzf(c[:-1], p) + ok + EOF_BLOCK)


@pytest.mark.parametrize("second", [False, True])
def test_bad_code(second):
    """A corrupted byte in the header / symbols of the first or second DEFLATE
    block: invalid code lengths, invalid codes, a walk off the true path."""
    rng = np.random.default_rng(11)
    p, c, mark = two_block_stream(rng)
    ok = good_neighbours(rng)
    seen = set()
    lo, hi = (mark + 1, len(c) - 1) if second else (0, mark - 1)
    ats = [lo, lo + 1, lo + 5, lo + 20] + [int(v) for v in rng.integers(lo, hi, 8)]
    for at in ats:
        bad = bytearray(c)
        bad[at] ^= int(rng.integers(1, 256))
        data = ok + bgzf(bytes(bad), p) + ok + EOF_BLOCK
        want = expected(data)
        seen.add(want[0])
        check(data, want)
    assert hbam.E_IO in seen


@pytest.mark.parametrize("second", [False, True])
def test_distance_before_the_start(second):
    """Matches that reach a preset dictionary the reader does not have: zlib's
    "invalid distance too far back", in dynamic blocks."""
    rng = np.random.default_rng(12)
    zd = letters(rng, 4000, 26, 97)
    plain = letters(rng, 9000)
    reach = zd[100:900] + letters(rng, 3000) + zd[1500:2500] + letters(rng, 3000)
    parts = [plain, reach] if second else [reach, plain]
    c, _ = deflate(parts, zdict=zd)
    ok = good_neighbours(rng)
    data = ok + bgzf(c, b"".join(parts)) + ok + EOF_BLOCK
    want = expected(data)
    assert want == (hbam.E_IO, len(ok))
    check(data, want)
    # the same stream with its dictionary-free part only decodes (the fixture is sound)
    c2, _ = deflate([plain])
    check(ok + bgzf(c2, plain) + EOF_BLOCK)
