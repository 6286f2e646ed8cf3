"""BAM files and split points that take the split guesser (hbam_guess.hip,
k_guess_splits / k_guess_bgzf_starts / k_block_crc and their host windows) off
its common path, with the oracle (orc_guess_record_start_hdr, an independent
restatement over the raw byte window with zlib) as the only source of
expected values.

The guesser searches the compressed window [beg, min(end, beg + MAX)) for a
BGZF header below beg + min(end - beg, 0xffff), looks inside that block for a
record candidate (guess_bam_pos) and verifies it by decoding records over
three blocks under htsjdk's BlockCompressedInputStream rules (decode_verify,
gz_read_block).  The families below each reach one part of that:

  A  window edges      the read limit inside a block / fewer than 18 bytes into
                       the next header, on five file shapes
  B  rejects           records the candidate test takes and the verification
                       refuses (and the other way round), header_n_ref
  C  corrupt blocks    bad CRC, bad ISIZE, bad DEFLATE, files cut inside a block
  D  CRC slices        block lengths around multiples of 256, and blocks whose
                       only fault is a CRC that no longer matches
  E  empty blocks      in mid-file, two in a row, first after beg, file ending
                       on one
  F  false magic       BGZF magic / headers inside a stored block's payload
  G  decoys            the files of chain_cases.py
  H  grouping          a 2 MB file whose points fall into several host windows

A case is dict(data=file bytes, pts=[(beg, end)], intact=the undamaged file of
the same layout or None, header_n_ref=int or None, ...facts); get(name)
builds it once per process, want(name) is the oracle's answer per point.
"""
import bisect
import ctypes
import functools
import struct

import numpy as np

import chain_cases as cc
import orc
from hbam import synth

MAX = 3 * 0xffff + 0xfffe  # BAMSplitGuesser.MAX_BYTES_READ
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# an empty block in its other form: one stored DEFLATE block of length 0
EMPTY_STORED = bytes.fromhex("1f8b08040000000000ff0600424302001e00" "010000ffff" "0000000000000000")
assert len(EOF_BLOCK) == 28 and len(EMPTY_STORED) == 31


# ---------------------------------------------------------------------------
# blocks and points
# ---------------------------------------------------------------------------
def block_offsets(data):
    """c[0..n] of a file of standard BGZF blocks (BSIZE at +16), c[n] = file size."""
    c, p = [], 0
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04" and data[p + 12:p + 16] == b"BC\x02\x00", p
        c.append(p)
        p += struct.unpack_from("<H", data, p + 16)[0] + 1
    assert p == len(data)
    return c + [p]


def split_blocks(data):
    c = block_offsets(data)
    return [data[a:b] for a, b in zip(c, c[1:])]


def isize_of(block):
    return struct.unpack_from("<I", block, len(block) - 4)[0]


def window_edge_points(c, size, blocks, ts=(1, 2, 3, 4), ks=(0, 1, 17, 18, 19, 40)):
    """For every block j of `blocks`: beg just before / at / just after c[j],
    end at the read limit, the file size, the firstEnd cut-off, a short range,
    and k bytes into the header of each of the next blocks."""
    n = len(c) - 1
    pts = []
    for j in blocks:
        if not 1 <= j < n:
            continue
        for beg in (c[j] - 3, c[j] - 1, c[j], c[j] + 1):
            ends = [beg + MAX, max(size, beg), beg + 0xffff, beg + 100]
            ends += [c[j + t] + k for t in ts if j + t <= n for k in ks]
            pts += [(beg, e) for e in ends]
    assert all(0 < b <= e for b, e in pts)
    return pts


def tail_points(c, size):
    n = len(c) - 1
    begs = [(c[n - 2] + c[n - 1]) // 2, c[n - 1] + 5, size - 1, size, size + 5]
    return [(b, e) for b in begs for e in (b + MAX, max(size, b), b + 100)]


def thin(pts, cap):
    """At most about `cap` of pts, taken at a stride that shares no factor with
    the points per block, so that every (beg, end) kind stays in."""
    k = -(-len(pts) // cap)
    while k > 1 and (k % 2 == 0 or k % 3 == 0 or k % 7 == 0):
        k += 1
    return pts[::k]


def begs_ends(pts):
    return [b for b, _ in pts], [e for _, e in pts]


def oracle_guesses(intact, pts, header_n_ref=None, file=None):
    """The oracle's answer per point (an oracle error raises)."""
    s = orc.Stream(intact)
    buf = None if file is None else ctypes.create_string_buffer(file, len(file))
    return [s.guess_record_start(b, e, header_n_ref, file=buf) for b, e in pts]


def record_voffs(data):
    """The virtual offsets of all records, as the oracle reads the file."""
    rc, want = orc.Stream(data, stringency=orc.SILENT).decode_all()
    assert rc == 0
    return set(int(v) for v in want["voff"])


def case(name, data, pts, intact=None, header_n_ref=None, **facts):
    return dict(name=name, data=data, pts=pts, intact=intact, header_n_ref=header_n_ref, **facts)


# ---------------------------------------------------------------------------
# A. window edges
# ---------------------------------------------------------------------------
A_FILES = {
    "short65280": dict(n_records=3000, block_payload=65280),
    "short4096": dict(n_records=3000, block_payload=4096),
    "short700": dict(n_records=3000, block_payload=700),
    "long": dict(n_records=40, mode="long"),
    "stored8192": dict(n_records=3000, level=0, block_payload=8192),
}


@functools.lru_cache(maxsize=None)
def synth_file(name):
    data, _ = synth.make_bam(**A_FILES[name])
    return data


def case_edges(name):
    data = synth_file(name)
    c, size = block_offsets(data), len(data)
    n = len(c) - 1
    if name in ("short65280", "long"):  # ~50 ms of oracle time per point
        pts = thin(window_edge_points(c, size, range(1, n, 3), ts=(1, 3), ks=(0, 17, 18, 19)), 56)
    else:
        step = max(1, n * 112 // 3500)
        pts = window_edge_points(c, size, range(1, n, step))
    return case("edges_" + name, data, pts + tail_points(c, size), blocks=n)


# ---------------------------------------------------------------------------
# B. records the verification rejects
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base4096(n_records=3000):
    """(file, inflated stream, header end, record starts, n_ref, block lengths)
    of make_bam(n_records, block_payload=4096)."""
    data = synth_file("short4096") if n_records == 3000 else synth.make_bam(n_records, block_payload=4096)[0]
    s = orc.Stream(data)
    u = bytes(s.data)
    starts, q = [], s.header_end
    while q < len(u):
        starts.append(q)
        q += 4 + cc.rd32(u, q)
    assert len(starts) == n_records
    return data, u, s.header_end, tuple(starts), s.n_ref, tuple(int(x) for x in s.blocks["isize"] if x)


def _set32(off, v):
    return lambda rec, n_ref: rec[:off] + struct.pack("<i", v) + rec[off + 4:]


def _cigar9(rec, n_ref):
    lrn, ncig = rec[12], struct.unpack_from("<H", rec, 16)[0]
    assert ncig >= 1
    at = 36 + lrn
    return rec[:at] + bytes([(rec[at] & 0xf0) | 9]) + rec[at + 1:]


def _nonul(rec, n_ref):
    at = 36 + rec[12] - 1
    assert rec[at] == 0
    return rec[:at] + b"X" + rec[at + 1:]


def _append(tail):
    def f(rec, n_ref):
        body = rec[4:] + tail
        return struct.pack("<i", len(body)) + body
    return f


REJECTS = {
    "cigar9": _cigar9,
    "ref_nref": lambda rec, n_ref: _set32(4, n_ref)(rec, n_ref),
    "nref_nref": lambda rec, n_ref: _set32(24, n_ref)(rec, n_ref),
    "lseq_neg": _set32(20, -3),
    "bs31": _set32(0, 31),
    "lrn0": lambda rec, n_ref: rec[:12] + b"\0" + rec[13:],
    "nonul": _nonul,
    "aux_type": _append(b"XQ?\0"),
    "z_nonul": _append(b"XZZabc"),
    "b_subtype": _append(b"XBBx" + struct.pack("<i", 0)),
    "b_negcount": _append(b"XBBc" + struct.pack("<i", -1)),
    "b_overrun": _append(b"XBBi" + struct.pack("<i", 1000) + b"\1\0\0\0"),
    "stray2": _append(b"AB"),
}
REJECT_AT = (500, 1500, 2500)


def _mapped_from(u, starts, r):
    """The first record at or after r with a CIGAR."""
    while struct.unpack_from("<H", u, starts[r] + 16)[0] == 0:
        r += 1
    return r


def _block_first_from(starts, lens, r):
    """The first record at or after r that is the first to start in its block."""
    cuts = [0]
    for n in lens:
        cuts.append(cuts[-1] + n)
    while True:
        b0 = cuts[bisect.bisect_right(cuts, starts[r]) - 1]
        if starts[r - 1] < b0 <= starts[r]:
            return r
        r += 1


def reject_points(c):
    n = len(c) - 1
    pts = []
    for j in range(1, n):
        pts += [(c[j], c[j] + MAX), (c[j] - 1, c[j] + MAX), (c[j], c[min(j + 2, n)] + 18)]
    return pts


def case_reject(patch, header_n_ref=None, name=None):
    """The 4096-payload file with `patch` applied to three records, on the
    same block lengths (a patch that lengthens records lengthens the last
    block).  nonul is seen by the candidate test alone (the verification, as
    BAMRecordCodec, never looks at the name's end), so it goes on records that
    are the first to start in their block: the only place where it can move
    an answer."""
    _, u, head_end, starts, n_ref, lens = base4096()
    at = list(REJECT_AT)
    if patch == "cigar9":
        at = [_mapped_from(u, starts, r) for r in at]
    elif patch == "nonul":
        at = [_block_first_from(starts, lens, r) for r in at]
    ends = list(starts[1:]) + [len(u)]
    recs = [u[a:b] for a, b in zip(starts, ends)]
    if patch is not None:
        for r in at:
            recs[r] = REJECTS[patch](recs[r], n_ref)
    u2 = u[:head_end] + b"".join(recs)
    lens2 = list(lens)
    lens2[-1] += len(u2) - len(u)
    data = orc.bgzf_compress(u2, lens2, 5, eof=True)
    new_starts = [head_end]
    for r in recs[:-1]:
        new_starts.append(new_starts[-1] + len(r))
    return case(name or "reject_" + str(patch), data, reject_points(block_offsets(data)), header_n_ref=header_n_ref,
                u=u2, starts=new_starts, patched=at, n_ref=n_ref, lens=lens2)


# ---------------------------------------------------------------------------
# C. corrupt blocks
# ---------------------------------------------------------------------------
def _flip(data, at, mask=1):
    return data[:at] + bytes([data[at] ^ mask]) + data[at + 1:]


def damage(data, c, j, kind):
    csize = c[j + 1] - c[j]
    if kind == "crc":
        return _flip(data, c[j] + csize - 8)
    if kind == "isize":
        return _flip(data, c[j] + csize - 4)
    if kind == "cdata":
        at = c[j] + 18  # the DEFLATE block header and the start of its code lengths: no longer inflates
        return _flip(_flip(data, at, 0xff), at + 1, 0xff)
    if kind.startswith("cut"):
        k = csize - 1 if kind == "cut_last" else int(kind[3:])
        return data[:c[j] + k]
    raise ValueError(kind)


DAMAGE = ("crc", "isize", "cdata", "cut1", "cut17", "cut18", "cut19", "cut_last")


def case_corrupt(kind, where):
    data = base4096()[0]
    c = block_offsets(data)
    n = len(c) - 1
    j = 3 if where == "head" else n - 6
    bad = damage(data, c, j, kind)
    pts = window_edge_points(c, len(bad), range(j - 4, j + 3))
    return case(f"corrupt_{kind}_{where}", bad, pts, intact=data, j=j, c=c)


def case_corrupt_far():
    """Damage in two blocks more than 1 MiB apart: two host windows."""
    data = base4096(12000)[0]
    c = block_offsets(data)
    j1 = 50
    j2 = next(j for j in range(j1, len(c)) if c[j] - c[j1 + 1] > (1 << 20) + MAX + 0x20000)
    bad = damage(damage(data, c, j1, "crc"), c, j2, "cdata")
    pts = thin(window_edge_points(c, len(bad), list(range(j1 - 4, j1 + 3)) + list(range(j2 - 4, j2 + 3))), 1600)
    return case("corrupt_far", bad, pts, intact=data, j=(j1, j2), c=c)


# ---------------------------------------------------------------------------
# D. k_block_crc slices
# ---------------------------------------------------------------------------
CRC_LENS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 4095, 65279, 65280)


@functools.lru_cache(maxsize=None)
def crc_file():
    """(file, block lengths): the B base stream with every length of CRC_LENS,
    twice, each followed by three ordinary blocks."""
    u = base4096()[1]
    lens = [4096]
    for _ in range(2):
        for n in CRC_LENS:
            lens += [n, 4096, 4096, 4096]
    rest = len(u) - sum(lens)
    assert rest > 0
    lens += [4096] * (rest // 4096) + ([rest % 4096] if rest % 4096 else [])
    return orc.bgzf_compress(u, lens, 5), tuple(lens)


def case_crc_good():
    data, lens = crc_file()
    c = block_offsets(data)
    pts = thin(window_edge_points(c, len(data), range(1, len(c) - 1)), 3000)
    return case("crc_good", data, pts, lens=lens)


def crc_variant_positions(isize):
    sl = (isize + 255) // 256  # k_block_crc's slice
    return [p for p in (0, isize - 1, sl - 1, sl, 255 * sl) if p < isize]


def case_crc_undetected(isize, pos):
    """One payload byte of a block of `isize` bytes changed, the block
    recompressed, its CRC field left as the original's: well-formed DEFLATE
    that only a CRC check can refuse."""
    data, lens = crc_file()
    blocks = split_blocks(data)
    j = lens.index(isize)
    a = sum(lens[:j])
    payload = bytearray(base4096()[1][a:a + isize])
    payload[pos] ^= 0x20
    new = orc.bgzf_compress(bytes(payload), [isize], 5, eof=False)
    assert isize_of(new) == isize and len(block_offsets(new)) == 2
    new = new[:-8] + blocks[j][-8:-4] + new[-4:]
    blocks[j] = new
    bad = b"".join(blocks)
    c = block_offsets(bad)
    cg = block_offsets(data)
    pts, good_pts = (window_edge_points(x, len(f), range(max(1, j - 4), j + 3)) for x, f in ((c, bad), (cg, data)))
    if isize > 10000:
        pts, good_pts = thin(pts, 150), thin(good_pts, 150)
    # good_pts: the same points, block for block, on the good file
    return case(f"crc_undetected_{isize}_{pos}", bad, pts, intact=None, j=j, c=c, good_pts=good_pts)


CRC_VARIANTS = [(n, p) for n in (257, 513, 65280) for p in crc_variant_positions(n)]


# ---------------------------------------------------------------------------
# E. empty blocks
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def empties_file():
    """(file, indices of the inserted empty blocks in the new file)."""
    blocks = split_blocks(base4096()[0])
    out, empty = [], []
    for k, b in enumerate(blocks):
        out.append(b)
        ins = {10: [EOF_BLOCK], 20: [EMPTY_STORED, EMPTY_STORED], 30: [EOF_BLOCK]}.get(k, [])
        for e in ins:
            empty.append(len(out))
            out.append(e)
    return b"".join(out), tuple(empty)


def case_empties(cut=False):
    data, empty = empties_file()
    c = block_offsets(data)
    if cut:  # the file ends on a mid-file empty block, with no EOF block after it
        data = data[:c[empty[-1] + 1]]
        c = block_offsets(data)
    pts = window_edge_points(c, len(data), range(6, 40))
    return case("empties_cut" if cut else "empties", data, pts, empty=empty, c=c)


# ---------------------------------------------------------------------------
# F. false magic in a stored block's payload
# ---------------------------------------------------------------------------
def _hdr(xlen, extra):
    return b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", xlen) + extra


FALSE_MAGIC = {
    "magic_zeros": b"\x1f\x8b\x08\x04" + bytes(28),
    # a complete header, BSIZE + 1 = 301: what would be its footer is tag padding
    "header": _hdr(6, b"BC\x02\x00" + struct.pack("<H", 300)),
    "xlen_ffff": _hdr(0xffff, b"BC\x02\x00" + struct.pack("<H", 300)),
    "subfield_first": _hdr(12, b"XY\x02\x00\xaa\xbb" + b"BC\x02\x00" + struct.pack("<H", 300)),
    "overrun": _hdr(8, b"BC\x02\x00" + struct.pack("<H", 300) + b"ZZ"),  # 2 bytes left: no room for a subfield
}
FALSE_AT = (400, 1400, 2400)
MARK = bytes(range(0xc0, 0xd0))  # marks a payload in the file; no valid tag or record reads like it


def case_false_magic(kind):
    data = synth_file("stored8192")
    s = orc.Stream(data)
    u = bytes(s.data)
    lens = [int(x) for x in s.blocks["isize"] if x]
    starts, q = [], s.header_end
    while q < len(u):
        starts.append(q)
        q += 4 + cc.rd32(u, q)
    recs = [u[a:b] for a, b in zip(starts, starts[1:] + [len(u)])]
    payload = FALSE_MAGIC[kind] + MARK
    payload += bytes(400 - len(payload))
    for r in FALSE_AT:
        recs[r], _ = cc.with_tag(recs[r], payload)
    u2 = u[:s.header_end] + b"".join(recs)
    lens = [8192] * (len(u2) // 8192) + ([len(u2) % 8192] if len(u2) % 8192 else [])
    out = orc.bgzf_compress(u2, lens, 0)
    c = block_offsets(out)
    magics, at = [], -1
    while True:
        at = out.find(FALSE_MAGIC[kind] + MARK, at + 1)
        if at < 0:
            break
        magics.append(at)
    pts = []
    for m in magics:
        host = c[bisect.bisect_right(c, m) - 1]
        for beg in list(range(m - 40, m + 5)) + [host]:
            pts += [(beg, e) for e in (beg + MAX, m + 4, m + 12, m + 18, m + 30) if e >= beg]
    return case("false_" + kind, out, pts, magics=magics, c=c)


# ---------------------------------------------------------------------------
# G. the decoys and implausible records of chain_cases.py
# ---------------------------------------------------------------------------
def case_chain(name):
    k = cc.get(name)
    c = block_offsets(k["data"])
    pts = []
    for j in range(1, len(c) - 1):
        pts += [(c[j], c[j] + MAX), (c[j] - 1, c[j] + MAX)]
    return case("chain_" + name, k["data"], pts, c=c, chain=k)


# ---------------------------------------------------------------------------
# H. grouping
# ---------------------------------------------------------------------------
def case_grouping():
    data = base4096(12000)[0]
    c, n = block_offsets(data), len(data)
    pts = window_edge_points(c, n, range(1, len(c) - 1, 8))
    rng = np.random.default_rng(7)
    begs = sorted(set(int(x) for x in rng.integers(1, n, 300)))
    ends = [min(n, b + int(w)) for b, w in zip(begs, rng.integers(1, 200000, len(begs)))]
    ends[::7] = [n] * len(ends[::7])
    pts = thin(pts, 3000) + list(zip(begs, ends))
    return case("grouping", data, pts, c=c)


# ---------------------------------------------------------------------------
CASES = {}
for _n in A_FILES:
    CASES["edges_" + _n] = functools.partial(case_edges, _n)
for _p in REJECTS:
    CASES["reject_" + _p] = functools.partial(case_reject, _p)
CASES["reject_ref_nref_hdr"] = lambda: case_reject("ref_nref", header_n_ref=base4096()[4] + 1, name="reject_ref_nref_hdr")
CASES["reject_none_hdr0"] = lambda: case_reject(None, header_n_ref=0, name="reject_none_hdr0")
CASES["reject_none_hdr1"] = lambda: case_reject(None, header_n_ref=1, name="reject_none_hdr1")
for _k in DAMAGE:
    for _w in ("head", "tail"):
        CASES[f"corrupt_{_k}_{_w}"] = functools.partial(case_corrupt, _k, _w)
CASES["corrupt_far"] = case_corrupt_far
CASES["crc_good"] = case_crc_good
for _n, _p in CRC_VARIANTS:
    CASES[f"crc_undetected_{_n}_{_p}"] = functools.partial(case_crc_undetected, _n, _p)
CASES["empties"] = case_empties
CASES["empties_cut"] = functools.partial(case_empties, True)
for _k in FALSE_MAGIC:
    CASES["false_" + _k] = functools.partial(case_false_magic, _k)
for _n in list(cc.FALSE_START_CASES) + list(cc.IMPLAUSIBLE_CASES):
    CASES["chain_" + _n] = functools.partial(case_chain, _n)
CASES["grouping"] = case_grouping

FAMILY = {
    "A": [n for n in CASES if n.startswith("edges_")],
    "B": [n for n in CASES if n.startswith("reject_")],
    "C": [n for n in CASES if n.startswith("corrupt_")],
    "D": [n for n in CASES if n.startswith("crc_")],
    "E": [n for n in CASES if n.startswith("empties")],
    "F": [n for n in CASES if n.startswith("false_")],
    "G": [n for n in CASES if n.startswith("chain_")],
    "H": ["grouping"],
}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case `name`, built once per process."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """The oracle's guess per point of the case; shared, never modified."""
    k = get(name)
    damaged = k["intact"] is not None
    return tuple(oracle_guesses(k["intact"] if damaged else k["data"], k["pts"], k["header_n_ref"],
                                file=k["data"] if damaged else None))


@functools.lru_cache(maxsize=None)
def want_bgzf(name):
    """BGZFSplitGuesser's answer at the case's begs and the first three kinds of end."""
    k = get(name)
    pts = bgzf_points(k)
    return tuple(orc.guess_next_bgzf_block_start(k["data"], b, e) for b, e in pts)


def bgzf_points(k):
    size = len(k["data"])
    pts = []
    for b in sorted(set(b for b, _ in k["pts"])):
        pts += [(b, b + MAX), (b, max(size, b)), (b, b + 0xffff)]
    return pts
