"""Inputs and expected results of the sort tests (hbam_sort_writables).

The expected result needs no oracle of its own: it is the oracle's in-order
encoding (orc.Stream.writable_encode_span) sliced per record and concatenated
in the order of a NumPy stable argsort of the sort word, computed from the
oracle's columns.  Every case asserts what it is there for on the CPU, before
any comparison with the GPU.  Test data only."""
import functools
import os
import struct

import numpy as np

import bai
import orc
from conftest import GOLDEN
from hbam import synth
from bam_patch import recompress

ORDERS = ("key", "coordinate")
TILE = 32768  # output bytes per workgroup of the gather
INT_MAX = 0x7FFFFFFF


def sort_word(cols, order):
    """The word each order sorts by, as an array NumPy compares the same way."""
    if order == "key":  # LongWritable.compareTo: signed
        return cols["key"].astype(np.int64)
    ref = cols["ref_id"].astype(np.int64) & 0xFFFFFFFF
    pos1 = (cols["pos"].astype(np.int64) + 1) & 0xFFFFFFFF
    return ((ref << 32) | pos1).astype(np.uint64)


class SortCase:
    """A BAM, its oracle columns (SILENT) and the oracle's in-order encoding."""

    def __init__(self, data):
        self.data = data
        self.stream = orc.Stream(data, stringency=orc.SILENT)
        rc, self.cols = self.stream.decode_all()
        assert rc == 0
        rc, self.enc, self.offs = self.stream.writable_encode_span(self.stream.first_record_voff, (1 << 64) - 1)
        assert rc == 0
        self.n = len(self.cols["key"])
        assert len(self.offs) == self.n + 1
        self.lens = np.diff(self.offs.astype(np.int64))
        assert np.array_equal(self.lens, 36 + self.cols["rest_len"].astype(np.int64))

    def perm(self, order, lo=0, hi=None):
        hi = self.n if hi is None else hi
        w = sort_word({k: v[lo:hi] for k, v in self.cols.items()}, order)
        return np.argsort(w, kind="stable").astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def expected(self, order, lo=0, hi=None):
        """(bytes, offs[u64, m + 1], perm[u32, m]) of records [lo, hi) sorted on their own."""
        hi = self.n if hi is None else hi
        perm = self.perm(order, lo, hi)
        o = [int(x) for x in self.offs]
        out = b"".join(self.enc[o[lo + int(i)]:o[lo + int(i) + 1]] for i in perm)
        offs = np.zeros(hi - lo + 1, np.uint64)
        offs[1:] = np.cumsum(self.lens[lo:hi][perm])
        return out, offs, perm

    def source_starts(self):
        """Where each record's bytes start in the inflated stream."""
        return self.cols["offset"].astype(np.int64)


def equal_word_groups(case, order, at_least=3):
    _, counts = np.unique(sort_word(case.cols, order), return_counts=True)
    return int(np.count_nonzero(counts >= at_least))


def alignment_pairs(case, order):
    """The (source start & 15, destination start & 15) pairs among the records."""
    _, offs, perm = case.expected(order)
    src = case.source_starts()[perm] & 15
    dst = offs[:-1].astype(np.int64) & 15
    return set(zip(src.tolist(), dst.tolist()))


def max_records_per_tile(case, order):
    _, offs, _ = case.expected(order)
    o = offs.astype(np.int64)
    starts, ends = o[:-1], o[1:]
    best = 0
    for t0 in range(0, int(o[-1]), TILE):
        best = max(best, int(np.count_nonzero((starts < t0 + TILE) & (ends > t0))))
    return best


# ---- mixed: short reads dealt over contigs, unplaced and half-placed reads ------
def _mixed_data(n_records, seed):
    data, _ = synth.make_bam(n_records, seed=seed)
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, r = s.decode_all()
    assert rc == 0
    u = bytearray(s.data)
    rng = np.random.default_rng(seed)
    for p in r["offset"]:
        p = int(p)
        (flag,) = struct.unpack_from("<H", u, p + 18)
        ref = int(rng.integers(-1, 5))
        if ref < 0:  # unplaced: no position, bin 4680 (write() zeroes it), unmapped
            pos, b, flag = -1, 4680, flag | 4
        else:
            pos = int(rng.integers(0, 40))
            kind = rng.random()
            if kind < 0.05:  # a contig and no position
                pos = -1
            elif kind < 0.15:  # a placed unmapped read
                flag |= 4
            if pos < 0:
                b = 4680
            elif flag & 4:
                b = bai._reg2bin(pos, pos + 1)
            else:
                _, _, end, _ = bai._ref_span(u, p)
                span = end - struct.unpack_from("<i", u, p + 8)[0]
                b = bai._reg2bin(pos, pos + span)
        struct.pack_into("<ii", u, p + 4, ref, pos)
        struct.pack_into("<H", u, p + 14, b)
        struct.pack_into("<H", u, p + 18, flag)
    return recompress(s, bytes(u))


@functools.lru_cache(maxsize=None)
def mixed_case():
    case = SortCase(_mixed_data(4000, 0x534F5254))
    c = case.cols
    assert case.n == 4000
    assert set(np.unique(c["ref_id"]).tolist()) == {-1, 0, 1, 2, 3, 4}
    assert np.count_nonzero((c["ref_id"] >= 0) & (c["pos"] == -1)) > 20
    assert np.count_nonzero((c["ref_id"] >= 0) & (c["pos"] >= 0) & (c["flag"] & 4 != 0)) > 20
    assert np.all(c["bin"][c["ref_id"] < 0] == 4680)
    for order in ORDERS:
        assert equal_word_groups(case, order) >= 100, order
        assert len(alignment_pairs(case, order)) == 256, order
    unmapped = c["key"][(c["flag"] & 4 != 0) | (c["ref_id"] < 0) | (c["pos"] < 0)]
    assert np.any(unmapped < 0) and np.any(unmapped >> 32 == INT_MAX)  # hashes of both signs
    # not sorted in either order: the sort has work to do
    for order in ORDERS:
        assert not np.array_equal(case.perm(order), np.arange(case.n))
    return case


# ---- long: ONT-like unmapped reads, records of many tiles -----------------------
@functools.lru_cache(maxsize=None)
def long_case():
    case = SortCase(synth.make_bam(60, mode="long", all_unmapped=True, seed=0x534F5255)[0])
    assert case.n == 60 and int(case.lens.max()) > 2 * TILE
    assert np.count_nonzero(case.cols["rest_len"] > 2048) > 30  # keys of the long-hash path
    return case


# ---- hand-packed minimal records ------------------------------------------------
def _header():
    """A BAM header (synth's 25 contigs) to put hand-packed records behind."""
    s = orc.Stream(synth.make_bam(1, seed=1)[0], stringency=orc.SILENT)
    return bytes(s.data[:s.header_end])


def packed_record(length, ref, pos, flag, tag):
    """A record of `length` >= 38 bytes: no cigar, no bases, the padding in the
    read name (as _record of tests/test_writable.py, l_seq 0); l_seq 1 when the
    length leaves room for it and `tag` is odd."""
    assert 38 <= length <= 36 + 255
    l_seq = 1 if (tag & 1 and length >= 40) else 0
    name = bytes(65 + (tag + k) % 26 for k in range(length - 36 - 1 - 2 * l_seq))
    rest = name + b"\0" + bytes(l_seq) + bytes([30] * l_seq)
    assert 36 + len(rest) == length
    b = 4680 if ref < 0 or pos < 0 else bai._reg2bin(pos, pos + 1)
    return struct.pack("<iiiBBHHHiiii", 32 + len(rest), ref, pos, len(name) + 1, 0, b, 0, flag, l_seq, -1, -1,
                       0) + rest


def packed_bam(lengths, seed, block=60000):
    """A BAM of hand-packed records with these encoded lengths, refID / pos /
    flag drawn at random (unplaced and placed, mapped and unmapped), written
    through the oracle's BGZF writer in blocks of `block` bytes."""
    rng = np.random.default_rng(seed)
    recs = []
    for i, ln in enumerate(lengths):
        ref = int(rng.integers(-1, 4))
        pos = -1 if ref < 0 else int(rng.integers(0, 12))
        flag = 4 if ref < 0 or rng.random() < 0.3 else 0
        recs.append(packed_record(int(ln), ref, pos, flag, i))
    payload = _header() + b"".join(recs)
    lens = [min(block, len(payload) - p) for p in range(0, len(payload), block)]
    return orc.bgzf_compress(payload, lens, level=5, eof=True)


@functools.lru_cache(maxsize=None)
def tiny_case():
    rng = np.random.default_rng(0x534F5256)
    case = SortCase(packed_bam(rng.choice([38, 40], 3000), 0x534F5256))
    assert case.n == 3000
    for order in ORDERS:
        assert max_records_per_tile(case, order) >= 800, order
    return case


def _lengths(n, total, seed):
    """n record lengths in [38, 135] that add up to total."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(38, 57, n).astype(np.int64)
    if int(ln.sum()) > total:
        ln[:] = 38
    rest = total - int(ln.sum())
    assert 0 <= rest <= n * 40, (n, total)
    ln[:rest // 40] += 40
    ln[rest // 40 if rest // 40 < n else n - 1] += rest % 40
    assert int(ln.sum()) == total and ln.min() >= 38 and ln.max() <= 36 + 255
    return ln


# name -> (records, total encoded bytes): the record counts around a workgroup's
# 256 lanes, totals = 0, 1 and 15 mod 16, and totals one byte short of, equal to
# and one byte over a whole number of tiles
BOUNDARY = {
    "n1": (1, 41),
    "n255_mod0": (255, 15296),
    "n256_mod1": (256, 15361),
    "n257_mod15": (257, 15423),
    "tile_minus1": (1100, 2 * TILE - 1),
    "tile_exact": (1100, 2 * TILE),
    "tile_plus1": (1100, 2 * TILE + 1),
    "one_tile_exact": (500, TILE),
}


@functools.lru_cache(maxsize=None)
def boundary_case(name):
    n, total = BOUNDARY[name]
    case = SortCase(packed_bam(_lengths(n, total, n + total), n + total))
    assert case.n == n and len(case.enc) == total
    return case


def _check_boundary_table():
    mod = {k: v[1] % 16 for k, v in BOUNDARY.items()}
    assert (mod["n255_mod0"], mod["n256_mod1"], mod["n257_mod15"]) == (0, 1, 15), mod
    assert (mod["tile_minus1"], mod["tile_exact"], mod["tile_plus1"]) == (15, 0, 1)


_check_boundary_table()


@functools.lru_cache(maxsize=None)
def test_bam_case():
    return SortCase(open(os.path.join(GOLDEN, "test.bam"), "rb").read())


CASES = {"mixed": mixed_case, "long": long_case, "tiny": tiny_case, "test.bam": test_bam_case}
CASES.update({k: functools.partial(boundary_case, k) for k in BOUNDARY})


def as_bam(case, order):
    """The expected records of `order` written as a BAM (the case's header in
    front, the oracle's BGZF writer): what sort_bam should produce, up to the
    header's @HD line and the block cuts."""
    payload = bytes(case.stream.data[:case.stream.header_end]) + case.expected(order)[0]
    lens = [min(65280, len(payload) - p) for p in range(0, len(payload), 65280)]
    return orc.bgzf_compress(payload, lens, level=5, eof=True)
