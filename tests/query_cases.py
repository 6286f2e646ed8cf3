"""Bounded traversal (hbam_query_*): the restated filter, its inputs and the
test data.  Test infrastructure only (imported by the query tests).

The rules are htsjdk's BAMFileReader.BAMFileIndexIterator,
BAMQueryFilteringIterator, BAMQueryMultipleIntervalsIteratorFilter.
compareIntervalToRecord and BAMFileIndexUnmappedIterator as the project
restates them (include/hbam.h); parity with htsjdk itself is unpinned (no JVM
here, and the reference's interval tests run on BAMs htsjdk writes at test
time).  `filter_loop` is the literal per-record loop; the GPU computes the
scan form (`filter_scan`), so comparing the two checks one against the other.
"""
import functools
import struct

import numpy as np

import bai
import orc
from bai_cases import spread_bam
from hbam import synth
from test_bai import PLACEMENTS
from bam_patch import recompress

INT32_MAX = (1 << 31) - 1
ALL = (1 << 64) - 1
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X consume the reference
FIELDS = ("ref_id", "pos", "l_seq", "next_ref_id", "next_pos", "tlen", "l_read_name", "mapq", "bin", "n_cigar",
          "flag", "key", "voff", "rest_len")


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def cigar_ref_len(u, p):
    """Reference length of the record at u[p] (block_size first), summed in
    32-bit wrapping arithmetic like a Java int."""
    lrn = u[p + 12]
    (ncig,) = struct.unpack_from("<H", u, p + 16)
    n = 0
    for (c,) in struct.iter_unpack("<I", bytes(u[p + 36 + lrn:p + 36 + lrn + 4 * ncig])):
        if (c & 15) in REF_OPS:
            n += c >> 4
    return _i32(n)


def alignment_end(u, p):
    """(ref, start, alignmentEnd) of the record at u[p]: 1-based; an unmapped
    record ends where it starts."""
    ref, pos = struct.unpack_from("<ii", u, p + 4)
    (flag,) = struct.unpack_from("<H", u, p + 18)
    start = _i32(pos + 1)
    if flag & 4:
        return ref, start, start
    return ref, start, _i32(start + cigar_ref_len(u, p) - 1)


def record_table(u, offsets):
    return [alignment_end(u, int(p)) for p in offsets]


def _eff(iv):
    return [(r, s, INT32_MAX if e <= 0 else e) for r, s, e in iv]


def filter_loop(records, intervals, idx=0):
    """The literal loop: records = [(ref, start, alignmentEnd)].  Returns
    (kept indices, stop index or None, interval index after the last record)."""
    iv = _eff(intervals)
    kept = []
    for i, (ref, start, aend) in enumerate(records):
        while idx < len(iv):
            r, s, e = iv[idx]
            if r < ref or (r == ref and e < start):  # BEFORE
                idx += 1
                continue
            if not (r > ref or aend < s):  # not AFTER: CONTAINED or OVERLAPPING
                kept.append(i)
            break
        if idx == len(iv):
            return kept, i, idx
    return kept, None, idx


def filter_scan(records, intervals):
    """The parallel form: p = leading intervals BEFORE the record, idx = running
    max of p, keep iff idx < L and intervals[idx] is not AFTER."""
    iv = _eff(intervals)
    kept, stop, idx = [], None, 0
    for i, (ref, start, aend) in enumerate(records):
        p = 0
        while p < len(iv) and (iv[p][0] < ref or (iv[p][0] == ref and iv[p][2] < start)):
            p += 1
        idx = max(idx, p)
        if idx == len(iv):
            stop = i
            break
        r, s, _ = iv[idx]
        if not (r > ref or aend < s):
            kept.append(i)
    return kept, stop


def overlaps_any(records, intervals):
    """Brute force: the records overlapping any interval (what the filter
    yields on coordinate-sorted input)."""
    iv = _eff(intervals)
    return [i for i, (ref, start, aend) in enumerate(records)
            if any(r == ref and s <= aend and start <= e for r, s, e in iv)]


def _take(cols, idx):
    idx = np.asarray(idx, np.int64)
    return {k: v[idx] for k, v in cols.items()}


def _concat(parts, like):
    return {k: np.concatenate([p[k] for p in parts]) if parts else like[k][:0] for k in like}


def query_oracle(stream, intervals, chunks):
    """The chunks [(vstart, vend)] read in order through the oracle's
    decode_span (under the stream's stringency) and filtered by the loop.
    Returns (status, kept columns, stopped): a failing record counts only if
    the iteration has not stopped before it; nothing is read after a stop."""
    u = stream.data
    parts, idx, status, stopped = [], 0, 0, False
    like = {name: np.zeros(0, dt) for name, dt in orc.RECORD_FIELDS}
    if not intervals:
        return 0, like, True  # idx == L at the first record
    for a, e in chunks:
        rc, r = stream.decode_span(a, e)
        kept, stop, idx = filter_loop(record_table(u, r["offset"]), intervals, idx)
        parts.append(_take(r, kept))
        if stop is not None:
            stopped = True
            break
        if rc != 0:
            status = rc
            break
    return status, _concat(parts, like), stopped


def unmapped_oracle(stream, start_voff):
    """queryUnmapped(): from start_voff to the end of the file, skip to the
    first record with refID -1, then every record."""
    rc, r = stream.decode_span(start_voff, ALL)
    first = np.flatnonzero(r["ref_id"] == -1)
    k = int(first[0]) if len(first) else len(r["ref_id"])
    return rc, _take(r, np.arange(k, len(r["ref_id"])))


def expected_rests(u, want):
    """The kept records' rests back to back (what a query batch's data holds)."""
    return b"".join(bytes(u[int(p) + 36:int(p) + 36 + int(n)]) for p, n in zip(want["offset"], want["rest_len"]))


# ---- chunk lists -----------------------------------------------------------
def _reg2bins(beg, end):
    """SAM spec 5.3: the bins overlapping the 0-based half-open [beg, end)."""
    end -= 1
    bins = [0]
    for shift, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(off + (beg >> shift), off + (end >> shift) + 1)
    return bins


def merge_chunks(chunks):
    out = []
    for a, e in sorted(chunks):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([a, e])
    return [(a, e) for a, e in out]


def bai_chunks(index: bytes, ref, start, end):
    """The chunk list a BAM index gives for the 1-based inclusive interval:
    the chunks of every bin overlapping it (reg2bins), without those that end
    at or before the linear index's offset of the interval's first 16 kbp
    window, merged.  It only generates test data."""
    beg0 = max(start - 1, 0)
    end0 = (1 << 29) if end <= 0 else end
    assert index[:4] == b"BAI\1"
    (n_ref,) = struct.unpack_from("<i", index, 4)
    p = 8
    bins, lin = {}, []
    for r in range(n_ref):
        (nb,) = struct.unpack_from("<i", index, p)
        p += 4
        for _ in range(nb):
            b, nc = struct.unpack_from("<Ii", index, p)
            p += 8
            ch = [struct.unpack_from("<QQ", index, p + 16 * k) for k in range(nc)]
            p += 16 * nc
            if r == ref:
                bins[b] = ch
        (ni,) = struct.unpack_from("<i", index, p)
        p += 4
        if r == ref:
            lin = list(struct.unpack_from(f"<{ni}Q", index, p)) if ni else []
        p += 8 * ni
    w = beg0 >> bai.LIDX_SHIFT
    min_off = lin[w] if w < len(lin) else (lin[-1] if lin else 0)
    want = set(_reg2bins(beg0, end0))
    chunks = [(a, e) for b, ch in bins.items() if b in want for a, e in ch if e > min_off]
    return merge_chunks(chunks)


def bai_chunks_for(index, intervals):
    return merge_chunks([c for r, s, e in intervals for c in bai_chunks(index, r, s, e)])


def flat(chunks):
    return [v for c in chunks for v in c]


# ---- test data ---------------------------------------------------------------
NEW_OPS = (2, 3, 7, 8, 6, 5)  # D N = X P H: the short-read model only emits M, I and S


def with_cigar_ops(data, seed):
    """data with about half of its cigar operators' codes rewritten (lengths
    kept) to D, N, =, X, P and H, recompressed with the original block cuts.
    The records stay decodable under SILENT only (bins and read lengths no
    longer agree with the cigars)."""
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, r = s.decode_all()
    assert rc == 0
    u = bytearray(s.data)
    rng = np.random.default_rng(seed)
    for p in r["offset"]:
        p = int(p)
        lrn = u[p + 12]
        (ncig,) = struct.unpack_from("<H", u, p + 16)
        for k in range(ncig):
            if rng.random() < 0.5:
                at = p + 36 + lrn + 4 * k
                u[at] = (u[at] & 0xF0) | NEW_OPS[int(rng.integers(len(NEW_OPS)))]
    return recompress(s, bytes(u))


class Case:
    """A BAM with its oracle stream (SILENT), records and (ref, start, end) table."""

    def __init__(self, data):
        self.data = data
        self.stream = orc.Stream(data, stringency=orc.SILENT)
        rc, self.records = self.stream.decode_all()
        assert rc == 0
        self.u = self.stream.data
        self.table = record_table(self.u, self.records["offset"])
        self.first = self.stream.first_record_voff
        self.whole = [(self.first, len(data) << 16)]


@functools.lru_cache(maxsize=None)
def main_case():
    return Case(spread_bam(6000, PLACEMENTS[1]))


@functools.lru_cache(maxsize=None)
def unsorted_case():
    return Case(spread_bam(6000, [(4, 0, 500), (1, 5000, 300)]))


@functools.lru_cache(maxsize=None)
def long_case():
    return Case(synth.make_bam(300, seed=7, mode="long")[0])


@functools.lru_cache(maxsize=None)
def cigar_ops_case():
    return Case(with_cigar_ops(main_case().data, 5))


@functools.lru_cache(maxsize=None)
def unplaced_case():
    return Case(synth.make_bam(6000, seed=7)[0])


# interval sets on main_case() with the records each keeps from one chunk
# covering the file (None: the iteration does not stop early)
MAIN_SETS = [
    ([(1, 5000, 9999)], 17, 17),
    ([(1, 20000, 22999), (4, 1, 0)], 2010, "any"),
    ([(0, 1, 0)], 0, 0),
    ([(7, 1, 0)], 2000, None),
    ([(4, 100000, 100200), (4, 100400, 100900), (7, 2000000, 2000100)], 4, "any"),
]
LONG_SETS = [([(0, 100000, 200000), (0, 300000, 350000)], 119), ([(0, 200000, 200000)], 15)]
UNSORTED_SETS = [([(1, 5000, 9999), (4, 1, 0)], 3000, 3017), ([(1, 5000, 9999), (4, 1, 20000)], 40, 57)]


def hand_chunks(case):
    """Chunks cut by hand at record voffs in different blocks, an empty one
    among them; they leave some records out."""
    v = [int(x) for x in case.records["voff"]]
    n = len(v)
    cuts = [v[0], v[n // 7], v[n // 7], v[n // 7], v[n // 3], v[n // 2], v[n // 2 + 1], v[(4 * n) // 5],
            len(case.data) << 16]
    assert len({c >> 16 for c in cuts}) >= 5
    return [(cuts[0], cuts[1]), (cuts[2], cuts[3]), (cuts[3], cuts[4]), (cuts[5], cuts[6]), (cuts[7], cuts[8])]
