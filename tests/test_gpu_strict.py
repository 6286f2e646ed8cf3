"""The GPU's validation verdict, record by record, against the oracle's.

A span that holds exactly one record -- decode_span(voff_i, voff_{i+1}) -- has
a known entry, so the walk goes by block_size alone and the span's status and
record count are that record's verdict (k_rec_check_out: record_invalid_h for
cigars up to kWaveCigarOps = 32 operators, record_invalid_wave above).  Many
records of one file are broken in place (block_size kept, so every record
stays where it was in the inflated stream), the file is opened once per
stringency, and every verdict is compared with orc.Stream's on the same two voffs, under STRICT and
LENIENT:
  short   400 records of a 3,000-record short-read file, test_strict._mutate
  long    reads of hundreds to 4,000 M/I/D operators: the same mutations, and
          cigar patches aimed at operator 0, 1, the 64-operator chunk edge
          (62 .. 65), ncig - 2 and ncig - 1 -- placement (S, H, P), zero
          lengths, operators above 8, I / D pairs, M blocks past the reference,
          the cigar's read length, the bin.  Where a patch changes the cigar's
          read length or the bin only as a side effect, an M far from the
          patch and the bin field are adjusted, so that the verdict turns on
          the rule the patch is about.
  edge    encoded records of 31, 32, 33, 64, 65 and 129 operators (either side
          of the two passes' boundary and of the chunk edge), valid and with a
          doubled I as the last operator pair; and the empty-read rule's five
          aux variants (test_strict.test_empty_read_needs_fz_or_cq_cs).
In each of short and long at least 100 patched records are invalid under
STRICT and at least 100 valid, by the oracle alone."""
import functools
import struct

import numpy as np
import pytest

import bai
import hbam
import orc
import sam_parse_cases as spc
from bam_patch import recompress
from hbam import synth
from test_strict import _mutate, _records

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)
READ_OPS, REF_OPS = (M, I, S, EQ, X), (M, D, N, EQ, X)
FAR = 70  # operators from here on are past the chunk edge under test: the balancing M is taken there


def _spans(data):
    """(stream, record offsets, one-record spans) of a file read without validation."""
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, r = s.decode_all()
    assert rc == 0
    v = [int(x) for x in r["voff"]]
    return s, [int(x) for x in r["offset"]], list(zip(v, v[1:]))  # (the last record has no span)


class Base:
    """An unpatched file: its inflated bytes and record offsets."""

    def __init__(self, data):
        self.stream, self.off, _ = _spans(data)
        self.u = self.stream.data

    def record(self, i):
        p = self.off[i]
        return bytes(self.u[p:p + 4 + struct.unpack_from("<i", self.u, p)[0]])

    def with_records(self, recs):
        """(file, spans) with records {index: bytes} written over the
        originals, the blocks cut as before: the records stay where they
        were in the inflated stream (block_size is kept); the compressed
        blocks, and with them the voffs, move."""
        u = bytearray(self.u)
        for i, rec in recs.items():
            p = self.off[i]
            assert rec[:4] == u[p:p + 4] and len(rec) == 4 + struct.unpack_from("<i", rec, 0)[0]
            u[p:p + len(rec)] = rec
        data = recompress(self.stream, bytes(u))
        _, off, spans = _spans(data)
        assert off == self.off
        return data, spans


def oracle_verdicts(data, spans, stringency):
    s = orc.Stream(data, stringency=stringency)
    out = []
    for a, b in spans:
        rc, r = s.decode_span(a, b)
        out.append((rc, len(r["key"])))
    return out


def gpu_verdicts(data, spans, stringency):
    with hbam.BamFile(data, stringency=stringency) as f:
        out = []
        for a, b in spans:
            r = f.decode_span(a, b, raise_on_error=False)
            out.append((r["status"], len(r["key"])))
        return out


class Case:
    """A patched file, the spans of its patched records, what each patch is,
    and the oracle's verdicts (computed once, on the CPU)."""

    def __init__(self, data, spans, labels):
        self.data, self.spans, self.labels = data, spans, labels
        self.want = {st: oracle_verdicts(data, spans, st) for st in (hbam.STRICT, hbam.LENIENT)}
        for st, w in self.want.items():  # one record: taken whole or refused
            assert all(v == (0, 1) or (v[0] != 0 and v[1] == 0) for v in w), st
        # LENIENT refuses only what STRICT refuses
        assert all(s[0] != 0 for s, l in zip(self.want[hbam.STRICT], self.want[hbam.LENIENT]) if l[0] != 0)

    def split(self):
        bad = sum(1 for v in self.want[hbam.STRICT] if v[0] != 0)
        return bad, len(self.spans) - bad

    def check_gpu(self):
        for st in (hbam.STRICT, hbam.LENIENT):
            got = gpu_verdicts(self.data, self.spans, st)
            wrong = [(self.labels[k], got[k], self.want[st][k]) for k in range(len(got)) if got[k] != self.want[st][k]]
            assert not wrong, (st, len(wrong), wrong[:10])


# ---- short cigars: the lane pass
@functools.lru_cache(maxsize=None)
def short_case():
    base = Base(synth.make_bam(3000)[0])
    rng = np.random.default_rng(20)
    picks = sorted(int(i) for i in rng.choice(2999, 400, replace=False))
    recs = {}
    for i in picks:
        rec = _mutate(base.record(i), rng)
        if rng.random() < 0.3:
            rec = _mutate(rec, rng)
        recs[i] = rec
    data, spans = base.with_records(recs)
    return Case(data, [spans[i] for i in picks], ["record %d" % i for i in picks])


# ---- long cigars: the wave pass
def _cigar(rec):
    at = 36 + rec[12]
    return at, list(struct.unpack_from("<%dI" % struct.unpack_from("<H", rec, 16)[0], rec, at))


def _sum(cig, ops):
    return sum(c >> 4 for c in cig if c & 15 in ops)


def _rebin(r):
    at, cig = _cigar(r)
    pos, span = struct.unpack_from("<i", r, 8)[0], _sum(cig, REF_OPS)
    struct.pack_into("<H", r, 14, bai._reg2bin(pos, pos + (span if span > 0 else 1)) & 0xFFFF)


def edit(rec, changes, balance=True, rebin=True):
    """rec with cigar operators {k: (op or None, length or None)} replaced
    (None: kept).  balance: an M at index >= FAR takes up the change of the
    cigar's read length; rebin: the bin field follows the new reference span."""
    r = bytearray(rec)
    at, cig = _cigar(rec)
    for k, (op, ln) in changes.items():
        c = cig[k]
        cig[k] = ((c >> 4 if ln is None else ln) << 4) | (c & 15 if op is None else op)
    if balance:
        delta = struct.unpack_from("<i", rec, 20)[0] - _sum(cig, READ_OPS)
        j = next(j for j in range(FAR, len(cig) - 3)
                 if j not in changes and cig[j] & 15 == M and (cig[j] >> 4) + delta >= 1)
        cig[j] += delta << 4
    struct.pack_into("<%dI" % len(cig), r, at, *cig)
    if rebin:
        _rebin(r)
    return bytes(r)


def _nearest(cig, k, ops):
    return min((j for j in range(len(cig)) if cig[j] & 15 in ops), key=lambda j: (abs(j - k), j))


def _run(k, n, ncig):  # n consecutive operator indices from k, moved down to fit
    k = min(k, ncig - n)
    return range(k, k + n)


def targeted(rec):
    """[(label, edit's arguments)] for one long record: every kind at every
    index (as many for every record)."""
    at, cig = _cigar(rec)
    ncig = len(cig)
    out = []
    for k in (0, 1, 62, 63, 64, 65, ncig - 2, ncig - 1):
        def add(kind, *a, **kw):
            out.append(("%s at %d of %d" % (kind, k, ncig), a, kw))
        add("zero length", {k: (None, 0)})
        add("operator 9", {k: (9, None)}, balance=False, rebin=False)
        add("operator 15", {k: (15, None)}, balance=False, rebin=False)
        add("S", {k: (S, None)})
        add("H", {k: (H, None)})
        add("P", {k: (P, None)})
        a, b = _run(k, 2, ncig)
        add("P S", {a: (P, None), b: (S, None)})
        add("I I", {a: (I, None), b: (I, None)})
        add("D D", {a: (D, None), b: (D, None)})
        a, b, c = _run(k, 3, ncig)
        add("I D I", {a: (I, None), b: (D, None), c: (I, None)})
        add("D I D", {a: (D, None), b: (I, None), c: (D, None)})
        add("I M I", {a: (I, None), b: (M, None), c: (I, None)})
        add("D P D", {a: (D, None), b: (P, None), c: (D, None)})
        add("M off the reference", {k: (M, 250_000_000)}, balance=False, rebin=False)
        j = _nearest(cig, k, READ_OPS)
        add("read length + 1", {j: (None, (cig[j] >> 4) + 1)}, balance=False)
        j = _nearest(cig, k, (D,))
        add("D + 65536, bin kept", {j: (None, (cig[j] >> 4) + 65536)}, rebin=False)
        add("D + 2^23, bin kept", {j: (None, (cig[j] >> 4) + (1 << 23))}, rebin=False)
        add("D as N", {j: (N, None)})
        j = _nearest(cig, k, (M,))
        add("M as X", {j: (X, None)})
        add("M as =", {j: (EQ, None)})
    k = 0
    add("H S first", {0: (H, None), 1: (S, None)})
    add("S P first", {0: (S, None), 1: (P, None)})
    add("S H last", {ncig - 2: (S, None), ncig - 1: (H, None)})
    add("S S H last", {ncig - 3: (S, None), ncig - 2: (S, None), ncig - 1: (H, None)})
    return out


def at_reference_end(rec, ref_len, d):
    """rec moved so that its alignment ends d bases past its reference's end."""
    r = bytearray(rec)
    at, cig = _cigar(rec)
    ref = struct.unpack_from("<i", rec, 4)[0]
    struct.pack_into("<i", r, 8, ref_len[ref] - _sum(cig, REF_OPS) + d)
    _rebin(r)
    return bytes(r)


def _ref_lengths(u):
    """(names, lengths) of the BAM header at the start of the inflated bytes u."""
    p = 8 + struct.unpack_from("<i", u, 4)[0]
    n = struct.unpack_from("<i", u, p)[0]
    p += 4
    names, lens = [], []
    for _ in range(n):
        ln = struct.unpack_from("<i", u, p)[0]
        names.append(bytes(u[p + 4:p + 4 + ln - 1]))
        lens.append(struct.unpack_from("<i", u, p + 4 + ln)[0])
        p += 8 + ln
    return names, lens


LONG_RECORDS = 40


@functools.lru_cache(maxsize=None)
def long_cases():
    """The long-read file patched in rounds: every round breaks each record
    but the last in a new way."""
    base = Base(synth.make_bam(LONG_RECORDS, mode="long")[0])
    n = LONG_RECORDS - 1
    recs = [base.record(i) for i in range(n)]
    ncigs = [len(_cigar(r)[1]) for r in recs]
    mapped = [i for i in range(n) if ncigs[i] > 2 * FAR]  # (the rest are unmapped reads without a cigar)
    assert len(mapped) >= 30 and max(ncigs) > 500
    _, ref_len = _ref_lengths(base.u)
    rng = np.random.default_rng(21)
    jobs = []  # (record, label, bytes)
    for j in range(len(targeted(recs[mapped[0]]))):  # patch j on one mapped read after the other
        i = mapped[j % len(mapped)]
        lab, a, kw = targeted(recs[i])[j]
        jobs.append((i, lab, edit(recs[i], *a, **kw)))
    for t, d in enumerate((-1, 0, 1, 2, 1000)):
        i = mapped[t]
        jobs.append((i, "alignment end %+d past the reference" % d, at_reference_end(recs[i], ref_len, d)))
    for t in range(200):
        i = t % n
        r = _mutate(recs[i], rng)
        if rng.random() < 0.3:
            r = _mutate(r, rng)
        jobs.append((i, "mutation %d of record %d" % (t, i), r))
    cases = []
    while jobs:  # a round takes the first job of every record that has one left
        taken, rest = {}, []
        for j in jobs:
            if j[0] in taken:
                rest.append(j)
            else:
                taken[j[0]] = j
        order = sorted(taken)
        data, spans = base.with_records({i: taken[i][2] for i in order})
        cases.append(Case(data, [spans[i] for i in order], ["%s (record %d)" % (taken[i][1], i) for i in order]))
        jobs = rest
    return cases


# ---- the boundary of the two passes, and the empty-read rule
def _encoded(nops, rname, doubled):
    ops = [(S, 2)] if nops % 2 == 0 else []
    ops += [(M, 3) if k % 2 == 0 else ((I, 1), (D, 2))[(k // 2) % 2] for k in range(nops - len(ops))]
    if doubled:
        ops[-2:] = [(I, 1), (I, 1)]
    assert len(ops) == nops
    qlen = sum(ln for op, ln in ops if op in READ_OPS)
    cigar = b"".join(b"%d%c" % (ln, b"MIDNSHP=X"[op]) for op, ln in ops)
    return spc._line(b"r%d" % nops, b"0", rname, b"1000", b"30", cigar, b"*", b"0", b"0", spc._bases(qlen),
                     spc._quals(qlen))


EMPTY_READ_AUX = ((b"", True), (b"FZB" + b"S" + struct.pack("<i", 0), False), (b"CQZab\0CSZcd\0", False),
                  (b"CQZ\0CSZcd\0", True), (b"RGZx\0", True))


@functools.lru_cache(maxsize=None)
def edge_case():
    s = orc.Stream(synth.make_bam(60, all_unmapped=True)[0], stringency=orc.SILENT)
    head = bytes(s.data[:s.header_end])
    names, _ = _ref_lengths(head)
    recs, labels, expect = [], [], []
    for nops in (31, 32, 33, 64, 65, 129):
        for doubled in (False, True):
            recs.append(spc.encode_line(_encoded(nops, names[0], doubled), names))
            labels.append("%d operators%s" % (nops, ", I I last" if doubled else ""))
            expect.append(doubled)
    rec = _records(n_records=60, all_unmapped=True)[0]
    stem = bytearray(rec[:36 + rec[12] + 4 * struct.unpack_from("<H", rec, 16)[0]])
    struct.pack_into("<i", stem, 20, 0)  # l_seq 0: no seq / qual
    for aux, bad in EMPTY_READ_AUX:
        r = bytearray(stem + aux)
        struct.pack_into("<i", r, 0, len(r) - 4)
        recs.append(bytes(r))
        labels.append("empty read, aux %r" % aux)
        expect.append(bad)
    recs.append(bytes(rec))  # (its start ends the last span)
    payload = head + b"".join(recs)
    data = orc.bgzf_compress(payload, [len(payload)], level=5, eof=True)
    _, off, spans = _spans(data)
    assert len(off) == len(recs)
    case = Case(data, spans, labels)
    assert [v[0] != 0 for v in case.want[hbam.STRICT]] == expect
    assert all(v == (0, 1) for v in case.want[hbam.LENIENT])
    return case


def test_short_cigars_lane_pass():
    case = short_case()
    bad, good = case.split()
    assert bad >= 100 and good >= 100, (bad, good)
    case.check_gpu()


def test_long_cigars_wave_pass():
    cases = long_cases()
    bad = sum(c.split()[0] for c in cases)
    good = sum(c.split()[1] for c in cases)
    assert bad >= 100 and good >= 100, (bad, good)
    for c in cases:
        c.check_gpu()


def test_pass_boundary_and_empty_reads():
    edge_case().check_gpu()
