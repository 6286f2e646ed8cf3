"""The expected side of the SAM text tests (hbam_format_sam, hbam.sam.view).

  format_record   a plain-Python formatter of one BAM record, written from the
                  rules in include/hbam.h and the SAM specification (1.4 / 1.5,
                  4.2), independent of the C++: floats go through Python's own
                  '%g' of the float32's value
  encode_line     a small SAM line -> BAM record encoder
  the case builders: BAMs of hand-packed records put behind a header with the
                  oracle's BGZF writer, as sort_cases.packed_bam and
                  name_cases.named_bam do

Every case asserts what it is there for on the CPU, before any comparison with
the GPU.  Test data only."""
import functools
import os
import struct

import numpy as np

import bai
import orc
import sort_cases as sc
from conftest import GOLDEN
from hbam import synth

NIBBLES = b"=ACMGRSVTWYHKDBN"
OPS = b"MIDNSHP=X"
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
TILE = 16384  # output bytes per workgroup of the write pass
LONG = 4096   # line bytes from which the whole workgroup works on one line


class Malformed(Exception):
    """The record's aux fields (or its fixed-length fields) leave the record."""


# ---- the formatter --------------------------------------------------------------
def float_text(bits):
    """printf("%g") of the float32 with these bits; a NaN has no sign."""
    v = float(np.uint32(bits).view(np.float32))
    if v != v:
        return "nan"
    return "%g" % v


_SCALAR = {ord("c"): ("<b", 1), ord("C"): ("<B", 1), ord("s"): ("<h", 2), ord("S"): ("<H", 2),
           ord("i"): ("<i", 4), ord("I"): ("<I", 4)}


def _element(u, p, t):
    if t == ord("f"):
        return float_text(struct.unpack_from("<I", u, p)[0])
    return str(struct.unpack_from(_SCALAR[t][0], u, p)[0])


def aux_text(u, a, end):
    """The aux fields u[a:end] as text, a tab before every tag."""
    out = []
    while a < end:
        if end - a < 3:
            raise Malformed("tag header cut by the end")
        tag, t = bytes(u[a:a + 2]), u[a + 2]
        a += 3
        if t == ord("A"):
            if end - a < 1:
                raise Malformed("A")
            val, a = b"A:" + bytes(u[a:a + 1]), a + 1
        elif t in _SCALAR or t == ord("f"):
            size = 4 if t == ord("f") else _SCALAR[t][1]
            if end - a < size:
                raise Malformed("scalar")
            val = (b"f:" if t == ord("f") else b"i:") + _element(u, a, t).encode()
            a += size
        elif t in (ord("Z"), ord("H")):
            nul = bytes(u[a:end]).find(b"\0")
            if nul < 0:
                raise Malformed("no NUL")
            val, a = bytes([t]) + b":" + bytes(u[a:a + nul]), a + nul + 1
        elif t == ord("B"):
            if end - a < 5:
                raise Malformed("B header")
            sub, count = u[a], struct.unpack_from("<I", u, a + 1)[0]
            if sub not in _SCALAR and sub != ord("f"):
                raise Malformed("B subtype")
            size = 4 if sub == ord("f") else _SCALAR[sub][1]
            a += 5
            if (end - a) // size < count:
                raise Malformed("B elements")
            val = b"B:" + bytes([sub]) + b"".join(b"," + _element(u, a + k * size, sub).encode() for k in range(count))
            a += count * size
        else:
            raise Malformed("type %r" % chr(t))
        out.append(b"\t" + tag + b":" + val)
    return b"".join(out)


def _wrap32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def format_record(u, p, refs):
    """The SAM line (with its newline) of the record whose block_size is at u[p]."""
    bs, ref, pos, lrn, mapq, _bin, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", u, p)
    end = p + 4 + bs
    a = p + 36
    if lseq < 0 or lrn + 4 * ncig + (lseq + 1) // 2 + lseq > end - a:
        raise Malformed("fixed-length fields")

    def refname(r):
        return b"*" if r < 0 or r >= len(refs) else refs[r]

    f = [b"*" if lrn <= 1 else bytes(u[a:a + lrn - 1]), str(flag).encode(), refname(ref),
         str(_wrap32(pos + 1)).encode(), str(mapq).encode()]
    a += lrn
    if ncig == 0:
        f.append(b"*")
    else:
        ops = struct.unpack_from("<%dI" % ncig, u, a)
        f.append(b"".join(str(v >> 4).encode() + (OPS[v & 15:(v & 15) + 1] or b"?") for v in ops))
    a += 4 * ncig
    f.append(b"*" if nref < 0 or nref >= len(refs) else b"=" if nref == ref else refs[nref])
    f += [str(_wrap32(npos + 1)).encode(), str(tlen).encode()]
    if lseq == 0:
        f += [b"*", b"*"]
    else:
        packed = np.frombuffer(bytes(u[a:a + (lseq + 1) // 2]), np.uint8)
        nib = np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:lseq]
        f.append(np.frombuffer(NIBBLES, np.uint8)[nib].tobytes())
        q = np.frombuffer(bytes(u[a + (lseq + 1) // 2:a + (lseq + 1) // 2 + lseq]), np.uint8)
        f.append(b"*" if q[0] == 0xFF else ((q.astype(np.uint16) + 33) & 0xFF).astype(np.uint8).tobytes())
    a += (lseq + 1) // 2 + lseq
    return b"\t".join(f) + aux_text(u, a, end) + b"\n"


def format_stream(u, starts, refs):
    """(text, offs[u64, n + 1]) of the records starting at `starts` in u."""
    lines = [format_record(u, int(p), refs) for p in starts]
    offs = np.zeros(len(lines) + 1, np.uint64)
    if lines:
        offs[1:] = np.cumsum([len(x) for x in lines])
    return b"".join(lines), offs


# ---- the encoder ----------------------------------------------------------------
def aux_int(tag, v):
    """An integer tag in the smallest type that holds it (as htsjdk and samtools choose)."""
    for t, fmt, lo, hi in (("C", "<B", 0, 255), ("c", "<b", -128, 127), ("S", "<H", 0, 65535),
                           ("s", "<h", -32768, 32767), ("I", "<I", 0, (1 << 32) - 1), ("i", "<i", INT_MIN, INT_MAX)):
        if lo <= v <= hi:
            return tag + t.encode() + struct.pack(fmt, v)
    raise ValueError(v)


def aux(tag, t, value=None):
    """One aux field: t = a type letter; for "B" value = (subtype, [elements])
    (float elements as uint32 bit patterns)."""
    tag = tag if isinstance(tag, bytes) else tag.encode()
    if t == "A":
        return tag + b"A" + bytes(value)
    if t in "cCsSiI":
        return tag + t.encode() + struct.pack(_SCALAR[ord(t)][0], value)
    if t == "f":  # value: the bit pattern
        return tag + b"f" + struct.pack("<I", value)
    if t in "ZH":
        return tag + t.encode() + bytes(value) + b"\0"
    sub, elems = value
    fmt = "<I" if sub == "f" else _SCALAR[ord(sub)][0]
    return tag + b"B" + sub.encode() + struct.pack("<I", len(elems)) + b"".join(struct.pack(fmt, e) for e in elems)


def record(name=b"r\0", flag=0, ref=-1, pos=-1, mapq=0, cigar=(), nref=-1, npos=-1, tlen=0, nibbles=(), qual=None,
           aux_bytes=b"", l_read_name=None, l_seq=None, bin_=None):
    """A BAM record (block_size first).  name: the read_name field with its
    NUL; cigar: u32 values; nibbles: base codes; qual: bytes (default 30s)."""
    nibbles = list(nibbles)
    n = len(nibbles)
    qual = bytes([30] * n) if qual is None else bytes(qual)
    packed = bytes(((nibbles[i] << 4) | (nibbles[i + 1] if i + 1 < n else 0)) for i in range(0, n, 2))
    rest = bytes(name) + b"".join(struct.pack("<I", v) for v in cigar) + packed + qual + bytes(aux_bytes)
    lrn = len(name) if l_read_name is None else l_read_name
    b = bin_ if bin_ is not None else 4680 if ref < 0 or pos < 0 else bai._reg2bin(pos, pos + 1)
    return struct.pack("<iiiBBHHHiiii", 32 + len(rest), ref, pos, lrn, mapq, b, len(cigar), flag,
                       n if l_seq is None else l_seq, nref, npos, tlen) + rest


def encode_line(line, refs):
    """The BAM record of one SAM alignment line (no newline)."""
    f = line.split(b"\t")
    ref = -1 if f[2] == b"*" else refs.index(f[2])
    nref = -1 if f[6] == b"*" else ref if f[6] == b"=" else refs.index(f[6])
    cigar = []
    if f[5] != b"*":
        num = b""
        for ch in f[5]:
            if 48 <= ch <= 57:
                num += bytes([ch])
            else:
                cigar.append((int(num) << 4) | OPS.index(bytes([ch])))
                num = b""
    nib = [] if f[9] == b"*" else [NIBBLES.index(bytes([c])) for c in f[9]]
    qual = bytes([0xFF] * len(nib)) if f[10] == b"*" else bytes(c - 33 for c in f[10])
    ax = b""
    for t in f[11:]:
        tag, ty, val = t[:2], t[3:4], t[5:]
        if ty == b"i":
            ax += aux_int(tag, int(val))
        elif ty == b"A":
            ax += aux(tag, "A", val)
        elif ty in (b"Z", b"H"):
            ax += aux(tag, ty.decode(), val)
        elif ty == b"f":
            ax += aux(tag, "f", int(np.float32(float(val)).view(np.uint32)))
        else:
            raise ValueError(t)
    pos = int(f[3]) - 1
    span = sum(v >> 4 for v in cigar if (v & 15) in (0, 2, 3, 7, 8)) or 1
    return record(f[0] + b"\0", int(f[1]), ref, pos, int(f[4]), cigar, nref, int(f[7]) - 1, int(f[8]), nib, qual, ax,
                  bin_=4680 if ref < 0 or pos < 0 else bai._reg2bin(pos, pos + span))


# ---- BAMs -----------------------------------------------------------------------
def bam_header(text, refs):
    """The BAM header bytes: text and the binary dictionary refs = [(name, length)]."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, ln in refs:
        out += [struct.pack("<i", len(name) + 1), name, b"\0", struct.pack("<i", ln)]
    return b"".join(out)


def bam_of(recs, header=None, block=60000):
    payload = (sc._header() if header is None else header) + b"".join(recs)
    lens = [min(block, len(payload) - p) for p in range(0, len(payload), block)]
    return orc.bgzf_compress(payload, lens, level=5, eof=True)


class TextCase:
    """A BAM, its inflated stream, record starts and reference names (from the
    oracle, SILENT), and the expected text."""

    def __init__(self, data):
        self.data = data
        self.stream = orc.Stream(data, stringency=orc.SILENT)
        rc, self.cols = self.stream.decode_all()
        assert rc == 0
        self.u = bytes(self.stream.data)
        self.starts = self.cols["offset"].astype(np.int64)
        self.n = len(self.starts)
        self.refs = header_refs(self.u)
        self.text, self.offs = format_stream(self.u, self.starts, self.refs)
        self.lens = np.diff(self.offs.astype(np.int64))

    def lines(self):
        o = [int(x) for x in self.offs]
        return [self.text[o[i]:o[i + 1]] for i in range(self.n)]

    def header_text(self):
        (l_text,) = struct.unpack_from("<i", self.u, 4)
        t = self.u[8:8 + l_text]
        return t + b"\n" if t and not t.endswith(b"\n") else t


def header_refs(u):
    """The names of the binary dictionary of the inflated BAM u."""
    assert u[:4] == b"BAM\x01"
    (l_text,) = struct.unpack_from("<i", u, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", u, p)
    p += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", u, p)
        names.append(bytes(u[p + 4:p + 4 + ln]).rstrip(b"\0"))
        p += 8 + ln
    return names


@functools.lru_cache(maxsize=None)
def test_bam_case():
    return TextCase(open(os.path.join(GOLDEN, "test.bam"), "rb").read())


# ---- test.sam: the reference's own text fixture ---------------------------------
def test_sam_lines():
    """(header text, [alignment lines without newline]) of tests/golden/test.sam."""
    raw = open(os.path.join(GOLDEN, "test.sam"), "rb").read()
    lines = raw.split(b"\n")
    assert lines[-1] == b""
    head = [x for x in lines[:-1] if x.startswith(b"@")]
    body = [x for x in lines[:-1] if not x.startswith(b"@")]
    return b"".join(x + b"\n" for x in head), body


@functools.lru_cache(maxsize=None)
def test_sam_case():
    text, body = test_sam_lines()
    refs = [(b"chr21", 62435964)]
    assert b"SN:chr21\tLN:62435964" in text and len(body) == 2
    case = TextCase(bam_of([encode_line(x, [r[0] for r in refs]) for x in body], bam_header(text, refs)))
    assert case.n == 2 and case.refs == [b"chr21"]
    return case


# ---- field edges ----------------------------------------------------------------
FLOAT_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x00000001, 0x007FFFFF,
              0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000,
              0x47C35040,  # 100000.5: a tie at the sixth digit, to even (100000)
              0x47C350C0,  # 100001.5 -> 100002
              0x49742450,  # 1000005 -> 1e+06
              0x497424F0,  # 1000015 -> 1.00002e+06
              0x38D1B717,  # ~1e-4: the fixed / exponent switch
              0x38D1B716, 0x4974239F, 0x49742400, 0x497423F8,  # around 999999.5 and 1e6
              0x3DCCCCCD, 0x40490FDB, 0x501502F9, 0x2EDBE6FF]


def _check_float_bits():
    f = lambda b: float(np.uint32(b).view(np.float32))
    assert f(0x47C35040) == 100000.5 and f(0x47C350C0) == 100001.5 and f(0x49742450) == 1000005.0
    assert float_text(0x47C35040) == "100000" and float_text(0x47C350C0) == "100002"
    assert float_text(0x49742450) == "1e+06" and float_text(0x80000000) == "-0"
    assert float_text(0x00000001) == "1.4013e-45" and float_text(0xFFC00001) == "nan"
    assert float_text(0xFF800000) == "-inf" and float_text(0x3F800000) == "1"


_check_float_bits()

B_COUNTS = (0, 1, 63, 64, 65, 4097)
_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (INT_MIN, INT_MAX),
          "I": (0, (1 << 32) - 1)}
# values on both sides of every digit boundary, both signs
DIGIT_EDGES = [0] + [s * (10 ** k + d) for k in range(0, 10) for d in (-1, 0) for s in (1, -1)]


def _b_elements(sub, count, rng):
    if sub == "f":
        pool = FLOAT_BITS + [int(x) for x in rng.integers(0, 1 << 32, 40, dtype=np.uint64)]
        return [pool[k % len(pool)] for k in range(count)]
    lo, hi = _RANGE[sub]
    pool = [lo, hi] + [v for v in DIGIT_EDGES if lo <= v <= hi]
    return [pool[(k * 7) % len(pool)] for k in range(count)]


@functools.lru_cache(maxsize=None)
def edges_case():
    rng = np.random.default_rng(0x53414D31)
    name255 = bytes(33 + (k * 7) % 94 for k in range(254)) + b"\0"
    all_ops = [((k + 1) << 4) | k for k in range(16)]  # nine ops and op 9-15
    wide_cigar = [(abs(v) << 4) | (k % 9) for k, v in enumerate(DIGIT_EDGES * 3) if abs(v) < (1 << 28)]
    assert len(wide_cigar) > 64  # widths change inside a wave and across two
    recs = [
        record(b"plain\0"),                                             # ref -1, RNEXT *, pos -1, no cigar, l_seq 0, no aux
        record(b"same\0", ref=0, pos=9, nref=0, npos=99, nibbles=[1, 2, 4, 8]),          # RNEXT =
        record(b"other\0", ref=0, pos=9, nref=2, npos=0, nibbles=[1]),                   # RNEXT another contig
        record(b"half\0", ref=-1, pos=-1, nref=1, npos=5, nibbles=[1, 2]),               # RNAME *, RNEXT a name
        record(b"ends\0", flag=65535, mapq=255, ref=3, pos=0, tlen=INT_MIN),
        record(b"ends2\0", ref=3, pos=INT_MAX - 1, npos=-1, tlen=INT_MAX, bin_=0),
        record(b"ops\0", ref=1, pos=3, cigar=all_ops, nibbles=list(range(16))),          # all 16 nibble codes
        record(b"biglen\0", ref=1, pos=3, cigar=[((1 << 28) - 1) << 4 | 0, 1 << 4 | 8]),
        record(b"wide\0", ref=1, pos=3, cigar=wide_cigar),
        record(b"\0"),                                                  # l_read_name 1 -> *
        record(b"a\0"),                                                 # l_read_name 2
        record(name255),                                                # l_read_name 255
        record(b"noqual\0", nibbles=[1, 2, 4], qual=[0xFF, 0xFF, 0xFF]),
        record(b"quals\0", nibbles=[1, 2, 4, 8], qual=[0, 93, 222, 223]),  # 222 + 33 = 255, 223 wraps to 0
    ]
    for n in (1, 2, 63, 64, 65):
        recs.append(record(b"seq%d\0" % n, nibbles=[(k * 5 + 1) % 16 for k in range(n)],
                           qual=[(k * 11) % 94 for k in range(n)]))
    scal = b"".join(aux("X" + t, t, v) for t in "cCsSiI" for v in _RANGE[t])
    scal += b"".join(aux("F%d" % (k % 10), "f", b) for k, b in enumerate(FLOAT_BITS))
    recs.append(record(b"scalars\0", aux_bytes=scal))
    recs.append(record(b"chars\0", aux_bytes=aux("XA", "A", b"!") + aux("XZ", "Z", b"") + aux("XH", "H", b"1AE301") +
                       aux("ZZ", "Z", b"a longer string, with spaces") + aux("XB", "A", b"~")))
    recs.append(record(b"digits\0", aux_bytes=b"".join(aux_int(b"D%d" % (k % 10), v) for k, v in enumerate(DIGIT_EDGES)
                                                        if INT_MIN <= v <= INT_MAX)))
    for sub in "cCsSiIf":
        small = b"".join(aux("B%d" % k, "B", (sub, _b_elements(sub, c, rng))) for k, c in enumerate(B_COUNTS[:5]))
        recs.append(record(b"arr_" + sub.encode() + b"\0", nibbles=[1, 2], aux_bytes=small + aux("NM", "C", 7)))
        recs.append(record(b"arrbig_" + sub.encode() + b"\0",
                           aux_bytes=aux("BB", "B", (sub, _b_elements(sub, B_COUNTS[5], rng))) + aux("ZE", "Z", b"end")))
    case = TextCase(bam_of(recs))
    assert case.n == len(recs)
    lines = case.lines()
    assert lines[0] == b"plain\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
    assert lines[1].split(b"\t")[6] == b"=" and lines[2].split(b"\t")[6] == case.refs[2]
    assert lines[3].split(b"\t")[2] == b"*" and lines[3].split(b"\t")[6] == case.refs[1]
    assert b"\t65535\t" in lines[4] and b"\t255\t" in lines[4] and b"\t-2147483648\t" in lines[4]
    assert b"\t2147483647\t" in lines[5]
    assert lines[6].split(b"\t")[5] == b"1M2I3D4N5S6H7P8=9X10?11?12?13?14?15?16?"
    assert lines[6].split(b"\t")[9] == NIBBLES
    assert lines[7].split(b"\t")[5] == b"268435455M1X"
    assert lines[9].startswith(b"*\t") and lines[10].startswith(b"a\t") and lines[11].startswith(name255[:-1] + b"\t")
    assert lines[12].split(b"\t")[10] == b"*\n" and lines[13].split(b"\t")[10] == b"!~\xff\x00\n"
    assert b"\tXZ:Z:\t" in case.text and b"\tXH:H:1AE301\t" in case.text and b"\tXA:A:!\t" in case.text
    assert b"\tXc:i:-128\tXc:i:127\tXC:i:0\tXC:i:255\t" in case.text and b"\tXI:i:4294967295\t" in case.text
    assert b":f:100000\t" in case.text and b":f:1e+06\t" in case.text and b":f:1.4013e-45\t" in case.text
    assert b"\tB0:B:c\tB1:B:c,-128\t" in case.text
    assert int(case.lens.max()) > TILE  # a 4,097-element array is longer than a tile
    return case


# ---- sizes ----------------------------------------------------------------------
def small_record(k):
    """A 40-byte record (a 44-byte line or so)."""
    return record(b"q%02d\0" % (k % 100), ref=k % 3, pos=k)


@functools.lru_cache(maxsize=None)
def count_case(n):
    case = TextCase(bam_of([small_record(k) for k in range(n)]))
    assert case.n == n
    return case


@functools.lru_cache(maxsize=None)
def long_between_short_case():
    """Records longer than a tile (l_seq 70,001, a 17,500-element B:C) between 40-byte ones."""
    rng = np.random.default_rng(0x53414D32)
    recs = []
    for k in range(3):
        recs += [small_record(10 * k + j) for j in range(5)]
        nib = rng.integers(0, 16, 70001).tolist()
        ml = rng.integers(0, 256, 17500).tolist()
        recs.append(record(b"long%d\0" % k, ref=2, pos=100, cigar=[(70001 << 4) | 0], nibbles=nib,
                           qual=rng.integers(0, 94, 70001).astype(np.uint8).tobytes(),
                           aux_bytes=aux("ML", "B", ("C", ml)) + aux_int(b"NM", k)))
    recs += [small_record(90 + j) for j in range(5)]
    case = TextCase(bam_of(recs))
    assert case.n == 23 and int(np.count_nonzero(case.lens > 8 * TILE)) == 3
    assert int(case.lens.min()) < 64
    return case


@functools.lru_cache(maxsize=None)
def synth_case(mode):
    n = 5000 if mode == "short" else 40
    case = TextCase(synth.make_bam(n, mode=mode, seed=0x53414D33)[0])
    assert case.n == n
    if mode == "short":
        assert len(case.text) > 40 * TILE and int(case.lens.max()) < LONG  # many tiles, every line one wave's
    else:
        assert int(case.lens.max()) > 2 * TILE and b"\tML:B:C," in case.text
    return case


# ---- malformed aux --------------------------------------------------------------
MALFORMED = {
    "unknown_type": b"XXq\x01\x02",
    "type_d": b"XDd" + struct.pack("<d", 1.5),
    "z_no_nul": b"XZZno terminator here",
    "h_no_nul": b"XHH1AE3",
    "b_subtype": b"XBBd" + struct.pack("<I", 1) + bytes(8),
    "b_past_end": b"XBBi" + struct.pack("<I", 1000) + bytes(12),
    "b_header_cut": b"XBBi\x01\x00",
    "header_cut": b"NMC\x05XY",
    "scalar_cut": b"XIi\x01\x02",
}


@functools.lru_cache(maxsize=None)
def malformed_case(kind):
    """Six good records, then one whose aux is malformed, as the last record of the data."""
    recs = [record(b"ok%d\0" % k, ref=0, pos=k, nibbles=[1, 2, 4, 8], aux_bytes=aux_int(b"NM", k)) for k in range(6)]
    recs.append(record(b"bad\0", nibbles=[1, 2], aux_bytes=aux_int(b"NM", 1) + MALFORMED[kind]))
    data = bam_of(recs)
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, cols = s.decode_all()
    assert rc == 0 and len(cols["offset"]) == 7
    u = bytes(s.data)
    assert int(cols["offset"][6]) + 36 + int(cols["rest_len"][6]) == len(u)  # the last record ends the data
    refs = header_refs(u)
    for p in cols["offset"][:6]:
        format_record(u, int(p), refs)
    try:
        format_record(u, int(cols["offset"][6]), refs)
    except Malformed:
        return data
    raise AssertionError("the test-side formatter accepts " + kind)
