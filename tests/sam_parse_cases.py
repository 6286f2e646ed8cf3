"""The expected side of the SAM parse tests (hbam_parse_sam, hbam.sam.to_bam).

  float_bits      a decimal text as the nearest float32, by exact rational
                  arithmetic (fractions.Fraction): no float() on the way
  encode_line     a plain-Python SAM line -> BAM record encoder written from
                  the rules in include/hbam.h, complete: B arrays, htsjdk's
                  integer tag types (signed first), the flag-0x4 bin rule, and
                  every violation raised as BadLine
  encode_text     the lines of a text as hbam_parse_sam cuts them
  the case builders: texts with the dictionary they are parsed against

Every case asserts what it is there for on the CPU, before any comparison with
the GPU.  Test data only."""
import functools
import re
import struct
from fractions import Fraction

import numpy as np

import bai
import sam_text_cases as stc

INT_MIN, INT_MAX = stc.INT_MIN, stc.INT_MAX
LONG = 4096  # line bytes from which the whole workgroup works on one line


class BadLine(Exception):
    """The line breaks a rule of hbam_parse_sam; args[0] names the field."""


# ---- numbers ----------------------------------------------------------------------
_DEC = re.compile(rb"-?[0-9]+\Z")
_FLOAT = re.compile(rb"(-?)(?:([0-9]+)(?:\.([0-9]+))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?\Z")


def dec(text, lo, hi, field):
    """A decimal field: an optional '-', digits; in [lo, hi]."""
    if not _DEC.match(text):
        raise BadLine(field)
    v = int(text)
    if not lo <= v <= hi:
        raise BadLine(field)
    return v


def _round_half_even(x):
    """The integer nearest to the Fraction x >= 0, ties to even."""
    q, r = divmod(x.numerator, x.denominator)
    twice = 2 * r
    if twice > x.denominator or (twice == x.denominator and q & 1):
        q += 1
    return q


def float_bits(text):
    """The bits of the float32 nearest to the decimal's exact value (ties to
    even; overflow -> inf, underflow -> denormals or zero); BadLine for a text
    outside the grammar."""
    if text == b"nan":
        return 0x7FC00000
    if text in (b"inf", b"-inf"):
        return 0x7F800000 | (0x80000000 if text[:1] == b"-" else 0)
    m = _FLOAT.match(text)
    if not m:
        raise BadLine("aux")
    sign = 0x80000000 if m.group(1) else 0
    ip, fp = (m.group(2), m.group(3) or b"") if m.group(2) is not None else (b"", m.group(4))
    digits = int(ip + fp)
    e10 = int(m.group(5) or b"0") - len(fp)
    if digits == 0:
        return sign
    top = len(str(digits)) + e10  # 10^(top - 1) <= value < 10^top
    if top > 40:
        return sign | 0x7F800000
    if top < -50:
        return sign
    x = Fraction(digits) * Fraction(10) ** e10
    e = x.numerator.bit_length() - x.denominator.bit_length()  # 2^(e - 1) < x < 2^(e + 1)
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    if e < -126:
        return sign | _round_half_even(x / Fraction(2) ** -149)
    mant = _round_half_even(x / Fraction(2) ** (e - 23))  # 2^23 .. 2^24
    return sign | min(((e + 126) << 23) + mant, 0x7F800000)


def _check_float_bits():
    assert float_bits(b"1.0000000596046448") == 0x3F800001  # (through a double: 0x3F800000)
    assert int(np.float32(float("1.0000000596046448")).view(np.uint32)) == 0x3F800000
    assert float_bits(b"3.4028236e38") == 0x7F800000 and float_bits(b"3.40282356e38") == 0x7F7FFFFF
    assert float_bits(b"-0") == 0x80000000 and float_bits(b"0") == 0 and float_bits(b"-inf") == 0xFF800000
    assert float_bits(b"1e-46") == 0 and float_bits(b"1.4e-45") == 1 and float_bits(b".5") == 0x3F000000
    assert float_bits(b"16777217") == 0x4B800000 and float_bits(b"16777219") == 0x4B800002  # ties to even
    assert float_bits(b"1e99999999999999999999") == 0x7F800000 and float_bits(b"1e-99999999999999999999") == 0
    for bad in (b"", b"-", b"+1", b"1.", b".", b"1e", b"1e+", b"0x1p3", b"infinity", b"NaN", b"-nan", b"1.5x", b"1 "):
        try:
            float_bits(bad)
        except BadLine:
            continue
        raise AssertionError(bad)


_check_float_bits()


# ---- the encoder ------------------------------------------------------------------
_BASE = {c: k for k, c in enumerate(stc.NIBBLES)}
_BASE.update({c + 32: k for k, c in enumerate(stc.NIBBLES) if 65 <= c <= 90})
_BASE[ord(".")] = 15
_INT_TYPES = (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", INT_MIN, INT_MAX),
              ("I", 0, (1 << 32) - 1))  # htsjdk's BinaryTagCodec order: the signed type first
_RANGE = {t: (lo, hi) for t, lo, hi in _INT_TYPES}
_CIGAR = re.compile(rb"([0-9]*)([^0-9])")


def aux_int(tag, v):
    for t, lo, hi in _INT_TYPES:
        if lo <= v <= hi:
            return stc.aux(tag, t, v)
    raise BadLine("aux")


def encode_aux(t):
    if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
        raise BadLine("aux")
    tag, ty, val = t[:2], t[3:4], t[5:]
    if ty == b"A":
        if len(val) != 1:
            raise BadLine("aux")
        return stc.aux(tag, "A", val)
    if ty == b"i":
        return aux_int(tag, dec(val, INT_MIN, (1 << 32) - 1, "aux"))
    if ty == b"f":
        return stc.aux(tag, "f", float_bits(val))
    if ty in (b"Z", b"H"):
        return stc.aux(tag, ty.decode(), val)
    if ty == b"B":
        sub = val[:1].decode("latin-1")
        if sub == "" or sub not in "cCsSiIf":
            raise BadLine("aux")
        if len(val) == 1:
            return stc.aux(tag, "B", (sub, []))
        if val[1:2] != b",":
            raise BadLine("aux")
        elems = val[2:].split(b",")
        if sub == "f":
            return stc.aux(tag, "B", (sub, [float_bits(e) for e in elems]))
        return stc.aux(tag, "B", (sub, [dec(e, *_RANGE[sub], "aux") for e in elems]))
    raise BadLine("aux")


def encode_line(line, refs):
    """The BAM record (block_size first) of one SAM alignment line (no newline)."""
    if line == b"":
        raise BadLine("empty")
    f = line.split(b"\t")
    if len(f) < 11:
        raise BadLine("fields")
    for k, x in enumerate(f):
        if x == b"":
            raise BadLine("empty field %d" % k)
    if not 1 <= len(f[0]) <= 254:
        raise BadLine("QNAME")
    flag = dec(f[1], 0, 65535, "FLAG")

    def ref_of(x, same, field):
        if x == b"*":
            return -1
        if x == b"=" and same is not None:
            return same
        if x not in refs:
            raise BadLine(field)
        return refs.index(x)  # (the lowest index of a name that appears twice)

    ref = ref_of(f[2], None, "RNAME")
    pos = stc._wrap32(dec(f[3], INT_MIN, INT_MAX, "POS") - 1)
    mapq = dec(f[4], 0, 255, "MAPQ")
    cigar = []
    if f[5] != b"*":
        at = 0
        for m in _CIGAR.finditer(f[5]):
            if m.start() != at or m.group(1) == b"" or m.group(2) not in stc.OPS or int(m.group(1)) >= 1 << 28:
                raise BadLine("CIGAR")
            cigar.append((int(m.group(1)) << 4) | stc.OPS.index(m.group(2)))
            at = m.end()
        if at != len(f[5]) or len(cigar) > 65535:
            raise BadLine("CIGAR")
    nref = ref_of(f[6], ref, "RNEXT")
    npos = stc._wrap32(dec(f[7], INT_MIN, INT_MAX, "PNEXT") - 1)
    tlen = dec(f[8], INT_MIN, INT_MAX, "TLEN")
    if f[9] == b"*":
        nib = []
    else:
        nib = [_BASE.get(c, 16) for c in f[9]]
        if 16 in nib:
            raise BadLine("SEQ")
    if f[10] == b"*":
        qual = bytes([0xFF] * len(nib))
    else:
        if len(f[10]) != len(nib) or min(f[10]) < 33 or max(f[10]) > 126:
            raise BadLine("QUAL")
        qual = bytes(c - 33 for c in f[10])
    ax = b"".join(encode_aux(t) for t in f[11:])
    span = sum(v >> 4 for v in cigar if (v & 15) in (0, 2, 3, 7, 8))
    if flag & 4 or span == 0:
        span = 1
    bin_ = 0 if ref < 0 else bai._reg2bin(pos, pos + span) & 0xFFFF
    return stc.record(f[0] + b"\0", flag, ref, pos, mapq, cigar, nref, npos, tlen, nib, qual, ax, bin_=bin_)


def split_lines(text, final=True):
    """([lines without newline and without one '\\r' before it], consumed) as hbam_parse_sam cuts text."""
    parts = text.split(b"\n")
    tail = parts.pop()
    if final and tail != b"":
        parts.append(tail)
        tail = b""
    return [x[:-1] if x.endswith(b"\r") else x for x in parts], len(text) - len(tail)


def encode_text(text, refs, final=True):
    """(enc, offs[u64, n + 1], consumed) expected of parse_sam(text, final); BadLine carries the line index."""
    lines, consumed = split_lines(text, final)
    recs = []
    for k, x in enumerate(lines):
        try:
            recs.append(encode_line(x, refs))
        except BadLine as e:
            raise BadLine(e.args[0], k)
    offs = np.zeros(len(recs) + 1, np.uint64)
    if recs:
        offs[1:] = np.cumsum([len(r) for r in recs])
    return b"".join(recs), offs, consumed


class ParseCase:
    """A text, the dictionary it is parsed against, and the expected records."""

    def __init__(self, text, refs):
        self.text, self.refs = text, list(refs)
        self.enc, self.offs, consumed = encode_text(text, self.refs)
        assert consumed == len(text)
        self.n = len(self.offs) - 1

    def line_of_byte(self, k):
        return int(np.searchsorted(self.offs, k, side="right")) - 1


# ---- the cases --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def test_bam_case():
    """test.bam's text; every record comes back byte for byte (the self-check)."""
    t = stc.test_bam_case()
    case = ParseCase(t.text, t.refs)
    assert case.n == 2277
    return case


def test_bam_records():
    """test.bam's records as they lie in the file (block_size first)."""
    t = stc.test_bam_case()
    out = []
    for p in t.starts:
        (bs,) = struct.unpack_from("<i", t.u, int(p))
        out.append(bytes(t.u[int(p):int(p) + 4 + bs]))
    return out


@functools.lru_cache(maxsize=None)
def test_sam_case():
    _, body = stc.test_sam_lines()
    case = ParseCase(b"".join(x + b"\n" for x in body), [b"chr21"])
    assert case.n == 2
    for i, x in enumerate(body):  # the formatter gives the lines back
        assert stc.format_record(case.enc, int(case.offs[i]), case.refs) == x + b"\n"
    return case


EDGE_REFS = [b"chr10", b"chr1", b"chr", b"chr1x", b"*x", b"=", b"chr1"]  # prefixes, odd names, one name twice
INT_EDGES = [-129, -128, 127, 128, 255, 256, 32767, 32768, 65535, 65536, INT_MAX, 1 << 31, (1 << 32) - 1, INT_MIN,
             -32768, -32769, 0]
SEQ_LENS = (1, 2, 63, 64, 65, 127, 128, 129)
FLOAT_TEXTS = [b"1.0000000596046448", b".5", b"-.5", b"1e-46", b"3.4028236e38", b"3.40282356e38", b"-0", b"0", b"nan",
               b"inf", b"-inf", b"1E+2", b"1e2", b"0005.2500", b"1.4e-45", b"16777217", b"-1.17549435e-38",
               b"0.000000000000000000000000000000000000000000001"]


def _line(name=b"r", flag=b"0", rname=b"*", pos=b"0", mapq=b"0", cigar=b"*", rnext=b"*", pnext=b"0", tlen=b"0",
          seq=b"*", qual=b"*", aux=()):
    return b"\t".join([name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(aux))


def _bases(n):
    return bytes(stc.NIBBLES[(k * 5 + 1) % 16] for k in range(n))


def _quals(n):
    return bytes(33 + (k * 11) % 94 for k in range(n))


@functools.lru_cache(maxsize=None)
def edges_case():
    rng = np.random.default_rng(0x53414D34)
    L = [
        _line(),
        _line(b"*"),                                                       # stored as "*\0"
        _line(bytes(33 + (k * 7) % 94 for k in range(254))),               # l_read_name 255
        _line(b"@starts_with_at", b"65535", b"chr1", b"2147483647", b"255", b"5M", b"=", b"-2147483648", b"2147483647"),
        _line(b"wrap", b"-0", b"chr", b"-2147483648", b"000", b"*", b"chr10", b"0", b"-2147483648"),
        _line(b"zeros", b"00000000000000000000000000000000000000000000000000000000000000000000000004",
              b"chr1x", b"0000000000100", b"07", b"007M01D", b"*x", b"1", b"-0"),
        _line(b"eqname", b"0", b"=", b"5", b"0", b"3M", b"=", b"5"),        # a reference named "=", RNEXT the same
        _line(b"eqstar", b"0", b"*", b"0", b"0", b"*", b"="),               # "=" with RNAME "*" -> -1
        _line(b"twice", b"0", b"chr1", b"1", b"0", b"1M", b"chr10"),        # chr1 appears twice: index 1
        _line(b"pos0", b"0", b"chr1", b"0", b"0", b"10M"),                  # pos -1 on a contig: the span leaves bin 4680
        _line(b"pos0b", b"0", b"chr1", b"0"),                               # pos -1, no span: bin 4680
        _line(b"unmapped_flag", b"4", b"chr1", b"100000", b"0", b"100000M"),  # flag 0x4: the bin of [pos, pos + 1)
        _line(b"mapped", b"0", b"chr1", b"100000", b"0", b"100000M"),
        _line(b"noref", b"0", b"chr1", b"100000", b"0", b"5I3S2H1P"),       # reference length 0
        _line(b"allops", b"0", b"chr1", b"9", b"0", b"1M2I3D4N5S6H7P8=9X"),
        _line(b"biglen", b"0", b"chr1", b"9", b"0", b"268435455M1X268435455N"),
        _line(b"cig64", b"0", b"chr1", b"9", b"0", b"".join(b"%d%c" % (k + 1, stc.OPS[k % 9]) for k in range(64))),
        _line(b"cig65", b"0", b"chr1", b"9", b"0", b"".join(b"%d%c" % (10 ** (k % 9), stc.OPS[k % 9]) for k in range(65))),
        _line(b"cases", seq=b"acgtn.=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn", qual=_quals(37)),
        _line(b"noqual", seq=b"ACG"),
        _line(b"qualends", seq=b"AC", qual=b"!~"),
        _line(b"star1", seq=b"A", qual=b"*"),
    ]
    assert len(L[5].split(b"\t")[1]) > 64  # a number longer than a wave
    for n in SEQ_LENS:
        L.append(_line(b"seq%d" % n, seq=_bases(n), qual=_quals(n), aux=[b"NM:i:%d" % n]))
    L.append(_line(b"ints", aux=[b"X%c:i:%d" % (65 + k, v) for k, v in enumerate(INT_EDGES)]))
    L.append(_line(b"floats", aux=[b"F%c:f:%s" % (65 + k, t) for k, t in enumerate(FLOAT_TEXTS)]))
    L.append(_line(b"fmtfloats", aux=[b"G%c:f:%s" % (65 + k, stc.float_text(b).encode()) for k, b in enumerate(stc.FLOAT_BITS)]))
    L.append(_line(b"chars", aux=[b"XA:A:!", b"XZ:Z:", b"XH:H:", b"YH:H:1AE301", b"ZZ:Z:a longer string, with spaces: and:colons",
                                  b"XB:A:~", b"XC:A::"]))
    for sub in "cCsSiIf":
        small = []
        for k, c in enumerate(stc.B_COUNTS[:5]):
            e = stc._b_elements(sub, c, rng)
            small.append(b"B%d:B:%s" % (k, sub.encode()) +
                         b"".join(b"," + (stc.float_text(v).encode() if sub == "f" else b"%d" % v) for v in e))
        L.append(_line(b"arr_" + sub.encode(), seq=b"AC", qual=b"II", aux=small + [b"NM:i:7"]))
        e = stc._b_elements(sub, stc.B_COUNTS[5], rng)
        L.append(_line(b"arrbig_" + sub.encode(), aux=[b"BB:B:%s" % sub.encode() + b"".join(
            b"," + (stc.float_text(v).encode() if sub == "f" else b"%d" % v) for v in e), b"ZE:Z:end"]))
    # \r\n on every third line
    text = b"".join(x + (b"\r\n" if k % 3 == 0 else b"\n") for k, x in enumerate(L))
    case = ParseCase(text, EDGE_REFS)
    assert case.n == len(L)
    recs = [case.enc[int(case.offs[i]):int(case.offs[i + 1])] for i in range(case.n)]
    head = lambda r: struct.unpack_from("<iiiBBHHHiiii", r, 0)
    assert recs[1][36:38] == b"*\0" and head(recs[1])[3] == 2 and head(recs[2])[3] == 255
    assert head(recs[3])[1:3] == (1, INT_MAX - 1) and head(recs[3])[7] == 65535 and head(recs[3])[9:12] == (1, INT_MAX, INT_MAX)
    assert head(recs[4])[1:3] == (2, INT_MAX) and head(recs[4])[9:12] == (0, -1, INT_MIN)  # POS -2^31 wraps
    assert head(recs[5])[1:5] == (3, 99, 6, 7) and head(recs[5])[6:8] == (2, 4) and head(recs[5])[9] == 4
    assert head(recs[6])[1] == 5 and head(recs[6])[9] == 5 and head(recs[7])[9] == -1 and head(recs[8])[1] == 1
    assert head(recs[9])[5] == 0 and head(recs[10])[5] == 4680
    assert head(recs[11])[5] == bai._reg2bin(99999, 100000) != head(recs[12])[5] == bai._reg2bin(99999, 199999)
    assert head(recs[13])[5] == head(recs[11])[5]
    assert head(recs[16])[6] == 64 and head(recs[17])[6] == 65
    ints = recs[22 + len(SEQ_LENS)]
    assert b"XAs" + struct.pack("<h", -129) in ints and b"XBc\x80" in ints and b"XCc\x7f" in ints
    assert b"XDC\x80" in ints and b"XES\xff\x00" not in ints and b"XEC\xff" in ints and b"XFs\x00\x01" in ints
    assert b"XGs\xff\x7f" in ints and b"XHS\x00\x80" in ints and b"XIS\xff\xff" in ints and b"XJi\x00\x00\x01\x00" in ints
    assert b"XKi\xff\xff\xff\x7f" in ints and b"XLI\x00\x00\x00\x80" in ints and b"XMI\xff\xff\xff\xff" in ints
    assert b"XNi\x00\x00\x00\x80" in ints and b"XQc\x00" in ints
    assert b"FAf" + struct.pack("<I", 0x3F800001) in recs[23 + len(SEQ_LENS)]
    assert int(np.diff(case.offs.astype(np.int64)).max()) > 4 * 4097
    assert max(len(x) for x in L) > LONG
    return case


@functools.lru_cache(maxsize=None)
def count_case(n):
    t = stc.count_case(n)
    case = ParseCase(t.text, t.refs)
    assert case.n == n
    return case


@functools.lru_cache(maxsize=None)
def long_between_short_case():
    """Three lines of 70,001 bases (and a 17,500-element B:C) among 44-byte ones."""
    t = stc.long_between_short_case()
    case = ParseCase(t.text, t.refs)
    lens = [len(x) for x in t.lines()]
    assert case.n == 23 and sum(1 for x in lens if x > 140000) == 3 and min(lens) < 64
    return case


GOOD = [_line(b"ok%d" % k, b"0", b"chr1", b"%d" % (k + 1), b"30", b"4M", b"=", b"%d" % (k + 9), b"0", b"ACGT", b"IIII",
              [b"NM:i:%d" % k]) for k in range(6)]
_LONG_SEQ = b"ACGT" * 17500
MALFORMED = {
    "empty_line": b"",
    "only_cr": b"\r",
    "ten_fields": b"\t".join(GOOD[0].split(b"\t")[:10]),
    "empty_qname": _line(b""),
    "empty_pos": _line(pos=b""),
    "doubled_tab": _line(aux=[b"NM:i:1", b"", b"XA:A:!"]),
    "trailing_tab": _line(aux=[b"NM:i:1", b""]),
    "trailing_tab_no_aux": _line() + b"\t",
    "qname_255": _line(b"q" * 255),
    "flag_plus": _line(flag=b"+4"),
    "flag_65536": _line(flag=b"65536"),
    "flag_negative": _line(flag=b"-1"),
    "flag_not_digits": _line(flag=b"0x10"),
    "mapq_256": _line(mapq=b"256"),
    "rname_unknown": _line(rname=b"chr2"),
    "rname_longer": _line(rname=b"chr1y"),
    "rname_prefix": _line(rname=b"ch"),
    "rname_equals": _line(rname=b"=="),
    "rnext_unknown": _line(rnext=b"chrX"),
    "pos_2_31": _line(pos=b"2147483648"),
    "pos_below": _line(pos=b"-2147483649"),
    "pos_lone_minus": _line(pos=b"-"),
    "pos_many_digits": _line(pos=b"1" + b"0" * 80),
    "pnext_2_31": _line(pnext=b"2147483648"),
    "tlen_2_31": _line(tlen=b"2147483648"),
    "tlen_text": _line(tlen=b"12a"),
    "cigar_no_number": _line(cigar=b"M"),
    "cigar_no_number_2": _line(cigar=b"5MI"),
    "cigar_no_op": _line(cigar=b"10"),
    "cigar_trailing_digits": _line(cigar=b"5M10"),
    "cigar_bad_op": _line(cigar=b"5Z"),
    "cigar_lower_op": _line(cigar=b"5m"),
    "cigar_2_28": _line(cigar=b"268435456M"),
    "cigar_many_digits": _line(cigar=b"1" + b"0" * 70 + b"M"),
    "cigar_65536_ops": _line(cigar=b"1M" * 65536),
    "seq_bad_base": _line(seq=b"ACGE", qual=b"IIII"),
    "seq_bad_x": _line(seq=b"ACXT", qual=b"*"),
    "seq_star_qual_not": _line(seq=b"*", qual=b"II"),
    "qual_short": _line(seq=b"ACGT", qual=b"III"),
    "qual_long": _line(seq=b"ACGT", qual=b"IIIII"),
    "qual_space": _line(seq=b"ACGT", qual=b"II I"),
    "qual_127": _line(seq=b"ACGT", qual=b"II\x7fI"),
    "aux_short": _line(aux=[b"NM:i"]),
    "aux_no_colon": _line(aux=[b"NMxi:1"]),
    "aux_no_colon_2": _line(aux=[b"NM:ix1"]),
    "aux_a_two": _line(aux=[b"XA:A:ab"]),
    "aux_a_empty": _line(aux=[b"XA:A:"]),
    "aux_i_empty": _line(aux=[b"NM:i:"]),
    "aux_i_2_32": _line(aux=[b"NM:i:4294967296"]),
    "aux_i_below": _line(aux=[b"NM:i:-2147483649"]),
    "aux_i_plus": _line(aux=[b"NM:i:+1"]),
    "aux_f_empty": _line(aux=[b"XF:f:"]),
    "aux_f_text": _line(aux=[b"XF:f:1.5x"]),
    "aux_f_hex": _line(aux=[b"XF:f:0x1p3"]),
    "aux_f_infinity": _line(aux=[b"XF:f:infinity"]),
    "aux_f_plus": _line(aux=[b"XF:f:+1.5"]),
    "aux_f_dot": _line(aux=[b"XF:f:1."]),
    "aux_type_d": _line(aux=[b"XD:d:1.5"]),
    "aux_type_c": _line(aux=[b"NM:c:1"]),
    "aux_b_empty": _line(aux=[b"XB:B:"]),
    "aux_b_subtype": _line(aux=[b"XB:B:d,1"]),
    "aux_b_no_comma": _line(aux=[b"XB:B:c1"]),
    "aux_b_c_128": _line(aux=[b"XB:B:c,127,128"]),
    "aux_b_C_negative": _line(aux=[b"XB:B:C,-1"]),
    "aux_b_S_65536": _line(aux=[b"XB:B:S,65536"]),
    "aux_b_I_2_32": _line(aux=[b"XB:B:I,4294967296"]),
    "aux_b_empty_element": _line(aux=[b"XB:B:c,1,,2"]),
    "aux_b_trailing_comma": _line(aux=[b"XB:B:c,1,"]),
    "aux_b_float_text": _line(aux=[b"XB:B:f,1,x"]),
    "aux_b_many_digits": _line(aux=[b"XB:B:i,1" + b"0" * 70]),
    # in a line the whole workgroup works on, outside the first wave's share
    "long_seq_bad_base": _line(seq=_LONG_SEQ[:40000] + b"E" + _LONG_SEQ[40001:], qual=b"I" * 70000),
    "long_qual_bad": _line(seq=_LONG_SEQ, qual=b"I" * 50100 + b" " + b"I" * 19899),
    "long_b_bad_element": _line(aux=[b"ML:B:C" + b",255" * 3000 + b",256" + b",0" * 3000]),
}


@functools.lru_cache(maxsize=None)
def malformed_text(kind):
    """Six good lines, then the malformed one (line 6); the six good ones parse."""
    good = b"".join(x + b"\n" for x in GOOD)
    text = good + MALFORMED[kind] + b"\n"
    assert encode_text(good, EDGE_REFS)[1].size == 7
    try:
        encode_text(text, EDGE_REFS)
    except BadLine as e:
        assert e.args[1] == 6, (kind, e.args)
        return text
    raise AssertionError("the test-side encoder accepts " + kind)
