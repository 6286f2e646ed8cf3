"""DEFLATE streams zlib's deflate() never writes, built by deflate_enc: the
cases of test_deflate_enc.py (zlib's inflate decides each of them, on the CPU)
and of test_gpu_inflate_shapes.py (the GPU decoder has to agree with it).

A case is the CDATA of one BGZF block.  A valid case carries the bytes it
stands for (`out` = expand(tokens), cut to `isize` where the footer is smaller
on purpose); an invalid one carries the status [htsjdk] BlockGunzipper would
end with ("E_IO": zlib refuses the stream, with `msg` in its message;
"E_FORMAT": the stream comes up short of ISIZE)."""
import functools
from collections import namedtuple

import numpy as np

import deflate_enc as enc

Case = namedtuple("Case", "id cdata out isize want msg lean0")
# lean0: True where the design fixes that round 0 of this BGZF block is not a
# lean one (its first DEFLATE block is not a well-formed dynamic one)

LETTERS = list(range(32, 96))  # the 64-letter alphabet of test_gpu_inflate_lean.letters()


def lits(b):
    return [("L", int(v)) for v in b]


def rand_letters(rng, n, k=64, lo=32):
    return bytes(rng.integers(lo, lo + k, n, dtype=np.uint8))


def rand_tokens(rng, n, pos, maxdist=32768, k=64):
    """n tokens, about a third of them matches (short lengths and near
    distances more likely), for an output that already holds `pos` bytes."""
    out = []
    for _ in range(n):
        if pos == 0 or rng.random() < 0.65:
            out.append(("L", 32 + int(rng.integers(k))))
            pos += 1
            continue
        length = int(min(258, 3 + rng.geometric(0.08)))
        d = int(min(pos, maxdist, rng.geometric(0.002) if rng.random() < 0.7 else rng.integers(1, 32769)))
        out.append(("M", length, d))
        pos += length
    return out


def enc_auto(payload):
    """The payload as one final dynamic block of literals."""
    return Stream().auto(lits(payload), True).w.getvalue()


def lengths_at(n, pairs):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


class Stream:
    """DEFLATE blocks written one after another, and the tokens they stand for."""

    def __init__(self):
        self.w, self.toks = enc.BitWriter(), []

    @property
    def pos(self):
        return sum(1 if t[0] == "L" else t[1] for t in self.toks)

    def dyn(self, tokens, ll, dl, final=False, **kw):
        enc.put_dynamic(self.w, tokens, ll, dl, final, **kw)
        self.toks += tokens
        return self

    def auto(self, tokens, final=False, **kw):
        enc.put_auto(self.w, tokens, final, **kw)
        self.toks += tokens
        return self

    def fixed(self, tokens, final=False):
        enc.put_fixed(self.w, tokens, final)
        self.toks += tokens
        return self

    def stored(self, payload, final=False, nlen=None):
        enc.put_stored(self.w, payload, final, nlen)
        self.toks += lits(payload)
        return self

    def ok(self, cid, isize=None, fill=0, lean0=False):
        out = enc.expand(self.toks)
        if isize is not None:
            out = out[:isize]
        assert 0 < len(out) <= 65536
        return Case(cid, self.w.getvalue(fill), out, len(out), "OK", None, lean0)

    def bad(self, cid, want, msg, isize, lean0=False):
        return Case(cid, self.w.getvalue(), None, isize, want, msg, lean0)


REGISTRY = {}  # id -> builder; insertion order is the order of the tables in the issue


VALID, INVALID = [], []


def case(cid, valid=True):
    def reg(fn):
        assert cid not in REGISTRY
        REGISTRY[cid] = fn
        (VALID if valid else INVALID).append(cid)
        return fn
    return reg


@functools.lru_cache(maxsize=None)
def get(cid):
    c = REGISTRY[cid]()
    assert c.id == cid and len(c.cdata) + 26 <= 65536, (cid, len(c.cdata))
    return c


# ---------------------------------------------------------------- block structure
S1_LL = lengths_at(257, [(65, 2), (67, 2), (71, 2), (84, 3), (256, 3)])


@case("S1")
def _s1():
    rng = np.random.default_rng(101)
    data = bytes(np.array([65, 67, 71, 84], dtype=np.uint8)[rng.integers(0, 4, 65280)])
    return Stream().dyn(lits(data), S1_LL, [1], True).ok("S1")


S2_LL = lengths_at(257, [(c, 6) for c in LETTERS[:63]] + [(LETTERS[63], 7), (256, 7)])
for _n in (65280, 65536):
    @case("S2-%d" % _n)
    def _s2(n=_n):
        return Stream().dyn(lits(rand_letters(np.random.default_rng(102), n)), S2_LL, [1], True).ok("S2-%d" % n)


def long_nonfinal(cid, n, k):
    """A non-final dynamic block of n literals over k letters (S1's or S2's code), then a short
    final block under another code.  The first all-lane pass over a non-final block ends
    where block_bits_estimate puts the end of a 16,383-symbol block (a final block runs to the
    end of CDATA in one pass, so S1 and S2 never continue); the rest takes n / 16,383 times as
    many bits, in continuation passes of a quarter of the estimate each."""
    rng = np.random.default_rng(110)
    if k == 4:
        s = Stream().dyn(lits(bytes(np.array([65, 67, 71, 84], dtype=np.uint8)[rng.integers(0, 4, n)])), S1_LL, [1])
    else:
        s = Stream().dyn(lits(rand_letters(rng, n)), S2_LL, [1])
    return s.auto(rand_tokens(rng, 1500, s.pos), True).ok(cid)


case("S1-cont1")(lambda: long_nonfinal("S1-cont1", 20000, 4))  # one continuation pass
case("S1-cont")(lambda: long_nonfinal("S1-cont", 52000, 4))
case("S2-cont")(lambda: long_nonfinal("S2-cont", 45000, 64))  # the round's CDATA is more than the lean stage holds


def s3(cid, nstored=777, order="dsd", nlen=None):
    """A dynamic block of 3,001 literals ("d"), a stored block ("s") and a
    dynamic block whose first token is a match reaching back through the block
    before it into the one before that (distance: that block's length + 100,
    so 877 past the 777 stored bytes of S3), in the given order."""
    rng = np.random.default_rng(103)
    s, sizes, last_d = Stream(), [], order.rindex("d")
    for i, kind in enumerate(order):
        before = s.pos
        if kind == "s":
            if i:
                assert (s.w.nbits + 3) % 8, "the stored block must start off a byte boundary"
            s.stored(bytes(rng.integers(0, 256, nstored, dtype=np.uint8)), i == 2, nlen)
        elif i == last_d:
            d = min(32768, s.pos, sizes[-1] + 100 if i == 2 else 877)
            s.auto([("M", 258, d)] + rand_tokens(rng, 400, s.pos + 258), i == 2)
        else:
            s.auto(lits(rand_letters(rng, 3001)), i == 2)
        sizes.append(s.pos - before)
    if nlen is not None:
        return s.bad(cid, "E_IO", "invalid stored block lengths", s.pos)
    return s.ok(cid, lean0=order[0] == "s")


case("S3")(lambda: s3("S3"))
case("S3b")(lambda: s3("S3b", 0))
case("S3c")(lambda: s3("S3c", 40000))
case("S3d")(lambda: s3("S3d", order="sdd"))
case("S3e")(lambda: s3("S3e", order="dds"))
case("S3f", False)(lambda: s3("S3f", nlen=0x1234))


@case("S4")
def _s4():
    rng = np.random.default_rng(104)
    s = Stream()
    for i in range(300):
        s.auto(lits(rand_letters(rng, int(rng.integers(0, 40)))), i == 299, clen_mode=dict(rle=i % 2 == 0))
    return s.ok("S4")


H1_LL = lengths_at(257, [(65, 1), (256, 1)])


@case("S4-empty")
def _s4e():
    s = Stream()
    for _ in range(300):
        s.dyn([], H1_LL, [0])
    return s.auto(rand_tokens(np.random.default_rng(105), 3000, 0), True).ok("S4-empty")


@case("S5-fixed-dyn")
def _s5a():
    rng = np.random.default_rng(106)
    s = Stream().fixed(rand_tokens(rng, 2500, 0))
    return s.auto(rand_tokens(rng, 2500, s.pos), True).ok("S5-fixed-dyn", lean0=True)


@case("S5-dyn-fixed")
def _s5b():
    rng = np.random.default_rng(107)
    s = Stream().auto(rand_tokens(rng, 2500, 0))
    return s.fixed(rand_tokens(rng, 2500, s.pos), True).ok("S5-dyn-fixed")


@case("S6-empty-first")
def _s6a():
    s = Stream().dyn([], H1_LL, [0])
    return s.auto(rand_tokens(np.random.default_rng(108), 3000, 0), True).ok("S6-empty-first")


S6_LL = lengths_at(257, [(65, 2), (66, 2), (67, 2), (68, 3), (256, 3)])
for _pad in range(8):
    @case("S6-pad%d" % _pad)
    def _s6b(pad=_pad):
        """The end-of-block code ends `pad` bits before the end of CDATA; the
        padding bits are ones (pad 0: the EOB's last bit is the last bit)."""
        rng = np.random.default_rng(109)
        body = lits(bytes(np.array([65, 66, 67], dtype=np.uint8)[rng.integers(0, 3, 5000)]))
        for k in range(8):  # each 3-bit literal moves the end by 3 bits: every residue is reached
            s = Stream().dyn(body + [("L", 68)] * k, S6_LL, [1], True)
            if -s.w.nbits % 8 == pad:
                return s.ok("S6-pad%d" % pad, fill=1)
        raise AssertionError("alignment not reached")


# ---------------------------------------------------------------- match geometry
M1_TAIL = [("M", 258, 32768), ("M", 258, 1), ("M", 3, 32768), ("M", 258, 32768)]


@case("M1")
def _m1():
    return Stream().auto(lits(rand_letters(np.random.default_rng(201), 32768)) + M1_TAIL, True).ok("M1")


@case("M2", False)
def _m2():
    s = Stream()
    enc.put_auto(s.w, lits(rand_letters(np.random.default_rng(202), 32767)) + [("M", 258, 32768)], True)
    return s.bad("M2", "E_IO", "invalid distance too far back", 32767 + 258)


def m2b(cid, after, pos, over):
    """A match of distance pos (+1: one too far) as the first token of the
    second DEFLATE block, the first one a dynamic or a stored block of pos bytes."""
    rng = np.random.default_rng(203)
    s = Stream()
    head = rand_letters(rng, pos)
    if after == "dyn":
        s.auto(lits(head))
    else:
        s.stored(head)
    tail = rand_tokens(rng, 300, pos + 3)
    if not over:
        return s.auto([("M", 3, pos)] + tail, True).ok(cid, lean0=after == "stored")
    enc.put_auto(s.w, [("M", 3, pos + 1)] + tail, True)
    return s.bad(cid, "E_IO", "invalid distance too far back", pos + 3 + sum(1 if t[0] == "L" else t[1] for t in tail),
                 lean0=after == "stored")


for _after in ("dyn", "stored"):
    for _pos in (1, 1000):
        for _over in (False, True):
            _cid = "M2b-%s-%d-%s" % (_after, _pos, "over" if _over else "ok")
            case(_cid, not _over)(functools.partial(m2b, _cid, _after, _pos, _over))


@case("M3")
def _m3():
    rng = np.random.default_rng(204)
    toks = lits(rand_letters(rng, 500)) + [("M", 258, 333), ("L", 40), ("M", 258, 77, 284), ("L", 41), ("M", 258, 500)]
    return Stream().auto(toks, True).ok("M3")


def every_length_code(rng, pos):
    """Each length code 257-285 with its lowest and its highest extra value."""
    toks = []
    for i in range(29):
        for length in sorted({enc.LEN_BASE[i], min(258, enc.LEN_BASE[i] + (1 << enc.LEN_EXTRA[i]) - 1)}):
            toks += [("M", length, int(rng.integers(1, pos + 1)), 257 + i), ("L", 32 + int(rng.integers(64)))]
            pos += length + 1
    return toks


@case("M3b")
def _m3b():
    rng = np.random.default_rng(205)
    return Stream().auto(lits(rand_letters(rng, 300)) + every_length_code(rng, 300), True).ok("M3b")


def every_dist_code(rng, pos, limit=60000):
    """Each distance code 0-29 with its lowest and its highest extra value; the
    output is brought up to each distance by long matches at random distances,
    a literal after each, so that it never turns periodic."""
    toks = []
    for j in range(30):
        for d in sorted({enc.DIST_BASE[j], enc.DIST_BASE[j] + (1 << enc.DIST_EXTRA[j]) - 1}):
            while pos < d:
                toks += [("M", 258, int(rng.integers(1, pos + 1))), ("L", 32 + int(rng.integers(64)))]
                pos += 259
            length = int(rng.integers(3, 40))
            toks += [("M", length, d), ("L", 32 + int(rng.integers(64)))]
            pos += length + 1
    assert pos <= limit
    return toks


@case("M3c")
def _m3c():
    rng = np.random.default_rng(206)
    return Stream().auto(lits(rand_letters(rng, 300)) + every_dist_code(rng, 300), True).ok("M3c")


def periodic(p, isize, length=258):
    """p literals, then matches of distance p (and the given length) up to isize bytes."""
    toks = lits(rand_letters(np.random.default_rng(207 + p), p))
    left = isize - p
    while left:
        n = min(length, left)
        if 0 < left - n < 3:  # no match shorter than 3: leave 3 for the last one
            n = left - 3
        toks.append(("M", n, p))
        left -= n
    return toks


for _p, _n in [(p, 65280) for p in (1, 2, 3, 7, 255, 256, 257, 258, 259)] + [(1, 65536), (3, 65536)]:
    @case("M4-p%d-%d" % (_p, _n))
    def _m4(p=_p, n=_n):
        return Stream().auto(periodic(p, n), True).ok("M4-p%d-%d" % (p, n))


@case("M4b")
def _m4b():
    toks = periodic(3, 65280, 3)
    assert len(toks) == 3 + 21759
    return Stream().auto(toks, True).ok("M4b")


for _over in (1, 257):
    @case("M6-%d" % _over)
    def _m6(over=_over):
        """The last token is a match that runs `over` bytes past ISIZE."""
        toks = rand_tokens(np.random.default_rng(208), 3000, 0)
        s = Stream().auto(toks + [("M", 258, 1234)], True)
        return s.ok("M6-%d" % over, isize=s.pos - over)


# ---------------------------------------------------------------- code tables
T1_SYMS = [97, 257] + list(range(98, 110)) + [110, 256]  # lengths 1, 2, ..., 14, 15, 15
T1_LENS = list(range(1, 16)) + [15]
T1_LL = lengths_at(258, list(zip(T1_SYMS, T1_LENS)))
T1_DL = T1_LENS  # on distance codes 0-15


def draw_by_length(rng, syms, lens, n):
    """n symbols, each drawn with probability 2^-length, every symbol at least twice."""
    p = np.array([2.0 ** -l for l in lens])
    got = [syms[i] for i in rng.choice(len(syms), n, p=p / p.sum())]
    for i, s in enumerate(syms * 2):
        got[(i * 7919) % n] = s
    return got


@case("T1")
def _t1():
    rng = np.random.default_rng(301)
    lsyms = draw_by_length(rng, T1_SYMS[:-1], T1_LENS[:-1], 20000)
    dsyms = iter(draw_by_length(rng, list(range(16)), T1_DL, sum(1 for s in lsyms if s == 257)))
    toks = lits(b"a" * 256)  # room for every distance of codes 0-15 (at most 255)
    for s in lsyms:
        if s == 257:
            j = next(dsyms)
            toks.append(("M", 3, enc.DIST_BASE[j] + int(rng.integers(1 << enc.DIST_EXTRA[j]))))
        else:
            toks.append(("L", s))
    return Stream().dyn(toks, T1_LL, T1_DL, True).ok("T1")


# T2: complete codes whose long codes fill the sub-tables.  Codes per length 1..15, found by
# a seeded search (random splits of a Kraft-complete tree, then single split+merge moves that
# do not lose sub-table entries); sub_entries() of them: 306 litlen (root 10), 80 distance (root 9).
T2_LIT_COUNTS = [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 3, 17, 17, 17, 226]
T2_DIST_COUNTS = [1, 1, 0, 3, 1, 1, 0, 0, 0, 13, 5, 1, 1, 1, 2]
# the shortest codes go to the symbols the data uses to cover ground
T2_LIT_ORDER = [285, 65, 256, 66, 67, 68] + [s for s in range(286) if s not in (285, 65, 256, 66, 67, 68)]
T2_DIST_ORDER = [0, 29, 28, 27, 26, 25] + list(range(1, 25))


def lengths_from_counts(counts, order):
    lens, out = [l for l, c in enumerate(counts, 1) for _ in range(c)], [0] * len(order)
    for s, l in zip(order, lens):
        out[s] = l
    return out


T2_LL = lengths_from_counts(T2_LIT_COUNTS, T2_LIT_ORDER)
T2_DL = lengths_from_counts(T2_DIST_COUNTS, T2_DIST_ORDER)


def sub_entries(lengths, root):
    """Sub-table entries of the decoder's table image, by the rule DESIGN.md
    states: per root prefix with longer codes, 2^(longest code under it - root)."""
    longest = {}
    for c, n in zip(enc.canonical_codes(lengths), lengths):
        if n > root:
            longest[c >> (n - root)] = max(longest.get(c >> (n - root), 0), n)
    return sum(1 << (n - root) for n in longest.values())


@case("T2")
def _t2():
    rng = np.random.default_rng(302)
    toks = lits(bytes(range(256)))
    toks += every_length_code(rng, 256)
    toks += every_dist_code(rng, sum(1 if t[0] == "L" else t[1] for t in toks))
    toks += lits(bytes(rng.integers(0, 256, 200, dtype=np.uint8)))
    return Stream().dyn(toks, T2_LL, T2_DL, True).ok("T2")


T3_LL = lengths_at(286, [(97 + i, i + 1) for i in range(13)] + [(256, 14), (284, 15), (285, 15)])
T3_DL = lengths_at(30, [(i, i + 1) for i in range(14)] + [(28, 15), (29, 15)])


@case("T3")
def _t3():
    rng = np.random.default_rng(303)
    toks = lits(bytes(draw_by_length(rng, list(range(97, 110)), list(range(1, 14)), 33000)))
    toks += [("M", 258, 24577), ("L", 98), ("M", 227, 32768), ("M", 257, 16385, 284), ("L", 99), ("M", 258, 20000, 284)]
    for j in range(14):
        toks += [("M", 258, enc.DIST_BASE[j]), ("L", 97 + j % 13)]
    return Stream().dyn(toks, T3_LL, T3_DL, True, hlit=286, hdist=30).ok("T3")


@case("T3-257-1")
def _t3b():
    toks = lits(rand_letters(np.random.default_rng(304), 4000))
    lf, _ = enc.token_freqs(toks)
    return Stream().dyn(toks, enc.limited_lengths(lf, 15), [1], True, hlit=257, hdist=1).ok("T3-257-1")


# ---------------------------------------------------------------- header cases
# Each is written as the first DEFLATE block of its BGZF block (k_huff_tables
# parses it) and as the third (the fallback parses it inline).
TOO_MANY = "too many length or distance symbols"
HDR_LITS = lits(rand_letters(np.random.default_rng(400), 700, 26, 97))
HDR_LL = enc.limited_lengths(enc.token_freqs(HDR_LITS)[0], 15)
A500 = lits(b"A" * 500)


def h_h1(s):
    s.dyn(A500, H1_LL, [0], True)


def h_h1b(s):
    s.dyn(A500, H1_LL, [1], True)


def h_h1c(s):
    """One litlen code would not do for matches: 'A', EOB and length code 285 with the one distance code."""
    s.dyn(A500 + [("M", 258, 1)] * 3 + A500[:7], lengths_at(286, [(65, 1), (256, 2), (285, 2)]), [1], True)


def h_h5(s):
    s.dyn(HDR_LITS, HDR_LL, [0] * 30, True, hdist=30)


def h_h6_5(s):
    """HCLEN = 5: code-length codes for 16, 17, 18, 0 and 8 only; 256 litlen codes of 8 bits."""
    ll = [8] * 255 + [0, 8]
    s.dyn(lits(bytes(np.random.default_rng(401).integers(0, 255, 900, dtype=np.uint8))), ll, [0], True,
          clen_mode=dict(hclen=5, cl_lengths=lengths_at(19, [(8, 1), (0, 2), (16, 3), (17, 3)])))


def h_h6_19(s):
    s.dyn(HDR_LITS, HDR_LL, [1], True, clen_mode=dict(hclen=19))


def h_h6_norle(s):
    s.dyn(HDR_LITS, HDR_LL, [1], True, clen_mode=dict(rle=False))


H6C_LL = lengths_at(258, [(65, 1), (66, 2), (256, 3), (257, 3)])
H6C_DL = [0] * 5 + [1]


def h_h6c(s):
    """Litlen lengths 258-269 and distance lengths 0-4 are zero: one 18-run of 17 covers both."""
    syms = enc.rle_lengths(H6C_LL + [0] * 12 + H6C_DL)
    assert (18, 17 - 11) in syms
    toks = lits(b"ABAABABBAAAB") + [("M", 3, 7), ("L", 66), ("M", 3, 8)] * 40 + lits(b"BA")
    s.dyn(toks, H6C_LL, H6C_DL, True, hlit=270, hdist=6)


VALID_HEADERS = [("H1", h_h1), ("H1b", h_h1b), ("H1c", h_h1c), ("H5", h_h5), ("H6-5", h_h6_5), ("H6-19", h_h6_19),
                 ("H6-norle", h_h6_norle), ("H6c", h_h6c)]


def raw_dyn(s, ll, dl=(1,), toks=(), **kw):
    enc.put_dynamic(s.w, list(toks), ll, list(dl), True, **kw)


ZEROS_ONLY = dict(hclen=4, cl_lengths=lengths_at(19, [(0, 1), (18, 1)]))
INVALID_HEADERS = [
    ("H2", "missing end-of-block", lambda s: raw_dyn(s, lengths_at(257, [(65, 1), (66, 1)]), toks=A500)),
    ("H3", "invalid literal/lengths set", lambda s: raw_dyn(s, lengths_at(257, [(65, 1), (256, 2)]), toks=A500)),
    ("H3b", "invalid literal/lengths set",
     lambda s: raw_dyn(s, lengths_at(257, [(65, 1), (66, 1), (256, 1)]), toks=A500)),
    ("H3c", "invalid distances set", lambda s: raw_dyn(s, H1_LL, [2, 2], toks=A500)),
    ("H4", TOO_MANY, lambda s: raw_dyn(s, HDR_LL, toks=HDR_LITS, hlit=288)),
    ("H4b", TOO_MANY, lambda s: raw_dyn(s, HDR_LL, toks=HDR_LITS, hdist=31)),
    ("H4c", TOO_MANY, lambda s: raw_dyn(s, HDR_LL, toks=HDR_LITS, hdist=32)),
    ("H5b", "invalid distance code",
     lambda s: raw_dyn(s, lengths_at(258, [(65, 1), (256, 2), (257, 2)]), [0] * 30,
                       toks=A500 + [("R", 257, (0, 0), None, None)] + A500, hdist=30)),
    # HCLEN = 4 leaves only 16, 17, 18 and 0: every length is zero
    ("H6", "missing end-of-block", lambda s: raw_dyn(s, [0] * 257, [0], clen_mode=ZEROS_ONLY)),
    ("H6b", "invalid bit length repeat",
     lambda s: raw_dyn(s, H1_LL, [0], toks=A500,
                       clen_mode=dict(syms=[(16, 0)] + enc.rle_lengths(H1_LL + [0])[1:],
                                      cl_lengths=lengths_at(19, [(0, 2), (1, 2), (16, 2), (17, 3), (18, 3)])))),
    ("H6d", "invalid bit length repeat",
     lambda s: raw_dyn(s, H1_LL, [0], toks=A500, clen_mode=dict(syms=enc.rle_lengths(H1_LL + [0])[:-1] + [(18, 127)]))),
    ("H6e", "invalid code lengths set",
     lambda s: raw_dyn(s, [8] * 255 + [0, 8], [0], toks=A500,
                       clen_mode=dict(cl_lengths=lengths_at(19, [(0, 1), (8, 1), (16, 1)])))),
    ("H6f", "invalid code lengths set",
     lambda s: raw_dyn(s, [8] * 255 + [0, 8], [0], toks=A500,
                       clen_mode=dict(cl_lengths=lengths_at(19, [(0, 2), (8, 1), (16, 3)])))),
    ("H7", "invalid literal/length code",
     lambda s: enc.put_fixed(s.w, HDR_LITS + [("R", 286, (0, 0), None, None)] + HDR_LITS, True)),
    ("H7b", "invalid literal/length code",
     lambda s: enc.put_fixed(s.w, HDR_LITS + [("R", 287, (0, 0), None, None)] + HDR_LITS, True)),
    # a length on distance code 30 can only be announced with HDIST = 31
    ("H7c", TOO_MANY, lambda s: raw_dyn(s, HDR_LL, [1] + [0] * 29 + [1], toks=HDR_LITS, hdist=31)),
]


@functools.lru_cache(maxsize=None)
def _header_prefix():
    rng = np.random.default_rng(402)
    s = Stream().auto(rand_tokens(rng, 1500, 0))
    return s.auto(rand_tokens(rng, 1500, s.pos))


SYMBOL_ERRORS = ("H5b",)  # a good dynamic header: the error comes with a symbol, after a lean round may have begun


def header_prefix():
    """Two good dynamic blocks, so that the case's block is the third."""
    p, s = _header_prefix(), Stream()
    s.w.vals, s.w.lens, s.w.nbits, s.toks = list(p.w.vals), list(p.w.lens), p.w.nbits, list(p.toks)
    return s


def _valid_header(cid, fn, third):
    s = header_prefix() if third else Stream()
    fn(s)
    return s.ok(cid)


def _invalid_header(cid, msg, fn, third):
    s = header_prefix() if third else Stream()
    fn(s)
    return s.bad(cid, "E_IO", msg, s.pos + 1000, lean0=not third and cid[:-2] not in SYMBOL_ERRORS)


for _third in (False, True):
    for _cid, _fn in VALID_HEADERS:
        _cid += "@3" if _third else "@1"
        case(_cid)(functools.partial(_valid_header, _cid, _fn, _third))
    for _cid, _msg, _fn in INVALID_HEADERS:
        _cid += "@3" if _third else "@1"
        case(_cid, False)(functools.partial(_invalid_header, _cid, _msg, _fn, _third))
