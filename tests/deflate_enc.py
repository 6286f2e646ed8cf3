"""A plain DEFLATE (RFC 1951) encoder for tests.

zlib's deflate() writes only a narrow slice of legal DEFLATE; this writer puts
down whatever the caller asks for: any block kind in any order, any code-length
set (legal or not), any match the format can express, and a code-length section
chosen symbol by symbol.  It holds no project code: the decoders under test and
zlib's inflate are the only judges of what it writes.

Tokens:
  ('L', byte)                       a literal
  ('M', length, distance)           a match, by the usual length / distance codes
  ('M', length, distance, lcode)    the same with the length code forced (258 = code 284 + extra 31)
  ('R', lsym, (lextra, lbits), dsym, (dextra, dbits))
                                    raw symbols: any litlen symbol, then (dsym not None) any distance
                                    symbol, each with the extra bits given; expand() refuses it
"""
import bisect
import heapq

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def length_code(length):
    """(index into LEN_BASE, extra value) of a match length, by the shortest code (258 = code 285)."""
    assert 3 <= length <= 258
    i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return i, length - LEN_BASE[i]


def dist_code(distance):
    assert 1 <= distance <= 32768
    i = bisect.bisect_right(DIST_BASE, distance) - 1
    return i, distance - DIST_BASE[i]


_LEN_CODE = [None] * 3 + [length_code(n) for n in range(3, 259)]


class BitWriter:
    """Little-endian bit writer: bits() puts a value LSB first (header fields,
    extra bits), code() a Huffman code MSB first."""

    def __init__(self):
        self.vals, self.lens, self.nbits = [], [], 0

    def bits(self, v, n):
        assert 0 <= n <= 32 and 0 <= v < (1 << n)
        self.vals.append(v)
        self.lens.append(n)
        self.nbits += n

    def code(self, c, n):
        self.bits(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self, fill=0):
        """Pad to a byte boundary with zero (or one) bits; returns the number of pad bits."""
        n = -self.nbits % 8
        self.bits(((1 << n) - 1) if fill else 0, n)
        return n

    def raw(self, payload):
        assert self.nbits % 8 == 0
        self.vals.extend(payload)
        self.lens.extend([8] * len(payload))
        self.nbits += 8 * len(payload)

    def getvalue(self, fill=0):
        """The bytes written, the last one padded with zero (or one) bits."""
        vals = np.asarray(self.vals, dtype=np.uint64)
        lens = np.asarray(self.lens, dtype=np.int64)
        pos = np.cumsum(lens) - lens
        bits = np.full((self.nbits + 7) // 8 * 8, 1 if fill else 0, dtype=np.uint8)
        bits[:self.nbits] = 0
        for k in range(int(lens.max()) if len(lens) else 0):
            m = lens > k
            bits[pos[m] + k] = (vals[m] >> np.uint64(k)) & np.uint64(1)
        return np.packbits(bits, bitorder="little").tobytes()


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol (0 where its length is 0).  Over-subscribed
    sets still get codes (they wrap), so an illegal set can be written down."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        out.append(nxt[n] & ((1 << n) - 1) if n else 0)
        nxt[n] += 1 if n else 0
    return out


def kraft(lengths, maxbits=15):
    """Sum of 2^(maxbits - l) over the used codes: 2^maxbits for a complete set."""
    return sum(1 << (maxbits - n) for n in lengths if n)


def limited_lengths(freqs, maxbits):
    """Code lengths (<= maxbits) for the symbols with freq > 0: a heap Huffman,
    then a Kraft fix-up.  Complete whenever two or more symbols are used; one
    used symbol gets length 1."""
    used = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if len(used) <= 1:
        for s in used:
            lens[s] = 1
        return lens
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ta, a = heapq.heappop(heap)
        fb, tb, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, min(ta, tb), a + b))
    for s in used:
        lens[s] = min(lens[s], maxbits)
    full = 1 << maxbits
    k = kraft(lens, maxbits)
    while k > full:  # over-subscribed after the clamp: lengthen the longest code that still can be
        s = max((s for s in used if lens[s] < maxbits), key=lambda s: (lens[s], -freqs[s]))
        k -= 1 << (maxbits - lens[s] - 1)
        lens[s] += 1
    while k < full:  # room left: shorten the longest code that fits
        s = max((s for s in used if k + (1 << (maxbits - lens[s])) <= full), key=lambda s: (lens[s], freqs[s]))
        k += 1 << (maxbits - lens[s])
        lens[s] -= 1
    return lens


def expand(tokens, history=b""):
    """The bytes the tokens stand for, after `history` (which matches may reach into)."""
    out = bytearray(history)
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        elif t[0] == "M":
            length, d = t[1], t[2]
            assert 1 <= d <= len(out), "match before the start of the output"
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                seg = bytes(out[-d:])
                out += (seg * (length // d + 1))[:length]
        else:
            raise ValueError("raw tokens have no expansion")
    return bytes(out[len(history):])


def _reversed_codes(lengths, n):
    """(code bit-reversed for the LSB-first writer, length) per symbol, padded with unused symbols to n."""
    out = [(int(format(c, "0%db" % l)[::-1], 2) if l else 0, l) for c, l in zip(canonical_codes(lengths), lengths)]
    return out + [(0, 0)] * (n - len(out))


def put_tokens(w, tokens, litlen_lengths, dist_lengths):
    """The tokens and the end-of-block code under the given code lengths."""
    lit, dist = _reversed_codes(litlen_lengths, 288), _reversed_codes(dist_lengths, 32)
    vals, lens = [], []

    def put(v, n):
        vals.append(v)
        lens.append(n)

    for t in tokens:
        if t[0] == "L":
            c, n = lit[t[1]]
            assert n, "literal without a code"
            vals.append(c)
            lens.append(n)
            continue
        if t[0] == "M":
            i, ex = _LEN_CODE[t[1]] if len(t) < 4 else (t[3] - 257, t[1] - LEN_BASE[t[3] - 257])
            j, dx = dist_code(t[2])
            lsym, lex, dsym, dex = 257 + i, (ex, LEN_EXTRA[i]), j, (dx, DIST_EXTRA[j])
            assert 0 <= ex < (1 << LEN_EXTRA[i]) or ex == 0
        else:
            _, lsym, lex, dsym, dex = t
        assert lit[lsym][1], "litlen symbol without a code"
        put(*lit[lsym])
        put(*lex)
        if dsym is not None:
            assert dist[dsym][1], "distance symbol without a code"
            put(*dist[dsym])
            put(*dex)
    if lit[256][1]:
        put(*lit[256])
    w.vals += vals
    w.lens += lens
    w.nbits += sum(lens)


def put_fixed(w, tokens, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LITLEN, FIXED_DIST)


def put_stored(w, payload, final, nlen=None):
    """A stored block; the padding up to the byte boundary is zero bits."""
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(payload), 16)
    w.bits((len(payload) ^ 0xffff) if nlen is None else nlen, 16)
    w.raw(payload)


def rle_lengths(lengths, rle=True):
    """The code-length symbols [(symbol, extra value)] for a run of code lengths."""
    out, i = [], 0
    while i < len(lengths):
        v, n = lengths[i], 1
        while i + n < len(lengths) and lengths[i + n] == v:
            n += 1
        i += n
        if not rle:
            out += [(v, 0)] * n
            continue
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11))
                n -= k
            if n >= 3:
                out.append((17, n - 3))
                n = 0
        else:
            out.append((v, 0))
            n -= 1
            while n >= 3:
                k = min(n, 6)
                out.append((16, k - 3))
                n -= k
        out += [(v, 0)] * n
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def put_dynamic(w, tokens, litlen_lengths, dist_lengths, final, hlit=None, hdist=None, clen_mode=None):
    """A dynamic-Huffman block.  The caller gives the code lengths (legal or
    not).  hlit / hdist override the symbol counts the header announces (257..288
    and 1..32; the lengths are padded with zeros or cut to that many).
    clen_mode chooses the code-length section:
      rle         use the repeat codes 16 / 17 / 18 (default True)
      hclen       how many code-length-code lengths to send, 4..19 (default: as few as possible)
      syms        the code-length symbols [(symbol, extra value)] themselves, instead of
                  an encoding of the lengths (runs may cross from litlen into distance
                  lengths, start with 16, or overshoot)
      cl_lengths  the 19 code-length-code lengths by symbol, instead of a Huffman code
                  for the symbols used (may be over-subscribed or incomplete)"""
    mode = dict(rle=True, hclen=None, syms=None, cl_lengths=None)
    mode.update(clen_mode or {})
    ll, dl = list(litlen_lengths), list(dist_lengths)
    if hlit is None:
        hlit = max(257, max((i + 1 for i, n in enumerate(ll) if n), default=0))
    if hdist is None:
        hdist = max(1, max((i + 1 for i, n in enumerate(dl) if n), default=0))
    assert 257 <= hlit <= 288 and 1 <= hdist <= 32
    sent = (ll + [0] * 288)[:hlit] + (dl + [0] * 32)[:hdist]
    syms = mode["syms"] if mode["syms"] is not None else rle_lengths(sent, mode["rle"])
    cl = mode["cl_lengths"]
    if cl is None:
        freqs = [0] * 19
        for s, _ in syms:
            freqs[s] += 1
        if sum(1 for f in freqs if f) == 1:  # zlib wants the code-length code complete: a second 1-bit code
            freqs[0 if freqs[0] == 0 else 18] = 1
        cl = limited_lengths(freqs, 7)
    hclen = mode["hclen"]
    if hclen is None:
        hclen = max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl[s]), default=0))
    assert 4 <= hclen <= 19
    assert all(cl[s] == 0 for s in CL_ORDER[hclen:]), "a code-length code beyond HCLEN"
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl[s], 3)
    cc = canonical_codes(cl)
    for s, extra in syms:
        assert cl[s], "code-length symbol without a code"
        w.code(cc[s], cl[s])
        if s >= 16:
            w.bits(extra, CL_EXTRA[s])
    put_tokens(w, tokens, ll, dl)


def token_freqs(tokens):
    """(litlen, distance) symbol frequencies of the tokens plus one end-of-block."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if t[0] == "L":
            lf[t[1]] += 1
        else:
            lf[257 + (_LEN_CODE[t[1]][0] if len(t) < 4 else t[3] - 257)] += 1
            df[dist_code(t[2])[0]] += 1
    return lf, df


def put_auto(w, tokens, final, **kw):
    """A dynamic block under Huffman codes made for the tokens."""
    lf, df = token_freqs(tokens)
    dl = limited_lengths(df, 15)
    put_dynamic(w, tokens, limited_lengths(lf, 15), dl if any(dl) else [0], final, **kw)
