"""A plain DEFLATE (RFC 1951) token reader for tests.

parse() walks a raw DEFLATE stream and returns, per DEFLATE block, what an
encoder chose: the block type, the token list in deflate_enc's notation
(('L', byte) or ('M', length, distance)) and, for a dynamic block, how often
each of the 19 code-length symbols occurs in its header.  It holds no project
code and is run on zlib's output only, to prove that a test input drove zlib
down the path the input is named for.
"""
import collections
import heapq

import deflate_enc as enc

STORED, FIXED, DYNAMIC = 0, 1, 2

Block = collections.namedtuple("Block", "btype final tokens cl_counts stored")
# btype      STORED / FIXED / DYNAMIC
# final      the BFINAL bit
# tokens     [('L', byte) | ('M', length, distance)] (empty for a stored block)
# cl_counts  dynamic blocks: 19 counts, by code-length symbol, of the symbols that spell
#            the literal/length and distance code lengths in the header; else None
# stored     the bytes of a stored block, else None


def _table(lengths):
    """(lookup table indexed by the next `bits` stream bits LSB first -> length << 9 | symbol, bits)."""
    bits = max(lengths) if any(lengths) else 1
    size = 1 << bits
    tab = [0] * size
    for sym, (code, n) in enumerate(zip(enc.canonical_codes(lengths), lengths)):
        if n:
            r = int(format(code, "0%db" % n)[::-1], 2)
            tab[r::1 << n] = [n << 9 | sym] * (size >> n)
    return tab, bits


_FIXED = (_table(enc.FIXED_LITLEN), _table(enc.FIXED_DIST))


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.buf, self.cnt = data, 0, 0, 0

    def need(self, n):
        while self.cnt < n:
            chunk = self.data[self.pos:self.pos + 8]
            if not chunk:
                raise ValueError("DEFLATE stream ends inside a block")
            self.buf |= int.from_bytes(chunk, "little") << self.cnt
            self.cnt += 8 * len(chunk)
            self.pos += len(chunk)

    def take(self, n):
        self.need(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def sym(self, tab, bits):
        """One Huffman symbol; near the stream end the peek is padded with zero bits."""
        if self.cnt < bits and self.pos < len(self.data):
            self.need(min(bits, self.cnt + 8 * (len(self.data) - self.pos)))
        e = tab[self.buf & ((1 << bits) - 1)]
        n = e >> 9
        if n == 0 or n > self.cnt:
            raise ValueError("no such code" if n == 0 else "DEFLATE stream ends inside a code")
        self.buf >>= n
        self.cnt -= n
        return e & 511

    def raw(self, n):
        """n bytes from a byte boundary."""
        assert self.cnt % 8 == 0
        start = self.pos - self.cnt // 8
        if start + n > len(self.data):
            raise ValueError("DEFLATE stream ends inside a stored block")
        self.pos, self.buf, self.cnt = start + n, 0, 0
        return self.data[start:start + n]

    def consumed(self):
        return 8 * self.pos - self.cnt


def _header(r):
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    cl = [0] * 19
    for s in enc.CL_ORDER[:hclen]:
        cl[s] = r.take(3)
    tab, bits = _table(cl)
    counts, lens = [0] * 19, []
    while len(lens) < hlit + hdist:
        s = r.sym(tab, bits)
        counts[s] += 1
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise ValueError("repeat without a previous length")
            lens += [lens[-1]] * (3 + r.take(2))
        else:
            lens += [0] * ((3 + r.take(3)) if s == 17 else (11 + r.take(7)))
    if len(lens) != hlit + hdist:
        raise ValueError("code lengths overshoot")
    return _table(lens[:hlit]), _table(lens[hlit:]), counts


def _tokens(r, lit, dist):
    (ltab, lbits), (dtab, dbits) = lit, dist
    out = []
    while True:
        s = r.sym(ltab, lbits)
        if s < 256:
            out.append(("L", s))
        elif s == 256:
            return out
        else:
            i = s - 257
            if i >= 29:
                raise ValueError("length symbol %d" % s)
            length = enc.LEN_BASE[i] + r.take(enc.LEN_EXTRA[i])
            j = r.sym(dtab, dbits)
            if j >= 30:
                raise ValueError("distance symbol %d" % j)
            out.append(("M", length, enc.DIST_BASE[j] + r.take(enc.DIST_EXTRA[j])))


def parse(raw):
    """The blocks of one raw DEFLATE stream, which must end with its final block
    (less than a byte of padding after it)."""
    r = _Bits(bytes(raw))
    blocks = []
    while True:
        final, btype = r.take(1), r.take(2)
        if btype == STORED:
            r.take(r.cnt % 8)
            n, nn = r.take(16), r.take(16)
            if n ^ nn != 0xffff:
                raise ValueError("stored length check")
            body = r.raw(n)
            blocks.append(Block(STORED, final, [], None, body))
        elif btype == FIXED:
            blocks.append(Block(FIXED, final, _tokens(r, *_FIXED), None, None))
        elif btype == DYNAMIC:
            lit, dist, counts = _header(r)
            blocks.append(Block(DYNAMIC, final, _tokens(r, lit, dist), counts, None))
        else:
            raise ValueError("block type 3")
        if final:
            break
    if (r.consumed() + 7) // 8 != len(raw):
        raise ValueError("bytes after the final block")
    return blocks


def expand(blocks):
    """The bytes the blocks stand for."""
    out = bytearray()
    for b in blocks:
        if b.btype == STORED:
            out += b.stored
        else:
            out += enc.expand(b.tokens, bytes(out[-32768:]))
    return bytes(out)


def huffman_depth(counts):
    """Depth of an unrestricted Huffman tree over the symbols with count > 0,
    ties broken towards the shallower subtree (as zlib's build_tree does, which
    keeps the tree as flat as the counts allow)."""
    heap = [(c, 0, i) for i, c in enumerate(counts) if c > 0]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    tick = len(counts)
    while len(heap) > 1:
        fa, da, _ = heapq.heappop(heap)
        fb, db, _ = heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1, tick))
        tick += 1
    return heap[0][1]
