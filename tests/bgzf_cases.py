"""Inputs for the BGZF write path (hbam_deflate.h under k_deflate_blocks, k_dfl_crc,
k_dfl_frame) aimed at what a run of ordinary files reaches only by accident:
several lanes of one wave at work, zlib's rare encoder paths, and every CRC
regime at every payload alignment.

A case is (name, payload, block_lens, levels): the payload is cut into
block_lens and compressed at each of levels.  Everything is deterministic (the
numpy default_rng seeds below); nothing here imports the package or needs a
GPU.  test_bgzf_cases.py proves from zlib's output that each family reaches the
path it is named for; test_gpu_bgzf_cases.py compares the GPU with zlib.

Families (one payload is at most 65,536 bytes):
  W  shared waves: 5,121 and 10,241 blocks (2 and 3 lanes per wave), small
     blocks next to 64 KiB ones of four kinds, every 7th empty
  F  every length 0..300 over an 8-letter alphabet (fixed-Huffman selection)
  E  no repeated trigram, so a symbol per byte: lengths around the 16,383-symbol
     buffer, and a 16,382-byte prefix closed by one match
  B  noise with a 3-byte copy every 4 bytes: the bit-length tree overflows 7 bits
  D  one copy at the TOO_FAR (4096 / 4097) and MAX_DIST (32506 / 32507) edges;
     D7 is D over 7-bit noise, which zlib codes (D's noise it stores, so only
     D's 258-byte copies show in its tokens)
  R  runs that end with the payload
  C  CRC lengths 4..16, 60..70, 127..129, 4095..4097, 65535, 65536, each at
     every start alignment modulo 8
  L  the four payload kinds of test_bgzf_write.py at levels 7 and 8
"""
import collections
import functools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Case = collections.namedtuple("Case", "name payload block_lens levels")


def split_bgzf_blocks(data):
    """[(raw DEFLATE stream, CRC32 field, ISIZE field)] of a BGZF file's blocks."""
    p, out = 0, []
    while p < len(data):
        assert data[p:p + 4] == b"\x1f\x8b\x08\x04" and data[p + 12:p + 16] == b"BC\x02\x00"
        bs = int.from_bytes(data[p + 16:p + 18], "little") + 1
        out.append((data[p + 18:p + bs - 8], int.from_bytes(data[p + bs - 8:p + bs - 4], "little"),
                    int.from_bytes(data[p + bs - 4:p + bs], "little")))
        p += bs
    assert p == len(data)
    return out


@functools.lru_cache(maxsize=None)
def bam_payload():
    """The inflated payload of tests/golden/test.bam."""
    data = open(os.path.join(GOLDEN, "test.bam"), "rb").read()
    return b"".join(zlib.decompressobj(-15).decompress(raw) for raw, _, _ in split_bgzf_blocks(data))


def _noise(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _letters(rng, alphabet, n):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)]


def _runs(n, step=3000):
    return (np.arange(n) // step).astype(np.uint8)


# ------------------------------------------------------------------ W ----

W_LARGE = ("noise", "acgt", "two", "runs")  # every 64th block, in turn
W_LARGE_LEN = {"noise": 65498, "acgt": 65280, "two": 65275, "runs": 40000}


def _shared_waves(n_blocks, seed, small_max=200):
    rng = np.random.default_rng(seed)
    bam = np.frombuffer(bam_payload(), np.uint8)
    text = _letters(rng, b"ACGT", 1 << 20)
    parts, lens, large = [], [], 0
    for i in range(n_blocks):
        if i % 64 == 63:
            kind = W_LARGE[large % 4]
            large += 1
            n = W_LARGE_LEN[kind]
            part = {"noise": lambda: _noise(rng, n), "acgt": lambda: _letters(rng, b"ACGT", n),
                    "two": lambda: _letters(rng, b"AC", n), "runs": lambda: _runs(n)}[kind]()
        elif i % 7 == 0:
            part = bam[:0]
        else:
            n = int(rng.integers(1, small_max + 1))
            src = bam if i % 2 else text
            at = int(rng.integers(0, len(src) - n))
            part = src[at:at + n]
        parts.append(part)
        lens.append(len(part))
    return np.concatenate(parts).tobytes(), lens


def _w1():
    return [Case("W1", *_shared_waves(5121, 0x5701), levels=(1, 5, 0))]


def _w1_second():
    """5,121 + 300 blocks: with 5,121 arenas the last 300 go through a second batch."""
    return [Case("W1b", *_shared_waves(5121 + 300, 0x5702), levels=(5,))]


def _w2():
    return [Case("W2", *_shared_waves(10241, 0x5703), levels=(5,))]


# ------------------------------------------------------------------ F ----

F_ALPHABET = b"ACGTNacg"


def _f():
    """Every third length is plain draws from the alphabet, which zlib codes
    with a fixed block only up to about 35 bytes (three bits a letter soon pay
    for a dynamic header).  The others tile a drawn motif of 2..40 letters and
    then change about one letter in 50, so a few literals and matches make up
    the block and the fixed code stays the cheaper one at every length."""
    rng = np.random.default_rng(0xF1)
    parts = []
    for n in range(301):
        if n % 3 == 0:
            part = _letters(rng, F_ALPHABET, n)
        else:
            motif = _letters(rng, F_ALPHABET, int(rng.integers(2, 41)))
            part = np.tile(motif, n // len(motif) + 1)[:n].copy()
            hit = rng.random(n) < 0.02
            part[hit] = _letters(rng, F_ALPHABET, int(hit.sum()))
        parts.append(part)
    return [Case("F", np.concatenate(parts).tobytes(), list(range(301)), tuple(range(1, 10)))]


# ------------------------------------------------------------------ E ----

E_PLAIN = (16382, 16383, 16384, 16385, 32766)
E_PREFIX = 16382
E_COPY = (3, 5, 258)  # the prefix, then a copy of this many earlier bytes
E_COPY_FROM = 15000   # near enough (1,382 back) for a 3-byte match at every level


@functools.lru_cache(maxsize=None)
def no_repeated_trigram(n=max(E_PLAIN), seed=0xE1):
    """n bytes over a 64-letter alphabet in which no three consecutive bytes
    occur twice: a draw that would repeat a trigram is rejected.  zlib finds no
    match in it, so it tallies one symbol per byte."""
    rng = np.random.default_rng(seed)
    draws = rng.integers(0x30, 0x70, 4 * n).tolist()
    out, seen = bytearray(draws[:2]), set()
    for d in draws[2:]:
        t = (out[-2], out[-1], d)
        if t not in seen:
            seen.add(t)
            out.append(d)
            if len(out) == n:
                break
    assert len(out) == n
    tri = {bytes(out[i:i + 3]) for i in range(n - 2)}
    assert len(tri) == n - 2, "a trigram repeats"
    return bytes(out)


def _e():
    t = no_repeated_trigram()
    parts = [t[:n] for n in E_PLAIN]
    parts += [t[:E_PREFIX] + t[E_COPY_FROM:E_COPY_FROM + k] for k in E_COPY]
    return [Case("E", b"".join(parts), [len(p) for p in parts], (1, 5))]


def e_block(what):
    """Index in E's block list of a plain length or of ('copy', k)."""
    return E_PLAIN.index(what) if isinstance(what, int) else len(E_PLAIN) + E_COPY.index(what[1])


# ------------------------------------------------------------------ B ----

# seeds (of 1..8 tried) kept because zlib's output shows the overflow at each of
# levels 1, 2, 3 and 5 (test_bgzf_cases.py checks it); seed 2 is also cut in halves
B_SEEDS = (2, 5)
B_LEVELS = (1, 2, 3, 5)


def _b_payload(seed):
    rng = np.random.default_rng(seed)
    a = _noise(rng, 65536)
    draws = rng.integers(0, 1 << 30, 65536)
    for i in range(6000, 65536 - 3, 4):
        s = i - 5000 - int(draws[i] % 800)
        a[i:i + 3] = a[s:s + 3]
    return a.tobytes()


def _b():
    out = [Case("B-s%d" % s, _b_payload(s), [65536], B_LEVELS) for s in B_SEEDS]
    return out + [Case("B-s2-halves", _b_payload(2), [32768, 32768], B_LEVELS)]


# ------------------------------------------------------------------ D ----

D_DIST = (4095, 4096, 4097, 32505, 32506, 32507, 32768)
D_LEN = (3, 4, 10, 258)
D_GRID = [(d, m) for d in D_DIST for m in D_LEN]  # block order of D and D7
D_FROM, D_SIZE = 100, 40000
D_LEVELS = (1, 4, 9)


def _d_payload(seed, mask):
    rng = np.random.default_rng(seed)
    parts = []
    for d, m in D_GRID:
        a = _noise(rng, D_SIZE) & mask
        a[D_FROM + d:D_FROM + d + m] = a[D_FROM:D_FROM + m]
        parts.append(a)
    return np.concatenate(parts).tobytes()


# A copy shows in zlib's tokens only if no later trigram of the noise shares the
# hash of its first three bytes (at the MAX_DIST edge the copy's source is reached
# as the head of its hash chain only) and no chance match gets in the way: the
# first seeds from 0xD0 up whose output passes test_bgzf_cases.py's D tests.
D_SEED, D7_SEED = 0xD4, 0xD1


def _d():
    lens = [D_SIZE] * len(D_GRID)
    return [Case("D", _d_payload(D_SEED, 0xFF), lens, D_LEVELS), Case("D7", _d_payload(D7_SEED, 0x7F), lens, D_LEVELS)]


# ------------------------------------------------------------------ R ----

R_LENS = (258, 259, 260, 261, 262, 263, 264, 516, 517, 520)
R_LEVELS = (1, 4, 6, 9)


def _r():
    parts = [b"A" * n for n in R_LENS] + [b"B" + b"A" * (n - 1) for n in R_LENS]
    return [Case("R", b"".join(parts), [len(p) for p in parts], R_LEVELS)]


# ------------------------------------------------------------------ C ----

C_LENS = (list(range(4, 17)) + list(range(60, 71)) + [127, 128, 129] + [4095, 4096, 4097] + [65535, 65536])


def _c_block_lens():
    pad = -sum(C_LENS) % 8  # a repeat is a multiple of 8 bytes, so only the one-byte blocks shift the next
    lens = []
    for k in range(8):
        lens += [1] * k + C_LENS + ([pad] if pad else [])
    return lens


def _c():
    rng = np.random.default_rng(0xC1)
    lens = _c_block_lens()
    bam, text = np.frombuffer(bam_payload(), np.uint8), _letters(rng, b"ACGTN", sum(lens))
    payload = text.copy()  # compressible throughout: BAM records and read text, 4 KiB each in turn
    for at in range(0, len(payload) - 4096, 8192):
        payload[at:at + 4096] = bam[at % (len(bam) - 4096):][:4096]
    starts = np.cumsum([0] + lens[:-1])
    seen = collections.defaultdict(set)
    for s, n in zip(starts, lens):
        seen[n].add(int(s) % 8)
    assert all(seen[n] == set(range(8)) for n in C_LENS), "a length misses a start alignment"
    return [Case("C", payload.tobytes(), lens, (5,))]


# ------------------------------------------------------------------ L ----

def _l():
    rng = np.random.default_rng(0x5A)
    n = 3 * 65498 + 1000
    kinds = {"acgt": _letters(rng, b"ACGT", n).tobytes(), "runs": _runs(n).tobytes(),
             "noise": _noise(rng, n).tobytes(), "bam": (bam_payload() * (n // len(bam_payload()) + 1))[:n]}
    lens = [65498] * 3 + [1000]
    return [Case("L-" + k, v, lens, (7, 8)) for k, v in kinds.items()]


# ----------------------------------------------------------- registry ----

FAMILIES = {"W1": _w1, "W1b": _w1_second, "W2": _w2, "F": _f, "E": _e, "B": _b, "D": _d, "R": _r, "C": _c, "L": _l}
NAMES = {"W1": ["W1"], "W1b": ["W1b"], "W2": ["W2"], "F": ["F"], "E": ["E"],
         "B": ["B-s%d" % s for s in B_SEEDS] + ["B-s2-halves"], "D": ["D", "D7"], "R": ["R"], "C": ["C"],
         "L": ["L-acgt", "L-runs", "L-noise", "L-bam"]}
LEVELS = {"W1": (1, 5, 0), "W1b": (5,), "W2": (5,), "F": tuple(range(1, 10)), "E": (1, 5), "D": D_LEVELS,
          "D7": D_LEVELS, "R": R_LEVELS, "C": (5,), "L-acgt": (7, 8), "L-runs": (7, 8), "L-noise": (7, 8),
          "L-bam": (7, 8), "B-s2": B_LEVELS, "B-s5": B_LEVELS, "B-s2-halves": B_LEVELS}
_FAMILY_OF = {n: f for f, names in NAMES.items() for n in names}
SMALL = [n for f, names in NAMES.items() if not f.startswith("W") for n in names]  # every family except W
ALL = [n for names in NAMES.values() for n in names]


@functools.lru_cache(maxsize=None)
def _family(f):
    cases = FAMILIES[f]()
    assert [c.name for c in cases] == NAMES[f]
    for c in cases:
        assert sum(c.block_lens) == len(c.payload) and max(c.block_lens) <= 65536
        assert tuple(c.levels) == tuple(LEVELS[c.name])
    return {c.name: c for c in cases}


def get(name):
    """The case of that name (built once per process)."""
    return _family(_FAMILY_OF[name])[name]


def params(names=None):
    """[(case name, level)] for pytest.mark.parametrize, without building a payload."""
    return [(n, lv) for n in (ALL if names is None else names) for lv in LEVELS[n]]


def cases():
    """Every case: [(name, payload bytes, block_lens, levels)]."""
    return [get(n) for n in ALL]


@functools.lru_cache(maxsize=None)
def want(name, level):
    """The oracle's BGZF file (system zlib, EOF block included) of a case at a level, computed once."""
    import orc
    c = get(name)
    return orc.bgzf_compress(c.payload, c.block_lens, level=level, eof=True)


def starts(block_lens):
    """Payload offset of every block."""
    return np.concatenate([[0], np.cumsum(block_lens[:-1], dtype=np.int64)]).tolist() if block_lens else []
