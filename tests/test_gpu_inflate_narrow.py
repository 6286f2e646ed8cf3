"""Inflate phase A's narrow instance: in a round after a BGZF block's first,
the lean body runs 128 lanes wide over the chunk (k_inflate_huff<128>, a 16 KB
workgroup), hands a block whose round window its stage does not hold up to the
256-lane instance through a list, and anything else it cannot finish to the
fallback, as the 256-lane instance does.

Every case is a few BGZF blocks built with Python's zlib (Z_BLOCK between the
parts, so each part is one DEFLATE block) or tests/deflate_enc.py, compared
byte for byte (or by first failing block) with zlib, and checks the path
through inflate_narrow_counts() and inflate_path_counts()."""
import functools
import zlib

import numpy as np
import pytest

import deflate_enc as enc
import hbam
from deflate_cases import S1_LL, Stream, lengths_at, lits
from test_gpu_inflate_lean import EOF_BLOCK, bgzf, deflate, expected, letters, texty

pytestmark = pytest.mark.gpu


def run(data):
    """The GPU's bytes equal zlib's; returns (lean, fallback, narrow, stage cap)."""
    want = expected(data)
    assert want[0] == hbam.OK
    with hbam.BamFile(data, bam=False) as f:
        n = int(sum(int(x) for x in f.blocks()["isize"]))
        got = f.read_inflated(0, n)
        lean, fb, _ = f.inflate_path_counts()
        narrow, resident, cap = f.inflate_narrow_counts()
    assert got == want[1]
    assert narrow <= lean
    assert resident >= 1 and 8192 <= cap <= 32768
    return lean, fb, narrow, cap


def two_part(a, b, **kw):
    return bgzf(deflate([a, b], **kw)[0], a + b)


def test_ordinary_two_part_blocks_run_narrow():
    rng = np.random.default_rng(21)
    blocks = [two_part(letters(rng, 9000), texty(rng, 9000)) for _ in range(5)]
    lean, fb, narrow, _ = run(b"".join(blocks) + EOF_BLOCK)
    assert (lean, fb, narrow) == (10, 0, 5)


def test_narrow_occupancy_and_cap_before_any_inflate():
    rng = np.random.default_rng(22)
    with hbam.BamFile(two_part(letters(rng, 3000), texty(rng, 3000)) + EOF_BLOCK, bam=False) as f:
        narrow, resident, cap = f.inflate_narrow_counts()
    assert narrow == 0 and resident >= 1 and cap % 16 == 0


def dynamic_tail(first_tokens, tail):
    """One BGZF block of two dynamic-code DEFLATE blocks, the second (final)
    one the literals of `tail` (at most three different bytes).  zlib's
    encoder writes so short a tail with the fixed codes, which have no
    prebuilt tables and go to the fallback.  So does a dynamic block whose
    header ends within 14 bits of the end of CDATA: k_huff_tables' parallel
    parse stops at a code-length symbol that might cross the end and leaves
    the header to the fallback's serial one, so a 1-bit code for one byte
    never reaches a lean instance of either width.  Here the tail's bytes and
    the end-of-block take the four 8-bit codes of a complete code (lengths 1
    to 6 on unused letters): 16 to 32 bits of symbols, which the narrow
    instance cuts into slices of one bit with most of its lanes empty."""
    used = sorted(set(tail)) + [256]
    spare = [s for s in range(32, 64) if s not in used]
    ll = lengths_at(257, [(spare[i], i + 1) for i in range(6)] + [(s, 8) for s in used + spare[6:10 - len(used)]])
    assert enc.kraft(ll) == 1 << 15
    c = Stream().auto(first_tokens).dyn(lits(tail), ll, [0], True).ok("tail")
    assert c.out.endswith(tail)
    return bgzf(c.cdata, c.out)


@pytest.mark.parametrize("tail", [b"zq", b"z", b"BBB"])
def test_second_block_far_shorter_than_a_slice_per_lane(tail):
    rng = np.random.default_rng(23)
    lean, fb, narrow, _ = run(dynamic_tail(lits(texty(rng, 5000)), tail) + EOF_BLOCK)
    assert (lean, fb, narrow) == (2, 0, 1)


def test_single_code_run_then_a_short_tail():
    """b"A" * 20000 as zlib cuts it (a literal, then matches at distance 1),
    then b"B" * 3 as a dynamic block of its own."""
    run_a = [("L", 65)] + [("M", 258, 1)] * 77 + [("M", 133, 1)]
    data = dynamic_tail(run_a, b"B" * 3)
    assert expected(data)[1] == b"A" * 20000 + b"B" * 3
    lean, fb, narrow, _ = run(data + EOF_BLOCK)
    assert (lean, fb, narrow) == (2, 0, 1)


def round1_window(ncdata, b0):
    """Bytes of the round-1 window of a BGZF block at file offset 0 with
    ncdata bytes of CDATA, the second DEFLATE block's first symbol b0 bits into
    it: whole 16 B units of the file from the unit that holds that
    symbol to the unit 176 bits past the end of CDATA, the block's own units
    plus one at the most."""
    base = 18 & ~15  # CDATA starts 18 B into the block
    first = (8 * (18 - base) + b0) >> 7
    last = min((8 * (18 - base + ncdata) + 176) >> 7, (ncdata + 26 - base + 15) >> 4)
    return 16 * (last + 1 - first)


def test_stage_cap_boundary():
    """The second part is near-incompressible literals under a code made for
    them, its length stepped so that the round-1 window crosses the narrow
    stage's cap.  The encoder's bit count gives the window exactly: every
    length whose window lies within 64 B of the cap is run, the cap itself and
    the 16 B above it among them, and one far to either side.  A window up to
    the cap is the narrow instance's, a larger one the 256-lane instance's
    through the hand-up list, none the fallback's."""
    with hbam.BamFile(bgzf(deflate([b"x"])[0], b"x") + EOF_BLOCK, bam=False) as f:
        cap = f.inflate_narrow_counts()[2]
    rng = np.random.default_rng(24)
    first = lits(letters(rng, 4000))
    pool = letters(rng, cap + cap // 4, 200, 20)
    nbits1 = Stream().auto(first).w.nbits

    @functools.lru_cache(maxsize=None)
    def window(n2):
        tok2 = lits(pool[:n2])
        nbits = nbits1 + Stream().auto(tok2, True).w.nbits
        ll = enc.limited_lengths(enc.token_freqs(tok2)[0], 15)  # the code auto() made
        return round1_window((nbits + 7) // 8, nbits - sum(ll[t[1]] for t in tok2) - ll[256])

    lengths = [cap // 2]
    n2 = cap - 64  # (more than 7 bits a letter: this window is still below the cap)
    assert window(n2) < cap - 64
    while window(n2) <= cap + 64:
        if window(n2) >= cap - 64 and window(n2) != window(lengths[-1]):
            lengths.append(n2)  # the first length of each window size
        n2 += 8  # 8 B of CDATA at the most: no 16 B unit is stepped over
    lengths.append(len(pool))
    wins = [window(n) for n in lengths]
    assert wins[0] < cap - 64 and wins[-1] > cap + 64
    assert wins[1:-1] == [cap + d for d in range(-64, 65, 16)]
    for n, win in zip(lengths, wins):
        c = Stream().auto(first).auto(lits(pool[:n]), True).ok("cap")
        lean, fb, narrow, got_cap = run(bgzf(c.cdata, c.out) + EOF_BLOCK)
        assert got_cap == cap
        assert (lean, fb, narrow) == (2, 0, 1 if win <= cap else 0), (n, win, cap)


def test_continuation_pass_in_the_second_block():
    """A long non-final second block under S1's code, whose size estimate
    (16,383 symbols) is short of it: the first all-lane pass ends inside the
    block.  Its length is stepped over the end of that pass, so that in some
    blocks the rest is staged and a continuation pass runs in the narrow
    instance, in others not.

    What this checks is the hand-over, not the continuation's own work.  A
    continuation exists only in a non-final block (a final one is one pass to
    the end of CDATA), and with two rounds a non-final second block ends at a
    third header in the last round, which the design leaves to the fallback:
    the narrow instance's continuation branch can only end in a hand-over, the
    fallback redoes the round from the state at round entry, and nothing the
    narrow continuation computed is observed.  So the test holds that such
    blocks are handed over with that state intact (the bytes are right) and
    never counted as narrow rounds; it passes whether or not the continuation
    pass itself is right.  Only a build with three rounds would show that."""
    rng = np.random.default_rng(25)
    first = letters(rng, 3000)
    blocks = []
    for n in range(17200, 19300, 150):
        acgt = bytes(np.array([65, 67, 71, 84], dtype=np.uint8)[rng.integers(0, 4, n)])
        s = Stream().auto(lits(first)).dyn(lits(acgt), S1_LL, [1]).auto(lits(b"end"), True)
        c = s.ok("cont")
        assert c.out == first + acgt + b"end"
        blocks.append(bgzf(c.cdata, c.out))
    lean, fb, narrow, _ = run(b"".join(blocks) + EOF_BLOCK)
    assert (lean, fb, narrow) == (len(blocks), len(blocks), 0)


def test_matches_reach_back_into_the_first_block():
    rng = np.random.default_rng(26)
    first = texty(rng, 9000)
    second = bytearray()
    while len(second) < 9000:
        o, n = int(rng.integers(0, 8900)), int(rng.integers(8, 90))
        second += first[o:o + n]
    blocks = [two_part(first, bytes(second)), two_part(first[:5000], bytes(second[:7000]))]
    lean, fb, narrow, _ = run(b"".join(blocks) + EOF_BLOCK)
    assert (lean, fb, narrow) == (4, 0, 2)


@pytest.mark.parametrize("kind", ["geometric", "two symbols"])
def test_second_block_where_walks_hardly_converge(kind):
    """Literals only under a steeply skewed code: code lengths from 1 bit up,
    so a walk started off the true path stays off it for long and sync runs
    many iterations."""
    rng = np.random.default_rng(27)
    if kind == "geometric":
        second = bytes(np.minimum(rng.geometric(0.5, 16000) + 47, 90).astype(np.uint8))
    else:
        second = bytes(np.where(rng.random(16000) < 0.97, 65, 66).astype(np.uint8))
    first = letters(rng, 6000)
    blk = two_part(first, second, strategy=zlib.Z_HUFFMAN_ONLY)
    lean, fb, narrow, _ = run(blk + blk + EOF_BLOCK)
    assert (lean, fb, narrow) == (4, 0, 2)


def test_every_block_handed_up():
    """300 blocks whose round-1 window exceeds the narrow stage: all go
    through the hand-up list (its 16 sub-lists), none to the fallback."""
    rng = np.random.default_rng(28)
    pool = letters(rng, 16000, 200, 20)
    blocks, len2 = [], []
    for i in range(300):
        a, b = letters(rng, 600), pool[i:i + 9600 + 7 * (i % 11)]
        c, marks = deflate([a, b], mem=9)
        blocks.append(bgzf(c, a + b))
        len2.append(len(c) - marks[0])
    lean, fb, narrow, cap = run(b"".join(blocks) + EOF_BLOCK)
    assert min(len2) - 300 > cap  # (less the header: every window is larger than the stage)
    assert (lean, fb, narrow) == (600, 0, 0)
