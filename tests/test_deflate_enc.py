"""The fixtures of test_gpu_inflate_shapes.py are sound: zlib's inflate, driven
as [htsjdk] BlockGunzipper drives it (one raw inflate, ISIZE bytes of room),
decodes every valid case of deflate_cases to expand(tokens) and refuses or
comes up short on every invalid one, with the message the case names.  zlib
alone decides; no case is skipped or filtered."""
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_enc as enc


def zlib_says(cdata, isize):
    """(status, bytes | zlib's message) of one raw inflate with isize bytes of room."""
    try:
        out = zlib.decompressobj(-15).decompress(cdata, isize)
    except zlib.error as e:
        return "E_IO", str(e)
    return ("OK", out) if len(out) == isize else ("E_FORMAT", None)


def test_every_case_of_the_tables_is_there():
    ids = set(dc.REGISTRY)
    assert set(dc.VALID) | set(dc.INVALID) == ids and not set(dc.VALID) & set(dc.INVALID)
    heads = {i.split("-")[0].split("@")[0] for i in ids}
    assert heads >= {"S1", "S2", "S3", "S3b", "S3c", "S3d", "S3e", "S3f", "S4", "S5", "S6",
                     "M1", "M2", "M2b", "M3", "M3b", "M3c", "M4", "M4b", "M6", "T1", "T2", "T3",
                     "H1", "H1b", "H2", "H3", "H3b", "H3c", "H4", "H4b", "H4c", "H5", "H5b",
                     "H6", "H6b", "H6c", "H6d", "H6e", "H6f", "H7", "H7b", "H7c"}
    for h in [i for i in ids if i.endswith("@1")]:  # every header case as first and as third block
        assert h[:-2] + "@3" in ids
    assert {"M4-p%d-65280" % p for p in (1, 2, 3, 7, 255, 256, 257, 258, 259)} <= ids
    assert {"M4-p1-65536", "M4-p3-65536", "S2-65280", "S2-65536", "S1-cont1", "S1-cont", "S2-cont"} <= ids


@pytest.mark.parametrize("cid", dc.VALID)
def test_valid_case_inflates_to_its_tokens(cid):
    c = dc.get(cid)
    assert c.want == "OK" and len(c.out) == c.isize
    assert zlib_says(c.cdata, c.isize) == ("OK", c.out)


@pytest.mark.parametrize("cid", dc.INVALID)
def test_invalid_case_fails_as_listed(cid):
    c = dc.get(cid)
    assert c.want in ("E_IO", "E_FORMAT") and c.out is None
    rc, msg = zlib_says(c.cdata, c.isize)
    assert rc == c.want
    if c.msg is not None:
        assert c.msg in msg


def test_cases_have_the_shapes_they_are_for():
    assert dc.get("S1").isize == 65280 and 18000 < len(dc.get("S1").cdata) < 19000
    assert dc.get("S2-65536").isize == 65536
    assert dc.get("M4b").isize == 65280
    for pad in range(8):  # the stream ends in `pad` one bits after the end-of-block code
        last = dc.get("S6-pad%d" % pad).cdata[-1]
        assert last >> (8 - pad) == (1 << pad) - 1
    # M1 / T3 reach distance 32,768: code 29 with all 13 extra bits set
    assert enc.dist_code(32768) == (29, 8191)
    # M6: the stream stands for more than the footer says
    d = zlib.decompressobj(-15)
    assert len(d.decompress(dc.get("M6-257").cdata)) == dc.get("M6-257").isize + 257


def test_t2_fills_the_sub_tables():
    """The committed T2 length sets are complete codes over all 286 / 30
    symbols and need 306 litlen and 80 distance sub-table entries (root 10 /
    9; the search that found them: seeded random splits of a Kraft-complete
    tree, 20,000 draws, then split+merge moves).  The issue's floor is 256 / 64."""
    assert sorted(dc.T2_LIT_ORDER) == list(range(286)) and sorted(dc.T2_DIST_ORDER) == list(range(30))
    assert all(dc.T2_LL) and all(dc.T2_DL) and len(dc.T2_LL) == 286 and len(dc.T2_DL) == 30
    assert enc.kraft(dc.T2_LL) == enc.kraft(dc.T2_DL) == 1 << 15
    lit, dist = dc.sub_entries(dc.T2_LL, 10), dc.sub_entries(dc.T2_DL, 9)
    assert (lit, dist) == (306, 80)
    assert lit >= 256 and dist >= 64
    # T1: complete, 15-bit codes on both sides
    assert enc.kraft(dc.T1_LL) == enc.kraft(dc.T1_DL) == 1 << 15 and max(dc.T1_LL) == max(dc.T1_DL) == 15


# ---- the encoder's own parts
def test_canonical_codes_rfc1951_example():
    assert enc.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]


def test_fixed_codes_are_the_rfc_ones():
    c = enc.canonical_codes(enc.FIXED_LITLEN)
    assert (c[0], c[143], c[144], c[255], c[256], c[279], c[280], c[287]) == \
        (0x30, 0xbf, 0x190, 0x1ff, 0, 0x17, 0xc0, 0xc7)


@pytest.mark.parametrize("maxbits", [7, 9, 15])
def test_limited_lengths_are_complete_and_limited(maxbits):
    rng = np.random.default_rng(maxbits)
    for n in (2, 3, 19, 30, 100):
        if n > 1 << maxbits:
            continue
        freqs = [int(v) for v in (rng.integers(1, 4, n) ** rng.integers(1, 12, n))]
        lens = enc.limited_lengths(freqs + [0, 0], maxbits)
        assert lens[-2:] == [0, 0] and 0 < min(lens[:n]) and max(lens) <= maxbits
        assert enc.kraft(lens, maxbits) == 1 << maxbits
    assert enc.limited_lengths([0, 5, 0], maxbits) == [0, 1, 0]


def test_length_and_distance_codes_cover_their_ranges():
    assert [enc.length_code(n) for n in (3, 10, 11, 12, 257, 258)] == [(0, 0), (7, 0), (8, 0), (8, 1), (27, 30), (28, 0)]
    assert [enc.dist_code(d) for d in (1, 4, 5, 6, 7, 24576, 24577)] == \
        [(0, 0), (3, 0), (4, 0), (4, 1), (5, 0), (28, 8191), (29, 0)]
    for n in range(3, 259):
        i, x = enc.length_code(n)
        assert enc.LEN_BASE[i] + x == n and (x < 1 << enc.LEN_EXTRA[i])
    for d in range(1, 32769):
        j, x = enc.dist_code(d)
        assert enc.DIST_BASE[j] + x == d and x < 1 << enc.DIST_EXTRA[j]


def test_expand_overlapping_matches_and_history():
    assert enc.expand([("L", 97), ("M", 5, 1)]) == b"aaaaaa"
    assert enc.expand([("L", 97), ("L", 98), ("M", 5, 2)]) == b"abababa"
    assert enc.expand([("M", 4, 3)], history=b"xyz") == b"xyzx"
    with pytest.raises(AssertionError):
        enc.expand([("L", 97), ("M", 3, 2)])


@pytest.mark.parametrize("kind", ["fixed", "dynamic", "norle", "hclen19", "stored"])
def test_block_writers_round_trip(kind):
    rng = np.random.default_rng(5)
    toks = dc.rand_tokens(rng, 2000, 0)
    w = enc.BitWriter()
    if kind == "fixed":
        enc.put_fixed(w, toks, True)
    elif kind == "stored":
        enc.put_fixed(w, [], False)  # 10 bits: the stored block's header starts off a byte boundary
        enc.put_stored(w, enc.expand(toks), True)
    else:
        mode = dict(norle=dict(rle=False), hclen19=dict(hclen=19)).get(kind)
        enc.put_auto(w, toks, True, clen_mode=mode)
    d = zlib.decompressobj(-15)
    assert d.decompress(w.getvalue()) == enc.expand(toks)
    assert d.eof and d.unused_data == b""
