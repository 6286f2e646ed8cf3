"""Inflate on DEFLATE streams zlib's own encoder never writes: single blocks of
65 K symbols, stored blocks between dynamic ones, hundreds of DEFLATE blocks in
one BGZF block, distance 32,768, periodic matches up to ISIZE, 15-bit and
sub-table-filling codes, and the legal-but-odd (and the illegal) dynamic
headers.  The streams come from deflate_cases (a test-side encoder; its CPU
tests show that zlib alone decides each case); the reference is what it is for
every inflate test: zlib's inflate driven as [htsjdk] BlockGunzipper drives it,
plus the oracle's status (check() of test_gpu_inflate_lean).  All comparisons
are bit-exact.

Path counts (lean, fallback rounds of a BGZF block) are asserted only where
the design fixes them: where the first DEFLATE block is stored, fixed or has a
header k_huff_tables refuses, round 0 is the fallback's.  It decodes on until
the next header it may defer, so a lean round can only be the second (and
last) one, and a block that fails in round 0 takes no lean round at all.
Elsewhere the counts are recorded in the assertion message."""
import numpy as np
import pytest

import deflate_cases as dc
import hbam
from hbam import synth
from test_gpu_inflate_lean import EOF_BLOCK, bgzf, check, expected, good_neighbours, letters

pytestmark = pytest.mark.gpu

STATUS = {"OK": hbam.OK, "E_IO": hbam.E_IO, "E_FORMAT": hbam.E_FORMAT}


def block(c):
    return bgzf(c.cdata, c.out or b"", isize=c.isize)


@pytest.fixture(scope="module")
def neighbours():
    """A good block to put on either side of a bad one, and the rounds two of them take."""
    ok = good_neighbours(np.random.default_rng(20))
    lean, fb, _ = check(ok + ok + EOF_BLOCK)
    assert (lean, fb) == (2, 0)
    return ok, lean


@pytest.mark.parametrize("cid", dc.VALID)
def test_valid_case(cid):
    c = dc.get(cid)
    data = block(c) + EOF_BLOCK
    want = expected(data)
    assert want == (hbam.OK, c.out)  # zlib and expand() agree
    lean, fb, _ = check(data, want)
    print("%s (lean, fallback) = (%d, %d)" % (cid, lean, fb))
    assert lean + fb >= 1, (cid, lean, fb)
    if c.lean0:  # round 0 went to the fallback; of the two rounds only the second can be lean
        assert fb >= 1 and lean <= 1, (cid, lean, fb)


@pytest.mark.parametrize("cid", dc.INVALID)
def test_invalid_case_between_good_blocks(cid, neighbours):
    c = dc.get(cid)
    ok, ok_lean = neighbours
    data = ok + block(c) + ok + EOF_BLOCK
    want = expected(data)
    assert want == (STATUS[c.want], len(ok))
    lean, fb, _ = check(data, want)
    print("%s (lean, fallback) = (%d, %d) with %d lean rounds of the neighbours" % (cid, lean, fb, ok_lean))
    if c.lean0:  # the block failed in round 0, in the fallback: the neighbours' lean rounds only
        assert (lean, fb) == (ok_lean, 1), (cid, lean, fb)


@pytest.mark.parametrize("k", range(1, 16))
@pytest.mark.parametrize("cid", ["M4-p7-65280", "M1"])
def test_match_case_at_every_output_offset(cid, k):
    """M5: a block of k bytes in front moves the case's first output byte over
    all offsets within 16 B (k = 0 is test_valid_case); the neighbours' bytes
    on both sides stay intact."""
    c = dc.get(cid)
    rng = np.random.default_rng(500 + k)
    head, tail = letters(rng, k), letters(rng, 100)
    data = bgzf(dc.enc_auto(head), head) + block(c) + bgzf(dc.enc_auto(tail), tail) + EOF_BLOCK
    want = expected(data)
    assert want == (hbam.OK, head + c.out + tail)
    lean, fb, _ = check(data, want)
    assert lean + fb >= 3, (cid, k, lean, fb)


def test_all_valid_cases_in_one_file():
    rng = np.random.default_rng(600)
    blocks = [block(dc.get(cid)) for cid in dc.VALID]
    want_out = [dc.get(cid).out for cid in dc.VALID]
    bam, _ = synth.make_bam(1200, level=5, eof_block=False)
    rc, bam_out = expected(bam)
    assert rc == hbam.OK
    order = [int(i) for i in rng.permutation(2 * len(blocks) + 1) % (len(blocks) + 1)]
    assert sorted(order).count(len(blocks)) >= 1
    data = b"".join(bam if i == len(blocks) else blocks[i] for i in order) + EOF_BLOCK
    want = (hbam.OK, b"".join(bam_out if i == len(blocks) else want_out[i] for i in order))
    assert expected(data) == want
    lean, fb, _ = check(data, want)
    assert lean > 0 and fb > 0, (lean, fb)
