"""End-to-end pass from host memory (hbam_gpu_run_streamed): the compressed
file is copied to HBM in pieces while the blocks of landed pieces are located
and inflated.  Results must be identical to the device-resident pass (which
the parity tests pin against the oracle) and to the oracle itself."""
import numpy as np
import pytest

import deflate_cases as dc
import hbam
import locate_cases as lc
import orc
from hbam import synth
from test_gpu_inflate_lean import gunzip_block
from test_gpu_inflate_shapes import STATUS, block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw,piece", [
    (dict(n_records=60000), 1 << 20),                          # ~18 pieces, blocks cut at every piece end
    (dict(n_records=40000, block_payload=4096), 1 << 20),      # small blocks: many per piece
    (dict(n_records=8000, level=0), 1 << 20),                  # stored blocks (csize ~ 64 KiB)
    (dict(n_records=300, mode="long"), 3 << 20),               # records spanning blocks and pieces
    (dict(n_records=20000), 64 << 20),                         # one piece
])
def test_streamed_matches_resident_and_oracle(kw, piece):
    data, info = synth.make_bam(as_numpy=True, **kw)
    g = hbam.Gpu(0)
    buf = hbam.PinnedBuffer(data.nbytes)
    try:
        g.load(data)
        st0 = g.run()
        k0, v0 = g.fetch(st0["records"])
        buf.array[:] = data
        st = g.run_streamed(buf.ptr, data.nbytes, piece)
        assert st["status"] == 0
        assert st["records"] == st0["records"] == kw["n_records"]
        assert st["n_blocks"] == info["blocks"]
        assert st["inflated_bytes"] == info["uncompressed"]
        k1, v1 = g.fetch(st["records"])
        np.testing.assert_array_equal(k1, k0)
        np.testing.assert_array_equal(v1, v0)
        # and a second streamed pass over the same buffers (state reset)
        st2 = g.run_streamed(buf.ptr, data.nbytes, piece)
        k2, _ = g.fetch(st2["records"])
        np.testing.assert_array_equal(k2, k0)
    finally:
        buf.close()
        g.close()
    s = orc.Stream(data.tobytes())
    rc, want = s.decode_all()
    assert rc == 0
    np.testing.assert_array_equal(k1, want["key"])
    np.testing.assert_array_equal(v1, want["voff"])


# ---- a DEFLATE error in a later piece: one verdict for the resident and the streamed pass
def _short_of_isize(cid):
    """A valid case of deflate_cases under a footer ISIZE one byte larger than
    its stream holds: [htsjdk] BlockGunzipper's "Did not inflate expected
    amount".  (deflate_cases.INVALID has no case of that status: zlib refuses
    every one of its streams.)"""
    c = dc.get(cid)
    assert c.want == "OK" and c.isize < 65536
    return c._replace(id=cid + "+1", out=None, isize=c.isize + 1, want="E_FORMAT")


BAD_BLOCKS = {
    "M2": ("E_IO", "invalid DEFLATE data", lambda: dc.get("M2")),
    "S3+1": ("E_FORMAT", "Did not inflate expected amount", lambda: _short_of_isize("S3")),
}
assert "M2" in dc.INVALID


@pytest.fixture(scope="module")
def two_pieces():
    """A BAM of more than two 1 MiB pieces, its oracle keys and the end of the
    first block that starts in the second piece."""
    data, _ = synth.make_bam(17000)
    assert len(data) > (2 << 20)
    starts = lc.block_starts(data)
    k = next(i for i, p in enumerate(starts) if p >= (1 << 20))
    assert starts[k + 1] < (2 << 20)
    rc, want = orc.Stream(data).decode_all()
    assert rc == 0
    return data, want["key"], starts[k + 1]


@pytest.mark.parametrize("cid", list(BAD_BLOCKS))
def test_deflate_error_in_second_piece(cid, two_pieces):
    want, text, make = BAD_BLOCKS[cid]
    c = make()
    assert c.want == want and gunzip_block(c.cdata, c.isize)[0] == STATUS[want]
    good, keys, at = two_pieces
    bad = np.frombuffer(good[:at] + block(c) + good[at:], np.uint8)
    msg = "%s in BGZF block at offset %d" % (text, at)
    g = hbam.Gpu(0)
    buf = hbam.PinnedBuffer(bad.nbytes)
    try:
        g.load(bad)
        buf.array[:] = bad
        with pytest.raises(hbam.HbamError) as resident:
            g.run()
        with pytest.raises(hbam.HbamError) as streamed:
            g.run_streamed(buf.ptr, bad.nbytes, 1 << 20)
        print("resident: %s\nstreamed: %s" % (resident.value, streamed.value))
        assert resident.value.code == streamed.value.code == STATUS[want]
        assert str(resident.value) == str(streamed.value) == "%s: %s" % (hbam.ERROR_NAMES[STATUS[want]], msg)
        # the failed passes leave no block marked inflated: the good file decodes
        g.load(good)
        st = g.run()
        assert st["status"] == 0 and st["records"] == len(keys)
        np.testing.assert_array_equal(g.fetch(st["records"])[0], keys)
    finally:
        buf.close()
        g.close()
