"""GPU: the anchored BGZF locate against the oracle and against the full scan
(hbam_set_locate with 0 segment bytes: the library as it was before the
anchored path).  Every case of locate_cases.py runs at 4 KiB and 64 KiB
segments, at the default and with the hook at 0; the four results must agree
with each other and with the oracle, and hbam_locate_counters must show the
path test_locate_cases.py proves for the case: an accepted range never
declines on the way, a declined one is counted once and not as anchored."""
import numpy as np
import pytest

import hbam
import locate_cases as lc
import orc
from test_gpu_parity import assert_same_records

pytestmark = pytest.mark.gpu

ALL = (1 << 64) - 1
CASES = lc.cases()
HOOKS = (lc.S_SMALL, lc.S_MID, hbam.LOCATE_SEG_DEFAULT, 0)


def _expect(case, S):
    return case.expect[lc.S_DEFAULT if S == hbam.LOCATE_SEG_DEFAULT else S]


def _delta(f, c0):
    c1 = f.pipeline_counters()
    return c1["locate_anchored"] - c0["locate_anchored"], c1["locate_declined"] - c0["locate_declined"]


def _table(f):
    b = f.blocks()
    return [b[k].tolist() for k in ("coff", "csize", "isize", "ustart")]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_match_oracle_and_scan(case):
    results = []
    for S in HOOKS:
        # a file of its own per hook: the whole-file block table is kept once built
        with hbam.BamFile(case.data, bam=case.bam) as f:
            f.set_locate(S, case.cap_limit)
            c0 = f.pipeline_counters()
            # the whole file is one window: this is its one locate
            r = f.decode_all() if case.bam else _table(f)
            anchored, declined = _delta(f, c0)
            if S == 0:
                assert (anchored, declined) == (0, 0)
            elif _expect(case, S) == "anchored":
                assert (anchored, declined) == (1, 0), S
            else:
                assert (anchored, declined) == (0, 1), S
            results.append((r, _table(f)))
    tables = [t for _, t in results]
    assert tables[0] == tables[1] == tables[2] == tables[3]
    if case.name == "other_subfield":
        # the oracle's framing needs the BC subfield: the scan path (the
        # parent's behaviour) is the reference
        want = results[3][0]
        assert want["status"] == 0 and len(want["key"]) > 0
        assert tables[3][0] == lc.block_starts(case.data)
        for r, _ in results[:3]:
            assert_same_records(r, want)
            assert r["data"] == want["data"]
        return
    s = orc.Stream(case.data, parse_header=case.bam)
    ob = s.blocks
    assert tables[0] == [ob[k].tolist() for k in ("coff", "csize", "isize", "ustart")]
    if case.bam:
        rc, want = s.decode_all()
        assert rc == 0
        for r, _ in results:
            assert r["status"] == 0
            assert_same_records(r, want, s.data)
    else:
        for S in HOOKS:
            with hbam.BamFile(case.data, bam=False) as f:
                f.set_locate(S)
                assert f.read_inflated(0, len(s.data)) == s.data


def test_window_from_the_third_block(test_bam):
    s = orc.Stream(test_bam)
    rc, allr = s.decode_all()
    third = int(s.blocks["coff"][2])
    vs = int(next(v for v in allr["voff"] if int(v) >> 16 >= third))
    assert vs >> 16 == third
    rc, want = s.decode_span(vs, ALL)
    got = []
    with hbam.BamFile(test_bam, window_bytes=1 << 30) as f:
        for S in HOOKS:
            f.set_locate(S)
            c0 = f.pipeline_counters()
            r = f.decode_span(vs, ALL)
            anchored, declined = _delta(f, c0)
            assert declined == 0 and (anchored >= 1 if S else anchored == 0)
            assert_same_records(r, want)
            got.append(r["key"])
    assert all(np.array_equal(g, got[3]) for g in got)


def test_two_window_read():
    """64 KiB windows: every range but the last ends at a block that the
    window's end cuts (the partial rule), none declines."""
    data = lc.windowed()
    s = orc.Stream(data)
    rc, want = s.decode_all()
    assert rc == 0
    for S in HOOKS:
        with hbam.BamFile(data, window_bytes=1 << 16) as f:
            f.set_locate(S)
            c0 = f.pipeline_counters()
            got = f.decode_all()
            anchored, declined = _delta(f, c0)
            assert declined == 0 and (anchored >= 2 if S else anchored == 0), S
            assert_same_records(got, want, s.data)


def _outcome(fn):
    try:
        r = fn()
    except hbam.HbamError as e:
        return ("error", e.code, str(e))
    return ("ok", r)


def test_truncated_file_errors_are_the_scans():
    """A file cut mid-block.  Whole (no `partial`): the anchored path declines
    and the error is the scan path's, status and message.  In 64 KiB windows
    the ranges before the cut are accepted, the one holding the cut declines."""
    data = lc.truncated()
    whole, windows = [], []
    for S in HOOKS:
        g = hbam.Gpu(0)
        try:
            g.set_window(1 << 16)  # (the load reads the header from the first window only)
            g.load(data)
            g.set_locate(S)
            g.set_window(0)
            a0, d0 = g.locate_counters()
            whole.append(_outcome(lambda: g.run()["status"]))
            a1, d1 = g.locate_counters()
            assert (a1 - a0, d1 - d0) == ((0, 1) if S else (0, 0)), S
        finally:
            g.close()
        with hbam.BamFile(data, window_bytes=1 << 16) as f:
            f.set_locate(S)
            c0 = f.pipeline_counters()
            out = _outcome(lambda: f.decode_all(raise_on_error=False))
            anchored, declined = _delta(f, c0)
            assert (anchored >= 1 and declined >= 1) if S else (anchored, declined) == (0, 0), S
            windows.append(out if out[0] == "error" else ("ok", out[1]["status"], out[1]["key"].tobytes()))
    assert whole[3][0] == "error" and whole[3][1] == hbam.E_TRUNC
    assert whole[0] == whole[1] == whole[2] == whole[3]
    assert windows[0] == windows[1] == windows[2] == windows[3]


def test_streamed_pieces():
    """run_streamed with 1 MiB pieces: ranges appended to a table that already
    holds blocks (nprev > 0, ubase != 0), each cut by its piece's end."""
    from hbam import synth
    data, info = synth.make_bam(17000, as_numpy=True)
    assert data.nbytes > (2 << 20)
    s = orc.Stream(data.tobytes())
    rc, want = s.decode_all()
    assert rc == 0
    g = hbam.Gpu(0)
    buf = hbam.PinnedBuffer(data.nbytes)
    try:
        g.load(data)
        buf.array[:] = data
        for S in HOOKS:
            g.set_locate(S)
            a0, d0 = g.locate_counters()
            st = g.run_streamed(buf.ptr, data.nbytes, 1 << 20)
            a1, d1 = g.locate_counters()
            assert d1 == d0 and (a1 - a0 >= 3 if S else a1 == a0), S
            assert st["status"] == 0 and st["n_blocks"] == info["blocks"]
            k, v = g.fetch(st["records"])
            np.testing.assert_array_equal(k, want["key"])
            np.testing.assert_array_equal(v, want["voff"])
    finally:
        buf.close()
        g.close()


def test_truncated_streamed_upload_errors_are_the_scans():
    data = np.frombuffer(lc.truncated(), np.uint8)
    outs = []
    for S in HOOKS:
        g = hbam.Gpu(0)
        buf = hbam.PinnedBuffer(data.nbytes)
        try:
            g.set_window(1 << 16)
            g.load(data)
            g.set_locate(S)
            buf.array[:] = data
            outs.append(_outcome(lambda: g.run_streamed(buf.ptr, data.nbytes, 1 << 20)["status"]))
        finally:
            buf.close()
            g.close()
    assert outs[3][0] == "error"
    assert outs[0] == outs[1] == outs[2] == outs[3]
