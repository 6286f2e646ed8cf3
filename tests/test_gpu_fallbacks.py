"""The record pass's edge paths (Pipeline::decode_span_pos):
  (a) an early stop that is not an error, with records listed after it:
      [htsjdk] an empty BGZF block right after an exhausted one reads as EOF,
      so the reader stops mid-file, and when the blocks after it start at a
      record (a chain the walks follow) the fused check + output launch
      (k_rec_check_out) lists records there too.  The span ends at the first
      stop: those records are dropped (before round 5 a fallback rescanned
      the counts and kept them: 5,808 records where the reference reads
      3,000);
  (b) a list overflow: SplittingBAMIndexer.index (SplittingBAMIndexer.java:
      262-287) skips block_size bytes whatever they are, so block_size-0
      records are 4 bytes long and a 64 KiB block holds more of them than a
      list has room for (kListCap, sized for >= 36-byte reader records): the
      per-block walks count and emit the records instead (k_rec_count,
      k_rec_emit), and stop at EOF the same way.
Each case is checked against the oracle, and hbam_pipeline_counters shows
the path that ran."""
import struct

import numpy as np
import pytest

import hbam
import orc
from hbam import synth
from test_gpu_parity import assert_same_records

pytestmark = pytest.mark.gpu
ALL = (1 << 64) - 1


def _with_eof_stop(break_record=None):
    """3,000 records, an EOF block, then 3,000 more from a block start
    (break_record: that one of them with a wrong bin, a STRICT-only error)."""
    d1, _ = synth.make_bam(3000, eof_block=True)
    d2, _ = synth.make_bam(3000, seed=99, eof_block=False)
    s2 = orc.Stream(d2)
    # file 2's records re-cut into blocks that start at its first record, so
    # that the chain goes on through them past file 1's EOF block: the reader
    # stops at the empty block (no error), and the walks list records after it
    recs = bytearray(s2.data[s2.header_end:])
    if break_record is not None:
        q = 0
        for _ in range(break_record):
            q += 4 + struct.unpack_from("<i", recs, q)[0]
        struct.pack_into("<H", recs, q + 14, 1)
    recs = bytes(recs)
    lens = [min(65280, len(recs) - a) for a in range(0, len(recs), 65280)]
    return d1 + orc.bgzf_compress(recs, lens, level=5, eof=True)


def test_records_after_an_eof_block_take_the_separate_launches():
    data = _with_eof_stop()
    s = orc.Stream(data)
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 3000
    with hbam.BamFile(data, window_bytes=1 << 30) as f:
        c0 = f.pipeline_counters()
        got = f.decode_all()
        assert_same_records(got, want)
        c1 = f.pipeline_counters()
        assert c1["records_after_stop"] > c0["records_after_stop"]
        st = f.decode_span_device(f.header()["first_record_voff"], ALL)
        assert st["records"] == 3000 and st["status"] == 0
        assert f.splitting_index(5) == s.splitting_index(5)


def test_an_invalid_record_after_an_eof_block():
    """(a) with a STRICT-invalid record among the records listed after the
    EOF block.  From the file's start the reader stops at the empty block
    before it reaches that record: 3,000 records, status 0 -- the verdict on
    a record listed past the first stop never becomes the span's.  A span
    that starts at the block after the EOF block reaches it: the records up
    to it and the oracle's status.  (Reader-mode lists cannot overflow --
    kListCap holds every start of records of 36 bytes or more -- so both go
    through k_rec_check_out; k_rec_count runs for the indexer only, below.)"""
    d1, _ = synth.make_bam(3000, eof_block=True)
    data = _with_eof_stop(break_record=700)
    assert data[:len(d1)] == d1
    s = orc.Stream(data)
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 3000
    rc2, want2 = s.decode_span(len(d1) << 16, ALL)
    assert rc2 == 1 and len(want2["key"]) == 700
    with hbam.BamFile(data, window_bytes=1 << 30) as f:
        c0 = f.pipeline_counters()
        got = f.decode_all()
        assert got["status"] == 0
        assert_same_records(got, want)
        assert f.pipeline_counters()["records_after_stop"] > c0["records_after_stop"]
        got2 = f.decode_span(len(d1) << 16, ALL, raise_on_error=False)
        assert got2["status"] == rc2
        # (the span's first position is the end of the empty block as well as
        # the start of the next: the oracle names it by the former)
        np.testing.assert_array_equal(got2["key"], want2["key"])
        np.testing.assert_array_equal(got2["voff"][1:], want2["voff"][1:])


@pytest.mark.parametrize("eof_mid", [False, True])
@pytest.mark.parametrize("g", [1, 7, 4096])
def test_indexer_list_overflow_takes_the_separate_launches(g, eof_mid):
    d, _ = synth.make_bam(4000, seed=5)
    s0 = orc.Stream(d)
    u = bytes(s0.data)
    h = s0.header_end
    # the first 1500 records, 40,000 block_size-0 records (160 KB: more than
    # kListCap per 64 KiB block), then the rest
    q, n = h, 0
    while n < 1500:
        q += 4 + struct.unpack_from("<i", u, q)[0]
        n += 1
    payload = u[:q] + b"\0" * (4 * 40000) + u[q:]
    lens = [min(65280, len(payload) - a) for a in range(0, len(payload), 65280)]
    data = orc.bgzf_compress(payload, lens, level=5, eof=True)
    if eof_mid:  # an EOF block mid-file, then records from a block start: the index ends at it
        d2, _ = synth.make_bam(2000, seed=8, eof_block=False)
        s2 = orc.Stream(d2)
        recs = bytes(s2.data)[s2.header_end:]
        data += orc.bgzf_compress(recs, [min(65280, len(recs) - a) for a in range(0, len(recs), 65280)], level=5)
    s = orc.Stream(data)
    want = s.splitting_index(g)
    with hbam.BamFile(data) as f:
        c0 = f.pipeline_counters()
        assert f.splitting_index(g) == want
        assert f.pipeline_counters()["record_fallbacks"] > c0["record_fallbacks"]


def _with_false_start(n=3000, at=(1000,), seed=3):
    """A C2-like BAM whose records `at` each carry, as their last tag (B:c),
    the bytes of another whole record, and a BGZF block that starts exactly
    there: the block's first plausible record start is that embedded copy,
    whose chain runs on into the true next record."""
    d, _ = synth.make_bam(n, seed=seed)
    s0 = orc.Stream(d)
    u = bytes(s0.data)
    h = s0.header_end
    starts, q = [], h
    while q < len(u):
        starts.append(q)
        q += 4 + struct.unpack_from("<i", u, q)[0]
    out, cuts, prev = bytearray(u[:h]), [], h
    for r in sorted(at):
        a, b = starts[r], starts[r + 1]
        donor = u[starts[n - 1 - r]:starts[n - r]] if n - r < len(starts) else u[starts[n - 1 - r]:]
        out += u[prev:a]
        body = bytearray(u[a + 4:b]) + b"XXBc" + struct.pack("<i", len(donor))
        cuts.append(len(out) + 4 + len(body))  # the embedded copy's first byte
        body += donor
        out += struct.pack("<i", len(body)) + body
        prev = b
    out += u[prev:]
    lens, p = [], 0
    for c in cuts + [len(out)]:
        while c - p > 65280:
            lens.append(65280)
            p += 65280
        if c > p:
            lens.append(c - p)
            p = c
    return orc.bgzf_compress(bytes(out), lens, level=5, eof=True)


@pytest.mark.parametrize("at", [(1000,), (700, 1400, 2100)])
def test_false_start_at_a_block_start_is_rewalked(at):
    """(c) the link check's re-walk round: the speculative list bound queued
    with the first link check is discarded and recomputed after it."""
    data = _with_false_start(at=at)
    s = orc.Stream(data)
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 3000
    with hbam.BamFile(data, window_bytes=1 << 30) as f:
        c0, r0 = f.pipeline_counters(), f.chain_counters()["rewalked"]
        got = f.decode_all()
        assert_same_records(got, want)
        c1 = f.pipeline_counters()
        assert c1["link_rewalks"] + c1["link_fallbacks"] > c0["link_rewalks"] + c0["link_fallbacks"]
        # every block that starts with an embedded copy is re-walked from its true entry
        assert f.chain_counters()["rewalked"] >= r0 + len(at)
        st = f.decode_span_device(f.header()["first_record_voff"], ALL)
        assert st["records"] == 3000 and st["status"] == 0
        assert st["first_voff"] == want["voff"][0] and st["last_voff"] == want["voff"][-1]
        assert f.splitting_index(5) == s.splitting_index(5)


@pytest.mark.parametrize("which", ["eof_stop", "false_starts"])
def test_timed_pass_takes_the_edge_paths(which):
    """(d) a timed pass (timing=True) queues nothing ahead of a verdict: the
    inflate is checked at once, the chain end and the list bound follow the
    link check's read-back, and the tail follows k_rec_check_out's.  The
    early stop (a) and the re-walk (c) go through those branches too."""
    from test_gpu_windows import _digest
    data = _with_eof_stop() if which == "eof_stop" else _with_false_start(at=(700, 1400, 2100))
    s = orc.Stream(data)
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 3000
    with hbam.BamFile(data, window_bytes=1 << 30) as f:
        c0, r0 = f.pipeline_counters(), f.chain_counters()["rewalked"]
        st = f.decode_span_device(f.header()["first_record_voff"], ALL, timing=True)
        c1, r1 = f.pipeline_counters(), f.chain_counters()["rewalked"]
        print(which, st, c0, c1, r0, r1)
        assert st["records"] == 3000 and st["status"] == 0
        assert st["first_voff"] == want["voff"][0] and st["last_voff"] == want["voff"][-1]
        assert (st["key_xor"], st["voff_sum"]) == _digest(want)
        if which == "eof_stop":
            assert c1["records_after_stop"] > c0["records_after_stop"]
        else:
            assert c1["link_rewalks"] + c1["link_fallbacks"] > c0["link_rewalks"] + c0["link_fallbacks"]
            assert r1 >= r0 + 3


@pytest.fixture(scope="module")
def long_reads():
    """40 long reads in 4 KiB blocks: every record spans 4.5 to 22 blocks."""
    d, info = synth.make_bam(40, mode="long", block_payload=4096)
    s = orc.Stream(d)
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 40 and info["blocks"] > 400
    return d, s, want


@pytest.mark.parametrize("r", [0, 5, 17, 39])
def test_a_record_past_the_inflated_range_goes_round_again(long_reads, r):
    """(e) the pass inflates the span's blocks and two more; a record that
    needs bytes beyond them (`need` > e_inf) makes it inflate up to the
    record's end and go round again.  [voff[r], voff[r] + 1) holds record r
    alone, which no three blocks hold."""
    d, s, want = long_reads
    v0, vr = int(want["voff"][0]), int(want["voff"][r])
    for vs, n in ((vr, 1), (v0, r + 1)):
        rc, w = s.decode_span(vs, vr + 1)
        assert rc == 0 and len(w["key"]) == n
        with hbam.BamFile(d, window_bytes=1 << 30) as f:
            c0 = f.pipeline_counters()
            assert_same_records(f.decode_span(vs, vr + 1), w)
            launches = f.pipeline_counters()["inflate_launches"] - c0["inflate_launches"]
            print(r, n, "inflate_launches", launches)
            if n == 1:  # the first round's blocks, then the rest of the record's
                assert launches >= 2
            for timing in (False, True):
                st = f.decode_span_device(vs, vr + 1, timing=timing)
                assert st["records"] == n and st["status"] == 0
