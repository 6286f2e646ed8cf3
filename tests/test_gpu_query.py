"""GPU: bounded traversal (hbam_query_intervals / hbam_query_unmapped /
hbam_query_next; BAMRecordReader.java:170-178) against the restated filter of
tests/query_cases.py: every column, the rest bytes and the voffs of every kept
record, with the default window and with 64 KiB windows (many windows per
chunk: the filter's carry from window to window is what is tested there)."""
import struct

import numpy as np
import pytest

import bai
import hbam
import orc
import query_cases as q
from bam_patch import recompress

pytestmark = pytest.mark.gpu
WINDOWS = [0, 65536]


def assert_query(got, want, u):
    """Every kept record: the 14 fixed columns, rest_off (the rests lie back
    to back from 0) and the rest bytes."""
    n = len(want["voff"])
    assert len(got["voff"]) == n
    for f in q.FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    off = np.concatenate([[0], np.cumsum(want["rest_len"].astype(np.uint64))]).astype(np.uint64)
    np.testing.assert_array_equal(got["rest_off"], off[:-1], err_msg="rest_off")
    assert got["data"] == q.expected_rests(u, want)


def run_query(f, intervals, chunks, max_records=0, raise_on_error=True):
    """The whole query in batches of max_records: (status, concatenated dict, batches)."""
    f.query_intervals(intervals, q.flat(chunks))
    return drain(f, max_records, raise_on_error)


def drain(f, max_records=0, raise_on_error=True):
    parts, status = [], 0
    while True:
        r = f.query_next(max_records, raise_on_error)
        status = r["status"]
        if len(r["voff"]):
            base = sum(len(p["data"]) for p in parts)
            r["rest_off"] = r["rest_off"] + np.uint64(base)
            parts.append(r)
        if status != 0 or not len(r["voff"]) or max_records == 0:
            break
    out = {k: np.concatenate([p[k] for p in parts]) if parts else r[k] for k in r if k not in ("data", "status",
                                                                                                "next_voff")}
    out["data"] = b"".join(p["data"] for p in parts)
    return status, out, len(parts)


@pytest.fixture(scope="module")
def main_files():
    fs = {w: hbam.BamFile(q.main_case().data, window_bytes=w) for w in WINDOWS}
    yield fs
    for f in fs.values():
        f.close()


@pytest.fixture(scope="module")
def main_bai():
    return bai.write_bai(q.main_case().data)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("chunks", ["whole", "bai", "hand"])
@pytest.mark.parametrize("k", range(len(q.MAIN_SETS)))
def test_interval_sets(main_files, main_bai, k, chunks, window):
    c = q.main_case()
    iv, kept, _ = q.MAIN_SETS[k]
    ch = {"whole": c.whole, "bai": q.bai_chunks_for(main_bai, iv), "hand": q.hand_chunks(c)}[chunks]
    rc, want, _ = q.query_oracle(c.stream, iv, ch)
    assert rc == 0
    if chunks != "hand":
        assert len(want["voff"]) == kept
    status, got, _ = run_query(main_files[window], iv, ch)
    assert status == 0
    assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_edges_of_a_record_and_of_a_placed_unmapped_read(main_files, window):
    c = q.main_case()
    assert c.table[11] == (1, 8301, 8447) and c.table[15] == (1, 9501, 9501)
    f = main_files[window]
    for iv, keeps in (((1, 8447, 8447), 11), ((1, 8301, 8301), 11), ((1, 8448, 8448), None),
                      ((1, 8300, 8300), None), ((1, 9501, 9501), 15), ((1, 9502, 9502), None)):
        rc, want, _ = q.query_oracle(c.stream, [iv], c.whole)
        voffs = [int(v) for v in want["voff"]]
        if keeps is None:
            assert int(c.records["voff"][11]) not in voffs and int(c.records["voff"][15]) not in voffs
        else:
            assert int(c.records["voff"][keeps]) in voffs
        status, got, _ = run_query(f, [iv], c.whole)
        assert status == 0
        assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("max_records", [1, 7, 64, 1000, 0])
def test_batching_gives_the_same_concatenation(main_files, max_records, window):
    c = q.main_case()
    iv = q.MAIN_SETS[1][0]
    rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
    n = len(want["voff"])
    status, got, batches = run_query(main_files[window], iv, c.whole, max_records)
    assert status == 0
    assert_query(got, want, c.u)
    if max_records == 0:
        assert batches == 1
    elif window == 0:
        # one window holds the file: its kept records are cut every max_records
        # (2010 at 1000: two full slices and one of 10)
        assert batches == -(-n // max_records)
    else:
        assert batches >= -(-n // max_records)


@pytest.mark.parametrize("window", WINDOWS)
def test_scan_query_counts(main_files, window):
    c = q.main_case()
    iv = q.MAIN_SETS[1][0]
    rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
    f = main_files[window]
    f.query_intervals(iv, q.flat(c.whole))
    n, batches, nbytes = f.scan_query(1000)
    assert (n, nbytes) == (len(want["voff"]), int(want["rest_len"].sum()))
    assert batches == 3 if window == 0 else batches >= 3
    assert f.scan_query(1000) == (0, 0, 0)  # the end stays the end


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("cap", [150_000, 1])
def test_bounded_query_batches_cap_their_rest_bytes(monkeypatch, cap, window):
    """As a split's bounded batches (tests/test_gpu_windows.py): a query batch
    ends before its rests pass the cap (2 GiB; HBAM_MAX_BATCH_BYTES lowers it
    here), one record at least.  Long reads reach 150 KB every few records."""
    c = q.long_case()
    iv = q.LONG_SETS[0][0]
    rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
    monkeypatch.setenv("HBAM_MAX_BATCH_BYTES", str(cap))
    with hbam.BamFile(c.data, window_bytes=window) as f:
        f.query_intervals(iv, q.flat(c.whole))
        parts = []
        while True:
            r = f.query_next(1 << 20)
            if not len(r["voff"]):
                break
            assert r["status"] == 0 and (len(r["data"]) <= cap or len(r["voff"]) == 1)
            parts.append(r)
    if cap == 1:
        assert [len(p["voff"]) for p in parts] == [1] * len(want["voff"])
    else:
        assert len(parts) > 4
        if window == 0:  # (a batch holds records of one window; small windows hold few long reads)
            assert any(len(p["voff"]) > 1 for p in parts)
    base = 0
    for p in parts:
        p["rest_off"] = p["rest_off"] + np.uint64(base)
        base += len(p["data"])
    got = {k: np.concatenate([p[k] for p in parts]) for k in q.FIELDS + ("rest_off",)}
    got["data"] = b"".join(p["data"] for p in parts)
    assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_all_that_remain_after_bounded_batches(main_files, window):
    c = q.main_case()
    iv = q.MAIN_SETS[1][0]
    rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
    f = main_files[window]
    f.query_intervals(iv, q.flat(c.whole))
    parts = [f.query_next(7), f.query_next(64), f.query_next(0), f.query_next(0), f.query_next(5)]
    # (a bounded batch holds records of one window: it may be shorter than asked)
    assert len(parts[0]["voff"]) == 7 and 0 < len(parts[1]["voff"]) <= 64
    if window == 0:
        assert len(parts[1]["voff"]) == 64
    assert len(parts[2]["voff"]) > 64 and len(parts[3]["voff"]) == len(parts[4]["voff"]) == 0
    base = 0
    for p in parts:
        p["rest_off"] = p["rest_off"] + np.uint64(base)
        base += len(p["data"])
    got = {k: np.concatenate([p[k] for p in parts]) for k in q.FIELDS + ("rest_off",)}
    got["data"] = b"".join(p["data"] for p in parts)
    assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_every_cigar_operator_counts(window):
    """D, N, = and X lengthen the span, P and H (like I and S) do not."""
    c, m = q.cigar_ops_case(), q.main_case()
    longer = next(i for i, (a, b) in enumerate(zip(c.table, m.table)) if a[2] > b[2] and a[0] == 1)
    shorter = next(i for i, (a, b) in enumerate(zip(c.table, m.table)) if a[2] < b[2] and a[0] == 4)
    with hbam.BamFile(c.data, window_bytes=window, stringency=hbam.SILENT) as f:
        for iv, i, keeps in (([(1, c.table[longer][2], c.table[longer][2])], longer, True),
                             ([(4, m.table[shorter][2], m.table[shorter][2])], shorter, False),
                             ([(1, 5000, 9999), (4, 100000, 100900), (7, 2000000, 2000100)], None, None)):
            rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
            if i is None:
                assert 0 < len(want["voff"]) < len(c.table)
            else:
                assert (int(c.records["voff"][i]) in [int(v) for v in want["voff"]]) == keeps
            status, got, _ = run_query(f, iv, c.whole)
            assert status == 0
            assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_long_cigars_take_the_wave_path(window):
    c = q.long_case()
    assert sum(1 for x in c.records["n_cigar"] if x > 32) == 261
    with hbam.BamFile(c.data, window_bytes=window) as f:
        for iv, kept in q.LONG_SETS:
            rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
            assert rc == 0 and len(want["voff"]) == kept
            status, got, _ = run_query(f, iv, c.whole)
            assert status == 0
            assert_query(got, want, c.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_unsorted_input_follows_the_single_interval_index(window):
    c = q.unsorted_case()
    with hbam.BamFile(c.data, window_bytes=window) as f:
        for iv, kept, brute in q.UNSORTED_SETS:
            rc, want, _ = q.query_oracle(c.stream, iv, c.whole)
            assert len(want["voff"]) == kept != brute
            status, got, _ = run_query(f, iv, c.whole)
            assert status == 0
            assert_query(got, want, c.u)


def _corrupt(case, i):
    """Record i with a wrong bin: a STRICT-only error (as tests/test_strict.py)."""
    u = bytearray(case.u)
    struct.pack_into("<H", u, int(case.records["offset"][i]) + 14, 1)
    return recompress(case.stream, bytes(u))


@pytest.mark.parametrize("window", WINDOWS)
def test_a_failing_record_counts_only_before_the_stop(window):
    c = q.main_case()
    iv = [(1, 5000, 9999)]  # stops at record 17
    for bad_at, fails in ((3000, False), (18, False), (10, True), (17, True)):
        bad = _corrupt(c, bad_at)
        s = orc.Stream(bad, stringency=orc.STRICT)
        rc, want, stopped = q.query_oracle(s, iv, c.whole)
        assert (rc == hbam.E_FORMAT) == fails and stopped != fails
        with hbam.BamFile(bad, window_bytes=window) as f:
            status, got, _ = run_query(f, iv, c.whole, raise_on_error=False)
            assert status == rc
            assert_query(got, want, s.data)
            if fails:
                with pytest.raises(hbam.HbamError) as e:
                    run_query(f, iv, c.whole)
                assert e.value.code == hbam.E_FORMAT
    # bounded batches: the status comes with the last records before the failure
    bad = _corrupt(c, 10)
    with hbam.BamFile(bad, window_bytes=window) as f:
        f.query_intervals(iv, q.flat(c.whole))
        a = f.query_next(4, raise_on_error=False)
        b = f.query_next(1000, raise_on_error=False)
        assert (len(a["voff"]), a["status"], len(b["voff"]), b["status"]) == (4, 0, 6, hbam.E_FORMAT)
    # a failing record in a chunk after the one the iteration stopped in is never read
    hand = q.hand_chunks(c)
    bad = _corrupt(c, 5000)
    with hbam.BamFile(bad, window_bytes=window) as f:
        status, got, _ = run_query(f, iv, hand)
        assert status == 0 and len(got["voff"]) == 17


def test_no_window_follows_a_stop():
    c = q.main_case()
    with hbam.BamFile(c.data, window_bytes=65536) as f:
        before = f.bytes_read()
        status, got, _ = run_query(f, [(1, 5000, 9999)], c.whole)
        assert status == 0 and len(got["voff"]) == 17
        assert f.bytes_read() - before < len(c.data) // 2
        assert f.bytes_read() < len(c.data) // 2


@pytest.mark.parametrize("window", WINDOWS)
def test_unmapped_only(window):
    c = q.unplaced_case()
    lin = [e for e in bai.linear_index(bai.write_bai(c.data)) if e]
    starts = [lin[-1][-1], c.first]
    assert c.first < starts[0] <= int(c.records["voff"][5970])
    with hbam.BamFile(c.data, window_bytes=window) as f:
        for start in starts:
            rc, want = q.unmapped_oracle(c.stream, start)
            assert rc == 0 and len(want["voff"]) == 30
            f.query_unmapped(start)
            status, got, _ = drain(f, 0)
            assert status == 0
            assert_query(got, want, c.u)
        f.query_unmapped(c.first)
        status, got, batches = drain(f, 7)
        assert status == 0 and batches >= 5
        assert_query(got, want, c.u)


def test_unmapped_only_with_no_unplaced_read(main_files):
    c = q.main_case()
    for f in main_files.values():
        f.query_unmapped(c.first)
        r = f.query_all()
        assert r["status"] == 0 and len(r["voff"]) == 0 and r["data"] == b""


def test_arguments_and_state(main_files):
    c = q.main_case()
    f = main_files[0]
    whole = q.flat(c.whole)
    for iv, ptrs in (([(1, 100, 200), (1, 150, 300)], whole),      # overlapping
                     ([(1, 100, 200), (1, 200, 300)], whole),      # start not past the previous end
                     ([(1, 100, 0), (1, 5000, 6000)], whole),      # the first runs to the end of the reference
                     ([(4, 1, 10), (1, 1, 10)], whole),            # unsorted
                     ([(1, 300, 400), (1, 100, 200)], whole),
                     ([(1, 100, 50)], whole),                      # ends more than one base before its start
                     ([(1, 10, 20), (1, 100, 98)], whole),
                     ([(1, 1, 10)], whole + [whole[0]]),           # odd n_ptrs
                     ([(1, 1, 10)], [whole[1], whole[0]]),         # a chunk that ends before it starts
                     ([(1, 1, 10)], [whole[0] + 5, whole[1], whole[0], whole[0] + 5])):  # descending chunks
        with pytest.raises(hbam.HbamError) as e:
            f.query_intervals(iv, ptrs)
        assert e.value.code == hbam.E_ARG, (iv, ptrs)
    with hbam.BamFile(c.data) as g:
        with pytest.raises(hbam.HbamError) as e:
            g.query_next()
        assert e.value.code == hbam.E_STATE
        first = g.decode_span(c.first, hbam_all(), max_records=0)
        some = g.decode_span(c.first, hbam_all(), max_records=100)
        status, got, _ = run_query(g, q.MAIN_SETS[1][0], c.whole, 64)
        assert status == 0 and len(got["voff"]) == 2010
        for call in (g.encode_writables, lambda: g.reader_position(0)):
            with pytest.raises(hbam.HbamError) as e:
                call()
            assert e.value.code == hbam.E_STATE
        # a call that moves the ctx's window ends the query (include/hbam.h) ...
        g.query_intervals(q.MAIN_SETS[3][0], whole)
        assert len(g.query_next(5)["voff"]) == 5
        assert g.header()["n_ref"] > 7 and g.bytes_read() > 0  # ... these leave it open
        assert len(g.query_next(5)["voff"]) == 5
        g.prefetch(0, 65536)
        with pytest.raises(hbam.HbamError) as e:
            g.query_next(5)
        assert e.value.code == hbam.E_STATE
        # a split read ends the query and is not disturbed by it
        g.query_intervals(q.MAIN_SETS[3][0], whole)
        assert len(g.query_next(5)["voff"]) == 5
        again = g.decode_span(c.first, hbam_all(), max_records=0)
        some2 = g.decode_span(c.first, hbam_all(), max_records=100)
        for k in first:
            assert np.array_equal(first[k], again[k]) if k != "data" else first[k] == again[k], k
            assert np.array_equal(some[k], some2[k]) if k != "data" else some[k] == some2[k], k
        assert len(g.encode_writables()[1]) == 101
        with pytest.raises(hbam.HbamError) as e:
            g.query_next()
        assert e.value.code == hbam.E_STATE
    # no interval: the first record already ends the iteration
    f.query_intervals([], whole)
    assert len(f.query_all()["voff"]) == 0
    # no chunk: nothing to read
    f.query_intervals([(1, 1, 0)], [])
    assert len(f.query_all()["voff"]) == 0


def hbam_all():
    return (1 << 64) - 1
