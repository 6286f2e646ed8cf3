"""CPU: the restated bounded-traversal filter (tests/query_cases.py) that the
GPU query tests compare against.  The literal per-record loop and the scan
form the kernels compute agree; on coordinate-sorted input both equal a plain
"overlaps any interval" test, on unsorted input they do not (the filter's one
interval index never goes back).  Parity with htsjdk is unpinned: the rules
are restated in include/hbam.h."""
import re

import pytest

import bai
import hbam
import query_cases as q


@pytest.mark.parametrize("iv,kept,stop", q.MAIN_SETS, ids=[str(i) for i in range(len(q.MAIN_SETS))])
def test_loop_scan_and_brute_force_agree_on_sorted_input(iv, kept, stop):
    c = q.main_case()
    assert len(c.table) == 6000 and sum(1 for f in c.records["flag"] if f & 4) == 123
    k, st, _ = q.filter_loop(c.table, iv)
    assert (k, st) == q.filter_scan(c.table, iv)
    assert k == q.overlaps_any(c.table, iv)
    assert len(k) == kept
    if stop != "any":
        assert st == stop


@pytest.mark.parametrize("iv,kept", q.LONG_SETS, ids=["two", "point"])
def test_long_cigar_sets(iv, kept):
    c = q.long_case()
    assert sum(1 for x in c.records["n_cigar"] if x > 32) == 261 and max(c.records["n_cigar"]) == 806
    k, st, _ = q.filter_loop(c.table, iv)
    assert (k, st) == q.filter_scan(c.table, iv)
    assert len(k) == kept and 0 < kept < len(c.table)


@pytest.mark.parametrize("iv,kept,brute", q.UNSORTED_SETS, ids=["open", "closed"])
def test_loop_and_scan_differ_from_brute_force_on_unsorted_input(iv, kept, brute):
    c = q.unsorted_case()
    k, st, _ = q.filter_loop(c.table, iv)
    assert (k, st) == q.filter_scan(c.table, iv)
    assert len(k) == kept and len(q.overlaps_any(c.table, iv)) == brute


def test_every_nonempty_case_keeps_some_records_and_not_all():
    m = q.main_case()
    idx = bai.write_bai(m.data)
    for iv, kept, _ in q.MAIN_SETS:
        if kept == 0:
            continue
        for chunks in (m.whole, q.bai_chunks_for(idx, iv)):
            rc, want, _ = q.query_oracle(m.stream, iv, chunks)
            assert rc == 0 and len(want["voff"]) == kept < len(m.table)
    for case, sets in ((q.long_case(), q.LONG_SETS), (q.unsorted_case(), q.UNSORTED_SETS)):
        for s in sets:
            assert 0 < len(q.filter_loop(case.table, s[0])[0]) < len(case.table)
    # the rewritten cigars move alignment ends both ways
    ops = q.cigar_ops_case()
    assert sum(a[2] > b[2] for a, b in zip(ops.table, m.table)) > 100
    assert sum(a[2] < b[2] for a, b in zip(ops.table, m.table)) > 100
    up = q.unplaced_case()
    rc, want = q.unmapped_oracle(up.stream, up.first)
    assert rc == 0 and len(want["voff"]) == 30 and int(want["voff"][0]) == int(up.records["voff"][5970])


def test_edges_come_from_the_data():
    t = q.main_case().table
    assert t[11] == (1, 8301, 8447)
    assert t[15] == (1, 9501, 9501) and q.main_case().records["flag"][15] & 4


def test_bai_chunks_are_ordered_and_cover_the_interval():
    m = q.main_case()
    idx = bai.write_bai(m.data)
    for iv, _, _ in q.MAIN_SETS:
        ch = q.bai_chunks_for(idx, iv)
        assert all(a <= e for a, e in ch) and all(ch[k][1] <= ch[k + 1][0] for k in range(len(ch) - 1))
        got = q.query_oracle(m.stream, iv, ch)[1]["voff"].tolist()
        assert got == q.query_oracle(m.stream, iv, m.whole)[1]["voff"].tolist()
    assert len({c >> 16 for pair in q.hand_chunks(m) for c in pair}) >= 5
    assert any(a == e for a, e in q.hand_chunks(m))


def test_header_declares_the_query_entry_points():
    declared = set(hbam.exported_symbols_from_header())
    assert {"hbam_query_intervals", "hbam_query_unmapped", "hbam_query_next"} <= declared
    txt = open(hbam.HEADER_PATH).read()
    assert re.search(r"typedef struct hbam_interval \{ int32_t ref_id, start, end; \} hbam_interval;", txt)
    assert "#define HBAM_ABI_VERSION 6" in txt
