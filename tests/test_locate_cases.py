"""CPU: the anchored locate's model (locate_cases.model) takes, on every case
and at every segment size, the path the case is meant to reach, and whenever
it accepts, its table is the oracle's block table.  No GPU."""
import numpy as np
import pytest

import locate_cases as lc
import orc

CASES = lc.cases()


def _run(case, S, lo=0, hi=None, partial=False):
    hi = len(case.data) if hi is None else hi
    return lc.model(case.data, lo, hi, partial, S, lc.library_cap(hi - lo, case.cap_limit))


def _oracle_blocks(data, bam):
    return orc.Stream(data, parse_header=bam).blocks


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_reach_their_paths(case):
    assert _run(case, 0) == ("scan", None)
    for S in lc.SIZES:
        path, what = _run(case, S)
        want = case.expect[S]
        if want == "anchored":
            assert path == "anchored", (S, what)
        else:
            assert path == "declined" and want in what, (S, path, what if path == "declined" else None)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_accepted_tables_are_the_oracles(case):
    if not any(case.expect[S] == "anchored" for S in lc.SIZES):  # (the oracle may refuse such a file's framing)
        assert all(_run(case, S)[0] == "declined" for S in lc.SIZES)
        return
    want = _oracle_blocks(case.data, case.bam)
    assert [int(x) for x in want["coff"]] == lc.block_starts(case.data)
    if case.bam:
        r, _ = orc.scan(case.data)
        assert r["rc"] == 0 and r["blocks"] == len(want)
    accepted = 0
    for S in lc.SIZES:
        path, table = _run(case, S)
        if path == "anchored":
            accepted += 1
            np.testing.assert_array_equal(np.array(table, np.uint64), want["coff"])
    assert accepted == sum(1 for S in lc.SIZES if case.expect[S] == "anchored")


def test_a_range_from_the_third_block():
    data = lc.test_bam()
    starts = lc.block_starts(data)
    for S in lc.SIZES:
        assert lc.model(data, starts[2], len(data), False, S, 1 << 20) == ("anchored", starts[2:])


def test_segments_without_a_block_start():
    """max_blocks at S = 4 KiB: runs of fifteen empty segments, as intended."""
    case = next(c for c in CASES if c.name == "max_blocks")
    starts = np.array(lc.block_starts(case.data))
    nseg = (len(case.data) + lc.S_SMALL - 1) // lc.S_SMALL
    has = np.zeros(nseg, bool)
    has[starts // lc.S_SMALL] = True
    runs = "".join("x" if h else "." for h in has).split("x")
    assert sum(1 for r in runs if len(r) == 15) >= 3


def test_boundary_case_hits_the_boundaries():
    case = next(c for c in CASES if c.name == "boundary")
    starts = set(lc.block_starts(case.data))
    assert {65536, 2 * 65536 - 1, 3 * 65536 + 1} <= starts
    assert 2 * 65536 not in starts and 3 * 65536 not in starts


def test_empty_run_makes_a_large_count():
    case = next(c for c in CASES if c.name == "empty_run")
    starts = lc.block_starts(case.data)
    isz = [int.from_bytes(case.data[p + 24:p + 28], "little") if case.data[p + 16] == 27 else 1 for p in starts]
    assert sum(1 for x in isz if x == 0) == 201 and len(starts) > 64  # (the run and the EOF block)
    assert len(starts) <= lc.library_cap(len(case.data))


def test_truncated_file_declines_unless_partial():
    """Cut mid-block: without `partial` every size declines (tail); a partial
    range that the cut block ends is accepted with that block as its last
    candidate; windows of 64 KiB before the cut are accepted."""
    data = lc.truncated()
    whole = lc.block_starts(lc.Builder(lc.bam_stream()).finish())
    kept = [p for p in whole if p < len(data)]
    assert kept[-1] + 5000 == len(data) and len(data) > 65536
    for S in lc.SIZES:
        path, what = lc.model(data, 0, len(data), False, S, 1 << 20)
        assert path == "declined" and "tail" in what
        assert lc.model(data, 0, len(data), True, S, 1 << 20) == ("anchored", kept)
        path, table = lc.model(data, 0, 65536, True, S, 1 << 20)
        assert path == "anchored" and table == [p for p in kept if p < 65536]


def test_windowed_ranges_are_accepted():
    """A file read in 64 KiB ranges, each from the block the last one cut."""
    data = lc.windowed()
    want = lc.block_starts(data)
    assert len(data) > 3 * 65536
    for S in lc.SIZES:
        lo, got = 0, []
        while lo < len(data):
            hi = min(lo + 65536, len(data))
            path, table = lc.model(data, lo, hi, hi < len(data), S, 1 << 20)
            assert path == "anchored"
            cut = table[-1] + lc.header_at(data, table[-1], hi) > hi
            got += table[:-1] if cut else table
            lo = table[-1] if cut else hi
        assert got == want
