"""GPU: the split guesser (k_guess_splits, k_guess_bgzf_starts, k_block_crc and
the host's windows, hbam_guess.hip) against the oracle, point for point, on
the cases of guess_cases.py: read limits at block edges, records the
verification rejects, corrupt and cut blocks, CRC slices, empty blocks, false
BGZF magic in payloads, the chain cases' decoys, and the grouping of points
into host windows.  One batched call per file; the oracle's answers are
computed once per case (guess_cases.want)."""
import io
import random
import time

import pytest

import guess_cases as gc
import hbam

pytestmark = pytest.mark.gpu


def _differences(pts, got, want):
    assert len(got) == len(want) == len(pts)
    return [(p, g, w) for p, g, w in zip(pts, got, want) if g != w]


def _check(name, **open_kw):
    """One batched guess_record_starts over the case's points == the oracle."""
    k = gc.get(name)
    want = gc.want(name)
    begs, ends = gc.begs_ends(k["pts"])
    t0 = time.perf_counter()
    with hbam.BamFile(k["data"], **open_kw) as f:
        got = f.guess_record_starts(begs, ends, k["header_n_ref"])
    dt = time.perf_counter() - t0
    bad = _differences(k["pts"], got, want)
    print(f"guess {name}: {len(got)} points in {dt:.2f} s, {len(bad)} differ"
          + "".join(f"\n  (beg, end) {p}: device {g:#x}, oracle {w:#x}" for p, g, w in bad[:8]))
    assert not bad, f"{len(bad)} of {len(got)} points differ, first (point, device, oracle): {bad[0]}"


def _check_bgzf(name):
    """guess_bgzf_block_starts (k_guess_bgzf_starts shares valid[], find_block
    and the host windows) on the same file at the same begs."""
    k = gc.get(name)
    pts = gc.bgzf_points(k)
    begs, ends = gc.begs_ends(pts)
    with hbam.BamFile(k["data"]) as f:
        got = f.guess_bgzf_block_starts(begs, ends)
    bad = _differences(pts, got, gc.want_bgzf(name))
    assert not bad, f"{len(bad)} of {len(got)} points differ, first (point, device, oracle): {bad[0]}"


@pytest.mark.parametrize("name", gc.FAMILY["A"])
def test_window_edges(name):
    _check(name)


@pytest.mark.parametrize("name", gc.FAMILY["B"])
def test_verification_rejects(name):
    _check(name)


@pytest.mark.parametrize("name", gc.FAMILY["C"])
def test_corrupt_blocks(name):
    _check(name)
    _check_bgzf(name)


@pytest.mark.parametrize("name", gc.FAMILY["D"])
def test_crc_slices(name):
    _check(name)
    _check_bgzf(name)


@pytest.mark.parametrize("name", gc.FAMILY["E"])
def test_empty_blocks(name):
    _check(name)
    _check_bgzf(name)


@pytest.mark.parametrize("name", gc.FAMILY["F"])
def test_false_magic(name):
    _check(name)


@pytest.mark.parametrize("name", gc.FAMILY["G"])
def test_chain_case_decoys(name):
    _check(name)


def _grouping_subset():
    k = gc.get("grouping")
    idx = list(range(0, len(k["pts"]), len(k["pts"]) // 60))[:60]
    return k, idx


@pytest.mark.parametrize("order", ["sorted", "reversed", "shuffled", "one_by_one"])
def test_grouping_and_call_shape(order):
    """window_bytes = 64 KiB puts the host's window cap at its 1 MiB floor, so
    the 2 MB file's points fall into several windows."""
    k = gc.get("grouping")
    want = list(gc.want("grouping"))
    pts = list(k["pts"])
    idx = list(range(len(pts)))
    if order == "reversed":
        idx.reverse()
    elif order == "shuffled":
        random.Random(11).shuffle(idx)
    elif order == "one_by_one":
        idx = _grouping_subset()[1]
    with hbam.BamFile(k["data"], window_bytes=1 << 16) as f:
        if order == "one_by_one":
            got = [f.guess_record_starts([pts[i][0]], [pts[i][1]])[0] for i in idx]
        else:
            got = f.guess_record_starts([pts[i][0] for i in idx], [pts[i][1] for i in idx])
    bad = _differences([pts[i] for i in idx], got, [want[i] for i in idx])
    assert not bad, f"{len(bad)} of {len(got)} points differ, first (point, device, oracle): {bad[0]}"


def test_grouping_through_the_drop_in():
    """hbam.BAMSplitGuesser over an io.BytesIO: positioned reads, the file is never mapped."""
    k, idx = _grouping_subset()
    want = gc.want("grouping")
    with hbam.BAMSplitGuesser(io.BytesIO(k["data"])) as g:
        got = [g.guessNextBAMRecordStart(*k["pts"][i]) for i in idx]
    bad = _differences([k["pts"][i] for i in idx], got, [want[i] for i in idx])
    assert not bad, f"{len(bad)} of {len(got)} points differ, first (point, device, oracle): {bad[0]}"
