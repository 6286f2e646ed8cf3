"""GPU: the walk stage as one wave per block (k_rec_walk_wave, the default)
against the same stage as k_rec_cand + one lane per block
(HBAM_CHAIN_WALK=lane).  Each input is decoded once either way, each in its
own context opened with HBAM_CHAIN_KEEP_WALK=1, and the two must agree in
  the walk stage's g, x, wcnt and lists (hbam_chain_lists), array for array;
  the chain_counters() and pipeline_counters() deltas (the same paths taken);
  the device decode's counts and digests, and the decoded columns.
The inputs are the smallest that reach each branch of the kernel; the CPU
model of the stitch (walk_wave_model.py) names them."""
import functools
import os

import numpy as np
import pytest

import chain_cases as cc
import hbam
import orc
from test_gpu_chain import WINDOWS
from test_gpu_parity import FIELDS
from test_walk_wave_model import probe_decoy_case, synth_case, tiny_case

pytestmark = pytest.mark.gpu
ALL = (1 << 64) - 1


def _one_way(data, lane, window, stringency, vstart, vend):
    keep = {k: os.environ.get(k) for k in ("HBAM_CHAIN_WALK", "HBAM_CHAIN_KEEP_WALK")}
    os.environ["HBAM_CHAIN_KEEP_WALK"] = "1"
    if lane:
        os.environ["HBAM_CHAIN_WALK"] = "lane"
    else:
        os.environ.pop("HBAM_CHAIN_WALK", None)
    try:
        with hbam.BamFile(data, window_bytes=window, stringency=stringency) as f:  # (the knobs are read at the open)
            v0 = f.header()["first_record_voff"] if vstart is None else vstart
            c0, p0 = f.chain_counters(), f.pipeline_counters()
            try:
                st = f.decode_span_device(v0, vend)
                st = {k: v for k, v in st.items() if not k.startswith("ms_")}
            except hbam.HbamError as e:
                st = {"error": e.code}
            lists = f.chain_lists()
            c1, p1 = f.chain_counters(), f.pipeline_counters()
            got = f.decode_span(v0, vend, raise_on_error=False)
            cols = {k: np.array(got[k]) for k in FIELDS}
            cols["status"] = got["status"]
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    delta = {k: c1[k] - c0[k] for k in c1}
    delta.update({k: p1[k] - p0[k] for k in p1})
    return lists, delta, st, cols


def _same_both_ways(data, window=1 << 30, stringency=hbam.STRICT, vstart=None, vend=ALL):
    lane = _one_way(data, True, window, stringency, vstart, vend)
    wave = _one_way(data, False, window, stringency, vstart, vend)
    assert len(wave[0]["g"]) == len(lane[0]["g"]) > 0
    assert (wave[0]["stage"], lane[0]["stage"]) == (5, 4)  # kStageWalk, kStageWalkLane: two different launches
    for k in ("g", "x", "wcnt", "list"):
        np.testing.assert_array_equal(wave[0][k], lane[0][k], err_msg=k)
    assert wave[1] == lane[1]
    assert wave[2] == lane[2]
    for k in FIELDS:
        np.testing.assert_array_equal(wave[3][k], lane[3][k], err_msg=k)
    assert wave[3]["status"] == lane[3]["status"]
    return wave


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(cc.FALSE_START_CASES) + list(cc.IMPLAUSIBLE_CASES))
def test_chain_cases_walk_the_same(name, window):
    """(a small window: e_inf < e_true, records plausible unread)"""
    stringency = hbam.SILENT if name in cc.IMPLAUSIBLE_CASES else hbam.STRICT  # (SILENT reads the whole file)
    _same_both_ways(cc.get(name)["data"], window, stringency)


@pytest.mark.parametrize("window", WINDOWS)
def test_short_reads_walk_the_same(window):
    lists, _, st, _ = _same_both_ways(synth_case(3000, "short")["data"], window)
    assert st["records"] == 3000


@pytest.mark.parametrize("window", WINDOWS)
def test_long_reads_walk_the_same(window):
    """Records of several segments each, some longer than a block: most
    segments hold no start, and the stitch walks on serially where one ends."""
    lists, _, st, _ = _same_both_ways(synth_case(40, "long")["data"], window)
    assert st["records"] == 40


def test_span_from_mid_block_walks_the_same():
    """The span's first block is walked from p0 by block_size (the p0 branch)."""
    data = synth_case(3000, "short")["data"]
    rc, want = orc.Stream(data).decode_all()
    assert rc == 0
    for r in (1500, 2999):
        lists, _, st, _ = _same_both_ways(data, vstart=int(want["voff"][r]))
        assert st["records"] == 3000 - r and lists["g"][0] != ALL


@functools.lru_cache(maxsize=None)
def _empty_block_and_short_tail():
    """The base file with an empty BGZF block after its third block and a last
    block of 1000 bytes (shorter than one segment)."""
    head, recs, _ = cc.base()
    u, _ = cc.layout(head, recs)
    cut = 3 * cc.BLOCK
    tail = cc.cut_lens(len(u) - cut, [len(u) - cut - 1000])
    assert tail[-1] == 1000
    return (orc.bgzf_compress(u[:cut], [cc.BLOCK] * 3, level=5, eof=True) +
            orc.bgzf_compress(u[cut:], tail, level=5, eof=True))


@pytest.mark.parametrize("stringency", [hbam.STRICT, hbam.SILENT])
def test_empty_block_and_short_last_block_walk_the_same(stringency):
    lists, _, _, _ = _same_both_ways(_empty_block_and_short_tail(), stringency=stringency)
    assert len(lists["g"]) >= 5


def test_false_start_in_a_probe_window_walks_the_same():
    """A decoy at an interior segment's start: its walker is off the chain."""
    c = probe_decoy_case()
    lists, delta, st, _ = _same_both_ways(c["data"])
    assert st["records"] == cc.N and delta["rewalked"] == 0 and delta["searched"] == 0


def test_shortest_records_fill_a_segment_and_walk_the_same():
    """111 starts in a segment, 128 entries in a walker's row."""
    c = tiny_case()
    lists, _, st, _ = _same_both_ways(c["data"], stringency=hbam.SILENT)
    assert st["records"] == len(c["starts"])
    assert int((lists["wcnt"] & 0x7FFFFFFF).max()) > 700  # (the 1500 lie in two blocks at the most)
