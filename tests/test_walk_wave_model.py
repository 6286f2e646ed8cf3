"""CPU: the segmented walk of k_rec_walk_wave (walk_wave_model.py) gives, for
every block, the candidate, verdict, record list and exit of the one-lane
guess walk (chain_cases.guess_walk from k_rec_cand's candidate), at segment
sizes 1024, 4096 (kWalkSeg) and 65536 (one segment: the walk itself), on
fully inflated data and with the inflated range ending inside the file."""
import functools
import struct

import pytest

import chain_cases as cc
import orc
import walk_wave_model as wm
from chain_cases import guess_walk, plausible2, rd32
from hbam import synth

SEGS = (1024, 4096, 65536)


def tiny_record():
    """The shortest record plausible() takes when it can read it: block_size
    33 = 32 + a read name of one NUL (36 bytes is the bound of the unreadable
    case, block_size >= 32)."""
    return struct.pack("<iiiBBHHHiiii", 33, -1, -1, 1, 0, 4680, 0, 4, 0, -1, -1, 0) + b"\0"


@functools.lru_cache(maxsize=None)
def tiny_case():
    """1500 37-byte records between true ones: whole segments of them, 111 starts each."""
    head, recs, n_ref = cc.base()
    recs = list(recs[:200]) + [tiny_record()] * 1500 + list(recs[200:400])
    u, starts = cc.layout(head, recs)
    return cc.finish("tiny", u, starts, n_ref, [])


@functools.lru_cache(maxsize=None)
def probe_decoy_case():
    """A merge decoy (chain_cases) that starts exactly at an interior segment
    start of its block, inside a tag of record 1000: the segment's probe takes
    it, the true chain never reaches it, so the stitch walks that segment
    serially."""
    head, recs, n_ref = cc.base()
    donor, r = recs[2000], 1000
    _, starts = cc.layout(head, recs)
    pay = starts[r] + len(recs[r]) + 8  # where with_tag puts the payload
    b0 = pay // cc.BLOCK * cc.BLOCK
    pad = -(pay - b0) % wm.SEG
    assert pay + pad + len(donor) < b0 + cc.BLOCK
    recs = list(recs)
    recs[r], off = cc.with_tag(recs[r], cc.filler(pad, 5) + donor)
    u, starts = cc.layout(head, recs)
    assert starts[r] + off == pay and starts[r + 1] == pay + pad + len(donor)
    return cc.finish("probe_decoy", u, starts, n_ref, [], [dict(pos=pay + pad, host=r)])


@functools.lru_cache(maxsize=None)
def synth_case(n, mode):
    d, _ = synth.make_bam(n, mode=mode, seed=11)
    s = orc.Stream(d)
    return dict(name=f"{mode}{n}", u=bytes(s.data), n_ref=s.n_ref, lens=[int(x) for x in s.blocks["isize"] if x],
                data=d)


def _case(name):
    if name == "tiny":
        return tiny_case()
    if name == "probe_decoy":
        return probe_decoy_case()
    if name == "short3000":
        return synth_case(3000, "short")
    if name == "long40":
        return synth_case(40, "long")
    return cc.get(name)


def _blocks(lens):
    p = 0
    for n in lens:
        yield p, p + n
        p += n


def _check(c, seg, e_inf=None):
    """Every block of c: model == one-lane walk.  Returns (walker pieces, serial pieces)."""
    u, n_ref = c["u"], c["n_ref"]
    pre = wm.prefilter_mask(u, n_ref, e_inf)
    taken = serial = 0
    for b0, bend in _blocks(c["lens"]):
        if e_inf is not None and bend > e_inf:  # not inflated: not walked
            break
        cand, ok, listed, x, t, s = wm.block_walk_wave(u, pre, b0, bend, n_ref, e_inf, seg)
        # the candidate: the first plausible2 start of the block, then the shift rule
        first = wm.first_start(u, pre, b0, bend, n_ref, e_inf)
        if first is None:
            assert cand is None
            continue
        assert cand in (first, first + 1, first + 2, first + 3)
        if cand != first:
            assert first + 4 + rd32(u, first) >= bend and plausible2(u, cand, n_ref, e_inf)
        # chain_cases' own restatement of k_rec_cand + walk + search, which shares no code with the model
        g, gx, searched = cc.block_guess(u, b0, bend, n_ref, e_inf)
        if not searched:
            assert ok and (cand, x) == (g, gx), (c["name"], b0)
        else:
            assert not ok, (c["name"], b0)
        want_ok, want_list, want_x = guess_walk(u, cand, bend, n_ref, e_inf)
        assert ok == want_ok, (c["name"], b0)
        if ok:
            assert listed == want_list and x == want_x, (c["name"], b0)
        taken += t
        serial += s
    return taken, serial


ALL_CASES = list(cc.FALSE_START_CASES) + list(cc.IMPLAUSIBLE_CASES) + ["short3000", "long40", "tiny", "probe_decoy"]


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("name", ALL_CASES)
def test_model_matches_the_one_lane_walk(name, seg):
    c = _case(name)
    taken, serial = _check(c, seg)
    if seg == 65536:
        assert serial == 0  # one segment, one walker: the walk itself


@pytest.mark.parametrize("name", ["merge", "look3", "six", "short3000", "long40", "probe_decoy"])
def test_model_matches_under_a_short_inflated_range(name):
    """e_inf < e_true: records past the inflated range are plausible unread."""
    c = _case(name)
    ends = [e for _, e in _blocks(c["lens"])]
    for e_inf in {ends[len(ends) // 2], ends[len(ends) // 2] + 20, ends[-2] + 3}:
        _check(c, wm.SEG, e_inf)


def test_short_reads_are_walked_by_the_segment_walkers():
    c = _case("short3000")
    taken, serial = _check(c, wm.SEG)
    nseg = sum((e - b + wm.SEG - 1) // wm.SEG for b, e in _blocks(c["lens"]))
    assert serial == 0 and taken >= nseg - len(c["lens"])  # (a block's first segment may hold no start past c)


def test_long_reads_land_in_segments_without_a_start():
    c = _case("long40")
    u, n_ref = c["u"], c["n_ref"]
    pre = wm.prefilter_mask(u, n_ref)
    got = [wm.block_walk_wave(u, pre, b0, bend, n_ref) for b0, bend in _blocks(c["lens"])]
    assert max(len(g[2]) for g in got) <= 4  # records of several segments each
    # a record ends where no probe window looked: the stitch walks on serially
    assert sum(g[5] for g in got) >= len(got) // 2


def test_probe_decoy_is_rejected_by_the_stitch():
    c = _case("probe_decoy")
    u, n_ref, d = c["u"], c["n_ref"], c["decoys"][0]["pos"]
    b0, bend = cc.block_of(c["lens"], d)
    assert (d - b0) % wm.SEG == 0 and d > b0 and plausible2(u, d, n_ref)
    pre = wm.prefilter_mask(u, n_ref)
    assert wm.first_start(u, pre, d, d + wm.PROBE, n_ref) == d
    cand, ok, listed, x, taken, serial = wm.block_walk_wave(u, pre, b0, bend, n_ref)
    assert ok and d not in listed and serial >= 1 and taken >= 10
    assert set(listed) == {q for q in c["starts"] if cand <= q < bend}


def test_tiny_records_fill_a_segment_within_the_list_bound():
    c = _case("tiny")
    u, n_ref = c["u"], c["n_ref"]
    pre = wm.prefilter_mask(u, n_ref)
    most = 0
    for b0, bend in _blocks(c["lens"]):
        cand, ok, listed, x, _, _ = wm.block_walk_wave(u, pre, b0, bend, n_ref)
        assert ok
        for j in range((bend - b0 + wm.SEG - 1) // wm.SEG):
            most = max(most, sum(b0 + j * wm.SEG <= q < b0 + (j + 1) * wm.SEG for q in listed))
    assert most == (wm.SEG + 36) // 37 == 111 < 128
