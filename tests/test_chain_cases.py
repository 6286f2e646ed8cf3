"""CPU: the record-chain cases of chain_cases.py are what they are named for.

The oracle reads every false-start file as 3000 valid records under STRICT,
and every implausible-record file as 3000 records under SILENT and up to the
first patched record under STRICT.  The restated plausible() / plausible2()
/ guess walk (chain_cases.py) then confirm, per case, the property that sends
the GPU chain down the path the case is meant to reach."""
import pytest

import chain_cases as cc
import orc
from chain_cases import block_guess, block_of, guess_walk, plausible, plausible2, plausible_run, rd32


@pytest.mark.parametrize("name", list(cc.FALSE_START_CASES))
def test_false_start_files_read_as_3000_valid_records(name):
    c = cc.get(name)
    s, rc, want = cc.expected(name, orc.STRICT)
    assert rc == 0 and len(want["key"]) == cc.N
    assert bytes(s.data) == c["u"]
    assert [int(x) for x in want["offset"]] == c["starts"]
    assert [int(x) for x in s.blocks["isize"] if x] == c["lens"]
    assert len(c["u"]) <= 1_300_000
    for d in c["decoys"]:  # a block starts at every decoy, inside its host record
        b0, _ = block_of(c["lens"], d["pos"])
        assert b0 == d["pos"]
        assert c["starts"][d["host"]] < d["pos"] < (c["starts"] + [len(c["u"])])[d["host"] + 1]


@pytest.mark.parametrize("name", list(cc.IMPLAUSIBLE_CASES))
def test_implausible_files_read_whole_under_silent(name):
    c = cc.get(name)
    _, rc, want = cc.expected(name, orc.SILENT)
    assert rc == 0 and len(want["key"]) == cc.N
    _, rc, want = cc.expected(name, orc.STRICT)
    assert rc == 1 and len(want["key"]) == c["patched"][0]
    u, n_ref = c["u"], c["n_ref"]
    for r in c["patched"]:
        assert not plausible(u, c["starts"][r], n_ref)
    # a full-length .splitting-bai: an entry per record, as for the unpatched file
    head, recs, _ = cc.base()
    whole = orc.Stream(orc.bgzf_compress(cc.layout(head, recs)[0], c["lens"], level=5)).splitting_index(1)
    assert len(orc.Stream(c["data"]).splitting_index(1)) == len(whole) > 8 * cc.N


def test_restatement_accepts_every_true_record_start():
    head, recs, n_ref = cc.base()
    u, starts = cc.layout(head, recs)
    assert len(starts) == cc.N and all(plausible2(u, q, n_ref) for q in starts)
    # and under a short inflated range: what cannot be read is not refuted
    e_inf = starts[1500] + 20
    assert all(plausible2(u, q, n_ref, e_inf) == (q + 4 <= e_inf) for q in starts)
    q, n = starts[0], 0
    while q is not None and q < len(u):
        q, n = cc.chain_step(u, q), n + 1
    assert n == cc.N and q == len(u)


def _decoy(c, i=0):
    d = c["decoys"][i]
    return d["pos"], block_of(c["lens"], d["pos"])[1]


def _joins_true_chain(c, q):
    starts = set(c["starts"]) | {len(c["u"])}
    while q not in starts:
        q = cc.chain_step(c["u"], q)
        assert q is not None and q <= len(c["u"])
    return q


@pytest.mark.parametrize("name", ["merge", "merge3", "tail_eof", "tail_noeof"])
def test_merge_decoys_join_the_true_chain(name):
    c = cc.get(name)
    u, n_ref = c["u"], c["n_ref"]
    for i, d in enumerate(c["decoys"]):
        p, bend = _decoy(c, i)
        assert plausible2(u, p, n_ref)
        host_end = (c["starts"] + [len(u)])[d["host"] + 1]
        assert _joins_true_chain(c, p) == host_end  # the host ends right after the donor
        ok, listed, _ = guess_walk(u, p, bend, n_ref)
        assert ok and listed[0] == p
        assert block_guess(u, p, bend, n_ref) [0] == p
    if name.startswith("tail"):
        assert host_end == len(u) and bend == len(u)
        assert (len(orc.Stream(c["data"]).blocks) == len(c["lens"]) + 1) == (name == "tail_eof")


def test_deadend_fails_at_its_third_step_and_a_later_start_walks_clean():
    c = cc.get("deadend")
    u, n_ref = c["u"], c["n_ref"]
    p, bend = _decoy(c)
    assert plausible2(u, p, n_ref)
    inside, beyond, stop = plausible_run(u, p, bend, n_ref)
    assert (inside, beyond) == (2, 0) and stop == c["junk"] < bend
    assert not plausible(u, c["junk"], n_ref) and not guess_walk(u, p, bend, n_ref)[0]
    t = c["starts"][c["decoys"][0]["host"] + 1]
    assert t == c["junk"] + 40 and t < bend
    assert plausible2(u, t, n_ref) and guess_walk(u, t, bend, n_ref)[0]
    assert block_guess(u, p, bend, n_ref) == (t, guess_walk(u, t, bend, n_ref)[2], True)


@pytest.mark.parametrize("k", [3, 4])
def test_lookahead_decoys_stay_plausible_for_exactly_k_records_past_the_block(k):
    c = cc.get(f"look{k}")
    u, n_ref = c["u"], c["n_ref"]
    p, bend = _decoy(c)
    assert bend == c["decoy_block_end"] and plausible2(u, p, n_ref)
    inside, beyond, stop = plausible_run(u, p, bend, n_ref)
    assert (inside, beyond) == (5, k) and not plausible(u, stop, n_ref)
    host = c["decoys"][0]["host"]
    assert c["starts"][host] < p and stop + 40 == c["starts"][host + 1]  # the host covers all of it
    assert guess_walk(u, p, bend, n_ref)[0] == (k == 4)
    # the case sits on the boundary: one record less (more) of lookahead flips it
    assert guess_walk(u, p, bend, n_ref, lookahead=k)[0] and not guess_walk(u, p, bend, n_ref, lookahead=k + 1)[0]
    g, x, searched = block_guess(u, p, bend, n_ref)
    assert (g, x, searched) == ((p, bend, False) if k == 4 else (None, None, True))
    # the block after it starts on the lookahead records and meets the bad head: searched, no guess
    assert block_guess(u, bend, block_of(c["lens"], bend)[1], n_ref)[2]


@pytest.mark.parametrize("name", ["stray_in", "stray_out", "cascade"])
def test_stray_decoys_walk_a_block_inside_their_host(name):
    c = cc.get(name)
    u, n_ref = c["u"], c["n_ref"]
    p, bend = _decoy(c)
    host = c["decoys"][0]["host"]
    h0, h1 = c["starts"][host], c["starts"][host + 1]
    assert bend == c["decoy_block_end"] and h1 == c["host_end"]
    assert h1 - h0 > 3 * cc.BLOCK - 2 and h0 < p and bend < h1  # no true record start in the block
    assert plausible2(u, p, n_ref)
    ok, listed, x = guess_walk(u, p, bend, n_ref)
    assert ok and len(listed) == 8
    assert block_guess(u, p, bend, n_ref) == (p, x, False)
    if name == "stray_in":
        assert x == bend < h1
        assert plausible_run(u, p, bend, n_ref)[:2] == (8, cc.LOOKAHEAD)
    else:
        assert x == c["exit"] > h1 and x in c["starts"]
        i = c["starts"].index(x)
        assert all(plausible(u, q, n_ref) for q in c["starts"][i:i + cc.LOOKAHEAD])
    if name == "cascade":
        blocks = [block_of(c["lens"], d["pos"]) for d in c["decoys"][1:]]
        assert len(blocks) == 8 and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))  # consecutive
        assert h1 < blocks[0][0] and x > blocks[-1][1]
        for d, (b0, b1) in zip(c["decoys"][1:], blocks):
            assert b0 == d["pos"] and plausible2(u, b0, n_ref)
            assert _joins_true_chain(c, b0) == c["starts"][d["host"] + 1] < b1
            assert block_guess(u, b0, b1, n_ref)[0] == b0


def test_shift1_start_one_byte_early_passes_on_fully_inflated_data():
    c = cc.get("shift1")
    u, n_ref, t = c["u"], c["n_ref"], c["t"]
    p, bend = _decoy(c)
    assert p == t - 1 and u[p] == 0 and t in c["starts"]
    assert (rd32(u, t + 4), rd32(u, t + 24)) == (0, 0)
    assert plausible2(u, p, n_ref)  # e_inf == e_true
    assert p + 4 + rd32(u, p) == c["far"] >= bend and c["far"] in c["starts"]
    assert plausible2(u, t, n_ref) and t + 4 + rd32(u, t) < bend
    assert block_guess(u, p, bend, n_ref)[0] == t  # the rescue takes t
    # without the rescue the walk from t - 1 would stand: its exit is a true record start
    assert guess_walk(u, p, bend, n_ref)[0]


def test_decoys_under_a_short_inflated_range():
    """e_inf < e_true: plausible() accepts what it cannot read, so a decoy cut
    short by the inflated range still passes."""
    c = cc.get("look3")
    u, n_ref = c["u"], c["n_ref"]
    p, bend = _decoy(c)
    assert not guess_walk(u, p, bend, n_ref)[0]
    assert guess_walk(u, p, bend, n_ref, e_inf=bend + 20)[0]
    assert plausible(u, bend, n_ref, e_inf=bend + 20) and not plausible(u, bend, n_ref, e_inf=bend + 3)
