"""CPU: the guesser cases of guess_cases.py are what they are named for, by the
oracle alone, and the oracle reports no error at any point of any case."""
import bisect
import struct

import pytest

import chain_cases as cc
import guess_cases as gc
import orc


def upos(k, answers, ref=None):
    """Answers as positions in the inflated stream (None for `end`), so that
    files whose blocks compress to other sizes can be compared point by point.
    ref: the file whose block table applies (a damaged file's intact twin)."""
    ref = ref if ref is not None else (k["intact"] if k["intact"] is not None else k["data"])
    c = gc.block_offsets(ref)
    ustart = [0]
    for a, b in zip(c, c[1:]):
        ustart.append(ustart[-1] + struct.unpack_from("<I", ref, b - 4)[0])
    out = []
    for (beg, end), v in zip(k["pts"], answers):
        if v == end:
            out.append(None)
            continue
        j = bisect.bisect_left(c, v >> 16)
        assert c[j] == v >> 16, "a guess names a block start"
        out.append(ustart[j] + (v & 0xffff))
    return out


def moved(a, b):
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_oracle_answers_every_point(name):
    k = gc.get(name)
    got = gc.want(name)  # (an oracle error raises)
    assert len(got) == len(k["pts"]) > 0
    assert all(0 < b <= e for b, e in k["pts"])
    upos(k, got)  # every answer is `end` or names a block of the file
    if name in gc.FAMILY["C"] + gc.FAMILY["D"] + gc.FAMILY["E"]:  # (the BGZF guesser runs on these too)
        c = set(gc.block_offsets(k["intact"] if k["intact"] is not None else k["data"]))
        assert all(v == e or v in c for (b, e), v in zip(gc.bgzf_points(k), gc.want_bgzf(name)))


def test_orc_file_argument():
    data = gc.base4096()[0]
    s = orc.Stream(data)
    c = gc.block_offsets(data)
    pts = [(c[5], c[5] + gc.MAX), (c[9] - 1, c[12] + 17)]
    for b, e in pts:
        assert s.guess_record_start(b, e, file=data) == s.guess_record_start(b, e)
        assert s.guess_record_start(b, e, 1, file=data) == s.guess_record_start(b, e, 1)
    with pytest.raises(ValueError):
        s.guess_record_start(c[5], c[6], file=data + b"\0")
    with pytest.raises(orc.OracleError):
        orc.Stream(gc.damage(data, c, 3, "cdata"))


# --- A ----------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FAMILY["A"])
def test_edges_reach_the_read_limit_rules(name):
    k = gc.get(name)
    ans = dict(zip(k["pts"], gc.want(name)))
    ends = sum(1 for (b, e), v in ans.items() if v == e)
    assert 0.2 * len(ans) < ends < 0.7 * len(ans)
    true = gc.record_voffs(k["data"])
    assert all(v == e or v in true for (b, e), v in ans.items())
    if name in ("edges_short65280", "edges_long"):
        return  # thinned: the pairs below need not both be in
    # a window that ends 17 bytes into the next header is a RuntimeIOException
    # (no record start), one that ends 18 bytes into it a FileTruncatedException
    # after decoded records (a record start)
    c = gc.block_offsets(k["data"])
    pairs = 0
    for j in range(1, len(c) - 2):
        a17, a18 = ans.get((c[j], c[j + 1] + 17)), ans.get((c[j], c[j + 1] + 18))
        if a17 is None or a18 is None:
            continue
        pairs += a17 == c[j + 1] + 17 and a18 != c[j + 1] + 18 and a18 >> 16 == c[j]
    assert pairs >= 5
    # the tail: nothing at or past the file's end, nothing in the EOF block
    for (b, e), v in ans.items():
        if b >= c[-2]:
            assert v == e


# --- B ----------------------------------------------------------------------
@pytest.mark.parametrize("patch", list(gc.REJECTS))
def test_rejects_move_answers_past_the_patched_record(patch):
    k, base = gc.get("reject_" + patch), gc.get("reject_none_hdr1")
    assert k["lens"][:-1] == base["lens"][:-1] and len(k["pts"]) == len(base["pts"])
    n_ref = k["n_ref"]
    plain = upos(base, gc.oracle_guesses(base["data"], base["pts"]))
    got = upos(k, gc.want("reject_" + patch))
    # positions past a lengthened record shift by the bytes added before them
    per = (len(k["u"]) - len(base["u"])) // 3
    shift = lambda q: None if q is None else q - per * sum(1 for r in k["patched"] if k["starts"][r] < q)
    got = [shift(q) for q in got]
    changed = [(a, b) for a, b in zip(plain, got) if a != b]
    print(f"{patch}: {len(changed)} of {len(got)} answers moved")
    assert changed
    # every patched record sends answers to the record after it (a window that
    # ends before that record has no answer; the files compress to slightly
    # different sizes, so a window end may also fall elsewhere in a record)
    after = {base["starts"][r + 1] for r in k["patched"]}
    assert after <= {b for _, b in changed}
    assert n_ref > 1


def test_rejects_header_n_ref():
    k = gc.get("reject_ref_nref")
    hdr = gc.get("reject_ref_nref_hdr")
    assert hdr["data"] == k["data"] and hdr["header_n_ref"] == k["n_ref"] + 1
    base = gc.get("reject_none_hdr1")
    plain = upos(base, gc.oracle_guesses(base["data"], base["pts"]))
    # with one more sequence in the header, refID = n_ref is acceptable: the
    # answers of the unpatched file
    assert upos(hdr, gc.want("reject_ref_nref_hdr")) == plain
    assert moved(upos(k, gc.want("reject_ref_nref")), plain) > 0
    # a header without sequences refuses every placed record; the file's
    # records lie on its first sequence or none, so one sequence is enough
    assert moved(upos(gc.get("reject_none_hdr0"), gc.want("reject_none_hdr0")), plain) > 300
    assert upos(gc.get("reject_none_hdr1"), gc.want("reject_none_hdr1")) == plain


# --- C ----------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FAMILY["C"])
def test_damage_changes_answers(name):
    k = gc.get(name)
    intact = gc.oracle_guesses(k["intact"], k["pts"])
    got = gc.want(name)
    n = moved(list(intact), list(got))
    print(f"{name}: {n} of {len(got)} answers changed")
    assert n > 0
    if "_crc_" in name:  # DEFLATE intact: only a CRC check sees the damage
        orc.Stream(k["data"])
    if "_crc_" in name or "_isize_" in name or "_cdata_" in name or name == "corrupt_far":
        with pytest.raises(orc.OracleError):
            orc.Stream(k["data"], check_crc=True)
    if "_isize_" in name or "_cdata_" in name or "_cut" in name:
        with pytest.raises(orc.OracleError):  # (why the oracle guesses over file=)
            orc.Stream(k["data"])
    if name == "corrupt_far":
        j1, j2 = k["j"]
        c = k["c"]
        assert c[j2] - c[j1] > (1 << 20) + gc.MAX
        for j in (j1, j2):  # each damage changes answers of its own
            assert any(a != b for (beg, _), a, b in zip(k["pts"], intact, got) if abs(beg - c[j]) < 20000)


# --- D ----------------------------------------------------------------------
def test_crc_file_has_every_length():
    data, lens = gc.crc_file()
    s = orc.Stream(data, check_crc=True)
    assert tuple(int(x) for x in s.blocks["isize"] if x) == lens
    for n in gc.CRC_LENS:
        assert lens.count(n) >= 2
        j = lens.index(n)
        assert lens[j + 1:j + 4] == (4096,) * 3
    assert bytes(s.data) == gc.base4096()[1]


@pytest.mark.parametrize("isize,pos", gc.CRC_VARIANTS)
def test_crc_only_corruption_changes_answers(isize, pos):
    name = f"crc_undetected_{isize}_{pos}"
    k = gc.get(name)
    good, lens = gc.crc_file()
    # well-formed: every block inflates to its ISIZE; only the CRC check refuses it
    s = orc.Stream(k["data"])
    assert tuple(int(x) for x in s.blocks["isize"] if x) == lens
    with pytest.raises(orc.OracleError):
        orc.Stream(k["data"], check_crc=True)
    diff = [i for i, (a, b) in enumerate(zip(bytes(s.data), gc.base4096()[1])) if a != b]
    assert diff == [sum(lens[:k["j"]]) + pos]
    same = k["good_pts"]  # the same points, block for block, on the good file
    assert len(same) == len(k["pts"])
    kg = dict(k, data=good, pts=same)
    n = moved(upos(k, gc.want(name)), upos(kg, gc.oracle_guesses(good, same)))
    print(f"{name}: {n} of {len(same)} answers changed")
    assert n > 0


# --- E ----------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FAMILY["E"])
def test_empty_blocks_are_in_the_file(name):
    k = gc.get(name)
    s = orc.Stream(k["data"])
    isz = [int(x) for x in s.blocks["isize"]]
    c = k["c"]
    empty = [j for j in k["empty"] if j < len(c) - 1]
    assert all(isz[j] == 0 for j in empty)
    assert all(c[j + 1] - c[j] in (28, 31) for j in empty)
    if name == "empties":
        assert len(empty) == 4 and empty[2] == empty[1] + 1 and isz[-1] == 0 and len(isz) - 1 not in empty
    else:
        assert isz[-1] == 0 and len(isz) - 1 == empty[-1]
    ans = dict(zip(k["pts"], gc.want(name)))
    true = gc.record_voffs(gc.empties_file()[0])  # (the cut file ends inside a record)
    assert all(v == e or v in true for (b, e), v in ans.items())
    for j in empty:  # an empty block first after beg: no guess inside it
        v = ans[(c[j], c[j] + gc.MAX)]
        assert v == c[j] + gc.MAX or v >> 16 > c[j]


# --- F ----------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FAMILY["F"])
def test_false_magic_is_in_a_payload(name):
    k = gc.get(name)
    assert len(k["magics"]) == 3 and not set(k["magics"]) & set(k["c"])
    s = orc.Stream(k["data"])
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == 3000
    true = set(int(v) for v in want["voff"])
    ans = dict(zip(k["pts"], gc.want(name)))
    assert all(v == e or v in true for (b, e), v in ans.items())
    for m in k["magics"]:
        # the scan meets the false magic and goes on to the next real block
        nxt = k["c"][bisect.bisect_right(k["c"], m)]
        assert ans[(m, m + gc.MAX)] >> 16 == nxt == ans[(m - 40, m - 40 + gc.MAX)] >> 16
        assert ans[(m - 1, m + 30)] == m + 30


# --- G ----------------------------------------------------------------------
DECOY_ANSWERED = ("merge", "merge3", "cascade", "tail_eof", "tail_noeof")


@pytest.mark.parametrize("name", list(cc.FALSE_START_CASES))
def test_chain_decoys(name):
    k = gc.get("chain_" + name)
    ch = k["chain"]
    s, _, want = cc.expected(name, orc.STRICT)
    true = set(int(v) for v in want["voff"])
    ans = dict(zip(k["pts"], gc.want("chain_" + name)))
    false = {v for (b, e), v in ans.items() if v != e and v not in true}
    decoys = {s.voff_of(d["pos"]) for d in ch["decoys"]}
    if name in DECOY_ANSWERED:
        # the reference's own answer at a decoy's block is the decoy: a
        # position inside tag data
        assert false and false <= decoys
        for d in ch["decoys"]:
            v = s.voff_of(d["pos"])
            if v in false:
                assert ans[(v >> 16, (v >> 16) + gc.MAX)] == v and v & 0xffff == 0
    else:
        assert not false


# --- H ----------------------------------------------------------------------
def test_grouping_points_span_several_windows():
    k = gc.get("grouping")
    begs = sorted(b for b, _ in k["pts"])
    assert begs[-1] - begs[0] > (1 << 20) + gc.MAX  # the host's window cap at its floor
    assert len(k["pts"]) > 3000 and sum(1 for b, e in k["pts"] if e == len(k["data"])) > 40
