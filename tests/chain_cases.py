"""BAM files that take the record chain off its common path, with the oracle
as the only source of expected outputs.

The chain finds record boundaries by guessing ("record chain"):
each BGZF block's first plausible record start (k_rec_cand), a walk from it
that must stay plausible to the block end and for kGuessLookahead records
beyond (k_rec_walk), later candidates when that walk fails (k_rec_search), a
max-scan link check that re-walks blocks off the true chain or drops stray
walks (k_rec_linkfix), and the serial link after kMaxLinkFix rounds.  On
well-formed files the first candidate of every block is the true one, so two
families of inputs are built here from synth.make_bam(3000, seed=...):

False starts (FALSE_START_CASES).  A *decoy* is a run of bytes inside the
payload of a B:c tag appended to a host record, with a BGZF block cut exactly
at its first byte, made of copies of other records of the same file
("donors").  The reference reads it as tag data; the chain's guess starts a
walk on it.  Every file reads as 3000 valid records under STRICT.

Implausible but readable records (IMPLAUSIBLE_CASES).  True records that
BAMRecordCodec.decode under SILENT (and SplittingBAMIndexer always) accepts
and plausible() rejects: the guess of their block fails, and only the link
step can put them on the chain.

plausible / plausible2 / chain_step / guess_walk / block_guess restate the
device functions of hbam_chain.hip in plain Python, with e_inf (the end of
the inflated range) as a parameter.  They are used only to assert that an
input has the property its case is named for, never for expected outputs.

shift1: a start one byte before a true record t passes plausible2 on fully
inflated data when the byte before t is 0 and the record at t has refID and
next_refID 0, bit 23 of pos and next_pos clear, and pos's top byte equal to
l_read_name + 1 (so that the shifted l_read_name's name-end byte is the true
name's NUL).  Such a pos is at least 37 << 24, past every contig of the
synthetic header, so the case lengthens chr1 to 999,999,999 in the binary
and the text header (same number of digits); the record is an unmapped
paired read placed at that pos, which STRICT accepts.  The construction
passes plausible2 with e_inf == e_true, so shift1 is not windowed-only.
"""
import functools
import struct

import numpy as np

import orc
from hbam import synth

N = 3000
BLOCK = 65280
LOOKAHEAD = 4  # kGuessLookahead


def rd32(u, q):
    return struct.unpack_from("<i", u, q)[0]


# ---------------------------------------------------------------------------
# the device functions, restated
# ---------------------------------------------------------------------------
def plausible(u, q, n_ref, e_inf=None):
    e_true = len(u)
    e_inf = e_true if e_inf is None else e_inf
    if q + 36 > e_inf:
        return e_inf < e_true and q + 4 <= e_inf and rd32(u, q) >= 32
    bs, ref, pos, lrn, _mq, _bin, ncig, _flag, lseq, nref, npos = struct.unpack_from("<iiiBBHHHiii", u, q)
    if ref < -1 or ref >= n_ref or nref < -1 or nref >= n_ref:
        return False
    if pos < -1 or npos < -1 or lrn < 1 or lseq < 0:
        return False
    if bs < 32 + lrn + 4 * ncig + lseq + (lseq + 1) // 2:
        return False
    if q + 4 + bs > e_true:
        return False
    if q + 36 + lrn > e_inf:
        return e_inf < e_true
    return u[q + 36 + lrn - 1] == 0


def plausible2(u, q, n_ref, e_inf=None):
    e_true = len(u)
    e_inf = e_true if e_inf is None else e_inf
    if not plausible(u, q, n_ref, e_inf):
        return False
    q2 = q + 4 + rd32(u, q)
    return q2 == e_true or q2 + 36 > e_inf or plausible(u, q2, n_ref, e_inf)


def chain_step(u, q, e_inf=None, indexer=False):
    """The next record start after q under the reader's (indexer's) rules, or None."""
    e_inf = len(u) if e_inf is None else e_inf
    if q + 4 > e_inf:
        return None
    bs = rd32(u, q)
    if indexer:
        return q + 4 + max(bs, 0)
    return None if bs < 32 else q + 4 + bs


def guess_walk(u, c, bend, n_ref, e_inf=None, lookahead=LOOKAHEAD):
    """k_rec_walk's guess branch (and k_rec_search's walk) from candidate c of
    a block ending at bend: (valid, record starts listed, exit)."""
    e_true = len(u)
    e_inf = e_true if e_inf is None else e_inf
    q, exitq, left, listed = c, c, lookahead, []
    while True:
        inside = q < bend
        if not inside:
            if left <= 0 or q == e_true or q + 36 > e_inf:
                break
            left -= 1
        if not plausible(u, q, n_ref, e_inf):
            return False, listed, exitq
        q2 = q + 4 + rd32(u, q)
        if inside:
            listed.append(q)
            exitq = q2
        q = q2
    return True, listed, exitq


def plausible_run(u, c, bend, n_ref, e_inf=None):
    """Walking from c while records are plausible: (records that start inside
    [c, bend), records that start at or past bend, where the run stopped)."""
    e_true = len(u)
    inside = beyond = 0
    q = c
    while q < e_true and plausible(u, q, n_ref, e_inf):
        if q < bend:
            inside += 1
        else:
            beyond += 1
        q += 4 + rd32(u, q)
    return inside, beyond, q


def block_guess(u, b0, bend, n_ref, e_inf=None, lookahead=LOOKAHEAD):
    """k_rec_cand, the guess walk and k_rec_search for the block [b0, bend):
    (g, x, searched) with g None when the block ends up without a guess."""
    e_true = len(u)
    e_inf = e_true if e_inf is None else e_inf
    c = next((q for q in range(b0, bend) if plausible2(u, q, n_ref, e_inf)), None)
    if c is None:
        return None, None, False
    if c + 4 + rd32(u, c) >= bend:  # the 1-3-byte shift rescue
        for d in (1, 2, 3):
            q = c + d
            if q + 36 <= e_inf and q + 4 + rd32(u, q) < bend and plausible2(u, q, n_ref, e_inf):
                c = q
                break
    ok, _, x = guess_walk(u, c, bend, n_ref, e_inf, lookahead)
    if ok:
        return c, x, False
    for q in range(c + 1, bend):
        if plausible2(u, q, n_ref, e_inf):
            ok, _, x = guess_walk(u, q, bend, n_ref, e_inf, lookahead)
            if ok:
                return q, x, True
    return None, None, True


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(seed=3):
    """(header bytes, the 3000 records as bytes each, n_ref) of make_bam(3000, seed)."""
    d, _ = synth.make_bam(N, seed=seed)
    s = orc.Stream(d)
    u = bytes(s.data)
    q, recs = s.header_end, []
    while q < len(u):
        e = q + 4 + rd32(u, q)
        recs.append(u[q:e])
        q = e
    assert len(recs) == N
    return u[:s.header_end], tuple(recs), s.n_ref


def with_tag(rec, payload, tag=b"XX"):
    """rec with a B:c tag holding payload appended: (record, payload's offset in it)."""
    body = rec[4:] + tag + b"Bc" + struct.pack("<i", len(payload))
    return struct.pack("<i", len(body) + len(payload)) + body + payload, 4 + len(body)


def junk_head():
    """40 bytes whose head passes the refID prefilter and fails plausible() (pos < -1)."""
    return struct.pack("<iiiBBHHHiiii", 100, 0, -7, 40, 0, 0, 0, 0, 100, 0, 0, 0) + b"\0\0\0\0"


def filler(n, seed):
    """Tag bytes with no plausible record start: refID would be 0x40404040."""
    return bytes(np.random.default_rng(seed).integers(0x40, 0x80, n, dtype=np.uint8))


def layout(head, recs):
    """(inflated stream, start of every record)."""
    starts, q = [], len(head)
    for r in recs:
        starts.append(q)
        q += len(r)
    return head + b"".join(recs), starts


def cut_lens(total, cuts):
    """Block lengths with a cut at every position of cuts and no block above 65280."""
    lens, p = [], 0
    for c in sorted(set(cuts)) + [total]:
        while c - p > BLOCK:
            lens.append(BLOCK)
            p += BLOCK
        if c > p:
            lens.append(c - p)
            p = c
    return lens


def block_of(lens, pos):
    """[b0, bend) of the block holding pos."""
    p = 0
    for n in lens:
        if p <= pos < p + n:
            return p, p + n
        p += n
    raise ValueError(pos)


def finish(name, u, starts, n_ref, cuts, decoys=(), eof=True, **facts):
    lens = cut_lens(len(u), cuts)
    return dict(name=name, u=u, starts=starts, n_ref=n_ref, lens=lens, decoys=list(decoys),
                data=orc.bgzf_compress(u, lens, level=5, eof=eof), **facts)


def donors(recs, first, n):
    return [recs[first + i] for i in range(n)]


# ---------------------------------------------------------------------------
# false starts
# ---------------------------------------------------------------------------
def _hosted(hosts, seed=3):
    """The base file with payload hosts[r] in a tag of record r:
    (head, recs, n_ref, u, starts, {r: payload start})."""
    head, recs, n_ref = base(seed)
    recs, at = list(recs), {}
    for r, payload in hosts.items():
        recs[r], at[r] = with_tag(recs[r], payload)
    u, starts = layout(head, recs)
    return head, recs, n_ref, u, starts, {r: starts[r] + o for r, o in at.items()}


def case_merge(at=(1000,), name="merge"):
    _, recs, _ = base()
    _, _, n_ref, u, starts, pay = _hosted({r: recs[N - 1 - r] for r in at})
    decoys = [dict(pos=pay[r], host=r) for r in sorted(at)]
    return finish(name, u, starts, n_ref, pay.values(), decoys)


def case_deadend():
    _, recs, _ = base()
    r = 1000
    d = donors(recs, 2000, 2)
    _, _, n_ref, u, starts, pay = _hosted({r: b"".join(d) + junk_head()})
    return finish("deadend", u, starts, n_ref, pay.values(), [dict(pos=pay[r], host=r)],
                  junk=pay[r] + len(d[0]) + len(d[1]))


def case_look(k):
    """5 donors to the block end, k more past it, then an implausible head."""
    _, recs, _ = base()
    r = 1000
    inb, past = donors(recs, 2000, 5), donors(recs, 2100, k)
    _, _, n_ref, u, starts, pay = _hosted({r: b"".join(inb + past) + junk_head()})
    bend = pay[r] + sum(map(len, inb))
    return finish(f"look{k}", u, starts, n_ref, [pay[r], bend], [dict(pos=pay[r], host=r)], decoy_block_end=bend)


def _stray(name, patch_exit, host=1000, extra_hosts=None, exit_rec=None):
    _, recs, _ = base()
    inb = donors(recs, 2000, 8)
    tail = b"" if patch_exit else b"".join(donors(recs, 2100, LOOKAHEAD)) + junk_head()
    payload = filler(70000, 1) + b"".join(inb) + tail + filler(130000, 2)
    hosts = {host: payload}
    hosts.update(extra_hosts or {})
    _, _, n_ref, u, starts, pay = _hosted(hosts)
    c = pay[host] + 70000
    bend = c + sum(map(len, inb))
    facts = dict(decoy_block_end=bend, host_end=starts[host + 1])
    if patch_exit:
        # the last in-block donor's block_size now leads to a true record start past the host
        last = bend - len(inb[-1])
        t = starts[exit_rec]
        ub = bytearray(u)
        struct.pack_into("<i", ub, last, t - last - 4)
        u = bytes(ub)
        facts["exit"] = t
    decoys = [dict(pos=c, host=host)] + [dict(pos=pay[r], host=r) for r in sorted(extra_hosts or {})]
    return finish(name, u, starts, n_ref, [c, bend] + [pay[r] for r in (extra_hosts or {})], decoys, **facts)


def case_stray_in():
    return _stray("stray_in", False)


def case_stray_out():
    return _stray("stray_out", True, exit_rec=1300)


def case_cascade():
    """A stray_out decoy whose exit lies past 8 consecutive blocks that each
    start with a merge decoy."""
    _, recs, _ = base()
    merges = [1200 + 100 * i for i in range(8)]
    c = _stray("cascade", True, host=600, extra_hosts={r: recs[N - 1 - r] for r in merges},
               exit_rec=merges[-1] + 250)
    c["merge_hosts"] = merges
    return c


def case_tail(eof):
    """A merge decoy in the file's last record: its chain ends with the stream."""
    c = case_merge(at=(N - 1,), name="tail_eof" if eof else "tail_noeof")
    if not eof:
        c["data"] = orc.bgzf_compress(c["u"], c["lens"], level=5, eof=False)
    return c


def case_shift1():
    head, recs, n_ref = base()
    recs = list(recs)
    # chr1 long enough for a pos of (l_read_name + 1) << 24
    old, new = b"SN:chr1\tLN:249250621", b"SN:chr1\tLN:999999999"
    assert head.count(old) == 1
    head = head.replace(old, new)
    at = head.index(b"chr1\0", len(old) + 8) + 5
    assert rd32(head, at) == 249250621
    head = head[:at] + struct.pack("<i", 999999999) + head[at + 4:]
    # the record at t: an unmapped paired read (no cigar) placed on chr1
    ti = 1500
    src = bytearray(recs[682])
    bs, ref, pos, lrn, mq, _bin, ncig, flag, lseq, nref, npos = struct.unpack_from("<iiiBBHHHiii", src, 0)
    assert (ref, nref, ncig, mq) == (0, 0, 0, 0) and flag & 5 == 5 and not npos & 0x800000
    pos = ((lrn + 1) << 24) | (pos & 0x7FFFFF)
    struct.pack_into("<i", src, 8, pos)
    struct.pack_into("<H", src, 14, 4681 + (pos >> 14))  # reg2bin(pos, pos + 1)
    recs[ti] = bytes(src)
    # t - 1 reads block_size << 8: pad a record on the way so that it leads to a true record start
    u, starts = layout(head, recs)
    t = starts[ti]
    target = t - 1 + 4 + ((bs & 0xFFFFFF) << 8)
    j = max(i for i in range(N) if starts[i] <= target)
    if target - starts[j] < 8:
        j -= 1
    pad = target - starts[j]
    recs[j - 1], _ = with_tag(recs[j - 1], b"\x55" * (pad - 8), tag=b"XP")
    u, starts = layout(head, recs)
    assert starts[ti] == t and starts[j] == target
    return finish("shift1", u, starts, n_ref, [t - 1], [dict(pos=t - 1, host=ti - 1)], t=t, far=target)


FALSE_START_CASES = {
    "merge": case_merge,
    "merge3": lambda: case_merge(at=(700, 1400, 2100), name="merge3"),
    "deadend": case_deadend,
    "look3": lambda: case_look(3),
    "look4": lambda: case_look(4),
    "stray_in": case_stray_in,
    "stray_out": case_stray_out,
    "shift1": case_shift1,
    "cascade": case_cascade,
    "tail_eof": lambda: case_tail(True),
    "tail_noeof": lambda: case_tail(False),
}


# ---------------------------------------------------------------------------
# implausible but readable records
# ---------------------------------------------------------------------------
def _p32(off, v):
    def f(rec):
        b = bytearray(rec)
        struct.pack_into("<i", b, off, v)
        return bytes(b)
    return f


def _lrn0(rec):
    return rec[:12] + b"\0" + rec[13:]


def _nonul(rec):
    at = 36 + rec[12] - 1
    assert rec[at] == 0
    return rec[:at] + b"X" + rec[at + 1:]


PATCHES = {
    "pos": _p32(8, -5),
    "lrn0": _lrn0,
    "lseq_big": _p32(20, 1 << 20),
    "npos": _p32(28, -9),
    "nonul": _nonul,
    "lseq_neg": _p32(20, -3),
}


def _patched(name, patches, cut_at_record=None):
    """The base file with patches {record: patch name} applied, on 65280-byte
    blocks (plus a cut at the start of record cut_at_record)."""
    head, recs, n_ref = base()
    recs = list(recs)
    for r, p in patches.items():
        recs[r] = PATCHES[p](recs[r])
    u, starts = layout(head, recs)
    cuts = [] if cut_at_record is None else [starts[cut_at_record]]
    return finish(name, u, starts, n_ref, cuts, patched=sorted(patches))


def _first_record_at_or_after(pos):
    head, recs, _ = base()
    _, starts = layout(head, recs)
    return next(i for i, s in enumerate(starts) if s >= pos)


def _implausible_cases():
    cases = {"six": lambda: _patched("six", {500: "pos", 900: "lrn0", 1300: "lseq_big", 1700: "npos",
                                             2100: "nonul", 2500: "lseq_neg"})}

    def add(name, fn):
        cases[name] = fn

    for p in ("pos", "lrn0"):
        add(f"{p}_blockfirst", lambda p=p: _patched(f"{p}_blockfirst", {1000: p}, cut_at_record=1000))
        for k in range(1, 5):  # the k-th record start past the end of block 4 (block 4's lookahead zone)
            add(f"{p}_after{k}", lambda p=p, k=k: _patched(
                f"{p}_after{k}", {_first_record_at_or_after(5 * BLOCK) + k - 1: p}))
        add(f"{p}_first", lambda p=p: _patched(f"{p}_first", {0: p}))
        add(f"{p}_last", lambda p=p: _patched(f"{p}_last", {N - 1: p}))
        add(f"{p}_pair", lambda p=p: _patched(f"{p}_pair", {1500: p, 1501: p}))
        add(f"{p}_wholeblock", lambda p=p: _patched(f"{p}_wholeblock", {
            i: p for i in range(_first_record_at_or_after(7 * BLOCK), _first_record_at_or_after(8 * BLOCK))}))
    return cases


IMPLAUSIBLE_CASES = _implausible_cases()


@functools.lru_cache(maxsize=None)
def get(name):
    """The case `name`, built once per process."""
    return (FALSE_START_CASES.get(name) or IMPLAUSIBLE_CASES[name])()


@functools.lru_cache(maxsize=None)
def expected(name, stringency):
    """(oracle Stream, rc, records) of the whole file under `stringency`; shared, never modified."""
    s = orc.Stream(get(name)["data"], stringency=stringency)
    rc, want = s.decode_all()
    return s, rc, want
