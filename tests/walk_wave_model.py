"""k_rec_walk_wave (hbam_chain.hip) restated in plain Python: a block's guess
walk taken by a wave of segment walkers whose lists are stitched together.

The chain from a block's candidate c is deterministic: the record at q names
the next start q + 4 + block_size, so a walk that starts at any record start
on that chain lists exactly what the walk from c lists from there on.  The
block [b0, bend) is cut into segments of `seg` bytes counted from b0:

  probe    the start c_j of segment j is the first position of [s_j, s_j +
           PROBE) that passes the refID prefilter and plausible2 (None when
           there is none).  The block's candidate is c_0 (a full scan of the
           block when segment 0's window holds no start), moved by the 1-3
           byte shift rule; the segment holding c starts its walk at c, the
           segments before it take no part.
  walk     walker j lists the plausible records from c_j that start before
           s_{j+1}; the last segment's walker also walks the lookahead past
           the block end.
  stitch   cur = c.  While cur is inside the block: walker k of the segment
           holding cur is taken when c_k == cur (the block fails when that
           walker met an implausible record), else the walk goes on serially
           from cur to the end of segment k.  When the last piece did not end
           at the block end, the lookahead is walked from the exit.

block_walk_wave returns what guess_walk(u, c, bend, ...) returns, plus how
many pieces were walker lists and how many were serial walks: the tests
compare the first three and use the counts to show which branch an input
reached."""
import numpy as np

from chain_cases import LOOKAHEAD, plausible, plausible2, rd32

PROBE = 512  # positions probed at the start of every segment
SEG = 4096   # kWalkSeg


def prefilter_mask(u, n_ref, e_inf=None):
    """cand_prefilter at every position of u."""
    n = len(u)
    e_inf = n if e_inf is None else e_inf
    a = np.frombuffer(bytes(u) + b"\0" * 32, dtype=np.uint8).astype(np.uint32)

    def i32_at(off):
        w = a[off:off + n] | (a[off + 1:off + 1 + n] << 8) | (a[off + 2:off + 2 + n] << 16) | (a[off + 3:off + 3 + n] << 24)
        return w.view(np.int32)

    ref, nref = i32_at(4), i32_at(24)
    ok = (ref >= -1) & (ref < n_ref) & (nref >= -1) & (nref < n_ref)
    return ok | (np.arange(n) + 36 > e_inf)


def first_start(u, pre, lo, hi, n_ref, e_inf=None):
    """The first position of [lo, hi) that passes the prefilter and plausible2."""
    for q in np.flatnonzero(pre[lo:hi]):
        if plausible2(u, lo + int(q), n_ref, e_inf):
            return lo + int(q)
    return None


def block_candidate(u, pre, b0, bend, n_ref, e_inf=None):
    """k_rec_cand's result for the block: segment 0's probe, the full scan when
    that finds nothing, then the 1-3-byte shift rule."""
    e_inf = len(u) if e_inf is None else e_inf
    c = first_start(u, pre, b0, min(b0 + PROBE, bend), n_ref, e_inf)
    if c is None:
        c = first_start(u, pre, b0, bend, n_ref, e_inf)
    if c is None:
        return None
    if c + 4 + rd32(u, c) >= bend:
        for d in (1, 2, 3):
            q = c + d
            if q + 36 <= e_inf and q + 4 + rd32(u, q) < bend and plausible2(u, q, n_ref, e_inf):
                return q
    return c


def piece_walk(u, start, lim, bend, n_ref, e_inf=None, lookahead=LOOKAHEAD):
    """The shared plausible walk: records from `start` are listed while they
    start before lim; with lim == bend the lookahead past the block end is
    walked too (guess_walk), with lim < bend the walk ends at lim."""
    e_true = len(u)
    e_inf = e_true if e_inf is None else e_inf
    q, exitq, left, listed = start, start, lookahead, []
    while True:
        inside = q < lim
        if not inside:
            if lim < bend or left <= 0 or q == e_true or q + 36 > e_inf:
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


def block_walk_wave(u, pre, b0, bend, n_ref, e_inf=None, seg=SEG, lookahead=LOOKAHEAD):
    """(c, valid, listed, exit, walker pieces, serial pieces) of the block; c
    None: no candidate, nothing walked."""
    c = block_candidate(u, pre, b0, bend, n_ref, e_inf)
    if c is None:
        return None, False, [], None, 0, 0
    nseg = (bend - b0 + seg - 1) // seg
    k0 = (c - b0) // seg
    start = [None] * nseg
    start[k0] = c
    for j in range(k0 + 1, nseg):
        s = b0 + j * seg
        start[j] = first_start(u, pre, s, min(s + PROBE, bend), n_ref, e_inf)
    lim = [min(b0 + (j + 1) * seg, bend) for j in range(nseg)]
    walks = [None if start[j] is None else piece_walk(u, start[j], lim[j], bend, n_ref, e_inf, lookahead)
             for j in range(nseg)]
    cur, listed, taken, serial, looked = c, [], 0, 0, False
    while cur < bend:
        k = (cur - b0) // seg
        if start[k] == cur:
            ok, part, x = walks[k]
            taken += 1
        else:
            ok, part, x = piece_walk(u, cur, lim[k], bend, n_ref, e_inf, lookahead)
            serial += 1
        if not ok:
            return c, False, [], None, taken, serial
        assert part and x >= lim[k] > cur and len(part) <= (seg + 35) // 36
        listed += part
        cur = x
        looked = lim[k] == bend
    if not looked and not piece_walk(u, cur, bend, bend, n_ref, e_inf, lookahead)[0]:
        return c, False, [], None, taken, serial
    return c, True, listed, cur, taken, serial
