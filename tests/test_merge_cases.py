"""CPU: the merge tests' inputs (tests/merge_cases.py) are what they are there
for, and the identity the GPU tests rest on holds: consecutive record ranges
of a case, each sorted on its own and merged with ties to the earlier run,
are the sort of the whole case, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hbam
import merge_cases as mc
import sort_cases as sc
from hbam.sort import sort_words


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_merged_consecutive_runs_are_the_sorted_whole(name, order):
    case = sc.CASES[name]()
    want_enc, want_offs, want_perm = case.expected(order)
    for cut, bounds in mc.cuts(case.n).items():
        runs = mc.consecutive_runs(case, order, bounds)
        assert sum(r.n for r in runs) == case.n, cut
        enc, offs, src = mc.merged(runs)
        assert enc == want_enc, cut
        np.testing.assert_array_equal(offs, want_offs, err_msg=cut)
        ids = np.array([runs[int(s) >> 32].ids[int(s) & 0xFFFFFFFF] for s in src], np.int64)
        np.testing.assert_array_equal(ids, want_perm.astype(np.int64), err_msg=cut)


def test_cuts_are_uneven_with_empty_and_one_record_runs():
    assert list(mc.cuts(1)) == ["k1"]
    for n in (60, 255, 500, 4000):
        c = mc.cuts(n)
        sizes = {k: np.diff(v).tolist() for k, v in c.items()}
        assert [len(v) for v in sizes.values()] == [1, 2, 3, 7]
        assert sizes["k2"][0] != sizes["k2"][1]
        assert sizes["k3_empty_middle"][1] == 0 and sizes["k3_empty_middle"][0] > 0 < sizes["k3_empty_middle"][2]
        k7 = sizes["k7_one_record_runs"]
        assert k7[0] == 1 and k7[-1] == 1 and min(k7) >= 1 and len(set(k7)) >= 5
        assert all(sum(v) == n for v in sizes.values())
    assert set(mc.SMALL_PARTS) <= set(sc.CASES)
    for name, (lo, hi) in mc.SMALL_PARTS.items():
        assert 0 <= lo < hi <= sc.CASES[name]().n and hi - lo <= 500


def test_sort_words_restates_the_kernel_word():
    for name in ("mixed", "long", "test.bam"):
        c = sc.CASES[name]().cols
        for order in sc.ORDERS:
            w = sort_words(c["key"], c["ref_id"], c["pos"], order)
            assert w.dtype == np.uint64
            np.testing.assert_array_equal(w, mc.words_u64(c, order))
            # ascending unsigned words = the order sort_cases sorts by
            np.testing.assert_array_equal(np.argsort(w, kind="stable"),
                                          np.argsort(sc.sort_word(c, order), kind="stable"))
    assert int(sort_words([-1], [0], [0], "key")[0]) == (1 << 63) - 1 and int(sort_words([0], [0], [0], "key")[0]) == 1 << 63
    assert int(sort_words([0], [-1], [-1], "coordinate")[0]) == 0xFFFFFFFF << 32
    with pytest.raises(hbam.HbamError):
        sort_words([0], [0], [0], 5)


@pytest.mark.parametrize("order", sc.ORDERS)
def test_part_sizes_cut_mixed_where_the_merge_can_go_wrong(order):
    case = sc.mixed_case()
    seen_every = False
    for cut in ("k2", "k7_one_record_runs"):
        runs = mc.consecutive_runs(case, order, mc.cuts(case.n)[cut])
        _, offs, src = mc.merged(runs)
        words = np.concatenate([r.words for r in runs])[np.argsort(np.concatenate([r.words for r in runs]),
                                                                    kind="stable")]
        run_of = (src >> np.uint64(32)).astype(np.int64)
        for pb in mc.PART_BYTES[:3]:
            heads = mc.part_heads(offs, pb)
            assert len(heads) >= 20
            # a part boundary inside a group of equal words that spans two runs
            inside = [j for j in heads[1:] if words[j] == words[j - 1]
                      and len(set(run_of[words == words[j]].tolist())) >= 2]
            assert inside, (cut, pb)
            per_part = mc.part_runs(src, heads)
            seen_every |= any(len(s) == len(runs) for s in per_part)
        assert len(mc.part_heads(offs, mc.BIG)) == 1
    assert seen_every
    # ... and parts fed by a single run: the 64-byte parts, and disjoint pieces
    lo, hi = mc.SMALL_PARTS["mixed"]
    runs = mc.consecutive_runs(case, order, [lo, lo + (hi - lo) // 3, hi])
    _, offs, src = mc.merged(runs)
    heads = mc.part_heads(offs, 64)
    sizes = np.diff(np.concatenate([heads, [len(src)]]))
    assert 1 <= sizes.min() and sizes.max() <= 2
    assert all(len(s) == 1 for s in mc.part_runs(src, heads)[:10])
    _, offs, src = mc.merged(mc.reversed_piece_runs(case, order))
    assert any(len(s) == 1 for s in mc.part_runs(src, mc.part_heads(offs, mc.TILE)))


@pytest.mark.parametrize("name", list(mc.SMALL_PARTS))
def test_64_byte_parts_hold_one_or_two_records(name):
    case = sc.CASES[name]()
    lo, hi = mc.SMALL_PARTS[name]
    for order in sc.ORDERS:
        _, offs, _ = case.expected(order, lo, hi)
        heads = mc.part_heads(offs, 64)
        sizes = np.diff(np.concatenate([heads, [hi - lo]]))
        assert sizes.min() >= 1 and sizes.max() <= 2
        if hi - lo > 1:
            assert len(heads) > (hi - lo) // 2


def test_long_records_give_one_record_parts_and_skipped_parts():
    case = sc.long_case()
    assert int(case.lens.min()) > 0 and int(case.lens.max()) > 2 * mc.TILE
    for order in sc.ORDERS:
        _, offs, _ = case.expected(order)
        heads = mc.part_heads(offs, mc.TILE)
        ends = np.concatenate([heads[1:], [case.n]])
        nbytes = offs[ends].astype(np.int64) - offs[heads].astype(np.int64)
        single_big = (ends - heads == 1) & (nbytes > mc.TILE)
        assert np.count_nonzero(single_big) >= 10
        # parts in which no record starts do not exist
        assert len(heads) < -(-int(offs[-1]) // mc.TILE)
        assert np.all(nbytes < mc.TILE + int(case.lens.max()))


@pytest.mark.parametrize("order", sc.ORDERS)
def test_arrangements_are_sorted_runs_of_the_same_records(order):
    case = sc.mixed_case()
    want = sorted(case.enc[int(a):int(b)] for a, b in zip(case.offs[:-1], case.offs[1:]))
    rr = mc.round_robin_runs(case, order)
    assert len(rr) == 4 and {r.n for r in rr} == {case.n // 4}
    rev = mc.reversed_piece_runs(case, order)
    assert len(rev) == 3 and int(rev[0].words[0]) >= int(rev[1].words[-1]) >= int(rev[2].words[-1])
    for runs in (rr, rev):
        enc, offs, src = mc.merged(runs)
        assert sorted(enc[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])) == want
        got = np.array([runs[int(s) >> 32].words[int(s) & 0xFFFFFFFF] for s in src], np.uint64)
        assert np.all(got[1:] >= got[:-1])
    # the interleave takes from all four runs all the way; the reversed pieces come out last run first
    _, _, src = mc.merged(rr)
    assert set((src[:64] >> np.uint64(32)).tolist()) == {0, 1, 2, 3}
    _, _, src = mc.merged(rev)
    assert int(src[0]) >> 32 == 2 and int(src[-1]) >> 32 == 0


def test_equal_words_come_out_run_after_run():
    for order in sc.ORDERS:
        runs = mc.equal_word_runs(order)
        assert [r.n for r in runs] == [5, 1, 9]
        assert len({int(w) for r in runs for w in r.words}) == 1
        assert len({len(r.record(i)) for r in runs for i in range(r.n)}) >= 8
        enc, offs, src = mc.merged(runs)
        assert enc == b"".join(r.enc for r in runs)
        assert src.tolist() == [(k << 32) | i for k, r in enumerate(runs) for i in range(r.n)]


def test_merge_entry_points_are_declared_and_refuse_a_null_ctx():
    names = hbam.exported_symbols_from_header()
    L = hbam.lib()
    a, b, c = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    for f in ("hbam_merge_begin", "hbam_merge_add_run", "hbam_merge_plan", "hbam_merge_next", "hbam_merge_end"):
        assert f in names
    assert L.hbam_merge_begin(None, hbam.SORT_KEY) == hbam.E_STATE
    assert L.hbam_merge_add_run(None, None, 0, None, 0, None) == hbam.E_STATE
    assert L.hbam_merge_plan(None, 0, C.byref(a), C.byref(b), C.byref(c)) == hbam.E_STATE
    assert (a.value, b.value, c.value) == (0, 0, 0)
    a.value = b.value = 7
    assert L.hbam_merge_next(None, None, 0, None, None, C.byref(a), C.byref(b)) == hbam.E_STATE
    assert (a.value, b.value) == (0, 0)
    assert L.hbam_merge_end(None) == hbam.E_STATE
    for cls in (hbam.Codec, hbam.BamFile):
        for m in ("merge_begin", "merge_add_run", "merge_plan", "merge_next", "merge_end", "iter_merged"):
            assert callable(getattr(cls, m))
