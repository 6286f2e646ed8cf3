"""GPU: hbam_merge_* (k sorted runs of SAMRecordWritable encodings merged on
the GPU, the runs' bytes in host memory) against the expected result of
tests/merge_cases.py, bit for bit: the concatenated parts, their offsets and
src; the words computed by the library against the caller's; the calls
interleaved with decodes and sorts on one ctx; the errors; and
hbam.sort.sort_bam(merge=True) from a multi-window read against the
one-window sort of the same file."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import bai
import hbam
import merge_cases as mc
import sort_cases as sc
from hbam.sort import sort_bam, sort_words, sorted_header

pytestmark = pytest.mark.gpu


def run_merge(ctx, order, runs, part_bytes, words=True):
    """The merge of the runs on ctx: (bytes, offs, src, parts) with the parts'
    offsets made global."""
    ctx.merge_begin(order)
    try:
        for r in runs:
            ctx.merge_add_run(r.enc, r.offs, r.words if words else None)
        n_parts, n_records, nbytes = ctx.merge_plan(part_bytes)
        enc, offs, src, heads = [], [np.zeros(1, np.uint64)], [], []
        at = 0
        while True:
            part = ctx.merge_next()
            if part is None:
                break
            b, o, s = part
            assert o.dtype == np.uint64 and s.dtype == np.uint64 and len(o) == len(s) + 1
            assert int(o[0]) == 0 and int(o[-1]) == len(b) and len(s) >= 1
            heads.append(sum(len(x) for x in src))
            enc.append(b)
            offs.append(o[1:] + np.uint64(at))
            src.append(s)
            at += len(b)
        assert len(heads) == n_parts and at == nbytes
        src = np.concatenate(src) if src else np.zeros(0, np.uint64)
        assert len(src) == n_records
        return b"".join(enc), np.concatenate(offs), src, np.array(heads, np.int64)
    finally:
        ctx.merge_end()


def check(got, runs, part_bytes, what):
    enc, offs, src, heads = got
    wenc, woffs, wsrc = mc.merged(runs)
    np.testing.assert_array_equal(src, wsrc, err_msg=what)
    np.testing.assert_array_equal(offs, woffs, err_msg=what)
    np.testing.assert_array_equal(heads, mc.part_heads(woffs, part_bytes), err_msg=what)
    assert len(enc) == len(wenc), what
    if enc != wenc:  # name the first byte that differs and the record it lies in
        a, b = np.frombuffer(enc, np.uint8), np.frombuffer(wenc, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woffs, at, side="right")) - 1
        raise AssertionError(f"{what}: byte {at} differs: output record {j} (run {int(wsrc[j]) >> 32} record "
                             f"{int(wsrc[j]) & 0xFFFFFFFF}) at its byte {at - int(woffs[j])}")


@pytest.fixture(scope="module")
def codec():
    with hbam.Codec(0) as c:
        yield c


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_consecutive_runs_merge_to_the_sorted_whole(codec, name, order):
    case = sc.CASES[name]()
    for cut, bounds in mc.cuts(case.n).items():
        runs = mc.consecutive_runs(case, order, bounds)
        for pb in mc.PART_BYTES:
            got = run_merge(codec, order, runs, pb)
            check(got, runs, pb, f"{cut} part_bytes={pb}")
            # ... which is the one-window sort of the whole case
            assert got[0] == case.expected(order)[0]
            np.testing.assert_array_equal(got[1], case.expected(order)[1])
    if name in mc.SMALL_PARTS:
        lo, hi = mc.SMALL_PARTS[name]
        m = hi - lo
        for cut, bounds in mc.cuts(m).items():
            runs = mc.consecutive_runs(case, order, [lo + b for b in bounds])
            got = run_merge(codec, order, runs, 64)
            check(got, runs, 64, f"{cut} part_bytes=64")
            assert got[0] == case.expected(order, lo, hi)[0]


@pytest.mark.parametrize("order", sc.ORDERS)
def test_library_words_equal_the_callers(codec, order):
    # long: in key order the words of its unmapped reads come from the long-hash path
    for name, cut in (("long", "k3_empty_middle"), ("mixed", "k7_one_record_runs"), ("n1", "k1")):
        case = sc.CASES[name]()
        runs = mc.consecutive_runs(case, order, mc.cuts(case.n)[cut])
        with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
            for ctx in (codec, f):
                given = run_merge(ctx, order, runs, mc.TILE, words=True)
                computed = run_merge(ctx, order, runs, mc.TILE, words=False)
                check(computed, runs, mc.TILE, f"{name} words=None")
                assert computed[0] == given[0]
                for a, b in zip(given[1:], computed[1:]):
                    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("order", sc.ORDERS)
def test_arrangements_consecutive_cuts_never_give(codec, order):
    case = sc.mixed_case()
    for what, runs in (("round robin", mc.round_robin_runs(case, order)),
                       ("reversed pieces", mc.reversed_piece_runs(case, order)),
                       ("equal words", list(mc.equal_word_runs(order)))):
        for pb in (mc.TILE, mc.BIG) if what != "equal words" else (64, mc.BIG):
            check(run_merge(codec, order, runs, pb), runs, pb, f"{what} part_bytes={pb}")
    runs = list(mc.equal_word_runs(order))
    got = run_merge(codec, order, runs, 64, words=False)  # the library's words agree that they are equal
    assert got[0] == b"".join(r.enc for r in runs)


def test_sizing_call_keeps_the_part(codec):
    case = sc.boundary_case("tile_plus1")
    runs = mc.consecutive_runs(case, "key", mc.cuts(case.n)["k2"])
    want = mc.merged(runs)
    L = hbam.lib()
    codec.merge_begin("key")
    try:
        for r in runs:
            codec.merge_add_run(r.enc, r.offs, r.words)
        heads = mc.part_heads(want[1], mc.TILE)
        assert len(heads) >= 2 and codec.merge_plan(mc.TILE) == (len(heads), case.n, len(case.enc))
        n, ln = C.c_uint64(), C.c_uint64()
        offs = np.full(case.n + 1, 7, np.uint64)
        src = np.full(case.n, 7, np.uint64)
        for _ in range(2):
            assert L.hbam_merge_next(codec._h, None, 0, offs.ctypes.data, src.ctypes.data, C.byref(n),
                                     C.byref(ln)) == hbam.OK
            assert n.value == heads[1] and ln.value == int(want[1][n.value])
            assert np.all(offs == 7) and np.all(src == 7)
        # a buffer one byte short is refused and the part stays; offs and src are optional
        out = C.create_string_buffer(ln.value)
        assert L.hbam_merge_next(codec._h, out, ln.value - 1, None, None, C.byref(n), C.byref(ln)) == hbam.E_ARG
        assert L.hbam_merge_next(codec._h, out, ln.value, None, None, C.byref(n), C.byref(ln)) == hbam.OK
        assert out.raw == want[0][:ln.value]
        rest = [codec.merge_next() for _ in heads[1:]]
        assert b"".join(p[0] for p in rest) == want[0][ln.value:]
        assert codec.merge_next() is None and codec.merge_next() is None
        assert L.hbam_merge_next(codec._h, out, ln.value, None, None, C.byref(n), C.byref(ln)) == hbam.OK
        assert (n.value, ln.value) == (0, 0)
    finally:
        codec.merge_end()


@pytest.mark.parametrize("order", sc.ORDERS)
def test_interleaved_with_decodes_and_sorts_on_one_file_ctx(order):
    case = sc.mixed_case()
    lo, runs, keep = 0, [], []
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        first = f.header()["first_record_voff"]
        f.merge_begin(order)
        for r in f.iter_batches(first, (1 << 64) - 1, max_records=900):
            m = len(r["key"])
            enc, offs, perm = f.sort_writables(order)
            want = mc.range_run(case, order, lo, lo + m)
            assert enc == want.enc
            w = sort_words(r["key"], r["ref_id"], r["pos"], order)[perm]
            np.testing.assert_array_equal(w, want.words)
            f.merge_add_run(enc, offs, w)
            runs.append(want)
            lo += m
        assert lo == case.n and len(runs) == 5
        assert f.merge_plan(mc.TILE)[1:] == (case.n, len(case.enc))
        # a sort between the plan and the parts uses none of the merge's state
        v = f.decode_span(first, (1 << 64) - 1, max_records=700)
        assert len(v["key"]) == 700
        got = f.sort_writables(order)
        assert got[0] == case.expected(order, 0, 700)[0]
        parts = []
        while True:
            part = f.merge_next()
            if part is None:
                break
            parts.append(part)
        assert b"".join(p[0] for p in parts) == case.expected(order)[0] == mc.merged(runs)[0]
        np.testing.assert_array_equal(np.concatenate([p[2] for p in parts]), mc.merged(runs)[2])
        f.merge_end()
        # the ctx serves as before
        assert len(f.decode_all()["key"]) == case.n
        assert f.encode_writables()[0] == case.enc
        f.merge_begin(order)  # and a merge can be opened again
        assert f.merge_plan() == (0, 0, 0) and f.merge_next() is None
        f.merge_end()


def test_errors(codec):
    case = sc.boundary_case("n257_mod15")
    L = hbam.lib()
    run = mc.range_run(case, "key", 0, case.n)
    with pytest.raises(hbam.HbamError) as e:
        codec.merge_begin(2)
    assert e.value.code == hbam.E_ARG and "order" in str(e.value)
    n, ln = C.c_uint64(), C.c_uint64()
    assert L.hbam_merge_next(codec._h, None, 0, None, None, C.byref(n), C.byref(ln)) == hbam.E_STATE
    with pytest.raises(hbam.HbamError) as e:
        codec.merge_add_run(run.enc, run.offs, run.words)
    assert e.value.code == hbam.E_STATE
    codec.merge_begin("key")
    try:
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_begin("key")
        assert e.value.code == hbam.E_STATE
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_next()
        assert e.value.code == hbam.E_STATE
        codec.merge_add_run(run.enc, run.offs, run.words)  # run 0
        # run 1 with two records swapped (their words differ): refused, the run and the index named
        i = int(np.flatnonzero(run.words[1:] != run.words[:-1])[3]) + 1
        w = run.words.copy()
        w[[i - 1, i]] = w[[i, i - 1]]
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(run.enc, run.offs, w)
        assert e.value.code == hbam.E_ARG and "run 1" in str(e.value) and f"record {i}" in str(e.value)
        # the swap in the bytes themselves, found by the library's own words
        o = [int(x) for x in run.offs]
        recs = [run.enc[a:b] for a, b in zip(o, o[1:])]
        recs[i - 1], recs[i] = recs[i], recs[i - 1]
        so = np.zeros(run.n + 1, np.uint64)
        so[1:] = np.cumsum([len(r) for r in recs])
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(b"".join(recs), so, None)
        assert e.value.code == hbam.E_ARG and "run 1" in str(e.value) and f"record {i}" in str(e.value)
        # offs[n] != len; a 35-byte record; offsets that go back
        bad = run.offs.copy()
        bad[-1] -= np.uint64(1)
        for words in (run.words, None):
            with pytest.raises(hbam.HbamError) as e:
                codec.merge_add_run(run.enc, bad, words)
            assert e.value.code == hbam.E_ARG and "offs[n]" in str(e.value)
        bad = run.offs.copy()
        bad[5] = bad[4] + np.uint64(35)
        assert int(bad[6]) - int(bad[5]) >= 36
        for words in (run.words, None):
            with pytest.raises(hbam.HbamError) as e:
                codec.merge_add_run(run.enc, bad, words)
            assert e.value.code == hbam.E_ARG and "record 4" in str(e.value) and "35" in str(e.value)
        bad = run.offs.copy()
        bad[[7, 8]] = bad[[8, 7]]
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(run.enc, bad, run.words)
        assert e.value.code == hbam.E_ARG and "record 7" in str(e.value)
        # none of the refused runs was added
        assert codec.merge_plan(0) == (1, case.n, len(case.enc))
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(run.enc, run.offs, run.words)
        assert e.value.code == hbam.E_STATE
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_plan(0)
        assert e.value.code == hbam.E_STATE
        assert codec.merge_next()[0] == run.enc
    finally:
        codec.merge_end()
    # no runs, and only empty runs
    for runs in ([], [mc.Run(b"", [0], [], [])] * 2):
        codec.merge_begin("coordinate")
        for r in runs:
            codec.merge_add_run(r.enc, r.offs, r.words)
        assert codec.merge_plan(64) == (0, 0, 0)
        assert L.hbam_merge_next(codec._h, None, 0, None, None, C.byref(n), C.byref(ln)) == hbam.OK
        assert (n.value, ln.value) == (0, 0) and codec.merge_next() is None
        codec.merge_end()
    # the codec still decodes
    enc, offs, _ = case.expected("key")
    assert np.array_equal(codec.decode_writables(enc, offs[:-1])["key"], case.cols["key"][case.perm("key")])


def test_runs_from_bytearray_numpy_and_memmap(codec, tmp_path):
    case = sc.boundary_case("tile_minus1")
    runs = mc.consecutive_runs(case, "coordinate", mc.cuts(case.n)["k3_empty_middle"])
    path = tmp_path / "run.spill"
    path.write_bytes(runs[2].enc)
    codec.merge_begin("coordinate")
    try:
        codec.merge_add_run(bytearray(runs[0].enc), runs[0].offs, runs[0].words)
        codec.merge_add_run(np.frombuffer(runs[1].enc, np.uint8), runs[1].offs.tolist(), runs[1].words)
        codec.merge_add_run(np.memmap(path, np.uint8, "r"), runs[2].offs, None)
        assert b"".join(p[0] for p in codec.iter_merged(mc.TILE)) == case.expected("coordinate")[0]
    finally:
        codec.merge_end()


def test_sort_bam_merges_a_multi_window_read(tmp_path, monkeypatch):
    case = sc.mixed_case()
    kw = dict(order="coordinate", granularity=100, stringency=hbam.SILENT)
    one, one_sbi = io.BytesIO(), io.BytesIO()
    assert sort_bam(case.data, one, splitting_bai=one_sbi, **kw) == case.n  # the one-window path, as before
    # the same call on windows of 64 KiB still refuses without merge=True ...
    with pytest.raises(hbam.HbamError) as e:
        sort_bam(case.data, io.BytesIO(), window_bytes=65536, **kw)
    assert e.value.code == hbam.E_STATE and "window_bytes" in str(e.value)
    # ... and merges with it: the same file, byte for byte, and the same index
    out, sbi = io.BytesIO(), io.BytesIO()
    added = []
    add_run = hbam.BamFile.merge_add_run
    monkeypatch.setattr(hbam.BamFile, "merge_add_run", lambda f, enc, offs, w=None: (added.append(len(w)),
                                                                                      add_run(f, enc, offs, w))[1])
    assert sort_bam(case.data, out, splitting_bai=sbi, window_bytes=65536, merge=True, part_bytes=100000,
                    **kw) == case.n
    assert len(added) >= 3 and sum(added) == case.n  # several windows, a run each
    data = out.getvalue()
    assert data == one.getvalue()
    assert sbi.getvalue() == one_sbi.getvalue()
    with hbam.BamFile(data, stringency=hbam.SILENT) as f:
        assert f.header_bytes() == sorted_header(bytes(case.stream.data[:case.stream.header_end]))
        assert f.build_bai(metadata=False) == bai.write_bai(data)
        assert f.decode_all()["status"] == 0
        assert f.encode_writables()[0] == case.expected("coordinate")[0]
    # a one-window file takes the same route with a single run
    out1 = io.BytesIO()
    assert sort_bam(case.data, out1, merge=True, **kw) == case.n and out1.getvalue() == data
    # runs spilled to files: the same bytes, and nothing left behind
    spill = tmp_path / "spill"
    spill.mkdir()
    dst = tmp_path / "out.bam"
    assert sort_bam(case.data, str(dst), window_bytes=65536, merge=True, spill_dir=spill, **kw) == case.n
    assert dst.read_bytes() == data and os.listdir(spill) == []
    # ... also when the sort fails after the runs were spilled
    class Full(io.BytesIO):
        def write(self, b):
            raise OSError("disk full")

    with pytest.raises(OSError):
        sort_bam(case.data, Full(), window_bytes=65536, merge=True, spill_dir=spill, **kw)
    assert os.listdir(spill) == []


def test_sort_bam_merge_in_key_order_keeps_the_header():
    case = sc.tiny_case()
    out = io.BytesIO()
    assert sort_bam(case.data, out, order="key", merge=True, part_bytes=mc.TILE, window_bytes=65536,
                    stringency=hbam.SILENT) == case.n
    with hbam.BamFile(out.getvalue(), stringency=hbam.SILENT) as f:
        assert f.header_bytes() == bytes(case.stream.data[:case.stream.header_end])
        f.decode_all()
        assert f.encode_writables()[0] == case.expected("key")[0]
