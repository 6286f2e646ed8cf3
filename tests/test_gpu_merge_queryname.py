"""GPU: hbam_merge_* in queryname order (the runs' names copied into HBM, the
order planned by the same chunk sort as the window sort) against the one-window
sort's expected result of tests/name_cases.py, bit for bit; ties across runs;
a run that is out of order; words refused; codec and file contexts; and
hbam.sort.sort_bam(order="queryname") with and without merge=True."""
import io

import numpy as np
import pytest

import hbam
import name_cases as nc
from hbam.sort import sort_bam, sorted_header
from test_gpu_merge import run_merge

pytestmark = pytest.mark.gpu

Q = nc.ORDER


class _Run:
    def __init__(self, enc, offs):
        self.enc, self.offs, self.words = enc, offs, None


def merge_and_check(ctx, case, bounds, part_bytes, what):
    runs = [_Run(*r) for r in nc.runs_of(case, bounds)]
    enc, offs, src, heads = run_merge(ctx, Q, runs, part_bytes, words=False)
    wenc, woffs, _ = case.expected(Q, bounds[0], bounds[-1])
    np.testing.assert_array_equal(src, nc.merged_src(case, bounds), err_msg=what)
    np.testing.assert_array_equal(offs, woffs, err_msg=what)
    assert enc == wenc, what
    o = woffs[:-1].astype(np.int64) // part_bytes  # record j belongs to part offs[j] // part_bytes
    assert len(heads) == (1 + int(np.count_nonzero(o[1:] != o[:-1])) if len(o) else 0), what
    return src


@pytest.fixture(scope="module")
def codec():
    with hbam.Codec(0) as c:
        yield c


@pytest.mark.parametrize("name", ["random_small_alphabet", "all_equal"])
def test_consecutive_runs_merge_to_the_sorted_whole(codec, name):
    case = nc.random_small_alphabet_case() if name == "random_small_alphabet" else nc.all_equal_case()
    for cut, bounds in nc.cuts(case.n).items():
        merge_and_check(codec, case, bounds, 4096, f"{name} {cut} part_bytes=4096")
    if name == "random_small_alphabet":
        # the plan's order went through the same chunk sort (the sixth chunk is the longest names' NUL alone)
        assert codec.sort_name_counters()[:2] == (6, len(case.chunks_differing())) == (6, 5)
    else:
        assert codec.sort_name_counters() == (3, 0, 0)
    # parts of 64 bytes: every record a part of its own (a few hundred records: a launch set per part)
    lo, m = (1000, 300) if name == "random_small_alphabet" else (0, 300)
    for cut, bounds in nc.cuts(m, lo).items():
        merge_and_check(codec, case, bounds, 64, f"{name} {cut} part_bytes=64")


def test_equal_name_and_tie_goes_to_the_earlier_run(codec):
    case = nc.all_equal_case(True)  # one name, one flag
    bounds = nc.cuts(case.n)["k16_one_empty"]
    src = merge_and_check(codec, case, bounds, 4096, "all equal")
    assert np.all(np.diff(src.astype(np.int64)) > 0)  # run-major, each run in its own order
    assert sorted(set((src >> np.uint64(32)).tolist())) == [r for r in range(16) if r != 5]


def test_codec_and_file_ctx_agree():
    case = nc.chunk_edges_case()
    bounds = nc.cuts(case.n)["k3_empty_middle"]
    with hbam.Codec(0) as c, hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        for ctx in (c, f):
            merge_and_check(ctx, case, bounds, 4096, type(ctx).__name__)
        # the file ctx decodes and sorts as before afterwards
        assert len(f.decode_all()["key"]) == case.n
        assert f.sort_writables(Q)[0] == case.expected(Q)[0]


def test_errors(codec):
    case = nc.random_small_alphabet_case()
    lo, hi = 0, 400
    enc, offs, perm = case.expected(Q, lo, hi)
    with pytest.raises(hbam.HbamError) as e:
        codec.merge_begin(2)
    assert e.value.code == hbam.E_ARG and "order" in str(e.value)
    codec.merge_begin(Q)
    try:
        # there are no words in this order
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(enc, offs, np.zeros(hi - lo, np.uint64))
        assert e.value.code == hbam.E_ARG and "words" in str(e.value)
        codec.merge_add_run(enc, offs)  # run 0
        # run 1 with two records swapped whose (name, tie) differ: refused, the run and the index named
        key = [(case.raw[lo + int(i)].rstrip(b"\0"), int(case.ties[lo + int(i)])) for i in perm]
        i = [j for j in range(1, len(key)) if key[j] != key[j - 1]][7]
        o = [int(x) for x in offs]
        recs = [enc[a:b] for a, b in zip(o, o[1:])]
        recs[i - 1], recs[i] = recs[i], recs[i - 1]
        so = np.zeros(len(recs) + 1, np.uint64)
        so[1:] = np.cumsum([len(r) for r in recs])
        with pytest.raises(hbam.HbamError) as e:
            codec.merge_add_run(b"".join(recs), so)
        assert e.value.code == hbam.E_ARG and "run 1" in str(e.value) and f"record {i} " in str(e.value)
        # the merge goes on without the refused run: run 1 is the next one added
        enc2, offs2, _ = case.expected(Q, hi, hi + 300)
        codec.merge_add_run(enc2, offs2)
        assert codec.merge_plan(4096)[1:] == (700, len(enc) + len(enc2))
        got = b"".join(p[0] for p in iter(codec.merge_next, None))
        assert got == case.expected(Q, lo, hi + 300)[0]
    finally:
        codec.merge_end()
    # no runs, and only empty runs
    for runs in ([], [(b"", [0])] * 2):
        codec.merge_begin(Q)
        for r in runs:
            codec.merge_add_run(*r)
        assert codec.merge_plan(64) == (0, 0, 0) and codec.merge_next() is None
        codec.merge_end()


def _records_of(data):
    with hbam.BamFile(data, stringency=hbam.SILENT) as f:
        header = f.header_bytes()
        assert f.decode_all()["status"] == 0
        return header, f.encode_writables()[0]


def test_sort_bam_by_name(tmp_path):
    case = nc.illumina_case()
    header = bytes(case.stream.data[:case.stream.header_end])
    out, sbi = io.BytesIO(), io.BytesIO()
    assert sort_bam(case.data, out, order="queryname", splitting_bai=sbi, granularity=100,
                    stringency=hbam.SILENT) == case.n
    got_header, got = _records_of(out.getvalue())
    assert got_header == sorted_header(header, "queryname") and b"SO:queryname" in got_header
    assert got == case.expected(Q)[0]
    with hbam.BamFile(out.getvalue(), stringency=hbam.SILENT) as f:
        assert f.splitting_index(100) == sbi.getvalue()
    # path in, path out
    src, dst = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(case.data)
    assert sort_bam(str(src), str(dst), order="queryname", stringency=hbam.SILENT) == case.n
    assert dst.read_bytes() == out.getvalue()


def test_sort_bam_by_name_merges_a_multi_window_read(tmp_path, monkeypatch):
    case = nc.illumina_case()
    kw = dict(order="queryname", granularity=100, stringency=hbam.SILENT)
    one = io.BytesIO()
    assert sort_bam(case.data, one, **kw) == case.n
    with pytest.raises(hbam.HbamError) as e:
        sort_bam(case.data, io.BytesIO(), window_bytes=65536, **kw)
    assert e.value.code == hbam.E_STATE and "window_bytes" in str(e.value)
    # the runs go to a merge on a codec ctx (the run's decode would end the split the file ctx is reading)
    added = []
    add_run = hbam.Codec.merge_add_run
    monkeypatch.setattr(hbam.Codec, "merge_add_run", lambda c, enc, offs, w=None: (added.append((len(offs) - 1, w)),
                                                                                   add_run(c, enc, offs, w))[1])
    out = io.BytesIO()
    assert sort_bam(case.data, out, window_bytes=65536, merge=True, part_bytes=32768, **kw) == case.n
    assert len(added) >= 3 and sum(a[0] for a in added) == case.n  # several windows, a run each
    assert all(a[1] is None for a in added)  # and no words
    assert out.getvalue() == one.getvalue()
    # runs spilled to files: the same bytes, and nothing left behind
    spill = tmp_path / "spill"
    spill.mkdir()
    out2 = io.BytesIO()
    assert sort_bam(case.data, out2, window_bytes=65536, merge=True, part_bytes=32768, spill_dir=spill,
                    **kw) == case.n
    assert out2.getvalue() == one.getvalue() and list(spill.iterdir()) == []
