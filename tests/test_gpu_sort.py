"""GPU: hbam_sort_writables (the last decoded batch's SAMRecordWritable
encodings in key or coordinate order, sorted and gathered in HBM) against the
expected result of tests/sort_cases.py, bit for bit: bytes, output starts and
permutation; its errors; BamWriter.write_records against n write_record calls;
and the loop it closes, decode -> sort -> compress -> index (hbam.sort.sort_bam,
hbam_build_bai on its output)."""
import ctypes as C
import io

import numpy as np
import pytest

import bai
import hbam
import sort_cases as sc
from hbam.sort import sort_bam, sorted_header
from test_sort_cases import write_both_ways

pytestmark = pytest.mark.gpu

COLUMNS = ["ref_id", "pos", "l_seq", "next_ref_id", "next_pos", "tlen", "l_read_name", "mapq", "bin", "n_cigar",
           "flag", "key", "rest_len"]


def check(got, want):
    enc, offs, perm = got
    wenc, woffs, wperm = want
    np.testing.assert_array_equal(perm, wperm)
    np.testing.assert_array_equal(offs, woffs)
    assert offs.dtype == np.uint64 and perm.dtype == np.uint32
    assert len(enc) == len(wenc)
    if enc != wenc:  # name the first byte that differs and the record it lies in
        a, b = np.frombuffer(enc, np.uint8), np.frombuffer(wenc, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(woffs, at, side="right")) - 1
        raise AssertionError(f"byte {at} differs: output record {j} (batch record {int(wperm[j])}) "
                             f"at its byte {at - int(woffs[j])}")


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_sorted_encoding_is_the_expected_one(name, order):
    case = sc.CASES[name]()
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        r = f.decode_all()
        assert r["status"] == 0 and len(r["key"]) == case.n
        check(f.sort_writables(order), case.expected(order))
        # the sizing call: the same *len, offs and perm untouched, and the batch still there
        n = C.c_uint64()
        offs = np.full(case.n + 1, 7, np.uint64)
        perm = np.full(case.n, 7, np.uint32)
        rc = hbam.lib().hbam_sort_writables(f._h, hbam.SORT_ORDERS[order], None, 0, offs.ctypes.data,
                                            perm.ctypes.data, C.byref(n))
        assert rc == hbam.OK and n.value == len(case.enc)
        assert np.all(offs == 7) and np.all(perm == 7)
        # offs and perm are optional
        out = C.create_string_buffer(n.value)
        rc = hbam.lib().hbam_sort_writables(f._h, hbam.SORT_ORDERS[order], out, n.value, None, None, C.byref(n))
        assert rc == hbam.OK and out.raw == case.expected(order)[0]
        # ... and the in-order encoding of the same batch is still the oracle's
        enc, eoffs = f.encode_writables()
        assert enc == case.enc


def test_empty_batch():
    case = sc.mixed_case()
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        v = f.header()["first_record_voff"]
        assert len(f.decode_span(v, v)["key"]) == 0
        for order in sc.ORDERS:
            enc, offs, perm = f.sort_writables(order)
            assert enc == b"" and offs.tolist() == [0] and len(perm) == 0


@pytest.mark.parametrize("order", sc.ORDERS)
def test_bounded_batches_sort_on_their_own(order):
    case = sc.mixed_case()
    lo = 0
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        first = f.header()["first_record_voff"]
        for r in f.iter_batches(first, (1 << 64) - 1, max_records=1000):
            m = len(r["key"])
            assert r["status"] == 0 and 0 < m <= 1000
            np.testing.assert_array_equal(r["key"], case.cols["key"][lo:lo + m])
            check(f.sort_writables(order), case.expected(order, lo, lo + m))
            lo += m
    assert lo == case.n


def test_state_errors(test_bam):
    case = sc.mixed_case()
    n = C.c_uint64()
    L = hbam.lib()
    # no file ctx
    with hbam.Codec(0) as c:
        assert L.hbam_sort_writables(c._h, hbam.SORT_KEY, None, 0, None, None, C.byref(n)) == hbam.E_STATE
    with hbam.BamFile(test_bam) as f:
        got = f.decode_all()
        # a batch from hbam_query_next
        f.query_intervals([(int(got["ref_id"][0]), 1, int(got["pos"][1000]) + 1)],
                          [int(got["voff"][0]), len(test_bam) << 16])
        assert len(f.query_all()["key"]) > 1000
        with pytest.raises(hbam.HbamError) as e:
            f.sort_writables("key")
        assert e.value.code == hbam.E_STATE and "hbam_sort_writables needs a one-window batch" in str(e.value)
        # a batch from hbam_decode_writables
        f.decode_all()
        enc, offs = f.encode_writables()
        f.decode_writables(enc, offs[:-1])
        with pytest.raises(hbam.HbamError) as e:
            f.sort_writables("coordinate")
        assert e.value.code == hbam.E_STATE
        # ... and a decode_span after either serves again
        f.decode_all()
        check(f.sort_writables("key"), sc.test_bam_case().expected("key"))
    # a batch of several windows
    with hbam.BamFile(case.data, stringency=hbam.SILENT, window_bytes=65536) as f:
        assert len(f.decode_all()["key"]) == case.n
        with pytest.raises(hbam.HbamError) as e:
            f.sort_writables("key")
        assert e.value.code == hbam.E_STATE
    with pytest.raises(hbam.HbamError) as e:
        sort_bam(case.data, io.BytesIO(), stringency=hbam.SILENT, window_bytes=65536)
    assert e.value.code == hbam.E_STATE and "window_bytes" in str(e.value)


def test_argument_errors():
    case = sc.boundary_case("n257_mod15")
    L = hbam.lib()
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        f.decode_all()
        for order in (2, -1, 7):
            with pytest.raises(hbam.HbamError) as e:
                f.sort_writables(order)
            assert e.value.code == hbam.E_ARG and "order" in str(e.value)
        n = C.c_uint64()
        total = len(case.enc)
        out = C.create_string_buffer(total)
        assert L.hbam_sort_writables(f._h, hbam.SORT_KEY, out, total - 1, None, None, C.byref(n)) == hbam.E_ARG
        assert n.value == total
        assert L.hbam_sort_writables(f._h, hbam.SORT_KEY, out, total, None, None, C.byref(n)) == hbam.OK
        assert out.raw == case.expected("key")[0]


@pytest.mark.parametrize("buffer_blocks", [1, 4])
def test_write_records_equals_single_calls(buffer_blocks):
    import hbam.writer as W
    # 1,200 records: seven stock blocks, so one block per GPU call, and four, both cut the records
    single, bulk = write_both_ways(W, sc.mixed_case(), "coordinate", buffer_blocks, 100, count=1200)
    assert bulk == single and len(single[0]) > 5 * 20000 and len(single[1]) == 8 * (1 + 12 + 1)


def test_sort_bam_closes_the_loop():
    case = sc.mixed_case()
    # before: the index builder refuses the unsorted input
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        with pytest.raises(hbam.HbamError) as e:
            f.build_bai(metadata=False)
        assert e.value.code == hbam.E_FORMAT
        header = f.header_bytes()
    assert header == bytes(case.stream.data[:case.stream.header_end])
    out, sbi = io.BytesIO(), io.BytesIO()
    assert sort_bam(case.data, out, order="coordinate", splitting_bai=sbi, granularity=100,
                    stringency=hbam.SILENT) == case.n
    data = out.getvalue()
    perm = case.expected("coordinate")[2]
    with hbam.BamFile(data, stringency=hbam.SILENT) as f:
        assert f.header_bytes() == sorted_header(header)
        got = f.decode_all()
        assert got["status"] == 0
        for name in COLUMNS:
            want = case.cols[name][perm]
            if name == "bin":  # write() stores indexBin 0 for a record without a reference
                want = np.where(case.cols["ref_id"][perm] < 0, 0, want)
            np.testing.assert_array_equal(got[name], want, err_msg=name)
        # its records, encoded in file order, are the expected sorted encoding
        assert f.encode_writables()[0] == case.expected("coordinate")[0]
        assert f.build_bai(metadata=False) == bai.write_bai(data)
        assert f.splitting_index(100) == sbi.getvalue()


def test_sort_bam_key_order_keeps_the_header(tmp_path):
    case = sc.tiny_case()
    src, dst = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(case.data)
    assert sort_bam(str(src), str(dst), order="key", eof=False, stringency=hbam.SILENT) == case.n
    data = dst.read_bytes()
    assert not data.endswith(hbam.writer.BGZF_EOF_BLOCK)
    with hbam.BamFile(data + hbam.writer.BGZF_EOF_BLOCK, stringency=hbam.SILENT) as f:
        assert f.header_bytes() == bytes(case.stream.data[:case.stream.header_end])
        f.decode_all()
        assert f.encode_writables()[0] == case.expected("key")[0]


@pytest.mark.parametrize("order", sc.ORDERS)
def test_device_session_sort(order):
    case = sc.mixed_case()
    g = hbam.Gpu(0)
    try:
        g.set_stringency(hbam.SILENT)
        g.load(case.data)
        assert g.run()["records"] == case.n
        _, nb = g.encode_writables(iters=1)
        ms, sorted_nb = g.sort_writables(order, iters=2)
        assert sorted_nb == nb == len(case.enc)
        assert len(ms) == 3 and all(t > 0 for t in ms)
        assert g.fetch_encoded(0, nb) == case.expected(order)[0]
        with pytest.raises(hbam.HbamError) as e:
            g.sort_writables(5, iters=1)
        assert e.value.code == hbam.E_ARG
    finally:
        g.close()
