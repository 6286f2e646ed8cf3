"""GPU: hbam_sort_writables in queryname order (HBAM_SORT_QUERYNAME: the read
name as unsigned bytes, the flag's tie word, then batch order) against the
expected result of tests/name_cases.py, bit for bit: bytes, output starts and
permutation; the counters that show which chunks and bits were sorted; the
sizes around a workgroup; bounded batches (the cursor's padded copy as the
source); the errors; and the device session's timed call."""
import ctypes as C

import numpy as np
import pytest

import hbam
import name_cases as nc
from test_gpu_sort import check

pytestmark = pytest.mark.gpu

Q = nc.ORDER


def sort_whole(case):
    """(sort_writables' result, the ctx's name counters) of the whole file as one batch."""
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        r = f.decode_all()
        assert r["status"] == 0 and len(r["key"]) == case.n
        got = f.sort_writables(Q)
        counters = f.sort_name_counters()
        # the in-order encoding of the same batch is still the oracle's
        assert f.encode_writables()[0] == case.enc
    return got, counters


def test_chunk_edges():
    case = nc.chunk_edges_case()
    got, (present, sorted_, bits) = sort_whole(case)
    check(got, case.expected(Q))
    assert present == 32 and sorted_ == len(case.chunks_differing())


def test_unsigned_bytes():
    case = nc.unsigned_bytes_case()
    got, _ = sort_whole(case)
    check(got, case.expected(Q))


@pytest.mark.parametrize("equal_flags", [False, True], ids=["flags_differ", "flags_equal"])
def test_all_equal(equal_flags):
    case = nc.all_equal_case(equal_flags)
    got, (present, sorted_, bits) = sort_whole(case)
    check(got, case.expected(Q))
    assert present == 3 and (sorted_, bits) == (0, 0)  # 17 bytes of name: three chunks, none sorted
    if equal_flags:
        np.testing.assert_array_equal(got[2], np.arange(case.n, dtype=np.uint32))


def test_illumina():
    case = nc.illumina_case()
    got, (present, sorted_, bits) = sort_whole(case)
    check(got, case.expected(Q))
    assert present == case.chunks_present()
    assert sorted_ == len(case.chunks_differing()) < present  # the shared first chunk is skipped
    assert 0 < bits < 64 * sorted_  # and a chunk whose names differ in a few bits sorts only those


def test_random_small_alphabet():
    case = nc.random_small_alphabet_case()
    got, (present, sorted_, bits) = sort_whole(case)
    check(got, case.expected(Q))
    # 41 bytes at most: six chunks, the last of them the longest names' NUL alone, which differs from
    # nothing.  'A' ^ 'B' = 3, against the zero bytes of a shorter name 0x43: bit 7 of no byte differs
    assert present == 6 and sorted_ == len(case.chunks_differing()) == 5 and 0 < bits <= 5 * 63


def test_ends_of_stream():
    case = nc.ends_of_stream_case()
    got, _ = sort_whole(case)
    check(got, case.expected(Q))
    # the same records as bounded batches: the source is the cursor's copy, 16 bytes of padding behind it
    lo = 0
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        for r in f.iter_batches(f.header()["first_record_voff"], (1 << 64) - 1, max_records=100):
            m = len(r["key"])
            assert r["status"] == 0 and 0 < m <= 100
            check(f.sort_writables(Q), case.expected(Q, lo, lo + m))
            lo += m
    assert lo == case.n


@pytest.mark.parametrize("n", nc.SIZES)
def test_sizes(n):
    case = nc.size_case(n)
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        assert len(f.decode_all()["key"]) == n
        enc, offs, perm = got = f.sort_writables(Q)
        check(got, case.expected(Q))
        if n == 0:
            assert enc == b"" and offs.tolist() == [0] and len(perm) == 0
        # the sizing call: the same *len, offs and perm untouched
        total = C.c_uint64()
        o = np.full(n + 1, 7, np.uint64)
        p = np.full(max(n, 1), 7, np.uint32)
        rc = hbam.lib().hbam_sort_writables(f._h, hbam.SORT_QUERYNAME, None, 0, o.ctypes.data, p.ctypes.data,
                                            C.byref(total))
        assert rc == hbam.OK and total.value == len(case.enc)
        assert np.all(o == 7) and np.all(p == 7)


def test_the_other_orders_are_as_before_on_a_name_case():
    case = nc.random_small_alphabet_case()
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        f.decode_all()
        by_name = f.sort_writables(Q)
        for order in ("key", "coordinate"):
            check(f.sort_writables(order), case.expected(order))
        check(f.sort_writables(hbam.SORT_QUERYNAME), case.expected(Q))  # by number, and again after the others
        assert f.sort_writables(Q)[0] == by_name[0]


def test_errors():
    case = nc.size_case(257)
    L = hbam.lib()
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        f.decode_all()
        for order in (2, 5, 7, -1):
            with pytest.raises(hbam.HbamError) as e:
                f.sort_writables(order)
            assert e.value.code == hbam.E_ARG and "order" in str(e.value)
        n = C.c_uint64()
        total = len(case.enc)
        out = C.create_string_buffer(total)
        assert L.hbam_sort_writables(f._h, hbam.SORT_QUERYNAME, out, total - 1, None, None, C.byref(n)) == hbam.E_ARG
        assert n.value == total
        assert L.hbam_sort_writables(f._h, hbam.SORT_QUERYNAME, out, total, None, None, C.byref(n)) == hbam.OK
        assert out.raw == case.expected(Q)[0]
    # a batch of several windows
    big = nc.illumina_case()
    with hbam.BamFile(big.data, stringency=hbam.SILENT, window_bytes=65536) as f:
        assert len(f.decode_all()["key"]) == big.n
        with pytest.raises(hbam.HbamError) as e:
            f.sort_writables(Q)
        assert e.value.code == hbam.E_STATE
    # no file ctx
    with hbam.Codec(0) as c:
        n = C.c_uint64()
        assert L.hbam_sort_writables(c._h, hbam.SORT_QUERYNAME, None, 0, None, None, C.byref(n)) == hbam.E_STATE
        assert c.sort_name_counters() == (0, 0, 0)


def test_device_session_sort():
    case = nc.illumina_case()
    g = hbam.Gpu(0)
    try:
        g.set_stringency(hbam.SILENT)
        g.load(case.data)
        assert g.run()["records"] == case.n
        _, nb = g.encode_writables(iters=1)
        ms, sorted_nb = g.sort_writables(Q, iters=2)
        assert sorted_nb == nb == len(case.enc)
        assert len(ms) == 3 and all(t > 0 for t in ms)
        assert g.fetch_encoded(0, nb) == case.expected(Q)[0]
        present, sorted_, bits = g.sort_name_counters()
        assert present == case.chunks_present() and sorted_ == len(case.chunks_differing())
        split = g.sort_name_times()  # inside ms[0]: census + read-back, tie pass, chunk passes
        assert len(split) == 3 and all(t > 0 for t in split)
        for order in (2, 5):
            with pytest.raises(hbam.HbamError) as e:
                g.sort_writables(order, iters=1)
            assert e.value.code == hbam.E_ARG and "order" in str(e.value)
    finally:
        g.close()
