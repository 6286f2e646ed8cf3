"""GPU: hbam_format_sam (the last decoded batch as SAM text, measured, scanned
and written in HBM) against the plain-Python formatter of
tests/sam_text_cases.py, byte for byte: the text and the line starts; bounded
batches; its errors, the malformed aux forms under SILENT among them; the
device session's timed twin; and hbam.sam.view over a whole file."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import hbam
import hbam.sam
import sam_text_cases as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def check(got, case_text, case_offs):
    text, offs = got
    assert offs.dtype == np.uint64
    np.testing.assert_array_equal(offs, case_offs)
    assert len(text) == len(case_text)
    if text != case_text:  # name the first byte that differs and the line it lies in
        a, b = np.frombuffer(text, np.uint8), np.frombuffer(case_text, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        j = int(np.searchsorted(case_offs, at, side="right")) - 1
        lo = max(int(case_offs[j]), at - 20)
        raise AssertionError(f"byte {at} differs: line {j} at its byte {at - int(case_offs[j])}: "
                             f"got {text[lo:at + 12]!r} want {case_text[lo:at + 12]!r}")


def format_whole(case):
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        r = f.decode_all()
        assert r["status"] == 0 and len(r["key"]) == case.n
        return f.format_sam()


def test_test_bam_as_one_batch():
    case = tc.test_bam_case()
    check(format_whole(case), case.text, case.offs)


def test_test_sam_records_and_view():
    case = tc.test_sam_case()
    raw = open(os.path.join(GOLDEN, "test.sam"), "rb").read()
    text, offs = format_whole(case)
    check((text, offs), case.text, case.offs)
    head, body = tc.test_sam_lines()
    assert text == b"".join(x + b"\n" for x in body)
    out = io.BytesIO()
    assert hbam.sam.view(case.data, out) == 2
    assert out.getvalue() == raw


def test_field_edges():
    case = tc.edges_case()
    check(format_whole(case), case.text, case.offs)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_record_counts(n):
    case = tc.count_case(n)
    text, offs = format_whole(case)
    check((text, offs), case.text, case.offs)
    if n == 0:
        assert text == b"" and offs.tolist() == [0]


def test_long_records_between_short_ones():
    case = tc.long_between_short_case()
    check(format_whole(case), case.text, case.offs)


@pytest.mark.parametrize("mode", ["short", "long"])
def test_synthetic_reads(mode):
    case = tc.synth_case(mode)
    check(format_whole(case), case.text, case.offs)


def test_sizing_call_and_optional_offs():
    case = tc.count_case(65)
    with hbam.BamFile(case.data, stringency=hbam.SILENT) as f:
        f.decode_all()
        n = C.c_uint64()
        offs = np.full(case.n + 1, 7, np.uint64)
        assert hbam.lib().hbam_format_sam(f._h, None, 0, offs.ctypes.data, C.byref(n)) == hbam.OK
        assert n.value == len(case.text)
        np.testing.assert_array_equal(offs, case.offs)
        out = C.create_string_buffer(n.value)
        assert hbam.lib().hbam_format_sam(f._h, out, n.value, None, C.byref(n)) == hbam.OK
        assert out.raw == case.text
        # the batch is still there for the other writers
        enc, _ = f.encode_writables()
        assert len(enc) == int(np.sum(36 + case.cols["rest_len"].astype(np.int64)))


@pytest.mark.parametrize("max_records", [700, 1])
def test_bounded_batches_concatenate(max_records):
    case = tc.test_bam_case() if max_records > 1 else tc.count_case(5)
    got, starts, k = [], [], 0
    with hbam.BamFile(case.data, stringency=hbam.SILENT, batch_records=max_records) as f:
        for b in f.iter_batches(f.header()["first_record_voff"], (1 << 64) - 1, max_records):
            m = len(b["key"])
            text, offs = f.format_sam()
            lo = int(case.offs[k])
            np.testing.assert_array_equal(offs, case.offs[k:k + m + 1] - np.uint64(lo))
            got.append(text)
            starts.append(k)
            k += m
    assert k == case.n and len(got) == -(-case.n // max_records)
    assert b"".join(got) == case.text


def test_state_and_argument_errors():
    case = tc.test_bam_case()
    n = C.c_uint64(5)
    with hbam.BamFile(case.data) as f:
        # no batch yet
        assert hbam.lib().hbam_format_sam(f._h, None, 0, None, C.byref(n)) == hbam.E_STATE and n.value == 0
        f.decode_all()
        out = C.create_string_buffer(16)
        assert hbam.lib().hbam_format_sam(f._h, out, 16, None, C.byref(n)) == hbam.E_ARG
        assert n.value == len(case.text)  # the size is still reported
        text, _ = f.format_sam()
        assert text == case.text
        # a batch from hbam_decode_writables
        enc, eoffs = f.encode_writables()
        f.decode_writables(enc, eoffs[:-1])
        with pytest.raises(hbam.HbamError) as e:
            f.format_sam()
        assert e.value.code == hbam.E_STATE
        # a query batch
        f.query_unmapped(f.header()["first_record_voff"])
        f.query_next(10)
        with pytest.raises(hbam.HbamError) as e:
            f.format_sam()
        assert e.value.code == hbam.E_STATE
        # a call that moves the window forgets the batch
        f.decode_all()
        f.file_stats()
        with pytest.raises(hbam.HbamError) as e:
            f.format_sam()
        assert e.value.code == hbam.E_STATE
    # a batch from several windows
    with hbam.BamFile(case.data, window_bytes=64 << 10) as f:
        r = f.decode_all()
        assert len(r["key"]) == case.n
        with pytest.raises(hbam.HbamError) as e:
            f.format_sam()
        assert e.value.code == hbam.E_STATE


@pytest.mark.parametrize("kind", sorted(tc.MALFORMED))
def test_malformed_aux_is_a_format_error(kind):
    data = tc.malformed_case(kind)
    with hbam.BamFile(data, stringency=hbam.SILENT) as f:
        r = f.decode_all()
        assert r["status"] == 0 and len(r["key"]) == 7
        with pytest.raises(hbam.HbamError) as e:
            f.format_sam()
        assert e.value.code == hbam.E_FORMAT
        assert "record 6 " in str(e.value)
        # the good records before it format on their own
        good = f.decode_span(f.header()["first_record_voff"], (1 << 64) - 1, max_records=6)
        assert len(good["key"]) == 6
        text, offs = f.format_sam()
        assert text.count(b"\n") == 6 and int(offs[6]) == len(text)


def test_device_session_twin():
    case = tc.test_bam_case()
    g = hbam.Gpu(0)
    try:
        g.load(case.data)
        st = g.run()
        assert st["records"] == case.n
        ms, nb = g.format_sam(iters=2)
        assert nb == len(case.text) and all(t > 0 for t in ms)
        assert g.fetch_encoded(0, nb) == case.text
    finally:
        g.close()
    assert format_whole(case)[0] == case.text


@pytest.mark.parametrize("header", [True, False])
def test_view_over_three_batches(tmp_path, header):
    case = tc.test_bam_case()
    dst = str(tmp_path / "out.sam")
    src = os.path.join(GOLDEN, "test.bam")
    assert hbam.sam.view(src, dst, header=header, batch_records=800) == case.n  # 800 + 800 + 677
    got = open(dst, "rb").read()
    want = (case.header_text() if header else b"") + case.text
    assert got == want
    assert got.startswith(b"@") == header
