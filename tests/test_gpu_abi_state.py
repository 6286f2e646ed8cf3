"""GPU: which calls leave a ctx's last batch servable from HBM.  One table of
how the ctx got here x consumer: hbam_encode_writables, hbam_sort_writables and
hbam_format_sam (size queries) and hbam_reader_position(0).  Every cell asserts
the return code; an E_STATE cell of the three batch-to-bytes calls the text
"<function> needs a one-window batch", a size query *len; the OK cells of the
whole file and of its first 100 records the bytes of tests/sort_cases.py and
tests/sam_text_cases.py.

The states behind the table (hbam_abi.cpp): none, span, query,
writables.  A window-moving call (file_stats, decode_span_device, ...) takes
span to none and leaves query and writables as they are; only the next
hbam_decode_span serves again."""
import ctypes as C

import pytest

import hbam
import sam_text_cases as tc
import sort_cases as sc
from test_gpu_sort import check

pytestmark = pytest.mark.gpu

END = (1 << 64) - 1
BOUNDED = 100
OK, E = "ok", "state"


def first_voff(f):
    return f.header()["first_record_voff"]


def decode_all(f):
    assert len(f.decode_all()["key"]) == sc.test_bam_case().n


def decode_bounded(f):
    assert len(f.decode_span(first_voff(f), END, max_records=BOUNDED)["key"]) == BOUNDED


def file_stats(f):
    f.file_stats()


def query_batch(f):
    f.query_unmapped(first_voff(f))
    f.query_next(10)


def empty_query_batch(f):
    # test.bam is sorted: nothing overlaps the bases before its first record's start
    got = f.decode_all()
    ref, start0 = int(got["ref_id"][0]), int(got["pos"][0])
    assert ref >= 0 and start0 >= 1
    f.query_intervals([(ref, 1, start0)], [int(got["voff"][0]), f.size << 16])
    assert len(f.query_next()["key"]) == 0


def writables_batch(f):
    enc, offs = f.encode_writables()
    assert len(f.decode_writables(enc, offs[:-1])["key"]) == sc.test_bam_case().n


def device_decode(f):
    assert f.decode_span_device(first_voff(f), END)["records"] == sc.test_bam_case().n


# row: (open options, the calls that bring the ctx here, records of the batch the OK cells serve,
#       encode / sort, format_sam, reader_position)
ROWS = {
    "S0_fresh": ({}, [], 0, OK, E, E),
    "S1_decode_all": ({}, [decode_all], None, OK, OK, OK),
    "S2_bounded_batch": ({}, [decode_bounded], BOUNDED, OK, OK, OK),
    "S3_several_windows": ({"window_bytes": 64 << 10}, [decode_all], None, E, E, OK),
    "S4_span_then_file_stats": ({}, [decode_all, file_stats], None, E, E, E),
    "S5_query": ({}, [query_batch], None, E, E, E),
    "S6_query_then_file_stats": ({}, [query_batch, file_stats], None, E, E, E),
    "S7_empty_query_then_file_stats": ({}, [empty_query_batch, file_stats], None, E, E, E),
    "S8_writables": ({}, [decode_all, writables_batch], None, E, E, E),
    "S9_writables_then_file_stats": ({}, [decode_all, writables_batch, file_stats], None, E, E, E),
    "S10_span_then_device_decode": ({}, [decode_all, device_decode], None, E, E, E),
}
# S11: a decode_span after any of S5-S10 serves as S1 does
for _name in [k for k in ROWS if k.split("_")[0] in ("S5", "S6", "S7", "S8", "S9", "S10")]:
    ROWS["S11_after_" + _name] = ({}, ROWS[_name][1] + [decode_all], None, OK, OK, OK)


def size_query(name, h):
    """(rc, *len) of the size query of one of the three batch-to-bytes calls."""
    L = hbam.lib()
    n = C.c_uint64(5)
    if name == "hbam_sort_writables":
        rc = L.hbam_sort_writables(h, hbam.SORT_KEY, None, 0, None, None, C.byref(n))
    else:
        rc = getattr(L, name)(h, None, 0, None, C.byref(n))
    return rc, n.value


def last_error(h):
    return hbam.lib().hbam_last_error(h).decode(errors="replace")


def cells(h, m, enc_sort, sam, position):
    """Every cell of one row that is not what the table says ([] = the row holds).
    m = the records of the batch the OK cells serve."""
    enc_case, text_case = sc.test_bam_case(), tc.test_bam_case()
    want_len = {"hbam_encode_writables": int(enc_case.offs[m]), "hbam_sort_writables": int(enc_case.offs[m]),
                "hbam_format_sam": int(text_case.offs[m])}
    bad = []
    for name, want in (("hbam_encode_writables", enc_sort), ("hbam_sort_writables", enc_sort),
                       ("hbam_format_sam", sam)):
        rc, n = size_query(name, h)
        print(f"{name}: rc {rc} len {n} error {last_error(h)!r}")
        if want == OK:
            if (rc, n) != (hbam.OK, want_len[name]):
                bad.append(f"{name}: rc {rc} len {n}, want OK len {want_len[name]}")
        elif rc != hbam.E_STATE or n != 0 or f"{name} needs a one-window batch" not in last_error(h):
            bad.append(f"{name}: rc {rc} len {n} error {last_error(h)!r}, want E_STATE with its text")
    pos = C.c_uint64(5)
    rc = hbam.lib().hbam_reader_position(h, 0, C.byref(pos))
    print(f"hbam_reader_position: rc {rc} pos {pos.value} error {last_error(h)!r}")
    if position == OK:
        if rc != hbam.OK or pos.value == 0:
            bad.append(f"hbam_reader_position: rc {rc} pos {pos.value}, want OK")
    elif rc != hbam.E_STATE or pos.value != 0 or "hbam_reader_position needs the last call" not in last_error(h):
        bad.append(f"hbam_reader_position: rc {rc} pos {pos.value} error {last_error(h)!r}, want E_STATE")
    return bad


@pytest.mark.parametrize("row", list(ROWS))
def test_state_table(row, test_bam):
    opts, steps, m, enc_sort, sam, position = ROWS[row]
    enc_case, text_case = sc.test_bam_case(), tc.test_bam_case()
    m = enc_case.n if m is None else m
    with hbam.BamFile(test_bam, **opts) as f:
        for step in steps:
            step(f)
        assert cells(f._h, m, enc_sort, sam, position) == []
        if (enc_sort, sam) == (OK, OK) and m:  # the bytes too, and no consumer changed the state
            assert f.encode_writables()[0] == enc_case.enc[:int(enc_case.offs[m])]
            check(f.sort_writables("key"), enc_case.expected("key", 0, m))
            text, offs = f.format_sam()
            assert text == text_case.text[:int(text_case.offs[m])]
            assert offs.tolist() == text_case.offs[:m + 1].tolist()
            assert cells(f._h, m, enc_sort, sam, position) == []


def test_codec_ctx_has_no_batch():
    """S12: a ctx with no file (hbam_open_codec) is refused before the state is looked at: no text."""
    with hbam.Codec(0) as c:
        for name in ("hbam_encode_writables", "hbam_sort_writables", "hbam_format_sam"):
            assert size_query(name, c._h) == (hbam.E_STATE, 0), name
        pos = C.c_uint64(5)
        assert hbam.lib().hbam_reader_position(c._h, 0, C.byref(pos)) == hbam.E_STATE and pos.value == 0
        assert last_error(c._h) == ""
