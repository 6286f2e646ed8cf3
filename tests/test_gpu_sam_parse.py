"""GPU: hbam_parse_sam (SAM text into BAM records: lines found, measured,
scanned and written in HBM) against the plain-Python encoder of
tests/sam_parse_cases.py, byte for byte: the records and their starts; the round
trip through hbam_format_sam on a file ctx; chunked input; its errors, one
malformed line of every kind among six good ones; the dictionary; and
hbam.sam.to_bam over whole files."""
import io
import os
import struct

import numpy as np
import pytest

import hbam
import hbam.sam
import orc
import sam_parse_cases as pc
import sam_text_cases as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def check(got, case):
    enc, offs, consumed = got
    assert offs.dtype == np.uint64 and consumed == len(case.text)
    if len(offs) == len(case.offs):
        k = np.flatnonzero(offs != case.offs)
        assert len(k) == 0, f"record {int(k[0]) - 1} has {int(offs[k[0]] - offs[k[0] - 1])} bytes, want " \
                            f"{int(case.offs[k[0]] - case.offs[k[0] - 1])}"
    np.testing.assert_array_equal(offs, case.offs)
    assert len(enc) == len(case.enc)
    if enc != case.enc:  # name the first byte that differs and the line it lies in
        a, b = np.frombuffer(enc, np.uint8), np.frombuffer(case.enc, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        j = case.line_of_byte(at)
        lo = max(int(case.offs[j]), at - 12)
        raise AssertionError(f"byte {at} differs: line {j} at its record's byte {at - int(case.offs[j])}: "
                             f"got {enc[lo:at + 8].hex()} want {case.enc[lo:at + 8].hex()}")


def parse_whole(case):
    with hbam.Codec() as c:
        c.parse_sam_dict(case.refs)
        return c.parse_sam(case.text)


def test_test_bam_text():
    check(parse_whole(pc.test_bam_case()), pc.test_bam_case())


def test_test_sam_lines():
    check(parse_whole(pc.test_sam_case()), pc.test_sam_case())


def test_field_edges():
    check(parse_whole(pc.edges_case()), pc.edges_case())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_line_counts(n):
    case = pc.count_case(n)
    got = parse_whole(case)
    check(got, case)
    if n == 0:
        assert got[0] == b"" and got[1].tolist() == [0]


def test_long_lines_between_short_ones():
    check(parse_whole(pc.long_between_short_case()), pc.long_between_short_case())


def test_round_trip_on_a_file_ctx():
    data = open(os.path.join(GOLDEN, "test.bam"), "rb").read()
    with hbam.BamFile(data) as f:
        r = f.decode_all()
        text, toffs = f.format_sam()
        want, woffs = f.encode_writables()
        enc, offs, consumed = f.parse_sam(text)  # the file's own dictionary
        assert consumed == len(text) and enc == want
        np.testing.assert_array_equal(offs, woffs)
        # the last batch is still the span's: the formatter serves it after the parse
        again, _ = f.format_sam()
        assert again == text
        back = f.decode_writables(enc, offs[:-1])
        for k in ("key", "ref_id", "pos", "l_seq", "next_ref_id", "next_pos", "tlen", "l_read_name", "mapq", "bin",
                  "n_cigar", "flag", "rest_len"):
            np.testing.assert_array_equal(back[k], r[k], err_msg=k)


@pytest.mark.parametrize("chunk", [1000, 1])
def test_chunks_with_carry_over(chunk):
    case = pc.test_bam_case() if chunk > 1 else pc.count_case(5)
    encs, n, carry, calls = [], 0, b"", 0
    with hbam.Codec() as c:
        c.parse_sam_dict(case.refs)
        for p in range(0, len(case.text), chunk):
            buf = carry + case.text[p:p + chunk]
            enc, offs, used = c.parse_sam(buf, final=False)
            assert used <= len(buf) and (used == 0 or buf[used - 1:used] == b"\n") and b"\n" not in buf[used:]
            assert int(offs[-1]) == len(enc) and len(offs) - 1 == buf[:used].count(b"\n")
            encs.append(enc)
            n += len(offs) - 1
            carry = buf[used:]
            calls += 1
        assert carry == b""
    assert calls >= 3 and n == case.n and b"".join(encs) == case.enc


def test_last_line_without_newline():
    case = pc.count_case(5)
    text = case.text[:-1]
    with hbam.Codec() as c:
        c.parse_sam_dict(case.refs)
        enc, offs, used = c.parse_sam(text, final=False)
        assert len(offs) == 5 and used == int(tc.count_case(5).offs[4]) and enc == case.enc[:int(case.offs[4])]
        enc, offs, used = c.parse_sam(text, final=True)
        assert used == len(text) and enc == case.enc
        np.testing.assert_array_equal(offs, case.offs)
        enc, offs, used = c.parse_sam(b"no newline at all", final=False)
        assert (enc, offs.tolist(), used) == (b"", [0], 0)


@pytest.mark.parametrize("kind", sorted(pc.MALFORMED))
def test_malformed_line_is_a_format_error(kind):
    text = pc.malformed_text(kind)
    good = b"".join(x + b"\n" for x in pc.GOOD)
    with hbam.Codec() as c:
        c.parse_sam_dict(pc.EDGE_REFS)
        with pytest.raises(hbam.HbamError) as e:
            c.parse_sam(text)
        assert e.value.code == hbam.E_FORMAT
        assert "line 6 " in str(e.value)
        r = hbam.SamRecords()
        buf = np.frombuffer(text, np.uint8)
        assert hbam.lib().hbam_parse_sam(c._h, buf.ctypes.data, len(buf), 1, r) == hbam.E_FORMAT and r.n == 0
        # the six good lines parse on their own
        want = pc.encode_text(good, pc.EDGE_REFS)
        enc, offs, used = c.parse_sam(good)
        assert enc == want[0] and used == len(good)
        np.testing.assert_array_equal(offs, want[1])


def test_lowest_bad_line_is_named():
    bad = pc.MALFORMED["cigar_bad_op"] + b"\n"
    good = b"".join(x + b"\n" for x in pc.GOOD)
    with hbam.Codec() as c:
        c.parse_sam_dict(pc.EDGE_REFS)
        with pytest.raises(hbam.HbamError) as e:
            c.parse_sam(good * 20 + bad + good * 20 + bad * 30)
        assert "line 120 CIGAR" in str(e.value)


def test_dictionary():
    line = pc.GOOD[0] + b"\n"
    star = line.replace(b"chr1", b"*")
    with hbam.Codec() as c:
        # no dictionary: only "*" and "="
        with pytest.raises(hbam.HbamError) as e:
            c.parse_sam(line)
        assert e.value.code == hbam.E_FORMAT and "line 0 RNAME" in str(e.value)
        assert c.parse_sam(star)[0] == pc.encode_line(star[:-1], [])
        c.parse_sam_dict([b"chr0", b"chr1"])
        assert c.parse_sam(line)[0] == pc.encode_line(line[:-1], [b"chr0", b"chr1"])
        # a name that appears twice resolves to its lowest index
        names = [b"b", b"chr1", b"a", b"chr1", b"chr1", b"a"]
        c.parse_sam_dict(names)
        enc = c.parse_sam(line + line.replace(b"chr1", b"a"))[0]
        assert enc == pc.encode_line(line[:-1], names) + pc.encode_line(line[:-1].replace(b"chr1", b"a"), names)
        assert struct.unpack_from("<i", enc, 4)[0] == 1
        c.parse_sam_dict(None)  # a codec ctx has no dictionary of its own to go back to
        with pytest.raises(hbam.HbamError):
            c.parse_sam(line)
        c.parse_sam_dict([])
        with pytest.raises(hbam.HbamError):
            c.parse_sam(line)
    data = open(os.path.join(GOLDEN, "test.bam"), "rb").read()
    case = pc.test_bam_case()
    first = case.text[:case.text.index(b"\n") + 1]
    with hbam.BamFile(data) as f:
        assert f.parse_sam(first)[0] == case.enc[:int(case.offs[1])]
        f.parse_sam_dict([b"other"])
        with pytest.raises(hbam.HbamError):
            f.parse_sam(first)
        f.parse_sam_dict(None)  # the file's dictionary again
        assert f.parse_sam(first)[0] == case.enc[:int(case.offs[1])]


def _inflate(data):
    s = orc.Stream(data, stringency=orc.SILENT)
    rc, cols = s.decode_all()
    assert rc == 0
    return bytes(s.data), cols


def test_to_bam_of_test_sam_and_back():
    raw = open(os.path.join(GOLDEN, "test.sam"), "rb").read()
    out = io.BytesIO()
    assert hbam.sam.to_bam(raw, out) == 2
    back = io.BytesIO()
    assert hbam.sam.view(out.getvalue(), back) == 2
    assert back.getvalue() == raw


def test_to_bam_of_test_bam_text_in_chunks(tmp_path):
    src = os.path.join(GOLDEN, "test.bam")
    sam = io.BytesIO()
    assert hbam.sam.view(src, sam) == 2277
    dst = str(tmp_path / "out.bam")
    chunk = len(sam.getvalue()) // 3 - 100  # four chunks
    assert hbam.sam.to_bam(sam.getvalue(), dst, chunk_bytes=chunk) == 2277
    got, cols = _inflate(open(dst, "rb").read())
    want, wcols = _inflate(open(src, "rb").read())
    assert tc.header_refs(got) == tc.header_refs(want)
    g0, w0 = int(cols["offset"][0]), int(wcols["offset"][0])
    assert got[g0:] == want[w0:]  # the records, byte for byte
    assert got[8 + struct.unpack_from("<i", got, 4)[0]:g0] == want[8 + struct.unpack_from("<i", want, 4)[0]:w0]
    with hbam.BamFile(path=dst) as f:
        assert hbam.bai_summary(f.build_bai())["n_ref"] == len(tc.header_refs(want))


def test_times_are_positive():
    case = pc.test_bam_case()
    with hbam.Codec() as c:
        c.parse_sam_dict(case.refs)
        c.parse_sam(case.text)
        ms = c.parse_sam_times()
        assert len(ms) == 4 and all(t > 0 for t in ms)
