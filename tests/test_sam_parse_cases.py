"""CPU checks of the SAM parse tests' expected side (sam_parse_cases), of
hbam.sam.split_text and hbam_sam_header_to_bam (host code), and of the float
reader in csrc/hbam_fmt.h against glibc (lib/parse_check).  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hbam
import hbam.sam
import sam_parse_cases as spc
import sam_text_cases as stc
from conftest import GOLDEN, ROOT


def test_test_bam_records_come_back_byte_for_byte():
    case = spc.test_bam_case()
    want = spc.test_bam_records()
    assert case.n == len(want) == 2277
    for i, r in enumerate(want):
        got = case.enc[int(case.offs[i]):int(case.offs[i + 1])]
        assert got == r, "record %d" % i


def test_float_texts():
    assert spc.float_bits(b"1.0000000596046448") == 0x3F800001
    assert spc.float_bits(b"3.4028236e38") == 0x7F800000 and spc.float_bits(b"3.40282356e38") == 0x7F7FFFFF
    assert spc.float_bits(b"-0") == 0x80000000
    for bits in stc.FLOAT_BITS:
        # what the formatter prints parses to the float nearest to that text: the float itself when six
        # digits name it, else one that prints the same; a six-digit text is far from every midpoint of
        # two floats on the double's scale, so rounding it through a double gives the same float
        text = stc.float_text(bits).encode()
        got = spc.float_bits(text)
        if text == b"nan":
            assert got == 0x7FC00000
            continue
        assert got == int(np.float32(float(text)).view(np.uint32)), text
        assert stc.float_text(got).encode() == text
        if float(np.uint32(bits).view(np.float32)) == float(text):
            assert got == bits, hex(bits)


def test_cases_build():
    assert spc.test_sam_case().n == 2
    assert spc.edges_case().n > 40
    for n in (0, 1, 63, 64, 65):
        assert spc.count_case(n).n == n
    assert spc.long_between_short_case().n == 23


@pytest.mark.parametrize("kind", sorted(spc.MALFORMED))
def test_malformed_cases_are_refused_by_the_encoder(kind):
    assert spc.malformed_text(kind).count(b"\n") == 7


def _check_partition(raw, n_header):
    lines = raw.split(b"\n")
    assert lines.pop() == b""
    body = [x + b"\n" for x in lines[n_header:]]
    for cut in range(len(raw) + 1):
        a = hbam.sam.split_text(raw, 0, cut)
        b = hbam.sam.split_text(raw, cut, len(raw) - cut)
        assert a + b == body, cut
    # three splits
    for c1, c2 in ((1, 2), (len(raw) // 3, 2 * len(raw) // 3), (len(raw) - 2, len(raw) - 1)):
        parts = hbam.sam.split_text(raw, 0, c1) + hbam.sam.split_text(raw, c1, c2 - c1) + \
            hbam.sam.split_text(raw, c2, len(raw) - c2)
        assert parts == body


def test_split_text_partitions_test_sam():
    raw = open(os.path.join(GOLDEN, "test.sam"), "rb").read()
    head, body = stc.test_sam_lines()
    _check_partition(raw, head.count(b"\n"))
    assert hbam.sam.split_text(raw, 0, len(raw)) == [x + b"\n" for x in body]


def test_split_text_partitions_65_lines():
    text = b"@HD\tVN:1.5\n@SQ\tSN:chr1\tLN:1000\n" + spc.count_case(65).text
    _check_partition(text, 2)
    # a last line without its newline belongs to the split its first byte lies in
    cut = text[:-1]
    k = cut.rfind(b"\n") + 1
    assert hbam.sam.split_text(cut, k, len(cut) - k) == [cut[k:]] and hbam.sam.split_text(cut, k + 1, 5) == []


def test_sam_header_to_bam():
    head, _ = stc.test_sam_lines()
    h = hbam.sam_header_to_bam(head)
    assert h == stc.bam_header(head, [(b"chr21", 62435964)])
    text = b"@HD\tVN:1.5\n@SQ\tLN:5\tXX:y\tSN:b\n@CO\t@SQ\tSN:no\tLN:1\n@SQ\tSN:a\tLN:2147483647\r\n@SQ\tSN:b\tLN:0"
    assert hbam.sam_header_to_bam(text) == stc.bam_header(text, [(b"b", 5), (b"a", 2147483647), (b"b", 0)])
    assert hbam.sam_header_to_bam(b"") == b"BAM\x01" + struct.pack("<ii", 0, 0)
    for bad in (b"@SQ\tLN:5\n", b"@SQ\tSN:a\n", b"@SQ\tSN:a\tLN:5x\n", b"@SQ\tSN:a\tLN:\n", b"@SQ\tSN:\tLN:5\n",
                b"@SQ\tSN:a\tLN:-5\n", b"@SQ\tSN:a\tLN:2147483648\n", b"@SQ\tSN:a\tLN:99999999999999999999999\n"):
        with pytest.raises(hbam.HbamError) as e:
            hbam.sam_header_to_bam(bad)
        assert e.value.code == hbam.E_FORMAT, bad


def test_float_reader_against_strtof():
    exe = os.path.join(ROOT, "hadoop-bam_amd", "lib", "parse_check")
    assert os.path.exists(exe), "lib/parse_check is not built (make -C hadoop-bam_amd)"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, bad = [int(x) for x in r.stdout.replace(",", "").split() if x.isdigit()]
    assert bad == 0 and checked > 4000000
