"""CPU: the expected side of the SAM text tests is sound, and the number
formatters of the SAM text writer agree with libc.

  - the test-side formatter (sam_text_cases.format_record) reproduces the
    alignment lines of the reference's own test.sam from their BAM encoding,
    byte for byte, and its columns over test.bam agree with the recorded
    columns of test.bam.records.npz;
  - every case of sam_text_cases builds and asserts what it is there for;
  - lib/fmt_check (csrc/hbam_fmt.h against snprintf) reports zero mismatches;
  - the C ABI declares and exports the entry points."""
import os
import subprocess

import numpy as np
import pytest

import hbam
import hbam.sam
import sam_text_cases as tc
from conftest import GOLDEN, ROOT

PKG = os.path.join(ROOT, "hadoop-bam_amd")
CHECK = os.path.join(PKG, "lib", "fmt_check")


def test_test_sam_round_trip():
    text, body = tc.test_sam_lines()
    case = tc.test_sam_case()
    assert case.lines() == [x + b"\n" for x in body]
    assert case.header_text() == text
    raw = open(os.path.join(GOLDEN, "test.sam"), "rb").read()
    assert text + case.text == raw and len(raw) == 500
    # what the fixture is there for: i and Z tags, a deletion, '=' mates
    assert b"10M1D25M" in raw and b"\tRG:Z:L1\t" in raw and b"\tMF:i:130\t" in raw and b"\t=\t" in raw


def test_formatter_agrees_with_recorded_columns_of_test_bam():
    case = tc.test_bam_case()
    rec = np.load(os.path.join(GOLDEN, "test.bam.records.npz"))
    assert case.n == 2277 == len(rec["pos"])
    lines = case.lines()
    for i, line in enumerate(lines):
        assert line.endswith(b"\n")
        f = line[:-1].split(b"\t")
        assert len(f) >= 11, i
        assert len(f[0]) == int(rec["l_read_name"][i]) - 1
        assert int(f[1]) == int(rec["flag"][i])
        ref, nref = int(rec["ref_id"][i]), int(rec["next_ref_id"][i])
        assert f[2] == (b"*" if ref < 0 else case.refs[ref])
        assert int(f[3]) == int(rec["pos"][i]) + 1 and int(f[4]) == int(rec["mapq"][i])
        n_ops = sum(1 for ch in f[5] if not 48 <= ch <= 57) if f[5] != b"*" else 0
        assert n_ops == int(rec["n_cigar"][i])
        assert f[6] == (b"*" if nref < 0 else b"=" if nref == ref else case.refs[nref])
        assert int(f[7]) == int(rec["next_pos"][i]) + 1 and int(f[8]) == int(rec["tlen"][i])
        lseq = int(rec["l_seq"][i])
        assert len(f[9]) == (lseq or 1) and len(f[10]) in (lseq, 1)
        for t in f[11:]:
            assert t[2:3] == b":" and t[4:5] == b":" and t[3:4] in b"AifZHB"
    assert int(case.offs[-1]) == len(case.text) == sum(len(x) for x in lines)


@pytest.mark.parametrize("name", ["edges", "long_between_short", "synth_short", "synth_long"] +
                         ["n%d" % n for n in (0, 1, 63, 64, 65)])
def test_cases_are_what_they_claim(name):
    if name.startswith("n"):
        case = tc.count_case(int(name[1:]))
    elif name.startswith("synth_"):
        case = tc.synth_case(name[6:])
    else:
        case = getattr(tc, name + "_case")()
    assert int(case.offs[-1]) == len(case.text)
    assert case.text.count(b"\n") >= case.n and (case.n == 0 or case.text.endswith(b"\n"))


@pytest.mark.parametrize("kind", sorted(tc.MALFORMED))
def test_malformed_cases_are_malformed(kind):
    assert tc.malformed_case(kind)


def test_float_text_is_percent_g():
    for bits, want in ((0x3DCCCCCD, "0.1"), (0x40490FDB, "3.14159"), (0x501502F9, "1e+10"), (0x2EDBE6FF, "1e-10"),
                       (0x7F7FFFFF, "3.40282e+38"), (0x00800000, "1.17549e-38"), (0x007FFFFF, "1.17549e-38"),
                       (0x497423F0, "999999"), (0x497423F8, "1e+06"), (0x497423F7, "999999"),
                       (0x49742400, "1e+06"), (0x38D1B717, "0.0001")):
        assert tc.float_text(bits) == want, hex(bits)


def test_fmt_check_reports_no_mismatch():
    subprocess.check_call(["make", "-C", PKG, "lib/fmt_check"], stdout=subprocess.DEVNULL)
    assert os.path.exists(CHECK)
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("fmt_check: ") and last.endswith(" 0 mismatches"), last
    assert int(last.split()[1]) > 2000000


def test_entry_points_declared_and_exported():
    names = hbam.exported_symbols_from_header()
    for fn in ("hbam_format_sam", "hbam_gpu_format_sam"):
        assert fn in names and hasattr(hbam.lib(), fn)
    assert hbam.lib().hbam_abi_version() == 6
    assert callable(hbam.sam.view)
