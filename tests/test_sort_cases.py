"""CPU: the sort tests' inputs and expected results (tests/sort_cases.py) are
what the GPU tests take them for, and the host pieces of the sort feature that
need no GPU: hbam.sort.sorted_header, BamWriter.write_records' host logic (the
oracle's compressor standing in for the GPU call, as in test_writer) and the
ABI's answer to a NULL ctx."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

import bai
import hbam
import orc
import sort_cases as sc
from hbam.sort import sorted_header


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_expected_permutation_computed_a_second_way(name, order):
    case = sc.CASES[name]()  # (asserts the case's own preconditions)
    enc, offs, perm = case.expected(order)
    c = case.cols
    if order == "key":
        word = [int(k) for k in c["key"]]
    else:
        word = [((int(r) & 0xFFFFFFFF) << 32) | ((int(p) + 1) & 0xFFFFFFFF) for r, p in zip(c["ref_id"], c["pos"])]
    assert perm.tolist() == sorted(range(case.n), key=lambda i: (word[i], i))
    assert len(enc) == len(case.enc) == int(offs[-1])
    # each output record is that record's in-order encoding
    o = [int(x) for x in case.offs]
    for j in list(range(0, case.n, max(case.n // 50, 1))) + [case.n - 1]:
        i = int(perm[j])
        assert enc[int(offs[j]):int(offs[j + 1])] == case.enc[o[i]:o[i + 1]]


def test_orders_are_what_the_header_says():
    case = sc.mixed_case()
    c = case.cols
    # key: negative keys (unmapped reads with a negative hash) first, then contigs, then the other hashes
    k = c["key"][case.expected("key")[2]]
    assert np.all(np.diff(k) >= 0) and k[0] < 0 and k[-1] >> 32 == sc.INT_MAX
    # coordinate: contigs in dictionary order, refID -1 last, pos -1 first within its contig
    p = case.expected("coordinate")[2]
    ref, pos = c["ref_id"][p], c["pos"][p]
    assert ref[0] == 0 and pos[0] == -1 and ref[-1] == -1
    placed = ref >= 0
    assert not np.any(placed[np.argmin(placed):])  # every unplaced read after every placed one
    assert np.all(np.diff(ref[placed]) >= 0)
    for r in range(5):
        assert np.all(np.diff(pos[ref == r]) >= 0)
    # the bin is zeroed in the encoding of exactly the refID < 0 records
    enc, offs, _ = case.expected("coordinate")
    for j in range(0, case.n, 37):
        b = struct.unpack_from("<H", enc, int(offs[j]) + 14)[0]
        assert b == (0 if ref[j] < 0 else c["bin"][p[j]])


def test_boundary_cases_cover_the_sizes():
    for name, (n, total) in sc.BOUNDARY.items():
        case = sc.boundary_case(name)
        assert (case.n, len(case.enc)) == (n, total)
    assert {sc.BOUNDARY[k][0] for k in ("n1", "n255_mod0", "n256_mod1", "n257_mod15")} == {1, 255, 256, 257}


def test_coordinate_expectation_is_a_bam_the_index_oracle_accepts():
    case = sc.mixed_case()
    data = sc.as_bam(case, "coordinate")
    index = bai.write_bai(data)
    assert index[:4] == b"BAI\1"
    lin = bai.linear_index(index)
    assert [bool(e) for e in lin[:6]] == [True] * 5 + [False]
    # ... and its records are the input's taken at perm, in coordinate order
    rc, got = orc.Stream(data, stringency=orc.SILENT).decode_all()
    assert rc == 0
    perm = case.expected("coordinate")[2]
    for f in ("ref_id", "pos", "flag", "key", "rest_len"):
        np.testing.assert_array_equal(got[f], case.cols[f][perm], err_msg=f)
    w = sc.sort_word(got, "coordinate")
    assert np.all(w[1:] >= w[:-1])


def _hdr(text, refs=((b"chr1", 1000), (b"chrM", 16571))):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return out


SQ = b"@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrM\tLN:16571\n@PG\tID:x\tSO:keep\n"


@pytest.mark.parametrize("text,want", [
    (b"@HD\tVN:1.4\tSO:unsorted\tGO:none\n" + SQ, b"@HD\tVN:1.4\tSO:coordinate\tGO:none\n" + SQ),
    (b"@HD\tVN:1.6\n" + SQ, b"@HD\tVN:1.6\tSO:coordinate\n" + SQ),
    (SQ, b"@HD\tVN:1.5\tSO:coordinate\n" + SQ),
    (b"", b"@HD\tVN:1.5\tSO:coordinate\n"),
    (b"@HD\tVN:1.0\tSO:queryname", b"@HD\tVN:1.0\tSO:coordinate"),
    (b"@HD\tVN:1.0\0\0", b"@HD\tVN:1.0\tSO:coordinate\0\0"),
], ids=["replace", "append", "prepend", "empty", "unterminated", "nul-padded"])
def test_sorted_header(text, want):
    got = sorted_header(_hdr(text))
    assert got == _hdr(want)  # l_text follows, the references are untouched
    assert sorted_header(got) == got
    with pytest.raises(ValueError):
        sorted_header(b"BAI\1" + got[4:])


def test_sorted_header_of_a_real_file(test_bam):
    s = orc.Stream(test_bam)
    h = bytes(s.data[:s.header_end])
    got = sorted_header(h)
    l_text = struct.unpack_from("<i", got, 4)[0]
    assert got[8:8 + l_text].split(b"\n")[0].split(b"\t")[0] == b"@HD"
    assert b"SO:coordinate" in got[8:8 + l_text].split(b"\n")[0]
    assert got[8 + l_text:] == h[8 + struct.unpack_from("<i", h, 4)[0]:]


def _oracle_deflate(monkeypatch):
    import hbam.writer as W
    monkeypatch.setattr(W, "bgzf_compress",
                        lambda d, block_lens, level, eof, device: orc.bgzf_compress(d, block_lens, level=level, eof=eof))
    return W


def write_both_ways(W, case, order, buffer_blocks, granularity, block=hbam.HTSJDK_BLOCK_SIZE, pieces=1, count=None):
    """(file, .splitting-bai) of the case's first `count` records (all of them
    by default), sorted, through n write_record calls and through write_records."""
    n = case.n if count is None else count
    enc, offs, _ = case.expected(order, 0, n)
    hdr = bytes(case.stream.data[:case.stream.header_end])
    o = [int(x) for x in offs]
    out = []
    for bulk in (False, True):
        f, sbi = io.BytesIO(), io.BytesIO()
        w = W.BamWriter(f, header=hdr, buffer_blocks=buffer_blocks, splitting_bai=sbi, granularity=granularity,
                        block=block)
        if bulk:
            cuts = [n * k // pieces for k in range(pieces + 1)]
            for a, b in zip(cuts, cuts[1:]):  # (offsets from anywhere in enc: only their differences count)
                w.write_records(enc, offs[a:b + 1])
        else:
            for i in range(n):
                w.write_record(enc[o[i]:o[i + 1]])
        w.close()
        out.append((f.getvalue(), sbi.getvalue()))
    return out


@pytest.mark.parametrize("buffer_blocks,granularity,block,pieces", [
    (1, 4096, hbam.HTSJDK_BLOCK_SIZE, 1), (4, 4096, hbam.HTSJDK_BLOCK_SIZE, 1), (1, 100, hbam.HTSJDK_BLOCK_SIZE, 3),
    (3, 7, 1000, 2), (2, 1, 1000, 1)])
def test_write_records_host_logic_equals_single_calls(monkeypatch, buffer_blocks, granularity, block, pieces):
    W = _oracle_deflate(monkeypatch)
    single, bulk = write_both_ways(W, sc.mixed_case(), "coordinate", buffer_blocks, granularity, block, pieces)
    assert bulk == single
    assert len(single[1]) >= 16


def test_write_records_mixes_with_write_record_and_block_starts(monkeypatch):
    """Records that start exactly at a block or buffer start, and a bulk call
    after single calls (the index counts across both)."""
    W = _oracle_deflate(monkeypatch)
    rec = (96).to_bytes(4, "little") + bytes(96)  # 100-byte records: 10 per 1000-byte block
    enc = rec * 45
    offs = np.arange(46, dtype=np.uint64) * 100
    got = []
    for k in (0, 7, 45):  # single calls for the first k records, one bulk call for the rest
        f, sbi = io.BytesIO(), io.BytesIO()
        w = W.BamWriter(f, buffer_blocks=2, splitting_bai=sbi, granularity=4, block=1000)
        for _ in range(k):
            w.write_record(rec)
        w.write_records(enc, offs[k:])
        w.close()
        got.append((f.getvalue(), sbi.getvalue()))
    assert got[0] == got[1] == got[2]
    v = [int.from_bytes(got[0][1][8 * i:8 * i + 8], "big") for i in range(len(got[0][1]) // 8)]
    assert len(v) == 1 + 45 // 4 + 1 and v[0] & 0xFFFF == 0 and v[1] & 0xFFFF == 300


def test_writer_eof_is_counted_in_the_index(monkeypatch):
    W = _oracle_deflate(monkeypatch)
    rec = (96).to_bytes(4, "little") + bytes(96)
    f, sbi = io.BytesIO(), io.BytesIO()
    w = W.BamWriter(f, splitting_bai=sbi, block=1000)
    w.write_records(rec * 3, [0, 100, 200, 300])
    w.close(eof=True)
    z = f.getvalue()
    assert z.endswith(W.BGZF_EOF_BLOCK) and len(W.BGZF_EOF_BLOCK) == 28
    assert int.from_bytes(sbi.getvalue()[-8:], "big") == len(z) << 16


def test_null_ctx_is_a_state_error():
    n = C.c_uint64(7)
    assert hbam.lib().hbam_sort_writables(None, hbam.SORT_KEY, None, 0, None, None, C.byref(n)) == hbam.E_STATE
    assert n.value == 0
    assert "hbam_sort_writables" in hbam.exported_symbols_from_header()
    assert "hbam_gpu_sort_writables" in hbam.exported_symbols_from_header()
