"""GPU: the BAM index built on the GPU (hbam_build_bai) against the oracle's
writer (oracle/bai.py write_bai), byte for byte, with the default window and
with 64 KiB windows (many windows per file: the carry of the last record's
key, of the open chunk and of the sort order from window to window is what is
tested there); the metadata pseudo-bins against values computed from the
oracle's record table; and the loop closed end to end: index built here ->
hbam_bai_query / hbam_bai_summarize -> hbam_query_intervals /
hbam_query_unmapped -> records."""
import functools
import struct

import numpy as np
import pytest

import bai
import hbam
import orc
import query_cases as q
from bai_cases import spread_bam
from test_bai import PLACEMENTS
from test_gpu_query import assert_query, drain

pytestmark = pytest.mark.gpu
WINDOWS = [0, 65536]
TRAP = [(3, 49152, 0), (5, 65536, 16384)]  # every record of contig 3 at one position: lin[2] > lin[3]
META_BIN = 37450


@functools.lru_cache(maxsize=None)
def one_case():
    return q.Case(spread_bam(6000, PLACEMENTS[0]))


@functools.lru_cache(maxsize=None)
def trap_case():
    return q.Case(spread_bam(3000, TRAP))


@functools.lru_cache(maxsize=None)
def big_case():
    # runs of thousands of records per bin, several sort tiles of records, ~215 windows of 64 KiB
    return q.Case(spread_bam(100000, [(0, 100, 7), (2, 5000, 7), (5, 1000000, 7)]))


CASES = {"main": (q.main_case, hbam.STRICT), "unplaced": (q.unplaced_case, hbam.STRICT),
         "long": (q.long_case, hbam.STRICT), "cigar_ops": (q.cigar_ops_case, hbam.SILENT),
         "one": (one_case, hbam.STRICT), "trap": (trap_case, hbam.STRICT)}


@functools.lru_cache(maxsize=None)
def oracle_index(name):
    case = big_case() if name == "big" else CASES[name][0]()
    return bai.write_bai(case.data)


@functools.lru_cache(maxsize=None)
def built(name, window, metadata):
    """The index the GPU builds (computed once per input, window and flag)."""
    case, stringency = (big_case, hbam.STRICT) if name == "big" else CASES[name]
    with hbam.BamFile(case().data, window_bytes=window, stringency=stringency) as f:
        return f.build_bai(metadata=metadata)


def split_metadata(index):
    """(the index without bin 37450 and without the trailer, {ref: its pseudo-bin's
    four values}, n_no_coor or None)."""
    (n_ref,) = struct.unpack_from("<i", index, 4)
    out = bytearray(index[:8])
    meta = {}
    p = 8
    for r in range(n_ref):
        (nb,) = struct.unpack_from("<i", index, p)
        p += 4
        kept = bytearray()
        nk = 0
        for k in range(nb):
            b, nc = struct.unpack_from("<Ii", index, p)
            if b == META_BIN:
                assert nc == 2 and k == nb - 1  # the contig's last bin
                meta[r] = struct.unpack_from("<QQQQ", index, p + 8)
            else:
                kept += index[p:p + 8 + 16 * nc]
                nk += 1
            p += 8 + 16 * nc
        (ni,) = struct.unpack_from("<i", index, p)
        out += struct.pack("<i", nk) + kept + index[p:p + 4 + 8 * ni]
        p += 4 + 8 * ni
    no_coor = struct.unpack_from("<Q", index, p)[0] if len(index) - p == 8 else None
    assert len(index) - p in (0, 8)
    return bytes(out), meta, no_coor


def expected_metadata(case):
    """From the oracle's record table: per contig (voff of its first indexed
    record, chunk end of its last one, indexed records without 0x4, with 0x4);
    the records without coordinates."""
    r = case.records
    voff = [int(v) for v in r["voff"]] + [len(case.data) << 16]
    meta, no_coor = {}, 0
    for i in range(len(r["voff"])):
        ref, pos, unm = int(r["ref_id"][i]), int(r["pos"][i]), bool(r["flag"][i] & 4)
        if ref < 0 or pos < 0:
            no_coor += 1
            continue
        first, _, m, u = meta.get(ref, (voff[i], 0, 0, 0))
        meta[ref] = (first, voff[i + 1], m + (not unm), u + unm)
    return meta, no_coor


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(CASES))
def test_index_is_the_oracles_byte_for_byte(name, window):
    assert built(name, window, False) == oracle_index(name)


def test_inputs_are_what_the_tests_need():
    assert len(q.main_case().table) == 6000 and len(q.long_case().table) == 300
    r = q.long_case().records
    assert int(np.count_nonzero(r["ref_id"] < 0)) == 39 and 0 < int(np.flatnonzero(r["ref_id"] < 0)[0]) < 200
    assert int(r["n_cigar"].max()) > 64  # the whole-wave cigar sum runs
    assert int(np.count_nonzero(q.unplaced_case().records["ref_id"] < 0)) == 30
    lin = bai.linear_index(oracle_index("trap"))[3]
    assert lin[2] > lin[3]  # not monotone: a placed unmapped read touches the window below


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(CASES))
def test_metadata(name, window):
    case = CASES[name][0]()
    index = built(name, window, True)
    plain, meta, no_coor = split_metadata(index)
    assert plain == oracle_index(name)
    want_meta, want_no_coor = expected_metadata(case)
    assert meta == want_meta and no_coor == want_no_coor
    s = hbam.bai_summary(index)
    lin = [e for e in bai.linear_index(plain) if e]
    assert s == {"n_ref": case.stream.n_ref, "has_no_coor": True, "no_coor_count": want_no_coor,
                 "start_of_last_linear_bin": lin[-1][-1]}
    assert not hbam.bai_summary(plain)["has_no_coor"]


@pytest.mark.parametrize("placement", [0, 1], ids=["one", "three"])
@pytest.mark.parametrize("split_size", [60000, 150000, 400000])
def test_split_planner_takes_the_built_index(placement, split_size):
    name = ["one", "main"][placement]
    data = CASES[name][0]().data
    sp = bai.file_splits(len(data), split_size)
    starts, lengths = [a for a, _ in sp], [n for _, n in sp]
    with hbam.BamFile(data) as f:
        want = f.get_splits(starts, lengths, bai=oracle_index(name))
        assert f.get_splits(starts, lengths, bai=built(name, 0, False)) == want
        assert f.get_splits(starts, lengths, bai=built(name, 65536, True)) == want  # pseudo-bins and trailer


SETS = [("main", iv) for iv, _, _ in q.MAIN_SETS] + [("long", iv) for iv, _ in q.LONG_SETS]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("k", range(len(SETS)))
def test_end_to_end_interval_read(k, window):
    name, iv = SETS[k]
    case = CASES[name][0]()
    with hbam.BamFile(case.data, window_bytes=window) as f:
        index = f.build_bai()
        ptrs = hbam.bai_query(index, iv)
        chunks = list(zip(ptrs[0::2], ptrs[1::2]))
        assert chunks == q.bai_chunks_for(oracle_index(name), iv)
        f.query_intervals(iv, ptrs)
        status, got, _ = drain(f)
    rc, want, _ = q.query_oracle(case.stream, iv, chunks)
    assert rc == 0 and status == 0
    assert_query(got, want, case.u)
    # ... which are the records of the whole file that overlap an interval
    keep = q.overlaps_any(case.table, iv)
    np.testing.assert_array_equal(got["voff"], case.records["voff"][keep])


@pytest.mark.parametrize("window", WINDOWS)
def test_end_to_end_unmapped_read(window):
    case = q.unplaced_case()
    with hbam.BamFile(case.data, window_bytes=window) as f:
        s = hbam.bai_summary(f.build_bai())
        assert s["no_coor_count"] == 30 and s["start_of_last_linear_bin"] > 0
        f.query_unmapped(s["start_of_last_linear_bin"])
        status, got, _ = drain(f)
    rc, want = q.unmapped_oracle(case.stream, s["start_of_last_linear_bin"])
    assert rc == 0 and status == 0 and len(want["voff"]) == 30
    assert_query(got, want, case.u)


@pytest.mark.parametrize("window", WINDOWS)
def test_unsorted_file_is_a_format_error(window):
    with hbam.BamFile(q.unsorted_case().data, window_bytes=window) as f:
        with pytest.raises(hbam.HbamError) as e:
            f.build_bai(metadata=False)
        assert e.value.code == hbam.E_FORMAT and "sorted" in str(e.value)
        assert len(f.decode_all()["voff"]) == 6000  # the ctx goes on working


def test_bgzf_ctx_is_a_state_error_and_a_build_ends_a_query():
    case = q.main_case()
    with hbam.BamFile(case.data, bam=False) as f:
        with pytest.raises(hbam.HbamError) as e:
            f.build_bai()
        assert e.value.code == hbam.E_STATE
    with hbam.BamFile(case.data) as f:
        f.query_intervals(q.MAIN_SETS[0][0], q.flat(case.whole))
        f.build_bai()
        with pytest.raises(hbam.HbamError) as e:
            f.query_next()
        assert e.value.code == hbam.E_STATE


@pytest.mark.parametrize("window", WINDOWS)
def test_header_only_bam_gives_the_empty_index(window):
    s = q.main_case().stream
    hdr_len = int(s.first_record_voff & 0xffff)
    assert s.first_record_voff >> 16 == 0  # the header lies in the first block
    data = orc.bgzf_compress(bytes(s.data[:hdr_len]), [hdr_len], level=5, eof=True)
    want = b"BAI\1" + struct.pack("<i", s.n_ref) + struct.pack("<ii", 0, 0) * s.n_ref
    assert bai.write_bai(data) == want
    with hbam.BamFile(data, window_bytes=window) as f:
        assert f.build_bai(metadata=False) == want
        assert f.build_bai() == want + struct.pack("<Q", 0)


@pytest.mark.parametrize("window", WINDOWS)
def test_larger_input(window):
    want = oracle_index("big")
    assert built("big", window, False) == want
    plain, meta, no_coor = split_metadata(built("big", window, True))
    assert plain == want and no_coor == 0
    assert meta == expected_metadata(big_case())[0]
