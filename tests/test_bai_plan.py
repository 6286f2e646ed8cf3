"""CPU: reading a .bai in the library (hbam_bai_summarize / hbam_bai_query: host
code, no ctx, no device) against the restated chunk lookup of
tests/query_cases.py (bai_chunks_for), on indexes the oracle writes
(oracle/bai.py write_bai), as they are and with a hand-appended pseudo-bin
37450 per contig and the trailing n_no_coor (SAM spec 5.2)."""
import functools
import struct

import pytest

import bai
import hbam
import query_cases as q
from bai_cases import spread_bam
from test_bai import PLACEMENTS

TRAP = [(3, 49152, 0), (5, 65536, 16384)]  # every record of contig 3 at one position: lin[2] > lin[3]


def with_metadata(index, no_coor=30):
    """index with a bin 37450 (two chunks) appended to every contig that has
    bins, and the trailing n_no_coor."""
    (n_ref,) = struct.unpack_from("<i", index, 4)
    out = bytearray(index[:8])
    p = 8
    for r in range(n_ref):
        (nb,) = struct.unpack_from("<i", index, p)
        a = p + 4
        p = a
        for _ in range(nb):
            (nc,) = struct.unpack_from("<i", index, p + 4)
            p += 8 + 16 * nc
        out += struct.pack("<i", nb + (1 if nb else 0)) + index[a:p]
        if nb:
            # chunk values that would join the result if the pseudo-bin were ever read as a bin
            out += struct.pack("<IiQQQQ", 37450, 2, 1 << 16, (1 << 62), 1000 + r, 7)
        (ni,) = struct.unpack_from("<i", index, p)
        out += index[p:p + 4 + 8 * ni]
        p += 4 + 8 * ni
    assert p == len(index)
    return bytes(out) + struct.pack("<Q", no_coor)


@functools.lru_cache(maxsize=None)
def index_of(name):
    data = {"main": lambda: q.main_case().data, "long": lambda: q.long_case().data,
            "unsorted": lambda: q.unsorted_case().data, "unplaced": lambda: q.unplaced_case().data,
            "trap": lambda: spread_bam(3000, TRAP), "one": lambda: spread_bam(6000, PLACEMENTS[0])}[name]()
    return bai.write_bai(data)


def variants(name):
    b = index_of(name)
    return [b, with_metadata(b)]


SETS = ([("main", iv) for iv, _, _ in q.MAIN_SETS] + [("long", iv) for iv, _ in q.LONG_SETS] +
        [("unsorted", iv) for iv, _, _ in q.UNSORTED_SETS] +
        [("trap", [(3, 49152, 49152)]), ("trap", [(3, 1, 0)]), ("trap", [(3, 40000, 49000), (5, 1, 100000)]),
         ("trap", [(5, 16384 * 9, 16384 * 11)]),
         # an interval starting past the contig's linear table; a contig with no bins
         ("main", [(1, 50000000, 0)]), ("main", [(1, 50000000, 50000100), (7, 400000000, 0)]),
         ("main", [(2, 1, 0)]), ("main", [(0, 1, 1000), (2, 5, 10), (3, 1, 0)]),
         ("one", [(0, 10000, 10040), (0, 20000, 30000), (0, 250000, 0)]), ("unplaced", [(0, 1, 0)]),
         ("main", [])])


@pytest.mark.parametrize("k", range(len(SETS)))
def test_query_matches_the_restated_lookup(k):
    name, iv = SETS[k]
    plain, meta = variants(name)
    want = q.flat(q.bai_chunks_for(plain, iv))
    assert hbam.bai_query(plain, iv) == want
    # the pseudo-bin is never a query bin and the trailer is not index data
    assert hbam.bai_query(meta, iv) == want


def test_sets_are_not_vacuous():
    assert sum(bool(q.bai_chunks_for(index_of(n), iv)) for n, iv in SETS) >= 12
    # the trap: a placed unmapped read touches the window below its position's
    lin = bai.linear_index(index_of("trap"))[3]
    assert lin[2] > lin[3]


def test_summary():
    for name in ("main", "long", "unplaced", "trap"):
        plain, meta = variants(name)
        lin = [e for e in bai.linear_index(plain) if e]
        s = hbam.bai_summary(plain)
        assert s["n_ref"] == len(bai.linear_index(plain))
        assert s["start_of_last_linear_bin"] == lin[-1][-1]
        assert not s["has_no_coor"] and s["no_coor_count"] == 0
        m = hbam.bai_summary(meta)
        assert m["has_no_coor"] and m["no_coor_count"] == 30
        assert m["start_of_last_linear_bin"] == lin[-1][-1] and m["n_ref"] == s["n_ref"]
    empty = b"BAI\1" + struct.pack("<i", 2) + struct.pack("<ii", 0, 0) * 2
    s = hbam.bai_summary(empty)
    assert s == {"n_ref": 2, "has_no_coor": False, "start_of_last_linear_bin": -1, "no_coor_count": 0}
    assert hbam.bai_query(empty, [(1, 1, 0)]) == []
    assert hbam.bai_summary(b"BAI\1" + struct.pack("<i", 0))["start_of_last_linear_bin"] == -1


def test_error_codes():
    b = index_of("main")

    def code(fn, *a):
        with pytest.raises(hbam.HbamError) as e:
            fn(*a)
        return e.value.code

    # [htsjdk] assertIntervalsOptimized, as hbam_query_intervals
    assert code(hbam.bai_query, b, [(1, 100, 200), (1, 150, 300)]) == hbam.E_ARG
    assert code(hbam.bai_query, b, [(4, 1, 0), (1, 1, 0)]) == hbam.E_ARG
    assert code(hbam.bai_query, b, [(1, 100, 50)]) == hbam.E_ARG
    (n_ref,) = struct.unpack_from("<i", b, 4)
    assert code(hbam.bai_query, b, [(n_ref, 1, 0)]) == hbam.E_ARG
    assert code(hbam.bai_query, b, [(-1, 1, 0)]) == hbam.E_ARG
    assert hbam.bai_query(b, [(n_ref - 1, 1, 0)]) == []
    for bad in (b"BAM\1junk", b"BAI\1", b[:8 + 8 + 4 + 8 + 5], b[:len(b) - 3], b"BAI\1" + struct.pack("<i", -1)):
        assert code(hbam.bai_query, bad, [(1, 1, 0)]) == hbam.E_FORMAT
        assert code(hbam.bai_summary, bad) == hbam.E_FORMAT
