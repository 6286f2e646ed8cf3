"""CPU: the queryname order's reference restated on hand-written records, the
test cases' own preconditions (tests/name_cases.py), and the parts of the order
that need no GPU: hbam.sort.sorted_header(h, "queryname"), the order's number
and sort_words' refusal (the order has no sort word)."""
import numpy as np
import pytest

import hbam
import name_cases as nc
from hbam.sort import sort_words, sorted_header
from test_sort_cases import SQ, _hdr


def test_tie_word():
    assert [nc.tie(f) for f in (0x41, 0x141, 0x841, 0x1, 0xC1, 0x101, 0x81, 0x181, 0x0, 0x4, 0x40, 0x100, 0x800)] \
        == [0, 1, 1, 2, 2, 3, 4, 5, 6, 6, 6, 7, 7]
    # the flag bits that are not named leave it alone
    assert nc.tie(0x41 | 0x2 | 0x10 | 0x20 | 0x200 | 0x400) == 0


def test_reference_order_on_hand_written_records():
    rec = [(b"b\0", 0x41),        # 0
           (b"a\0", 0x81),        # 1  second of pair ...
           (b"a\0", 0x41),        # 2  ... after the first of the same name
           (b"a\0", 0x141),       # 3  a secondary first-of-pair: between the two
           (b"ab\0", 0x0),        # 4  "a" is a prefix of "ab"
           (b"a\0", 0x0),         # 5  unpaired after paired
           (b"a\0\0\0", 0x41),    # 6  = "a" zero-extended: ties with 2, batch order
           (b"", 0x41),           # 7  the empty name first
           (b"a\x80\0", 0x41),    # 8  0x80 after ASCII
           (b"a\x7f\0", 0x41),    # 9
           (b"a\0b\0", 0x41),     # 10 an interior NUL: above "a", below "a\x01"
           (b"a\x01\0", 0x41),    # 11
           (b"B\0", 0x41)]        # 12 upper case before lower: bytes, not a collation
    got = nc.reference_order([r[0] for r in rec], [r[1] for r in rec])
    assert got == [7, 12, 2, 6, 3, 1, 5, 10, 11, 4, 9, 8, 0]


@pytest.mark.parametrize("build", [nc.chunk_edges_case, nc.unsigned_bytes_case, nc.all_equal_case,
                                   lambda: nc.all_equal_case(True), nc.illumina_case,
                                   nc.random_small_alphabet_case, nc.ends_of_stream_case]
                         + [lambda n=n: nc.size_case(n) for n in nc.SIZES],
                         ids=["chunk_edges", "unsigned_bytes", "all_equal", "all_equal_flags", "illumina",
                              "random_small_alphabet", "ends_of_stream"] + [f"n{n}" for n in nc.SIZES])
def test_cases_hold_what_they_are_there_for(build):
    case = build()  # (asserts the case's own preconditions)
    enc, offs, perm = case.expected(nc.ORDER)
    assert sorted(perm.tolist()) == list(range(case.n)) and len(enc) == len(case.enc)
    # the order computed a second way: no earlier record is above a later one
    key = [(case.raw[int(i)].rstrip(b"\0"), int(case.ties[int(i)]), int(i)) for i in perm]
    assert all(a < b for a, b in zip(key, key[1:]))
    # ... and a merge of ranges sorted on their own is the whole's order
    if case.n >= 60:
        for bounds in nc.cuts(case.n).values():
            src = nc.merged_src(case, bounds)
            runs = nc.runs_of(case, bounds)
            o = [[int(x) for x in r[1]] for r in runs]
            got = b"".join(runs[int(s) >> 32][0][o[int(s) >> 32][int(s) & 0xFFFFFFFF]:
                                                 o[int(s) >> 32][(int(s) & 0xFFFFFFFF) + 1]] for s in src)
            assert got == enc


@pytest.mark.parametrize("text,want", [
    (b"@HD\tVN:1.4\tSO:unsorted\tGO:none\n" + SQ, b"@HD\tVN:1.4\tSO:queryname\tGO:none\n" + SQ),
    (b"@HD\tVN:1.6\n" + SQ, b"@HD\tVN:1.6\tSO:queryname\n" + SQ),
    (SQ, b"@HD\tVN:1.5\tSO:queryname\n" + SQ),
], ids=["replace", "append", "prepend"])
def test_sorted_header_queryname(text, want):
    got = sorted_header(_hdr(text), "queryname")
    assert got == _hdr(want) and b"SS:" not in got
    assert sorted_header(got, order="queryname") == got
    # the default is the coordinate order's header, as before
    assert sorted_header(_hdr(text)) == sorted_header(_hdr(text), "coordinate") \
        == _hdr(want.replace(b"SO:queryname", b"SO:coordinate"))
    assert sorted_header(sorted_header(_hdr(text)), "queryname") == got
    with pytest.raises(ValueError):
        sorted_header(_hdr(text), "key")


def test_the_order_has_a_number_and_no_word():
    assert hbam.SORT_QUERYNAME == hbam.SORT_ORDERS["queryname"] == 3
    assert sorted(hbam.SORT_ORDERS.values()) == [0, 1, 3]  # 2 is not an order
    for order in ("queryname", 3):
        with pytest.raises(hbam.HbamError) as e:
            sort_words(np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32), order)
        assert e.value.code == hbam.E_ARG
    assert len(sort_words(np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32), "key")) == 2
