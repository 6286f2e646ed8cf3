"""Inputs and expected results of the queryname sort and merge tests
(HBAM_SORT_QUERYNAME of hbam_sort_writables and hbam_merge_*).

The expected order is restated in plain Python from the contract in
include/hbam.h: the name (the min(l_read_name, rest_len) bytes at byte 36 of
the record, zero-extended and compared as unsigned bytes: Python's bytes
comparison after stripping trailing zeros), then the tie word from the flag,
then the input order.  The expected bytes are the oracle's in-order encoding
(sort_cases.SortCase) sliced per record and concatenated in that order.  Every
case asserts what it is there for on the CPU, before any comparison with the
GPU.  Test data only."""
import functools
import struct

import numpy as np

import orc
import sort_cases as sc
from bam_patch import recompress

ORDER = "queryname"
FLAGS = (0x0, 0x1, 0x41, 0x81, 0xC1, 0x141, 0x841, 0x4)  # tie words 6, 2, 0, 4, 2, 1, 1, 6


def tie(flag):
    """The tie word t = 2 * m + s of include/hbam.h."""
    if not flag & 0x1:
        m = 3
    else:
        ends = flag & 0xC0
        m = 0 if ends == 0x40 else 2 if ends == 0x80 else 1
    return 2 * m + (1 if flag & 0x900 else 0)


def reference_order(raw_name, flag):
    """The order of records with these name fields (already cut to
    min(l_read_name, rest_len)) and flags."""
    n = len(raw_name)
    return sorted(range(n), key=lambda i: (bytes(raw_name[i]).rstrip(b"\0"), tie(int(flag[i])), i))


class NameCase(sc.SortCase):
    """A SortCase that also knows the queryname order: raw[i] = record i's name
    field read from the inflated stream."""

    def __init__(self, data):
        super().__init__(data)
        u = bytes(self.stream.data)
        c = self.cols
        self.raw = [u[int(p) + 36:int(p) + 36 + min(int(a), int(b))]
                    for p, a, b in zip(c["offset"], c["l_read_name"], c["rest_len"])]
        self.ties = np.array([tie(int(f)) for f in c["flag"]], np.int64)

    def perm(self, order, lo=0, hi=None):
        if order != ORDER:
            return super().perm(order, lo, hi)
        hi = self.n if hi is None else hi
        return np.array(reference_order(self.raw[lo:hi], self.cols["flag"][lo:hi]), np.uint32)

    def chunks_present(self):
        return max((len(r) + 7) // 8 for r in self.raw) if self.n else 0

    def chunks_differing(self):
        """The chunk indices in which two records' zero-extended names differ."""
        m = self.chunks_present()
        padded = [r.ljust(8 * m, b"\0") for r in self.raw]
        return [c for c in range(m) if len({p[8 * c:8 * c + 8] for p in padded}) > 1]


# ---- hand-packed records: the name field and the flag given ---------------------
def named_record(name, flag, extra=b"", l_read_name=None):
    """An unplaced record with no cigar and no bases whose read_name field is
    `name` (its NUL included, if it has one) and whose other variable bytes are
    `extra` (an aux field, or nothing)."""
    rest = bytes(name) + bytes(extra)
    lrn = len(name) if l_read_name is None else l_read_name
    assert 0 <= lrn <= 255
    return struct.pack("<iiiBBHHHiiii", 32 + len(rest), -1, -1, lrn, 0, 4680, 0, flag, 0, -1, -1, 0) + rest


AUX = b"XPZpadding-after-the-name\0"  # a Z aux field: the name then ends well before the record does


def named_bam(recs, block=60000):
    payload = sc._header() + b"".join(recs)
    lens = [min(block, len(payload) - p) for p in range(0, len(payload), block)]
    return orc.bgzf_compress(payload, lens, level=5, eof=True)


def _shuffled(recs, seed):
    rng = np.random.default_rng(seed)
    return [recs[int(i)] for i in rng.permutation(len(recs))]


# ---- chunk_edges ----------------------------------------------------------------
EDGE_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 254)


def _edge_name(length):
    return bytes(65 + (7 * k + 3) % 26 for k in range(length))


def _edge_positions(length):
    """The characters whose change the case probes: the last byte of every
    chunk, the first byte of every later chunk and the final character."""
    pos = {length - 1}
    pos.update(p for p in range(7, length, 8))
    pos.update(p for p in range(8, length, 8))
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def chunk_edges_case():
    recs, k = [], 0
    for length in EDGE_LENGTHS:
        base = _edge_name(length)
        names = [base]
        if length > 1:
            for p in _edge_positions(length):
                names.append(base[:p] + bytes([base[p] + 1]) + base[p + 1:])  # differs from base in byte p alone
            names.append(base[:-1])  # a proper prefix
        for nm in names:
            recs.append(named_record(nm + b"\0", FLAGS[k % len(FLAGS)], AUX if k % 3 == 0 else b""))
            k += 1
    case = NameCase(named_bam(_shuffled(recs, 0x4E414D45)))
    assert case.n == len(recs) and case.chunks_present() == 32  # 254 characters + NUL
    lens = {len(r) - 1 for r in case.raw}
    assert set(EDGE_LENGTHS) <= lens
    stripped = {r.rstrip(b"\0") for r in case.raw}
    for length in EDGE_LENGTHS[1:]:
        base = _edge_name(length)
        assert base in stripped and base[:-1] in stripped
        for p in _edge_positions(length):
            assert base[:p] + bytes([base[p] + 1]) + base[p + 1:] in stripped
    starts = case.source_starts()
    assert set(((starts + 36) % 8).tolist()) == set(range(8))
    ends_late = {bool(36 + len(r) > int(ln) - 8) for r, ln in zip(case.raw, case.lens)}
    assert ends_late == {False, True}  # the name ends inside the record's last 8 bytes, and well before them
    assert not np.array_equal(case.perm(ORDER), np.arange(case.n))
    return case


# ---- unsigned_bytes -------------------------------------------------------------
BYTE_VALUES = (0x00, 0x01, 0x41, 0x7F, 0x80, 0xFF)
BYTE_POSITIONS = (0, 7, 8)  # the first and the last byte of chunk 0, the first of chunk 1
BYTE_BASE = b"BCDEFGHIJKL"


@functools.lru_cache(maxsize=None)
def unsigned_bytes_case():
    """Placeholder names patched in the inflated stream (as _mixed_data patches
    positions) to bytes no well-formed name holds; record 0 gets l_read_name 0
    (the empty name) and record 1 an l_read_name past its rest (the name is cut
    to the rest)."""
    want = []
    for p in BYTE_POSITIONS:
        for v in BYTE_VALUES:
            want.append(BYTE_BASE[:p] + bytes([v]) + BYTE_BASE[p + 1:] + b"\0")
    want = _shuffled(want * 2, 0x4E414D46)
    recs = [named_record(b"A" * 11 + b"\0", FLAGS[k % len(FLAGS)], AUX if k % 2 else b"") for k in range(len(want) + 2)]
    s = orc.Stream(named_bam(recs), stringency=orc.SILENT)
    rc, r = s.decode_all()
    assert rc == 0 and len(r["offset"]) == len(recs)
    u = bytearray(s.data)
    for k, p in enumerate(r["offset"]):
        p = int(p)
        if k == 0:
            u[p + 12] = 0
        elif k == 1:
            u[p + 12] = 200
        else:
            u[p + 36:p + 48] = want[k - 2]
    case = NameCase(recompress(s, bytes(u)))
    assert case.n == len(recs)
    assert case.raw[0] == b"" and case.cols["l_read_name"][0] == 0
    assert case.cols["l_read_name"][1] == 200 and len(case.raw[1]) == int(case.cols["rest_len"][1]) < 200
    assert [bytes(x) for x in case.raw[2:]] == want
    assert any(0 in x[:-1] for x in want)  # an interior NUL
    # in the expected order the probed byte never decreases as an unsigned value: >= 0x80 after ASCII
    perm = case.perm(ORDER)
    for p in BYTE_POSITIONS:
        seen = [case.raw[int(i)][p] for i in perm
                if int(i) >= 2 and case.raw[int(i)][:p] + case.raw[int(i)][p + 1:] == BYTE_BASE[:p] + BYTE_BASE[p + 1:] + b"\0"]
        assert len(seen) == 2 * len(BYTE_VALUES) and seen == sorted(seen) and seen[-1] == 0xFF and 0x80 in seen
    assert int(perm[0]) == 0  # the empty name first
    return case


# ---- all_equal ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_equal_case(equal_flags=False):
    recs = [named_record(b"one/name:for:all\0", 0x41 if equal_flags else FLAGS[k % len(FLAGS)],
                         AUX if k % 5 == 0 else b"") for k in range(300)]
    case = NameCase(named_bam(recs))
    assert case.n == 300 and len(set(case.raw)) == 1 and case.chunks_differing() == []
    perm = case.perm(ORDER)
    if equal_flags:
        assert np.array_equal(perm, np.arange(300))
    else:
        assert sorted(set(case.ties.tolist())) == [0, 1, 2, 4, 6]
        t = case.ties[perm]
        assert np.all(t[1:] >= t[:-1])
        for v in set(t.tolist()):  # batch order inside one tie word
            assert np.all(np.diff(perm[t == v].astype(np.int64)) > 0)
    return case


# ---- illumina -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def illumina_case():
    """4,000 synthetic short reads (mixed_case's data: positions dealt at random;
    the names are the generator's, mates sharing one)."""
    case = NameCase(sc._mixed_data(4000, 0x534F5254))
    assert case.n == 4000
    assert len({r[:8] for r in case.raw}) == 1  # the names share their first chunk
    _, counts = np.unique(np.array(case.raw, dtype=object), return_counts=True)
    assert int(np.count_nonzero(counts >= 2)) >= 100
    diff = case.chunks_differing()
    assert 0 not in diff and 0 < len(diff) < case.chunks_present()
    assert not np.array_equal(case.perm(ORDER), np.arange(case.n))
    return case


# ---- random names over {A, B} ---------------------------------------------------
def _ab_records(n, seed, last_plain=False):
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(n):
        name = bytes(rng.choice([65, 66], int(rng.integers(0, 41))).astype(np.uint8))
        recs.append(named_record(name + b"\0", FLAGS[int(rng.integers(0, len(FLAGS)))],
                                 AUX if rng.random() < 0.5 else b""))
    if last_plain:
        recs[-1] = named_record(b"B\0", 0x41)
    return recs


@functools.lru_cache(maxsize=None)
def random_small_alphabet_case():
    case = NameCase(named_bam(_ab_records(5000, 0x4E414D47)))
    assert case.n == 5000
    names, counts = np.unique(np.array(case.raw, dtype=object), return_counts=True)
    assert int(np.count_nonzero(counts >= 3)) >= 50  # exact ties ...
    key = list(zip(case.raw, case.ties.tolist()))
    assert len(set(key)) < len(key) - 200  # ... also in (name, tie): batch order decides
    first = [a[:8] for a in names if len(a) > 8]
    assert len(first) - len(set(first)) > 100  # distinct names that share their first chunk
    assert min(len(r) for r in case.raw) == 1 and max(len(r) for r in case.raw) == 41
    return case


@functools.lru_cache(maxsize=None)
def ends_of_stream_case():
    """The file's last record has a 1-character name and nothing after it: its
    name's chunk is the last 2 bytes of the inflated stream."""
    case = NameCase(named_bam(_ab_records(250, 0x4E414D48, last_plain=True)))
    assert case.n == 250 and case.raw[-1] == b"B\0" and int(case.lens[-1]) == 38
    assert int(case.source_starts()[-1]) + 38 == len(bytes(case.stream.data))
    return case


SIZES = (0, 1, 2, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def size_case(n):
    case = NameCase(named_bam(_ab_records(n, 0x4E414D49 + n)))
    assert case.n == n
    return case


# ---- merge: consecutive record ranges sorted on their own -----------------------
def runs_of(case, bounds):
    """[(enc, offs)] of the ranges [bounds[k], bounds[k + 1]) each in queryname order."""
    return [case.expected(ORDER, a, b)[:2] for a, b in zip(bounds, bounds[1:])]


def merged_src(case, bounds):
    """src[j] = run << 32 | record-in-run of the j-th record of the merge of
    runs_of(case, bounds): the order of the whole range (ties go to the earlier
    record, hence to the earlier run), each record named by where its run holds it."""
    lo, hi = bounds[0], bounds[-1]
    where = np.zeros(hi - lo, np.uint64)
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        p = case.perm(ORDER, a, b).astype(np.int64)
        where[a - lo + p] = (np.uint64(k) << np.uint64(32)) | np.arange(b - a, dtype=np.uint64)
    return where[case.perm(ORDER, lo, hi).astype(np.int64)]


def cuts(n, lo=0):
    """name -> bounds over records [lo, lo + n): 1, 3 and 16 runs, an empty run in each of the latter."""
    k16 = [lo + (n * i) // 15 for i in range(16)]
    k16.insert(5, k16[5])  # 17 bounds: run 5 is empty
    return {"k1": [lo, lo + n], "k3_empty_middle": [lo, lo + n // 4, lo + n // 4, lo + n], "k16_one_empty": k16}
