"""Inputs and expected results of the merge tests (hbam_merge_*).

No oracle of its own: a run is `case.expected(order, lo, hi)` of
tests/sort_cases.py (a consecutive record range sorted on its own) or any
other sorted arrangement of a case's records, and the expected output is the
concatenated runs' records in the order of a NumPy stable argsort over the
concatenated run words -- ties to the earlier run, then to the earlier record
of a run.  Test data only."""
import functools

import numpy as np

import sort_cases as sc

TILE = sc.TILE
BIG = 1 << 40  # a part_bytes larger than any output here: one part
PART_BYTES = (TILE - 1, TILE, TILE + 1, BIG)  # every case; 64 as well where SMALL_PARTS says so


def words_u64(cols, order):
    """The merge's sort word (k_sort_words) of decoded columns, as uint64."""
    if order == "key":
        return cols["key"].astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return sc.sort_word(cols, order).astype(np.uint64)


class Run:
    """One sorted run: its encodings, n + 1 offsets, n words, and for each
    record the index of the case's record it is (diagnostics)."""

    def __init__(self, enc, offs, words, ids):
        self.enc, self.offs, self.words, self.ids = bytes(enc), np.asarray(offs, np.uint64), \
            np.asarray(words, np.uint64), np.asarray(ids, np.int64)
        self.n = len(self.words)
        assert len(self.offs) == self.n + 1 and int(self.offs[-1]) == len(self.enc)
        assert np.all(self.words[1:] >= self.words[:-1])

    def record(self, i):
        return self.enc[int(self.offs[i]):int(self.offs[i + 1])]


def range_run(case, order, lo, hi):
    """Records [lo, hi) of the case sorted on their own: what hbam_sort_writables gives for that batch."""
    enc, offs, perm = case.expected(order, lo, hi)
    w = words_u64({k: v[lo:hi] for k, v in case.cols.items()}, order)[perm]
    return Run(enc, offs, w, lo + perm.astype(np.int64))


def consecutive_runs(case, order, bounds):
    assert bounds[0] >= 0 and all(a <= b for a, b in zip(bounds, bounds[1:])) and bounds[-1] <= case.n
    return [range_run(case, order, a, b) for a, b in zip(bounds, bounds[1:])]


def picked_run(case, order, idx):
    """The records idx (positions in the case's sorted whole, increasing) as one run."""
    enc, offs, perm = case.expected(order)
    o = [int(x) for x in offs]
    w = words_u64(case.cols, order)[perm]
    idx = [int(i) for i in idx]
    out = b"".join(enc[o[i]:o[i + 1]] for i in idx)
    ro = np.zeros(len(idx) + 1, np.uint64)
    ro[1:] = np.cumsum([o[i + 1] - o[i] for i in idx])
    return Run(out, ro, w[idx], perm[idx].astype(np.int64))


def merged(runs):
    """(bytes, offs[u64, n + 1], src[u64, n]) the merge of the runs must give."""
    words = np.concatenate([r.words for r in runs]) if runs else np.zeros(0, np.uint64)
    src = np.concatenate([(np.uint64(k) << np.uint64(32)) | np.arange(r.n, dtype=np.uint64)
                          for k, r in enumerate(runs)]) if runs else np.zeros(0, np.uint64)
    order = np.argsort(words, kind="stable")
    src = src[order]
    recs = [runs[int(s) >> 32].record(int(s) & 0xFFFFFFFF) for s in src]
    offs = np.zeros(len(recs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in recs])
    return b"".join(recs), offs, src.astype(np.uint64)


def part_heads(offs, part_bytes):
    """The output indices at which a part starts: record j belongs to part
    offs[j] // part_bytes, parts without a record start do not exist."""
    o = offs[:-1].astype(np.int64) // int(part_bytes)
    if len(o) == 0:
        return np.zeros(0, np.int64)
    return np.flatnonzero(np.concatenate([[True], o[1:] != o[:-1]]))


def part_runs(src, heads):
    """Per part, the set of runs it takes records from."""
    ends = list(heads[1:]) + [len(src)]
    return [set((src[a:b] >> np.uint64(32)).astype(np.int64).tolist()) for a, b in zip(heads, ends)]


# ---- the cuts: consecutive record ranges ---------------------------------------
def cuts(n):
    """name -> bounds of consecutive runs over n records: k in {1, 2, 3, 7},
    uneven, an empty run in the middle, one-record runs."""
    if n == 1:
        return {"k1": [0, 1]}
    assert n >= 60
    return {"k1": [0, n],
            "k2": [0, n // 3, n],
            "k3_empty_middle": [0, n // 4, n // 4, n],
            "k7_one_record_runs": [0, 1, n // 9, n // 4, n // 2, (7 * n) // 10, n - 1, n]}


# name -> the record range the 64-byte parts run on (a few hundred records: one launch set per part)
SMALL_PARTS = {"mixed": (1000, 1500), "tiny": (0, 400), "n255_mod0": (0, 255), "n1": (0, 1)}


# ---- arrangements consecutive cuts never give -----------------------------------
def round_robin_runs(case, order, k=4):
    """The sorted whole dealt to k runs in turn: a perfect interleave."""
    return [picked_run(case, order, range(r, case.n, k)) for r in range(k)]


def reversed_piece_runs(case, order):
    """The sorted whole in 3 contiguous pieces, the last first: disjoint word
    ranges with the later run holding the smaller words."""
    a, b = case.n // 3, (2 * case.n) // 3
    return [picked_run(case, order, range(b, case.n)), picked_run(case, order, range(a, b)),
            picked_run(case, order, range(0, a))]


EQUAL_REF, EQUAL_POS = 1, 5


@functools.lru_cache(maxsize=None)
def equal_word_runs(order):
    """Three runs (5, 1 and 9 records of different lengths) whose records all
    have the same word: mapped reads at one position."""
    key = (EQUAL_REF << 32) | EQUAL_POS  # BAMRecordReader.getKey0(refID, pos) of a mapped read
    w = np.uint64(key ^ (1 << 63)) if order == "key" else np.uint64((EQUAL_REF << 32) | (EQUAL_POS + 1))
    runs, tag = [], 0
    for n in (5, 1, 9):
        recs = []
        for _ in range(n):
            recs.append(sc.packed_record(38 + (7 * tag) % 60, EQUAL_REF, EQUAL_POS, 0, tag))
            tag += 1
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([len(r) for r in recs])
        runs.append(Run(b"".join(recs), offs, np.full(n, w, np.uint64), np.arange(tag - n, tag)))
    return tuple(runs)
