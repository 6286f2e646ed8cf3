"""GPU: the record chain on false starts and on implausible records
(chain_cases.py), bit-exact against the oracle through every entry point, in
one window and in small ones (where the inflated range ends before the stream
and plausible() accepts what it cannot read), under STRICT, LENIENT and
SILENT (under SILENT and in indexer mode a list from a plausible walk skips
the per-record rules), with hbam_chain_counters showing the path a case took.

Paths observed on an MI355X, one decode_span_device over the whole file in
one window, as searched / re-walk requests / dropped blocks, link rounds
("Adversarial cases", has the table and the reasons):
  merge 0/1/0, 2 rounds; merge3 0/3/0, 2; deadend 1/0/0, 1; look3 2/0/0, 1;
  look4 1/0/0, 1; stray_in 1/0/0, 1; stray_out 0/2/1, 3 (the drop, then the
  two blocks its exit hid); shift1 0/0/0, 1 (the rescue works: no re-walk);
  cascade 0/10/1, 3; tail_eof and tail_noeof 0/0/0, 1.  No serial link.
Implausible records, the same under SILENT and STRICT: every case but
*_first ends in the serial link (link_fallbacks 1).
  six 6/30/0, pos_last, lrn0_last, pos_pair, lrn0_pair 1/5/0: 5 rounds.  The
    search settles on the record after the patched one, the link check asks
    for the true entry, and k_rec_walk's validate branch refuses it in each
    of the 4 re-walk rounds, as the chain from it is not plausible.
  *_blockfirst, *_after1..4, *_wholeblock 1/1/0 (2/1/0 for after3, after4):
    1 round.  A block ends up with no guess (every chain of the block before
    meets the patched record inside its lookahead; a whole block has no
    plausible start), so the block after it sees the chain stop short of it:
    a hard violation, the serial link at once.
  *_first 0/0/0, 1 round, no serial link: the span's first record is a known
    entry, walked by block_size alone.
"""
import numpy as np
import pytest

import chain_cases as cc
import hbam
import orc
from test_gpu_parity import FIELDS, assert_same_records
from test_gpu_windows import _digest

pytestmark = pytest.mark.gpu
ALL = (1 << 64) - 1
WINDOWS = (1 << 16, 150_000, 1 << 30)
STRINGENCIES = (orc.STRICT, orc.LENIENT, orc.SILENT)
assert (hbam.STRICT, hbam.LENIENT, hbam.SILENT) == STRINGENCIES


def _device_decode(f, first, rc, want):
    """decode_span_device over the whole file: its counts and digests, or the
    oracle's error (the call reports a failing record as an error)."""
    if rc != 0:
        with pytest.raises(hbam.HbamError) as e:
            f.decode_span_device(first, ALL)
        assert e.value.code == rc
        return
    st = f.decode_span_device(first, ALL)
    assert st["status"] == 0 and st["records"] == len(want["key"])
    assert st["first_voff"] == want["voff"][0] and st["last_voff"] == want["voff"][-1]
    assert (st["key_xor"], st["voff_sum"]) == _digest(want)


def _check_file(name, window, stringency):
    """Every entry point over the whole file against the oracle."""
    c = cc.get(name)
    s, rc, want = cc.expected(name, stringency)
    with hbam.BamFile(c["data"], window_bytes=window, stringency=stringency) as f:
        first = f.header()["first_record_voff"]
        got = f.decode_all(raise_on_error=False)
        assert got["status"] == rc
        assert_same_records(got, want, c["u"])
        _device_decode(f, first, rc, want)
        if stringency == orc.STRICT:  # (the indexer does not depend on it)
            for g in (1, 5):
                assert f.splitting_index(g) == s.splitting_index(g)


def _paths(name, stringency):
    """The chain's counters over one device decode of the whole file in one window."""
    c = cc.get(name)
    _, rc, want = cc.expected(name, stringency)
    with hbam.BamFile(c["data"], window_bytes=1 << 30, stringency=stringency) as f:
        first = f.header()["first_record_voff"]
        c0, p0 = f.chain_counters(), f.pipeline_counters()
        _device_decode(f, first, rc, want)
        c1, p1 = f.chain_counters(), f.pipeline_counters()
    d = {k: c1[k] - c0[k] for k in c1}
    d.update({k: p1[k] - p0[k] for k in ("link_fallbacks", "link_rewalks")})
    print(f"chain path {name} stringency {stringency}: {d}")
    return d


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(cc.FALSE_START_CASES))
def test_false_starts_match_oracle(name, window):
    for stringency in STRINGENCIES:
        _check_file(name, window, stringency)
    c = cc.get(name)
    s, _, want = cc.expected(name, orc.STRICT)
    ends = c["starts"] + [len(c["u"])]
    with hbam.BamFile(c["data"], window_bytes=window) as f:
        # spans that start at the true record just before / just after each
        # decoy and end with the file / just past the decoy's first byte
        for d in c["decoys"]:
            for q in (ends[d["host"]], ends[d["host"] + 1]):
                if q == len(c["u"]):
                    continue
                for ve in (ALL, s.voff_of(d["pos"] + 1)):
                    rc, wsp = s.decode_span(s.voff_of(q), ve)
                    got = f.decode_span(s.voff_of(q), ve, raise_on_error=False)
                    assert got["status"] == rc == 0
                    assert_same_records(got, wsp, c["u"])
        parts = list(f.iter_batches(f.header()["first_record_voff"], ALL, 333))
        assert all(0 < len(p["key"]) <= 333 for p in parts)
        for k in FIELDS:
            np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), want[k], err_msg=k)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", list(cc.IMPLAUSIBLE_CASES))
def test_implausible_records_match_oracle(name, window):
    """The oracle is the specification: a record the reference reader takes
    under SILENT (block_size >= 32, bytes present, reference indices in range)
    is a record, whatever plausible() says of it.  (BAMRecordCodec decodes
    the variable-length part lazily, so under SILENT nothing reads l_seq,
    l_read_name or the name's end; the oracle does the same.  Whether LENIENT
    or STRICT stop at the record is the oracle's restated validation.)"""
    for stringency in STRINGENCIES:
        _check_file(name, window, stringency)


@pytest.mark.parametrize("name", list(cc.FALSE_START_CASES))
def test_false_start_paths(name):
    d = _paths(name, orc.STRICT)
    passes = d["link_rounds"] - d["link_rewalks"]  # record passes (a pass ends with a clean round or the serial link)
    if name in ("merge", "merge3"):
        assert d["rewalked"] >= 1 and d["searched"] == 0 and d["dropped"] == 0
    elif name == "deadend":
        assert d["searched"] >= 1 and d["rewalked"] == 0 and d["dropped"] == 0
    elif name == "look3":
        # the decoy's block (3 records past it: not enough) and the block after
        # it, which starts on those 3 records and meets the bad head inside
        assert d["searched"] == 2 * passes and d["rewalked"] == 0 and d["dropped"] == 0
    elif name in ("look4", "stray_in"):
        # the decoy's walk stands (a listed stray walk in a pass-through block,
        # exit <= in: ignored; its records are not in the output, checked by
        # the digests above); only the block after it is searched
        assert d["searched"] == passes and d["rewalked"] == 0 and d["dropped"] == 0
    elif name == "stray_out":
        assert d["dropped"] >= 1
    elif name == "cascade":
        assert d["dropped"] >= 1 and (d["link_rounds"] > 1 or d["link_fallbacks"] >= 1)
    elif name == "shift1":
        # k_rec_cand's 1-3-byte rescue takes t: the block is on the chain at once
        assert d["rewalked"] == 0 and d["dropped"] == 0 and d["link_fallbacks"] == 0
    else:
        assert name.startswith("tail")
    assert passes >= 1


@pytest.mark.parametrize("name", list(cc.IMPLAUSIBLE_CASES))
def test_implausible_record_paths(name):
    """Correctness is the assertion (inside _paths); the path is printed for
    DESIGN.md's table."""
    for stringency in (orc.SILENT, orc.STRICT):
        d = _paths(name, stringency)
        assert d["link_rounds"] >= 1
