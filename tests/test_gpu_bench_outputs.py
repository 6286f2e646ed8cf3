"""bench.py's plain run and --dump-outputs on the GPU, at a small C2
(200,000 records: 4 sampled places, several BGZF blocks each): the result line
holds the headline only, and the dumped arrays are the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from hbam import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200_000


def _u64(a):
    """(n, 2) high / low 32-bit halves -> uint64."""
    return (a[:, 0].astype(np.uint64) << np.uint64(32)) | a[:, 1].astype(np.uint64)


def _limbs(a):
    v = 0
    for x in a:
        v = (v << 16) | int(x)
    return v


def test_plain_run_is_lean_and_dump_matches_oracle(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--records", str(N), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # value = inflated bytes of the timed steps / their time
    assert d["value"] == pytest.approx(d["config"]["uncompressed_bytes"] / d["ms_per_step"] / 1e6, rel=1e-3)
    for k in ("roofline", "stages_ms", "cpu_baseline", "extra"):  # the --full parts
        assert k not in d, k

    files = sorted(os.listdir(out))
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20

    seg, info = synth.make_bam_segment(N, 0, N, with_header=True, eof_block=True, seed=bench.SEED)
    s = orc.Stream(seg.tobytes())
    rc, want = s.decode_all()
    assert rc == 0 and len(want["key"]) == N
    st = dict(zip(bench.DUMP_STATS, arrs["stats"]))
    assert st["records"] == N and st["status"] == 0
    assert st["inflated_bytes"] == info["uncompressed"] and st["compressed_bytes"] == seg.nbytes
    assert st["first_voff"] == int(want["voff"][0]) and st["last_voff"] == int(want["voff"][-1])
    full, _ = orc.scan(seg, threads=2, mode="decode")
    assert _limbs(arrs["digests"][0]) == full["key_xor"] and _limbs(arrs["digests"][1]) == full["voff_sum"]
    assert _limbs(arrs["digests"][2]) == full["key_digest"] and _limbs(arrs["digests"][3]) == full["voff_digest"]

    voff = _u64(arrs["sample_voff"])
    # the split's start and every DUMP_SPOT_STRIDE-th record (fewer than DUMP_SPOTS here, so all of them)
    starts = [0] + [k * bench.DUMP_SPOT_STRIDE - 1 for k in range(1, N // bench.DUMP_SPOT_STRIDE + 1)]
    assert 1 < len(starts) <= bench.DUMP_SPOTS
    expect = np.concatenate([np.arange(a, min(N, a + bench.DUMP_SPOT_RECORDS)) for a in starts])
    idx = np.searchsorted(want["voff"], voff)
    assert np.array_equal(idx, expect)
    assert np.array_equal(want["voff"][idx], voff)
    assert np.array_equal(_u64(arrs["sample_key"]).view(np.int64), want["key"][idx])
    for f in ("ref_id", "pos", "l_seq", "next_ref_id", "next_pos", "tlen", "l_read_name", "mapq", "bin", "n_cigar",
              "flag", "rest_len"):
        assert np.array_equal(arrs["sample_" + f], want[f][idx].astype(np.float64)), f
    # rest-of-record bytes: their byte sums against the oracle's inflated stream
    csum = np.concatenate(([0], np.cumsum(np.frombuffer(s.data, np.uint8), dtype=np.int64)))
    lo = want["offset"][idx].astype(np.int64) + 36
    assert np.array_equal(arrs["sample_rest_bytes"], (csum[lo + want["rest_len"][idx]] - csum[lo]).astype(np.float64))
