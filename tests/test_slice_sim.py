"""scripts/slice_sim.c, the host model of phase A with the lane count as a
parameter (the figures the narrow instance was decided on), against
scripts/dual_sim.c, the model the design's earlier figures come from: at 256
lanes, with one and with two slices per lane, both must print the same
numbers for the same file.  dual_sim alternates its two rows DEFLATE block by
DEFLATE block ("1st", "2nd"), slice_sim tells a BGZF block's first DEFLATE
block from its later ones: the same thing over BGZF blocks of two DEFLATE
blocks each, which is what the comparison runs on (the file less its short
last data block and the EOF block)."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT
from hbam import synth

ROW = re.compile(r"DEFLATE block (\w+), .*?: per wave spec ([\d.]+)\s+sync \(all iterations\) ([\d.]+)\s+emit ([\d.]+)\s+"
                 r"total ([\d.]+);.*sync iterations per block ([\d.]+), symbols/slice ([\d.]+)")


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp("slice_sim")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler builds the model"
    exe = {}
    for name in ("slice_sim", "dual_sim"):
        exe[name] = str(d / name)
        subprocess.run([cc, "-O2", "-o", exe[name], os.path.join(ROOT, "scripts", name + ".c")], check=True,
                       capture_output=True, timeout=120)
    data, _ = synth.make_bam(2000)
    bam = str(d / "c2.bam")
    data = bytes(data)
    with open(bam, "wb") as f:
        f.write(data)
    nblocks, p = 0, 0
    while p < len(data):
        p += struct.unpack_from("<H", data, p + 16)[0] + 1
        nblocks += 1
    assert nblocks >= 8
    return exe, bam, str(nblocks - 2)


def rows(exe, *args):
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True, timeout=120).stdout
    return {m.group(1): tuple(m.group(i) for i in range(2, 8)) for m in map(ROW.search, out.splitlines()) if m}, out


@pytest.mark.parametrize("per", [1, 2])
def test_256_lane_rows_equal_dual_sim(sims, per):
    exe, bam, nb = sims
    new, out = rows(exe["slice_sim"], bam, nb, "256", str(per))
    old, _ = rows(exe["dual_sim"], bam, nb, str(256 * per))
    assert "bgzf blocks %s, deflate blocks %d," % (nb, 2 * int(nb)) in out  # two DEFLATE blocks each
    assert set(new) == {"first", "second"} and set(old) == {"1st", "2nd"}, out
    assert new["first"] == old["1st"]
    assert new["second"] == old["2nd"]


def test_narrower_workgroups_issue_fewer_wave_steps_for_the_second_block(sims):
    """Wave-steps per block = steps per wave x waves, as printed; the model's
    claim for a C2-like file is that the short second block costs fewer of
    them at 128 lanes than at 256."""
    exe, bam, nb = sims
    ws = {}
    for lanes in (256, 128, 64):
        r, out = rows(exe["slice_sim"], bam, nb, str(lanes))
        m = re.search(r"DEFLATE block second, .*total ([\d.]+); wave-steps per block ([\d.]+)", out)
        assert abs(float(m.group(1)) * (lanes // 64) - float(m.group(2))) <= 0.1 * (lanes // 64), out
        ws[lanes] = float(m.group(2))
    assert ws[128] < ws[256]
    assert re.search(r"round-1 window bytes over \d+ blocks: p1 \d+  p50 \d+", out)
