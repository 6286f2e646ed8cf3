"""bench.py's launch path on CPU: `--gpus N` with no launcher starts N rank
processes itself (the driver may run `python bench.py --gpus 8` directly),
and under a launcher --gpus must match WORLD_SIZE.  --dry-run stops after the
gloo rendezvous, so nothing here touches a GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env.update(kw)
    return env


def test_gpus_n_spawns_n_ranks():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--dist-backend", "gloo", "--dry-run"],
                       capture_output=True, text=True, timeout=180, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # rank 0's line only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 3
    assert [r["rank"] for r in d["ranks"]] == [0, 1, 2]
    assert [r["local_rank"] for r in d["ranks"]] == [0, 1, 2]
    assert len({r["pid"] for r in d["ranks"]}) == 3


def test_world_size_must_match_gpus():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run"], capture_output=True, text=True,
                       timeout=60, env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert p.returncode == 2
    assert "WORLD_SIZE" in p.stderr


def test_failing_rank_fails_the_run():
    # a bad backend name makes every rank fail at rendezvous: the parent must
    # not hang and must exit non-zero
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dist-backend", "gloo", "--dry-run"],
                       capture_output=True, text=True, timeout=180,
                       env=_env(MASTER_ADDR="127.0.0.1", HBAM_BENCH_FAIL_RANK="1"))
    assert p.returncode != 0


def test_full_and_dump_options_exist_and_steps_must_be_positive():
    """A plain run is the headline only; --full and --dump-outputs are options
    of their own, and --steps sets the number of timed steps (0 is refused)."""
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60, env=_env())
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs DIR" in p.stdout
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--dry-run"], capture_output=True,
                       text=True, timeout=60, env=_env())
    assert p.returncode == 2 and "--steps" in p.stderr


def test_inflate_rounds_match_the_library():
    """bench.py divides phase A's time over INFLATE_ROUNDS launches per chunk:
    it must be the library's kInflateRounds (HBAM_INFLATE_ROUNDS default)."""
    import re
    src = open(os.path.join(ROOT, "hadoop-bam_amd", "csrc", "hbam_device.h")).read()
    rounds = int(re.search(r"#define HBAM_INFLATE_ROUNDS (\d+)", src).group(1))
    bench = open(BENCH).read()
    assert int(re.search(r"^INFLATE_ROUNDS = (\d+)", bench, re.M).group(1)) == rounds


def test_roofline_bound_names_a_unit_only_when_it_is_near_saturation():
    """roofline.bound: the largest measured limit's unit when it reaches 0.7,
    "latency" when no unit is near its peak (round-5 verdict: 0.46 of the LDS
    array is not an LDS bound)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.BOUND_MIN == 0.7
    lim = {"hbm": 0.08, "valu_issue": 0.39, "salu_issue": 0.14, "lds": 0.46, "hbm_traffic": 0.13}
    assert bench.bound_of(lim) == "latency"
    assert bench.bound_of(dict(lim, lds=0.85)) == "lds"
    assert bench.bound_of(dict(lim, hbm_traffic=0.72)) == "hbm"
    assert bench.bound_of(dict(lim, valu_issue=0.7)) == "valu_issue"
