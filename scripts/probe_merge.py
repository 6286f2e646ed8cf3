#!/usr/bin/env python3
"""What merging sorted runs costs on the GPU, next to sorting the same records
in one window and to copying them in order.

Takes the input of scripts/probe_sort.py (1 M shuffled synthetic 150 bp
records by default), cuts its records into k = 1, 4 and 16 consecutive ranges,
puts each range in the stable order of its sort words (on the host: what
hbam_sort_writables gives for that batch) as a run held in host memory, and
merges the runs (hbam_merge_*, key order) with part_bytes of 64 MiB and of
1 GiB.  Per round it records
  * add_run: the host clock around the k hbam_merge_add_run calls (words and
    offsets H2D, the word and framing check, its readback);
  * the plan, by HIP events inside the library: radix sort, lengths + scan,
    parts + cuts;
  * per part, summed over the round's parts, by HIP events: H2D of the
    slices, source table + gather, D2H.
In the same process and on the same records it times hbam_gpu_sort_writables
(one window: the capability the merge extends; its gather copies the same
bytes) and hbam_gpu_encode_writables (the in-order copy: the roof), and states
the merge's gather as a ratio to each.

Every GPU step runs under a time limit of its own, as in probe_sort.py.
Writes one JSON object (min / median / max per figure) to --out and prints it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import hbam  # noqa: E402
from hbam.sort import sort_words  # noqa: E402
from probe_sort import limit, shuffled_bam, spread  # noqa: E402

ORDER = "key"


def decoded(data, records, device):
    """The file's in-order encodings, their offsets and the records' sort words."""
    with hbam.BamFile(data, device=device, stringency=hbam.SILENT) as f:
        r = f.decode_all()
        enc, offs = f.encode_writables()
    assert len(r["key"]) == records
    return enc, offs.astype(np.int64), sort_words(r["key"], r["ref_id"], r["pos"], ORDER)


def sorted_runs(enc, offs, words, k):
    """Exactly k runs: k consecutive ranges of the file's records, each in the
    stable order of its words (what hbam_sort_writables gives for that batch;
    built on the host so that the windows' sizes do not decide k)."""
    n = len(words)
    view = memoryview(enc)
    runs = []
    for r in range(k):
        lo, hi = (n * r) // k, (n * (r + 1)) // k
        p = np.argsort(words[lo:hi], kind="stable") + lo
        ro = np.zeros(hi - lo + 1, np.uint64)
        ro[1:] = np.cumsum(offs[p + 1] - offs[p])
        runs.append((np.frombuffer(b"".join(view[offs[i]:offs[i + 1]] for i in p), np.uint8), ro, words[p]))
    return runs


def merge_round(ctx, runs, part_bytes, out, offs, src):
    """One whole merge: (add_run ms, plan ms[3], per-part ms[3] summed, parts)."""
    L = hbam.lib()
    ctx.merge_begin(ORDER)
    try:
        t0 = time.perf_counter()
        for enc, o, w in runs:
            ctx.merge_add_run(enc, o, w)
        add_ms = (time.perf_counter() - t0) * 1e3
        parts, records, nbytes = ctx.merge_plan(part_bytes)
        plan, _ = ctx.merge_times()
        part = [0.0, 0.0, 0.0]
        n, ln = C.c_uint64(), C.c_uint64()
        done = 0
        while True:
            rc = L.hbam_merge_next(ctx._h, out.ctypes.data, out.nbytes, offs.ctypes.data, src.ctypes.data, C.byref(n),
                                   C.byref(ln))
            assert rc == hbam.OK, rc
            if n.value == 0:
                break
            done += ln.value
            _, t = ctx.merge_times()
            for i in range(3):
                part[i] += t[i]
        assert done == nbytes
        return add_ms, plan, part, parts
    finally:
        ctx.merge_end()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x534F5254)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "probe_merge.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    data, nbytes = shuffled_bam(a.records, a.seed, a.device)
    res = {"records": a.records, "record_bytes": nbytes, "order": ORDER, "reps": a.reps, "iters": a.iters}

    # the two references, on the same records in one window
    enc_ms, gather_ms, sort_total = [], [], []
    g = hbam.Gpu(a.device)
    try:
        g.set_stringency(hbam.SILENT)
        with limit(120, "load + decode"):
            g.load(data)
            assert g.run()["records"] == a.records
        with limit(60, "warm-up"):
            g.encode_writables(iters=1)
            g.sort_writables(ORDER, iters=1)
        for rep in range(a.reps):
            with limit(60, f"reference round {rep}"):
                ms, _ = g.encode_writables(iters=a.iters)
                enc_ms.append(ms)
                t, _ = g.sort_writables(ORDER, iters=a.iters)
                gather_ms.append(t[2])
                sort_total.append(sum(t))
    finally:
        g.close()
    res["encode_in_order_ms"] = spread(enc_ms)
    res["sort_one_window"] = {"gather_ms": spread(gather_ms), "total_ms": spread(sort_total)}
    enc_med, gather_med = statistics.median(enc_ms), statistics.median(gather_ms)

    out = np.empty(nbytes, np.uint8)
    offs = np.empty(a.records + 1, np.uint64)
    src = np.empty(a.records, np.uint64)
    with limit(120, "decode + in-order encoding of the shuffled file"):
        enc, eoffs, words = decoded(data, a.records, a.device)
    with hbam.Codec(a.device) as ctx:
        for k in (1, 4, 16):
            runs = sorted_runs(enc, eoffs, words, k)  # (host work: no GPU step)
            for pb_name, pb in (("64MiB", 64 << 20), ("1GiB", 1 << 30)):
                rows = []
                for rep in range(a.reps + 1):  # round 0 warms up (buffers, hipcub)
                    with limit(120, f"merge k={k} part_bytes={pb_name} round {rep}"):
                        row = merge_round(ctx, runs, pb, out, offs, src)
                    if rep:
                        rows.append(row)
                gth = [r[2][1] for r in rows]
                res[f"k{k}_{pb_name}"] = {
                    "runs": len(runs), "parts": rows[0][3],
                    "add_run_host_ms": spread([r[0] for r in rows]),
                    "plan_sort_ms": spread([r[1][0] for r in rows]),
                    "plan_offsets_ms": spread([r[1][1] for r in rows]),
                    "plan_parts_cuts_ms": spread([r[1][2] for r in rows]),
                    "parts_h2d_ms": spread([r[2][0] for r in rows]),
                    "parts_src_gather_ms": spread(gth),
                    "parts_d2h_ms": spread([r[2][2] for r in rows]),
                    "gather_over_one_window_gather": round(statistics.median(gth) / gather_med, 3),
                    "gather_over_in_order_copy": round(statistics.median(gth) / enc_med, 3),
                }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
