#!/usr/bin/env python3
"""What writing a decoded batch as SAM text costs on the GPU, next to
re-encoding it as SAMRecordWritable bytes.

For each of two inputs from hbam.synth -- a C2-shaped short-read file (1 M
records by default) and the long-read mode -- the file is made resident and
decoded once in a device session (hbam.Gpu).  Then, alternating, `reps` rounds
of `iters` launches each (HIP events inside the library):
  * hbam_gpu_format_sam: the measuring pass, the scan of the line lengths and
    the writing pass;
  * hbam_gpu_encode_writables: the existing output path that moves comparable
    bytes, the yardstick.
Per input two lines are printed: the three times of the text (medians, with
min and max), its bytes and GB/s of text written; then the encode's ms, its
bytes, and the ratios write pass / encode per launch and per output byte.

Every GPU step runs under a time limit of its own: a step that overruns ends
the process (a traceback on stderr, exit status 1) before anything else is
started.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
from contextlib import contextmanager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))

import hbam  # noqa: E402
from hbam import synth  # noqa: E402


@contextmanager
def limit(seconds, what):
    """The step ends the process if it takes longer (also when blocked inside the library)."""
    print(f"[sam_text_time] {what}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def measure(name, data, records, a):
    g = hbam.Gpu(a.device)
    fmt, enc = ([], [], []), []
    try:
        with limit(120, f"{name}: load + decode"):
            g.load(data)
            assert g.run()["records"] == records
        with limit(60, f"{name}: warm-up"):
            _, text_bytes = g.format_sam(iters=1)
            _, enc_bytes = g.encode_writables(iters=1)
        for rep in range(a.reps):
            with limit(60, f"{name}: round {rep}"):
                t, nb = g.format_sam(iters=a.iters)
                assert nb == text_bytes
                for k in range(3):
                    fmt[k].append(t[k])
                ms, nb = g.encode_writables(iters=a.iters)
                assert nb == enc_bytes
                enc.append(ms)
    finally:
        g.close()
    m, s, w = (statistics.median(x) for x in fmt)
    e = statistics.median(enc)
    print(json.dumps({"input": name, "records": records, "format_sam": {
        "measure_ms": spread(fmt[0]), "scan_ms": spread(fmt[1]), "write_ms": spread(fmt[2]),
        "total_ms": round(m + s + w, 4), "text_bytes": text_bytes,
        "write_text_gbps": round(text_bytes / w / 1e6, 1), "total_text_gbps": round(text_bytes / (m + s + w) / 1e6, 1)}}))
    print(json.dumps({"input": name, "encode_writables": {
        "ms": spread(enc), "bytes": enc_bytes, "gbps_written": round(enc_bytes / e / 1e6, 1),
        "write_over_encode": round(w / e, 3), "total_over_encode": round((m + s + w) / e, 3),
        "write_over_encode_per_output_byte": round((w / text_bytes) / (e / enc_bytes), 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=1_000_000, help="short-read records")
    ap.add_argument("--long-records", type=int, default=4000, help="long-read records")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x53414D54)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    for name, mode, n in (("short", "short", a.records), ("long", "long", a.long_records)):
        data, _ = synth.make_bam(n, mode=mode, seed=a.seed, as_numpy=True)
        measure(name, data, n, a)


if __name__ == "__main__":
    main()
