#!/usr/bin/env python3
"""What building the BAM index costs next to decoding the file.

Generates a short-read BAM with hbam.synth (2 M records by default), then in
one process and on one ctx times, alternating after a warm-up of each,
  * hbam_decode_span_device over the whole file (the yardstick: the decode
    pass, which every read of the file pays), and
  * hbam_build_bai (the same window loop + the index kernels + the sort, the
    gap fill and the serialisation),
with a host clock around each call (both end in a device synchronise).  The
file is read from host memory in ramped windows by both, and each pass ends in
another window than the next one starts in, so neither finds its input
inflated already.  Prints one JSON line: medians, spreads and the ratios.

The per-kernel split comes from a run of this script under
`rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host);
the index kernels are k_bai_* and the hipcub scans and sort between them.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))

import hbam  # noqa: E402
from hbam import synth  # noqa: E402

ALL = (1 << 64) - 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-metadata", action="store_true")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    data, info = synth.make_bam(a.records, mode="short")
    t_dec, t_bai, index = [], [], b""
    with hbam.BamFile(data, device=a.device) as f:
        first = f.header()["first_record_voff"]
        for rep in range(a.reps + 1):  # rep 0 warms both up
            t0 = time.perf_counter()
            st = f.decode_span_device(first, ALL, digest=False)
            t1 = time.perf_counter()
            index = f.build_bai(metadata=not a.no_metadata)
            t2 = time.perf_counter()
            assert st["records"] == a.records
            if rep:
                t_dec.append((t1 - t0) * 1e3)
                t_bai.append((t2 - t1) * 1e3)
    s = hbam.bai_summary(index)
    dec, bai = statistics.median(t_dec), statistics.median(t_bai)
    print(json.dumps({
        "records": a.records, "compressed_bytes": info["compressed"], "inflated_bytes": info["uncompressed"],
        "reps": a.reps, "index_bytes": len(index), "n_ref": s["n_ref"], "no_coor_count": s["no_coor_count"],
        "decode_ms": {"median": round(dec, 3), "min": round(min(t_dec), 3), "max": round(max(t_dec), 3)},
        "build_bai_ms": {"median": round(bai, 3), "min": round(min(t_bai), 3), "max": round(max(t_bai), 3)},
        "build_over_decode": round(bai / dec, 4),
        "indexing_share_of_decode": round((bai - dec) / dec, 4),
    }))


if __name__ == "__main__":
    main()
