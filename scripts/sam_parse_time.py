#!/usr/bin/env python3
"""What parsing SAM text into BAM records costs on the GPU, next to writing
the same records as that text.

For each of two inputs from hbam.synth -- a C2-shaped short-read file (1 M
records by default) and the long-read mode -- the file is made resident and
decoded once in a device session (hbam.Gpu), formatted (hbam_gpu_format_sam)
and the text fetched to the host.  Then, alternating, `reps` rounds of `iters`
launches each (HIP events inside the library):
  * hbam_parse_sam of the whole text on a codec ctx with the file's
    dictionary; hbam_parse_sam_times gives the line finding, the measure pass,
    the scan and the write pass of every call (the upload of the text and the
    copy of the records back are outside those events);
  * hbam_gpu_format_sam of the same records: the opposite direction, the
    yardstick.
Last, the text is copied host -> device from page-locked memory, timed
(hbam_gpu_reload): the rate of the link the text arrives over.
Per input one JSON line: the four parse times (medians of the rounds' means,
with min and max), the text's bytes and GB/s of text parsed, the three format
times, and the copy's GB/s.

Every GPU step runs under a time limit of its own: a step that overruns ends
the process (a traceback on stderr, exit status 1) before anything else is
started.
"""
import argparse
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys
from contextlib import contextmanager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))

import numpy as np  # noqa: E402

import hbam  # noqa: E402
from hbam import synth  # noqa: E402


@contextmanager
def limit(seconds, what):
    """The step ends the process if it takes longer (also when blocked inside the library)."""
    print(f"[sam_parse_time] {what}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def ref_names(data, device):
    with hbam.BamFile(data, device=device) as f:
        return [f.ref(i)[0] for i in range(f.header()["n_ref"])]


def measure(name, data, records, a):
    with limit(120, f"{name}: the dictionary"):
        names = ref_names(data, a.device)
    g = hbam.Gpu(a.device)
    c = hbam.Codec(a.device)
    parse, fmt = ([], [], [], []), ([], [], [])
    h2d = None
    try:
        with limit(180, f"{name}: load + decode + format + fetch"):
            g.load(data)
            assert g.run()["records"] == records
            _, text_bytes = g.format_sam(iters=1)
            text = np.frombuffer(g.fetch_encoded(0, text_bytes), np.uint8)
            assert int(np.count_nonzero(text == 10)) == records
        c.parse_sam_dict(names)
        r = hbam.SamRecords()
        ms = (C.c_float * 4)()

        def parse_once():
            rc = hbam.lib().hbam_parse_sam(c._h, text.ctypes.data, len(text), 1, C.byref(r))
            c._ok(rc)
            c._ok(hbam.lib().hbam_parse_sam_times(c._h, ms))
            assert r.n == records and r.consumed == len(text)
            return list(ms)

        with limit(120, f"{name}: warm-up"):
            parse_once()
            enc_bytes = int(r.bytes)
        for rep in range(a.reps):
            with limit(180, f"{name}: round {rep}"):
                t = [parse_once() for _ in range(a.iters)]
                for k in range(4):
                    parse[k].append(sum(x[k] for x in t) / a.iters)
                t, nb = g.format_sam(iters=a.iters)
                assert nb == text_bytes
                for k in range(3):
                    fmt[k].append(t[k])
        with limit(120, f"{name}: host -> device copy of the text"):
            with hbam.PinnedBuffer(len(text)) as pin:
                pin.array[:] = text
                copies = [g.reload(pin.ptr, len(text), pinned=True) for _ in range(5)]
            h2d = round(len(text) / statistics.median(copies) / 1e6, 1)
    finally:
        c.close()
        g.close()
    p = [statistics.median(x) for x in parse]
    f = [statistics.median(x) for x in fmt]
    print(json.dumps({"input": name, "records": records, "text_bytes": text_bytes, "record_bytes": enc_bytes,
                      "parse_sam": {"lines_ms": spread(parse[0]), "measure_ms": spread(parse[1]),
                                    "scan_ms": spread(parse[2]), "write_ms": spread(parse[3]),
                                    "total_ms": round(sum(p), 4), "text_gbps": round(text_bytes / sum(p) / 1e6, 1)},
                      "format_sam": {"measure_ms": spread(fmt[0]), "scan_ms": spread(fmt[1]), "write_ms": spread(fmt[2]),
                                     "total_ms": round(sum(f), 4), "text_gbps": round(text_bytes / sum(f) / 1e6, 1)},
                      "pinned_h2d_gbps": h2d}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=1_000_000, help="short-read records")
    ap.add_argument("--long-records", type=int, default=4000, help="long-read records")
    ap.add_argument("--reps", type=int, default=5)
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
