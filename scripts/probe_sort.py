#!/usr/bin/env python3
"""What sorting a decoded batch costs on the GPU, next to copying it in order.

Generates a C2-like short-read BAM with hbam.synth (1 M records by default),
shuffles its records (the generator's file is sorted already; the shuffled
payload is recompressed by hbam.bgzf_compress at level 1), makes it resident
and decodes it once.  Then, in this one process and on the same records, it
times, alternating, `reps` rounds of `iters` launches each (HIP events inside
the library):
  * hbam_gpu_encode_writables: the in-order copy of the same bytes, the roof
    of the gather;
  * hbam_gpu_sort_writables for the key, coordinate and queryname orders: the
    order (sort words + radix sort; for queryname the name references, the
    census and its read-back, the tie word's pass and the chunk passes, also
    split: hbam_gpu_sort_name_times), lengths + scan, gather;
  * the queryname order once more on a second session of the same file loaded
    with HBAM_NAME_FULL_PASSES=1: every chunk present sorted over all 64 bits,
    the A/B of the census's skipping and narrowing;
and once hbam_gpu_d2d_bandwidth.  Last, the host path a user has without the
feature, `reps` times with a host clock: hbam_decode_span of the whole file
(decode + the batch's D2H; hbam_decode_span_device beside it is the decode
alone), NumPy's stable argsort of the keys, and a byte gather on the host
(bytes.join over the records' rests as the batch delivers them; rebuilding the
36-byte heads from the columns would come on top); and for the queryname order
the names sliced out of the batch's rests and ordered by Python's sorted() and
by NumPy's stable argsort of a fixed-width bytes array (the names alone: no tie
word).

Every GPU step runs under a time limit of its own: a step that overruns ends
the process (a traceback on stderr, exit status 1) before anything else is
started.  Prints one JSON
object: min / median / max per figure.
"""
import argparse
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys
import time
from contextlib import contextmanager

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hadoop-bam_amd"))

import hbam  # noqa: E402
from hbam import synth  # noqa: E402

ALL = (1 << 64) - 1


@contextmanager
def limit(seconds, what):
    """The step ends the process if it takes longer (also when blocked inside the library)."""
    print(f"[probe_sort] {what}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def shuffled_bam(records, seed, device):
    data, info = synth.make_bam(records, mode="short", seed=seed)
    with limit(120, "decode + in-order encoding of the generated file"):
        with hbam.BamFile(data, device=device, stringency=hbam.SILENT) as f:
            header = f.header_bytes()
            n = len(f.decode_all()["key"])
            enc, offs = f.encode_writables()
    assert n == records
    o = offs.astype(np.int64)
    view = memoryview(enc)
    order = np.random.default_rng(seed).permutation(n)
    payload = header + b"".join(view[o[i]:o[i + 1]] for i in order)
    with limit(120, "BGZF compression of the shuffled payload"):
        return hbam.bgzf_compress(payload, block_size=65280, level=1, eof=True, device=device), len(enc)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x534F5254)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    data, nbytes = shuffled_bam(a.records, a.seed, a.device)
    out = {"records": a.records, "record_bytes": nbytes, "compressed_bytes": len(data), "reps": a.reps,
           "iters": a.iters}

    enc_ms, stages = [], {o: ([], [], []) for o in ("key", "coordinate", "queryname")}
    name_ms, full_ms, full_name_ms = ([], [], []), ([], [], []), ([], [], [])
    g = hbam.Gpu(a.device)
    g_full = hbam.Gpu(a.device)  # the same file, every name chunk sorted over 64 bits
    try:
        for s, full in ((g, "0"), (g_full, "1")):
            s.set_stringency(hbam.SILENT)
            with limit(120, "load + decode"):
                os.environ["HBAM_NAME_FULL_PASSES"] = full  # read when the session's pipeline is made
                s.load(data)
                assert s.run()["records"] == a.records
        del os.environ["HBAM_NAME_FULL_PASSES"]
        with limit(60, "warm-up"):
            g.encode_writables(iters=1)
            for order in stages:
                g.sort_writables(order, iters=1)
            g_full.encode_writables(iters=1)
            g_full.sort_writables("queryname", iters=1)
        out["queryname_counters"] = dict(zip(("chunks_present", "chunks_sorted", "bits_sorted"),
                                             g.sort_name_counters()))
        out["queryname_full_counters"] = dict(zip(("chunks_present", "chunks_sorted", "bits_sorted"),
                                                  g_full.sort_name_counters()))
        assert g.fetch_encoded(0, nbytes) == g_full.fetch_encoded(0, nbytes)  # the same order either way
        for rep in range(a.reps):
            with limit(60, f"round {rep}"):
                ms, nb = g.encode_writables(iters=a.iters)
                assert nb == nbytes
                enc_ms.append(ms)
                for order, lists in stages.items():
                    t, nb = g.sort_writables(order, iters=a.iters)
                    assert nb == nbytes
                    for k in range(3):
                        lists[k].append(t[k])
                    if order == "queryname":  # (the split of the round's last launch)
                        for k, v in enumerate(g.sort_name_times()):
                            name_ms[k].append(v)
                t, nb = g_full.sort_writables("queryname", iters=a.iters)
                for k in range(3):
                    full_ms[k].append(t[k])
                for k, v in enumerate(g_full.sort_name_times()):
                    full_name_ms[k].append(v)
        with limit(60, "device-to-device copy bandwidth"):
            out["d2d_gbps"] = round(g.d2d_bandwidth(1 << 30, 5), 1)
    finally:
        g.close()
        g_full.close()
    out["encode_in_order_ms"] = spread(enc_ms)
    enc = statistics.median(enc_ms)
    out["encode_in_order_gbps"] = round(2 * nbytes / enc / 1e6, 1)  # read + write
    for order, (s, l, gth) in stages.items():
        med = statistics.median(gth)
        out[order] = {"sort_ms": spread(s), "offsets_ms": spread(l), "gather_ms": spread(gth),
                      "total_ms": spread([x + y + z for x, y, z in zip(s, l, gth)]),
                      "gather_gbps": round(2 * nbytes / med / 1e6, 1), "gather_over_in_order_copy": round(med / enc, 3)}
    split = ("refs_census_readback_ms", "tie_pass_ms", "chunk_passes_ms")
    out["queryname"].update({k: spread(v) for k, v in zip(split, name_ms)})
    out["queryname_full_passes"] = {"sort_ms": spread(full_ms[0]), "offsets_ms": spread(full_ms[1]),
                                    "gather_ms": spread(full_ms[2])}
    out["queryname_full_passes"].update({k: spread(v) for k, v in zip(split, full_name_ms)})

    t_dev, t_d2h, t_arg, t_gather, t_names, t_sorted, t_np = [], [], [], [], [], [], []
    with hbam.BamFile(data, device=a.device, stringency=hbam.SILENT) as f:
        first = f.header()["first_record_voff"]
        for rep in range(a.reps + 1):  # rep 0 warms up
            with limit(120, f"host path {rep}"):
                t0 = time.perf_counter()
                f.decode_span_device(first, ALL, digest=False)
                t1 = time.perf_counter()
                b = hbam.Batch()
                rc = hbam.lib().hbam_decode_span(f._h, first, ALL, 0, C.byref(b))
                t2 = time.perf_counter()
                assert rc == hbam.OK and b.n == a.records
            keys = np.ctypeslib.as_array((C.c_int64 * b.n).from_address(b.key))
            rest_off = np.ctypeslib.as_array((C.c_uint64 * b.n).from_address(b.rest_off)).astype(np.int64)
            rest_len = np.ctypeslib.as_array((C.c_uint32 * b.n).from_address(b.rest_len)).astype(np.int64)
            raw = memoryview((C.c_uint8 * b.data_len).from_address(b.data)).cast("B")
            t3 = time.perf_counter()
            order = np.argsort(keys, kind="stable")
            t4 = time.perf_counter()
            hi = rest_off + rest_len
            gathered = b"".join(raw[rest_off[i]:hi[i]] for i in order)
            t5 = time.perf_counter()
            assert len(gathered) == nbytes - 36 * a.records
            lrn = np.ctypeslib.as_array((C.c_uint8 * b.n).from_address(b.l_read_name)).astype(np.int64)
            t6 = time.perf_counter()
            ends = (rest_off + np.minimum(lrn, rest_len)).tolist()
            names = [bytes(raw[x:y]) for x, y in zip(rest_off.tolist(), ends)]
            t7 = time.perf_counter()
            by_name = sorted(range(b.n), key=names.__getitem__)
            t8 = time.perf_counter()
            by_name_np = np.argsort(np.array(names, dtype=np.bytes_), kind="stable")
            t9 = time.perf_counter()
            assert len(by_name) == len(by_name_np) == b.n
            if rep:
                t_names.append((t7 - t6) * 1e3)
                t_sorted.append((t8 - t7) * 1e3)
                t_np.append((t9 - t8) * 1e3)
            if rep:
                t_dev.append((t1 - t0) * 1e3)
                t_d2h.append((t2 - t1) * 1e3)
                t_arg.append((t4 - t3) * 1e3)
                t_gather.append((t5 - t4) * 1e3)
    out["host_path"] = {"decode_device_ms": spread(t_dev), "decode_span_with_d2h_ms": spread(t_d2h),
                        "numpy_argsort_ms": spread(t_arg), "host_gather_ms": spread(t_gather),
                        "name_slices_ms": spread(t_names), "python_sorted_names_ms": spread(t_sorted),
                        "numpy_argsort_names_ms": spread(t_np),
                        "host_gather": "bytes.join over the records' rests as the batch delivers them "
                                       "(the 36-byte heads are not rebuilt)"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
