"""Sort a BAM on the GPU: decode -> hbam_sort_writables -> BGZF write, the
records staying in HBM between the decode and the sorted encoding.

This is the reference's sort job plus util/GetSortedBAMHeader's header
rewrite.  The map side (the shuffle orders records by BAMRecordReader.getKey)
sorts one batch of one window; a file that decodes as one window is written
straight from it.  With merge=True a file of any number of windows is sorted
batch by batch into runs, and the reduce side -- Hadoop's merge of the sorted
map outputs, hbam_merge_* -- streams the merged order part by part into one
writer.  The runs stay in host memory or, with spill_dir, in mapped files."""
import ctypes as C
import os
import tempfile

import numpy as np

from . import E_ARG, E_STATE, OK, SORT_ORDERS, STRICT, BamFile, Batch, Codec, HbamError, _L
from .writer import BamWriter

MERGE_BATCH_RECORDS = 1 << 20  # records per run at most (a run is also cut at its window's end)


def sort_words(key, ref_id, pos, order):
    """The 64-bit word hbam_sort_writables and hbam_merge_* order records by
    (k_sort_words, restated in NumPy): "key": (uint64)key ^ 1 << 63;
    "coordinate": (uint64)(uint32)refID << 32 | (uint32)(pos + 1).  Ascending
    unsigned order of the words is the order's.  "queryname" has no such word
    (its key is the read name's bytes): HbamError(E_ARG)."""
    o = SORT_ORDERS.get(order, order)
    if o == SORT_ORDERS["queryname"]:
        raise HbamError(E_ARG, "queryname order has no sort word")
    if o == SORT_ORDERS["key"]:
        return np.asarray(key, np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    if o != SORT_ORDERS["coordinate"]:
        raise HbamError(E_ARG, f"unknown sort order {order}")
    ref = np.asarray(ref_id, np.int32).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    pos1 = (np.asarray(pos, np.int32).astype(np.int64) + 1).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return (ref << np.uint64(32)) | pos1


def sorted_header(header_bytes: bytes, order="coordinate") -> bytes:
    """The BAM header (magic, l_text, text, references) with SO:coordinate in
    its @HD line: an existing SO: value is replaced, an @HD line without one
    gets "\\tSO:coordinate" appended, a text without an @HD line gets
    "@HD\\tVN:1.5\\tSO:coordinate\\n" in front.  l_text follows; every other
    byte is kept.  The role of util/GetSortedBAMHeader; htsjdk re-serialises
    the whole header there, and byte equality with that is not claimed.
    order "queryname": SO:queryname by the same three rules (no SS field is
    written: the collation is hbam_sort_writables', not one SS names)."""
    if order not in ("coordinate", "queryname"):
        raise ValueError(f"no SO: value for order {order!r}")
    so = b"SO:" + order.encode()
    h = bytes(header_bytes)
    if h[:4] != b"BAM\x01":
        raise ValueError("not a BAM header")
    l_text = int.from_bytes(h[4:8], "little")
    text, rest = h[8:8 + l_text], h[8 + l_text:]
    if text.startswith(b"@HD\t") or text.startswith(b"@HD\n") or text.rstrip(b"\0") == b"@HD":
        end = text.find(b"\n")
        if end < 0:  # a single unterminated line (NUL padding after it stays where it is)
            end = len(text.rstrip(b"\0"))
        fields = text[:end].split(b"\t")
        if any(f.startswith(b"SO:") for f in fields[1:]):
            fields = [fields[0]] + [so if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            fields.append(so)
        text = b"\t".join(fields) + text[end:]
    else:
        text = b"@HD\tVN:1.5\t" + so + b"\n" + text
    return h[:4] + len(text).to_bytes(4, "little") + text + rest


def sort_bam(src, out, order="coordinate", level=5, splitting_bai=None, granularity=4096, eof=True, device=0,
             stringency=STRICT, window_bytes=0, merge=False, part_bytes=0, spill_dir=None):
    """Write the BAM `src` (a path or the file's bytes) to `out` (a path or a
    binary file object) with its records sorted on the GPU: order "coordinate"
    (the header gets SO:coordinate), "queryname" (by read name, then first /
    second of pair and primary before secondary / supplementary; the header
    gets SO:queryname) or "key" (the shuffle's order, header unchanged).  Ties
    keep the input order.  splitting_bai: a binary file
    object that receives the write-time .splitting-bai.  Returns the number of
    records.  Without merge the file must decode as one window of window_bytes
    compressed bytes (0: the library's default).  merge=True: the file is read
    in batches of one window at most, each sorted into a run, and the runs are
    merged on the GPU (hbam_merge_*) in parts of part_bytes (0: 1 GiB) into the
    one writer: one header, one .splitting-bai, one EOF block, and the same
    bytes as the one-window sort of the same records.  spill_dir: each run's
    bytes go to a file there and are mapped read-only (the offsets stay in
    memory); the files are removed on return and on error."""
    if merge:
        return _sort_bam_merge(src, out, order, level, splitting_bai, granularity, eof, device, stringency,
                               window_bytes, part_bytes, spill_dir)
    opened = None
    kw = dict(device=device, stringency=stringency, window_bytes=window_bytes)
    f = BamFile(path=os.fspath(src), **kw) if isinstance(src, (str, os.PathLike)) else BamFile(src, **kw)
    try:
        header = f.header_bytes()
        if order in ("coordinate", "queryname"):
            header = sorted_header(header, order)
        # the whole file as one batch, left in the library's columns (nothing copied into Python)
        b = Batch()
        rc = _L.hbam_decode_span(f._h, f.header()["first_record_voff"], (1 << 64) - 1, 0, C.byref(b))
        if rc != OK:
            raise f._err(rc)
        f._last_n = b.n
        try:
            enc, offs, _ = f.sort_writables(order)
        except HbamError as e:
            if e.code != E_STATE:
                raise
            raise HbamError(E_STATE, f"{e.args[0].split(': ', 1)[-1]}: the file does not decode as one window "
                                     f"(window_bytes={window_bytes or 'default'}); pass merge=True to sort it "
                                     f"window by window and merge the runs, or open it with a larger "
                                     f"window_bytes") from None
        if isinstance(out, (str, os.PathLike)):
            out = opened = open(out, "wb")
        w = BamWriter(out, header=header, level=level, splitting_bai=splitting_bai, granularity=granularity,
                      device=device)
        w.write_records(enc, offs)
        w.close(eof=eof)
        return int(b.n)
    finally:
        f.close()
        if opened is not None:
            opened.close()


def _sort_bam_merge(src, out, order, level, splitting_bai, granularity, eof, device, stringency, window_bytes,
                    part_bytes, spill_dir):
    if SORT_ORDERS.get(order, order) not in SORT_ORDERS.values():
        raise HbamError(E_ARG, f"unknown sort order {order}")
    opened = None
    spilled = []
    kw = dict(device=device, stringency=stringency, window_bytes=window_bytes)
    f = BamFile(path=os.fspath(src), **kw) if isinstance(src, (str, os.PathLike)) else BamFile(src, **kw)
    # queryname order has no sort words: merge_add_run decodes each run
    # (hbam_decode_writables), which would end the split iter_batches is
    # reading on the file's ctx, so this order's merge runs on a ctx of its own
    by_name = SORT_ORDERS.get(order, order) == SORT_ORDERS["queryname"]
    m = f
    try:
        if by_name:
            m = Codec(device)
        header = f.header_bytes()
        if order in ("coordinate", "queryname"):
            header = sorted_header(header, order)
        m.merge_begin(order)
        total = 0
        for r in f.iter_batches(f.header()["first_record_voff"], (1 << 64) - 1, MERGE_BATCH_RECORDS):
            if r["status"] != OK:
                raise f._err(r["status"])
            enc, offs, perm = f.sort_writables(order)
            words = None if by_name else sort_words(r["key"], r["ref_id"], r["pos"], order)[perm]
            if spill_dir is not None and len(enc):
                fd, path = tempfile.mkstemp(prefix="hbam_run_", suffix=".spill", dir=os.fspath(spill_dir))
                spilled.append(path)
                with os.fdopen(fd, "wb") as g:
                    g.write(enc)
                enc = np.memmap(path, np.uint8, "r")
            m.merge_add_run(enc, offs, words)
            total += len(perm)
        if isinstance(out, (str, os.PathLike)):
            out = opened = open(out, "wb")
        w = BamWriter(out, header=header, level=level, splitting_bai=splitting_bai, granularity=granularity,
                      device=device)
        for enc, offs, _ in m.iter_merged(part_bytes):
            w.write_records(enc, offs)
        w.close(eof=eof)
        m.merge_end()
        return total
    finally:
        try:
            m.merge_end()  # (drops the references to the mapped runs before their files go)
        finally:
            if m is not f:
                m.close()
            f.close()
            for path in spilled:
                try:
                    os.unlink(path)
                except OSError:
                    pass
            if opened is not None:
                opened.close()
