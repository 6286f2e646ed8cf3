"""SAM text of a BAM file, formatted on the GPU (`samtools view` / the
reference's SAMRecordWriter over a whole file).

    import hbam.sam
    n = hbam.sam.view("in.bam", "out.sam")

The file is decoded in bounded batches (hbam_decode_span) and every batch is
formatted from its copy in HBM (hbam_format_sam): no record is formatted on the
host.  Float tags print as C's %g (samtools' text), not as htsjdk's
Float.toString; see include/hbam.h for the rules.
"""
import ctypes as C

import hbam

VEND = (1 << 64) - 1


def header_text(f) -> bytes:
    """The l_text bytes of the header, with one newline added when the text is
    non-empty and lacks it."""
    h = hbam.HeaderInfo()
    rc = hbam.lib().hbam_header(f._h, C.byref(h))
    if rc != hbam.OK:
        raise f._err(rc)
    text = C.string_at(h.text, h.l_text) if h.l_text else b""
    if text and not text.endswith(b"\n"):
        text += b"\n"
    return text


def view(src, dst, header=True, batch_records=1 << 20, **open_opts):
    """Write the SAM text of the BAM `src` (a path, or the file's bytes) to
    `dst` (a path, or a binary file object): the header text when `header`,
    then one line per record, batch_records records at a time.  open_opts go
    to hbam.BamFile (device, stringency, window_bytes, ...).  Returns the
    record count."""
    if batch_records <= 0:
        raise ValueError("batch_records must be positive")
    own = isinstance(dst, (str, bytes)) or hasattr(dst, "__fspath__")
    out = open(dst, "wb") if own else dst
    opts = dict(open_opts)
    opts.setdefault("batch_records", batch_records)
    f = hbam.BamFile(path=src, **opts) if isinstance(src, str) or hasattr(src, "__fspath__") \
        else hbam.BamFile(src, **opts)
    n = 0
    try:
        if header:
            out.write(header_text(f))
        b = hbam.Batch()
        v = f.header()["first_record_voff"]
        while v < VEND:
            rc = hbam.lib().hbam_decode_span(f._h, v, VEND, batch_records, C.byref(b))
            if rc != hbam.OK:
                raise f._err(rc)
            if b.n == 0:
                break
            f._last_n = b.n
            text, _ = f.format_sam()
            out.write(text)
            n += b.n
            v = b.next_voff
    finally:
        f.close()
        if own:
            out.close()
    return n
