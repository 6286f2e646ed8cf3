"""SAM text of a BAM file, formatted on the GPU (`samtools view` / the
reference's SAMRecordWriter over a whole file).

    import hbam.sam
    n = hbam.sam.view("in.bam", "out.sam")

The file is decoded in bounded batches (hbam_decode_span) and every batch is
formatted from its copy in HBM (hbam_format_sam): no record is formatted on the
host.  Float tags print as C's %g (samtools' text), not as htsjdk's
Float.toString; see include/hbam.h for the rules.

    n = hbam.sam.to_bam("in.sam", "out.bam")

goes the other way (`samtools view -b`): the alignment lines are parsed on the
GPU in chunks (hbam_parse_sam) and written through hbam.writer.BamWriter, whose
blocks are deflated on the GPU.  split_text is the host rule by which the
reference's SAMRecordReader assigns the lines of a file to byte splits.
"""
import ctypes as C
import struct

import hbam
from hbam.writer import BamWriter

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


def _leading_header(data):
    """The length of the leading run of '@' lines of data (a partial last line counts)."""
    p = 0
    while p < len(data) and data[p:p + 1] == b"@":
        nl = data.find(b"\n", p)
        p = len(data) if nl < 0 else nl + 1
    return p


def to_bam(src, dst, level=5, chunk_bytes=64 << 20, eof=True, device=0):
    """Write the SAM text `src` (a path, or the text's bytes) as the BAM `dst`
    (a path, or a binary file object).  The leading '@' lines are the header:
    its BAM form comes from hbam_sam_header_to_bam and its @SQ names are the
    dictionary RNAME and RNEXT resolve against.  The alignment lines are
    parsed chunk_bytes at a time (hbam_parse_sam, a chunk's partial last line
    carried into the next) and written with BamWriter.write_records.  eof: the
    BGZF terminator block ends the file.  Returns the record count."""
    if chunk_bytes <= 0:
        raise ValueError("chunk_bytes must be positive")
    if isinstance(src, str) or hasattr(src, "__fspath__"):
        with open(src, "rb") as f:
            data = f.read()
    else:
        data = bytes(src)
    own = isinstance(dst, (str, bytes)) or hasattr(dst, "__fspath__")
    out = open(dst, "wb") if own else dst
    n = 0
    try:
        h = _leading_header(data)
        header = hbam.sam_header_to_bam(data[:h])
        (l_text,) = struct.unpack_from("<i", header, 4)
        p = 12 + l_text
        names = []
        for _ in range(struct.unpack_from("<i", header, 8 + l_text)[0]):
            (ln,) = struct.unpack_from("<i", header, p)
            names.append(header[p + 4:p + 4 + ln - 1])
            p += 8 + ln
        w = BamWriter(out, header=header, level=level, device=device)
        with hbam.Codec(device=device) as c:
            c.parse_sam_dict(names)
            view = memoryview(data)
            p = h
            while p < len(data):
                q = min(len(data), p + chunk_bytes)
                final = q == len(data)
                enc, offs, used = c.parse_sam(view[p:q], final=final)
                if used == 0 and not final:  # no newline in the chunk: take more
                    nl = data.find(b"\n", q)
                    q = len(data) if nl < 0 else nl + 1
                    enc, offs, used = c.parse_sam(view[p:q], final=q == len(data))
                w.write_records(enc, offs)
                n += len(offs) - 1
                p += used
        w.close(eof=eof)
    finally:
        if own:
            out.close()
    return n


def split_text(data, start, length):
    """The alignment lines of the SAM text `data` that the byte split [start,
    start + length) owns, as the reference's SAMRecordReader assigns them
    (host only): the lines whose first byte lies in the split.  The split at 0
    drops the header lines (the leading run of '@' lines); a later split backs
    up one byte and skips through the first newline, so a line that begins
    exactly at `start` is its own; every split reads through the newline at or
    behind its last byte.  Returns the lines with their newlines (the file's
    last line as it stands)."""
    data = bytes(data)
    end = min(len(data), start + length)
    p = _leading_header(data)
    if start > 0:
        nl = data.find(b"\n", start - 1)
        p = max(p, len(data) if nl < 0 else nl + 1)  # (a split that begins inside the header owns none of it)
    lines = []
    while p < end:
        nl = data.find(b"\n", p)
        q = len(data) if nl < 0 else nl + 1
        lines.append(data[p:q])
        p = q
    return lines
