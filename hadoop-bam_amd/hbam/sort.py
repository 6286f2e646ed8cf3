"""Sort a BAM on the GPU: decode -> hbam_sort_writables -> BGZF write, the
records staying in HBM between the decode and the sorted encoding.

This is the map-side sort of the reference's sort job (the shuffle orders
records by BAMRecordReader.getKey) plus util/GetSortedBAMHeader's header
rewrite, for a file that decodes as one window.  Sorting a larger file
(sorted runs + a merge) is not implemented here."""
import ctypes as C
import os

from . import E_STATE, OK, STRICT, BamFile, Batch, HbamError, _L
from .writer import BamWriter


def sorted_header(header_bytes: bytes) -> bytes:
    """The BAM header (magic, l_text, text, references) with SO:coordinate in
    its @HD line: an existing SO: value is replaced, an @HD line without one
    gets "\\tSO:coordinate" appended, a text without an @HD line gets
    "@HD\\tVN:1.5\\tSO:coordinate\\n" in front.  l_text follows; every other
    byte is kept.  The role of util/GetSortedBAMHeader; htsjdk re-serialises
    the whole header there, and byte equality with that is not claimed."""
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
            fields = [fields[0]] + [b"SO:coordinate" if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            fields.append(b"SO:coordinate")
        text = b"\t".join(fields) + text[end:]
    else:
        text = b"@HD\tVN:1.5\tSO:coordinate\n" + text
    return h[:4] + len(text).to_bytes(4, "little") + text + rest


def sort_bam(src, out, order="coordinate", level=5, splitting_bai=None, granularity=4096, eof=True, device=0,
             stringency=STRICT, window_bytes=0):
    """Write the BAM `src` (a path or the file's bytes) to `out` (a path or a
    binary file object) with its records sorted on the GPU: order "coordinate"
    (the header gets SO:coordinate) or "key" (the shuffle's order, header
    unchanged).  Ties keep the input order.  splitting_bai: a binary file
    object that receives the write-time .splitting-bai.  Returns the number of
    records.  The file must decode as one window of window_bytes compressed
    bytes (0: the library's default)."""
    opened = None
    kw = dict(device=device, stringency=stringency, window_bytes=window_bytes)
    f = BamFile(path=os.fspath(src), **kw) if isinstance(src, (str, os.PathLike)) else BamFile(src, **kw)
    try:
        header = f.header_bytes()
        if order == "coordinate":
            header = sorted_header(header)
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
                                     f"(window_bytes={window_bytes or 'default'}); sort_bam does not merge "
                                     f"sorted runs, open it with a larger window_bytes") from None
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
