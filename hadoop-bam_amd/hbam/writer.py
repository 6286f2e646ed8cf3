"""The BAM write path's host side: BAMRecordWriter (BAMRecordWriter.java:51-168)
over a BGZF stream deflated on the GPU -- the Python mirror of
java/.../GpuBAMRecordWriter.java, same buffering and same voff rule.

The stock writer encodes each record into htsjdk's BlockCompressedOutputStream,
which deflates its buffer every time it fills (HTSJDK_BLOCK_SIZE bytes) and the
partial block at flush; BAMRecordWriter.close flushes and writes no EOF
terminator (:131-143).  BamWriter appends the same bytes to a buffer of many
such blocks and deflates the full buffer in one hbam_bgzf_compress call.  With
a write-time .splitting-bai (:69-74, 145-149) each record's virtual offset --
its block's address << 16 | its offset in the block, the stock stream's
getFilePointer() before the record -- is known once its block is deflated; the
buffered records' offsets are kept until then and fed to the indexer in order
(SplittingBAMIndexer.processAlignment(long) :197-202: record 0 and every
granularity-th record), finish(file length) at close (:240-243)."""
import struct

import numpy as np

from . import HTSJDK_BLOCK_SIZE, bgzf_compress


# the empty BGZF block a complete BAM ends with (SAM spec 4.1.2)
BGZF_EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class SplittingIndexWriter:
    """The write-time SplittingBAMIndexer (:154-243) in O(1) state."""

    def __init__(self, out, granularity=4096):
        self.out, self.granularity, self.count = out, granularity, 0

    def process_alignment(self, voff):
        if self.count == 0 or (self.count + 1) % self.granularity == 0:
            self.out.write(struct.pack(">Q", voff))
        self.count += 1

    def skip(self, k):
        """k records that get no entry: processAlignment k times, nothing written."""
        self.count += k

    def finish(self, input_size):
        self.out.write(struct.pack(">Q", input_size << 16))


class BamWriter:
    """out: a binary file object.  header: the BAM header bytes (magic, text,
    references), written into the same stream as writeHeader does (:152-167);
    None writes none (writeHeader false).  buffer_blocks: stock-stream blocks
    deflated per GPU call (hadoopbam.gpu.write-buffer-bytes / block)."""

    def __init__(self, out, header=None, level=5, buffer_blocks=1024, splitting_bai=None, granularity=4096,
                 block=HTSJDK_BLOCK_SIZE, device=0):
        if buffer_blocks < 1 or not 0 < block <= 65536:
            raise ValueError("buffer_blocks >= 1 and 0 < block <= 65536")
        self.out, self.level, self.block, self.device = out, level, block, device
        self.buf = bytearray(buffer_blocks * block)
        self.pos = 0                # bytes in the buffer
        self.block_address = 0      # compressed bytes written so far
        # the buffered records in order (indexer only): u >= 0 = a record at
        # buffer offset u; u < 0 = -u records the index only counts (write_records)
        self.pending = []
        self.index = SplittingIndexWriter(splitting_bai, granularity) if splitting_bai is not None else None
        if header:
            self._put(header)

    def write_record(self, rec):
        """writeAlignment (:145-150) of one encoded record (block_size included)."""
        if self.index is not None:
            self.pending.append(self.pos)
        self._put(rec)

    def write_records(self, enc, offs):
        """write_record of the n records enc[offs[i]:offs[i+1]] in one go: the
        same buffering, block cuts and index entries as n single calls, with a
        copy per buffer fill and an index step per entry instead of per record."""
        offs = np.asarray(offs, np.uint64).astype(np.int64)
        enc = memoryview(enc)
        n, end = len(offs) - 1, int(offs[-1]) if len(offs) else 0
        cur, i = int(offs[0]) if n > 0 else end, 0
        while cur < end:
            k = min(end - cur, len(self.buf) - self.pos)
            j = int(np.searchsorted(offs[:n], cur + k, side="left"))  # records [i, j) start in this piece
            if self.index is not None and j > i:
                self._pend(offs[i:j] - cur + self.pos)
            self.buf[self.pos:self.pos + k] = enc[cur:cur + k]
            self.pos += k
            cur += k
            i = j
            if self.pos == len(self.buf):
                self._deflate(self.pos)

    def _pend(self, at):
        """Buffer offsets `at` of the next records: the ones the index writes an
        entry for (ordinal 0 and every granularity-th), the others as counts."""
        g = self.index.granularity
        first = self.index.count + sum(1 if u >= 0 else -u for u in self.pending)  # the first one's ordinal
        o = first + np.arange(len(at), dtype=np.int64)
        last = -1
        for h in np.nonzero((o == 0) | ((o + 1) % g == 0))[0]:
            h = int(h)
            if h - last > 1:
                self.pending.append(-(h - last - 1))
            self.pending.append(int(at[h]))
            last = h
        if len(at) - last > 1:
            self.pending.append(-(len(at) - last - 1))

    def close(self, eof=False):
        """close (:131-143): the partial block deflated, no EOF; the index finished.
        eof: the 28-byte BGZF terminator follows (the stock writer leaves that to
        the merge step), counted in the file length the index ends with."""
        self._deflate(self.pos)
        if eof:
            self.out.write(BGZF_EOF_BLOCK)
            self.block_address += len(BGZF_EOF_BLOCK)
        if self.index is not None:
            self.index.finish(self.block_address)

    def _put(self, b):
        b = memoryview(bytes(b))
        while len(b):
            k = min(len(b), len(self.buf) - self.pos)
            self.buf[self.pos:self.pos + k] = b[:k]
            self.pos += k
            b = b[k:]
            if self.pos == len(self.buf):  # full: deflated now, as the stock stream deflates a full block
                self._deflate(self.pos)

    def _deflate(self, n):
        if n == 0:
            return
        lens = [min(self.block, n - p) for p in range(0, n, self.block)]
        z = bgzf_compress(bytes(self.buf[:n]), block_lens=lens, level=self.level, eof=False, device=self.device)
        starts, p = [], 0
        for _ in lens:  # each block's address: BSIZE (header bytes 16-17) + 1 is its length
            starts.append(self.block_address + p)
            p += int.from_bytes(z[p + 16:p + 18], "little") + 1
        self.out.write(z)
        for u in self.pending:
            if u < 0:
                self.index.skip(-u)
            else:
                self.index.process_alignment(starts[u // self.block] << 16 | u % self.block)
        self.pending = []
        self.block_address += len(z)
        self.pos = 0
