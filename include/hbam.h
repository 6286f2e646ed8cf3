/*
 * hbam.h -- C ABI of the MI355X-native Hadoop-BAM read path (libhbam.so).
 *
 * This is the boundary a JNI shim behind org.seqdoop.hadoop_bam binds (see
 * INTEGRATION.md and java/).  Plain C: pointers, sizes and status codes only.
 * Every entry point names the reference interface it replaces (paths relative
 * to /root/reference/src/main/java/org/seqdoop/hadoop_bam/).
 *
 * Status codes map 1:1 onto the Java exception a caller must raise:
 *   HBAM_E_FORMAT -> htsjdk.samtools.SAMFormatException
 *   HBAM_E_TRUNC  -> htsjdk.samtools.FileTruncatedException / RuntimeEOFException
 *   HBAM_E_ARG    -> java.lang.IllegalArgumentException
 *   HBAM_E_IO     -> java.io.IOException (RuntimeIOException for bad DEFLATE data)
 *   HBAM_E_DEVICE -> java.io.IOException (HIP runtime failure; never a silent CPU path)
 * The message is available from hbam_last_error(ctx).
 *
 * I/O: a ctx reads the file the way BAMRecordReader reads its split through
 * WrapSeekable (WrapSeekable.java:42-87): opening parses the header only, and
 * a decode copies into HBM just the window of compressed bytes it works on
 * (opts.window_bytes at a time, the next record's position carried from one
 * window to the next).  Device memory is bounded by the window, whatever the
 * file size.  hbam_open maps the path read-only and checks the file's
 * length before each read of it; hbam_open_reader reads through a caller's
 * positioned-read callback (a Hadoop FileSystem stream).  A file that turns
 * out shorter than its length at open (truncated while a ctx is open) fails
 * the call that reads there with HBAM_E_TRUNC, and a read error with
 * HBAM_E_IO, as the reference's stream reads throw (only a truncation that
 * races a copy of a mapped path can still raise SIGBUS).
 *
 * Threading: a ctx is single-threaded (RecordReader contract); the library is
 * re-entrant across ctxs.  Each ctx owns one HIP stream on its device.
 * Ownership: memory returned inside hbam_batch / hbam_header_info belongs to
 * the ctx and stays valid until the next call on that ctx or hbam_close.
 * Buffers returned through uint8_t** are released with hbam_free.
 */
#ifndef HBAM_H
#define HBAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBAM_OK 0
#define HBAM_E_FORMAT 1
#define HBAM_E_TRUNC 2
#define HBAM_E_ARG 3
#define HBAM_E_IO 4
#define HBAM_E_DEVICE 5
#define HBAM_E_STATE 6
#define HBAM_E_NOMEM 7

#define HBAM_ABI_VERSION 6

/* htsjdk ValidationStringency, as util/SAMHeaderReader.java:45-46 reads it */
#define HBAM_STRICT 0  /* htsjdk's default: SAMRecord.isValid errors -> SAMFormatException */
#define HBAM_LENIENT 1 /* errors are logged; records still decoded for the check */
#define HBAM_SILENT 2  /* no validation */

typedef struct hbam_ctx hbam_ctx;

/* Reader options: the hadoopbam.* Configuration properties a JNI shim reads. */
typedef struct hbam_opts {
  int32_t device;        /* hadoopbam.gpu.device: HIP device ordinal (default 0) */
  int32_t check_crc;     /* BlockCompressedInputStream.setCheckCrcs (default 0) */
  int32_t stringency;    /* hadoopbam.samheaderreader.validation-stringency (HBAM_STRICT when unset) */
  int32_t parallel_reads; /* hbam_open_reader: nonzero = the read callback may run on several library
                             threads at once (PositionedReadable positioned reads are thread-safe) */
  uint64_t window_bytes; /* hadoopbam.gpu.window-bytes: compressed bytes per HBM window (0 = 4 GiB) */
  uint64_t batch_records; /* hadoopbam.gpu.batch-records: the max_records the caller will pass to
                             hbam_decode_span (0 = not known); its page-locked batch slots are then
                             allocated on a helper thread from the open on */
} hbam_opts;

/* BAM header summary ([htsjdk] BAMFileReader.readHeader). */
typedef struct hbam_header_info {
  int32_t n_ref;                /* binary reference count (SAMSequenceDictionary size) */
  int32_t l_text;               /* SAM header text length */
  uint64_t first_record_voff;   /* getFilePointerSpanningReads().getFirstOffset() */
  uint64_t file_size;           /* compressed bytes */
  const char *text;             /* l_text bytes, owned by ctx */
} hbam_header_info;

/* A batch of decoded records in SoA form: exactly the argument list of
 * LazyBAMRecordFactory.createBAMRecord (LazyBAMRecordFactory.java:37-50)
 * plus the BAMRecordReader key (BAMRecordReader.java:81-121) and the BGZF
 * virtual offset of each record.  pos / next_pos are the 0-based BAM fields
 * (htsjdk alignmentStart = pos + 1).  The rest of record i (read name, cigar,
 * seq, qual, aux = getVariableBinaryRepresentation()) is
 * data[rest_off[i] .. rest_off[i] + rest_len[i]). */
typedef struct hbam_batch {
  uint64_t n;
  const int32_t *ref_id, *pos, *l_seq, *next_ref_id, *next_pos, *tlen;
  const uint8_t *l_read_name, *mapq;
  const uint16_t *bin, *n_cigar, *flag;
  const int64_t *key;
  const uint64_t *voff, *rest_off;
  const uint32_t *rest_len;
  const uint8_t *data;
  uint64_t data_len;
  int32_t status;      /* status of the record that ended the span early (0 = clean end) */
  int32_t reserved;
  uint64_t next_voff;  /* where the split continues: pass it as vstart of the next call; >= vend when done */
} hbam_batch;

/* Open a BAM file (read-only map; nothing but the header is read) / an
 * in-memory BAM / a plain BGZF file (VCF/BCF payloads: no BAM header).
 * Replaces BAMRecordReader.initialize's SamReader construction
 * (BAMRecordReader.java:142-149,186-200) and SAMHeaderReader.readSAMHeaderFrom
 * (util/SAMHeaderReader.java:57-75). */
int hbam_open(const char *path, const hbam_opts *opts, hbam_ctx **out);
int hbam_open_mem(const void *data, uint64_t len, const hbam_opts *opts, hbam_ctx **out);
int hbam_open_bgzf(const void *data, uint64_t len, const hbam_opts *opts, hbam_ctx **out);
/* Positioned read of a file of a known length: copy file bytes
 * [offset, offset + len) into dst and return the bytes copied (fewer only at
 * the end of the file, 0 there) or a negative value on an I/O error.  This is
 * PositionedReadable.read(position, buffer, offset, length) of the
 * FSDataInputStream that WrapSeekable.openPath wraps (util/WrapSeekable.java:
 * 56-87; BAMRecordReader.java:147, BAMInputFormat.java:476).  dst is
 * page-locked host memory the library owns.  The library calls read from its
 * own threads, one call at a time for one ctx (unless opts->parallel_reads): a JNI binding attaches
 * the calling thread to the JVM.  user is passed through.  With
 * opts->parallel_reads set, the library's copy threads call read at once for
 * disjoint ranges (HDFS DFSInputStream positioned reads are thread-safe). */
typedef int64_t (*hbam_read_fn)(void *user, uint64_t offset, void *dst, uint64_t len);
/* hbam_open for a file read through `read` (HDFS or any Hadoop FileSystem):
 * size = FileStatus.getLen().  user must stay valid until hbam_close. */
int hbam_open_reader(uint64_t size, hbam_read_fn read, void *user, const hbam_opts *opts, hbam_ctx **out);
void hbam_close(hbam_ctx *ctx);
const char *hbam_last_error(hbam_ctx *ctx);
void hbam_free(void *p);
int32_t hbam_abi_version(void);
/* Device (HBM) and page-locked host blocks freed by closed contexts stay in
 * a process-wide cache for the next split of the process (an executor or a
 * reused task JVM reads many); this returns them to the HIP runtime.  Call
 * it with no context open (HbamNative.releaseCachedMemory; no reference
 * counterpart).  Returns the bytes released. */
uint64_t hbam_release_cached_memory(void);

int hbam_header(hbam_ctx *ctx, hbam_header_info *out);
/* reference i of the binary dictionary: name (NUL-terminated, ctx-owned) and length */
int hbam_ref(hbam_ctx *ctx, int32_t i, const char **name, int32_t *length);
/* BGZF block count and inflated size of the whole file (reads every block header) */
int hbam_file_stats(hbam_ctx *ctx, uint64_t *n_blocks, uint64_t *uncompressed_size);
/* host -> HBM bytes this ctx has copied so far (its window loads + prefetch) */
int hbam_bytes_read(hbam_ctx *ctx, uint64_t *bytes);
/* Copy file bytes [lo, hi) into HBM now; later windows inside the range decode
 * from HBM without host reads. */
int hbam_prefetch(hbam_ctx *ctx, uint64_t lo, uint64_t hi);

/* Decode records of FileVirtualSplit [vstart, vend) (vStart inclusive, vEnd
 * exclusive: FileVirtualSplit.java:82-86) exactly as BAMRecordReader.initialize
 * + the nextKeyValue loop would (BAMRecordReader.java:151-154,181-182,223-232),
 * with the ctx's validation stringency.  At most max_records records are
 * returned (0 = every record of the split); out->next_voff is where the next
 * call continues, so a split streams in bounded batches:
 *   for (v = vStart; hbam_decode_span(ctx, v, vEnd, max, &b) == HBAM_OK && b.n; v = b.next_voff) ...
 * A call whose vstart is the previous batch's next_voff continues without
 * re-decoding.  Records before a failing record are returned with out->status
 * set and the call returns that status. */
int hbam_decode_span(hbam_ctx *ctx, uint64_t vstart, uint64_t vend, uint64_t max_records, hbam_batch *out);
/* BAMRecordReader.getProgress's in.position() (BAMRecordReader.java:209-219):
 * the compressed stream position after nextKeyValue returned record i of the
 * last batch (htsjdk's iterator has read one record ahead).  i == UINT64_MAX:
 * the position once the iterator exists and before record 0 of the batch is
 * handed out (the iterator has read record 0 only). */
int hbam_reader_position(hbam_ctx *ctx, uint64_t i, uint64_t *pos);

/* ---- bounded traversal (hadoopbam.bam.intervals / hadoopbam.bam.bounded-traversal) ---- */
/* [htsjdk] QueryInterval: 1-based inclusive; end <= 0 = to the end of the reference. */
typedef struct hbam_interval { int32_t ref_id, start, end; } hbam_interval;
/* BAMRecordReader.initialize's interval branch (BAMRecordReader.java:171-175):
 * bamFileReader.createIndexIterator(queryIntervals, false, filePointers).
 * iv = the intervals BAMInputFormat.prepareQueryIntervals returns, optimized
 * (sorted by ref_id, and within one ref_id each start past the previous
 * interval's end; an end may not lie more than one base before its start):
 * [htsjdk] assertIntervalsOptimized -> HBAM_E_ARG otherwise.  file_pointers =
 * FileVirtualSplit.getIntervalFilePointers(): n_ptrs / 2 chunks of virtual
 * offsets [file_pointers[2k], file_pointers[2k+1]), in ascending order (an odd
 * n_ptrs or a chunk out of order -> HBAM_E_ARG).  The chunks are read in turn,
 * each yielding the records hbam_decode_span(start, end) would, and
 * [htsjdk] BAMQueryFilteringIterator's filter runs over them on the GPU: one
 * interval index for the whole query, a record kept when the first interval
 * that does not lie before it overlaps it, and the iteration over -- nothing
 * further read -- at the first record that lies past every interval.  Records
 * read are validated under the ctx's stringency whether kept or not.
 * Opens the query: hbam_query_next returns its records.  The query ends,
 * and hbam_query_next returns HBAM_E_STATE until another is opened, with any
 * other call on the ctx that reads the file, since each of them moves the
 * ctx's window: hbam_decode_span*, hbam_decode_writables, hbam_prefetch,
 * hbam_file_stats, hbam_blocks, hbam_read_inflated,
 * hbam_build_splitting_index, hbam_splitting_entries, hbam_build_bai,
 * hbam_get_splits*, hbam_guess_*.  hbam_header, hbam_ref, hbam_bytes_read,
 * hbam_pipeline_counters and hbam_last_error leave it open. */
int hbam_query_intervals(hbam_ctx *ctx, const hbam_interval *iv, uint64_t n_iv, const uint64_t *file_pointers,
                         uint64_t n_ptrs);
/* The unmapped-only branch (BAMRecordReader.java:176-178):
 * bamFileReader.queryUnmapped().  Reads from start_voff
 * (getIndex().getStartOfLastLinearBin(), or the first record's offset when
 * that is -1) to the end of the file, skips (and validates) records up to the
 * first one with refID == -1, and yields every record from it on. */
int hbam_query_unmapped(hbam_ctx *ctx, uint64_t start_voff);
/* The next records of the open query, at most max_records (0 = all that
 * remain), as hbam_decode_span hands them out (out->data holds the rests back
 * to back); out->n == 0: the end.  out->next_voff is 0.  A batch with
 * max_records > 0 holds records of one window, so it may be shorter than
 * asked, and its rests stay below 2 GiB (one record at least), the size a JNI
 * caller can wrap as a direct ByteBuffer; max_records = 0 has no such bound
 * (as in hbam_decode_span), so a JNI caller passes a batch size.  Records before a
 * failing record are returned with out->status set and the call returns that
 * status; a failing record past the one that ended the iteration is never
 * read.  No query open -> HBAM_E_STATE.  After a query batch
 * hbam_encode_writables and hbam_reader_position return HBAM_E_STATE. */
int hbam_query_next(hbam_ctx *ctx, uint64_t max_records, hbam_batch *out);

/* SplittingBAMIndexer.index(in, out, inputSize, granularity)
 * (SplittingBAMIndexer.java:248-290): the .splitting-bai bytes, big-endian u64
 * entries, byte-identical to the reference; the file is streamed through HBM
 * window by window.  *buf released with hbam_free. */
int hbam_build_splitting_index(hbam_ctx *ctx, int32_t granularity, uint8_t **buf, uint64_t *len);
/* Write-time index: new SplittingBAMIndexer(out, granularity), processAlignment
 * for records with virtual offsets voffs[0..n) in file order, then
 * finish(file_size) (SplittingBAMIndexer.java:175-243, driven by
 * BAMRecordWriter.java:145-149).  Entries selected on the GPU. */
int hbam_splitting_index_for_records(const hbam_opts *opts, const uint64_t *voffs, uint64_t n, int32_t granularity,
                                     uint64_t file_size, uint8_t **buf, uint64_t *len);

/* BAMSplitGuesser.guessNextBAMRecordStart(beg, end) (BAMSplitGuesser.java:108-235)
 * for n split points at once (one GPU launch per window of nearby points);
 * out[i] == ends[i] when no record start is found, as in the reference. */
int hbam_guess_record_starts(hbam_ctx *ctx, const uint64_t *begs, const uint64_t *ends, uint64_t n,
                             uint64_t *out);
/* The same with the header read from another stream than the data
 * (BAMSplitGuesser(SeekableStream, InputStream headerStream, Configuration),
 * BAMSplitGuesser.java:93-103): header_n_ref = that header's sequence
 * dictionary size, which bounds the refIDs a guessed record may hold
 * (record.setHeaderStrict(header), :185); < 0 = the data file's header. */
int hbam_guess_record_starts_hdr(hbam_ctx *ctx, int32_t header_n_ref, const uint64_t *begs, const uint64_t *ends,
                                 uint64_t n, uint64_t *out);

/* util/BGZFSplitGuesser.guessNextBGZFBlockStart(beg, end)
 * (util/BGZFSplitGuesser.java:64-112) for n split points at once: the first
 * BGZF block start in [beg, beg + min(end-beg, 0xffff)) whose block lies in
 * the guesser's 2*0xffff-1 byte window and inflates with a good CRC;
 * out[i] == ends[i] when none.  The split search of the BGZF text formats
 * (VCFInputFormat / BCFSplitGuesser); works on a ctx from hbam_open_bgzf. */
int hbam_guess_bgzf_block_starts(hbam_ctx *ctx, const uint64_t *begs, const uint64_t *ends, uint64_t n,
                                 uint64_t *out);

/* BAMInputFormat.getSplits for the FileSplits of one file
 * (BAMInputFormat.java:222-318 addIndexedSplits, 469-530 addProbabilisticSplits).
 * sbi = .splitting-bai bytes or NULL.  vstarts/vends need room for n entries. */
int hbam_get_splits(hbam_ctx *ctx, const uint64_t *starts, const uint64_t *lengths, uint64_t n,
                    const uint8_t *sbi, uint64_t sbi_len, uint64_t *vstarts, uint64_t *vends,
                    uint64_t *nout);
/* The same with the BAI split calculator enabled (hadoopbam.bam.enable-bai-splitter,
 * BAMInputFormat.java:241-257, 322-465): with no usable .splitting-bai, splits
 * come from the linear index of the file's .bai (bai bytes; NULL: no .bai ->
 * probabilistic splits), a split no linear entry starts in getting a guessed
 * start.  At most n splits.  Errors as the reference's: a guesser I/O error
 * inside the BAI planner falls back to probabilistic splits (the IOException
 * getSplits catches, :249-253); a malformed .bai -> HBAM_E_FORMAT (htsjdk's
 * unchecked parse error); where addBAISplits dereferences null (no contig
 * with a linear index, a guessed first split) -> HBAM_E_STATE (the JNI glue
 * throws NullPointerException). */
int hbam_get_splits_bai(hbam_ctx *ctx, const uint64_t *starts, const uint64_t *lengths, uint64_t n,
                        const uint8_t *sbi, uint64_t sbi_len, const uint8_t *bai, uint64_t bai_len,
                        uint64_t *vstarts, uint64_t *vends, uint64_t *nout);

/* ---- the BAM index (.bai, SAM spec 5.2): built on the GPU, read on the host ---- */
/* The .bai of a coordinate-sorted BAM, computed on the GPU: the file is
 * streamed through HBM window by window from the first record to the end of
 * the file (as hbam_build_splitting_index does), its records validated under
 * the ctx's stringency, and per record the kernels compute
 *   - whether it is indexed: refID >= 0 and pos >= 0 (the others only count
 *     towards n_no_coor);
 *   - its end: pos + 1 for a placed unmapped read (flag 0x4), else pos +
 *     max(reference length of the CIGAR, 1) (M, D, N, = and X consume the
 *     reference; the sum wraps as a Java int and the CIGAR is clipped to the
 *     record, as in the bounded-traversal filter);
 *   - its bin reg2bin(pos, end) -- computed, not the record's stored bin;
 *   - the 16 kbp windows it touches: pos >> 14 .. (end - 1) >> 14, for a
 *     placed unmapped read the single window max(pos - 1, 0) >> 14.
 * Chunks: a record extends the last chunk of its (refID, bin) when the record
 * before it in the file was indexed into the same (refID, bin), else it starts
 * a chunk at its virtual offset; a chunk ends at the virtual offset of the
 * record after its last record (file_size << 16 after the file's last
 * record).  A bin's chunks are in file order, a contig's bins in ascending
 * order.  Linear index: entry w = the smallest virtual offset among the
 * records touching window w; an untouched window takes the last touched entry
 * before it (0 if none); n_intv = the highest touched window + 1; a contig
 * with no indexed record has n_bin = n_intv = 0.
 * flags: HBAM_BAI_METADATA adds, per contig with an indexed record, a last
 * bin 37450 with two chunks -- (offset of the contig's first indexed record,
 * chunk end of its last one) and (indexed records without 0x4, with 0x4) --
 * and, after the last contig, the u64 count of unindexed records.
 * The index follows the SAM specification and this repository's oracle; it is
 * a valid index for htsjdk and htslib readers, but byte equality with the file
 * htsjdk's BAMIndexer writes (its chunk coalescing) is not claimed.
 * HBAM_E_FORMAT: indexed records not in non-decreasing (refID, pos) order
 * (the file is not coordinate-sorted); a record ending past 2^29; a record
 * touching a window past (min(l_ref, 2^29) >> 14) + 1 windows of its contig
 * (the tables are sized from the header); a refID past the header's contigs.
 * HBAM_E_STATE on a ctx from hbam_open_bgzf or hbam_open_codec.  Ends an open
 * query.  *buf released with hbam_free. */
#define HBAM_BAI_METADATA 1   /* per-contig pseudo-bin 37450 + trailing n_no_coor (SAM spec 5.2) */
int hbam_build_bai(hbam_ctx *ctx, int32_t flags, uint8_t **buf, uint64_t *len);

/* Reading a .bai (host code: no device, no ctx; errors: hbam_last_error(NULL)). */
typedef struct hbam_bai_summary {
  int32_t n_ref, has_no_coor;
  int64_t start_of_last_linear_bin;   /* [htsjdk] getStartOfLastLinearBin: last entry of the last contig with a linear index; -1 if none */
  uint64_t no_coor_count;             /* trailing n_no_coor; 0 when absent */
} hbam_bai_summary;
/* A malformed index -> HBAM_E_FORMAT. */
int hbam_bai_summarize(const void *bai, uint64_t len, hbam_bai_summary *out);
/* The chunk side of BAMInputFormat.filterByInterval (BAMInputFormat.java:571-574):
 * the file pointers hbam_query_intervals takes.  Per interval (1-based
 * inclusive, end <= 0 = to the end of the reference): beg0 = max(start - 1, 0),
 * end0 = end <= 0 ? 2^29 : end; every chunk of the bins reg2bins(beg0, end0)
 * (never the pseudo-bin 37450) whose end lies above the linear entry of window
 * beg0 >> 14 (past the table: its last entry; no linear index: 0); sorted, two
 * chunks merged when start <= the previous end.  The result is the union over
 * the intervals, sorted and merged again: n_ptrs / 2 pairs (start, end),
 * ascending; *file_pointers released with hbam_free.  Intervals not optimized
 * (the rule of hbam_query_intervals) or a ref_id outside [0, n_ref) ->
 * HBAM_E_ARG; a malformed index -> HBAM_E_FORMAT. */
int hbam_bai_query(const void *bai, uint64_t len, const hbam_interval *iv, uint64_t n_iv,
                   uint64_t **file_pointers, uint64_t *n_ptrs);

/* ---- SAMRecordWritable codec (map-output serialization for the shuffle) ---- */
/* SAMRecordWritable.write (SAMRecordWritable.java:55-64) of every record of
 * the last hbam_decode_span batch on ctx, computed on the GPU: [htsjdk]
 * BAMRecordCodec.encode of each BAMRecord, back to back (block_size, the fixed
 * fields, the undecoded rest; indexBin written as 0 when refID < 0).  *len
 * receives the total size; out == NULL only sizes.  offs (NULL or n+1
 * entries) receives each record's start, offs[n] = *len.  cap < *len ->
 * HBAM_E_ARG.  A batch from several windows (max_records = 0 over a split
 * longer than a window) -> HBAM_E_STATE: encode bounded batches. */
int hbam_encode_writables(hbam_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *offs, uint64_t *len);
/* hbam_encode_writables of the last hbam_decode_span batch with the records in
 * sorted order, sorted and gathered on the GPU (the map-side sort of the
 * reference's sort job: the shuffle orders records by BAMRecordReader.getKey).
 * Each record's bytes are exactly what hbam_encode_writables writes for it;
 * only the order differs.  perm (NULL or n entries) receives the batch index
 * of the j-th output record, offs (NULL or n+1 entries) the output starts,
 * offs[n] = *len.  out == NULL only sizes: *len is set, nothing is launched,
 * offs and perm are left untouched.
 *   HBAM_SORT_KEY         ascending hbam_batch.key compared as a signed 64-bit
 *       value (LongWritable.compareTo).  An unmapped read's key is
 *       Integer.MAX_VALUE << 32 | hash with the int hash sign-extended, so about
 *       half of the unmapped reads have negative keys and sort first, as in the
 *       reference.
 *   HBAM_SORT_COORDINATE  ascending (uint64)(uint32)refID << 32 | (uint32)(pos + 1):
 *       contigs in dictionary order, refID -1 last, pos -1 first within its
 *       contig, a placed unmapped read at its position.
 *   HBAM_SORT_QUERYNAME   by read name (SO:queryname; samtools sort -n's and
 *       Picard SortSam SORT_ORDER=queryname's family).  Record a comes before
 *       record b when the first of these keys that differs says so:
 *       1. the name: the min(l_read_name, rest length) bytes at byte 36 of the
 *          record's encoding, zero-extended without end and compared as unsigned
 *          bytes, lexicographically (a name that is a prefix of another comes
 *          first; bytes >= 0x80 sort after ASCII).  For well-formed names
 *          (printable ASCII, one terminating NUL) this is String.compareTo on
 *          the read names.  l_read_name 0 (possible under SILENT) is the empty
 *          name.  No byte outside the record and the source's padding is read.
 *       2. the tie word t = 2 * m + s from the flag: m = 3 when 0x1 is clear;
 *          else 0 when exactly 0x40 of {0x40, 0x80} is set, 2 when exactly 0x80
 *          is set, 1 when both or neither; s = 1 when 0x100 or 0x800 is set,
 *          else 0.  First of pair before second of pair, paired before unpaired,
 *          primary before secondary or supplementary.
 *       3. the batch order (stable).
 *       The tie word is modelled on the leading rules of htsjdk's
 *       SAMRecordQueryNameComparator; equality with that comparator (which goes
 *       on to strand, the HI tag, ...) or with samtools' natural name order is
 *       NOT claimed: htsjdk was not available to compare against.  The order is
 *       a valid SO:queryname order under the SAM specification (which leaves the
 *       collation to the implementation).  There is no 64-bit sort word for
 *       this order; the value 2 is not an order and is refused.
 * All orders are stable: records with equal sort words keep their batch order.
 * For key and coordinate, that tie order is neither htsjdk's SAMRecordCoordinateComparator (which goes
 * on to strand, read name, flags, ...) nor samtools' strand tie-break; it is a
 * valid SO:coordinate order under the SAM specification, and the order
 * hbam_build_bai accepts.
 * Errors: no file ctx, a last batch from hbam_query_next or
 * hbam_decode_writables, or a batch from several windows (one call sorts one
 * window's records: open with a window_bytes that holds the split, or sort
 * bounded batches) -> HBAM_E_STATE; an unknown order, cap < *len with out set,
 * or n >= 2^31 - 1 -> HBAM_E_ARG.  n == 0 -> HBAM_OK with *len = 0. */
#define HBAM_SORT_KEY        0
#define HBAM_SORT_COORDINATE 1
#define HBAM_SORT_QUERYNAME  3
int hbam_sort_writables(hbam_ctx *ctx, int32_t order, uint8_t *out, uint64_t cap, uint64_t *offs, uint32_t *perm,
                        uint64_t *len);
/* ---- SAM text ---- */
/* SAMRecordWriter / [htsjdk] SAMTextWriter.writeAlignment (the text output of
 * AnySAMOutputFormat, KeyIgnoringSAMRecordWriter; `samtools view`) of every
 * record of the last hbam_decode_span batch on ctx, formatted on the GPU: one
 * line per record in batch order, the fields joined by '\t', the line ended by
 * '\n' (SAM specification 1.4 / 1.5).  No header text is written.
 *    1 QNAME  the l_read_name - 1 bytes at byte 36 of the record's encoding,
 *             verbatim; l_read_name <= 1 -> "*"
 *    2 FLAG   flag, unsigned decimal
 *    3 RNAME  ref_id == -1 -> "*", else the name of reference ref_id of the
 *             ctx's binary dictionary (hbam_ref), verbatim
 *    4 POS    pos + 1 (as a 32-bit sum), signed decimal
 *    5 MAPQ   mapq, decimal
 *    6 CIGAR  n_cigar == 0 -> "*", else for each u32 v: v >> 4 in decimal, then
 *             "MIDNSHP=X"[v & 15]; an op above 8 prints "?".  The CG:B:I
 *             long-CIGAR convention is not applied: the CIGAR prints as stored.
 *    7 RNEXT  next_ref_id == -1 -> "*"; == ref_id -> "="; else the reference name
 *    8 PNEXT  next_pos + 1, as POS
 *    9 TLEN   tlen, signed decimal
 *   10 SEQ    l_seq == 0 -> "*", else "=ACMGRSVTWYHKDBN"[nibble], high nibble first
 *   11 QUAL   l_seq == 0 or the first quality byte 0xFF -> "*", else each byte
 *             (q + 33) & 0xFF
 *   12+ aux   in stored order, each as "\tTG:t:value" (a tab before every tag,
 *             none behind the last):
 *             A            "A:" and the byte
 *             c C s S i I  "i:" and the decimal value (C, S, I unsigned)
 *             f            "f:" and the float (below)
 *             Z, H         "Z:" / "H:" and the bytes up to the NUL
 *             B            "B:", the subtype letter (c C s S i I f), then ",value"
 *                          for each element; a count of 0 prints only "B:c"
 * Floats: a 32-bit float prints as C's printf("%g") of its value in the "C"
 * locale: 6 significant digits correctly rounded from the exact binary value
 * (ties to even), trailing zeros dropped, exponent form below 1e-4 and from
 * 1e6 on; NaN is "nan", the infinities "inf" and "-inf", negative zero "-0".
 * This is samtools' text.  htsjdk prints Java's Float.toString: equality with
 * SAMTextWriter is NOT claimed for float tags (htsjdk was not available to
 * compare against); every other field follows the SAM specification, which
 * both writers implement.
 * *len receives the text's size; out == NULL only sizes (the measuring pass
 * still runs on the GPU, and offs is filled).  offs (NULL or n + 1 entries)
 * receives each line's start, offs[n] = *len.  cap < *len with out set ->
 * HBAM_E_ARG.  n == 0 -> HBAM_OK with *len = 0.
 * HBAM_E_FORMAT, with the batch index of the first such record in
 * hbam_last_error and the content of out unspecified: a record whose aux
 * fields are malformed -- an unknown type byte ('d' included), a Z or H with no
 * NUL before the record's end, a B with an unknown subtype, a B whose elements
 * run past the end, a tag header cut by the end -- or, possible under
 * HBAM_SILENT only, whose read name, CIGAR, bases and qualities do not fit its
 * rest (or l_seq < 0).  No kernel reads past a record's rest: every step of the
 * aux walk is bounded by the record's end, in the measuring pass too.
 * A ref_id or next_ref_id outside [-1, n_ref) cannot reach this call:
 * hbam_decode_span ends the batch before such a record with HBAM_E_ARG under
 * every stringency, HBAM_SILENT included (the kernels print "*" for one, and
 * never index the name table with it).
 * HBAM_E_STATE: no file ctx, a batch from several windows (format bounded
 * batches), or a last batch from hbam_query_next or hbam_decode_writables.
 * n >= 2^31 - 1 -> HBAM_E_ARG.  A failed device allocation -> HBAM_E_NOMEM. */
int hbam_format_sam(hbam_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *offs, uint64_t *len);
/* ---- SAM text in ---- */
/* The other direction: SAMRecordReader / [htsjdk] SAMLineParser (the text input
 * of AnySAMInputFormat, SAMInputFormat; `samtools view -b`) of the alignment
 * lines in text[0, len), parsed on the GPU.  Record i is line i as [htsjdk]
 * BAMRecordCodec.encode writes it -- block_size, the 32 fixed bytes, the rest:
 * the encoding hbam_encode_writables writes and hbam_decode_writables,
 * hbam_merge_add_run and a BAM writer take.
 * Lines: a line ends at '\n'; one '\r' directly before it is dropped.  With
 * final == 0 the bytes behind the last '\n' are not parsed and *consumed stops
 * before them (the caller carries them into its next chunk); with final != 0 a
 * last line without a newline is parsed too.  Every line is a record line, one
 * that starts with '@' too (read names may): as htsjdk stops reading header
 * lines at the first line that is not one, the caller strips only the leading
 * run of '@' lines.
 * Parsing is always strict; there is no stringency.  Every violation below is
 * HBAM_E_FORMAT, hbam_last_error names the lowest bad "line K " (0-based within
 * the call) and its field, and out->n is 0.
 *   fields   at least 11, separated by '\t'; none empty, an aux field from a
 *            doubled or trailing tab included; an empty line is an error
 *   decimals an optional '-', then one or more digits; leading zeros allowed,
 *            '+' not; overflow detected for any number of digits
 *    1 QNAME  1 to 254 bytes, stored with a NUL; "*" is stored as "*\0"
 *             (l_read_name 2), as the specification and both writers do
 *    2 FLAG   0..65535
 *    3 RNAME  "*" -> -1, else a name of the dictionary (below); unknown -> error
 *    4 POS    a decimal in [-2^31, 2^31 - 1], stored minus 1 as a wrapping 32-bit
 *             value: everything hbam_format_sam prints is accepted
 *    5 MAPQ   0..255
 *    6 CIGAR  "*", or number-then-operator pairs: the number present and below
 *             2^28, the operator of "MIDNSHP=X"; more than 65,535 operators ->
 *             error (the CG:B:I convention is not applied, as in the formatter)
 *    7 RNEXT  "*" -> -1, "=" -> ref_id (-1 when RNAME is "*"), else a name
 *    8 PNEXT  as POS
 *    9 TLEN   a decimal int32
 *   10 SEQ    "*" -> l_seq 0 (QUAL must then be "*"), else the letters of
 *             "=ACMGRSVTWYHKDBN" in either case, '.' -> 15, the high nibble
 *             first, the last low nibble 0 when l_seq is odd; any other byte is
 *             an error (htsjdk's rule, not samtools' silent 'N')
 *   11 QUAL   "*" -> l_seq bytes 0xFF, else exactly l_seq bytes in [33, 126],
 *             stored minus 33
 *   bin      0 when ref_id < 0, else reg2bin(pos, end) with arithmetic shifts
 *            (pos = -1 gives 4680), end = pos + the CIGAR's reference length
 *            (M D N = X), pos + 1 when flag 0x4 is set or that length is 0
 *   12+ aux  "TG:t:value", at least 5 bytes; only Z and H may have an empty value
 *            A   exactly one byte
 *            i   a decimal in [-2^31, 2^32 - 1], stored in the first type that
 *                holds it of c [-128, 127], C <= 255, s [-32768, 32767],
 *                S <= 65535, i, I: htsjdk's BinaryTagCodec rule.  samtools
 *                prefers the unsigned types; equality with samtools is NOT claimed
 *            f   a float (below)
 *            Z H the bytes verbatim plus a NUL (H is not validated, as in the formatter)
 *            B   a subtype letter of "cCsSiIf", then ",value" per element, each
 *                in the subtype's range; "B:c" alone is count 0
 *            any other type letter is an error; duplicate tags are not checked
 * Floats: -?digits[.digits][(e|E)[+-]digits] or -?.digits[(e|E)[+-]digits], and
 * "nan" (0x7FC00000), "inf", "-inf"; hex floats, "infinity" and upper-case
 * specials are errors.  The result is the float32 nearest to the decimal's
 * exact value, ties to even, with no rounding through a double; overflow gives
 * +-inf, underflow denormals or +-0.  Only the first 19 significant digits
 * enter the value, nonzero digits behind them act as a sticky bit: exact for
 * everything %g, %.9g, Float.toString and Double.toString print; a longer text
 * whose first 19 digits end exactly on a float or on the midpoint of two may
 * come out one unit off.
 * Dictionary: a file ctx resolves names against its binary dictionary;
 * hbam_parse_sam_dict replaces it with n_ref names (names == NULL with n_ref ==
 * -1 restores the file's).  A codec ctx (hbam_open_codec) with none set accepts
 * only "*" as RNAME and "*" or "=" as RNEXT.  A name that appears twice resolves
 * to its lowest index.
 * The calls work on a file ctx and on a codec ctx and leave the ctx's last batch
 * untouched (hbam_format_sam still serves it).  out->enc (the records back to
 * back, out->bytes of them) and out->offs (n + 1 starts, offs[n] == bytes) are
 * page-locked host memory the ctx owns: valid until the next hbam_parse_sam on
 * it or its close.  No kernel reads outside [text, text + len) and the zeroed
 * padding the upload provides.
 * n >= 2^31 - 1 lines -> HBAM_E_ARG; a failed device allocation -> HBAM_E_NOMEM. */
typedef struct {
  uint64_t n;          /* records parsed = complete lines consumed */
  uint64_t bytes;      /* size of enc */
  uint64_t consumed;   /* text bytes used: through the last complete line */
  const uint8_t  *enc; /* the records back to back, ctx-owned page-locked host memory */
  const uint64_t *offs;/* n + 1 starts, offs[n] == bytes */
} hbam_sam_records;
int hbam_parse_sam_dict(hbam_ctx *ctx, const char *const *names, int32_t n_ref);
int hbam_parse_sam(hbam_ctx *ctx, const void *text, uint64_t len, int32_t final, hbam_sam_records *out);
/* HIP-event milliseconds of the last hbam_parse_sam on ctx: the line finding,
 * the measure pass, the scan of the record sizes, the write pass (0 where
 * nothing ran).  For measuring. */
int hbam_parse_sam_times(hbam_ctx *ctx, float ms[4]);
/* The BAM header of a SAM header text (host only, no handle): "BAM\1", l_text,
 * the text verbatim, n_ref and one entry per @SQ line in order, its name from
 * SN and its length from LN.  A missing SN, or a missing or non-numeric LN ->
 * HBAM_E_FORMAT (hbam_last_error(NULL)).  *hdr is released with hbam_free. */
int hbam_sam_header_to_bam(const void *text, uint64_t l_text, uint8_t **hdr, uint64_t *len);
/* SAMRecordWritable.readFields (SAMRecordWritable.java:65-68) for n serialized
 * values at once: value i = buf[offs[i], offs[i+1]) (the last ends at len), as
 * the shuffle frames them.  Decodes into out like hbam_decode_span (voff =
 * UINT64_MAX: no file position; key = BAMRecordReader.getKey of the record).
 * Stops at the first bad value: too short for block_size (readFields would
 * get a null record) or a short rest -> HBAM_E_TRUNC; block_size < 32 ->
 * HBAM_E_FORMAT; framing outside buf -> HBAM_E_ARG. */
int hbam_decode_writables(hbam_ctx *ctx, const void *buf, uint64_t len, const uint64_t *offs, uint64_t n,
                          hbam_batch *out);
/* Measurement: what the last HBAM_SORT_QUERYNAME order computed on ctx (an
 * hbam_sort_writables or an hbam_merge_plan) did.  The order is a radix sort
 * over the names' 8-byte chunks; a chunk index in which no two names differ is
 * skipped and the others sort only the bits that differ.  out[0] = the chunks
 * of the longest name, out[1] = the chunks sorted, out[2] = the radix bits
 * those sorts covered (the tie word's 3-bit pass is not counted).  Zeros
 * before the first such order. */
int hbam_sort_name_counters(hbam_ctx *ctx, uint64_t out[3]);
/* A ctx with a device and no file, for reducers that only call
 * hbam_decode_writables. */
int hbam_open_codec(const hbam_opts *opts, hbam_ctx **out);

/* ---- Merge of sorted runs (the reduce side of the sort job) ---- */
/* Hadoop's reduce-side merge of the sorted map outputs (the shuffle's
 * Merger.merge feeding the reducer of the reference's sort job), for k runs of
 * SAMRecordWritable encodings that are each sorted by one hbam_sort_writables
 * order: the output is the order one stable sort of the concatenated runs
 * would give.  Ties go to the earlier run, then to the earlier record of a
 * run.  The order is planned and every part gathered on the GPU; the run bytes
 * stay in the caller's host memory (which may be an mmap of a spill file), only
 * the sort word and the framing of every record live in HBM, so the runs' total
 * size is not bounded by HBM.  Works on a file ctx or a codec ctx; one merge
 * per ctx at a time.  The ctx serves every other call meanwhile.
 *
 * hbam_merge_begin: order = HBAM_SORT_KEY / HBAM_SORT_COORDINATE /
 * HBAM_SORT_QUERYNAME; another value -> HBAM_E_ARG; a merge already open on ctx -> HBAM_E_STATE.
 *
 * hbam_merge_add_run: run = buf[0, len), record i = buf[offs[i], offs[i+1])
 * (offs: n + 1 entries, offs[n] == len).  buf and offs stay the caller's and
 * buf must stay valid and unchanged until hbam_merge_end.  n == 0 is allowed.
 * words: the n sort words of the run's records, exactly hbam_sort_writables':
 *   HBAM_SORT_KEY         (uint64)key ^ 1 << 63
 *   HBAM_SORT_COORDINATE  (uint64)(uint32)refID << 32 | (uint32)(pos + 1)
 * or NULL: computed on the GPU from the encodings (hbam_decode_writables of
 * the run, whose errors apply to a bad value; the ctx's last batch becomes that
 * decode's).  With words given the last batch is untouched: a file ctx can
 * alternate hbam_decode_span, hbam_sort_writables and hbam_merge_add_run.
 * HBAM_SORT_QUERYNAME has no sort word: words must be NULL (else HBAM_E_ARG,
 * "words" in the message), the run is decoded as above, its records' names are
 * copied into HBM (name bytes + 10 B per record, held until hbam_merge_end) and
 * checked to be in (name, tie word) order.  The decode ends a split being read
 * with hbam_decode_span on the same ctx: merge on a codec ctx beside it.
 * Checked on the GPU, HBAM_E_ARG: offsets that do not increase, a record
 * shorter than 36 bytes or ending past len, offs[n] != len, words that are not
 * non-decreasing (hbam_last_error names the run and the first offending
 * record).  A total of 2^31 - 1 records or more -> HBAM_E_ARG.  A refused run
 * is not added.  After hbam_merge_plan, or with no merge open -> HBAM_E_STATE.
 *
 * hbam_merge_plan (once): sorts, cuts the output into parts and reports the
 * number of parts, the total records and the total bytes.  Output record j
 * belongs to part (its output start) / part_bytes (0: 1 GiB); parts in which no
 * record starts do not exist, so a part holds at least one record and fewer
 * than part_bytes + the longest record bytes.  No runs, or only empty ones:
 * 0 / 0 / 0.
 *
 * hbam_merge_next: the next part.  out == NULL sizes it: *n and *len are set,
 * nothing is launched and the part stays.  Otherwise out receives its *len
 * bytes, offs (NULL or n + 1 entries) the record starts relative to the part,
 * offs[n] = *len, src (NULL or n entries) run << 32 | record index in that run
 * (hbam_sort_writables' perm), and the merge moves on.  cap < *len ->
 * HBAM_E_ARG, the part stays.  Past the last part: HBAM_OK with *n = *len = 0.
 * Before hbam_merge_plan -> HBAM_E_STATE.
 *
 * hbam_merge_end frees the merge's device state (HBAM_OK with none open);
 * hbam_close ends an open merge. */
int hbam_merge_begin(hbam_ctx *ctx, int32_t order);
int hbam_merge_add_run(hbam_ctx *ctx, const uint8_t *buf, uint64_t len, const uint64_t *offs, uint64_t n,
                       const uint64_t *words /* NULL: computed from the encodings */);
int hbam_merge_plan(hbam_ctx *ctx, uint64_t part_bytes /* 0: 1 GiB */, uint64_t *n_parts, uint64_t *n_records,
                    uint64_t *bytes);
int hbam_merge_next(hbam_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *offs, uint64_t *src, uint64_t *n,
                    uint64_t *len);
int hbam_merge_end(hbam_ctx *ctx);
/* Measurement: HIP-event milliseconds of the open merge's plan (radix sort,
 * output starts, parts + cuts) and of its last written part (H2D of the
 * slices, source table + gather, D2H).  No merge open -> HBAM_E_STATE. */
int hbam_merge_times(hbam_ctx *ctx, float plan_ms[3], float part_ms[3]);

/* ---- BGZF write path ---- */
#define HBAM_BGZF_EOF 1 /* append the 28-byte BGZF EOF terminator (BlockCompressedOutputStream.close) */
/* [htsjdk] BlockCompressedOutputStream.write + deflateBlock + writeGzipBlock
 * (the compressor BAMRecordWriter.java:131-149 writes through) for a whole
 * payload stream, every block DEFLATEd on the GPU in one launch: one
 * java.util.zip.Deflater(level, nowrap) reset per block, output
 * byte-identical to zlib 1.2.11 (levels 0..9; htsjdk's default is 5); a block
 * that does not fit the 65518-byte compressed buffer is written by the
 * NO_COMPRESSION fallback (one stored block).  Blocks: block_lens[0..n_blocks)
 * (each <= 65536, as BlockCompressedOutputStream.flush cuts them; their sum
 * must be len), or when block_lens is NULL, len cut every block_size bytes.
 * *out (BGZF file bytes) is released with hbam_free. */
int hbam_bgzf_compress(const hbam_opts *opts, const void *data, uint64_t len, const uint32_t *block_lens,
                       uint64_t n_blocks, int32_t block_size, int32_t level, int32_t flags, uint8_t **out,
                       uint64_t *out_len);

/* BGZF block table (coff, csize, isize, ustart) and inflated bytes of the
 * whole file: used by tests and by the BGZF text formats. */
int hbam_blocks(hbam_ctx *ctx, uint64_t *coff, uint32_t *csize, uint32_t *isize, uint64_t *ustart,
                uint64_t cap, uint64_t *n);
int hbam_read_inflated(hbam_ctx *ctx, uint64_t pos, uint64_t len, uint8_t *dst);

/* Static key helpers (BAMRecordReader.getKey0 :119-121, getKey(int,int) :114-116,
 * MurmurHash3.murmurhash3(byte[],int) util/MurmurHash3.java:32-102): scalar API
 * for the SAM/CRAM readers that call getKey; the batch path computes keys on
 * the GPU. */
int64_t hbam_get_key0(int32_t ref_idx, int32_t alignment_start0);
int64_t hbam_get_key(int32_t ref_idx, int32_t alignment_start);
int64_t hbam_murmurhash3(const void *key, uint64_t len, int32_t seed);

/* ---- device-resident decode (benchmark / multi-GPU shard driver) ---- */
typedef struct hbam_gpu_stats {
  uint64_t n_blocks;          /* BGZF blocks located (summed over windows) */
  uint64_t compressed_bytes;  /* C of the span: file bytes from its first block to where it ended, each byte once */
  uint64_t inflated_bytes;    /* U of those blocks (windows overlap by a record's blocks: counted once) */
  uint64_t records;           /* N */
  uint64_t first_voff, last_voff;
  uint64_t key_xor, voff_sum; /* order-independent digests of the keys / voffs */
  float ms_locate, ms_inflate, ms_huff, ms_lz77, ms_chain, ms_decode, ms_total;
  int32_t status;
  int32_t link_fallbacks;     /* record-chain spans that took the exact serial link */
  int32_t inflate_launches;   /* phase A + B launch pairs of this run */
  int32_t link_rewalks;       /* parallel-link re-walk rounds of this run */
  int32_t windows;            /* HBM windows the span was decoded in */
  float ms_tables;            /* k_huff_tables (ms_huff: k_inflate_huff, ms_lz77: k_inflate_lz77) */
  int32_t record_fallbacks;   /* windows whose record lists overflowed (indexer mode, records < 36 bytes):
                               * per-block walks counted and emitted the records instead of the fused pass */
  /* order-sensitive digests (flags bit2): sum over the span's records i of
   * fmix64(x_i) * P^(n-1-i) mod 2^64, x = key / voff, P = HBAM_DIGEST_P;
   * the digests of consecutive spans A, B compose as D(A) * P^|B| + D(B) */
  uint64_t key_digest, voff_digest;
} hbam_gpu_stats;
#define HBAM_DIGEST_P 0x100000001b3ull

/* hbam_decode_span with the records left in HBM (no host copies): counts,
 * digests (flags bit2) and per-stage timings (flags bit0) only; flags bit1
 * skips the field decode (chain + voffs only). */
int hbam_decode_span_device(hbam_ctx *ctx, uint64_t vstart, uint64_t vend, int32_t flags, hbam_gpu_stats *st);

/* Cumulative counters of the ctx's decode pipeline since the open, over every
 * call (reader, indexer, device decodes): out[0] spans that took the exact
 * serial link, out[1] parallel-link re-walk rounds, out[2] windows whose
 * record lists overflowed, so that per-block walks counted and emitted the
 * records (hbam_gpu_stats.record_fallbacks), out[3] inflate launch pairs,
 * out[4] spans that stopped early (an error, EOF at an empty block) with
 * records listed in later blocks, which the stop drops.  Diagnostics: tests
 * assert which path a decode took. */
int hbam_pipeline_counters(hbam_ctx *ctx, uint64_t out[5]);

/* The BGZF block table of a range that starts at a known block start is
 * located by anchored chain walks: the range is cut into segments, one true
 * block start is found near every segment boundary, BSIZE is walked from
 * there, and the walks must join.  When they cannot vouch for the whole chain
 * they decline and the full header scan locates the range, so results and
 * errors never depend on which path ran.  Cumulative since the open, counted
 * on the host: out[0] ranges the walks located, out[1] ranges they declined.
 * (Kept apart from hbam_pipeline_counters, whose callers pass five words.) */
int hbam_locate_counters(hbam_ctx *ctx, uint64_t out[2]);
/* Test and measurement hook: the segment size of the anchored walks in bytes
 * (0: the full scan only; HBAM_LOCATE_SEG_DEFAULT: the built-in size, which
 * HBAM_LOCATE_SEG in the environment overrides at open) and an upper bound on
 * the candidate capacity of a range (0: none; ranges with more blocks take
 * the serial walk).  The window in place is located again at its next use. */
#define HBAM_LOCATE_SEG_DEFAULT UINT64_MAX
int hbam_set_locate(hbam_ctx *ctx, uint64_t seg_bytes, uint32_t cap_limit);

/* The LZ77 tokens inflate phase A wrote for the blocks of the ctx's current
 * window in its last pass (u32 each: phase A's output bytes / 4).  A
 * measurement helper for the bench's traffic figures (no reference
 * counterpart); synchronous. */
int hbam_inflate_token_count(hbam_ctx *ctx, uint64_t *tokens);

/* Which of inflate phase A's two kernels decoded the ctx's last inflate,
 * counted per block and decode round (a BGZF block of two DEFLATE blocks
 * takes two rounds): out[0] block rounds the lean instance decoded (at either
 * of its widths), out[1] block rounds it handed to the fallback kernel,
 * out[2] the resident workgroups per CU the runtime reports for the 256-lane
 * lean instance (its answer: a process that has a second copy of the HIP
 * runtime loaded can be told less than the hardware runs).  A measurement
 * helper (no reference counterpart); synchronous, the counters are read only
 * here. */
int hbam_inflate_path_counts(hbam_ctx *ctx, uint64_t out[3]);

/* The share of the lean instance's 128-lane width, which decodes the rounds
 * after a block's first: out[0] block rounds it decoded in the ctx's last
 * inflate (included in hbam_inflate_path_counts' out[0]), out[1] its resident
 * workgroups per CU as the runtime reports them, out[2] the bytes of
 * compressed window its stage holds (a round with a larger window goes to the
 * 256-lane width).  A measurement helper; synchronous. */
int hbam_inflate_narrow_counts(hbam_ctx *ctx, uint64_t out[3]);

/* Which rare paths the ctx's record chain took, cumulative since the open
 * over every call (hbam_pipeline_counters counts spans and rounds; these
 * count blocks): out[0] BGZF blocks whose first plausible record start gave a
 * walk that failed, so that later starts were searched, out[1] blocks whose
 * walk was off the true chain and that the link check asked to re-walk from
 * the chain's entry (counted per round, also when the walk refuses the entry
 * because the chain from it is not plausible), out[2] walks in blocks lying wholly inside one record that
 * the link check dropped because their exit would have misled later blocks,
 * out[3] link-check rounds (one per record pass when every walk is on the
 * chain).  out[0..2] are 32-bit on the device and wrap.  Diagnostics (no
 * reference counterpart): tests assert which path a decode took;
 * synchronous, the device counters are read only here. */
int hbam_chain_counters(hbam_ctx *ctx, uint64_t out[4]);

/* What the walk stage of the ctx's last record pass left, before the link
 * check saw it: per BGZF block of the pass the walk's start g (~0: none), its
 * exit x and the list word wcnt (bit 31: a plausible() walk, the rest: the
 * record starts counted), and in *list the first min(count, 2048) listed
 * offsets of every block back to back (*n_list of them).  Kept only when
 * HBAM_CHAIN_KEEP_WALK=1 was in the environment at the open; otherwise, and
 * before the first pass, *n_blocks = 0.  HBAM_CHAIN_WALK=lane at the open
 * makes the stage run as k_rec_cand + one lane per block instead of one wave
 * per block: the two must agree array for array; *stage says which ran (5: a
 * wave per block, 4: a lane per block, 0: nothing kept).  Measurement and tests (no
 * reference counterpart); synchronous; every array is the caller's
 * (hbam_free). */
int hbam_chain_lists(hbam_ctx *ctx, uint64_t **g, uint64_t **x, uint32_t **wcnt, uint16_t **list,
                     uint64_t *n_blocks, uint64_t *n_list, uint32_t *stage);

/* The sharded SplittingBAMIndexer.index (SplittingBAMIndexer.java:262-287,
 * SURVEY 8e step 3): the records of FileVirtualSplit [vstart, vend) read
 * under the indexer's rules (readAlignment/fullySkip, :340-368), their count
 * in *n_records and, given the global ordinal of the split's first record,
 * the virtual offsets of those whose ordinal + 1 is a multiple of
 * granularity in *entries (*n_entries of them; hbam_free).  The ranks of a
 * multi-GPU read concatenate their entries in split order between the first
 * record's voff and file_size << 16: byte-identical to index() over the
 * whole file. */
int hbam_splitting_entries(hbam_ctx *ctx, uint64_t vstart, uint64_t vend, int32_t granularity, uint64_t ordinal0,
                           uint64_t **entries, uint64_t *n_entries, uint64_t *n_records);

typedef struct hbam_gpu hbam_gpu;

int hbam_gpu_create(int32_t device, hbam_gpu **out);
void hbam_gpu_destroy(hbam_gpu *g);
const char *hbam_gpu_error(hbam_gpu *g);
/* Make a whole BAM file resident in HBM (copied from host memory) and parse
 * its header. */
int hbam_gpu_load(hbam_gpu *g, const void *data, uint64_t len);
/* HBM window of the decode (default 4 GiB of compressed bytes): a file larger
 * than the window is decoded window by window. */
int hbam_gpu_set_window(hbam_gpu *g, uint64_t window_bytes);
/* Validation stringency of the files loaded from now on (HBAM_STRICT when
 * never set); an unknown value -> HBAM_E_ARG. */
int hbam_gpu_set_stringency(hbam_gpu *g, int32_t stringency);
/* hbam_set_locate / hbam_locate_counters of the loaded file's pipeline */
int hbam_gpu_set_locate(hbam_gpu *g, uint64_t seg_bytes, uint32_t cap_limit);
int hbam_gpu_locate_counters(hbam_gpu *g, uint64_t out[2]);
/* hbam_sort_name_counters of the loaded file's pipeline */
int hbam_gpu_sort_name_counters(hbam_gpu *g, uint64_t out[3]);
/* Measurement: HIP-event milliseconds inside the order step (ms[0] of
 * hbam_gpu_sort_writables) of the last round of the last HBAM_SORT_QUERYNAME
 * call: name references + census + its read-back, the tie word's pass, the
 * chunk passes.  With HBAM_NAME_FULL_PASSES=1 in the environment when the file
 * is loaded, every chunk present is sorted over all 64 bits (the A/B of the
 * census's skipping and narrowing; the order is the same). */
int hbam_gpu_sort_name_times(hbam_gpu *g, float ms[3]);
/* One pass of the hot path over the resident file, first record to EOF:
 * BGZF discovery, inflate, record scan, field decode + keys + voffs, window by
 * window (flags as hbam_decode_span_device). */
int hbam_gpu_run(hbam_gpu *g, int32_t flags, hbam_gpu_stats *stats);
/* .splitting-bai of the resident file (SplittingBAMIndexer.index), *ms = HIP-event
 * time of the whole call. */
int hbam_gpu_index(hbam_gpu *g, int32_t granularity, uint8_t **buf, uint64_t *len, float *ms);
/* End-to-end pass from host memory: the file (same bytes/length as the loaded
 * one, one window) is copied host->HBM in pieces of piece_bytes on a copy
 * stream while the BGZF blocks of every landed piece are located and inflated
 * on the compute streams; then the record chain + decode (as hbam_gpu_run).
 * st->ms_total = first copy to last decode.  data should come from
 * hbam_host_alloc (page-locked) for the copies to overlap the kernels. */
int hbam_gpu_run_streamed(hbam_gpu *g, const void *data, uint64_t len, uint64_t piece_bytes, hbam_gpu_stats *st);
/* Page-locked host memory (what a JNI caller would wrap as a direct
 * ByteBuffer for the copy engine); NULL on failure. */
void *hbam_host_alloc(uint64_t bytes);
void hbam_host_free(void *p);
/* Copy the loaded file's bytes (same length) from host memory into HBM again,
 * timed (*ms, HIP events): the host->device leg of a PCIe-inclusive rate.
 * pinned != 0 copies from a page-locked staging copy (made untimed). */
int hbam_gpu_reload(hbam_gpu *g, const void *data, uint64_t len, int32_t pinned, float *ms);
/* Measured hipMemcpy device-to-device bandwidth, (read + write) GB/s. */
int hbam_gpu_d2d_bandwidth(hbam_gpu *g, uint64_t bytes, int32_t iters, float *gbps);
/* SAMRecordWritable.write of every record of the last run's last window into
 * a device buffer owned by g, iters timed times (HIP events on the pipeline
 * stream); hbam_gpu_fetch_encoded copies [pos, pos+len) of it to the host. */
int hbam_gpu_encode_writables(hbam_gpu *g, int32_t iters, float *ms_per_iter, uint64_t *bytes);
int hbam_gpu_fetch_encoded(hbam_gpu *g, uint64_t pos, uint64_t len, uint8_t *dst);
/* hbam_sort_writables of the records of the last hbam_gpu_run into the same
 * device buffer (hbam_gpu_fetch_encoded reads it), iters timed times: ms =
 * the per-iteration HIP-event times of (sort words + radix sort, lengths +
 * scan, gather).  For measuring only. */
int hbam_gpu_sort_writables(hbam_gpu *g, int32_t order, int32_t iters, float ms[3], uint64_t *bytes);
/* hbam_format_sam of the records of the last run's last window into the same
 * device buffer (hbam_gpu_fetch_encoded reads the text), iters timed times:
 * ms = the per-iteration HIP-event times of (the measuring pass, the scan of
 * the line lengths, the writing pass); *bytes = the text's size.  Errors as
 * hbam_format_sam's.  For measuring only. */
int hbam_gpu_format_sam(hbam_gpu *g, int32_t iters, float ms[3] /* measure, scan, write */, uint64_t *bytes);
/* BGZF-compress the inflated stream of the last run (one window) on the GPU
 * with the loaded file's block boundaries (hbam_bgzf_compress semantics;
 * iters timed repetitions, HIP events); the result stays in HBM,
 * hbam_gpu_fetch_compressed copies [pos, pos+len) of it to the host.
 * Recompressing a file written by zlib at the same level reproduces it byte
 * for byte. */
int hbam_gpu_bgzf_compress(hbam_gpu *g, int32_t level, int32_t flags, int32_t iters, float *ms_per_iter,
                           uint64_t *out_len);
int hbam_gpu_fetch_compressed(hbam_gpu *g, uint64_t pos, uint64_t len, uint8_t *dst);
/* Copy keys / voffs of the last run's last window to the host (either may be NULL). */
int hbam_gpu_fetch(hbam_gpu *g, int64_t *keys, uint64_t *voffs, uint64_t cap);
int32_t hbam_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* HBAM_H */
