// hbam_pipeline.h -- one HBM window of the BAM read hot path on one GPU.
//
// A Pipeline holds one window of a BGZF file: the compressed bytes [lo, hi)
// (copied from host memory or attached from a device-resident copy), its BGZF
// block table, the inflated stream of those blocks and the per-span record
// arrays.  A window that stops short of the end of the file is "open": a
// record that runs past its last block is not truncated, it is left for the
// next window (BamFile in hbam_host.h moves windows along a span and carries
// the next record's position across).  All compute runs in the gfx950
// kernels behind hbam_launch.h; the host sizes buffers, launches and reads
// back counters.  There is no CPU fallback: any HIP failure is an error
// returned to the caller.
#pragma once
#include "hbam_feed.h"
#include "hbam_mem.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hbam_device.h"
#include "hbam_launch.h"  // ChainArgs (SpanPass)

namespace hbam {

// A device buffer.  `owner` = the streams that may have queued work on it
// (its Pipeline's): releasing or regrowing it waits for those streams only.
// A buffer without an owner waits for the whole device.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;  // elements
  const StreamSet* owner = nullptr;
  DevBuf() = default;
  explicit DevBuf(const StreamSet* o) : owner(o) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void swap(DevBuf& o) {  // the contents; both keep their owner
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  hipError_t quiesce() const { return owner ? owner->sync() : hipDeviceSynchronize(); }
  void release() {
    if (p) {
      (void)quiesce();
      dev_free(p, n * sizeof(T));
    }
    p = nullptr;
    n = 0;
  }
  // grow, keeping the contents
  hipError_t grow(size_t count) {
    if (count <= n && p) return hipSuccess;
    const size_t c = count > 2 * n ? count : 2 * n;
    void* q = nullptr;
    size_t got = 0;
    hipError_t e = dev_alloc(&q, c * sizeof(T), &got);
    if (e != hipSuccess) return e;
    if (p) {
      if ((e = quiesce()) != hipSuccess) return e;
      // on the owner's stream: a plain hipMemcpy waits for the whole device
      if (owner && owner->n) {
        if ((e = hipMemcpyAsync(q, p, n * sizeof(T), hipMemcpyDeviceToDevice, owner->s[0])) != hipSuccess ||
            (e = hipStreamSynchronize(owner->s[0])) != hipSuccess)
          return e;
      } else if ((e = hipMemcpy(q, p, n * sizeof(T), hipMemcpyDeviceToDevice)) != hipSuccess) {
        return e;
      }
      dev_free(p, n * sizeof(T));
    }
    p = static_cast<T*>(q);
    n = got / sizeof(T);
    return hipSuccess;
  }
  // grow-only (contents not preserved)
  hipError_t reserve(size_t count) {
    if (count <= n && p) return hipSuccess;
    // half again the old size at least: a count that creeps up window by
    // window does not reallocate every time
    const size_t c = std::max<size_t>(count ? count : 1, p ? n + n / 2 : 0);
    release();
    void* q = nullptr;
    size_t got = 0;
    hipError_t e = dev_alloc(&q, c * sizeof(T), &got);
    if (e == hipSuccess) {
      p = static_cast<T*>(q);
      n = got / sizeof(T);
    }
    return e;
  }
};

// A page-locked host array of a trivially copyable T that kernels read or
// write in place (k_readback): the block table (54 K entries, 1.7 MB for C2)
// lands where the host reads it -- no zero fill on resize and no copy out of
// the read-back bounce buffer, ~0.11 ms of idle GPU per locate
// (profiles/r06/gaps.txt).
template <typename T>
class HostTable {
 public:
  HostTable() = default;
  HostTable(const HostTable&) = delete;
  HostTable& operator=(const HostTable&) = delete;
  ~HostTable() {
    if (p_) pinned_free(p_, bytes_);
  }
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  T* data() { return p_; }
  const T* data() const { return p_; }
  T& operator[](size_t i) { return p_[i]; }
  const T& operator[](size_t i) const { return p_[i]; }
  const T* begin() const { return p_; }
  const T* end() const { return p_ + n_; }
  const T& back() const { return p_[n_ - 1]; }
  void clear() { n_ = 0; }
  // keeps the first min(n, size()) elements, the others uninitialised; the
  // caller has waited for every kernel that reads or writes the array
  hipError_t resize(size_t n) {
    if (n > bytes_ / sizeof(T)) {
      void* q = nullptr;
      size_t got = 0;
      // at least 1 MiB: smaller page-locked blocks are not cached
      // (hbam_mem.cpp kMinCached), and hipHostFree waits for the device --
      // a drop-in context would pay it per window (ramped windows grow the
      // table several times per split)
      const size_t c = std::max(std::max(n, n_ + n_ / 2), (size_t(1) << 20) / sizeof(T));
      const hipError_t e = pinned_alloc(&q, c * sizeof(T), &got);
      if (e != hipSuccess) return e;
      if (n_) memcpy(q, p_, n_ * sizeof(T));
      if (p_) pinned_free(p_, bytes_);
      p_ = static_cast<T*>(q);
      bytes_ = got;
    }
    n_ = n;
    return hipSuccess;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0, bytes_ = 0;
};

// Result of one span decode, resident on the device.
struct SpanDev {
  uint64_t n = 0;                 // records
  uint64_t p0 = 0, q_end = 0;     // window positions: span start, first position past the span
  uint64_t next_pos = 0;          // chain position after the last record (the next record's start)
  int status = kOk;               // status of the first failing record (records before it are valid)
  std::string error;
  uint64_t* rec_pos = nullptr;    // device
  uint64_t* rec_voff = nullptr;   // device
  uint64_t first_voff = 0, last_voff = 0;  // rec_voff[0], rec_voff[n - 1] (host; read back with the span)
  Columns col{};                  // device (reader mode + decode)
  const uint8_t* data = nullptr;  // device stream rec_pos / rest_off index (nullptr = the inflated stream)
};

struct StageTimes {  // milliseconds of the last decode (HIP events)
  float locate = 0, inflate = 0, huff = 0, lz77 = 0, chain = 0, decode = 0;
  float tables = 0;  // k_huff_tables (huff: k_inflate_huff only)
};

// Streams and hardware queues.  HIP maps streams onto GPU_MAX_HW_QUEUES
// hardware queues (default 4) per priority level, and a context drives seven
// streams: four decode streams, the staging copy, and the drop-in batches'
// D2H and small reads.  On a shared queue an event or stream wait queued
// behind a batch's D2H holds the decode kernels behind it (resident drop-in
// loop: 32 GB/s U on shared queues, 42-44 with 8 queues).  The decode
// streams take the normal level, the batch streams the high one and the
// staging copy the low one, so each gets its own queue at the default.
enum class StreamLevel { kNormal, kHigh, kLow };
hipError_t create_stream(hipStream_t* s, StreamLevel level);

// Record-level validation ([htsjdk] ValidationStringency, the
// hadoopbam.samheaderreader.validation-stringency property).
enum Stringency : int { kStrict = 0, kLenient = 1, kSilent = 2 };

// What one Pipeline::inflate call does besides queueing the chunks:
//   kChecked   checks the DEFLATE status of [b0, b1) and waits for it (one host wait)
//   kQueued    leaves the work queued, no host wait: the caller checks later
//              (span_inflate: queue_inflate_check, the verdict with the link's read-back)
//   kStreamed  kQueued, and: every block of [b0, b1) is inflated whether marked
//              or not, and the last chunk's phase B stays on the phase-B stream,
//              beside what is queued next (run_streamed: the next piece's phase A)
enum class InflateMode { kChecked, kQueued, kStreamed };

// Anchored locate: bytes per segment (the S sweep)
#ifndef HBAM_LOCATE_SEG_BYTES
#define HBAM_LOCATE_SEG_BYTES (512u << 10)
#endif
constexpr uint64_t kLocateSegBytes = HBAM_LOCATE_SEG_BYTES;

class Pipeline {
 public:
  explicit Pipeline(int device);
  ~Pipeline();
  Pipeline(const Pipeline&) = delete;
  Pipeline& operator=(const Pipeline&) = delete;

  int device() const { return device_; }
  hipStream_t stream() const { return stream_; }
  // every stream this pipeline queues work on (owner of its buffers and of
  // buffers its callers hand it: BamFile's resident copy, ABI temporaries)
  const StreamSet& streams() const { return streams_; }
  const std::string& error() const { return err_; }

  // Device -> host reads of the host logic, queued as k_readback launches on
  // stream s into a page-locked buffer (shader engines: a pageable D2H of the
  // block table waited ~13 ms behind a drop-in batch's D2H on another
  // stream).  The bytes land in dst when rb_sync(s) returns; rb_sync(s)
  // synchronizes s in any case.
  hipError_t rb(void* dst, const void* src, size_t bytes, hipStream_t s);
  hipError_t rb_sync(hipStream_t s);
  // Forget the queued reads without copying: the queue holds raw host
  // addresses, mostly of the caller's frame, and a call that fails returns
  // before its rb_sync.  hip_check does this on every failure; a caller with
  // an error path of its own does it there.
  void rb_cancel();
  // dst (device) <- file bytes [off, off + len) of src through the copy
  // threads and bounce buffers (HostFeed), synchronously on the pipeline's
  // stream (a short read of src: kErrTrunc)
  int copy_from_host(uint8_t* dst, const HostSource& src, uint64_t off, uint64_t len);

  // Copy file bytes [base, base + len) into the window buffer.  at_eof: the
  // range ends at the end of the file (else the window is open).
  // When the window in place was loaded from the host too and holds a prefix
  // of the new range, that prefix moves device to device and only the rest
  // crosses PCIe; *host_bytes (optional) = the bytes copied from `data`.
  // (src: the file, read from offset base; data: its bytes [base, base + len) in memory)
  int load(const HostSource& src, uint64_t len, uint64_t base, bool at_eof, uint64_t* host_bytes = nullptr);
  int load(const uint8_t* data, uint64_t len, uint64_t base, bool at_eof, uint64_t* host_bytes = nullptr);
  // Start copying file bytes [lo, hi) of src into a staging buffer on the
  // copy stream; a later load() takes the part of its window inside [lo, hi)
  // from there (device-to-device) instead of the host, so a window's H2D
  // overlaps the previous window's decode.  src must outlive the copy.
  int stage(const HostSource& src, uint64_t lo, uint64_t hi);
  // the staging buffer sized for windows of up to `bytes` at once (growing it
  // later waits for the device)
  int reserve_stage(uint64_t bytes);
  // Use device-resident file bytes [base, base + len) (readable for kFilePad
  // bytes past len).
  int attach_device(const uint8_t* dptr, uint64_t len, uint64_t base, bool at_eof);
  // Copy the same-size window bytes into the resident buffer again, timed with
  // HIP events (PCIe-inclusive measurements); pinned: from a page-locked copy.
  int reload(const uint8_t* data, uint64_t len, bool pinned, float* ms);
  // hipMemcpy device-to-device bandwidth (read + write bytes per second / 1e9)
  int d2d_bandwidth(uint64_t bytes, int iters, float* gbps);
  uint64_t file_len() const { return flen_; }
  uint64_t base() const { return base_; }
  bool at_eof() const { return at_eof_; }
  const uint8_t* d_file() const { return dfile_; }

  // BGZF block discovery over the window.  An open window keeps only the
  // blocks that end inside it.  free_start: the window may begin inside a
  // block (split-guess windows); the block chain starts at the first header
  // candidate whose BSIZE chain runs to the window end.
  // locate() is locate_range over the whole window, then finish_blocks;
  // run_streamed calls locate_range per piece.  locate_range decides between
  // the paths below; its steps share one LocatePass (private, defined in
  // hbam_pipeline.cpp beside the names of flags_' words), in this order:
  //   locate_begin        capacities, cand_, flags_ zeroed
  //   locate_anchored     (lo is a block start, locate_seg_ != 0) k_bgzf_anchor_walk, its
  //                       verdict; accepted: k_bgzf_seg_emit into sorted_; else counted declined
  //   locate_scan         (no anchored table) k_bgzf_scan, the candidate count
  //   locate_verify       (1 .. cap candidates) the sort unless anchored, a free start's
  //                       candidates, k_bgzf_verify, locate_table queued behind its verdict;
  //                       accepts the table (the cut tail dropped) or asks for the serial walk
  //   locate_serial_walk  (more candidates than cap, none in a range with bytes, or a
  //                       broken chain) k_bgzf_walk from lo, or from each free-start
  //                       candidate in turn; its error texts; then locate_table
  //   locate_table        ustart by a scan, the table read back in place into hblocks_
  // Host waits of one range (production and timed alike; every one is an rb_sync):
  //   anchored, accepted            2  the walks' verdict; verify's verdict with the table
  //   scan, accepted                2  the candidate count; verify's verdict with the table
  //   anchored declined, then scan  3  both of the above counts, then verify's
  //   free start, accepted          3  the count; the candidates to try; verify's
  //   serial walk                   the waits up to it (1 from the scan's count, 2 or 3
  //                                 through a verify that found the chain broken), then 1
  //                                 per candidate tried (one candidate unless free start)
  //                                 and 1 for the table
  // A free start with no header candidate ends after the count (1); a buffer
  // that has to grow waits for the streams besides.  A timed locate() adds one
  // event wait.  finish_blocks waits for nothing.
  int locate(bool free_start = false);
  const HostTable<BlockInfo>& blocks() const { return hblocks_; }
  uint64_t total_u() const { return total_u_; }
  const BlockInfo* d_blocks() const { return dblocks_.p; }
  // file offset just past the last located block (where the next window starts)
  uint64_t window_end() const { return window_end_; }

  // Inflate blocks [b0, b1) into the contiguous inflated stream (InflateMode,
  // above: what else the call does).  The steps share one InflatePass
  // (private, defined in hbam_pipeline.cpp), in this order:
  //   inflate_plan     chunks of [b0, b1): even, at most kInflateChunkBlocks blocks each,
  //                    without the blocks inflated already (kStreamed: every block); host only
  //   inflate_reserve  a timed pass's events; token / table / info / list buffers for one
  //                    parity (two when chunks overlap); pstats_ and its zero; the fork
  //   inflate_chunk    per chunk j, parity par = j & 1: the waits on chunk j - 2, the list's
  //                    zero, per round tables + phase A, then phase B
  //   inflate_join     stream() waits for the phase Bs that ran beside it
  //   inflate_times    (timed) waits for the last event; the sums per launch kind
  //   kChecked only:   queue_inflate_check, rb_sync, inflate_verdict -- the one place
  //                    the DEFLATE error text is produced, for every caller
  // Streams of a production (untimed) pass, s = stream(), sB = the phase-B
  // stream, sT = the table stream (sB and sT wait for a fork event on s first):
  //   zero of pstats_, of a chunk's list      s
  //   tables, round 0                         first chunk: s; every later chunk: sT, and s
  //                                           waits for them (tab_ev_[par])
  //   tables, later rounds                    s
  //   phase A, every round                    s
  //   phase B                                 first and middle chunks: sB, after phase A
  //                                           (sync_ev_[par]); the last chunk (the only
  //                                           one, too): s -- but sB under kStreamed, which
  //                                           does not join
  //   chunk j >= 2                            s waits for phase B of chunk j - 2 (its token
  //                                           buffer: sync_ev_[2 + par]); sT for phase A of
  //                                           chunk j - 2 (its tables: hdone_ev_[par])
  //   the join                                s waits for phase B of the last chunk but one
  //                                           and, under kStreamed, of the last one
  // A timed pass (timing = true) puts every launch on s, in the order above,
  // each between two events of its own, with one set of buffers and none of
  // the cross-stream events.
  // Host waits: kChecked one (the verdict's rb_sync; a failing block's status
  // one more), kQueued and kStreamed none.  A timed pass adds one (the last
  // event) in every mode.  A buffer that has to grow waits for the streams.
  int inflate(uint32_t b0, uint32_t b1, InflateMode mode = InflateMode::kChecked);

  // End-to-end pass from host memory: the file (same length as the loaded
  // one) is copied to HBM in pieces on a copy stream while the BGZF blocks of
  // every piece that has landed are located and inflated, then the record
  // chain + decode run over the whole file (first record at stream position
  // first_pos).  data should be page-locked for the copies to overlap.
  // *ms = first copy to last decode (HIP events).
  int run_streamed(const uint8_t* data, uint64_t len, uint64_t piece_bytes, uint64_t first_pos, SpanDev* out,
                   float* ms);
  const uint8_t* d_u() const { return du_.p; }

  // Record chain over the span [vstart, vend) under reader or indexer rules;
  // decode=true also fills the SoA columns + keys (reader mode only).  In an
  // open window the span also ends at the first record that does not end
  // inside the window (out->next_pos = its start).
  int decode_span(uint64_t vstart, uint64_t vend, ChainMode mode, bool decode, SpanDev* out);
  // Same, from a window position (index mode: a carried position may lie
  // past the first block).  The pass is a sequence of steps over one SpanPass
  // (private, below), in this order:
  //   span_range      blocks [k0, k1) of the span, the inflate's end, the constant ChainArgs
  //   per round, until span_grow has nothing to add:
  //     span_inflate    blocks [k0, inf_end); the DEFLATE verdict rides with the link's read-back
  //     span_scratch    buffers, ChainArgs pointers, per-pass memsets, the walks
  //     span_link       link check (+ re-walk rounds or the serial link); chain end, list bound
  //     span_check_out  lists hold every record: check + output in one launch, the tail behind it
  //     span_count      a list overflowed: count + validate by walking
  //     span_grow       inflate further / take more blocks and go round again?
  //   span_status     the first failing block's status and text
  //   span_emit_walks (a list overflowed) offsets, outputs, k_rec_emit, k_rec_decode
  //   span_tail       long keys, the next record's start, first / last voff
  //                   (unless span_check_out's ran and its gate opened)
  //   span_times      the timed pass's stage times
  // Host waits of a production (untimed) round that lists every record and
  // finds the chain linked: two -- span_link's first check, which carries the
  // inflate's verdict, the chain's end and the list bound, and
  // span_check_out's verdict, which carries the tail.  A failing or stopping
  // block adds one (its status), a re-walk round or the serial link one each.
  // A timed pass waits also in the inflate, once more in the link (nothing is
  // queued ahead of a verdict) and in the tail.
  int decode_span_pos(uint64_t p0, uint64_t vend, ChainMode mode, bool decode, SpanDev* out);

  // Header bytes: inflate the first blocks until `need` stream bytes exist.
  int read_stream(uint64_t pos, uint64_t len, std::vector<uint8_t>* out);

  // SAMRecordWritable.write (SAMRecordWritable.java:55-64) of every record of
  // a decoded reader span, back to back: *bytes = size of the encodings;
  // encode_writables writes them to dst (device; room for bytes rounded up
  // to 16).  Record i's encoding starts at rec_pos[i] - rec_pos[0].
  int encoded_bytes(const SpanDev& span, uint64_t* bytes);
  int encode_writables(const SpanDev& span, uint64_t bytes, uint8_t* dst);
  // encode_writables with the records in sorted order (order: kSortKey /
  // kSortCoordinate of hbam_launch.h; stable): bytes = encoded_bytes(span).
  // The order and the output starts stay on the device until the next call:
  // sort_perm() (n u32, the span index of the j-th output record) and
  // sort_offsets() (n + 1 u64, the last = bytes).  ms (optional): the HIP-event
  // times of the sort words + radix sort, the lengths + scan and the gather
  // (waits for the stream).
  int sort_writables(const SpanDev& span, int order, uint64_t bytes, uint8_t* dst, float* ms = nullptr);
  // order kSortQueryname: the read name, then the flag's tie word (hbam_names.hip)
  const uint32_t* sort_perm() const { return sort_perm_.p; }
  const uint64_t* sort_offsets() const { return sort_doff_.p; }
  // SAM text of a decoded reader span (hbam_samtext.hip), one line per record
  // in batch order.  set_sam_refs: the reference names of the file's binary
  // dictionary, uploaded once as a packed table.  sam_measure: the measure pass
  // and the scan; *bytes = the text's size, *bad = the span index of the first
  // record whose fields leave its rest or whose aux fields are malformed (~0:
  // none; *bytes is then meaningless); the line starts stay on the device
  // until the next call: sam_offsets() (n + 1 u64, the last = *bytes).
  // sam_write: the text to dst (device, 16 B-aligned, room for bytes), only
  // after a sam_measure of the same span that found nothing malformed.  ms
  // (optional): HIP-event times of (measure, scan) and of the write pass (each
  // waits for the stream).  A failed device allocation: kErrNoMem.
  int set_sam_refs(const std::vector<std::string>& names);
  int sam_measure(const SpanDev& span, uint64_t* bytes, uint64_t* bad, float* ms2 = nullptr);
  int sam_write(const SpanDev& span, uint64_t bytes, uint8_t* dst, float* ms1 = nullptr);
  const uint64_t* sam_offsets() const { return sam_doff_.p; }
  // SAM text into BAM records (hbam_samparse.hip), one record per line.
  // samp_set_dict: the reference names RNAME / RNEXT resolve against, uploaded
  // as a table sorted for the kernels' binary search (a name that appears twice
  // keeps its lowest index); samp_has_dict: one was set.  samp_lines: the text
  // up to its last '\n' (final: all of it, a '\n' added behind a last line that
  // lacks one) goes to the device and its lines are found; *n = the lines,
  // *consumed = the text bytes they take.  samp_measure: every line validated
  // and measured, the scan; *bytes = the encodings' size, *bad = line << 8 |
  // field code (samp_field_name) of the first malformed line (~0: none).
  // samp_write: the records, only after a samp_measure that found nothing
  // malformed; they and their n + 1 starts land in page-locked host memory that
  // stays valid until the next samp_write: samp_enc(), samp_offs().
  // samp_times: HIP-event ms of the line finding, the measure pass, the scan
  // and the write pass of the last samp_write (0 where nothing ran).  A failed
  // device allocation: kErrNoMem.
  int samp_set_dict(const std::vector<std::string>& names);
  bool samp_has_dict() const { return samp_dict_n_ >= 0; }
  int samp_lines(const uint8_t* text, uint64_t len, bool final, uint64_t* n, uint64_t* consumed);
  int samp_measure(uint64_t n, uint64_t* bytes, uint64_t* bad);
  int samp_write(uint64_t n, uint64_t bytes);
  const uint8_t* samp_enc() const { return samp_enc_.data(); }
  const uint64_t* samp_offs() const { return samp_offs_.data(); }
  const float* samp_times() const { return samp_ms_; }
  // SAMRecordWritable.readFields (SAMRecordWritable.java:65-68) of n values
  // framed by offs in host memory (value i = buf[offs[i], offs[i+1]), the
  // last ends at len): SoA columns + keys; out->n stops at the first bad value.
  int decode_writables(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n, SpanDev* out);
  // launch_name_order on this pipeline's stream with its read-back queue:
  // perm = the queryname order of n records named by (base, name_pos, name_len,
  // tie).  The caller owns every buffer (sizes: hbam_launch.h).  The counters
  // of the last one: name_counters (chunks present, chunks sorted, bits sorted).
  // timed: ev_[0] / ev_[1] are recorded behind the census read-back and the tie
  // word's pass (sort_writables with ms turns them into name_times).
  int name_order(void* tmp, size_t tmp_bytes, const uint8_t* base, const uint64_t* name_pos, const uint8_t* name_len,
                 const uint8_t* tie, uint64_t n, uint64_t* word, uint64_t* word2, uint32_t* scratch, uint32_t* perm,
                 bool timed = false);
  const uint64_t* name_counters() const { return name_counters_; }
  // HIP-event milliseconds of the last timed queryname sort_writables: name
  // references + census + read-back, the tie word's pass, the chunk passes
  const float* name_times() const { return name_ms_; }

  // .splitting-bai entries of a span whose first record has global ordinal
  // `ordinal0` (SplittingBAMIndexer.java:273-277: ordinals k*g - 1)
  int splitting_entries(const SpanDev& span, uint32_t granularity, uint64_t ordinal0, std::vector<uint64_t>* out);
  // digests of a decoded span (bench / test checks): key xor, voff sum and
  // the order-sensitive key / voff digests (k_digest)
  int span_digest(const SpanDev& span, uint64_t out[4]);

  // host helpers on the block table
  int64_t pos_of_voff(uint64_t voff) const;
  uint64_t voff_of(uint64_t pos) const;
  uint64_t q_end_of(uint64_t vend) const;
  uint32_t block_containing(uint64_t pos) const;  // non-empty block with ustart <= pos < end, or nblocks

  void set_n_ref(int32_t n) { n_ref_ = n; }
  int32_t n_ref() const { return n_ref_; }
  void set_stringency(int s) { stringency_ = s; }
  // reference lengths for the STRICT alignment-start checks (empty = none)
  int set_ref_lengths(const std::vector<int32_t>& lens);

  uint64_t link_fallbacks() const { return link_fallbacks_; }
  uint64_t link_rewalks() const { return link_rewalks_; }
  uint64_t record_fallbacks() const { return record_fallbacks_; }
  uint64_t records_after_stop() const { return records_after_stop_; }
  uint64_t inflate_launches() const { return inflate_launches_; }
  // Anchored locate (locate_range): ranges whose table it produced / ranges
  // it declined, which the scan path then located
  uint64_t locate_anchored() const { return locate_anchored_; }
  uint64_t locate_declined() const { return locate_declined_; }
  // Segment bytes of the anchored locate (0: the scan path only; default
  // kLocateSegBytes, or HBAM_LOCATE_SEG from the environment) and a bound on
  // the candidate capacity (0: none).  Test and measurement hooks.
  void set_locate(uint64_t seg_bytes, uint32_t cap_limit) {
    locate_seg_ = seg_bytes;
    locate_cap_limit_ = cap_limit;
  }
  uint64_t locate_seg() const { return locate_seg_; }
  // LZ77 tokens phase A wrote for the window's blocks in its last inflate
  // (the sum of HuffOut::ntok; a synchronous read, for measurements)
  int inflate_tokens(uint64_t* n);
  // Phase A's paths in the last inflate (a synchronous read, for
  // measurements): out[0] = block rounds the lean instance decoded (either
  // width), out[1] = block rounds it handed to the fallback, out[2] = resident
  // workgroups per CU the runtime reports for the 256-lane lean instance
  int inflate_path_counts(uint64_t out[3]);
  // The narrow (128-lane) lean instance's share: out[0] = block rounds it
  // decoded, out[1] = its resident workgroups per CU as the runtime reports
  // them, out[2] = the bytes of window its stage holds
  int inflate_narrow_counts(uint64_t out[3]);
  // The record chain's rare paths since the open (a synchronous read, for
  // tests): out[0] = blocks handed to k_rec_search, out[1] = blocks the link
  // check re-walked from a forced entry, out[2] = stray walks it dropped,
  // out[3] = link-check rounds
  int chain_counters(uint64_t out[4]);
  // What the walk stage of the last record pass left, before any link round
  // (kept only under HBAM_CHAIN_KEEP_WALK=1; empty otherwise): per block g, x
  // and wcnt, and in `list` the first wcnt & kListCountMask entries of every
  // block's list back to back; *stage = the ChainStage that ran (kStageWalk or
  // kStageWalkLane; 0: nothing kept).  A synchronous read, for tests.
  int chain_lists(std::vector<uint64_t>* g, std::vector<uint64_t>* x, std::vector<uint32_t>* wcnt,
                  std::vector<uint16_t>* list, uint32_t* stage);
  StageTimes times;
  bool timing = false;  // record per-stage HIP event times

 private:
  int fail(int code, const std::string& msg);
  // BGZF blocks of [lo, hi) appended at index nprev with ustart from ubase,
  // on stream s (synchronized).  partial: a block cut by hi is left out and
  // *tail = its start (hi when none).
  int locate_range(uint64_t lo, uint64_t hi, bool partial, bool free_start, uint32_t nprev, uint64_t ubase,
                   hipStream_t s, uint32_t* nnew, uint64_t* tail);
  // The state of one locate_range call / one inflate call: like SpanPass
  // below, declared once in that function's frame and handed to the steps by
  // reference (rb() keeps the addresses of LocatePass's fields).  The step
  // maps are above locate() and inflate().
  struct LocatePass;
  int locate_begin(LocatePass& p);
  int locate_anchored(LocatePass& p, uint32_t nseg);
  int locate_scan(LocatePass& p);
  int locate_verify(LocatePass& p);
  int locate_serial_walk(LocatePass& p);
  int locate_table(LocatePass& p, uint32_t n);
  int finish_blocks();  // total_u_, dead positions, pads, per-block state after locate
  struct InflatePass;
  void inflate_plan(InflatePass& p, bool force);
  int inflate_reserve(InflatePass& p);
  int inflate_chunk(InflatePass& p, size_t j);
  int inflate_join(InflatePass& p);
  int inflate_times(InflatePass& p);
  hipError_t inflate_mark(InflatePass& p);  // a timed pass's next event, on stream_
  // the first failing block of [b0, b1)'s inflate, read back into
  // infl_first_ at the next rb_sync; inflate_verdict: its error, if any
  hipError_t queue_inflate_check(uint32_t b0, uint32_t b1);
  int inflate_verdict(uint32_t b0, uint32_t b1);
  // run_streamed's seams: capacity up front; per piece copy, locate and
  // inflate (*nblocks = the blocks located); the check and the decode stay in it
  int streamed_reserve(uint64_t len, uint64_t piece);
  int streamed_copy(const uint8_t* data, uint64_t len, uint64_t piece, uint64_t k);
  int streamed_pieces(const uint8_t* data, uint64_t len, uint64_t piece, uint32_t* nblocks);
  uint32_t infl_first_ = 0xffffffffu;
  bool inflate_queued_ = false;  // the last inflate() queued any chunk
  // SoA store for n records (voff = rec_voff_) + the deferred long-key list
  int alloc_columns(uint64_t n, uint64_t stream_bytes, Columns* c, bool zero_long_n = true);
  int hip_check(hipError_t e, const char* what);

  // The state of one decode_span_pos call.  It is declared once, in that
  // function's frame, and handed to the steps by reference; it is never
  // copied or returned by value, because rb() keeps the addresses of its
  // fields until the next rb_sync (or rb_cancel).
  struct SpanPass {
    SpanPass() = default;
    SpanPass(const SpanPass&) = delete;
    SpanPass& operator=(const SpanPass&) = delete;
    ChainArgs a{};
    ChainMode mode = kReader;
    bool dec = false;   // fill the columns and keys (reader mode)
    // a production pass queues ahead of the verdicts it waits for (the
    // inflate's with the link's, the list bound with the first link check,
    // the tail with the check-out); a timed pass queues nothing early
    bool ahead = false;
    uint32_t k0 = 0, k1 = 0, inf_end = 0, nblk = 0;
    Columns c{};
    float infl_ms = 0, huff_ms = 0, lz_ms = 0, tab_ms = 0;
    bool check_pending = false;  // the inflate's verdict lands with the next read-back
    // the link
    uint32_t ctr[2] = {0, 0};    // serial requests, blocks off the chain (one check round)
    uint64_t end[2] = {0, 0};    // the max-scan's last entry, the last block's exit
    uint64_t sm[2] = {0, 0};     // the chain's final position, != 0: it stopped there
    uint64_t last_base = 0;      // list_offsets: base_arr_[nb - 1], cnt_[nb - 1]
    uint32_t last_cnt = 0;
    uint32_t ovf = 0;            // a block listed more starts than kListCap
    bool lists = true;           // ovf == 0: the lists hold every record start
    uint64_t bound = 0;          // the lists' records (>= the span's)
    // the check-out / the count
    unsigned long long need = 0; // the furthest stream byte a record needs
    uint64_t bad = 0;            // k_rec_check_out's early-stop key (~0: none)
    uint32_t fl[2] = {0, 0};     // its first failing block
    uint64_t total = 0;          // the span's records
    uint32_t first = 0xffffffffu;  // the first failing or stopping block (of [k0, k1))
    int32_t code = 0;            // its status
    // the tail
    bool tail_done = false;      // queued behind k_rec_check_out, and its gate opened
    uint64_t next = 0, voff[2] = {0, 0};  // the next record's start, first / last voff
  };
  bool span_range(uint64_t p0, uint64_t vend, ChainMode mode, bool decode, SpanDev* out, SpanPass& s);
  int span_inflate(SpanPass& s);
  int span_scratch(SpanPass& s);
  int span_link(SpanPass& s);
  hipError_t chain_end(SpanPass& s);
  hipError_t list_offsets(SpanPass& s);
  hipError_t list_bound(SpanPass& s);
  int span_check_out(SpanPass& s);
  int span_count(SpanPass& s);
  bool span_grow(SpanPass& s);
  int span_status(SpanPass& s, SpanDev* out);
  int span_emit_walks(SpanPass& s, SpanDev* out);
  int span_tail(SpanPass& s, uint64_t n, bool gated);
  void span_times(const SpanPass& s);
  void dump_off_chain(const SpanPass& s, bool list_offsets_in_base);

  template <typename... B>
  void own(B&... b) {
    ((b.owner = &streams_), ...);
  }

  int device_ = 0;
  StreamSet streams_;
  hipStream_t stream_ = nullptr;
  hipStream_t stream_copy_ = nullptr;  // run_streamed: host->HBM pieces
  hipStream_t stream_stage_ = nullptr;  // stage(): the next window's bytes (not in streams_)
  StreamSet stage_owner_;              // stage_'s owner: stream_stage_ + stream_
  std::vector<hipEvent_t> copy_ev_;
  std::string err_;

  uint8_t* dfile_ = nullptr;
  DevBuf<uint8_t> own_file_;  // window bytes copied from the host (+ kFilePad zeros)
  DevBuf<uint8_t> own_spare_;  // the other buffer of the pair (a window's kept prefix moves across)
  DevBuf<uint8_t> stage_;      // stage(): file bytes [stage_lo_, stage_hi_) in flight / landed
  uint64_t stage_lo_ = 0, stage_hi_ = 0;
  std::thread stage_thr_;      // issues the staged copy (pageable copies block their caller)
  HostFeed feed_load_, feed_stage_;  // host -> HBM copies of load() and of the stage thread
  int stage_rc_ = 0;           // the staged copy's status (kOk = 0) and message
  std::string stage_msg_;
  int stage_wait();            // the staged copy done (its error, if any)
  // load() of file bytes [base, base + len) read from src at src_off + (x - base)
  int load_from(const HostSource& src, uint64_t src_off, uint64_t len, uint64_t base, bool at_eof,
                uint64_t* host_bytes);
  uint64_t flen_ = 0, base_ = 0;
  bool at_eof_ = true;
  uint64_t window_end_ = 0;

  DevBuf<BlockInfo> dblocks_;
  HostTable<BlockInfo> hblocks_;  // read back in place (k_readback)
  HostTable<uint64_t> hdead_;      // dead positions, copied to dead_ by k_readback
  uint64_t total_u_ = 0;
  uint32_t ndead_ = 0;
  // empty blocks among hblocks_ (counted by the verify kernel), or unknown
  static constexpr uint32_t kEmptyUnknown = 0xffffffffu;
  uint32_t empty_blocks_ = kEmptyUnknown;
  int32_t n_ref_ = 0;
  int stringency_ = kStrict;
  DevBuf<int32_t> ref_len_;
  uint32_t n_ref_len_ = 0;
  uint64_t link_fallbacks_ = 0;
  uint64_t link_rewalks_ = 0;      // re-walk rounds of the parallel link
  uint64_t link_rounds_ = 0;       // link-check launches (one per pass when every guess is on the chain)
  uint64_t record_fallbacks_ = 0;  // spans whose lists overflowed: records counted and emitted by walks
  uint64_t records_after_stop_ = 0;  // spans that stopped early with records listed in later blocks (dropped)
  uint32_t after_stop_flag_ = 0;     // (read back with a span's last readback)
  bool after_stop_pending_ = false;
  uint64_t inflate_launches_ = 0;  // phase A/B launch pairs so far
  uint64_t locate_anchored_ = 0, locate_declined_ = 0;
  uint64_t locate_seg_ = kLocateSegBytes;
  uint32_t locate_cap_limit_ = 0;

  DevBuf<uint8_t> du_;
  std::vector<uint8_t> inflated_;  // per block flag
  DevBuf<uint32_t> tokens_[2];  // LZ77 token streams, by chunk parity (overlapped inflate)
  DevBuf<HuffOut> hout_;
  DevBuf<uint8_t> tables_[2];     // phase-A prebuilt table images (per chunk, by chunk parity)
  hipStream_t stream_b_ = nullptr;  // inflate phase B (overlaps phase A of the next chunk)
  hipStream_t stream_t_ = nullptr;  // round-0 table build of chunk j beside phase A of chunk j-1
  hipEvent_t tab_ev_[2];            // tables of the chunk of that parity built
  hipEvent_t hdone_ev_[2];          // phase A of the chunk of that parity done (tables free)
  hipEvent_t sync_ev_[4];           // [0,1] phase A done, [2,3] phase B done, per token buffer
  DevBuf<HuffTableInfo> tinfo_[2];
  DevBuf<uint32_t> flist_[2];  // phase A's hand-over lists (per chunk, by chunk parity)
  DevBuf<uint32_t> pstats_;    // phase A's path counters of the last inflate (kPathStatWords)

  // span scratch
  DevBuf<uint64_t> g_, x_, x2_, entry_, base_arr_, summary_, dead_;
  DevBuf<uint64_t> cand_, sorted_, isz_, ust_;  // locate scratch
  DevBuf<uint32_t> cnt_, flags_;
  DevBuf<uint64_t> seg_anchor_, seg_exit_;  // anchored locate: per segment
  DevBuf<uint32_t> seg_cnt_, seg_off_;
  DevBuf<int32_t> errv_;
  DevBuf<unsigned long long> need_;
  DevBuf<uint64_t> rec_pos_, rec_voff_;
  DevBuf<uint64_t> rcand_, force_;  // chain v2
  DevBuf<uint32_t> wcnt_, counters_;
  DevBuf<uint16_t> list_;
  // HBAM_CHAIN_WALK=lane: the walk stage by k_rec_cand + a lane per block (the A/B of k_rec_walk_wave);
  // HBAM_CHAIN_KEEP_WALK=1: a copy of g, x, wcnt and the lists as the walk stage left them (chain_lists)
  bool walk_lane_ = false, keep_walk_ = false;
  DevBuf<uint64_t> kept_g_, kept_x_;
  DevBuf<uint32_t> kept_wcnt_;
  DevBuf<uint16_t> kept_list_;
  uint32_t kept_nb_ = 0, kept_stage_ = 0;
  DevBuf<uint32_t> fuse_;  // k_rec_check_out: [0..1] early-stop key (u64), [2] first failing block, [3] last block with records + 1
  DevBuf<uint8_t> scan_tmp_;
  DevBuf<uint8_t> cols_;  // SoA backing store
  uint64_t cols_cap_ = 0;
  DevBuf<uint64_t> long_rec_;            // records whose key k_long_hash computes
  DevBuf<uint32_t> long_n_;
  DevBuf<uint8_t> wbuf_;                 // readFields: serialized values
  DevBuf<uint64_t> woffs_;               // readFields: value framing
  DevBuf<unsigned long long> wbad_;      // readFields: first bad value
  DevBuf<uint64_t> scalars_;             // next_pos / digests read back by the host
  // sort_writables: sort words in / out, sorted lengths, output starts; lengths, iota, order; hipcub storage
  DevBuf<uint64_t> sort_word_, sort_word2_, sort_slen_, sort_doff_;
  DevBuf<uint32_t> sort_len_, sort_iota_, sort_perm_;
  DevBuf<uint8_t> sort_tmp_;
  // queryname order: where each name starts, its length, the tie word; the census words
  DevBuf<uint64_t> name_pos_, name_census_;
  DevBuf<uint8_t> name_len_, name_tie_;
  uint64_t name_counters_[3] = {0, 0, 0};
  float name_ms_[3] = {0, 0, 0};
  bool name_full_ = false;  // HBAM_NAME_FULL_PASSES: no chunk skipped, no bit range narrowed (measurement)

  // SAM text: the reference-name table; head lengths, line lengths, line starts, the malformed flag
  DevBuf<uint32_t> sam_ref_off_, sam_head_;
  DevBuf<uint8_t> sam_ref_bytes_, sam_tmp_;
  DevBuf<uint64_t> sam_llen_, sam_doff_;
  DevBuf<unsigned long long> sam_bad_;
  int32_t sam_n_ref_ = -1;  // -1: no table uploaded yet
  // SAM parse: the text, the '\n' counts of its pieces and their sum, the line starts, the record sizes
  // and starts, the first bad line, hipcub storage, the records; the sorted dictionary; the host copies
  DevBuf<uint8_t> samp_text_, samp_tmp_, samp_rec_, samp_dict_bytes_;
  DevBuf<uint64_t> samp_cnt_, samp_first_, samp_start_, samp_rlen_, samp_roff_;
  DevBuf<unsigned long long> samp_bad_;
  DevBuf<uint32_t> samp_dict_off_;
  DevBuf<int32_t> samp_dict_idx_;
  int32_t samp_dict_n_ = -1;  // -1: no dictionary uploaded yet
  uint64_t samp_len_ = 0;     // the text bytes on the device
  HostTable<uint8_t> samp_enc_;
  HostTable<uint64_t> samp_offs_;
  float samp_ms_[4] = {0, 0, 0, 0};
  hipEvent_t ev_[8];
  std::vector<hipEvent_t> tev_;     // timing events of overlapped inflate chunks

  // read-back queue (rb / rb_sync)
  struct RbItem {
    void* dst;
    size_t off, bytes;
  };
  uint8_t* rb_buf_ = nullptr;
  size_t rb_cap_ = 0, rb_used_ = 0;
  hipStream_t rb_stream_ = nullptr;
  std::vector<RbItem> rb_items_;
};

}  // namespace hbam
