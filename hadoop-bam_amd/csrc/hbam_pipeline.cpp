// hbam_pipeline.cpp -- host orchestration of one HBM window of the gfx950 BAM
// read pipeline (see hbam_pipeline.h).
#include "hbam_pipeline.h"

#include <thread>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hbam_launch.h"

namespace hbam {

namespace {
constexpr uint32_t kStreamInflateBlocks = 8192;  // run_streamed: blocks per inflate call
#ifndef HBAM_INFLATE_CHUNK
#define HBAM_INFLATE_CHUNK 65536
#endif
// blocks per phase-A/B launch pair: C2's 52 K blocks in one chunk beat two
// overlapped ones (phase B cannot share a CU with phase A, and each chunk pays
// its launch tails): 16.07-16.16 vs 16.13-16.25 ms per pass in three A/B runs
// (profiles/r06_late/variants_chunk_*.log); 20 K: 16.31, 16 K: -0.7 %, 8 K: -4 %
constexpr uint32_t kInflateChunkBlocks = HBAM_INFLATE_CHUNK;
constexpr int kMaxChainIters = 64;
constexpr int kMaxLinkFix = 4;        // re-walk rounds before the serial link
constexpr int kMaxFreeStarts = 64;    // header candidates tried by a free-start locate
// e_true of an open window: records may run past its last block
constexpr uint64_t kOpenEnd = 1ull << 62;
constexpr uint32_t kNoBlock = 0xffffffffu;  // "no failing block" of the first-error kernels
// the next `bytes` of a buffer carved up in 16 B-aligned pieces
uint8_t* take16(uint8_t** p, uint64_t bytes) {
  uint8_t* r = *p;
  *p += (bytes + 15) & ~15ull;
  return r;
}
bool cursor_trace() {
  static const bool tr = getenv("HBAM_CURSOR_TRACE") != nullptr;
  return tr;
}
}  // namespace

hipError_t create_stream(hipStream_t* s, StreamLevel level) {
  if (level == StreamLevel::kNormal) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return e;
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, level == StreamLevel::kHigh ? greatest : least);
}

Pipeline::Pipeline(int device) : device_(device) {
  if (hipSetDevice(device) != hipSuccess) {
    err_ = "hipSetDevice failed";
    return;
  }
  if (create_stream(&stream_, StreamLevel::kNormal) != hipSuccess ||
      create_stream(&stream_b_, StreamLevel::kNormal) != hipSuccess ||
      create_stream(&stream_t_, StreamLevel::kNormal) != hipSuccess ||
      create_stream(&stream_copy_, StreamLevel::kNormal) != hipSuccess ||
      create_stream(&stream_stage_, StreamLevel::kLow) != hipSuccess)
    err_ = "hipStreamCreate failed";
  streams_.s[0] = stream_;
  streams_.s[1] = stream_b_;
  streams_.s[2] = stream_t_;
  streams_.s[3] = stream_copy_;
  streams_.n = 4;
  // the staging copy (stage()) runs on its own stream, outside streams_: a
  // buffer of the decode that grows waits for the decode's streams only, not
  // for the next window's bytes on their way (that wait cost 5-13 ms per
  // drop-in window); stage_ itself is written there and read on stream_
  stage_owner_.s[0] = stream_stage_;
  stage_owner_.s[1] = stream_;
  stage_owner_.n = 2;
  stage_.owner = &stage_owner_;
  own(own_file_, own_spare_, dblocks_, ref_len_, du_, tokens_[0], tokens_[1], hout_, tables_[0], tables_[1],
      tinfo_[0], tinfo_[1], flist_[0], flist_[1], pstats_, g_, x_, x2_, entry_, base_arr_, summary_, dead_, cand_, sorted_, isz_, ust_, cnt_, flags_,
      errv_, need_, rec_pos_, rec_voff_, rcand_, force_, wcnt_, counters_, list_, scan_tmp_, cols_, long_rec_,
      long_n_, wbuf_, woffs_, wbad_, scalars_, fuse_, sort_word_, sort_word2_, sort_slen_, sort_doff_, sort_len_,
      sort_iota_, sort_perm_, sort_tmp_, name_pos_, name_census_, name_len_, name_tie_, seg_anchor_, seg_exit_, seg_cnt_, seg_off_);
  if (const char* e = getenv("HBAM_LOCATE_SEG")) locate_seg_ = strtoull(e, nullptr, 0);
  if (const char* e = getenv("HBAM_NAME_FULL_PASSES")) name_full_ = strtoull(e, nullptr, 0) != 0;
  if (const char* e = getenv("HBAM_CHAIN_WALK")) walk_lane_ = strcmp(e, "lane") == 0;
  if (const char* e = getenv("HBAM_CHAIN_KEEP_WALK")) keep_walk_ = strtoull(e, nullptr, 0) != 0;
  own(kept_g_, kept_x_, kept_wcnt_, kept_list_);
  for (auto& e : ev_) (void)hipEventCreate(&e);
  for (auto& e : sync_ev_) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : tab_ev_) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : hdone_ev_) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
}

Pipeline::~Pipeline() {
  if (stage_thr_.joinable()) stage_thr_.join();
  (void)hipSetDevice(device_);
  // this pipeline's own streams only: other contexts on the GPU run on
  (void)streams_.sync();
  (void)stage_owner_.sync();
  streams_.n = 0;  // drained: the member buffers release without waiting (the streams go below)
  stage_owner_.n = 0;
  if (rb_buf_) pinned_free(rb_buf_, rb_cap_);
  for (auto& e : ev_) (void)hipEventDestroy(e);
  for (auto& e : sync_ev_) (void)hipEventDestroy(e);
  for (auto& e : tab_ev_) (void)hipEventDestroy(e);
  for (auto& e : hdone_ev_) (void)hipEventDestroy(e);
  for (auto& e : tev_) (void)hipEventDestroy(e);
  for (auto& e : copy_ev_) (void)hipEventDestroy(e);
  for (hipStream_t s : {stream_b_, stream_t_, stream_copy_, stream_stage_, stream_})
    if (s) (void)hipStreamDestroy(s);
}

int Pipeline::fail(int code, const std::string& msg) {
  err_ = msg;
  return code;
}

int Pipeline::hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return kOk;
  err_ = std::string(what) + ": " + hipGetErrorString(e);
  rb_cancel();  // the failing call returns before its rb_sync: no queued read outlives its frame
  return kErrDevice;
}

#define HIPCHK(expr)                                  \
  do {                                                 \
    int _rc = hip_check((expr), #expr);                \
    if (_rc != kOk) return _rc;                        \
  } while (0)

int Pipeline::load(const uint8_t* data, uint64_t len, uint64_t base, bool at_eof, uint64_t* host_bytes) {
  HostSource m;
  m.mem = data;
  m.size = len;
  return load_from(m, 0, len, base, at_eof, host_bytes);
}

int Pipeline::load(const HostSource& src, uint64_t len, uint64_t base, bool at_eof, uint64_t* host_bytes) {
  return load_from(src, base, len, base, at_eof, host_bytes);
}

int Pipeline::load_from(const HostSource& src, uint64_t src_off, uint64_t len, uint64_t base, bool at_eof,
                        uint64_t* host_bytes) {
  HIPCHK(hipSetDevice(device_));
  // dst <- file bytes [base + a, base + a + n) (src offset src_off + a)
  auto feed = [&](uint64_t a, uint64_t n) -> int {
    std::string e;
    const int rc = feed_load_.copy(dfile_ + a, src, src_off + a, n, stream_, &e);
    if (rc != kOk) err_ = e;
    return rc;
  };
  const bool tr = cursor_trace();
  const auto t0 = std::chrono::steady_clock::now();
  // the prefix of [base, base + len) that the window in place already holds
  uint64_t keep = 0;
  if (dfile_ && own_file_.p && dfile_ == own_file_.p + (base_ & 15) && base >= base_ && base < base_ + flen_)
    keep = std::min(base_ + flen_, base + len) - base;
  const uint8_t* old = keep ? dfile_ + (base - base_) : nullptr;
  if (keep) own_file_.swap(own_spare_);
  // byte `base` lands at a buffer offset of base % 16: the kernels address the
  // window in file coordinates (dfile_ - base_) with 16 B aligned loads
  HIPCHK(own_file_.reserve(len + 16 + kFilePad));
  dfile_ = own_file_.p + (base & 15);
  if (keep) HIPCHK(hipMemcpyAsync(dfile_, old, keep, hipMemcpyDeviceToDevice, stream_));
  uint64_t host = 0;
  if (len > keep) {
    // [a, b): the part of the new bytes a stage() copy already brought over
    const uint64_t a = std::max(base + keep, stage_lo_), b = std::min(base + len, stage_hi_);
    if (stage_hi_ > stage_lo_ && a < b) {
      if (int rc = stage_wait()) return rc;
      if (a > base + keep)
        if (int rc = feed(keep, a - base - keep)) return rc;
      HIPCHK(hipMemcpyAsync(dfile_ + (a - base), stage_.p + (a - stage_lo_), b - a, hipMemcpyDeviceToDevice, stream_));
      if (base + len > b)
        if (int rc = feed(b - base, base + len - b)) return rc;
      host = len - keep - (b - a);
    } else {
      if (int rc = feed(keep, len - keep)) return rc;
      host = len - keep;
    }
  }
  if (host_bytes) *host_bytes = host;
  HIPCHK(hipMemsetAsync(dfile_ + len, 0, kFilePad, stream_));
  HIPCHK(rb_sync(stream_));
  if (tr)
    fprintf(stderr, "[load] %.3f ms: %llu B kept, %llu B from host\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
            (unsigned long long)keep, (unsigned long long)host);
  flen_ = len;
  base_ = base;
  at_eof_ = at_eof;
  window_end_ = base + len;
  hblocks_.clear();
  inflated_.clear();
  total_u_ = 0;
  return kOk;
}

hipError_t Pipeline::rb(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  // every read, a counter as the block table, goes through k_readback into
  // page-locked memory: a D2H copy into pageable memory waits behind other
  // copies on the DMA engines (a drop-in batch's columns: the 4-byte candidate
  // count of a window's locate took 13 ms behind them)
  hipError_t e;
  if (rb_stream_ && rb_stream_ != s && (e = rb_sync(rb_stream_)) != hipSuccess) return e;
  size_t off = (rb_used_ + 15) & ~size_t(15);
  if (off + bytes > rb_cap_) {
    if (!rb_items_.empty() && (e = rb_sync(s)) != hipSuccess) return e;  // the old buffer drains first
    if (rb_buf_) pinned_free(rb_buf_, rb_cap_);
    rb_buf_ = nullptr;
    rb_cap_ = 0;
    void* q = nullptr;
    size_t got = 0;
    if ((e = pinned_alloc(&q, std::max<size_t>(bytes + 4096, 1 << 20), &got)) != hipSuccess) return e;
    rb_buf_ = static_cast<uint8_t*>(q);
    rb_cap_ = got;
    off = 0;
  }
  if ((e = launch_readback(rb_buf_ + off, src, bytes, s)) != hipSuccess) return e;
  rb_items_.push_back(RbItem{dst, off, bytes});
  rb_used_ = off + bytes;
  rb_stream_ = s;
  return hipSuccess;
}

hipError_t Pipeline::rb_sync(hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess && rb_stream_ && rb_stream_ != s) e = hipStreamSynchronize(rb_stream_);
  if (e != hipSuccess) return e;
  for (const RbItem& it : rb_items_) memcpy(it.dst, rb_buf_ + it.off, it.bytes);
  rb_items_.clear();
  rb_used_ = 0;
  rb_stream_ = nullptr;
  return hipSuccess;
}

void Pipeline::rb_cancel() {
  rb_items_.clear();
  rb_used_ = 0;
  rb_stream_ = nullptr;
}

int Pipeline::copy_from_host(uint8_t* dst, const HostSource& src, uint64_t off, uint64_t len) {
  HIPCHK(hipSetDevice(device_));
  std::string e;
  const int rc = feed_load_.copy(dst, src, off, len, stream_, &e);
  if (rc != kOk) {
    HIPCHK(rb_sync(stream_));  // pieces already queued land before the caller moves on
    return fail(rc, e);
  }
  HIPCHK(rb_sync(stream_));
  return kOk;
}

int Pipeline::stage_wait() {
  if (stage_thr_.joinable()) stage_thr_.join();
  const int rc = stage_rc_;
  stage_rc_ = kOk;
  if (rc != kOk) {
    stage_lo_ = stage_hi_ = 0;
    return fail(rc, "staged host->HBM copy: " + stage_msg_);
  }
  return kOk;
}

int Pipeline::reserve_stage(uint64_t bytes) {
  HIPCHK(hipSetDevice(device_));
  if (int rc = stage_wait()) return rc;
  HIPCHK(stage_.reserve(bytes));
  return kOk;
}

int Pipeline::stage(const HostSource& src, uint64_t lo, uint64_t hi) {
  HIPCHK(hipSetDevice(device_));
  if (hi <= lo || (lo == stage_lo_ && hi == stage_hi_)) return kOk;  // nothing new to stage
  if (int rc = stage_wait()) return rc;
  HIPCHK(stage_.reserve(hi - lo));  // growing it waits for the device
  // A copy from pageable memory (the mapped file) returns only when it is
  // done, so a helper thread issues it: the caller goes on queueing this
  // window's decode while the next window's bytes cross the link.
  uint8_t* dst = stage_.p;
  const int dev = device_;
  hipStream_t cs = stream_stage_;
  const HostSource* hs = &src;
  stage_thr_ = std::thread([this, dst, hs, lo, hi, dev, cs]() {
    std::string msg;
    hipError_t e = hipSetDevice(dev);
    int rc = e == hipSuccess ? feed_stage_.copy(dst, *hs, lo, hi - lo, cs, &msg) : (int)kErrDevice;
    if (rc == kOk && (e = hipStreamSynchronize(cs)) != hipSuccess) rc = kErrDevice;
    if (rc == kErrDevice && msg.empty()) msg = hipGetErrorString(e);
    if (rc != kOk) (void)hipStreamSynchronize(cs);  // pieces already queued land first
    stage_msg_ = msg;
    stage_rc_ = rc;
  });
  stage_lo_ = lo;
  stage_hi_ = hi;
  return kOk;
}

int Pipeline::attach_device(const uint8_t* dptr, uint64_t len, uint64_t base, bool at_eof) {
  if ((reinterpret_cast<uintptr_t>(dptr) - base) & 15)
    return fail(kErrArg, "attach_device: file offset and device address differ in 16 B alignment");
  dfile_ = const_cast<uint8_t*>(dptr);
  flen_ = len;
  base_ = base;
  at_eof_ = at_eof;
  window_end_ = base + len;
  hblocks_.clear();
  inflated_.clear();
  total_u_ = 0;
  return kOk;
}

int Pipeline::reload(const uint8_t* data, uint64_t len, bool pinned, float* ms) {
  if (!dfile_ || dfile_ != own_file_.p + (base_ & 15) || len != flen_)
    return fail(kErrState, "reload needs a loaded window of the same size");
  HIPCHK(hipSetDevice(device_));
  uint8_t* staging = nullptr;
  if (pinned && len) {  // page-locked copy of the bytes (untimed), as a JNI direct buffer would be
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&staging), len, hipHostMallocDefault));
    memcpy(staging, data, len);
  }
  auto body = [&]() -> int {
    HIPCHK(hipEventRecord(ev_[6], stream_));
    if (len) HIPCHK(hipMemcpyAsync(dfile_, staging ? staging : data, len, hipMemcpyHostToDevice, stream_));
    HIPCHK(hipEventRecord(ev_[7], stream_));
    HIPCHK(hipEventSynchronize(ev_[7]));
    HIPCHK(hipEventElapsedTime(ms, ev_[6], ev_[7]));
    return kOk;
  };
  const int rc = body();
  if (staging) (void)hipHostFree(staging);
  return rc;
}

int Pipeline::d2d_bandwidth(uint64_t bytes, int iters, float* gbps) {
  *gbps = 0;
  DevBuf<uint8_t> a(&streams_), b(&streams_);
  HIPCHK(a.reserve(bytes));
  HIPCHK(b.reserve(bytes));
  HIPCHK(hipMemsetAsync(a.p, 1, bytes, stream_));
  HIPCHK(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, stream_));  // warm-up
  HIPCHK(hipEventRecord(ev_[6], stream_));
  for (int i = 0; i < iters; ++i) HIPCHK(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, stream_));
  HIPCHK(hipEventRecord(ev_[7], stream_));
  HIPCHK(hipEventSynchronize(ev_[7]));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev_[6], ev_[7]));
  *gbps = (float)(2.0 * (double)bytes * iters / ((double)ms * 1e6));  // read + write
  return kOk;
}

int Pipeline::inflate_tokens(uint64_t* n) {
  *n = 0;
  const size_t nb = hblocks_.size();
  if (nb == 0) return kOk;
  std::vector<HuffOut> h(nb);
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipStreamSynchronize(stream_b_));
  HIPCHK(hipMemcpy(h.data(), hout_.p, nb * sizeof(HuffOut), hipMemcpyDeviceToHost));
  for (const HuffOut& o : h) *n += o.ntok;
  return kOk;
}

int Pipeline::inflate_path_counts(uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  HIPCHK(hipSetDevice(device_));
  int wgs = 0;
  HIPCHK(huff_lean_occupancy(&wgs));
  out[2] = (uint64_t)wgs;
  if (!pstats_.p) return kOk;  // nothing inflated yet
  std::vector<uint32_t> st(kPathStatWords);
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipMemcpy(st.data(), pstats_.p, kPathStatWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < kPathStatSlots; ++k)
    out[0] += st[kPathStatLean + k * kPathStatStride] + st[kPathStatNarrow + k * kPathStatStride];
  out[1] = st[kPathStatFallback];
  return kOk;
}

int Pipeline::inflate_narrow_counts(uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  HIPCHK(hipSetDevice(device_));
  int wgs = 0;
  uint32_t cap = 0;
  HIPCHK(huff_narrow_occupancy(&wgs, &cap));
  out[1] = (uint64_t)wgs;
  out[2] = cap;
  if (!pstats_.p) return kOk;  // nothing inflated yet
  std::vector<uint32_t> st(kPathStatSlots * kPathStatStride);
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipMemcpy(st.data(), pstats_.p + kPathStatNarrow, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < kPathStatSlots; ++k) out[0] += st[k * kPathStatStride];
  return kOk;
}

int Pipeline::chain_counters(uint64_t out[4]) {
  out[0] = out[1] = out[2] = 0;
  out[3] = link_rounds_;
  if (!counters_.p) return kOk;  // no record pass yet
  HIPCHK(hipSetDevice(device_));
  uint32_t w[3] = {0, 0, 0};
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipMemcpy(w, counters_.p + kChainCtr, sizeof(w), hipMemcpyDeviceToHost));
  out[0] = w[kChainCtrSearched - kChainCtr];
  out[1] = w[kChainCtrRewalked - kChainCtr];
  out[2] = w[kChainCtrDropped - kChainCtr];
  return kOk;
}

int Pipeline::chain_lists(std::vector<uint64_t>* g, std::vector<uint64_t>* x, std::vector<uint32_t>* wcnt,
                          std::vector<uint16_t>* list, uint32_t* stage) {
  const uint32_t nb = kept_nb_;
  *stage = nb ? kept_stage_ : 0;
  g->assign(nb, 0);
  x->assign(nb, 0);
  wcnt->assign(nb, 0);
  list->clear();
  if (!nb) return kOk;  // no record pass yet, or nothing kept
  HIPCHK(hipSetDevice(device_));
  std::vector<uint16_t> all((size_t)nb * kListCap);
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipMemcpy(g->data(), kept_g_.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(x->data(), kept_x_.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(wcnt->data(), kept_wcnt_.p, (size_t)nb * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(all.data(), kept_list_.p, all.size() * 2, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < nb; ++i) {
    const uint32_t n = std::min((*wcnt)[i] & 0x7fffffffu, kListCap);  // (kListCountMask)
    list->insert(list->end(), all.begin() + (size_t)i * kListCap, all.begin() + (size_t)i * kListCap + n);
  }
  return kOk;
}

int Pipeline::set_ref_lengths(const std::vector<int32_t>& lens) {
  HIPCHK(ref_len_.reserve(lens.size() + 1));
  if (!lens.empty())
    HIPCHK(hipMemcpyAsync(ref_len_.p, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, stream_));
  HIPCHK(rb_sync(stream_));
  n_ref_len_ = (uint32_t)lens.size();
  return kOk;
}

// The words of flags_.  The kernels of the scan / verify path of a locate
// write them under these names:
// flags_[0] = candidate count, [1] = chain break, [2] = first big ISIZE, [3] = cut tail,
// [4] = empty blocks, [5] = anchored locate declined, [6] = its block count
// (k_bgzf_scan takes word 0, k_bgzf_verify words 1..4, the anchor walks 5..6).
enum LocateWord : uint32_t {
  kLocCandidates = 0,
  kLocChainBreak = 1,
  kLocBigIsize = 2,  // kNoBigIsize: none
  kLocCutTail = 3,
  kLocEmptyBlocks = 4,
  kLocDeclined = 5,
  kLocAnchoredBlocks = 6,
  kLocWords = 7
};
constexpr uint32_t kNoBigIsize = 0xffffffffu;
// The serial walk zeroes the first four again and k_bgzf_walk writes them as
// out[0..3]: the blocks it found, its status, the offset (lo, hi) where it
// stopped -- the failing block's, or with `partial` the cut block's start.
enum WalkWord : uint32_t { kWalkBlocks = 0, kWalkStatus = 1, kWalkAtLo = 2, kWalkAtHi = 3, kWalkWords = 4 };
// Outside a locate, word 3 is where the first-error kernels leave the first
// failing block (kNoBlock: none): queue_inflate_check, span_emit_walks.
constexpr uint32_t kFirstFailWord = 3;

// One locate_range call (the step map is in hbam_pipeline.h).
struct Pipeline::LocatePass {
  LocatePass() = default;
  LocatePass(const LocatePass&) = delete;
  LocatePass& operator=(const LocatePass&) = delete;
  // the arguments
  uint64_t lo = 0, hi = 0;
  bool partial = false, free_start = false;
  uint32_t nprev = 0;
  uint64_t ubase = 0;
  hipStream_t s = nullptr;
  uint32_t* nnew = nullptr;   // the results: blocks appended,
  uint64_t* tail = nullptr;   // the start of a block cut by hi
  const uint8_t* fbase = nullptr;  // absolute file coordinates
  uint64_t len = 0;
  uint32_t cap = 0, walk_cap = 0;  // candidates the verify path holds; the serial walk's table bound
  // the path so far
  bool anchored = false;  // the anchored walks left the block starts in sorted_
  bool serial = false;    // the serial walk has to (re)build the table
  bool found = false;     // ... and found a chain
  uint32_t count = 0;    // block starts in cand_ (the scan) or sorted_ (anchored)
  // read-back words
  uint32_t res[2] = {1, 0};          // kLocDeclined, kLocAnchoredBlocks
  uint32_t fl[4] = {0, 0, 0, 0};     // kLocChainBreak .. kLocEmptyBlocks
  uint64_t last = 0;                 // the last candidate (the cut tail, if any)
  uint32_t out[kWalkWords] = {0, 0, 0, 0};
  std::vector<uint64_t> starts;      // free start: candidates to try, in order
  uint32_t verdict(LocateWord w) const { return fl[w - kLocChainBreak]; }
};

// The decision between the paths; the steps follow in call order.
int Pipeline::locate_range(uint64_t lo, uint64_t hi, bool partial, bool free_start, uint32_t nprev, uint64_t ubase,
                           hipStream_t s, uint32_t* nnew, uint64_t* tail) {
  *nnew = 0;
  *tail = hi;
  LocatePass p;
  p.lo = lo;
  p.hi = hi;
  p.partial = partial;
  p.free_start = free_start;
  p.nprev = nprev;
  p.ubase = ubase;
  p.s = s;
  p.nnew = nnew;
  p.tail = tail;
  if (int rc = locate_begin(p)) return rc;
  // lo is a block start unless the start is free: the anchored walks first,
  // and the scan where they do not apply or decline
  const uint64_t nseg = locate_seg_ ? (p.len + locate_seg_ - 1) / locate_seg_ : 0;
  if (!free_start && nseg > 0 && nseg <= 0x7fffffffu)
    if (int rc = locate_anchored(p, (uint32_t)nseg)) return rc;
  if (!p.anchored)
    if (int rc = locate_scan(p)) return rc;
  if (free_start && p.count == 0) return kOk;  // no header in the window: no blocks
  if (p.count > 0 && p.count <= p.cap) {
    if (int rc = locate_verify(p)) return rc;
    if (!p.serial) return kOk;  // the chain holds: the table is in hblocks_
  } else if (p.len > 0) {
    p.serial = true;  // more candidates than cap, or bytes without a header (the walk has the error)
  }
  uint32_t n = 0;  // (an empty range: an empty table)
  if (p.serial) {
    if (int rc = locate_serial_walk(p)) return rc;
    if (!p.found) return kOk;  // free start: no block chain in the window
    n = p.out[kWalkBlocks];
  }
  if (int rc = locate_table(p, n)) return rc;
  HIPCHK(rb_sync(s));
  *nnew = n;
  return kOk;
}

// Capacities, cand_, and flags_ zeroed (kLocBigIsize = none).  No host wait.
int Pipeline::locate_begin(LocatePass& p) {
  p.fbase = dfile_ - base_;
  p.len = p.hi - p.lo;
  // candidate capacity assumes >= 1 KiB per block on average; denser files
  // (or any chain break) take the serial walk, whose table bound is len/26.
  p.cap = (uint32_t)std::min<uint64_t>(p.len / 1024 + 4096, 0x7fffffffu);
  if (locate_cap_limit_) p.cap = std::min(p.cap, locate_cap_limit_);
  p.walk_cap = (uint32_t)std::min<uint64_t>(p.len / 26 + 16, 0x7fffffffu);
  HIPCHK(cand_.reserve(p.cap));
  HIPCHK(flags_.reserve(8));
  // {0, 0, 0xffffffff, 0, 0} by fill kernels: a small pageable H2D can wait
  // behind other contexts' or the drop-in batches' copies on the DMA engines
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flags_.p), 0, kLocWords, p.s));
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flags_.p + kLocBigIsize), (int)kNoBigIsize, 1, p.s));
  return kOk;
}

// Anchored locate: lo is a block start, so the table is the BSIZE chain
// from lo.  Walks from one anchor per segment find it from the bytes around
// the segment boundaries and the headers; the block starts land in sorted_
// in file order, as the scan and the sort leave them.  Whenever the walks
// cannot vouch for the whole chain they decline (counted), and the scan path
// locates the range as if they had not run (its errors are the range's).
// One host wait (the walks' verdict).  Leaves anchored and count.
int Pipeline::locate_anchored(LocatePass& p, uint32_t nseg) {
  HIPCHK(seg_anchor_.reserve(nseg));
  HIPCHK(seg_exit_.reserve(nseg));
  HIPCHK(seg_cnt_.reserve(nseg));
  HIPCHK(seg_off_.reserve(nseg));
  HIPCHK(launch_bgzf_anchor_walk(p.fbase, p.lo, p.hi, locate_seg_, nseg, p.partial ? 1u : 0u, seg_anchor_.p,
                                 seg_exit_.p, seg_cnt_.p, seg_off_.p, flags_.p + kLocDeclined, p.s));
  HIPCHK(rb(p.res, flags_.p + kLocDeclined, sizeof p.res, p.s));
  HIPCHK(rb_sync(p.s));
  if (!p.res[0] && p.res[1] > 0 && p.res[1] <= p.cap) {
    p.count = p.res[1];
    HIPCHK(sorted_.reserve(p.count));
    HIPCHK(launch_bgzf_seg_emit(p.fbase, seg_anchor_.p, seg_cnt_.p, seg_off_.p, nseg, p.count, sorted_.p, p.s));
    p.anchored = true;
  } else {
    ++locate_declined_;
  }
  return kOk;
}

// The full scan: every header candidate of [lo, hi) into cand_, unsorted.
// One host wait (their count).
int Pipeline::locate_scan(LocatePass& p) {
  HIPCHK(launch_bgzf_scan(p.fbase, base_, p.lo, p.hi, cand_.p, p.cap, flags_.p + kLocCandidates, p.s));
  HIPCHK(rb(&p.count, flags_.p + kLocCandidates, 4, p.s));
  HIPCHK(rb_sync(p.s));
  return kOk;
}

// The count candidates (1 .. cap) as one chain: sorts the scan's, reads a
// free start's candidates (a host wait) and verifies from the first of them,
// else from lo.  One host wait for the verdict, with the table behind it.
// The chain holds: *nnew, *tail and hblocks_ are final (serial stays false);
// it breaks: serial = true.  Counts the empty blocks and, for an anchored
// table, locate_anchored_ / locate_declined_.
int Pipeline::locate_verify(LocatePass& p) {
  hipStream_t s = p.s;
  uint32_t n = p.count;
  HIPCHK(dblocks_.grow(p.nprev + n + 1));
  if (!p.anchored) {
    HIPCHK(sorted_.reserve(n));
    size_t tmp_bytes = 0;
    HIPCHK(sort_u64(nullptr, &tmp_bytes, cand_.p, sorted_.p, n, s));
    HIPCHK(scan_tmp_.reserve(tmp_bytes + 16));
    HIPCHK(sort_u64(scan_tmp_.p, &tmp_bytes, cand_.p, sorted_.p, n, s));
  }
  uint64_t from = p.lo;
  if (p.free_start) {
    p.starts.resize(std::min<uint32_t>(n, kMaxFreeStarts));
    HIPCHK(rb(p.starts.data(), sorted_.p, p.starts.size() * 8, s));
    HIPCHK(rb_sync(s));
    from = p.starts[0];
  }
  HIPCHK(launch_bgzf_verify(p.fbase, from, p.hi, sorted_.p, n, dblocks_.p + p.nprev, flags_.p + kLocChainBreak,
                            p.partial ? 1u : 0u, s));
  HIPCHK(rb(p.fl, flags_.p + kLocChainBreak, sizeof p.fl, s));
  HIPCHK(rb(&p.last, sorted_.p + n - 1, 8, s));
  // the table queued behind the verdict as if the chain holds (a false
  // header candidate breaks it: the serial walk then rebuilds the table); a
  // block cut by hi is the last entry, and the scan's entries before it do
  // not depend on it
  if (int rc = locate_table(p, n)) return rc;
  HIPCHK(rb_sync(s));
  const bool broken = p.verdict(kLocChainBreak) != 0;
  if (!broken && empty_blocks_ != kEmptyUnknown) empty_blocks_ += p.verdict(kLocEmptyBlocks);
  if (p.anchored) ++(broken ? locate_declined_ : locate_anchored_);  // (the walks checked what verify checks)
  if (broken) {
    p.serial = true;
    return kOk;
  }
  if (p.verdict(kLocBigIsize) != kNoBigIsize)
    return fail(kErrFormat, "BGZF block with ISIZE > 65536 (unsupported on device)");
  if (p.verdict(kLocCutTail)) {  // the last candidate's block is cut by hi: next range
    n -= 1;
    *p.tail = p.last;
  }
  HIPCHK(hblocks_.resize(p.nprev + n));  // (drops the cut block's entry)
  *p.nnew = n;
  return kOk;
}

// The serial BSIZE walk from lo -- or, free start, from each candidate of
// verify in turn until one chains to the end (a false header candidate fails
// or finds nothing).  One host wait per start tried.  Leaves found and out
// (kWalkBlocks = the table's size) and, with `partial`, *tail.
int Pipeline::locate_serial_walk(LocatePass& p) {
  empty_blocks_ = kEmptyUnknown;  // (the walk does not count them)
  HIPCHK(dblocks_.grow(p.nprev + p.walk_cap + 1));
  if (p.starts.empty()) p.starts.push_back(p.lo);
  for (size_t j = 0; j < p.starts.size() && !p.found; ++j) {
    HIPCHK(hipMemsetAsync(flags_.p, 0, kWalkWords * sizeof(uint32_t), p.s));
    HIPCHK(launch_bgzf_walk(p.fbase, p.starts[j], p.hi, dblocks_.p + p.nprev, p.walk_cap, flags_.p,
                            p.partial ? 1u : 0u, p.s));
    HIPCHK(rb(p.out, flags_.p, sizeof p.out, p.s));
    HIPCHK(rb_sync(p.s));
    const uint64_t at = (uint64_t)p.out[kWalkAtLo] | ((uint64_t)p.out[kWalkAtHi] << 32);
    if (p.out[kWalkStatus] != kOk) {
      if (p.free_start) continue;  // a false header candidate: try the next one
      return fail((int)p.out[kWalkStatus], "malformed BGZF block at offset " + std::to_string(at));
    }
    if (p.free_start && p.out[kWalkBlocks] == 0) continue;
    if (p.partial) *p.tail = at;
    p.found = true;
  }
  if (!p.found && !p.free_start) return fail(kErrFormat, "malformed BGZF block");
  return kOk;
}

// The block table of n located blocks: ustart by a scan, read back in place
// into page-locked hblocks_ (the read lands at the next rb_sync).  No host wait.
int Pipeline::locate_table(LocatePass& p, uint32_t n) {
  HIPCHK(dblocks_.grow(p.nprev + n + 1));
  BlockInfo* blocks = dblocks_.p + p.nprev;
  HIPCHK(isz_.reserve(n + 1));
  HIPCHK(ust_.reserve(n + 1));
  size_t sb = 0;
  HIPCHK(launch_block_ustart(blocks, n, isz_.p, ust_.p, nullptr, &sb, p.ubase, p.s));
  HIPCHK(scan_tmp_.reserve(sb + 16));
  HIPCHK(launch_block_ustart(blocks, n, isz_.p, ust_.p, scan_tmp_.p, &sb, p.ubase, p.s));
  HIPCHK(hblocks_.resize(p.nprev + n));
  if (n) HIPCHK(launch_readback(hblocks_.data() + p.nprev, blocks, n * sizeof(BlockInfo), p.s));
  return kOk;
}

int Pipeline::finish_blocks() {
  const uint32_t n = (uint32_t)hblocks_.size();
  total_u_ = n ? hblocks_[n - 1].ustart + hblocks_[n - 1].isize : 0;
  HIPCHK(du_.grow(total_u_ + kUPad));
  HIPCHK(hipMemsetAsync(du_.p + total_u_, 0, kUPad, stream_));
  inflated_.resize(n, 0);
  HIPCHK(hout_.grow(n + 1));
  // dead positions: [htsjdk] an empty block right after an exhausted one.
  // The verify kernel counted the empty blocks: with none, or only the EOF
  // block at the end, no walk over the block table (1.7 MB for C2, read
  // while the GPU waits) is needed.
  std::vector<uint64_t> dead;
  if (empty_blocks_ == 1 && n >= 2 && hblocks_[n - 1].isize == 0) {
    dead.push_back(hblocks_[n - 1].ustart);
  } else if (empty_blocks_ != 0) {
    for (uint32_t k = 1; k < n; ++k)
      if (hblocks_[k].isize == 0 && (dead.empty() || dead.back() != hblocks_[k].ustart))
        dead.push_back(hblocks_[k].ustart);
  }
  HIPCHK(dead_.reserve(dead.size() + 1));
  // from page-locked memory by a copy kernel: no host wait before the
  // inflate is planned (hdead_ is rewritten only by the next locate, after
  // its own read-backs have synchronized stream_)
  HIPCHK(hdead_.resize(dead.size()));
  if (!dead.empty()) {
    memcpy(hdead_.data(), dead.data(), dead.size() * 8);
    HIPCHK(launch_readback(dead_.p, hdead_.data(), dead.size() * 8, stream_));
  }
  ndead_ = (uint32_t)dead.size();
  return kOk;
}

int Pipeline::locate(bool free_start) {
  HIPCHK(hipSetDevice(device_));
  if (timing) HIPCHK(hipEventRecord(ev_[0], stream_));
  hblocks_.clear();
  inflated_.clear();
  empty_blocks_ = 0;
  uint32_t n = 0;
  uint64_t tail = 0;
  // free start (the split guessers): a last block cut by the end of the file
  // ends the chain like one cut by an open window's end; the blocks before it
  // stand, as for a reader that has not got there yet
  int rc = locate_range(base_, base_ + flen_, !at_eof_ || free_start, free_start, 0, 0, stream_, &n, &tail);
  if (rc != kOk) return rc;
  window_end_ = at_eof_ ? base_ + flen_ : tail;
  if (n && at_eof_ && free_start) window_end_ = hblocks_[n - 1].coff + hblocks_[n - 1].csize;
  if (timing) {
    HIPCHK(hipEventRecord(ev_[1], stream_));
    HIPCHK(hipEventSynchronize(ev_[1]));
    (void)hipEventElapsedTime(&times.locate, ev_[0], ev_[1]);
  }
  return finish_blocks();
}

int Pipeline::run_streamed(const uint8_t* data, uint64_t len, uint64_t piece, uint64_t first_pos, SpanDev* out,
                           float* ms) {
  *ms = 0;
  *out = SpanDev();
  if (!dfile_ || dfile_ != own_file_.p || len != flen_ || base_ != 0 || !at_eof_)
    return fail(kErrState, "run_streamed needs the whole file loaded in one window");
  HIPCHK(hipSetDevice(device_));
  if (int rc = stage_wait()) return rc;  // no staged copy in flight over the window being replaced
  piece = std::max<uint64_t>(piece, 1ull << 20);
  if (int rc = streamed_reserve(len, piece)) return rc;
  HIPCHK(hipEventRecord(ev_[6], stream_copy_));
  uint32_t nb = 0;
  if (int rc = streamed_pieces(data, len, piece, &nb)) return rc;
  window_end_ = base_ + len;
  int rc = finish_blocks();  // (the inflates: ordered before stream_'s next work)
  if (rc != kOk) return rc;
  HIPCHK(queue_inflate_check(0, nb));
  HIPCHK(rb_sync(stream_));
  if ((rc = inflate_verdict(0, nb)) != kOk) return rc;
  rc = decode_span(voff_of(first_pos), ~0ull, kReader, true, out);
  if (rc != kOk) return rc;
  HIPCHK(hipEventRecord(ev_[7], stream_));
  HIPCHK(hipEventSynchronize(ev_[7]));
  HIPCHK(hipEventElapsedTime(ms, ev_[6], ev_[7]));
  return kOk;
}

// Capacity up front, so that nothing reallocates under queued work (grow()
// still handles a file that outruns the estimates, at the cost of a wait).
// Waits for the pipeline's streams.
int Pipeline::streamed_reserve(uint64_t len, uint64_t piece) {
  HIPCHK(dblocks_.grow(len / 16384 + 4096));
  HIPCHK(hout_.grow(len / 16384 + 4096));
  HIPCHK(du_.grow(std::max<uint64_t>(total_u_, 4 * len) + kUPad));
  const uint64_t chunk_u = std::min<uint64_t>(8 * piece, (uint64_t)kInflateChunkBlocks * 65536);
  for (int i = 0; i < 2; ++i) HIPCHK(tokens_[i].reserve(chunk_u + 16));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(tables_[i].reserve((uint64_t)kInflateChunkBlocks * kHuffTableImage));
    HIPCHK(tinfo_[i].reserve(kInflateChunkBlocks));
    HIPCHK(flist_[i].reserve(huff_list_words(kInflateChunkBlocks)));
  }
  HIPCHK(pstats_.reserve(kPathStatWords));
  HIPCHK(streams_.sync());
  return kOk;
}

// piece k of the file on its way to HBM, on stream_copy_
int Pipeline::streamed_copy(const uint8_t* data, uint64_t len, uint64_t piece, uint64_t k) {
  const uint64_t o = k * piece, sz = std::min(piece, len - o);
  HIPCHK(hipMemcpyAsync(dfile_ + o, data + o, sz, hipMemcpyHostToDevice, stream_copy_));
  return kOk;
}

// Piece k's copy and its locate run in order on stream_copy_, the inflate
// of located blocks on the inflate streams.  (With locate on its own stream,
// which shares a hardware queue with stream_ at GPU_MAX_HW_QUEUES = 4, every
// locate waited behind the queued inflates: copy and decode serialized.)
// Host waits: each piece's locate.  *nblocks = the blocks located, every one
// handed to inflate.
int Pipeline::streamed_pieces(const uint8_t* data, uint64_t len, uint64_t piece, uint32_t* nblocks) {
  const uint64_t np = std::max<uint64_t>(1, (len + piece - 1) / piece);
  if (int rc0 = streamed_copy(data, len, piece, 0)) return rc0;
  hblocks_.clear();
  inflated_.clear();
  empty_blocks_ = 0;
  total_u_ = 0;
  uint64_t lo = base_;
  uint32_t nb = 0, queued = 0;  // blocks located / handed to inflate
  for (uint64_t k = 0; k < np; ++k) {
    const bool last = k + 1 == np;
    const uint64_t hi = base_ + (last ? len : (k + 1) * piece);
    uint32_t nnew = 0;
    uint64_t tail = hi;
    int rc = locate_range(lo, hi, !last, false, nb, total_u_, stream_copy_, &nnew, &tail);
    if (rc != kOk) return rc;
    if (!last && (rc = streamed_copy(data, len, piece, k + 1)) != kOk) return rc;  // on the wire while piece k inflates
    if (nnew) {
      const BlockInfo& e = hblocks_[nb + nnew - 1];
      total_u_ = e.ustart + e.isize;
      HIPCHK(du_.grow(total_u_ + kUPad));
      HIPCHK(hout_.grow(nb + nnew + 1));
      inflated_.resize(nb + nnew, 0);
      nb += nnew;
    }
    // inflate in launches of >= kStreamInflateBlocks blocks: a piece's few
    // thousand blocks alone would leave most CUs idle in each round's tail
    if (nb > queued && (nb - queued >= kStreamInflateBlocks || last)) {
      rc = inflate(queued, nb, InflateMode::kStreamed);  // (phase B beside the next piece's phase A)
      if (rc != kOk) return rc;
      queued = nb;
    }
    lo = tail;
  }
  *nblocks = nb;
  return kOk;
}

// One inflate call (the step map, with the stream of every launch, is in
// hbam_pipeline.h).  Chunks of up to kInflateChunkBlocks blocks: per chunk
// the table build and phase A in rounds, then phase B.  Production runs
// overlap them: phase A on stream_, phase B on stream_b_ after it, the
// round-0 tables of chunk j on stream_t_ beside phase A of chunk j-1, token
// and table buffers by chunk parity (~0.7 ms per C2 pass faster than one
// stream).  A timed run (measurement) puts every launch on stream_, each
// bracketed by events, so its per-kernel times are kernel durations, as
// rocprofv3 reports them.
struct Pipeline::InflatePass {
  InflatePass() = default;
  InflatePass(const InflatePass&) = delete;
  InflatePass& operator=(const InflatePass&) = delete;
  uint32_t b0 = 0, b1 = 0;
  const uint8_t* fbase = nullptr;
  bool serial = false;  // a timed pass: one stream, one set of buffers, events around every launch
  bool join = true;     // the last chunk's phase B on stream_ itself
  struct Chunk { uint32_t b, e; };
  std::vector<Chunk> chunks;
  size_t ne = 0;  // events recorded (serial)
  float tab_ms = 0, huff_ms = 0, lz_ms = 0;
};

int Pipeline::inflate(uint32_t b0, uint32_t b1, InflateMode mode) {
  HIPCHK(hipSetDevice(device_));
  inflate_queued_ = false;
  b1 = std::min(b1, (uint32_t)hblocks_.size());
  if (b0 >= b1) return kOk;
  if (timing) HIPCHK(hipEventRecord(ev_[2], stream_));
  InflatePass p;
  p.b0 = b0;
  p.b1 = b1;
  p.fbase = dfile_ - base_;
  p.serial = timing;
  p.join = mode != InflateMode::kStreamed;
  inflate_plan(p, mode == InflateMode::kStreamed);
  if (p.chunks.empty()) {
    times.inflate = times.huff = times.lz77 = times.tables = 0;
    return kOk;
  }
  if (int rc = inflate_reserve(p)) return rc;
  for (size_t j = 0; j < p.chunks.size(); ++j)
    if (int rc = inflate_chunk(p, j)) return rc;
  if (int rc = inflate_join(p)) return rc;
  if (timing)
    if (int rc = inflate_times(p)) return rc;
  inflate_queued_ = true;
  if (mode != InflateMode::kChecked) return kOk;  // the caller checks hout_ once all blocks are queued
  HIPCHK(queue_inflate_check(b0, b1));
  if (timing) HIPCHK(hipEventRecord(ev_[3], stream_));
  HIPCHK(rb_sync(stream_));
  if (timing) {
    (void)hipEventElapsedTime(&times.inflate, ev_[2], ev_[3]);
    times.tables = p.tab_ms;
    times.huff = p.huff_ms;
    times.lz77 = p.lz_ms;
  }
  return inflate_verdict(b0, b1);
}

// The chunks of [b0, b1), without the blocks inflated already unless `force`.
// Host code only; reads inflated_.
void Pipeline::inflate_plan(InflatePass& p, bool force) {
  const uint32_t b0 = p.b0, b1 = p.b1;
  // (the GPU is idle here: the common case -- nothing of [b0, b1) inflated
  // yet -- is planned without a walk over the blocks)
  const bool fresh = force || std::find(inflated_.begin() + b0, inflated_.begin() + b1, (uint8_t)1) ==
                                  inflated_.begin() + b1;
  uint32_t b = b0;
  while (b < b1) {
    if (!fresh && inflated_[b]) { ++b; continue; }
    // even chunks (a short last chunk would pay a whole wave tail for few blocks)
    const uint32_t left = b1 - b;
    const uint32_t nchunks = (left + kInflateChunkBlocks - 1) / kInflateChunkBlocks;
    const uint32_t per = (left + nchunks - 1) / nchunks;
    uint32_t e = b;
    if (fresh) e = std::min(b1, b + per);
    else while (e < b1 && e - b < per && !inflated_[e]) ++e;
    p.chunks.push_back({b, e});
    b = e;
  }
}

// A timed pass's events; every buffer for the largest chunk, one set or (the
// chunks overlap) one per parity; pstats_ zeroed on stream_; the fork of
// stream_b_ and stream_t_ off stream_.  No host wait unless a buffer grows.
int Pipeline::inflate_reserve(InflatePass& p) {
  const size_t nc = p.chunks.size();
  const size_t per_chunk = 2 * (2 * kInflateRounds + 1);  // event pairs: tables + phase A per round, phase B
  if (timing && tev_.size() < per_chunk * nc) {
    const size_t old = tev_.size();
    tev_.resize(per_chunk * nc);
    for (size_t i = old; i < tev_.size(); ++i) HIPCHK(hipEventCreate(&tev_[i]));
  }
  // size every buffer up front: a reallocation inside the loop could free a
  // token buffer that phase B of an earlier chunk is still reading
  uint64_t max_u = 64, max_nb = 0;
  for (const InflatePass::Chunk& c : p.chunks) {
    max_u = std::max(max_u, hblocks_[c.e - 1].ustart + hblocks_[c.e - 1].isize - hblocks_[c.b].ustart);
    max_nb = std::max<uint64_t>(max_nb, c.e - c.b);
  }
  const int nbuf = nc > 1 && !p.serial ? 2 : 1;
  for (int i = 0; i < nbuf; ++i) {
    HIPCHK(tokens_[i].reserve(max_u + 16));  // phase B reads tokens as uint4
    HIPCHK(tables_[i].reserve(max_nb * kHuffTableImage));
    HIPCHK(tinfo_[i].reserve(max_nb));
    HIPCHK(flist_[i].reserve(huff_list_words(max_nb)));
  }
  HIPCHK(pstats_.reserve(kPathStatWords));
  HIPCHK(hipMemsetAsync(pstats_.p, 0, kPathStatWords * sizeof(uint32_t), stream_));
  if (!p.serial) {  // phase B and the table builds see everything queued on stream_ before this call
    // (sync_ev_[0] serves twice: here as the fork, then as "phase A of an
    // even chunk done" in inflate_chunk.  The two waits below are queued
    // before it is recorded again, and a wait holds the record it was queued on.)
    HIPCHK(hipEventRecord(sync_ev_[0], stream_));
    HIPCHK(hipStreamWaitEvent(stream_b_, sync_ev_[0], 0));
    HIPCHK(hipStreamWaitEvent(stream_t_, sync_ev_[0], 0));
  }
  return kOk;
}

hipError_t Pipeline::inflate_mark(InflatePass& p) {
  return p.serial ? hipEventRecord(tev_[p.ne++], stream_) : hipSuccess;
}

// Chunk j: the waits on chunk j-2 (same parity, same buffers), the list's
// zero, per round tables + phase A, then phase B; marks its blocks inflated.
// No host wait.
int Pipeline::inflate_chunk(InflatePass& p, size_t j) {
  const size_t nc = p.chunks.size();
  const uint32_t cb = p.chunks[j].b, ce = p.chunks[j].e;
  const bool serial = p.serial;
  const int par = serial ? 0 : (int)(j & 1);
  const uint64_t cu = hblocks_[cb].ustart;
  // The stream of the round-0 tables and of phase B; everything else, and
  // all of a timed pass, runs on stream_.
  // (the first chunk's round-0 tables run on stream_ itself: nothing runs
  // beside them, and a cross-stream wait costs ~15 us at the pass's start)
  const bool t_own = !serial && j > 0;
  // the last chunk's phase B on stream_ itself: nothing of this call is
  // left to overlap it, and the chain after it then needs no cross-stream wait
  const bool b_own = !serial && (j + 1 < nc || !p.join);
  hipStream_t sT = t_own ? stream_t_ : stream_, sB = b_own ? stream_b_ : stream_;
  if (!serial && j >= 2) {
    HIPCHK(hipStreamWaitEvent(stream_, sync_ev_[2 + par], 0));  // B(j-2) released the token buffer
    HIPCHK(hipStreamWaitEvent(stream_t_, hdone_ev_[par], 0));   // A(j-2) released the table buffer
  }
  // (the list is written and read on stream_ only: the chunk of the same
  // parity before this one is done with it)
  HIPCHK(hipMemsetAsync(flist_[par].p, 0, kHuffListHdr * sizeof(uint32_t), stream_));
  // rounds: each decode stops a block before its next DEFLATE header, which
  // the next round's table build parses (the last round decodes inline)
  for (uint32_t r = 0; r < kInflateRounds; ++r) {
    HIPCHK(inflate_mark(p));
    HIPCHK(launch_huff_tables(p.fbase, dblocks_.p, cb, ce - cb, tables_[par].p, tinfo_[par].p, hout_.p, r,
                              r == 0 ? sT : stream_));
    HIPCHK(inflate_mark(p));
    if (r == 0 && t_own) {
      HIPCHK(hipEventRecord(tab_ev_[par], stream_t_));
      HIPCHK(hipStreamWaitEvent(stream_, tab_ev_[par], 0));
    }
    HIPCHK(inflate_mark(p));
    HIPCHK(launch_inflate_huff_prebuilt(p.fbase, dblocks_.p, cb, ce - cb, cu, tokens_[par].p, hout_.p,
                                        tables_[par].p, tinfo_[par].p, r, r + 1 < kInflateRounds ? 1u : 0u,
                                        flist_[par].p, pstats_.p, stream_));
    HIPCHK(inflate_mark(p));
  }
  if (!serial) HIPCHK(hipEventRecord(hdone_ev_[par], stream_));
  if (b_own) {
    HIPCHK(hipEventRecord(sync_ev_[par], stream_));
    HIPCHK(hipStreamWaitEvent(stream_b_, sync_ev_[par], 0));
  }
  HIPCHK(inflate_mark(p));
  HIPCHK(launch_inflate_lz77(dblocks_.p, cb, ce - cb, cu, tokens_[par].p, hout_.p, du_.p, sB));
  HIPCHK(inflate_mark(p));
  if (!serial) HIPCHK(hipEventRecord(sync_ev_[2 + par], sB));
  std::fill(inflated_.begin() + cb, inflated_.begin() + ce, (uint8_t)1);
  ++inflate_launches_;
  return kOk;
}

// Everything after this call on stream_ sees phase B done: stream_ waits for
// the phase Bs that ran on stream_b_ and that no later chunk waited for (the
// last two chunks').
int Pipeline::inflate_join(InflatePass& p) {
  if (p.serial) return kOk;
  const size_t nc = p.chunks.size();
  if (!p.join) HIPCHK(hipStreamWaitEvent(stream_, sync_ev_[2 + ((nc - 1) & 1)], 0));  // (with join it ran on stream_)
  if (nc >= 2) HIPCHK(hipStreamWaitEvent(stream_, sync_ev_[2 + ((nc - 2) & 1)], 0));
  return kOk;
}

// A timed pass: waits for the last event; the kernel times per launch kind.
int Pipeline::inflate_times(InflatePass& p) {
  HIPCHK(hipEventSynchronize(tev_[p.ne - 1]));
  for (size_t i = 0; i < p.ne; i += 2) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, tev_[i], tev_[i + 1]);
    const size_t k = (i / 2) % (2 * kInflateRounds + 1);  // position of the pair within its chunk
    (k == 2 * kInflateRounds ? p.lz_ms : (k & 1) ? p.huff_ms : p.tab_ms) += ms;
  }
  return kOk;
}

hipError_t Pipeline::queue_inflate_check(uint32_t b0, uint32_t b1) {
  infl_first_ = kNoBlock;
  hipError_t e = flags_.reserve(4);
  if (e != hipSuccess) return e;
  uint32_t* first = flags_.p + kFirstFailWord;
  e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), (int)kNoBlock, 1, stream_);
  if (e == hipSuccess) e = launch_first_error_hout(hout_.p, b0, b1 - b0, first, stream_);
  if (e == hipSuccess) e = rb(&infl_first_, first, 4, stream_);
  return e;
}

int Pipeline::inflate_verdict(uint32_t b0, uint32_t b1) {
  const uint32_t first = infl_first_;
  if (first == kNoBlock) return kOk;
  HuffOut ho;
  HIPCHK(rb(&ho, hout_.p + b0 + first, sizeof ho, stream_));
  HIPCHK(rb_sync(stream_));
  for (uint32_t k = b0; k < b1; ++k) inflated_[k] = 0;
  const BlockInfo& bad = hblocks_[b0 + first];
  const char* what = ho.status == kErrFormat ? "Did not inflate expected amount" : "invalid DEFLATE data";
  return fail(ho.status, std::string(what) + " in BGZF block at offset " + std::to_string(bad.coff));
}

uint32_t Pipeline::block_containing(uint64_t pos) const {
  // first block with ustart + isize > pos (non-empty block containing pos)
  uint32_t lo = 0, hi = (uint32_t)hblocks_.size();
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (hblocks_[mid].ustart + hblocks_[mid].isize > pos) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// [htsjdk] BlockCompressedInputStream.getFilePointer normalization.
uint64_t Pipeline::voff_of(uint64_t pos) const {
  const uint32_t n = (uint32_t)hblocks_.size();
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (hblocks_[mid].ustart >= pos) hi = mid; else lo = mid + 1;
  }
  if (lo < n && hblocks_[lo].ustart == pos) return hblocks_[lo].coff << 16;
  if (lo == 0) return base_ << 16;
  const BlockInfo& b = hblocks_[lo - 1];
  if (pos - b.ustart < b.isize) return (b.coff << 16) | (pos - b.ustart);
  return (b.coff + b.csize) << 16;
}

int64_t Pipeline::pos_of_voff(uint64_t voff) const {
  const uint64_t coff = voff >> 16, uoff = voff & 0xffff;
  const uint32_t n = (uint32_t)hblocks_.size();
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (hblocks_[mid].coff >= coff) hi = mid; else lo = mid + 1;
  }
  if (lo >= n) return (coff == window_end_ && uoff == 0) ? (int64_t)total_u_ : -1;
  if (hblocks_[lo].coff != coff || uoff > hblocks_[lo].isize) return -1;
  return (int64_t)(hblocks_[lo].ustart + uoff);
}

// Smallest position q with voff_of(q) >= vend (voffs increase with q).
uint64_t Pipeline::q_end_of(uint64_t vend) const {
  const uint64_t c = vend >> 16, u = vend & 0xffff;
  const uint32_t n = (uint32_t)hblocks_.size();
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (hblocks_[mid].coff >= c) hi = mid; else lo = mid + 1;
  }
  if (lo >= n) return total_u_ + 1;  // every position of the window qualifies
  const BlockInfo& b = hblocks_[lo];
  if (b.coff == c) return b.ustart + std::min<uint64_t>(u, b.isize);
  return b.ustart;
}

int Pipeline::read_stream(uint64_t pos, uint64_t len, std::vector<uint8_t>* out) {
  out->clear();
  if (pos >= total_u_) return kOk;
  len = std::min(len, total_u_ - pos);
  uint32_t b0 = block_containing(pos), b1 = block_containing(pos + len - 1) + 1;
  int rc = inflate(b0, b1);
  if (rc != kOk) return rc;
  out->resize(len);
  HIPCHK(rb(out->data(), du_.p + pos, len, stream_));
  HIPCHK(rb_sync(stream_));
  return kOk;
}

int Pipeline::decode_span(uint64_t vstart, uint64_t vend, ChainMode mode, bool decode, SpanDev* out) {
  *out = SpanDev();
  const int64_t sp = pos_of_voff(vstart);
  if (sp < 0) return fail(kErrIO, "Invalid file pointer: " + std::to_string(vstart));
  return decode_span_pos((uint64_t)sp, vend, mode, decode, out);
}

// One record pass over a span: the steps (below, in call order) share a
// SpanPass; the map of the steps and their host waits is in hbam_pipeline.h.
int Pipeline::decode_span_pos(uint64_t p0, uint64_t vend, ChainMode mode, bool decode, SpanDev* out) {
  HIPCHK(hipSetDevice(device_));
  *out = SpanDev();
  SpanPass s;
  if (!span_range(p0, vend, mode, decode, out, s)) return kOk;  // an empty span
  if (timing) HIPCHK(hipEventRecord(ev_[0], stream_));
  for (int it = 0;; ++it) {
    if (it >= kMaxChainIters) return fail(kErrState, "record chain did not converge");
    after_stop_pending_ = false;  // (only the last round's stop counts)
    int rc = span_inflate(s);
    if (rc == kOk) rc = span_scratch(s);
    if (rc == kOk) rc = span_link(s);
    if (rc == kOk) rc = s.lists ? span_check_out(s) : span_count(s);
    if (rc != kOk) return rc;
    if (!span_grow(s)) break;
  }
  int rc = s.lists ? span_status(s, out) : span_emit_walks(s, out);
  if (rc != kOk) return rc;
  out->n = s.total;
  out->rec_pos = rec_pos_.p;
  out->rec_voff = rec_voff_.p;
  if (s.dec) out->col = s.c;
  if (!s.tail_done) {  // (else done and read with k_rec_check_out's verdict; then total == bound)
    if ((rc = span_tail(s, s.total, false)) != kOk) return rc;
    if (timing) HIPCHK(hipEventRecord(ev_[2], stream_));
    HIPCHK(rb_sync(stream_));
  }
  out->next_pos = s.next;
  out->first_voff = s.voff[0];
  out->last_voff = s.voff[1];
  if (after_stop_pending_ && after_stop_flag_) ++records_after_stop_;
  after_stop_pending_ = false;
  after_stop_flag_ = 0;
  if (timing) span_times(s);
  return kOk;
}

// Range setup.  Reads the block table.  Leaves in s: mode, dec, ahead, nblk,
// [k0, k1) = the blocks that hold [p0, q_end), inf_end = the inflate's end
// (two blocks further), and the ChainArgs fields that no round changes; in
// *out: p0, q_end and next_pos = p0.  Queues nothing.  false: the span is empty.
bool Pipeline::span_range(uint64_t p0, uint64_t vend, ChainMode mode, bool decode, SpanDev* out, SpanPass& s) {
  const uint64_t q_end = q_end_of(vend);
  out->p0 = p0;
  out->q_end = q_end;
  out->next_pos = p0;
  if (p0 >= q_end || p0 >= total_u_) return false;
  s.mode = mode;
  s.dec = decode && mode == kReader;
  s.ahead = !timing;
  s.nblk = (uint32_t)hblocks_.size();
  s.k0 = block_containing(p0);
  s.k1 = std::min(s.nblk, block_containing(std::min(q_end, total_u_) - 1) + 1);
  s.inf_end = std::min(s.nblk, s.k1 + 2);
  ChainArgs& a = s.a;
  a.blocks = dblocks_.p;
  a.e_true = at_eof_ ? total_u_ : kOpenEnd;
  a.p0 = p0;
  a.q_end = q_end;
  a.dead = dead_.p;
  a.ndead = ndead_;
  a.n_ref = n_ref_;
  a.k0 = s.k0;
  a.validate = mode != kReader ? 0 : stringency_ == kStrict ? 2 : stringency_ == kLenient ? 1 : 0;
  a.ref_len = n_ref_len_ == (uint32_t)std::max(n_ref_, 0) && n_ref_len_ ? ref_len_.p : nullptr;
  return true;
}

// Reads k0, inf_end, ahead.  Queues the inflate of the blocks of [k0,
// inf_end) not inflated yet.  A timed pass checks the DEFLATE status at once
// (the host wait is inside inflate()) and adds the stage times to s.  A
// production pass queues the check's read-back and sets s.check_pending:
// the verdict lands with span_link's first read-back (one host round trip
// fewer; the chain kernels take any bytes, and their results are not used
// before the verdict).  No host wait of its own.
int Pipeline::span_inflate(SpanPass& s) {
  const int rc = inflate(s.k0, s.inf_end, s.ahead ? InflateMode::kQueued : InflateMode::kChecked);
  s.check_pending = false;
  if (rc == kOk && s.ahead && inflate_queued_) {
    HIPCHK(queue_inflate_check(s.k0, s.inf_end));
    s.check_pending = true;
  }
  if (timing) {
    s.infl_ms += times.inflate;
    s.huff_ms += times.huff;
    s.lz_ms += times.lz77;
    s.tab_ms += times.tables;
  }
  return rc;
}

// Reads k0, k1, inf_end.  Sizes the per-block scratch for nb = k1 - k0
// blocks and leaves its pointers, u, e_inf and k1 in s.a.  Queues: the zero
// of counters_' cumulative words (on its first allocation only), of need_ and
// of the per-pass counter words, then the walks (candidates + lane-per-block
// walks).  No host wait (a buffer that grows waits for the streams).
int Pipeline::span_scratch(SpanPass& s) {
  ChainArgs& a = s.a;
  a.u = du_.p;
  a.e_inf = s.inf_end < s.nblk ? hblocks_[s.inf_end].ustart : total_u_;
  a.k1 = s.k1;
  const uint32_t nb = s.k1 - s.k0;
  HIPCHK(g_.reserve(nb));
  HIPCHK(x_.reserve(nb));
  HIPCHK(x2_.reserve(nb));
  HIPCHK(entry_.reserve(nb));
  HIPCHK(summary_.reserve(4));
  HIPCHK(cnt_.reserve(nb + 1));
  HIPCHK(errv_.reserve(nb + 1));
  HIPCHK(need_.reserve(1));
  HIPCHK(rcand_.reserve(nb));
  HIPCHK(force_.reserve(nb));
  HIPCHK(wcnt_.reserve(nb));
  HIPCHK(list_.reserve((uint64_t)nb * kListCap));
  HIPCHK(base_arr_.reserve(nb + 1));
  if (!counters_.p) {  // the cumulative words (kChainCtr..) are zeroed here only
    HIPCHK(counters_.reserve(kChainCtrWords));
    HIPCHK(hipMemsetAsync(counters_.p, 0, kChainCtrWords * 4, stream_));
  }
  size_t lsb = 0;
  HIPCHK(link_scan_bytes(nb, &lsb));
  HIPCHK(scan_tmp_.reserve(lsb + 16));
  HIPCHK(fuse_.reserve(4));
  a.g = g_.p;
  a.x = x_.p;
  a.x2 = x2_.p;
  a.entry = entry_.p;
  a.summary = summary_.p;
  a.cnt = cnt_.p;
  a.err = errv_.p;
  a.need = need_.p;
  a.cand = rcand_.p;
  a.force = force_.p;
  a.wcnt = wcnt_.p;
  a.list = list_.p;
  a.counters = counters_.p;
  a.base = base_arr_.p;
  a.scan_tmp = scan_tmp_.p;
  a.scan_bytes = lsb;
  HIPCHK(hipMemsetAsync(need_.p, 0, 8, stream_));
  HIPCHK(hipMemsetAsync(counters_.p, 0, kChainCtr * 4, stream_));  // the per-pass words only
  HIPCHK(launch_chain(a, s.mode, walk_lane_ ? kStageWalkLane : kStageWalk, stream_));  // candidates + walks
  if (keep_walk_) {  // (measurement: chain_lists)
    HIPCHK(kept_g_.reserve(nb));
    HIPCHK(kept_x_.reserve(nb));
    HIPCHK(kept_wcnt_.reserve(nb));
    HIPCHK(kept_list_.reserve((uint64_t)nb * kListCap));
    HIPCHK(hipMemcpyAsync(kept_g_.p, g_.p, (size_t)nb * 8, hipMemcpyDeviceToDevice, stream_));
    HIPCHK(hipMemcpyAsync(kept_x_.p, x_.p, (size_t)nb * 8, hipMemcpyDeviceToDevice, stream_));
    HIPCHK(hipMemcpyAsync(kept_wcnt_.p, wcnt_.p, (size_t)nb * 4, hipMemcpyDeviceToDevice, stream_));
    HIPCHK(hipMemcpyAsync(kept_list_.p, list_.p, (size_t)nb * kListCap * 2, hipMemcpyDeviceToDevice, stream_));
    kept_nb_ = nb;
    kept_stage_ = walk_lane_ ? kStageWalkLane : kStageWalk;
  }
  return kOk;
}

// HBAM_CURSOR_TRACE: the blocks the link check left off the chain (waits for
// the stream).  base_arr_ holds the link's max-scan ("in") unless list_bound
// was queued behind this check round: then its scan has put the list offsets there.
void Pipeline::dump_off_chain(const SpanPass& s, bool list_offsets_in_base) {
  const uint32_t nb = s.a.k1 - s.a.k0;
  std::vector<uint64_t> fv(nb), gv(nb), xv(nb), ev(nb), inv(nb);
  (void)hipStreamSynchronize(stream_);
  (void)hipMemcpy(fv.data(), force_.p, nb * 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(gv.data(), g_.p, nb * 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(xv.data(), x_.p, nb * 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(ev.data(), entry_.p, nb * 8, hipMemcpyDeviceToHost);
  (void)hipMemcpy(inv.data(), base_arr_.p, nb * 8, hipMemcpyDeviceToHost);
  for (uint32_t i = 0, shown = 0; i < nb && shown < 8; ++i) {
    if (fv[i] == ~0ull) continue;
    const BlockInfo& b = hblocks_[s.a.k0 + i];
    fprintf(stderr, "[chain]   block %u (of %u) ustart %llu end %llu: force %llx g %llx x %llx %s %llx entry %llx\n",
            i, nb, (unsigned long long)b.ustart, (unsigned long long)(b.ustart + b.isize),
            (unsigned long long)fv[i], (unsigned long long)gv[i], (unsigned long long)xv[i],
            list_offsets_in_base ? "list offset" : "in", (unsigned long long)inv[i], (unsigned long long)ev[i]);
    ++shown;
  }
}

// The chain's end, queued as read-backs into s.end: the link max-scan's last
// entry (it must be read before list_offsets' scan overwrites base_arr_) and
// the last block's exit.
hipError_t Pipeline::chain_end(SpanPass& s) {
  const uint32_t nb = s.a.k1 - s.a.k0;
  hipError_t e = rb(&s.end[0], base_arr_.p + nb - 1, 8, stream_);
  if (e == hipSuccess) e = rb(&s.end[1], x2_.p + nb - 1, 8, stream_);
  return e;
}

// cnt_ scanned into base_arr_ (a block's output offset); the last offset and
// count, whose sum is the total, queued as read-backs into s.last_base /
// s.last_cnt.  The scan may grow scan_tmp_: s.a.scan_tmp follows it (the
// grown buffer serves the next link check too).
hipError_t Pipeline::list_offsets(SpanPass& s) {
  const uint32_t nb = s.a.k1 - s.a.k0;
  size_t tb = 0;
  hipError_t e = scan_u32_to_u64(nullptr, &tb, cnt_.p, base_arr_.p, nb, stream_);
  if (e == hipSuccess) e = scan_tmp_.reserve(tb + 16);
  s.a.scan_tmp = scan_tmp_.p;
  if (e == hipSuccess) e = scan_u32_to_u64(scan_tmp_.p, &tb, cnt_.p, base_arr_.p, nb, stream_);
  if (e == hipSuccess) e = rb(&s.last_base, base_arr_.p + nb - 1, 8, stream_);
  if (e == hipSuccess) e = rb(&s.last_cnt, cnt_.p + nb - 1, 4, stream_);
  return e;
}

// The lists' record counts (k_list_counts -> cnt_) scanned into base_arr_
// (the output offsets of k_rec_check_out; their total bounds the span's
// records) and the list overflow flag, queued as read-backs into s.last_base,
// s.last_cnt, s.ovf: they come back with the chain's end in one host round trip.
hipError_t Pipeline::list_bound(SpanPass& s) {
  hipError_t e = launch_list_counts(s.a, stream_);
  if (e == hipSuccess) e = list_offsets(s);
  if (e == hipSuccess) e = rb(&s.ovf, counters_.p + 2, 4, stream_);
  return e;
}

// The link: a max-scan of the walk exits that asks blocks off the chain to be
// re-walked, in rounds; after kMaxLinkFix rounds, or on a hard violation, the
// exact serial link.  Reads s.a, ahead, check_pending.  Queues per round the
// zero of the round's two counter words, the link check and its read-back
// (s.ctr), then a host wait.  A production pass queues behind the first round,
// as if the link holds (it does in every production pass: link_rewalks 0),
// chain_end, list_bound and the zero of k_rec_check_out's long_n_ and fuse_
// words (after the host wait only its launch remains; span_check_out skips
// them when s.ahead); a re-walk or the serial link computes end and bound
// again, with one more host wait, as does a timed pass.  The inflate's
// verdict (check_pending) is taken after the first wait.  Leaves in s: sm
// (final position, stopped), bound, ovf, lists.
int Pipeline::span_link(SpanPass& s) {
  const uint32_t nb = s.a.k1 - s.a.k0;
  bool serial = false, held = false;
  for (int fix = 0;; ++fix) {
    HIPCHK(hipMemsetAsync(counters_.p, 0, 8, stream_));
    HIPCHK(launch_chain(s.a, s.mode, kStageLinkCheck, stream_));
    ++link_rounds_;
    HIPCHK(rb(s.ctr, counters_.p, 8, stream_));
    const bool spec = fix == 0 && s.ahead;
    if (spec) {
      HIPCHK(chain_end(s));
      HIPCHK(list_bound(s));
      HIPCHK(long_n_.reserve(1));
      HIPCHK(hipMemsetAsync(long_n_.p, 0, 4, stream_));
      HIPCHK(hipMemsetAsync(fuse_.p, 0xff, 12, stream_));  // early-stop key, first failing block: none
    }
    HIPCHK(rb_sync(stream_));
    if (s.check_pending) {
      s.check_pending = false;
      if (int vr = inflate_verdict(s.k0, s.inf_end)) return vr;
    }
    const bool linked = s.ctr[0] == 0 && s.ctr[1] == 0;
    held = spec && linked;  // what was queued behind this round stands
    if (linked) break;
    serial = s.ctr[0] || fix == kMaxLinkFix;
    if (cursor_trace()) {
      if (serial)
        fprintf(stderr, "[chain] serial link: blocks [%u, %u) e_inf %llu e_true %llu p0 %llu rewalk round %d, "
                "%u blocks off the chain, serial request %u\n", s.a.k0, s.a.k1, (unsigned long long)s.a.e_inf,
                (unsigned long long)s.a.e_true, (unsigned long long)s.a.p0, fix, s.ctr[1], s.ctr[0]);
      else
        fprintf(stderr, "[chain] rewalk round %d: %u blocks off the chain\n", fix, s.ctr[1]);
      dump_off_chain(s, spec);
    }
    if (serial) break;
    ++link_rewalks_;
    HIPCHK(launch_chain(s.a, s.mode, kStageRewalk, stream_));
  }
  if (serial) {  // exact serial link (writes entry[] + summary), then lists off entry[]
    ++link_fallbacks_;
    HIPCHK(launch_chain(s.a, s.mode, kStageSerialLink, stream_));
    HIPCHK(launch_chain(s.a, s.mode, kStageRewalkAll, stream_));
    HIPCHK(rb(s.sm, summary_.p, 16, stream_));
    HIPCHK(list_bound(s));
    HIPCHK(rb_sync(stream_));
  } else {  // final chain position = max of every walk exit; no stop
    if (!held) {
      HIPCHK(chain_end(s));
      HIPCHK(list_bound(s));
      HIPCHK(rb_sync(stream_));
    }
    s.sm[0] = nb == 1 ? s.end[1] : std::max(s.end[0], s.end[1]);
    s.sm[1] = 0;
  }
  s.bound = s.last_base + s.last_cnt;
  // a list overflowed (indexer mode: records shorter than 36 bytes): the
  // per-block walks count and emit the records instead (k_rec_count, k_rec_emit)
  s.lists = s.ovf == 0;
  if (!s.lists) ++record_fallbacks_;
  return kOk;
}

// The list path.  Reads s.a, bound, dec, ahead.  Sizes the outputs by the
// lists' records, then queues check + positions + voffs + fields + keys in
// one launch (k_rec_check_out), each block at its scanned list offset; a
// production pass queues the span's tail behind it, gated on its verdict
// (span_tail), and skips the zero of long_n_ and fuse_ that span_link queued.
// One host wait reads need, bad, fl (and the tail).  Leaves total, first,
// tail_done; when a block stopped the span, the records-after-stop flag is
// queued too and lands with the span's last read-back.
int Pipeline::span_check_out(SpanPass& s) {
  ChainArgs& a = s.a;
  HIPCHK(rec_pos_.reserve(s.bound + 1));
  HIPCHK(rec_voff_.reserve(s.bound + 1));
  if (s.dec) {
    const int rc = alloc_columns(s.bound, total_u_, &s.c, !s.ahead);
    if (rc != kOk) return rc;
  }
  if (!s.ahead) HIPCHK(hipMemsetAsync(fuse_.p, 0xff, 12, stream_));  // early-stop key, first failing block: none
  a.fuse_bad = reinterpret_cast<uint64_t*>(fuse_.p);
  a.fuse_flags = fuse_.p + 2;
  a.rec_pos = rec_pos_.p;
  a.rec_voff = rec_voff_.p;
  if (timing) HIPCHK(hipEventRecord(ev_[1], stream_));
  HIPCHK(launch_rec_check_out(a, s.mode, s.dec, s.c, s.bound + 1, stream_));
  if (s.ahead)
    if (int rc = span_tail(s, s.bound, true)) return rc;
  HIPCHK(rb(&s.need, need_.p, 8, stream_));
  HIPCHK(rb(&s.bad, fuse_.p, 8, stream_));
  HIPCHK(rb(s.fl, fuse_.p + 2, 4, stream_));
  HIPCHK(rb_sync(stream_));
  s.tail_done = s.ahead && s.bad == ~0ull && s.need <= a.e_inf;
  s.first = s.fl[0];
  s.total = s.bound;  // every block kept its whole list
  if (s.bad != ~0ull) {
    // the span ends at the first block that stops: its records stand at
    // their final offsets, later blocks' records lie past them and are
    // dropped, and that block's status (if any) is the span's -- a
    // failure in a later block is never reached (k_rec_check_out)
    const uint64_t k = s.bad >> kFusedBadShift;
    s.total = s.bad & ((1ull << kFusedBadShift) - 1);
    if (s.fl[0] != k) s.first = kNoBlock;
    // (diagnostic) records listed after the stop, which it drops: read
    // with the span's last readback, no round trip of its own
    HIPCHK(hipMemsetAsync(fuse_.p + 3, 0, 4, stream_));
    HIPCHK(launch_records_after(cnt_.p, a.k1 - a.k0, (uint32_t)k, fuse_.p + 3, stream_));
    HIPCHK(rb(&after_stop_flag_, fuse_.p + 3, 4, stream_));
    after_stop_pending_ = true;
  }
  return kOk;
}

// The walk path (a list overflowed).  Queues the count + validation by
// walking (k_rec_count) and the read-back of need; one host wait.
int Pipeline::span_count(SpanPass& s) {
  s.tail_done = false;
  HIPCHK(launch_chain(s.a, s.mode, kStageCount, stream_));
  HIPCHK(rb(&s.need, need_.p, 8, stream_));
  HIPCHK(rb_sync(stream_));
  return kOk;
}

// Go round again?  Reads need, sm, s.a.e_inf / q_end and the block table;
// changes only k1 and inf_end.  Queues nothing.
bool Pipeline::span_grow(SpanPass& s) {
  const uint64_t final_pos = s.sm[0], e_inf = s.a.e_inf, q_end = s.a.q_end;
  const bool stopped = s.sm[1] != 0;
  const uint32_t nblk = s.nblk;
  if (s.need > e_inf && s.inf_end < nblk) {  // a record needs bytes beyond the inflated range
    s.inf_end = std::min(nblk, block_containing(std::min<uint64_t>(s.need, total_u_) - 1) + 2);
    return true;
  }
  if (stopped && final_pos + 36 > e_inf && s.inf_end < nblk) {  // the chain stopped for want of bytes
    s.inf_end = std::min(nblk, s.inf_end + 4);
    return true;
  }
  if (!stopped && final_pos < q_end && final_pos < total_u_ && s.k1 < nblk && final_pos >= hblocks_[s.k1].ustart) {
    // the chain runs on inside the span past block k1 - 1: take the blocks up to its end
    s.k1 = std::min(nblk, block_containing(std::min(final_pos, q_end - 1)) + 1);
    s.inf_end = std::max(s.inf_end, std::min(nblk, s.k1 + 2));
    return true;
  }
  return false;
}

// The first failing block (s.first; none: nothing to do): records before it
// stand, later blocks are dropped.  Queues the read-back of its status
// (s.code); one host wait.  Unless the block stopped cleanly, leaves the
// status and its text in *out.
int Pipeline::span_status(SpanPass& s, SpanDev* out) {
  if (s.first == kNoBlock) return kOk;
  HIPCHK(rb(&s.code, errv_.p + s.first, 4, stream_));
  HIPCHK(rb_sync(stream_));
  if (s.code == kStopClean) return kOk;
  out->status = s.code;
  const BlockInfo& b = hblocks_[s.k0 + s.first];
  const char* what = s.code == kErrFormat ? "Invalid record (SAMFormatException)"
                     : s.code == kErrTrunc ? "Premature EOF in BAM record"
                     : s.code == kErrArg   ? "Reference index not found in sequence dictionary"
                                           : "Invalid alignment";
  out->error = std::string(what) + " (BGZF block at offset " + std::to_string(b.coff) + ")";
  return kOk;
}

// The walk path's output (a block listed more starts than kListCap), after
// the last span_count.  Queues the first failing block's search and read-back
// (a host wait), span_status (one more if there is one), the cut of the
// counts at that block -- the first block that stops, with or without an
// error: the iteration ends there --, list_offsets (a host wait: s.total),
// then the per-block walks that emit positions + voffs (k_rec_emit) and
// k_rec_decode.  Leaves first, code, total, c and the outputs' pointers in s.a.
int Pipeline::span_emit_walks(SpanPass& s, SpanDev* out) {
  ChainArgs& a = s.a;
  const uint32_t nb = a.k1 - a.k0;
  uint32_t* first = flags_.p + kFirstFailWord;
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(first), (int)kNoBlock, 1, stream_));
  HIPCHK(launch_first_error_i32(errv_.p, nb, first, stream_));
  HIPCHK(rb(&s.first, first, 4, stream_));
  HIPCHK(rb_sync(stream_));
  if (int rc = span_status(s, out)) return rc;
  if (s.first != kNoBlock) HIPCHK(launch_truncate_counts(cnt_.p, nb, first, stream_));
  HIPCHK(list_offsets(s));
  HIPCHK(rb_sync(stream_));
  s.total = s.last_base + s.last_cnt;
  HIPCHK(rec_pos_.reserve(s.total + 1));
  HIPCHK(rec_voff_.reserve(s.total + 1));
  a.rec_pos = rec_pos_.p;
  a.rec_voff = rec_voff_.p;
  if (s.dec) {
    const int rc = alloc_columns(s.total, total_u_, &s.c);
    if (rc != kOk) return rc;
  }
  HIPCHK(launch_chain(a, s.mode, kStageEmit, stream_));
  if (timing) HIPCHK(hipEventRecord(ev_[1], stream_));
  if (s.dec) HIPCHK(launch_rec_decode(du_.p, rec_pos_.p, s.total, s.c, stream_));
  return kOk;
}

// The span's tail over its n records.  Queues the deferred long keys
// (k_long_hash, when dec), the next record's start -- the chain successor of
// the last record (k_next_pos) -- and the read-backs of it and of the first
// and last voff into s.next, s.voff.  gated: queued behind k_rec_check_out
// before its verdict is known; the two kernels do nothing unless it found no
// stop and no record needs bytes past e_inf, and the words read are stale
// then (unused: tail_done stays false).  No host wait: the caller's follows.
int Pipeline::span_tail(SpanPass& s, uint64_t n, bool gated) {
  const unsigned long long* gate_bad = gated ? reinterpret_cast<const unsigned long long*>(fuse_.p) : nullptr;
  const unsigned long long* gate_need = gated ? need_.p : nullptr;
  const uint64_t gate_e_inf = gated ? s.a.e_inf : 0;
  s.voff[0] = s.voff[1] = 0;
  if (s.dec) HIPCHK(launch_long_hash(du_.p, rec_pos_.p, s.c, stream_, gate_bad, gate_need, gate_e_inf));
  HIPCHK(scalars_.reserve(8));
  HIPCHK(launch_next_pos(du_.p, rec_pos_.p, n, s.a.p0, s.mode, scalars_.p, stream_, gate_bad, gate_need, gate_e_inf));
  HIPCHK(rb(&s.next, scalars_.p, 8, stream_));
  if (n) {
    HIPCHK(rb(&s.voff[0], rec_voff_.p, 8, stream_));
    HIPCHK(rb(&s.voff[1], rec_voff_.p + n - 1, 8, stream_));
  }
  return kOk;
}

// A timed pass's stage times, from the events the steps recorded (ev_[0]
// the pass's start, [1] before the check-out or decode, [2] its end) and the
// inflates' sums in s.
void Pipeline::span_times(const SpanPass& s) {
  float all = 0, dcd = 0;
  (void)hipEventElapsedTime(&all, ev_[0], ev_[1]);
  (void)hipEventElapsedTime(&dcd, ev_[1], ev_[2]);
  times.chain = all - s.infl_ms;
  times.decode = dcd;
  times.inflate = s.infl_ms;
  times.huff = s.huff_ms;
  times.lz77 = s.lz_ms;
  times.tables = s.tab_ms;
}

int Pipeline::alloc_columns(uint64_t total, uint64_t stream_bytes, Columns* cp, bool zero_long_n) {
  // SoA backing store: 8-byte columns first, then 4, 2, 1 (alignment)
  const uint64_t n = std::max<uint64_t>(total, 1);
  const uint64_t per = 8 * 2 + 4 * 7 + 2 * 3 + 1 * 2;
  if (cols_cap_ < n) {
    HIPCHK(cols_.reserve(n * per + 256));
    cols_cap_ = n;
  }
  HIPCHK(rec_voff_.reserve(n + 1));
  uint8_t* p = cols_.p;
  Columns& c = *cp;
  c.key = reinterpret_cast<int64_t*>(take16(&p, 8 * n));
  c.rest_off = reinterpret_cast<uint64_t*>(take16(&p, 8 * n));
  c.voff = rec_voff_.p;
  c.ref_id = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.pos = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.l_seq = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.next_ref_id = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.next_pos = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.tlen = reinterpret_cast<int32_t*>(take16(&p, 4 * n));
  c.rest_len = reinterpret_cast<uint32_t*>(take16(&p, 4 * n));
  c.bin = reinterpret_cast<uint16_t*>(take16(&p, 2 * n));
  c.n_cigar = reinterpret_cast<uint16_t*>(take16(&p, 2 * n));
  c.flag = reinterpret_cast<uint16_t*>(take16(&p, 2 * n));
  c.l_read_name = take16(&p, n);
  c.mapq = take16(&p, n);
  // deferred long-record keys: at most one per kLongHash stream bytes
  const uint64_t cap = std::min<uint64_t>(stream_bytes / kLongHash + 64, 0xffffffffull);
  HIPCHK(long_rec_.reserve(cap));
  HIPCHK(long_n_.reserve(1));
  if (zero_long_n) HIPCHK(hipMemsetAsync(long_n_.p, 0, 4, stream_));
  c.long_rec = long_rec_.p;
  c.long_n = long_n_.p;
  c.long_cap = (uint32_t)cap;
  return kOk;
}

int Pipeline::encoded_bytes(const SpanDev& s, uint64_t* bytes) {
  *bytes = 0;
  if (s.n == 0) return kOk;
  if (!s.col.rest_off) return fail(kErrState, "span was not decoded in reader mode");
  uint64_t first = 0, last_off = 0;
  uint32_t last_len = 0;
  HIPCHK(rb(&first, s.rec_pos, 8, stream_));
  HIPCHK(rb(&last_off, s.col.rest_off + (s.n - 1), 8, stream_));
  HIPCHK(rb(&last_len, s.col.rest_len + (s.n - 1), 4, stream_));
  HIPCHK(rb_sync(stream_));
  *bytes = last_off + last_len - first;
  return kOk;
}

int Pipeline::encode_writables(const SpanDev& s, uint64_t bytes, uint8_t* dst) {
  if (s.n == 0) return kOk;
  if (!s.col.ref_id) return fail(kErrState, "span was not decoded in reader mode");
  uint64_t first = 0;
  HIPCHK(rb(&first, s.rec_pos, 8, stream_));
  HIPCHK(rb_sync(stream_));
  const uint8_t* src = s.data ? s.data : du_.p;
  HIPCHK(launch_wr_encode(src, first, bytes, s.rec_pos, s.col.ref_id, s.col.bin, s.n, dst, stream_));
  return kOk;
}

int Pipeline::sort_writables(const SpanDev& s, int order, uint64_t bytes, uint8_t* dst, float* ms) {
  if (ms) ms[0] = ms[1] = ms[2] = 0;
  if (s.n == 0) return kOk;
  if (!s.col.ref_id || !s.col.key) return fail(kErrState, "span was not decoded in reader mode");
  if (order != kSortKey && order != kSortCoordinate && order != kSortQueryname)
    return fail(kErrArg, "unknown sort order");
  if (s.n >= 0x7fffffffull) return fail(kErrArg, "too many records to sort in one batch");
  HIPCHK(hipSetDevice(device_));
  const uint64_t n = s.n;
  size_t tmp = 0;
  HIPCHK(sort_tmp_bytes(n, &tmp));
  HIPCHK(sort_tmp_.reserve(tmp));
  HIPCHK(sort_word_.reserve(n));
  HIPCHK(sort_word2_.reserve(n));
  HIPCHK(sort_len_.reserve(n));
  HIPCHK(sort_iota_.reserve(n));
  HIPCHK(sort_perm_.reserve(n));
  HIPCHK(sort_slen_.reserve(n + 1));
  HIPCHK(sort_doff_.reserve(n + 1));
  const uint8_t* src = s.data ? s.data : du_.p;
  if (ms) HIPCHK(hipEventRecord(ev_[4], stream_));
  if (order == kSortQueryname) {
    HIPCHK(name_pos_.reserve(n));
    HIPCHK(name_len_.reserve(n));
    HIPCHK(name_tie_.reserve(n));
    HIPCHK(launch_name_refs(s.rec_pos, s.col, n, name_pos_.p, name_len_.p, name_tie_.p, sort_len_.p, stream_));
    const int rc = name_order(sort_tmp_.p, tmp, src, name_pos_.p, name_len_.p, name_tie_.p, n, sort_word_.p,
                              sort_word2_.p, sort_iota_.p, sort_perm_.p, ms != nullptr);
    if (rc != kOk) return rc;
  } else {
    HIPCHK(launch_sort_perm(sort_tmp_.p, tmp, s.col, n, order, sort_word_.p, sort_word2_.p, sort_len_.p, sort_iota_.p,
                            sort_perm_.p, stream_));
  }
  if (ms) HIPCHK(hipEventRecord(ev_[5], stream_));
  HIPCHK(launch_sort_offsets(sort_tmp_.p, tmp, sort_len_.p, sort_perm_.p, n, sort_slen_.p, sort_doff_.p, stream_));
  if (ms) HIPCHK(hipEventRecord(ev_[6], stream_));
  HIPCHK(launch_sort_gather(src, s.rec_pos, s.col.ref_id, sort_perm_.p, sort_doff_.p, n, bytes, dst, stream_));
  if (ms) {
    HIPCHK(hipEventRecord(ev_[7], stream_));
    HIPCHK(hipEventSynchronize(ev_[7]));
    for (int k = 0; k < 3; ++k) HIPCHK(hipEventElapsedTime(&ms[k], ev_[4 + k], ev_[5 + k]));
    if (order == kSortQueryname) {
      HIPCHK(hipEventElapsedTime(&name_ms_[0], ev_[4], ev_[0]));
      HIPCHK(hipEventElapsedTime(&name_ms_[1], ev_[0], ev_[1]));
      HIPCHK(hipEventElapsedTime(&name_ms_[2], ev_[1], ev_[5]));
    }
  }
  return kOk;
}

// a device allocation of the SAM text path: its failure is kErrNoMem
#define SAMALLOC(expr)                                                        \
  do {                                                                        \
    if ((expr) != hipSuccess) return fail(kErrNoMem, "device allocation failed: " #expr); \
  } while (0)

int Pipeline::set_sam_refs(const std::vector<std::string>& names) {
  if (sam_n_ref_ >= 0) return kOk;
  HIPCHK(hipSetDevice(device_));
  std::vector<uint32_t> off(names.size() + 1, 0);
  std::string bytes;
  for (size_t i = 0; i < names.size(); ++i) {
    bytes += names[i];
    if (bytes.size() > 0xffffffffull) return fail(kErrArg, "reference names longer than 4 GiB");
    off[i + 1] = (uint32_t)bytes.size();
  }
  own(sam_ref_off_, sam_ref_bytes_, sam_head_, sam_tmp_, sam_llen_, sam_doff_, sam_bad_);
  SAMALLOC(sam_ref_off_.reserve(off.size()));
  SAMALLOC(sam_ref_bytes_.reserve(bytes.size() + 1));
  HIPCHK(hipMemcpyAsync(sam_ref_off_.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, stream_));
  if (!bytes.empty())
    HIPCHK(hipMemcpyAsync(sam_ref_bytes_.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, stream_));
  HIPCHK(hipStreamSynchronize(stream_));  // (the host vectors go away)
  sam_n_ref_ = (int32_t)names.size();
  return kOk;
}

int Pipeline::sam_measure(const SpanDev& s, uint64_t* bytes, uint64_t* bad, float* ms2) {
  *bytes = 0;
  *bad = ~0ull;
  if (ms2) ms2[0] = ms2[1] = 0;
  if (s.n == 0) return kOk;
  if (!s.col.ref_id || !s.col.rest_len) return fail(kErrState, "span was not decoded in reader mode");
  if (sam_n_ref_ < 0) return fail(kErrState, "no reference names set");
  if (s.n >= 0x7fffffffull) return fail(kErrArg, "too many records to format in one batch");
  HIPCHK(hipSetDevice(device_));
  const uint64_t n = s.n;
  size_t tmp = 0;
  HIPCHK(sam_tmp_bytes(n, &tmp));
  SAMALLOC(sam_tmp_.reserve(tmp));
  SAMALLOC(sam_head_.reserve(n));
  SAMALLOC(sam_llen_.reserve(n + 1));
  SAMALLOC(sam_doff_.reserve(n + 1));
  SAMALLOC(sam_bad_.reserve(1));
  const uint8_t* src = s.data ? s.data : du_.p;
  HIPCHK(hipMemsetAsync(sam_bad_.p, 0xff, sizeof(unsigned long long), stream_));
  if (ms2) HIPCHK(hipEventRecord(ev_[4], stream_));
  HIPCHK(launch_sam_measure(src, s.rec_pos, s.col, n, sam_ref_off_.p, sam_ref_bytes_.p, sam_n_ref_, sam_head_.p,
                            sam_llen_.p, sam_bad_.p, stream_));
  if (ms2) HIPCHK(hipEventRecord(ev_[5], stream_));
  HIPCHK(launch_sam_offsets(sam_tmp_.p, tmp, sam_llen_.p, n, sam_doff_.p, stream_));
  if (ms2) HIPCHK(hipEventRecord(ev_[6], stream_));
  unsigned long long b = ~0ull;
  HIPCHK(rb(&b, sam_bad_.p, sizeof b, stream_));
  HIPCHK(rb(bytes, sam_doff_.p + n, 8, stream_));
  HIPCHK(rb_sync(stream_));
  *bad = b;
  if (ms2) {
    HIPCHK(hipEventElapsedTime(&ms2[0], ev_[4], ev_[5]));
    HIPCHK(hipEventElapsedTime(&ms2[1], ev_[5], ev_[6]));
  }
  return kOk;
}

int Pipeline::sam_write(const SpanDev& s, uint64_t bytes, uint8_t* dst, float* ms1) {
  if (ms1) *ms1 = 0;
  if (s.n == 0 || bytes == 0) return kOk;
  if (!s.col.ref_id || sam_n_ref_ < 0) return fail(kErrState, "span was not measured");
  HIPCHK(hipSetDevice(device_));
  const uint8_t* src = s.data ? s.data : du_.p;
  if (ms1) HIPCHK(hipEventRecord(ev_[6], stream_));
  HIPCHK(launch_sam_write(src, s.rec_pos, s.col, s.n, sam_ref_off_.p, sam_ref_bytes_.p, sam_n_ref_, sam_head_.p,
                          sam_doff_.p, bytes, dst, stream_));
  if (ms1) {
    HIPCHK(hipEventRecord(ev_[7], stream_));
    HIPCHK(hipEventSynchronize(ev_[7]));
    HIPCHK(hipEventElapsedTime(ms1, ev_[6], ev_[7]));
  }
  return kOk;
}

int Pipeline::samp_set_dict(const std::vector<std::string>& names) {
  HIPCHK(hipSetDevice(device_));
  // sorted as unsigned bytes (std::string's order), equal names by index: the first of a run stays
  std::vector<int32_t> order(names.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return names[a] < names[b]; });
  std::vector<uint32_t> off(1, 0);
  std::vector<int32_t> idx;
  std::string bytes;
  for (size_t k = 0; k < order.size(); ++k) {
    if (k && names[order[k]] == names[order[k - 1]]) continue;
    bytes += names[order[k]];
    if (bytes.size() > 0xffffffffull) return fail(kErrArg, "reference names longer than 4 GiB");
    off.push_back((uint32_t)bytes.size());
    idx.push_back(order[k]);
  }
  own(samp_text_, samp_tmp_, samp_rec_, samp_dict_bytes_, samp_cnt_, samp_first_, samp_start_, samp_rlen_,
      samp_roff_, samp_bad_, samp_dict_off_, samp_dict_idx_);
  SAMALLOC(samp_dict_off_.reserve(off.size()));
  SAMALLOC(samp_dict_idx_.reserve(idx.size() + 1));
  SAMALLOC(samp_dict_bytes_.reserve(bytes.size() + 1));
  HIPCHK(hipMemcpyAsync(samp_dict_off_.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, stream_));
  if (!idx.empty()) {
    HIPCHK(hipMemcpyAsync(samp_dict_idx_.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, stream_));
    if (!bytes.empty())
      HIPCHK(hipMemcpyAsync(samp_dict_bytes_.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, stream_));
  }
  HIPCHK(hipStreamSynchronize(stream_));  // (the host vectors go away)
  samp_dict_n_ = (int32_t)idx.size();
  return kOk;
}

int Pipeline::samp_lines(const uint8_t* text, uint64_t len, bool final, uint64_t* n, uint64_t* consumed) {
  *n = *consumed = 0;
  for (float& m : samp_ms_) m = 0;
  samp_len_ = 0;
  if (samp_dict_n_ < 0) return fail(kErrState, "no dictionary set");
  // what is parsed: through the last '\n'; a final text's last line gets the '\n' it lacks
  uint64_t use = len;
  while (use && text[use - 1] != '\n') --use;
  const bool add = final && use < len;
  if (add) use = len;
  *consumed = use;
  const uint64_t dlen = use + (add ? 1 : 0);
  if (dlen == 0) return kOk;
  HIPCHK(hipSetDevice(device_));
  const uint64_t np = samp_pieces(dlen);
  // zero behind the text to the end of its last piece: the aligned 16-byte loads read there
  SAMALLOC(samp_text_.reserve(np * 4096 + 64));
  SAMALLOC(samp_cnt_.reserve(np + 1));
  SAMALLOC(samp_first_.reserve(np + 1));
  SAMALLOC(samp_bad_.reserve(1));
  size_t tmp = 0;
  HIPCHK(samp_scan_bytes(np + 1, &tmp));
  SAMALLOC(samp_tmp_.reserve(tmp));
  HIPCHK(hipMemcpyAsync(samp_text_.p, text, use, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipMemsetAsync(samp_text_.p + use, 0, np * 4096 + 64 - use, stream_));
  if (add) HIPCHK(hipMemsetAsync(samp_text_.p + use, '\n', 1, stream_));
  HIPCHK(hipEventRecord(ev_[0], stream_));
  HIPCHK(launch_samp_count(samp_text_.p, dlen, samp_cnt_.p, stream_));
  HIPCHK(launch_samp_scan(samp_tmp_.p, tmp, samp_cnt_.p, np + 1, samp_first_.p, stream_));
  uint64_t lines = 0;
  HIPCHK(rb(&lines, samp_first_.p + np, 8, stream_));
  HIPCHK(rb_sync(stream_));
  if (lines >= 0x7fffffffull) return fail(kErrArg, "too many lines to parse in one call");
  SAMALLOC(samp_start_.reserve(lines + 1));
  HIPCHK(launch_samp_starts(samp_text_.p, dlen, samp_first_.p, samp_start_.p, stream_));
  HIPCHK(hipEventRecord(ev_[1], stream_));
  samp_len_ = dlen;
  *n = lines;
  return kOk;
}

int Pipeline::samp_measure(uint64_t n, uint64_t* bytes, uint64_t* bad) {
  *bytes = 0;
  *bad = ~0ull;
  if (n == 0) return kOk;
  if (samp_len_ == 0 || samp_dict_n_ < 0) return fail(kErrState, "no text was split into lines");
  HIPCHK(hipSetDevice(device_));
  size_t tmp = 0;
  HIPCHK(samp_scan_bytes(n + 1, &tmp));
  SAMALLOC(samp_tmp_.reserve(tmp));
  SAMALLOC(samp_rlen_.reserve(n + 1));
  SAMALLOC(samp_roff_.reserve(n + 1));
  HIPCHK(hipMemsetAsync(samp_bad_.p, 0xff, sizeof(unsigned long long), stream_));
  HIPCHK(hipEventRecord(ev_[2], stream_));
  HIPCHK(launch_samp_measure(samp_text_.p, samp_start_.p, n, samp_dict_off_.p, samp_dict_bytes_.p, samp_dict_idx_.p,
                             samp_dict_n_, samp_rlen_.p, samp_bad_.p, stream_));
  HIPCHK(hipEventRecord(ev_[3], stream_));
  HIPCHK(launch_samp_scan(samp_tmp_.p, tmp, samp_rlen_.p, n + 1, samp_roff_.p, stream_));
  HIPCHK(hipEventRecord(ev_[4], stream_));
  unsigned long long b = ~0ull;
  HIPCHK(rb(&b, samp_bad_.p, sizeof b, stream_));
  HIPCHK(rb(bytes, samp_roff_.p + n, 8, stream_));
  HIPCHK(rb_sync(stream_));
  *bad = b;
  return kOk;
}

int Pipeline::samp_write(uint64_t n, uint64_t bytes) {
  samp_enc_.clear();  // (nothing to keep when the tables grow)
  samp_offs_.clear();
  if (samp_offs_.resize(n + 1) != hipSuccess || samp_enc_.resize(bytes ? bytes : 1) != hipSuccess)
    return fail(kErrNoMem, "page-locked memory for the parsed records");
  samp_offs_[0] = 0;
  if (n == 0) return kOk;
  HIPCHK(hipSetDevice(device_));
  SAMALLOC(samp_rec_.reserve(bytes + 16));
  HIPCHK(hipEventRecord(ev_[5], stream_));
  HIPCHK(launch_samp_write(samp_text_.p, samp_start_.p, n, samp_dict_off_.p, samp_dict_bytes_.p, samp_dict_idx_.p,
                           samp_dict_n_, samp_roff_.p, samp_rec_.p, stream_));
  HIPCHK(hipEventRecord(ev_[6], stream_));
  HIPCHK(hipMemcpyAsync(samp_enc_.data(), samp_rec_.p, bytes, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipMemcpyAsync(samp_offs_.data(), samp_roff_.p, (n + 1) * 8, hipMemcpyDeviceToHost, stream_));
  HIPCHK(hipStreamSynchronize(stream_));
  HIPCHK(hipEventElapsedTime(&samp_ms_[0], ev_[0], ev_[1]));
  HIPCHK(hipEventElapsedTime(&samp_ms_[1], ev_[2], ev_[3]));
  HIPCHK(hipEventElapsedTime(&samp_ms_[2], ev_[3], ev_[4]));
  HIPCHK(hipEventElapsedTime(&samp_ms_[3], ev_[5], ev_[6]));
  return kOk;
}

namespace {
hipError_t name_readback(void* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
  Pipeline* p = static_cast<Pipeline*>(ctx);
  const hipError_t e = p->rb(dst, src, bytes, s);
  return e != hipSuccess ? e : p->rb_sync(s);
}
}  // namespace

int Pipeline::name_order(void* tmp, size_t tmp_bytes, const uint8_t* base, const uint64_t* name_pos,
                         const uint8_t* name_len, const uint8_t* tie, uint64_t n, uint64_t* word, uint64_t* word2,
                         uint32_t* scratch, uint32_t* perm, bool timed) {
  HIPCHK(name_census_.reserve(kNameCensusWords));
  NameOrderStats st;
  HIPCHK(launch_name_order(tmp, tmp_bytes, base, name_pos, name_len, tie, n, word, word2, scratch, perm,
                           name_census_.p, name_readback, this, &st, stream_, name_full_, timed ? ev_[0] : nullptr,
                           timed ? ev_[1] : nullptr));
  name_counters_[0] = st.chunks_present;
  name_counters_[1] = st.chunks_sorted;
  name_counters_[2] = st.bits_sorted;
  return kOk;
}

int Pipeline::decode_writables(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n, SpanDev* out) {
  *out = SpanDev();
  // 64 zero bytes after the values: the 8-byte field loads and Murmur's tail
  // loads may read past the last value
  HIPCHK(wbuf_.reserve(len + 64));
  HIPCHK(woffs_.reserve(n + 1));
  HIPCHK(wbad_.reserve(1));
  HIPCHK(rec_pos_.reserve(n + 1));
  if (len) HIPCHK(hipMemcpyAsync(wbuf_.p, buf, len, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipMemsetAsync(wbuf_.p + len, 0, 64, stream_));
  if (n) HIPCHK(hipMemcpyAsync(woffs_.p, offs, n * 8, hipMemcpyHostToDevice, stream_));
  HIPCHK(hipMemsetAsync(wbad_.p, 0xff, sizeof(unsigned long long), stream_));
  Columns c{};
  int rc = alloc_columns(n, len, &c);
  if (rc != kOk) return rc;
  HIPCHK(launch_wr_decode(wbuf_.p, len, woffs_.p, n, c, rec_pos_.p, wbad_.p, stream_));
  HIPCHK(launch_long_hash(wbuf_.p, rec_pos_.p, c, stream_));
  unsigned long long bad = ~0ull;
  HIPCHK(rb(&bad, wbad_.p, sizeof bad, stream_));
  HIPCHK(rb_sync(stream_));
  out->n = n;
  if (bad != ~0ull) {
    out->n = bad >> 8;
    out->status = (int)(bad & 0xff);
    const std::string at = "value " + std::to_string(out->n);
    if (out->status == kErrFormat) out->error = "Invalid record length (" + at + ")";
    else if (out->status == kErrTrunc) out->error = "Premature EOF in serialized record (" + at + ")";
    else out->error = "value framing outside the buffer (" + at + ")";
  }
  out->p0 = 0;
  out->rec_pos = rec_pos_.p;
  out->rec_voff = rec_voff_.p;
  out->col = c;
  out->data = wbuf_.p;
  return kOk;
}

int Pipeline::splitting_entries(const SpanDev& span, uint32_t g, uint64_t o0, std::vector<uint64_t>* out) {
  out->clear();
  // global ordinals o0 .. o0+n-1; entries at ordinals k*g - 1
  const uint64_t m = (o0 + span.n) / g - o0 / g;
  if (m == 0) return kOk;
  DevBuf<uint64_t> ent(&streams_);
  HIPCHK(ent.reserve(m));
  HIPCHK(launch_sbi_emit(span.rec_voff, span.n, g, o0, ent.p, stream_));
  out->resize(m);
  HIPCHK(rb(out->data(), ent.p, m * 8, stream_));
  HIPCHK(rb_sync(stream_));
  return kOk;
}

int Pipeline::span_digest(const SpanDev& span, uint64_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (span.n == 0) return kOk;
  HIPCHK(scalars_.reserve(8));
  HIPCHK(hipMemsetAsync(scalars_.p + 2, 0, 32, stream_));
  HIPCHK(launch_digest(span.col.key, span.rec_voff, span.n, scalars_.p + 2, stream_));
  HIPCHK(rb(out, scalars_.p + 2, 32, stream_));
  HIPCHK(rb_sync(stream_));
  return kOk;
}

}  // namespace hbam
