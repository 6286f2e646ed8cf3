// hbam_abi.cpp -- extern "C" boundary (include/hbam.h) over the C++ mirror:
// the product API, everything on hbam_ctx and the calls that take no handle.
// The device-resident decode (hbam_gpu) is hbam_abi_gpu.cpp.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <memory>

#include "hbam_abi_util.h"
#include "hbam_deflate_api.h"
#include "hbam_mem.h"
#include "hbam_launch.h"
#include "hbam_merge.h"

using namespace hbam_abi;
using hadoop_bam::BAMInputFormat;
using hadoop_bam::BAMRecordReader;
using hadoop_bam::FileSplit;
using hadoop_bam::FileVirtualSplit;
using hadoop_bam::HostBatch;
using hadoop_bam::OpenOptions;
using hadoop_bam::QueryCursor;
using hadoop_bam::SpanCursor;
using hadoop_bam::SplittingBAMIndexer;

// Where the ctx's last batch came from: what hbam_encode_writables,
// hbam_sort_writables, hbam_format_sam and hbam_reader_position may serve.
//   kNone       no batch (a fresh ctx), or the span batch was forgotten
//   kSpan       hbam_decode_span handed it out (its result may still be an error or several windows:
//               the cursor knows)
//   kQuery      hbam_query_next handed it out
//   kWritables  hbam_decode_writables handed it out
// The one transition besides those three calls: a call that moves the ctx's
// window (reset_cursors: hbam_file_stats, hbam_prefetch, hbam_query_intervals,
// hbam_decode_span_device, the index, guess and split calls, ...) takes kSpan
// to kNone.  kQuery and kWritables stay until the next of the three calls.
enum class LastBatch { kNone, kSpan, kQuery, kWritables };

struct hbam_ctx {
  std::unique_ptr<BamFile> f;
  std::unique_ptr<hbam::Pipeline> codec;  // hbam_open_codec: a pipeline with no file
  std::string err;
  SpanCursor cursor;    // (destroyed before f: it drains its copies on f's pipeline stream)
  HostBatch wbatch;     // the columns of the last hbam_decode_writables
  hadoop_bam::BatchView batch;  // the last batch handed out (cursor slots or wbatch)
  hbam::SpanDev wspan;  // device result of the last hbam_decode_writables
  LastBatch last = LastBatch::kNone;
  // hbam_parse_sam's dictionary on the pipeline: none uploaded yet (the next parse uploads the file's, or an
  // empty one on a codec ctx), the file's, or the caller's (hbam_parse_sam_dict)
  enum class SamDict { kUnset, kFile, kCaller } sam_dict = SamDict::kUnset;
  std::unique_ptr<QueryCursor> query;  // the open bounded traversal (hbam_query_*), if any
  std::unique_ptr<hbam::Merger> merge;  // the open merge (hbam_merge_*), if any (destroyed first: its buffers
                                        // wait for the pipeline's streams)
};

// Forget the split and the query being read: the call about to run moves the
// ctx's window.
static void reset_cursors(hbam_ctx* ctx) {
  if (ctx->last == LastBatch::kSpan) ctx->last = LastBatch::kNone;
  ctx->cursor.reset();
  ctx->query.reset();
}

thread_local std::string hbam_abi::g_open_err;

namespace {
OpenOptions options_of(const hbam_opts* opts, bool header) {
  hbam_opts o{};
  if (opts) o = *opts;
  OpenOptions r;
  r.device = o.device;
  r.check_crc = o.check_crc != 0;
  r.stringency = o.stringency;
  r.window_bytes = o.window_bytes;
  r.parallel_reads = o.parallel_reads != 0;
  r.batch_records = o.batch_records;
  r.parse_header = header;
  return r;
}

int finish_open(int rc, std::unique_ptr<BamFile>&& f, const std::string& err, hbam_ctx** out,
                const hbam_opts* opts = nullptr) {
  auto* c = new hbam_ctx();
  *out = c;  // on failure the caller may read hbam_last_error, then must hbam_close
  if (rc != HBAM_OK) {
    g_open_err = err;
    c->err = err;
    return rc;
  }
  c->f = std::move(f);
  // the caller's batch size is known: its page-locked batch slots are pinned
  // on a helper thread while it goes on (the first hbam_decode_span joins it)
  if (opts && opts->batch_records) c->cursor.start_prealloc(opts->batch_records, opts->device);
  return HBAM_OK;
}

bool valid_stringency(const hbam_opts* o) { return !o || (o->stringency >= 0 && o->stringency <= 2); }

void fill_batch(const hadoop_bam::BatchView& h, hbam_batch* out) {
  out->n = h.n;
  out->ref_id = h.ref_id;
  out->pos = h.pos;
  out->l_seq = h.l_seq;
  out->next_ref_id = h.next_ref_id;
  out->next_pos = h.next_pos;
  out->tlen = h.tlen;
  out->l_read_name = h.l_read_name;
  out->mapq = h.mapq;
  out->bin = h.bin;
  out->n_cigar = h.n_cigar;
  out->flag = h.flag;
  out->key = h.key;
  out->voff = h.voff;
  out->rest_off = h.rest_off;
  out->rest_len = h.rest_len;
  out->data = h.data;
  out->data_len = h.data_len;
}

bool valid_sort_order(int order) {
  return order == HBAM_SORT_KEY || order == HBAM_SORT_COORDINATE || order == HBAM_SORT_QUERYNAME;
}

// the ctx's pipeline: its file's, else the codec's; null when it has neither
hbam::Pipeline* pipe_of(hbam_ctx* ctx) { return !ctx ? nullptr : ctx->f ? &ctx->f->pipe() : ctx->codec.get(); }

// The one rule of what hbam_encode_writables, hbam_sort_writables and
// hbam_format_sam (`who`) serve: the ctx's last batch, if hbam_decode_span
// handed it out and its records lie in one window in HBM (*span).
// need_span_batch: refuse kNone too.  True only for hbam_format_sam: the two
// encodings of a ctx that has no batch (n = 0) are empty and are served.
int batch_span_or_state_error(hbam_ctx* ctx, const char* who, bool need_span_batch, hbam::SpanDev* span) {
  const bool from_span = ctx->last == LastBatch::kSpan || (ctx->last == LastBatch::kNone && !need_span_batch);
  if (from_span && (!ctx->batch.n || ctx->cursor.last_batch_span(span))) return HBAM_OK;
  ctx->err = std::string(who) + " needs a one-window batch from hbam_decode_span";
  return HBAM_E_STATE;
}

// ---- the spine of the three batch-to-bytes calls ------------------------------
int check_cap(hbam_ctx* ctx, uint64_t cap, uint64_t bytes, const char* what) {
  if (cap >= bytes) return HBAM_OK;
  ctx->err = std::string("output buffer too small for the ") + what;
  return HBAM_E_ARG;
}

struct D2H {  // one copy back to the caller (dst NULL: not asked for)
  void* dst;
  const void* src;
  uint64_t bytes;
};

// queues the copies on the pipeline's stream and waits for them once
int copy_back(hbam_ctx* ctx, hipStream_t s, std::initializer_list<D2H> copies) {
  hipError_t e = hipSuccess;
  for (const D2H& c : copies)
    if (e == hipSuccess && c.dst) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && hipStreamSynchronize(s) == hipSuccess) return HBAM_OK;
  ctx->err = "hipMemcpy D2H failed";
  return HBAM_E_DEVICE;
}

// `bytes` of output for the caller: a device buffer of that size rounded up to
// 16, launch(buffer, more) writes it and names up to two further arrays that
// its kernels left in the pipeline; then out and those are copied back.
// alloc_text / alloc_code: what the call answers when the buffer cannot be had
// (the encodings and the SAM text differ, and stay so).
template <class Launch>
int write_and_copy_back(hbam_ctx* ctx, hbam::Pipeline& p, uint8_t* out, uint64_t bytes, const char* alloc_text,
                        int alloc_code, Launch launch) {
  hbam::DevBuf<uint8_t> dst(&p.streams());
  if (dst.reserve((bytes + 15) & ~15ull) != hipSuccess) {
    ctx->err = alloc_text;
    return alloc_code;
  }
  D2H more[2] = {};
  const int rc = launch(dst.p, more);
  if (rc != HBAM_OK) {
    ctx->err = p.error();
    return rc;
  }
  return copy_back(ctx, p.stream(), {{out, dst.p, bytes}, more[0], more[1]});
}

}  // namespace

extern "C" {

int32_t hbam_abi_version(void) { return HBAM_ABI_VERSION; }

int hbam_open_mem(const void* data, uint64_t len, const hbam_opts* opts, hbam_ctx** out) {
  if (!valid_stringency(opts)) return finish_open(HBAM_E_ARG, nullptr, "unknown validation stringency", out);
  std::unique_ptr<BamFile> f;
  std::string err;
  int rc = BamFile::open_memory(static_cast<const uint8_t*>(data), len, options_of(opts, true), &f, &err);
  return finish_open(rc, std::move(f), err, out, opts);
}

int hbam_open_bgzf(const void* data, uint64_t len, const hbam_opts* opts, hbam_ctx** out) {
  std::unique_ptr<BamFile> f;
  std::string err;
  int rc = BamFile::open_memory(static_cast<const uint8_t*>(data), len, options_of(opts, false), &f, &err);
  return finish_open(rc, std::move(f), err, out, opts);
}

int hbam_open(const char* path, const hbam_opts* opts, hbam_ctx** out) {
  if (!valid_stringency(opts)) return finish_open(HBAM_E_ARG, nullptr, "unknown validation stringency", out);
  std::unique_ptr<BamFile> f;
  std::string err;
  int rc = BamFile::open_path(path, options_of(opts, true), &f, &err);
  return finish_open(rc, std::move(f), err, out, opts);
}

int hbam_open_reader(uint64_t size, hbam_read_fn read, void* user, const hbam_opts* opts, hbam_ctx** out) {
  if (!valid_stringency(opts)) return finish_open(HBAM_E_ARG, nullptr, "unknown validation stringency", out);
  if (!read) return finish_open(HBAM_E_ARG, nullptr, "no reader", out);
  std::unique_ptr<BamFile> f;
  std::string err;
  int rc = BamFile::open_reader(size, read, user, options_of(opts, true), &f, &err);
  return finish_open(rc, std::move(f), err, out, opts);
}

void hbam_close(hbam_ctx* ctx) { delete ctx; }

const char* hbam_last_error(hbam_ctx* ctx) { return ctx ? ctx->err.c_str() : g_open_err.c_str(); }

void hbam_free(void* p) { free(p); }

uint64_t hbam_release_cached_memory(void) { return hbam::release_cached(); }

int hbam_bgzf_compress(const hbam_opts* opts, const void* data, uint64_t len, const uint32_t* block_lens,
                       uint64_t n_blocks, int32_t block_size, int32_t level, int32_t flags, uint8_t** out,
                       uint64_t* out_len) {
  *out = nullptr;
  *out_len = 0;
  hbam_opts o{};
  if (opts) o = *opts;
  std::vector<uint64_t> ustart;
  std::vector<uint32_t> lens;
  uint64_t pos = 0;
  if (block_lens) {
    for (uint64_t i = 0; i < n_blocks; ++i) {
      ustart.push_back(pos);
      lens.push_back(block_lens[i]);
      pos += block_lens[i];
    }
    if (pos != len) {
      g_open_err = "block_lens do not sum to len";
      return HBAM_E_ARG;
    }
  } else {
    if (block_size <= 0 || block_size > 65536) {
      g_open_err = "block_size must be 1..65536";
      return HBAM_E_ARG;
    }
    for (; pos < len; pos += (uint64_t)block_size) {
      ustart.push_back(pos);
      lens.push_back((uint32_t)std::min<uint64_t>((uint64_t)block_size, len - pos));
    }
  }
  if (check_device(o.device) != HBAM_OK) return HBAM_E_DEVICE;
  if (hipSetDevice(o.device) != hipSuccess) return HBAM_E_DEVICE;
  hipStream_t s;
  if (hipStreamCreate(&s) != hipSuccess) return HBAM_E_DEVICE;
  uint8_t* d_in = nullptr;
  int rc = HBAM_OK;
  if (hipMalloc(reinterpret_cast<void**>(&d_in), len + 64) != hipSuccess ||  // 64 B pad: deflate's 8-byte compares
      (len && hipMemcpyAsync(d_in, data, len, hipMemcpyHostToDevice, s) != hipSuccess)) {
    g_open_err = "device buffer for the payload";
    rc = HBAM_E_DEVICE;
  }
  {
    hbam::BgzfCompressor c(o.device);
    if (rc == HBAM_OK) {
      rc = c.compress(d_in, ustart, lens, level, (flags & HBAM_BGZF_EOF) != 0, s, nullptr);
      if (rc != HBAM_OK) g_open_err = c.error();
    }
    if (rc == HBAM_OK) {
      uint8_t* h = static_cast<uint8_t*>(malloc(c.out_len() ? c.out_len() : 1));
      if (!h) {
        rc = HBAM_E_NOMEM;
      } else if (c.out_len() && hipMemcpy(h, c.d_out(), c.out_len(), hipMemcpyDeviceToHost) != hipSuccess) {
        free(h);
        rc = HBAM_E_DEVICE;
      } else {
        *out = h;
        *out_len = c.out_len();
      }
    }
  }
  if (d_in) (void)hipFree(d_in);
  (void)hipStreamDestroy(s);
  return rc;
}

int hbam_header(hbam_ctx* ctx, hbam_header_info* out) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  BamFile& f = *ctx->f;
  out->n_ref = f.n_ref();
  out->l_text = f.l_text();
  out->first_record_voff = f.first_record_voff();
  out->file_size = f.file_size();
  out->text = f.text().c_str();
  return HBAM_OK;
}

int hbam_ref(hbam_ctx* ctx, int32_t i, const char** name, int32_t* length) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  if (i < 0 || i >= ctx->f->n_ref()) {
    ctx->err = "reference index out of range";
    return HBAM_E_ARG;
  }
  *name = ctx->f->ref_names()[(size_t)i].c_str();
  *length = ctx->f->ref_lens()[(size_t)i];
  return HBAM_OK;
}

int hbam_file_stats(hbam_ctx* ctx, uint64_t* n_blocks, uint64_t* uncompressed_size) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);  // all_blocks() moves the window
  const std::vector<hbam::BlockInfo>* B = nullptr;
  int rc = ctx->f->all_blocks(&B);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  *n_blocks = B->size();
  *uncompressed_size = B->empty() ? 0 : B->back().ustart + B->back().isize;
  return HBAM_OK;
}

int hbam_bytes_read(hbam_ctx* ctx, uint64_t* bytes) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  *bytes = ctx->f->bytes_read();
  return HBAM_OK;
}

int hbam_prefetch(hbam_ctx* ctx, uint64_t lo, uint64_t hi) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  if (hi < lo) {
    ctx->err = "prefetch range end before its start";
    return HBAM_E_ARG;
  }
  reset_cursors(ctx);
  int rc = ctx->f->prefetch(lo, hi);
  if (rc != HBAM_OK) ctx->err = ctx->f->error();
  return rc;
}

int hbam_decode_span(hbam_ctx* ctx, uint64_t vstart, uint64_t vend, uint64_t max_records, hbam_batch* out) {
  memset(out, 0, sizeof *out);
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  ctx->last = LastBatch::kSpan;
  ctx->query.reset();  // a split read ends an open query
  uint64_t next = vend;
  int rc = ctx->cursor.next_batch(*ctx->f, vstart, vend, max_records, &ctx->batch, &next, &ctx->err);
  fill_batch(ctx->batch, out);
  out->next_voff = next;
  out->status = rc;
  if (rc == HBAM_E_DEVICE || rc == HBAM_E_STATE || rc == HBAM_E_NOMEM) out->n = 0;
  return rc;
}

int hbam_query_intervals(hbam_ctx* ctx, const hbam_interval* iv, uint64_t n_iv, const uint64_t* file_pointers,
                         uint64_t n_ptrs) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  static_assert(sizeof(hbam_interval) == sizeof(hadoop_bam::QueryInterval), "hbam_interval is three int32");
  reset_cursors(ctx);
  std::unique_ptr<QueryCursor> q(new QueryCursor());
  const int rc = q->open_intervals(*ctx->f, reinterpret_cast<const hadoop_bam::QueryInterval*>(iv), n_iv,
                                   file_pointers, n_ptrs, &ctx->err);
  if (rc == HBAM_OK) ctx->query = std::move(q);
  return rc;
}

int hbam_query_unmapped(hbam_ctx* ctx, uint64_t start_voff) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::unique_ptr<QueryCursor> q(new QueryCursor());
  const int rc = q->open_unmapped(*ctx->f, start_voff, &ctx->err);
  if (rc == HBAM_OK) ctx->query = std::move(q);
  return rc;
}

int hbam_query_next(hbam_ctx* ctx, uint64_t max_records, hbam_batch* out) {
  memset(out, 0, sizeof *out);
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  if (!ctx->query) {
    ctx->err = "hbam_query_next needs an open query (hbam_query_intervals / hbam_query_unmapped)";
    return HBAM_E_STATE;
  }
  ctx->last = LastBatch::kQuery;
  const int rc = ctx->query->next_batch(*ctx->f, max_records, &ctx->batch, &ctx->err);
  fill_batch(ctx->batch, out);
  out->status = rc;
  if (rc == HBAM_E_DEVICE || rc == HBAM_E_STATE || rc == HBAM_E_NOMEM) out->n = 0;
  return rc;
}

int hbam_reader_position(hbam_ctx* ctx, uint64_t i, uint64_t* pos) {
  *pos = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  if (ctx->last != LastBatch::kSpan || !ctx->cursor.valid()) {
    ctx->err = "hbam_reader_position needs the last call on the ctx to be hbam_decode_span";
    return HBAM_E_STATE;
  }
  if (i == UINT64_MAX) return ctx->cursor.initial_position(pos, &ctx->err);  // before record 0 is handed out
  if (i >= ctx->batch.n) {
    ctx->err = "record index outside the last batch";
    return HBAM_E_ARG;
  }
  return ctx->cursor.reader_position(i, pos, &ctx->err);
}

int hbam_pipeline_counters(hbam_ctx* ctx, uint64_t out[5]) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  hbam::Pipeline& p = ctx->f->pipe();
  out[0] = p.link_fallbacks();
  out[1] = p.link_rewalks();
  out[2] = p.record_fallbacks();
  out[3] = p.inflate_launches();
  out[4] = p.records_after_stop();
  return HBAM_OK;
}

int hbam_locate_counters(hbam_ctx* ctx, uint64_t out[2]) {
  out[0] = out[1] = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  locate_counters(ctx->f->pipe(), out);
  return HBAM_OK;
}

int hbam_set_locate(hbam_ctx* ctx, uint64_t seg_bytes, uint32_t cap_limit) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  set_locate(*ctx->f, seg_bytes, cap_limit);
  return HBAM_OK;
}

int hbam_inflate_token_count(hbam_ctx* ctx, uint64_t* tokens) {
  *tokens = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  return ctx->f->pipe().inflate_tokens(tokens) == 0 ? HBAM_OK : HBAM_E_DEVICE;
}

int hbam_inflate_path_counts(hbam_ctx* ctx, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  return ctx->f->pipe().inflate_path_counts(out) == 0 ? HBAM_OK : HBAM_E_DEVICE;
}

int hbam_inflate_narrow_counts(hbam_ctx* ctx, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  return ctx->f->pipe().inflate_narrow_counts(out) == 0 ? HBAM_OK : HBAM_E_DEVICE;
}

int hbam_chain_counters(hbam_ctx* ctx, uint64_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  return ctx->f->pipe().chain_counters(out) == 0 ? HBAM_OK : HBAM_E_DEVICE;
}

int hbam_chain_lists(hbam_ctx* ctx, uint64_t** g, uint64_t** x, uint32_t** wcnt, uint16_t** list, uint64_t* n_blocks,
                     uint64_t* n_list, uint32_t* stage) {
  *stage = 0;
  *g = *x = nullptr;
  *wcnt = nullptr;
  *list = nullptr;
  *n_blocks = *n_list = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  return chain_lists(*ctx->f, g, x, wcnt, list, n_blocks, n_list, stage);
}

int hbam_decode_span_device(hbam_ctx* ctx, uint64_t vstart, uint64_t vend, int32_t flags, hbam_gpu_stats* st) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  return decode_device(*ctx->f, vstart, vend, flags, st, nullptr, &ctx->err);
}

int hbam_open_codec(const hbam_opts* opts, hbam_ctx** out) {
  *out = nullptr;
  hbam_opts o{};
  if (opts) o = *opts;
  if (check_device(o.device) != HBAM_OK) return HBAM_E_DEVICE;
  auto* c = new hbam_ctx();
  c->codec.reset(new hbam::Pipeline(o.device));
  *out = c;
  if (!c->codec->error().empty()) {
    c->err = g_open_err = c->codec->error();
    return HBAM_E_DEVICE;
  }
  return HBAM_OK;
}

int hbam_encode_writables(hbam_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* offs, uint64_t* len) {
  *len = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  hbam::Pipeline& p = ctx->f->pipe();
  hbam::SpanDev span;
  int rc = batch_span_or_state_error(ctx, "hbam_encode_writables", false, &span);
  if (rc != HBAM_OK) return rc;
  uint64_t bytes = 0;
  rc = ctx->batch.n ? p.encoded_bytes(span, &bytes) : HBAM_OK;
  if (rc != HBAM_OK) {
    ctx->err = p.error();
    return rc;
  }
  *len = bytes;
  if (offs) {  // encodings have the records' own lengths: record i starts where its bytes did
    const hadoop_bam::BatchView& h = ctx->batch;
    for (uint64_t i = 0; i < h.n; ++i) offs[i] = h.rest_off[i] - h.rest_off[0];
    offs[h.n] = bytes;
  }
  if (!out) return HBAM_OK;
  if ((rc = check_cap(ctx, cap, bytes, "encoded records")) != HBAM_OK || bytes == 0) return rc;
  return write_and_copy_back(ctx, p, out, bytes, "hipMalloc failed", HBAM_E_DEVICE,
                             [&](uint8_t* dst, D2H*) { return p.encode_writables(span, bytes, dst); });
}

int hbam_format_sam(hbam_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* offs, uint64_t* len) {
  *len = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  hbam::Pipeline& p = ctx->f->pipe();
  hbam::SpanDev span;
  int rc = batch_span_or_state_error(ctx, "hbam_format_sam", true, &span);
  if (rc != HBAM_OK) return rc;
  const uint64_t n = ctx->batch.n;
  if (n == 0) {
    if (offs) offs[0] = 0;
    return HBAM_OK;
  }
  if (n >= 0x7fffffffull) {
    ctx->err = "too many records to format in one batch";
    return HBAM_E_ARG;
  }
  uint64_t bytes = 0, bad = ~0ull;
  rc = p.set_sam_refs(ctx->f->ref_names());
  if (rc == HBAM_OK) rc = p.sam_measure(span, &bytes, &bad);
  if (rc != HBAM_OK) {
    ctx->err = p.error();
    return rc;
  }
  if (bad != ~0ull) {
    ctx->err = "malformed aux fields in record " + std::to_string(bad) + " of the batch";
    return HBAM_E_FORMAT;
  }
  *len = bytes;
  // the line starts go back with the size query too
  if (offs && (rc = copy_back(ctx, p.stream(), {{offs, p.sam_offsets(), (n + 1) * 8}})) != HBAM_OK) return rc;
  if (!out) return HBAM_OK;
  if ((rc = check_cap(ctx, cap, bytes, "SAM text")) != HBAM_OK) return rc;
  return write_and_copy_back(ctx, p, out, bytes, "device allocation of the SAM text failed", HBAM_E_NOMEM,
                             [&](uint8_t* dst, D2H*) { return p.sam_write(span, bytes, dst); });
}

int hbam_parse_sam_dict(hbam_ctx* ctx, const char* const* names, int32_t n_ref) {
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (!names && n_ref == -1) {  // back to the file's own (uploaded by the next parse)
    ctx->sam_dict = hbam_ctx::SamDict::kUnset;
    return HBAM_OK;
  }
  if (n_ref < 0 || (n_ref > 0 && !names)) {
    ctx->err = "hbam_parse_sam_dict: n_ref names, or NULL and -1";
    return HBAM_E_ARG;
  }
  std::vector<std::string> v;
  for (int32_t i = 0; i < n_ref; ++i) {
    if (!names[i]) {
      ctx->err = "hbam_parse_sam_dict: name " + std::to_string(i) + " is NULL";
      return HBAM_E_ARG;
    }
    v.emplace_back(names[i]);
  }
  hbam::Pipeline& p = *pipe_of(ctx);
  ctx->sam_dict = hbam_ctx::SamDict::kUnset;
  const int rc = p.samp_set_dict(v);
  if (rc != HBAM_OK) {
    ctx->err = p.error();
    return rc;
  }
  ctx->sam_dict = hbam_ctx::SamDict::kCaller;
  return HBAM_OK;
}

int hbam_parse_sam(hbam_ctx* ctx, const void* text, uint64_t len, int32_t final, hbam_sam_records* out) {
  memset(out, 0, sizeof *out);
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (!text && len) {
    ctx->err = "hbam_parse_sam: no text";
    return HBAM_E_ARG;
  }
  hbam::Pipeline& p = *pipe_of(ctx);
  auto failed = [&](int rc) {
    ctx->err = p.error();
    return rc;
  };
  int rc;
  if (ctx->sam_dict == hbam_ctx::SamDict::kUnset) {
    if ((rc = p.samp_set_dict(ctx->f ? ctx->f->ref_names() : std::vector<std::string>())) != HBAM_OK) return failed(rc);
    ctx->sam_dict = hbam_ctx::SamDict::kFile;
  }
  uint64_t n = 0, consumed = 0, bytes = 0, bad = ~0ull;
  if ((rc = p.samp_lines(static_cast<const uint8_t*>(text), len, final != 0, &n, &consumed)) != HBAM_OK)
    return failed(rc);
  if ((rc = p.samp_measure(n, &bytes, &bad)) != HBAM_OK) return failed(rc);
  if (bad != ~0ull) {
    const uint32_t field = (uint32_t)(bad & 0xff);
    const char* name = hbam::samp_field_name(field);
    ctx->err = "line " + std::to_string(bad >> 8) + " " + name + (name[0] >= 'A' && name[0] <= 'Z' ? " is malformed" : "") +
               " (hbam_parse_sam)";
    return HBAM_E_FORMAT;
  }
  if ((rc = p.samp_write(n, bytes)) != HBAM_OK) return failed(rc);
  out->n = n;
  out->bytes = bytes;
  out->consumed = consumed;
  out->enc = p.samp_enc();
  out->offs = p.samp_offs();
  return HBAM_OK;
}

int hbam_parse_sam_times(hbam_ctx* ctx, float ms[4]) {
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  for (int i = 0; i < 4; ++i) ms[i] = pipe_of(ctx)->samp_times()[i];
  return HBAM_OK;
}

int hbam_sam_header_to_bam(const void* text, uint64_t l_text, uint8_t** hdr, uint64_t* len) {
  *hdr = nullptr;
  *len = 0;
  if (l_text > 0x7fffffffull || (!text && l_text)) {
    g_open_err = "hbam_sam_header_to_bam: a header text of at most 2^31 - 1 bytes";
    return HBAM_E_ARG;
  }
  const char* t = static_cast<const char*>(text);
  std::vector<uint8_t> refs;
  auto put_i32 = [](std::vector<uint8_t>& v, uint32_t x) {
    for (int b = 0; b < 4; ++b) v.push_back((uint8_t)(x >> (8 * b)));
  };
  uint32_t n_ref = 0;
  for (uint64_t l0 = 0; l0 < l_text;) {
    uint64_t l1 = l0;
    while (l1 < l_text && t[l1] != '\n') ++l1;
    uint64_t e = l1;
    if (e > l0 && t[e - 1] == '\r') --e;
    if (e - l0 >= 4 && memcmp(t + l0, "@SQ\t", 4) == 0) {
      std::string sn, ln;
      bool has_sn = false, has_ln = false;
      for (uint64_t a = l0 + 4; a <= e;) {  // the tab-separated fields behind "@SQ"
        uint64_t b = a;
        while (b < e && t[b] != '\t') ++b;
        if (b - a >= 3 && t[a + 2] == ':') {
          if (!has_sn && t[a] == 'S' && t[a + 1] == 'N') sn.assign(t + a + 3, b - a - 3), has_sn = true;
          if (!has_ln && t[a] == 'L' && t[a + 1] == 'N') ln.assign(t + a + 3, b - a - 3), has_ln = true;
        }
        a = b + 1;
      }
      uint64_t v = 0;
      bool ok = has_sn && !sn.empty() && has_ln && !ln.empty();
      for (size_t k = 0; ok && k < ln.size(); ++k) {
        ok = ln[k] >= '0' && ln[k] <= '9' && v <= 0x7fffffffull;
        v = v * 10 + (uint64_t)(ln[k] - '0');
      }
      if (!ok || v > 0x7fffffffull) {
        g_open_err = "hbam_sam_header_to_bam: @SQ line " + std::to_string(n_ref) + " lacks SN or a numeric LN";
        return HBAM_E_FORMAT;
      }
      put_i32(refs, (uint32_t)sn.size() + 1);
      refs.insert(refs.end(), sn.begin(), sn.end());
      refs.push_back(0);
      put_i32(refs, (uint32_t)v);
      ++n_ref;
    }
    l0 = l1 + 1;
  }
  std::vector<uint8_t> h = {'B', 'A', 'M', 1};
  put_i32(h, (uint32_t)l_text);
  h.insert(h.end(), t, t + l_text);
  put_i32(h, n_ref);
  h.insert(h.end(), refs.begin(), refs.end());
  return copy_out(h, hdr, len);
}

int hbam_sort_writables(hbam_ctx* ctx, int32_t order, uint8_t* out, uint64_t cap, uint64_t* offs, uint32_t* perm,
                        uint64_t* len) {
  *len = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  hbam::Pipeline& p = ctx->f->pipe();
  hbam::SpanDev span;
  int rc = batch_span_or_state_error(ctx, "hbam_sort_writables", false, &span);
  if (rc != HBAM_OK) return rc;
  if (!valid_sort_order(order)) {
    ctx->err = "unknown sort order " + std::to_string(order);
    return HBAM_E_ARG;
  }
  const hadoop_bam::BatchView& h = ctx->batch;
  const uint64_t n = h.n;
  if (n >= 0x7fffffffull) {
    ctx->err = "too many records to sort in one batch";
    return HBAM_E_ARG;
  }
  // the encodings' size from the batch's own host columns: no launch
  uint64_t bytes = 36 * n;
  for (uint64_t i = 0; i < n; ++i) bytes += h.rest_len[i];
  *len = bytes;
  if (!out) return HBAM_OK;
  if ((rc = check_cap(ctx, cap, bytes, "encoded records")) != HBAM_OK) return rc;
  if (n == 0) {
    if (offs) offs[0] = 0;
    return HBAM_OK;
  }
  return write_and_copy_back(ctx, p, out, bytes, "hipMalloc failed", HBAM_E_DEVICE, [&](uint8_t* dst, D2H* more) {
    const int r = p.sort_writables(span, order, bytes, dst);
    more[0] = {offs, p.sort_offsets(), (n + 1) * 8};  // all three copies, then one wait
    more[1] = {perm, p.sort_perm(), n * 4};
    return r;
  });
}

int hbam_decode_writables(hbam_ctx* ctx, const void* buf, uint64_t len, const uint64_t* offs, uint64_t n,
                          hbam_batch* out) {
  memset(out, 0, sizeof *out);
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  hbam::Pipeline& p = *pipe_of(ctx);
  reset_cursors(ctx);
  ctx->last = LastBatch::kWritables;
  hbam::SpanDev& span = ctx->wspan;
  span = hbam::SpanDev();
  int rc = p.decode_writables(static_cast<const uint8_t*>(buf), len, offs, n, &span);
  if (rc != HBAM_OK) {
    ctx->err = p.error();
    span = hbam::SpanDev();
    return rc;
  }
  HostBatch& h = ctx->wbatch;
  h.n = 0;
  h.data_len = 0;
  h.window_pos.clear();
  ctx->batch = hadoop_bam::BatchView();
  rc = hadoop_bam::fetch_span(p, span, 0, span.n, &h, &ctx->err);
  if (rc != HBAM_OK) return rc;
  ctx->batch = hadoop_bam::BatchView::of(h);
  fill_batch(ctx->batch, out);
  out->status = span.status;
  if (span.status != HBAM_OK) {
    ctx->err = span.error;
    return span.status;
  }
  return HBAM_OK;
}

int hbam_merge_begin(hbam_ctx* ctx, int32_t order) {
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (ctx->merge) {
    ctx->err = "hbam_merge_begin: a merge is already open on this ctx (hbam_merge_end closes it)";
    return HBAM_E_STATE;
  }
  if (!valid_sort_order(order)) {
    ctx->err = "unknown sort order " + std::to_string(order);
    return HBAM_E_ARG;
  }
  ctx->merge.reset(new hbam::Merger(*pipe_of(ctx), order));
  return HBAM_OK;
}

int hbam_merge_add_run(hbam_ctx* ctx, const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n,
                       const uint64_t* words) {
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (!ctx->merge || ctx->merge->planned()) {
    ctx->err = ctx->merge ? "hbam_merge_add_run after hbam_merge_plan" : "hbam_merge_add_run needs hbam_merge_begin";
    return HBAM_E_STATE;
  }
  hbam::Merger& m = *ctx->merge;
  if (m.order() == HBAM_SORT_QUERYNAME && words) {
    ctx->err = "hbam_merge_add_run: words must be NULL in queryname order (there is no sort word: the names are "
               "read from the encodings)";
    return HBAM_E_ARG;
  }
  int rc = m.begin_run(buf, len, offs, n);
  if (rc != HBAM_OK) {
    ctx->err = "hbam_merge_add_run: " + m.error();
    return rc;
  }
  if (!words && n) {
    // the reducer's case: readFields of the run's values, the words from its columns
    hbam_batch b;
    rc = hbam_decode_writables(ctx, buf, len, offs, n, &b);
    if (rc != HBAM_OK) return rc;
  }
  rc = m.finish_run(words, words || !n ? nullptr : &ctx->wspan);
  if (rc != HBAM_OK) ctx->err = "hbam_merge_add_run: " + m.error();
  return rc;
}

int hbam_merge_plan(hbam_ctx* ctx, uint64_t part_bytes, uint64_t* n_parts, uint64_t* n_records, uint64_t* bytes) {
  *n_parts = *n_records = *bytes = 0;
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (!ctx->merge || ctx->merge->planned()) {
    ctx->err = ctx->merge ? "hbam_merge_plan was already called" : "hbam_merge_plan needs hbam_merge_begin";
    return HBAM_E_STATE;
  }
  const int rc = ctx->merge->plan(part_bytes ? part_bytes : (1ull << 30), n_parts, n_records, bytes);
  if (rc != HBAM_OK) ctx->err = "hbam_merge_plan: " + ctx->merge->error();
  return rc;
}

int hbam_merge_next(hbam_ctx* ctx, uint8_t* out, uint64_t cap, uint64_t* offs, uint64_t* src, uint64_t* n,
                    uint64_t* len) {
  *n = *len = 0;
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  if (!ctx->merge || !ctx->merge->planned()) {
    ctx->err = "hbam_merge_next needs hbam_merge_plan";
    return HBAM_E_STATE;
  }
  const int rc = ctx->merge->next(out, cap, offs, src, n, len);
  if (rc != HBAM_OK) ctx->err = "hbam_merge_next: " + ctx->merge->error();
  return rc;
}

int hbam_merge_end(hbam_ctx* ctx) {
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  ctx->merge.reset();
  return HBAM_OK;
}

int hbam_sort_name_counters(hbam_ctx* ctx, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!pipe_of(ctx)) return HBAM_E_STATE;
  sort_name_counters(*pipe_of(ctx), out);
  return HBAM_OK;
}

int hbam_merge_times(hbam_ctx* ctx, float plan_ms[3], float part_ms[3]) {
  if (!ctx || !ctx->merge) return HBAM_E_STATE;
  for (int i = 0; i < 3; ++i) {
    plan_ms[i] = ctx->merge->plan_ms[i];
    part_ms[i] = ctx->merge->part_ms[i];
  }
  return HBAM_OK;
}

int hbam_build_splitting_index(hbam_ctx* ctx, int32_t granularity, uint8_t** buf, uint64_t* len) {
  *buf = nullptr;
  *len = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<uint8_t> out;
  int rc = SplittingBAMIndexer::index(*ctx->f, granularity, &out);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  return copy_out(out, buf, len);
}

int hbam_build_bai(hbam_ctx* ctx, int32_t flags, uint8_t** buf, uint64_t* len) {
  *buf = nullptr;
  *len = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  if (!ctx->f->is_bam()) {
    ctx->err = "hbam_build_bai needs a BAM (the ctx was opened as plain BGZF)";
    return HBAM_E_STATE;
  }
  reset_cursors(ctx);
  std::vector<uint8_t> out;
  hadoop_bam::BaiBuilder b;
  const int rc = b.build(*ctx->f, (flags & HBAM_BAI_METADATA) != 0, &out, &ctx->err);
  if (rc != HBAM_OK) return rc;
  return copy_out(out, buf, len);
}

int hbam_bai_summarize(const void* bai, uint64_t len, hbam_bai_summary* out) {
  memset(out, 0, sizeof *out);
  out->start_of_last_linear_bin = -1;
  hadoop_bam::BaiIndex idx;
  const int rc = idx.parse(static_cast<const uint8_t*>(bai), len, &g_open_err);
  if (rc != HBAM_OK) return rc;
  out->n_ref = (int32_t)idx.refs.size();
  out->has_no_coor = idx.has_no_coor ? 1 : 0;
  out->no_coor_count = idx.no_coor;
  out->start_of_last_linear_bin = idx.start_of_last_linear_bin();
  return HBAM_OK;
}

int hbam_bai_query(const void* bai, uint64_t len, const hbam_interval* iv, uint64_t n_iv, uint64_t** file_pointers,
                   uint64_t* n_ptrs) {
  *file_pointers = nullptr;
  *n_ptrs = 0;
  hadoop_bam::BaiIndex idx;
  int rc = idx.parse(static_cast<const uint8_t*>(bai), len, &g_open_err);
  if (rc != HBAM_OK) return rc;
  std::vector<uint64_t> out;
  rc = idx.query(reinterpret_cast<const hadoop_bam::QueryInterval*>(iv), n_iv, &out, &g_open_err);
  if (rc != HBAM_OK) return rc;
  return copy_out(out, file_pointers, n_ptrs);
}

int hbam_splitting_entries(hbam_ctx* ctx, uint64_t vstart, uint64_t vend, int32_t granularity, uint64_t ordinal0,
                           uint64_t** entries, uint64_t* n_entries, uint64_t* n_records) {
  *entries = nullptr;
  *n_entries = *n_records = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<uint64_t> ent;
  int rc = SplittingBAMIndexer::entries(*ctx->f, vstart, vend, granularity, ordinal0, &ent, n_records);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  return copy_out(ent, entries, n_entries);
}

int hbam_splitting_index_for_records(const hbam_opts* opts, const uint64_t* voffs, uint64_t n, int32_t granularity,
                                     uint64_t file_size, uint8_t** buf, uint64_t* len) {
  *buf = nullptr;
  *len = 0;
  if (granularity <= 0) {
    g_open_err = "Granularity must be a positive integer";
    return HBAM_E_ARG;
  }
  hbam_opts o{};
  if (opts) o = *opts;
  if (check_device(o.device) != HBAM_OK) return HBAM_E_DEVICE;
  // processAlignment (SplittingBAMIndexer.java:197-202): record 0, then every
  // record whose ordinal + 1 is a multiple of g; finish writes size << 16
  hbam::Pipeline p(o.device);
  if (!p.error().empty()) {
    g_open_err = p.error();
    return HBAM_E_DEVICE;
  }
  hbam::DevBuf<uint64_t> dv(&p.streams());
  std::vector<uint64_t> ent;
  hbam::SpanDev span;
  if (n) {
    if (dv.reserve(n) != hipSuccess || hipMemcpy(dv.p, voffs, n * 8, hipMemcpyHostToDevice) != hipSuccess) {
      g_open_err = "device buffer for the voffs";
      return HBAM_E_DEVICE;
    }
    span.n = n;
    span.rec_voff = dv.p;
    int rc = p.splitting_entries(span, (uint32_t)granularity, 0, &ent);
    if (rc != HBAM_OK) {
      g_open_err = p.error();
      return rc;
    }
  }
  std::vector<uint64_t> all;
  if (n) all.push_back(voffs[0]);
  if (granularity == 1 && n) ent.erase(ent.begin());  // record 0 is written once
  all.insert(all.end(), ent.begin(), ent.end());
  all.push_back(file_size << 16);
  *len = all.size() * 8;
  *buf = static_cast<uint8_t*>(malloc(*len));
  if (!*buf) return HBAM_E_NOMEM;
  for (size_t i = 0; i < all.size(); ++i)
    for (int b = 0; b < 8; ++b) (*buf)[8 * i + b] = (uint8_t)(all[i] >> (56 - 8 * b));
  return HBAM_OK;
}

int hbam_guess_record_starts(hbam_ctx* ctx, const uint64_t* begs, const uint64_t* ends, uint64_t n, uint64_t* out) {
  return hbam_guess_record_starts_hdr(ctx, -1, begs, ends, n, out);
}

int hbam_guess_record_starts_hdr(hbam_ctx* ctx, int32_t header_n_ref, const uint64_t* begs, const uint64_t* ends,
                                 uint64_t n, uint64_t* out) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<uint64_t> b(begs, begs + n), e(ends, ends + n), r;
  hadoop_bam::BAMSplitGuesser g(*ctx->f, header_n_ref);
  int rc = g.guessNextBAMRecordStarts(b, e, &r);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  if (n) memcpy(out, r.data(), n * 8);
  return HBAM_OK;
}

int hbam_guess_bgzf_block_starts(hbam_ctx* ctx, const uint64_t* begs, const uint64_t* ends, uint64_t n,
                                 uint64_t* out) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<uint64_t> b(begs, begs + n), e(ends, ends + n), r;
  int rc = hadoop_bam::guess_bgzf_batch(*ctx->f, b, e, &r, &ctx->err);
  if (rc != HBAM_OK) return rc;
  if (n) memcpy(out, r.data(), n * 8);
  return HBAM_OK;
}

int hbam_get_splits(hbam_ctx* ctx, const uint64_t* starts, const uint64_t* lengths, uint64_t n, const uint8_t* sbi,
                    uint64_t sbi_len, uint64_t* vstarts, uint64_t* vends, uint64_t* nout) {
  return hbam_get_splits_bai(ctx, starts, lengths, n, sbi, sbi_len, nullptr, 0, vstarts, vends, nout);
}

int hbam_get_splits_bai(hbam_ctx* ctx, const uint64_t* starts, const uint64_t* lengths, uint64_t n,
                        const uint8_t* sbi, uint64_t sbi_len, const uint8_t* bai, uint64_t bai_len, uint64_t* vstarts,
                        uint64_t* vends, uint64_t* nout) {
  *nout = 0;
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<FileSplit> sp(n);
  for (uint64_t i = 0; i < n; ++i) {
    sp[i].path = "bam";
    sp[i].start = starts[i];
    sp[i].length = lengths[i];
  }
  std::vector<FileVirtualSplit> out;
  int rc = BAMInputFormat::getSplits(*ctx->f, sp, sbi, sbi_len, &out, bai, bai_len);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  for (size_t i = 0; i < out.size(); ++i) {
    vstarts[i] = out[i].vStart;
    vends[i] = out[i].vEnd;
  }
  *nout = out.size();
  return HBAM_OK;
}

int hbam_blocks(hbam_ctx* ctx, uint64_t* coff, uint32_t* csize, uint32_t* isize, uint64_t* ustart, uint64_t cap,
                uint64_t* n) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  const std::vector<hbam::BlockInfo>* B = nullptr;
  int rc = ctx->f->all_blocks(&B);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  *n = B->size();
  for (size_t i = 0; i < B->size() && i < cap; ++i) {
    if (coff) coff[i] = (*B)[i].coff;
    if (csize) csize[i] = (*B)[i].csize;
    if (isize) isize[i] = (*B)[i].isize;
    if (ustart) ustart[i] = (*B)[i].ustart;
  }
  return HBAM_OK;
}

int hbam_read_inflated(hbam_ctx* ctx, uint64_t pos, uint64_t len, uint8_t* dst) {
  if (!ctx || !ctx->f) return HBAM_E_STATE;
  reset_cursors(ctx);
  std::vector<uint8_t> v;
  int rc = ctx->f->read_inflated(pos, len, &v);
  if (rc != HBAM_OK) {
    ctx->err = ctx->f->error();
    return rc;
  }
  if (v.size() != len) {
    ctx->err = "range beyond the inflated stream";
    return HBAM_E_ARG;
  }
  if (len) memcpy(dst, v.data(), len);
  return HBAM_OK;
}

int64_t hbam_get_key0(int32_t ref_idx, int32_t alignment_start0) {
  return BAMRecordReader::getKey0(ref_idx, alignment_start0);
}
int64_t hbam_get_key(int32_t ref_idx, int32_t alignment_start) {
  return BAMRecordReader::getKey(ref_idx, alignment_start);
}
int64_t hbam_murmurhash3(const void* key, uint64_t len, int32_t seed) {
  return hadoop_bam::murmurhash3(static_cast<const uint8_t*>(key), len, seed);
}

}  // extern "C"
