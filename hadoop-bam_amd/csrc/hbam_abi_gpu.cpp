// hbam_abi_gpu.cpp -- extern "C" boundary, second half: the device-resident
// decode on hbam_gpu (include/hbam.h's benchmark / multi-GPU shard driver
// block) and the page-locked host blocks.  The product API: hbam_abi.cpp.
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>

#include "hbam_abi_util.h"
#include "hbam_deflate_api.h"
#include "hbam_mem.h"

using namespace hbam_abi;
using hadoop_bam::Carry;
using hadoop_bam::OpenOptions;
using hadoop_bam::SplittingBAMIndexer;
using hadoop_bam::Step;

struct hbam_gpu {
  std::unique_ptr<BamFile> f;
  int device = 0;
  uint64_t window = hadoop_bam::kDefaultWindowBytes;
  int stringency = HBAM_STRICT;  // of the next hbam_gpu_load
  std::string err;
  hbam::SpanDev span;  // last window of the last run
  hbam::DevBuf<uint8_t> enc;  // hbam_gpu_encode_writables output
  uint64_t enc_bytes = 0;
  std::unique_ptr<hbam::BgzfCompressor> bgzf;  // hbam_gpu_bgzf_compress
};

namespace hbam_abi {
// The decode of FileVirtualSplit [vstart, vend) window by window with the
// records left in HBM; stats accumulate over windows.  *last = the last
// window's span (C2-sized files: the whole split).
int decode_device(BamFile& f, uint64_t vstart, uint64_t vend, int32_t flags, hbam_gpu_stats* st,
                  hbam::SpanDev* last, std::string* err) {
  memset(st, 0, sizeof *st);
  hbam::Pipeline& p = f.pipe();
  p.timing = (flags & 1) != 0;
  const bool decode = (flags & 2) == 0, digest = (flags & 4) != 0;
  EventPair ev;
  ev.start(p.stream());
  const uint64_t lf0 = p.link_fallbacks(), il0 = p.inflate_launches(), lr0 = p.link_rewalks();
  const uint64_t rf0 = p.record_fallbacks();
  f.invalidate_window();  // a timed pass locates and inflates afresh
  Carry c{vstart >> 16, vstart & 0xffff};
  bool cont = false;
  int rc = HBAM_OK;
  bool first = true;
  // Windows read from the host ramp up (SpanCursor::ramp_window: 32 MiB,
  // doubling to the full window), so that decoding starts after the first
  // small copy instead of a whole 4 GiB window's (C3 from the mapped file);
  // a span already in HBM decodes in full windows.
  const uint64_t span_end = std::min<uint64_t>(f.file_size(), vend == ~0ull ? ~0ull : (vend >> 16) + 0x20000);
  const bool ramp = !f.window_explicit() && !f.resident(vstart >> 16, span_end);
  uint64_t nwin = 0;
  for (;;) {
    Step step;
    rc = ramp ? f.decode_step(c, vend, hbam::kReader, decode, cont, &step,
                              hadoop_bam::SpanCursor::ramp_window(f.window_bytes(), nwin),
                              hadoop_bam::SpanCursor::ramp_window(f.window_bytes(), nwin + 1))
              : f.decode_step(c, vend, hbam::kReader, decode, cont, &step);
    ++nwin;
    if (rc != HBAM_OK) {
      *err = f.error();
      break;
    }
    const hbam::SpanDev& s = step.span;
    st->windows += 1;
    st->records += s.n;
    st->n_blocks += p.blocks().size();
    // bytes of this window up to the block the next window starts at (it
    // starts at the record this one could not finish): each counted once
    const bool last_window = step.ended || step.status != HBAM_OK;
    const int64_t next_u = last_window ? -1 : p.pos_of_voff(step.next.coff << 16);
    if (next_u < 0) {
      st->compressed_bytes += p.window_end() - c.coff;
      st->inflated_bytes += p.total_u();
    } else {
      st->compressed_bytes += step.next.coff - c.coff;
      st->inflated_bytes += (uint64_t)next_u;
    }
    if (p.timing) {
      st->ms_locate += p.times.locate;
      st->ms_inflate += p.times.inflate;
      st->ms_huff += p.times.huff;
      st->ms_lz77 += p.times.lz77;
      st->ms_tables += p.times.tables;
      st->ms_chain += p.times.chain;
      st->ms_decode += p.times.decode;
    }
    if (s.n) {
      if (first) st->first_voff = s.first_voff;
      st->last_voff = s.last_voff;
      first = false;
      if (digest) {
        uint64_t dg[4];
        hbam::SpanDev d = s;
        if (!decode) d.col.key = nullptr;
        rc = p.span_digest(d, dg);
        if (rc != HBAM_OK) {
          *err = p.error();
          break;
        }
        st->key_xor ^= dg[0];
        st->voff_sum += dg[1];
        uint64_t w = 1, b = HBAM_DIGEST_P;  // P^n of this window's records
        for (uint64_t e = s.n; e; e >>= 1, b *= b)
          if (e & 1) w *= b;
        st->key_digest = st->key_digest * w + dg[2];
        st->voff_digest = st->voff_digest * w + dg[3];
      }
    }
    if (last) *last = s;
    if (step.status != HBAM_OK) {
      st->status = step.status;
      *err = step.error;
      break;
    }
    if (step.ended) break;
    c = step.next;
    cont = true;
  }
  st->ms_total = ev.stop_ms(p.stream());
  st->link_fallbacks = (int32_t)(p.link_fallbacks() - lf0);
  st->inflate_launches = (int32_t)(p.inflate_launches() - il0);
  st->link_rewalks = (int32_t)(p.link_rewalks() - lr0);
  st->record_fallbacks = (int32_t)(p.record_fallbacks() - rf0);
  if (rc != HBAM_OK) st->status = rc;
  return rc != HBAM_OK ? rc : st->status;
}

// hbam_chain_lists: Pipeline::chain_lists into malloc'ed arrays for the caller
int chain_lists(BamFile& f, uint64_t** g, uint64_t** x, uint32_t** wcnt, uint16_t** list, uint64_t* n_blocks,
                uint64_t* n_list, uint32_t* stage) {
  std::vector<uint64_t> gv, xv;
  std::vector<uint32_t> wv;
  std::vector<uint16_t> lv;
  if (f.pipe().chain_lists(&gv, &xv, &wv, &lv, stage) != 0) return HBAM_E_DEVICE;
  int rc = copy_out(gv, g, n_blocks);
  if (rc == HBAM_OK) rc = copy_out(xv, x, n_blocks);
  if (rc == HBAM_OK) rc = copy_out(wv, wcnt, n_blocks);
  if (rc == HBAM_OK) rc = copy_out(lv, list, n_list);
  if (rc != HBAM_OK) {
    for (void* p : {(void*)*g, (void*)*x, (void*)*wcnt, (void*)*list}) free(p);
    *g = *x = nullptr;
    *wcnt = nullptr;
    *list = nullptr;
    *n_blocks = *n_list = 0;
  }
  return rc;
}
}  // namespace hbam_abi

namespace {
// page-locked blocks handed out by hbam_host_alloc and their sizes (pinned_free needs them)
std::mutex& host_alloc_mu() {
  static std::mutex* m = new std::mutex();
  return *m;
}
std::map<void*, size_t>& host_allocs() {
  static std::map<void*, size_t>* m = new std::map<void*, size_t>();
  return *m;
}


// The shape of the three timed write-path calls into g->enc: size(&nb) gives the
// output's bytes (and g->err on failure), the buffer is reserved, round(nb, 0)
// runs once as the warm-up (it also checks the launches), then `iters` timed
// rounds, and enc_bytes is published.  per_round: round(nb, t) fills its own
// three times and ms[3] gets their means; else one event pair spans all rounds,
// started after the warm-up, and ms[0] gets the mean.
template <class Size, class Round>
int timed_rounds(hbam_gpu* g, int32_t iters, bool per_round, float* ms, uint64_t* bytes, const char* alloc_text,
                 int alloc_code, Size size, Round round) {
  for (int k = 0; k < (per_round ? 3 : 1); ++k) ms[k] = 0;
  *bytes = 0;
  if (!g->f) return HBAM_E_STATE;
  hbam::Pipeline& p = g->f->pipe();
  g->enc.owner = &p.streams();
  uint64_t nb = 0;
  int rc = size(p, &nb);
  if (rc != HBAM_OK) return rc;
  if (g->enc.reserve((nb + 15) & ~15ull) != hipSuccess) {
    g->err = alloc_text;
    return alloc_code;
  }
  if (per_round) {
    rc = round(p, nb, nullptr);
    for (int32_t i = 0; i < iters && rc == HBAM_OK; ++i) {
      float t[3] = {0, 0, 0};
      rc = round(p, nb, t);
      for (int k = 0; k < 3; ++k) ms[k] += t[k] / (float)iters;
    }
    if (rc == HBAM_OK && hipStreamSynchronize(p.stream()) != hipSuccess) {
      g->err = "hipStreamSynchronize failed";
      return HBAM_E_DEVICE;
    }
  } else {
    EventPair ev;
    rc = round(p, nb, nullptr);
    if (rc == HBAM_OK) {
      ev.start(p.stream());
      for (int32_t i = 0; i < iters && rc == HBAM_OK; ++i) rc = round(p, nb, nullptr);
      const float total = ev.stop_ms(p.stream());
      ms[0] = iters > 0 ? total / (float)iters : 0.f;
    }
  }
  if (rc != HBAM_OK) {
    g->err = p.error();
    return rc;
  }
  g->enc_bytes = nb;
  *bytes = nb;
  return HBAM_OK;
}

// the size of the encodings of the last run's records
int encoded_size(hbam_gpu* g, hbam::Pipeline& p, uint64_t* nb) {
  const int rc = p.encoded_bytes(g->span, nb);
  if (rc != HBAM_OK) g->err = p.error();
  return rc;
}
}  // namespace

extern "C" {

int32_t hbam_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int hbam_gpu_create(int32_t device, hbam_gpu** out) {
  *out = nullptr;
  if (check_device(device) != HBAM_OK) return HBAM_E_DEVICE;
  auto* g = new hbam_gpu();
  g->device = device;
  *out = g;
  return HBAM_OK;
}

void hbam_gpu_destroy(hbam_gpu* g) { delete g; }

const char* hbam_gpu_error(hbam_gpu* g) { return g ? g->err.c_str() : g_open_err.c_str(); }

int hbam_gpu_load(hbam_gpu* g, const void* data, uint64_t len) {
  OpenOptions o;
  o.device = g->device;
  o.window_bytes = g->window;
  o.stringency = g->stringency;
  g->enc.release();  // owned by the old file's pipeline streams
  g->enc.owner = nullptr;
  g->f.reset();
  g->span = hbam::SpanDev();
  std::string err;
  int rc = BamFile::open_device_copy(static_cast<const uint8_t*>(data), len, o, &g->f, &err);
  if (rc != HBAM_OK) g->err = err;
  return rc;
}

int hbam_gpu_set_window(hbam_gpu* g, uint64_t window_bytes) {
  g->window = window_bytes ? window_bytes : hadoop_bam::kDefaultWindowBytes;
  if (g->f) g->f->set_window_bytes(g->window);
  return HBAM_OK;
}

int hbam_gpu_set_stringency(hbam_gpu* g, int32_t stringency) {
  if (stringency < HBAM_STRICT || stringency > HBAM_SILENT) {
    g->err = "unknown validation stringency";
    return HBAM_E_ARG;
  }
  g->stringency = stringency;
  return HBAM_OK;
}

int hbam_gpu_set_locate(hbam_gpu* g, uint64_t seg_bytes, uint32_t cap_limit) {
  if (!g->f) {
    g->err = "hbam_gpu_set_locate needs a loaded file";
    return HBAM_E_STATE;
  }
  set_locate(*g->f, seg_bytes, cap_limit);
  return HBAM_OK;
}

int hbam_gpu_locate_counters(hbam_gpu* g, uint64_t out[2]) {
  out[0] = out[1] = 0;
  if (!g->f) return HBAM_E_STATE;
  locate_counters(g->f->pipe(), out);
  return HBAM_OK;
}

int hbam_gpu_run(hbam_gpu* g, int32_t flags, hbam_gpu_stats* st) {
  memset(st, 0, sizeof *st);
  if (!g->f) {
    g->err = "hbam_gpu_run needs a loaded file";
    return HBAM_E_STATE;
  }
  return decode_device(*g->f, g->f->first_record_voff(), ~0ull, flags, st, &g->span, &g->err);
}

int hbam_gpu_index(hbam_gpu* g, int32_t granularity, uint8_t** buf, uint64_t* len, float* ms) {
  *buf = nullptr;
  *len = 0;
  *ms = 0;
  if (!g->f) return HBAM_E_STATE;
  hbam::Pipeline& p = g->f->pipe();
  p.timing = false;
  g->f->invalidate_window();
  EventPair ev;
  ev.start(p.stream());
  std::vector<uint8_t> out;
  int rc = SplittingBAMIndexer::index(*g->f, granularity, &out);
  *ms = ev.stop_ms(p.stream());
  g->span = hbam::SpanDev();
  if (rc != HBAM_OK) {
    g->err = g->f->error();
    return rc;
  }
  return copy_out(out, buf, len);
}

int hbam_gpu_run_streamed(hbam_gpu* g, const void* data, uint64_t len, uint64_t piece_bytes, hbam_gpu_stats* st) {
  memset(st, 0, sizeof *st);
  if (!g->f || len != g->f->file_size()) {
    g->err = "hbam_gpu_run_streamed needs the loaded file's bytes";
    return HBAM_E_STATE;
  }
  hbam::Pipeline& p = g->f->pipe();
  p.timing = false;
  g->f->invalidate_window();
  // one window holding the whole file in the pipeline's own buffer (untimed)
  int rc = p.load(static_cast<const uint8_t*>(data), len, 0, true);
  if (rc != HBAM_OK) {
    g->err = p.error();
    return rc;
  }
  const uint64_t il0 = p.inflate_launches();
  g->span = hbam::SpanDev();
  // first record: the header end (the same position the resident pass starts at)
  std::unique_ptr<BamFile>& f = g->f;
  rc = p.locate();
  uint64_t first_pos = 0;
  if (rc == HBAM_OK) {
    const int64_t fp = p.pos_of_voff(f->first_record_voff());
    if (fp < 0) rc = HBAM_E_STATE;
    first_pos = (uint64_t)std::max<int64_t>(fp, 0);
  }
  if (rc == HBAM_OK)
    rc = p.run_streamed(static_cast<const uint8_t*>(data), len, piece_bytes, first_pos, &g->span, &st->ms_total);
  g->f->invalidate_window();
  if (rc != HBAM_OK) {
    g->err = p.error();
    st->status = rc;
    return rc;
  }
  st->n_blocks = p.blocks().size();
  st->compressed_bytes = p.file_len();
  st->inflated_bytes = p.total_u();
  st->records = g->span.n;
  st->status = g->span.status;
  st->windows = 1;
  st->inflate_launches = (int32_t)(p.inflate_launches() - il0);
  if (g->span.n) {
    (void)hipMemcpy(&st->first_voff, g->span.rec_voff, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&st->last_voff, g->span.rec_voff + g->span.n - 1, 8, hipMemcpyDeviceToHost);
  }
  if (g->span.status != HBAM_OK) g->err = g->span.error;
  return g->span.status;
}

void* hbam_host_alloc(uint64_t bytes) {
  // the library's page-locked blocks: on the current device's NUMA node (hbam_mem.cpp)
  void* p = nullptr;
  size_t got = 0;
  if (hbam::pinned_alloc(&p, bytes ? bytes : 1, &got) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(host_alloc_mu());
  host_allocs()[p] = got;
  return p;
}

void hbam_host_free(void* p) {
  if (!p) return;
  size_t bytes = 0;
  {
    std::lock_guard<std::mutex> lk(host_alloc_mu());
    auto it = host_allocs().find(p);
    if (it == host_allocs().end()) return;
    bytes = it->second;
    host_allocs().erase(it);
  }
  hbam::pinned_free(p, bytes);
}

int hbam_gpu_reload(hbam_gpu* g, const void* data, uint64_t len, int32_t pinned, float* ms) {
  *ms = 0;
  if (!g->f) return HBAM_E_STATE;
  hbam::Pipeline& p = g->f->pipe();
  g->f->invalidate_window();
  int rc = p.load(static_cast<const uint8_t*>(data), len, 0, true);  // the copy target (untimed)
  if (rc == HBAM_OK) rc = p.reload(static_cast<const uint8_t*>(data), len, pinned != 0, ms);
  if (rc != HBAM_OK) g->err = p.error();
  g->span = hbam::SpanDev();
  return rc;
}

int hbam_gpu_d2d_bandwidth(hbam_gpu* g, uint64_t bytes, int32_t iters, float* gbps) {
  if (!g->f) return HBAM_E_STATE;
  int rc = g->f->pipe().d2d_bandwidth(bytes, iters, gbps);
  if (rc != HBAM_OK) g->err = g->f->pipe().error();
  return rc;
}


int hbam_gpu_encode_writables(hbam_gpu* g, int32_t iters, float* ms_per_iter, uint64_t* bytes) {
  return timed_rounds(
      g, iters, false, ms_per_iter, bytes, "hipMalloc failed", HBAM_E_DEVICE,
      [&](hbam::Pipeline& p, uint64_t* nb) { return encoded_size(g, p, nb); },
      [&](hbam::Pipeline& p, uint64_t nb, float*) { return p.encode_writables(g->span, nb, g->enc.p); });
}

int hbam_gpu_sort_writables(hbam_gpu* g, int32_t order, int32_t iters, float ms[3], uint64_t* bytes) {
  return timed_rounds(
      g, iters, true, ms, bytes, "hipMalloc failed", HBAM_E_DEVICE,
      [&](hbam::Pipeline& p, uint64_t* nb) { return encoded_size(g, p, nb); },
      [&](hbam::Pipeline& p, uint64_t nb, float* t) { return p.sort_writables(g->span, order, nb, g->enc.p, t); });
}

int hbam_gpu_format_sam(hbam_gpu* g, int32_t iters, float ms[3], uint64_t* bytes) {
  uint64_t bad = ~0ull;
  return timed_rounds(
      g, iters, true, ms, bytes, "device allocation of the SAM text failed", HBAM_E_NOMEM,
      [&](hbam::Pipeline& p, uint64_t* nb) {  // the measure pass that sizes the text is the warm-up's
        int rc = p.set_sam_refs(g->f->ref_names());
        if (rc == HBAM_OK) rc = p.sam_measure(g->span, nb, &bad);
        if (rc != HBAM_OK) {
          g->err = p.error();
        } else if (bad != ~0ull) {
          g->err = "malformed aux fields in record " + std::to_string(bad) + " of the window";
          rc = HBAM_E_FORMAT;
        }
        return rc;
      },
      [&](hbam::Pipeline& p, uint64_t nb, float* t) {
        int rc = t ? p.sam_measure(g->span, &nb, &bad, t) : HBAM_OK;
        if (rc == HBAM_OK) rc = p.sam_write(g->span, nb, g->enc.p, t ? t + 2 : nullptr);
        return rc;
      });
}

int hbam_gpu_sort_name_counters(hbam_gpu* g, uint64_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!g->f) return HBAM_E_STATE;
  sort_name_counters(g->f->pipe(), out);
  return HBAM_OK;
}

int hbam_gpu_sort_name_times(hbam_gpu* g, float ms[3]) {
  ms[0] = ms[1] = ms[2] = 0;
  if (!g->f) return HBAM_E_STATE;
  for (int i = 0; i < 3; ++i) ms[i] = g->f->pipe().name_times()[i];
  return HBAM_OK;
}

int hbam_gpu_fetch_encoded(hbam_gpu* g, uint64_t pos, uint64_t len, uint8_t* dst) {
  if (pos > g->enc_bytes || len > g->enc_bytes - pos) {
    g->err = "range outside the encoded records";
    return HBAM_E_ARG;
  }
  if (len && hipMemcpy(dst, g->enc.p + pos, len, hipMemcpyDeviceToHost) != hipSuccess) return HBAM_E_DEVICE;
  return HBAM_OK;
}

int hbam_gpu_bgzf_compress(hbam_gpu* g, int32_t level, int32_t flags, int32_t iters, float* ms_per_iter,
                           uint64_t* out_len) {
  *ms_per_iter = 0;
  *out_len = 0;
  if (!g->f) return HBAM_E_STATE;
  hbam::Pipeline& p = g->f->pipe();
  if (!p.d_u() || p.base() != 0 || !p.at_eof() || p.blocks().empty()) {
    g->err = "hbam_gpu_bgzf_compress needs a one-window run (inflated stream) first";
    return HBAM_E_STATE;
  }
  std::vector<uint64_t> ustart;
  std::vector<uint32_t> lens;
  const auto& B = p.blocks();
  // the input's EOF terminator is re-added by HBAM_BGZF_EOF, not recompressed
  size_t nb = B.size();
  if ((flags & HBAM_BGZF_EOF) && nb && B[nb - 1].isize == 0) --nb;
  for (size_t i = 0; i < nb; ++i) {
    ustart.push_back(B[i].ustart);
    lens.push_back(B[i].isize);
  }
  // the run inflated the blocks from the first record on; the header's too
  int rc0 = p.inflate(0, (uint32_t)B.size());
  if (rc0 != HBAM_OK) {
    g->err = p.error();
    return rc0;
  }
  if (!g->bgzf) g->bgzf.reset(new hbam::BgzfCompressor(p.device()));
  float ms = 0, tot = 0;
  int rc = g->bgzf->compress(p.d_u(), ustart, lens, level, (flags & HBAM_BGZF_EOF) != 0, p.stream(), &ms);
  for (int32_t i = 0; i < iters && rc == HBAM_OK; ++i) {
    rc = g->bgzf->compress(p.d_u(), ustart, lens, level, (flags & HBAM_BGZF_EOF) != 0, p.stream(), &ms);
    tot += ms;
  }
  if (rc != HBAM_OK) {
    g->err = g->bgzf->error();
    return rc;
  }
  *ms_per_iter = iters > 0 ? tot / (float)iters : ms;
  *out_len = g->bgzf->out_len();
  return HBAM_OK;
}

int hbam_gpu_fetch_compressed(hbam_gpu* g, uint64_t pos, uint64_t len, uint8_t* dst) {
  const uint64_t n = g->bgzf ? g->bgzf->out_len() : 0;
  if (pos > n || len > n - pos) {
    g->err = "range outside the compressed output";
    return HBAM_E_ARG;
  }
  if (len && hipMemcpy(dst, g->bgzf->d_out() + pos, len, hipMemcpyDeviceToHost) != hipSuccess) return HBAM_E_DEVICE;
  return HBAM_OK;
}

int hbam_gpu_fetch(hbam_gpu* g, int64_t* keys, uint64_t* voffs, uint64_t cap) {
  const uint64_t n = std::min<uint64_t>(cap, g->span.n);
  if (keys && n && g->span.col.key) {
    if (hipMemcpy(keys, g->span.col.key, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return HBAM_E_DEVICE;
  }
  if (voffs && n) {
    if (hipMemcpy(voffs, g->span.rec_voff, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return HBAM_E_DEVICE;
  }
  return HBAM_OK;
}

}  // extern "C"
