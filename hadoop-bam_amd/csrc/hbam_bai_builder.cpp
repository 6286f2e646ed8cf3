// hbam_bai_builder.cpp -- BaiBuilder: the .bai behind hbam_build_bai.
//
// The window loop of hbam_decode_span_device (BamFile::decode_step from the
// first record, the next record's position carried across windows); per
// window the kernels of hbam_bai.h and one read-back of the window's verdict
// (first failing record, last key, largest sort key, boundaries); at the end
// the sort of the run list, the gap fill of the linear tables, their copy to
// the host and the serialisation (SAM spec 5.2).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "hbam_bai.h"
#include "hbam_host.h"

namespace hadoop_bam {

using hbam::kErrDevice;
using hbam::kErrFormat;
using hbam::kErrNoMem;
using hbam::kErrState;
using hbam::kOk;

namespace {
int hip_err(hipError_t e, const char* what, std::string* err) {
  if (e == hipSuccess) return kOk;
  *err = std::string(what) + ": " + hipGetErrorString(e);
  return kErrDevice;
}
#define BCHK(expr)                               \
  do {                                           \
    const int _rc = hip_err((expr), #expr, err); \
    if (_rc != kOk) return _rc;                  \
  } while (0)

void put_le(std::vector<uint8_t>* o, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; ++i) o->push_back((uint8_t)(v >> (8 * i)));
}
}  // namespace

int BaiBuilder::begin(BamFile& f, bool metadata, std::string* err) {
  const hbam::StreamSet* o = &f.pipe().streams();
  d_lin_off_.owner = bflag_.owner = slot_.owner = iota_.owner = perm_.owner = ord_.owner = last_.owner = o;
  lin_.owner = unm_.owner = state_.owner = key_.owner = sk_.owner = skmax_.owner = wspan_.owner = run_key_.owner =
      run_start_.owner = run_end_.owner = run_ord_.owner = s_key_.owner = s_start_.owner = s_end_.owner =
          s_count_.owner = filled_.owner = o;
  tmp_.owner = o;
  BCHK(hipSetDevice(f.pipe().device()));
  // a contig's linear table from the header's l_ref: (min(l_ref, 2^29) >> 14) + 1 windows
  const size_t n_ref = (size_t)f.n_ref();
  lin_off_.assign(n_ref + 1, 0);
  uint64_t total = 0;
  for (size_t r = 0; r < n_ref; ++r) {
    const int64_t l = std::min<int64_t>(std::max<int32_t>(f.ref_lens()[r], 0), hbam::kBaiMaxEnd);
    total += (uint64_t)(l >> hbam::kBaiLinShift) + 1;
    if (total >= (uint64_t)INT_MAX) {
      *err = "the linear tables of the header's references do not fit the index build";
      return kErrNoMem;
    }
    lin_off_[r + 1] = (uint32_t)total;
  }
  const hipStream_t s = f.pipe().stream();
  BCHK(d_lin_off_.reserve(n_ref + 1));
  BCHK(lin_.reserve(total ? total : 1));
  BCHK(unm_.reserve(n_ref ? n_ref : 1));
  BCHK(state_.reserve(hbam::kBaiStateWords));
  BCHK(hipMemcpyAsync(d_lin_off_.p, lin_off_.data(), 4 * (n_ref + 1), hipMemcpyHostToDevice, s));
  BCHK(hipMemsetAsync(lin_.p, 0xff, 8 * (total ? total : 1), s));
  BCHK(hipMemsetAsync(unm_.p, 0, 8 * (n_ref ? n_ref : 1), s));
  BCHK(hipStreamSynchronize(s));  // lin_off_ is pageable
  carry_key_ = (uint64_t)n_ref << 16;  // "unindexed": the first indexed record is a boundary
  carry_sk_ = 0;
  records_ = runs_ = 0;
  metadata_ = metadata;
  return kOk;
}

int BaiBuilder::add_window(BamFile& f, const SpanDev& s, std::string* err) {
  const uint64_t n = s.n;
  if (n == 0) return kOk;
  if (n >= (uint64_t)INT_MAX - 1) {
    *err = "too many records in one window for the index scans";
    return kErrState;
  }
  hbam::Pipeline& p = f.pipe();
  const hipStream_t st = p.stream();
  const uint8_t* u = s.data ? s.data : p.d_u();
  size_t tb = 0;
  BCHK(hbam::bai_scan_bytes(n, &tb));
  BCHK(tmp_.reserve(tb ? tb : 1));
  BCHK(key_.reserve(n));
  BCHK(sk_.reserve(n));
  BCHK(skmax_.reserve(n));
  BCHK(wspan_.reserve(n));
  BCHK(bflag_.reserve(n + 1));
  BCHK(slot_.reserve(n + 1));
  const hbam::BaiTables t{d_lin_off_.p, lin_.p, metadata_ ? unm_.p : nullptr, f.n_ref()};
  const hbam::BaiWindow w{key_.p, sk_.p, skmax_.p, reinterpret_cast<uint2*>(wspan_.p), bflag_.p, slot_.p};
  BCHK(hipMemsetAsync(state_.p, 0xff, 8 * hbam::kBaiStateWords, st));
  BCHK(hbam::launch_bai_classify(u, s.col, n, t, w, state_.p, st));
  BCHK(hbam::launch_bai_link(tmp_.p, tb, s.col, n, carry_key_, carry_sk_, t, w, state_.p, st));
  uint64_t v[hbam::kBaiStateWords];
  hipError_t e = p.rb(v, state_.p, sizeof v, st);
  if (e == hipSuccess) e = p.rb_sync(st);
  if (e != hipSuccess) {
    p.rb_cancel();  // v is a local: the queue must not keep its address
    return hip_err(e, "read-back of the index state", err);
  }
  if (v[hbam::kBaiErr] != ~0ull) {
    const std::string rec = "record " + std::to_string(records_ + (v[hbam::kBaiErr] >> 2));
    switch ((int)(v[hbam::kBaiErr] & 3)) {
      case hbam::kBaiErrOrder:
        *err = "the BAM is not coordinate-sorted: " + rec + " sorts before an earlier record";
        break;
      case hbam::kBaiErrEnd:
        *err = rec + " ends past 2^29, the largest coordinate a BAM index addresses";
        break;
      case hbam::kBaiErrWindow:
        *err = rec + " lies past the end of its reference (the header's l_ref sizes the linear index)";
        break;
      default:
        *err = rec + " has a refID past the header's references";
        break;
    }
    return kErrFormat;
  }
  const uint64_t heads = v[hbam::kBaiHeads];
  if (runs_ + heads >= (uint64_t)INT_MAX) {
    *err = "too many chunks for the index sort";
    return kErrState;
  }
  if (heads) {
    BCHK(run_key_.grow(runs_ + heads));
    BCHK(run_start_.grow(runs_ + heads));
    BCHK(run_end_.grow(runs_ + heads));
    BCHK(run_ord_.grow(runs_ + heads));
    BCHK(hbam::launch_bai_emit(s.col.voff, n, w, runs_, records_, run_key_.p, run_start_.p, run_end_.p, run_ord_.p,
                               st));
    BCHK(hipStreamSynchronize(st));  // the window's columns are decoded into again next
  }
  carry_key_ = v[hbam::kBaiLastKey];
  carry_sk_ = v[hbam::kBaiSkMax];
  records_ += n;
  runs_ += heads;
  return kOk;
}

int BaiBuilder::finish(BamFile& f, std::vector<uint8_t>* out, std::string* err) {
  hbam::Pipeline& p = f.pipe();
  const hipStream_t st = p.stream();
  const size_t n_ref = (size_t)f.n_ref();
  const uint64_t total = lin_off_[n_ref], R = runs_;
  std::vector<uint64_t> key(R), start(R), end(R), count(R), filled(total), unm(n_ref);
  std::vector<uint32_t> last(total);
  const uint64_t eof = f.file_size() << 16;  // (read by a copy queued below: alive until the synchronize)
  if (R) {
    // the run the last record belongs to ends with the file
    BCHK(hipMemcpyAsync(run_end_.p + (R - 1), &eof, 8, hipMemcpyHostToDevice, st));
    int end_bit = 17;  // bin + the bits of refID values 0 .. n_ref (n_ref: the unindexed runs, sorted last)
    while (end_bit < 64 && (n_ref >> (end_bit - 16)) != 0) ++end_bit;
    size_t tb = 0;
    BCHK(hbam::bai_sort_bytes(R, &tb));
    BCHK(tmp_.reserve(tb ? tb : 1));
    BCHK(s_key_.reserve(R));
    BCHK(iota_.reserve(R));
    BCHK(perm_.reserve(R));
    BCHK(s_start_.reserve(R));
    BCHK(s_end_.reserve(R));
    BCHK(s_count_.reserve(R));
    BCHK(hbam::launch_bai_sort(tmp_.p, tb, run_key_.p, s_key_.p, iota_.p, perm_.p, R, end_bit, st));
    BCHK(hbam::launch_bai_gather(perm_.p, run_start_.p, run_end_.p, run_ord_.p, R, records_, s_start_.p, s_end_.p,
                                 s_count_.p, st));
    BCHK(hipMemcpyAsync(key.data(), s_key_.p, 8 * R, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(start.data(), s_start_.p, 8 * R, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(end.data(), s_end_.p, 8 * R, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(count.data(), s_count_.p, 8 * R, hipMemcpyDeviceToHost, st));
  }
  if (total) {
    size_t tb = 0;
    BCHK(hbam::bai_fill_bytes(total, &tb));
    BCHK(tmp_.reserve(tb ? tb : 1));
    BCHK(ord_.reserve(total));
    BCHK(last_.reserve(total));
    BCHK(filled_.reserve(total));
    const hbam::BaiTables t{d_lin_off_.p, lin_.p, unm_.p, f.n_ref()};
    BCHK(hbam::launch_bai_fill(tmp_.p, tb, t, total, ord_.p, last_.p, filled_.p, st));
    BCHK(hipMemcpyAsync(filled.data(), filled_.p, 8 * total, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(last.data(), last_.p, 4 * total, hipMemcpyDeviceToHost, st));
  }
  if (n_ref) BCHK(hipMemcpyAsync(unm.data(), unm_.p, 8 * n_ref, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));

  out->clear();
  out->insert(out->end(), {'B', 'A', 'I', 1});
  put_le(out, (uint32_t)n_ref, 4);
  uint64_t k = 0, indexed = 0;
  for (size_t r = 0; r < n_ref; ++r) {
    uint64_t e = k;
    while (e < R && (key[e] >> 16) == r) ++e;
    uint32_t n_bin = 0;
    for (uint64_t i = k; i < e; ++i) n_bin += i == k || key[i] != key[i - 1];
    const bool meta = metadata_ && e > k;
    put_le(out, n_bin + (meta ? 1u : 0u), 4);
    uint64_t first = ~0ull, last_end = 0, recs = 0;
    for (uint64_t i = k; i < e;) {
      uint64_t j = i;
      while (j < e && key[j] == key[i]) ++j;
      put_le(out, key[i] & 0xffff, 4);
      put_le(out, j - i, 4);
      for (uint64_t c = i; c < j; ++c) {
        put_le(out, start[c], 8);
        put_le(out, end[c], 8);
        first = std::min(first, start[c]);
        last_end = std::max(last_end, end[c]);
        recs += count[c];
      }
      i = j;
    }
    if (meta) {  // SAM spec 5.2: the pseudo-bin's two "chunks"
      put_le(out, hbam::kBaiMetaBin, 4);
      put_le(out, 2, 4);
      put_le(out, first, 8);
      put_le(out, last_end, 8);
      put_le(out, recs - unm[r], 8);
      put_le(out, unm[r], 8);
    }
    indexed += recs;
    const uint32_t lo = lin_off_[r], m = last[lin_off_[r + 1] - 1];
    const uint32_t n_intv = m > lo ? m - lo : 0;
    put_le(out, n_intv, 4);
    for (uint32_t w = 0; w < n_intv; ++w) put_le(out, filled[lo + w], 8);
    k = e;
  }
  if (metadata_) put_le(out, records_ - indexed, 8);
  return kOk;
}

int BaiBuilder::build(BamFile& f, bool metadata, std::vector<uint8_t>* out, std::string* err) {
  int rc = begin(f, metadata, err);
  if (rc != kOk) return rc;
  const uint64_t fv = f.first_record_voff();
  Carry c{fv >> 16, fv & 0xffff};
  bool cont = false;
  // windows read from the host ramp up as in hbam_decode_span_device
  const bool ramp = !f.window_explicit() && !f.resident(fv >> 16, f.file_size());
  for (uint64_t nwin = 0;; ++nwin) {
    Step st;
    rc = ramp ? f.decode_step(c, ~0ull, hbam::kReader, true, cont, &st, SpanCursor::ramp_window(f.window_bytes(), nwin),
                              SpanCursor::ramp_window(f.window_bytes(), nwin + 1))
              : f.decode_step(c, ~0ull, hbam::kReader, true, cont, &st);
    if (rc != kOk) {
      *err = f.error();
      return rc;
    }
    // the records before a failing one are indexed first: an index error among them comes first in the file
    if ((rc = add_window(f, st.span, err)) != kOk) return rc;
    if (st.status != kOk) {
      *err = st.error;
      return st.status;
    }
    if (st.ended) break;
    c = st.next;
    cont = true;
  }
  return finish(f, out, err);
}

}  // namespace hadoop_bam
