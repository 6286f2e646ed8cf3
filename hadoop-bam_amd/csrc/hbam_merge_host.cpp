// hbam_merge_host.cpp -- host side of the merge of sorted runs (hbam_merge.h).
#include "hbam_merge.h"

#include <algorithm>

#include "hbam_launch.h"

namespace hbam {

#define MCHK(expr)                      \
  do {                                  \
    int _rc = hip_check((expr), #expr); \
    if (_rc != kOk) return _rc;         \
  } while (0)

Merger::Merger(Pipeline& p, int order) : p_(p), order_(order) {
  const StreamSet* o = &p.streams();
  off_.owner = word_.owner = word2_.owner = slen_.owner = doff_.owner = o;
  len_.owner = idx_.owner = perm_.owner = rank_.owner = flag_.owner = num_.owner = o;
  bad_.owner = o;
  names_.owner = name_len_.owner = tie_.owner = name_pos_.owner = o;
  tmp_.owner = stage_.owner = out_.owner = o;
  run_base_d_.owner = part_start_d_.owner = slice_base_d_.owner = src_pos_.owner = src_id_.owner = o;
  part_offs_.owner = o;
  part_first_d_.owner = cut_d_.owner = o;
  cut_off_d_.owner = o;
  run_base_.push_back(0);
  (void)hipSetDevice(p.device());
  for (auto& e : ev_)
    if (hipEventCreate(&e) != hipSuccess) e = nullptr;
}

Merger::~Merger() {
  (void)hipSetDevice(p_.device());
  (void)p_.streams().sync();
  for (auto& e : ev_)
    if (e) (void)hipEventDestroy(e);
}

int Merger::fail(int code, const std::string& msg) {
  err_ = msg;
  return code;
}

int Merger::hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return kOk;
  err_ = std::string(what) + ": " + hipGetErrorString(e);
  p_.rb_cancel();  // the failing call returns before its rb_sync: no queued read outlives its frame
  return kErrDevice;
}

int Merger::begin_run(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n) {
  has_pending_ = false;
  const std::string run = "run " + std::to_string(runs_.size());
  if (!offs || (len && !buf)) return fail(kErrArg, run + ": no buffer or no offsets");
  if (offs[n] != len)
    return fail(kErrArg, run + ": offs[n] = " + std::to_string(offs[n]) + " is not the run's length " +
                             std::to_string(len));
  if (total_ + n >= 0x7fffffffull) return fail(kErrArg, "too many records to merge (2^31 - 1 or more)");
  MCHK(hipSetDevice(p_.device()));
  hipStream_t s = p_.stream();
  const uint64_t k = runs_.size();
  // the run's n + 1 offsets behind the earlier runs' (run r's start at run_base[r] + r)
  MCHK(off_.grow(total_ + k + n + 1));
  if (order_ == kSortQueryname) {
    MCHK(name_pos_.grow(std::max<uint64_t>(total_ + n, 1)));
    MCHK(name_len_.grow(std::max<uint64_t>(total_ + n, 1)));
    MCHK(tie_.grow(std::max<uint64_t>(total_ + n, 1)));
  } else {
    MCHK(word_.grow(std::max<uint64_t>(total_ + n, 1)));
  }
  MCHK(len_.grow(std::max<uint64_t>(total_ + n, 1)));
  MCHK(idx_.grow(std::max<uint64_t>(total_ + n, 1)));
  MCHK(bad_.reserve(2));
  uint64_t* d_off = off_.p + total_ + k;
  MCHK(hipMemcpyAsync(d_off, offs, (n + 1) * 8, hipMemcpyHostToDevice, s));
  MCHK(hipMemsetAsync(bad_.p, 0xff, 2 * sizeof(unsigned long long), s));
  MCHK(launch_merge_check(d_off, n, len, nullptr, len_.p + total_, bad_.p, s));
  unsigned long long bad[2] = {~0ull, ~0ull};
  MCHK(p_.rb(bad, bad_.p, sizeof bad, s));
  MCHK(p_.rb_sync(s));
  if (bad[0] != ~0ull) {
    const uint64_t i = bad[0], a = offs[i], b = offs[i + 1];
    std::string why = b <= a ? "its offsets do not increase"
                      : b - a < kMergeMinRecord ? "it has " + std::to_string(b - a) + " bytes, fewer than 36"
                      : b > len ? "it ends past the run's length"
                                : "it is longer than 4 GiB";
    return fail(kErrArg, run + ": bad framing of record " + std::to_string(i) + ": " + why);
  }
  pending_ = Run{buf, len, n};
  has_pending_ = true;
  return kOk;
}

// The names of the run just decoded (span: its columns and its copy of the
// bytes): references, the order check on the decode's copy, then the names
// packed behind the earlier runs'.  Nothing of the run is kept before the check.
int Merger::finish_run_names(const Run& r, const SpanDev& span) {
  const std::string run = "run " + std::to_string(runs_.size());
  if (!span.col.flag || !span.col.l_read_name || !span.data || span.n != r.n)
    return fail(kErrState, run + ": no decoded columns");
  hipStream_t s = p_.stream();
  uint64_t* pos = name_pos_.p + total_;
  uint8_t* len = name_len_.p + total_;
  uint8_t* tie = tie_.p + total_;
  MCHK(launch_name_refs(span.rec_pos, span.col, r.n, pos, len, tie, nullptr, s));
  MCHK(hipMemsetAsync(bad_.p, 0xff, sizeof(unsigned long long), s));
  MCHK(launch_name_sorted(span.data, pos, len, tie, r.n, bad_.p, s));
  size_t tmp = 0;
  MCHK(merge_tmp_bytes(r.n, &tmp));
  MCHK(tmp_.reserve(tmp));
  MCHK(word_.reserve(r.n + 1));
  MCHK(word2_.reserve(r.n + 1));
  MCHK(launch_name_starts(tmp_.p, tmp, len, r.n, word_.p, word2_.p, s));
  unsigned long long bad = ~0ull;
  uint64_t bytes = 0;
  MCHK(p_.rb(&bad, bad_.p, sizeof bad, s));
  MCHK(p_.rb(&bytes, word2_.p + r.n, 8, s));
  MCHK(p_.rb_sync(s));
  if (bad != ~0ull)
    return fail(kErrArg, run + " is not sorted: record " + std::to_string(bad) + " sorts before record " +
                             std::to_string(bad - 1));
  MCHK(names_.grow(names_used_ + bytes + 8));
  MCHK(launch_name_pack(span.data, pos, len, word2_.p, r.n, names_.p, names_used_, s));
  names_used_ += bytes;
  return kOk;
}

int Merger::finish_run(const uint64_t* words, const SpanDev* span) {
  if (!has_pending_) return fail(kErrState, "no run begun");
  has_pending_ = false;
  const Run r = pending_;
  const std::string run = "run " + std::to_string(runs_.size());
  MCHK(hipSetDevice(p_.device()));
  hipStream_t s = p_.stream();
  const uint64_t k = runs_.size();
  const Columns* col = span ? &span->col : nullptr;
  if (r.n && order_ == kSortQueryname) {
    if (words) return fail(kErrArg, run + ": words given in queryname order");
    if (!span) return fail(kErrState, run + ": no decoded columns");
    const int rc = finish_run_names(r, *span);
    if (rc != kOk) return rc;
  } else if (r.n) {
    uint64_t* d_word = word_.p + total_;
    if (words) {
      MCHK(hipMemcpyAsync(d_word, words, r.n * 8, hipMemcpyHostToDevice, s));
    } else {
      if (!col || !col->key || !col->ref_id) return fail(kErrState, run + ": no words and no decoded columns");
      // (the lengths it writes are the decode's; the check below writes the framing's again)
      MCHK(launch_sort_words(*col, r.n, order_, d_word, len_.p + total_, idx_.p + total_, s));
    }
    MCHK(hipMemsetAsync(bad_.p, 0xff, 2 * sizeof(unsigned long long), s));
    MCHK(launch_merge_check(off_.p + total_ + k, r.n, r.len, d_word, len_.p + total_, bad_.p, s));
    unsigned long long bad[2] = {~0ull, ~0ull};
    MCHK(p_.rb(bad, bad_.p, sizeof bad, s));
    MCHK(p_.rb_sync(s));
    if (bad[1] != ~0ull)
      return fail(kErrArg, run + " is not sorted: record " + std::to_string(bad[1]) + " sorts before record " +
                               std::to_string(bad[1] - 1));
  }
  runs_.push_back(r);
  total_ += r.n;
  run_base_.push_back(total_);
  return kOk;
}

int Merger::plan(uint64_t part_bytes, uint64_t* n_parts, uint64_t* n_records, uint64_t* bytes) {
  *n_parts = *n_records = *bytes = 0;
  planned_ = true;
  has_pending_ = false;
  parts_ = next_part_ = bytes_ = 0;
  plan_ms[0] = plan_ms[1] = plan_ms[2] = 0;
  const uint64_t n = total_;
  const uint32_t k = (uint32_t)runs_.size();
  if (n == 0) return kOk;
  MCHK(hipSetDevice(p_.device()));
  hipStream_t s = p_.stream();
  size_t tmp = 0;
  MCHK(merge_tmp_bytes(n, &tmp));
  MCHK(tmp_.reserve(tmp));
  MCHK(word2_.reserve(n));
  MCHK(perm_.reserve(n));
  MCHK(slen_.reserve(n + 1));
  MCHK(doff_.reserve(n + 1));
  MCHK(hipEventRecord(ev_[0], s));
  if (order_ == kSortQueryname) {
    MCHK(word_.reserve(n));
    const int rc = p_.name_order(tmp_.p, tmp, names_.p, name_pos_.p, name_len_.p, tie_.p, n, word_.p, word2_.p,
                                 idx_.p, perm_.p);
    if (rc != kOk) return fail(rc, p_.error());
  } else {
    MCHK(launch_merge_perm(tmp_.p, tmp, word_.p, word2_.p, idx_.p, perm_.p, n, s));
  }
  MCHK(hipEventRecord(ev_[1], s));
  MCHK(launch_sort_offsets(tmp_.p, tmp, len_.p, perm_.p, n, slen_.p, doff_.p, s));
  MCHK(hipEventRecord(ev_[2], s));
  MCHK(p_.rb(&bytes_, doff_.p + n, 8, s));
  MCHK(p_.rb_sync(s));
  // the words, the lengths and the sort's input index have served
  word_.release();
  word2_.release();
  slen_.release();
  len_.release();
  idx_.release();
  MCHK(flag_.reserve(n + 1));
  MCHK(num_.reserve(n + 1));
  MCHK(launch_merge_heads(tmp_.p, tmp, doff_.p, n, part_bytes, flag_.p, num_.p, s));
  uint32_t parts = 0;
  MCHK(p_.rb(&parts, num_.p + n, 4, s));
  MCHK(p_.rb_sync(s));
  parts_ = parts;
  const uint64_t pairs = (parts_ + 1) * k;
  MCHK(rank_.reserve(n));
  MCHK(run_base_d_.reserve(k + 1));
  MCHK(part_first_d_.reserve(parts_ + 1));
  MCHK(part_start_d_.reserve(parts_ + 1));
  MCHK(cut_d_.reserve(pairs));
  MCHK(cut_off_d_.reserve(pairs));
  MCHK(hipMemcpyAsync(run_base_d_.p, run_base_.data(), (k + 1) * 8, hipMemcpyHostToDevice, s));
  MCHK(launch_merge_cuts(flag_.p, num_.p, doff_.p, perm_.p, n, run_base_d_.p, k, parts_, part_first_d_.p,
                         part_start_d_.p, rank_.p, off_.p, cut_d_.p, cut_off_d_.p, s));
  MCHK(hipEventRecord(ev_[3], s));
  part_first_.resize(parts_ + 1);
  part_start_.resize(parts_ + 1);
  cut_.resize(pairs);
  cut_off_.resize(pairs);
  MCHK(hipMemcpyAsync(part_first_.data(), part_first_d_.p, (parts_ + 1) * 4, hipMemcpyDeviceToHost, s));
  MCHK(hipMemcpyAsync(part_start_.data(), part_start_d_.p, (parts_ + 1) * 8, hipMemcpyDeviceToHost, s));
  MCHK(hipMemcpyAsync(cut_.data(), cut_d_.p, pairs * 4, hipMemcpyDeviceToHost, s));
  MCHK(hipMemcpyAsync(cut_off_.data(), cut_off_d_.p, pairs * 8, hipMemcpyDeviceToHost, s));
  MCHK(hipStreamSynchronize(s));
  for (int i = 0; i < 3; ++i) MCHK(hipEventElapsedTime(&plan_ms[i], ev_[i], ev_[i + 1]));
  rank_.release();
  flag_.release();
  num_.release();
  tmp_.release();
  cut_d_.release();
  cut_off_d_.release();
  part_first_d_.release();
  part_start_d_.release();
  MCHK(slice_base_d_.reserve(k));
  slice_base_.assign(k, 0);
  *n_parts = parts_;
  *n_records = n;
  *bytes = bytes_;
  return kOk;
}

int Merger::next(uint8_t* out, uint64_t cap, uint64_t* offs, uint64_t* src, uint64_t* n, uint64_t* len) {
  *n = *len = 0;
  if (next_part_ >= parts_) {
    if (out && offs) offs[0] = 0;
    return kOk;
  }
  const uint64_t p = next_part_;
  const uint32_t k = (uint32_t)runs_.size();
  const uint64_t j0 = part_first_[p], m = part_first_[p + 1] - j0;
  const uint64_t dbase = part_start_[p], bytes = part_start_[p + 1] - dbase;
  *n = m;
  *len = bytes;
  if (!out) return kOk;
  if (cap < bytes) return fail(kErrArg, "output buffer too small for the part");
  MCHK(hipSetDevice(p_.device()));
  hipStream_t s = p_.stream();
  // 16 bytes past the last slice for the gather's two-load chunks, and the
  // round-up of the staging positions to 16
  MCHK(stage_.reserve(bytes + 64));
  MCHK(out_.reserve((bytes + 15) & ~15ull));
  MCHK(src_pos_.reserve(m));
  MCHK(src_id_.reserve(m));
  MCHK(part_offs_.reserve(m + 1));
  MCHK(hipEventRecord(ev_[0], s));
  uint64_t at = 0;
  for (uint32_t r = 0; r < k; ++r) {
    const uint64_t a = cut_[p * k + r], b = cut_[(p + 1) * k + r];
    slice_base_[r] = 0;
    if (a == b) continue;
    const Run& R = runs_[r];
    // the offsets the device checked and the source table is built from (not the caller's array again)
    const uint64_t lo = cut_off_[p * k + r], hi = cut_off_[(p + 1) * k + r];
    if (hi <= lo || hi > R.len || at + (hi - lo) > bytes) return fail(kErrState, "the part's slices exceed its bytes");
    MCHK(hipMemcpyAsync(stage_.p + at, R.buf + lo, hi - lo, hipMemcpyHostToDevice, s));
    slice_base_[r] = at - lo;  // modulo 2^64: + a record's offset = its staging position
    at += hi - lo;
  }
  if (at != bytes) return fail(kErrState, "the part's slices do not add up to its bytes");
  MCHK(hipMemsetAsync(stage_.p + bytes, 0, 32, s));
  MCHK(hipMemcpyAsync(slice_base_d_.p, slice_base_.data(), k * 8, hipMemcpyHostToDevice, s));
  MCHK(hipEventRecord(ev_[1], s));
  MCHK(launch_merge_src(perm_.p + j0, doff_.p + j0, m, dbase, run_base_d_.p, k, off_.p, slice_base_d_.p, src_pos_.p,
                        src_id_.p, part_offs_.p, s));
  MCHK(launch_merge_gather(stage_.p, src_pos_.p, doff_.p + j0, m, dbase, bytes, out_.p, s));
  MCHK(hipEventRecord(ev_[2], s));
  MCHK(hipMemcpyAsync(out, out_.p, bytes, hipMemcpyDeviceToHost, s));
  if (offs) MCHK(hipMemcpyAsync(offs, part_offs_.p, (m + 1) * 8, hipMemcpyDeviceToHost, s));
  if (src) MCHK(hipMemcpyAsync(src, src_id_.p, m * 8, hipMemcpyDeviceToHost, s));
  MCHK(hipEventRecord(ev_[3], s));
  MCHK(hipStreamSynchronize(s));
  for (int i = 0; i < 3; ++i) MCHK(hipEventElapsedTime(&part_ms[i], ev_[i], ev_[i + 1]));
  ++next_part_;
  return kOk;
}

}  // namespace hbam
