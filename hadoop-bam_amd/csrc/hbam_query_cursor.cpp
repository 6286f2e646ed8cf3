// hbam_query_cursor.cpp -- QueryCursor: bounded traversal behind hbam_query_intervals
// / hbam_query_unmapped / hbam_query_next (BAMRecordReader.java:170-178).
//
// Per chunk the window loop of hbam_decode_span_device (BamFile::decode_step
// from the chunk's start, the next record's position carried across windows);
// per window the filter kernels of hbam_query.h, one read-back of the window's
// verdict (stop record, carry, kept records and bytes), the gather into a
// compact buffer and its copy into page-locked host columns.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "hbam_host.h"
#include "hbam_query.h"

namespace hadoop_bam {

using hbam::ColLayout;
using hbam::kErrArg;
using hbam::kErrDevice;
using hbam::kErrNoMem;
using hbam::kErrState;
using hbam::kOk;

namespace {
int hip_err(hipError_t e, const char* what, std::string* err) {
  if (e == hipSuccess) return kOk;
  *err = std::string(what) + ": " + hipGetErrorString(e);
  return kErrDevice;
}
#define QCHK(expr)                               \
  do {                                           \
    const int _rc = hip_err((expr), #expr, err); \
    if (_rc != kOk) return _rc;                  \
  } while (0)
// Rest bytes a bounded batch may hand out: below 2 GiB, the largest direct
// ByteBuffer a JNI caller wraps them in (GpuBAMRecordReader.recordAt uses int
// positions); the rule of SpanCursor's batches (HBAM_MAX_BATCH_BYTES lowers
// it, for tests).
uint64_t batch_data_cap() {
  const char* e = getenv("HBAM_MAX_BATCH_BYTES");
  const uint64_t hard = (1ull << 31) - 1024;
  const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
  return v && v < hard ? v : hard;
}
}  // namespace

int QueryCursor::begin(BamFile& f, std::string* err) {
  const hbam::StreamSet* o = &f.pipe().streams();
  iv_.owner = aend_.owner = p_.owner = idx_.owner = flag_.owner = slot_.owner = klen_.owner = roff_.owner =
      src_off_.owner = state_.owner = tmp_.owner = cols_.owner = rests_.owner = o;
  QCHK(hipSetDevice(f.pipe().device()));
  QCHK(state_.reserve(hbam::kQueryStateWords));
  return kOk;
}

int check_intervals_optimized(const QueryInterval* iv, uint64_t n_iv, std::string* err) {
  if (n_iv >= (1ull << 31)) {
    *err = "too many intervals";
    return kErrArg;
  }
  // [htsjdk] assertIntervalsOptimized: sorted, and neither overlapping nor abutting
  for (uint64_t k = 0; k < n_iv; ++k) {
    const int32_t end = iv[k].end <= 0 ? INT32_MAX : iv[k].end;
    if (k) {
      const int32_t pend = iv[k - 1].end <= 0 ? INT32_MAX : iv[k - 1].end;
      if (iv[k].ref_id < iv[k - 1].ref_id || (iv[k].ref_id == iv[k - 1].ref_id && iv[k].start <= pend)) {
        *err = "query intervals are not optimized: sort them and merge overlapping ones";
        return kErrArg;
      }
    }
    // an interval ending more than one base before its start would break the
    // order of the interval ends (BEFORE must hold for a prefix of them)
    if ((int64_t)end < (int64_t)iv[k].start - 1) {
      *err = "query interval ends before it starts";
      return kErrArg;
    }
  }
  return kOk;
}

int QueryCursor::open_intervals(BamFile& f, const QueryInterval* iv, uint64_t n_iv, const uint64_t* ptrs,
                                uint64_t n_ptrs, std::string* err) {
  int rc = check_intervals_optimized(iv, n_iv, err);
  if (rc != kOk) return rc;
  std::vector<int32_t> h(3 * n_iv);  // ref | start | effective end
  for (uint64_t k = 0; k < n_iv; ++k) {
    h[k] = iv[k].ref_id;
    h[n_iv + k] = iv[k].start;
    h[2 * n_iv + k] = iv[k].end <= 0 ? INT32_MAX : iv[k].end;
  }
  if (n_ptrs & 1) {
    *err = "file pointers come in pairs (chunk start, chunk end)";
    return kErrArg;
  }
  chunks_.clear();
  for (uint64_t k = 0; k < n_ptrs; k += 2) {
    if (ptrs[k] > ptrs[k + 1] || (k && ptrs[k] < ptrs[k - 1])) {
      *err = "file pointer chunks are not in ascending order";
      return kErrArg;
    }
    chunks_.emplace_back(ptrs[k], ptrs[k + 1]);
  }
  if ((rc = begin(f, err)) != kOk) return rc;
  unmapped_ = false;
  n_iv_ = (uint32_t)n_iv;
  if (n_iv) {
    const hipStream_t s = f.pipe().stream();
    QCHK(iv_.reserve(3 * n_iv));
    QCHK(hipMemcpyAsync(iv_.p, h.data(), 12 * n_iv, hipMemcpyHostToDevice, s));
    QCHK(hipStreamSynchronize(s));  // h is pageable and local
  }
  done_ = n_iv == 0;  // no interval: the first record already ends the iteration (nothing is read)
  return kOk;
}

int QueryCursor::open_unmapped(BamFile& f, uint64_t start_voff, std::string* err) {
  int rc = begin(f, err);
  if (rc != kOk) return rc;
  unmapped_ = true;
  chunks_.assign(1, {start_voff, ~0ull});
  return kOk;
}

int QueryCursor::filter(BamFile& f, const SpanDev& s, HostBatch* h, bool* stop, std::string* err) {
  *stop = false;
  const uint64_t n = s.n;
  if (n == 0) return kOk;
  if (n >= (uint64_t)INT_MAX - 1) {
    *err = "too many records in one window for the query scans";
    return kErrState;
  }
  hbam::Pipeline& p = f.pipe();
  const hipStream_t st = p.stream();
  const uint8_t* u = s.data ? s.data : p.d_u();
  size_t tb = 0;
  QCHK(hbam::query_scan_bytes(n + 1, &tb));
  QCHK(tmp_.reserve(tb ? tb : 1));
  QCHK(flag_.reserve(n + 1));
  QCHK(slot_.reserve(n + 1));
  QCHK(klen_.reserve(n + 1));
  QCHK(roff_.reserve(n + 1));
  QCHK(hipMemsetAsync(state_.p, 0xff, 8 * hbam::kQueryStateWords, st));
  if (unmapped_) {
    QCHK(hbam::launch_query_unmapped(s.col, n, found_, flag_.p, klen_.p, state_.p, st));
  } else {
    QCHK(aend_.reserve(n));
    QCHK(p_.reserve(n));
    QCHK(idx_.reserve(n));
    const hbam::QueryIntervals iv{iv_.p, iv_.p + n_iv_, iv_.p + 2ull * n_iv_, n_iv_};
    QCHK(hbam::launch_query_classify(u, s.col, n, iv, carry_, aend_.p, p_.p, st));
    QCHK(hbam::launch_query_scan(tmp_.p, tb, p_.p, idx_.p, n, st));
    QCHK(hbam::launch_query_select(s.col, aend_.p, idx_.p, n, iv, flag_.p, klen_.p, state_.p, st));
  }
  QCHK(hbam::launch_query_offsets(tmp_.p, tb, flag_.p, slot_.p, klen_.p, roff_.p, n, state_.p, st));
  uint64_t v[hbam::kQueryStateWords];
  hipError_t e = p.rb(v, state_.p, sizeof v, st);
  if (e == hipSuccess) e = p.rb_sync(st);
  if (e != hipSuccess) {
    p.rb_cancel();  // v is a local: the queue must not keep its address
    return hip_err(e, "read-back of the query state", err);
  }
  if (unmapped_) {
    if (v[hbam::kQueryStop] != ~0ull) found_ = true;
  } else {
    *stop = v[hbam::kQueryStop] != ~0ull;
    carry_ = (uint32_t)v[hbam::kQueryCarry];
  }
  const uint64_t kept = v[hbam::kQueryKept], bytes = v[hbam::kQueryBytes];
  if (kept == 0) return kOk;
  const ColLayout L(kept, false);
  QCHK(cols_.reserve(L.bytes));
  QCHK(rests_.reserve(bytes + 16));
  QCHK(src_off_.reserve(kept));
  const hbam::Columns d = L.at(cols_.p, nullptr);
  QCHK(hbam::launch_query_compact(u, s.col, n, flag_.p, slot_.p, roff_.p, d, kept, src_off_.p, rests_.p, st));
  // the compact records -> h at record h->n (page-locked columns, as fetch_span)
  const uint64_t n0 = h->n, d0 = h->data_len;
  if (h->reserve(n0 + kept, d0 + bytes) != kOk) {
    (void)hipStreamSynchronize(st);
    *err = "page-locked host memory for the batch";
    return kErrNoMem;
  }
  bool ok = true;
  auto cp = [&](auto& vec, const auto* src) {
    ok = ok && hipMemcpyAsync(vec.data() + n0, src, kept * sizeof(vec[0]), hipMemcpyDeviceToHost, st) == hipSuccess;
  };
  cp(h->ref_id, d.ref_id);
  cp(h->pos, d.pos);
  cp(h->l_seq, d.l_seq);
  cp(h->next_ref_id, d.next_ref_id);
  cp(h->next_pos, d.next_pos);
  cp(h->tlen, d.tlen);
  cp(h->l_read_name, d.l_read_name);
  cp(h->mapq, d.mapq);
  cp(h->bin, d.bin);
  cp(h->n_cigar, d.n_cigar);
  cp(h->flag, d.flag);
  cp(h->key, d.key);
  cp(h->voff, d.voff);
  cp(h->rest_off, d.rest_off);
  cp(h->rest_len, d.rest_len);
  if (bytes)
    ok = ok && hipMemcpyAsync(h->data.data() + d0, rests_.p, bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
  const bool drained = hipStreamSynchronize(st) == hipSuccess;  // always: the pinned columns may be freed next
  if (!ok || !drained) {
    *err = "hipMemcpy D2H failed";
    return kErrDevice;
  }
  for (uint64_t i = n0; i < n0 + kept; ++i) h->rest_off[i] += d0;
  h->n = n0 + kept;
  h->data_len = d0 + bytes;
  return kOk;
}

int QueryCursor::advance(BamFile& f, HostBatch* h, bool all, std::string* err) {
  const uint64_t n0 = h->n;
  while (!done_ && (all || h->n == n0)) {
    if (chunk_ >= chunks_.size()) {
      done_ = true;
      break;
    }
    const uint64_t vend = chunks_[chunk_].second;
    if (!in_chunk_) {  // a seek to the chunk's start
      c_ = Carry{chunks_[chunk_].first >> 16, chunks_[chunk_].first & 0xffff};
      cont_ = false;
      in_chunk_ = true;
    }
    Step st;
    int rc = f.decode_step(c_, vend, hbam::kReader, true, cont_, &st, f.dropin_window_bytes());
    if (rc != kOk) {
      *err = f.error();
      done_ = true;
      return rc;
    }
    bool stop = false;
    rc = filter(f, st.span, h, &stop, err);
    if (rc != kOk) {
      done_ = true;
      return rc;
    }
    if (stop) {
      done_ = true;  // the record that failed (if any) lies after the stop record: never read
    } else if (st.status != kOk) {
      status_ = st.status;
      status_err_ = st.error;
      done_ = true;
    } else if (st.ended) {
      ++chunk_;
      in_chunk_ = false;
    } else {
      c_ = st.next;
      cont_ = true;
    }
  }
  return kOk;
}

int QueryCursor::next_batch(BamFile& f, uint64_t max_records, BatchView* out, std::string* err) {
  *out = BatchView();
  int rc = kOk;
  if (max_records == 0) {
    // the rest of the last window's records, then every window to the end
    HostBatch& a = all_;
    a.n = 0;
    a.data_len = 0;
    if (k_ < win_.n) {
      const uint64_t m = win_.n - k_, base = win_.rest_off[k_], bytes = win_.data_len - base;
      if (a.reserve(m, bytes) != kOk) {
        *err = "page-locked host memory for the batch";
        return kErrNoMem;
      }
      auto cp = [&](auto& dst, const auto& src) { memcpy(dst.data(), src.data() + k_, m * sizeof(dst[0])); };
      cp(a.ref_id, win_.ref_id);
      cp(a.pos, win_.pos);
      cp(a.l_seq, win_.l_seq);
      cp(a.next_ref_id, win_.next_ref_id);
      cp(a.next_pos, win_.next_pos);
      cp(a.tlen, win_.tlen);
      cp(a.l_read_name, win_.l_read_name);
      cp(a.mapq, win_.mapq);
      cp(a.bin, win_.bin);
      cp(a.n_cigar, win_.n_cigar);
      cp(a.flag, win_.flag);
      cp(a.key, win_.key);
      cp(a.voff, win_.voff);
      cp(a.rest_len, win_.rest_len);
      for (uint64_t i = 0; i < m; ++i) a.rest_off[i] = win_.rest_off[k_ + i] - base;
      memcpy(a.data.data(), win_.data.data() + base, bytes);
      a.n = m;
      a.data_len = bytes;
    }
    win_.n = 0;
    win_.data_len = 0;
    k_ = 0;
    if ((rc = advance(f, &a, true, err)) != kOk) return rc;
    *out = BatchView::of(a);
  } else {
    if (k_ >= win_.n) {
      win_.n = 0;
      win_.data_len = 0;
      k_ = 0;
      if ((rc = advance(f, &win_, false, err)) != kOk) return rc;
    }
    uint64_t m = std::min(max_records, win_.n - k_);
    if (m) {
      // the slice's rests start at its first record's: rest_off from there
      const uint64_t base = win_.rest_off[k_];
      // ... and stay under the cap: the largest m' <= m whose rests do (one
      // record at least); rest_off past the slice is still window-relative
      auto rests_end = [&](uint64_t e) { return e < win_.n ? win_.rest_off[e] : win_.data_len; };
      if (m > 1 && rests_end(k_ + m) - base > batch_data_cap()) {
        const uint64_t cap = batch_data_cap();
        uint64_t lo = 1, hi = m;  // lo records fit (one always goes), hi do not
        while (hi - lo > 1) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (rests_end(k_ + mid) - base <= cap) lo = mid; else hi = mid;
        }
        m = lo;
      }
      const uint64_t end = k_ + m < win_.n ? win_.rest_off[k_ + m] : win_.data_len;
      for (uint64_t i = k_; i < k_ + m; ++i) win_.rest_off[i] -= base;
      BatchView v = BatchView::of(win_);
      out->n = m;
      out->ref_id = v.ref_id + k_;
      out->pos = v.pos + k_;
      out->l_seq = v.l_seq + k_;
      out->next_ref_id = v.next_ref_id + k_;
      out->next_pos = v.next_pos + k_;
      out->tlen = v.tlen + k_;
      out->l_read_name = v.l_read_name + k_;
      out->mapq = v.mapq + k_;
      out->bin = v.bin + k_;
      out->n_cigar = v.n_cigar + k_;
      out->flag = v.flag + k_;
      out->key = v.key + k_;
      out->voff = v.voff + k_;
      out->rest_off = v.rest_off + k_;
      out->rest_len = v.rest_len + k_;
      out->data = v.data + base;
      out->data_len = end - base;
      k_ += m;
    }
  }
  // the failing record's status, once the records before it are all handed out
  if (status_ != kOk && done_ && k_ >= win_.n) {
    *err = status_err_;
    return status_;
  }
  return kOk;
}

}  // namespace hadoop_bam
