// hbam_bai_index.cpp -- reading a .bai (SAM spec 5.2) on the host: the parser
// shared by the BAI split calculator (LinearBAMIndex) and by
// hbam_bai_summarize / hbam_bai_query, and the chunk side of
// BAMInputFormat.filterByInterval (BAMInputFormat.java:571-574).  No device.
#include <algorithm>
#include <climits>
#include <cstring>

#include "hbam_bai.h"
#include "hbam_host.h"

namespace hadoop_bam {

using hbam::kErrArg;
using hbam::kErrFormat;
using hbam::kOk;

namespace {
int32_t le_i32(const uint8_t* p) {
  int32_t v;
  memcpy(&v, p, 4);
  return v;
}
uint64_t le_u64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
}  // namespace

int BaiIndex::parse(const uint8_t* data, uint64_t len, std::string* err) {
  d = data;
  refs.clear();
  has_no_coor = false;
  no_coor = 0;
  uint64_t p = 0;
  auto need = [&](uint64_t k) { return k <= len - p; };  // (p <= len throughout)
  auto fail = [&](const char* m) {
    *err = m;
    return kErrFormat;
  };
  if (len < 8 || memcmp(data, "BAI\1", 4) != 0) return fail("Invalid file header in BAM index");
  const int32_t n_ref = le_i32(data + 4);
  p = 8;
  if (n_ref < 0) return fail("Invalid BAM index: negative reference count");
  if ((uint64_t)n_ref > (len - p) / 8) return fail("Premature end of BAM index");  // 8 bytes per contig at least
  refs.resize((size_t)n_ref);
  for (Ref& r : refs) {
    if (!need(4)) return fail("Premature end of BAM index");
    r.n_bin = le_i32(data + p);
    p += 4;
    r.bins = p;  // (a negative count reads as no bins)
    for (int32_t b = 0; b < r.n_bin; ++b) {
      if (!need(8)) return fail("Premature end of BAM index");
      const int32_t n_chunk = le_i32(data + p + 4);
      p += 8;
      if (n_chunk < 0 || !need(16ull * (uint64_t)n_chunk)) return fail("Premature end of BAM index");
      p += 16ull * (uint64_t)n_chunk;
    }
    if (!need(4)) return fail("Premature end of BAM index");
    r.n_intv = le_i32(data + p);
    p += 4;
    if (r.n_intv < 0 || !need(8ull * (uint64_t)r.n_intv)) return fail("Premature end of BAM index");
    r.lin = p;
    p += 8ull * (uint64_t)r.n_intv;
  }
  if (need(8)) {  // the optional count of records without coordinates
    has_no_coor = true;
    no_coor = le_u64(data + p);
  }
  return kOk;
}

uint64_t BaiIndex::lin_at(const Ref& r, int32_t w) const { return le_u64(d + r.lin + 8ull * (uint64_t)w); }

int64_t BaiIndex::start_of_last_linear_bin() const {
  for (size_t k = refs.size(); k-- > 0;)
    if (refs[k].n_intv > 0) return (int64_t)lin_at(refs[k], refs[k].n_intv - 1);
  return -1;
}

int BaiIndex::query(const QueryInterval* iv, uint64_t n_iv, std::vector<uint64_t>* out, std::string* err) const {
  out->clear();
  int rc = check_intervals_optimized(iv, n_iv, err);
  if (rc != kOk) return rc;
  std::vector<std::pair<uint64_t, uint64_t>> ch;
  for (uint64_t k = 0; k < n_iv; ++k) {
    if (iv[k].ref_id < 0 || (size_t)iv[k].ref_id >= refs.size()) {
      *err = "query interval on a reference the index does not have: " + std::to_string(iv[k].ref_id);
      return kErrArg;
    }
    const Ref& r = refs[(size_t)iv[k].ref_id];
    const int64_t beg = std::max<int64_t>((int64_t)iv[k].start - 1, 0);
    const int64_t end = (iv[k].end <= 0 ? hbam::kBaiMaxEnd : (int64_t)iv[k].end) - 1;  // inclusive
    // the linear entry of the interval's first window (past the table: the last one)
    const int64_t w = beg >> hbam::kBaiLinShift;
    const uint64_t min_off = r.n_intv == 0 ? 0 : lin_at(r, (int32_t)std::min<int64_t>(w, r.n_intv - 1));
    // reg2bins (SAM spec 5.3): bin 0 and, per level, the bins of beg .. end
    auto wanted = [&](uint32_t b) {
      if (b == hbam::kBaiMetaBin) return false;
      if (b == 0) return true;
      static const int shift[5] = {26, 23, 20, 17, 14};
      static const int64_t first[5] = {1, 9, 73, 585, 4681};
      for (int l = 0; l < 5; ++l)
        if ((int64_t)b >= first[l] + (beg >> shift[l]) && (int64_t)b <= first[l] + (end >> shift[l])) return true;
      return false;
    };
    uint64_t p = r.bins;
    for (int32_t b = 0; b < r.n_bin; ++b) {
      uint32_t bin;
      memcpy(&bin, d + p, 4);
      const int32_t n_chunk = le_i32(d + p + 4);
      p += 8;
      if (wanted(bin))
        for (int32_t c = 0; c < n_chunk; ++c) {
          const uint64_t a = le_u64(d + p + 16ull * (uint64_t)c), e = le_u64(d + p + 16ull * (uint64_t)c + 8);
          if (e > min_off) ch.emplace_back(a, e);
        }
      p += 16ull * (uint64_t)n_chunk;
    }
  }
  // sorted, and merged where a chunk starts at or before the end of the one
  // before it (merging per interval first gives the same union)
  std::sort(ch.begin(), ch.end());
  for (const auto& c : ch) {
    if (!out->empty() && c.first <= out->back()) {
      out->back() = std::max(out->back(), c.second);
    } else {
      out->push_back(c.first);
      out->push_back(c.second);
    }
  }
  return kOk;
}

}  // namespace hadoop_bam
