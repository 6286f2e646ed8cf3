// hbam_merge.h -- the merge of k sorted runs of SAMRecordWritable encodings
// (hbam_merge_*): the reduce side of the reference's sort job, Hadoop's merge
// of the sorted map outputs.  The run bytes stay in the caller's host memory;
// the sort word, the framing and the order of every record live in HBM, in
// buffers this object owns (never the Pipeline's sort_* temporaries: a
// sort_writables between two runs leaves them alone).  In queryname order there
// is no sort word: every record's name bytes are kept instead, packed, with
// where they start, their length and the tie word (name bytes + 10 B per
// record until the merge ends).  The order is planned
// once on the device (kernels of hbam_merge.hip); each part is then staged
// host -> HBM as k contiguous slices, gathered and copied back.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "hbam_pipeline.h"

namespace hbam {

class Merger {
 public:
  Merger(Pipeline& p, int order);
  Merger(const Merger&) = delete;
  Merger& operator=(const Merger&) = delete;

  bool planned() const { return planned_; }
  int order() const { return order_; }
  const std::string& error() const { return err_; }

  // A run in two steps, nothing kept if either fails.  begin_run: the framing
  // to HBM and checked (offs: n + 1 entries, offs[n] == len).  finish_run: the
  // words -- the caller's, or k_sort_words of the columns of a decode of the
  // same values (span) -- checked to be non-decreasing; the run is then added.
  // Queryname order: words == nullptr; the names are read from the decode's
  // copy of the run (span->data), checked to be in order and packed.
  int begin_run(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n);
  int finish_run(const uint64_t* words, const SpanDev* span);
  // The order, the output starts, the parts (part_bytes > 0) and the cut table.
  int plan(uint64_t part_bytes, uint64_t* n_parts, uint64_t* n_records, uint64_t* bytes);
  // The next part: out == nullptr sizes it (*n, *len) and keeps it; else its
  // bytes, offs (nullptr or n + 1, relative to the part) and src (nullptr or n:
  // run << 32 | record).  Past the last part: *n = *len = 0.
  int next(uint8_t* out, uint64_t cap, uint64_t* offs, uint64_t* src, uint64_t* n, uint64_t* len);

  // HIP-event times of the last plan (word-to-order sort, output starts,
  // parts + cuts) and of the last written part (H2D of the slices, source
  // table + gather, D2H), in milliseconds: measurements
  float plan_ms[3] = {0, 0, 0};
  float part_ms[3] = {0, 0, 0};

 private:
  struct Run {
    const uint8_t* buf;
    uint64_t len, n;
  };
  int fail(int code, const std::string& msg);
  int hip_check(hipError_t e, const char* what);
  int finish_run_names(const Run& r, const SpanDev& span);

  Pipeline& p_;
  int order_;
  bool planned_ = false;
  std::string err_;
  std::vector<Run> runs_;
  std::vector<uint64_t> run_base_;  // k + 1: the global index of each run's first record
  uint64_t total_ = 0;              // records of the runs added
  Run pending_{};                   // between begin_run and finish_run
  bool has_pending_ = false;

  // per record, run-major, alive from the first run to the end: framing
  // (n_r + 1 per run) and, until the plan, words, lengths and the sort's input index
  DevBuf<uint64_t> off_, word_;
  DevBuf<uint32_t> len_, idx_;
  DevBuf<unsigned long long> bad_;
  // queryname order, alive to the end: the names back to back (names_used_
  // bytes, 8 readable past them), each record's start in them, length and tie word
  DevBuf<uint8_t> names_, name_len_, tie_;
  DevBuf<uint64_t> name_pos_;
  uint64_t names_used_ = 0;
  // the plan: sorted words, output starts (+ the lengths they are summed from),
  // order and its inverse, part flags / numbers, hipcub storage
  DevBuf<uint64_t> word2_, slen_, doff_;
  DevBuf<uint32_t> perm_, rank_, flag_, num_;
  DevBuf<uint8_t> tmp_;
  DevBuf<uint64_t> run_base_d_, part_start_d_, cut_off_d_;
  DevBuf<uint32_t> part_first_d_, cut_d_;
  std::vector<uint32_t> part_first_, cut_;  // parts + 1; (parts + 1) * k
  std::vector<uint64_t> part_start_;        // parts + 1
  std::vector<uint64_t> cut_off_;           // (parts + 1) * k: the runs' offsets at the cuts
  uint64_t parts_ = 0, next_part_ = 0, bytes_ = 0;
  // one part: the staged slices, each run's base in them, the source table,
  // (run, record) names, relative starts, the gathered bytes
  DevBuf<uint8_t> stage_, out_;
  DevBuf<uint64_t> slice_base_d_, src_pos_, src_id_, part_offs_;
  std::vector<uint64_t> slice_base_;
  hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};

 public:
  ~Merger();
};

}  // namespace hbam
