// hbam_bai.h -- launch wrappers of the BAM index (.bai, SAM spec 5.2) kernels
// (hbam_bai.hip): the per-record pass of an indexer over one decoded window
// and the passes that finish the index.
//
// Per record i of the file, in file order:
//   indexed_i = refID >= 0 and pos >= 0
//   end_i     = pos + 1 for a placed unmapped read (flag 0x4), else
//               pos + max(reference length of the cigar, 1)
//   key_i     = refID << 16 | reg2bin(pos, end)   (kUnindexed: n_ref << 16)
//   windows   = max(pos - 1, 0) >> 14 for a placed unmapped read, else
//               pos >> 14 .. (end - 1) >> 14
// A chunk is a maximal run of consecutive records with one key; it starts at
// its first record's voff and ends at the voff of the record after its last.
// So the records where the key changes (the boundaries, an unindexed record
// after an indexed one among them) are compacted into a run list, and each
// boundary also closes the run before it -- in the same window or in an
// earlier one.  A window's linear entry is the smallest voff of the records
// touching it; a record leaves out the windows its predecessor touches too
// (the predecessor's voff is smaller), so a deep pile-up costs no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbam_device.h"

namespace hbam {

constexpr int64_t kBaiMaxEnd = 1ll << 29;  // the largest coordinate the bin scheme addresses
constexpr uint32_t kBaiLinShift = 14;      // 16 kbp linear windows
constexpr uint32_t kBaiMetaBin = 37450;    // the metadata pseudo-bin

// Per-window results the host reads back (u64 each).
enum : int {
  kBaiErr = 0,      // min (record index << 2 | BaiError) over the window's failing records; ~0 = none
  kBaiLastKey = 1,  // key of the window's last record: the next window's carry-in
  kBaiSkMax = 2,    // max sort key so far (carry-in included)
  kBaiHeads = 3,    // boundaries of the window
  kBaiStateWords = 4,
};
enum BaiError : int {
  kBaiErrOrder = 0,   // an indexed record sorts before an earlier one
  kBaiErrEnd = 1,     // end > 2^29
  kBaiErrWindow = 2,  // a window beyond the contig's table (the header's l_ref)
  kBaiErrRef = 3,     // refID >= n_ref
};

// The tables that live across windows.
struct BaiTables {
  const uint32_t* lin_off;  // n_ref + 1: first window of each contig in lin
  uint64_t* lin;            // lin_off[n_ref] entries, ~0 = untouched
  uint64_t* unm;            // per contig: indexed records with flag 0x4 (nullptr: not counted)
  int32_t n_ref;
};

struct BaiWindow {  // per-record scratch of one window (n entries; bflag, slot: n + 1)
  uint64_t *key, *sk, *skmax;
  uint2* wspan;  // first and last window touched (first > last: none)
  uint32_t *bflag, *slot;
};

// temp bytes of the per-window scans over n records
hipError_t bai_scan_bytes(uint64_t n, size_t* bytes);
// key, sort key (0 for an unindexed record) and window span of records [0, n);
// state[kBaiErr] (= ~0 before) takes the failing records
hipError_t launch_bai_classify(const uint8_t* u, const Columns& col, uint64_t n, const BaiTables& t,
                               const BaiWindow& w, uint64_t* state, hipStream_t s);
// skmax = inclusive max-scan of sk; then the order check, the boundary flags
// (n + 1 entries, the last 0), the linear entries, the 0x4 counts and
// state[kBaiLastKey], state[kBaiSkMax]; then slot = exclusive sum of the
// flags and state[kBaiHeads]
hipError_t launch_bai_link(void* tmp, size_t tmp_bytes, const Columns& col, uint64_t n, uint64_t carry_key,
                           uint64_t carry_sk, const BaiTables& t, const BaiWindow& w, uint64_t* state,
                           hipStream_t s);
// boundary i -> run base + slot[i] (key, start = voff, ordinal = ord0 + i) and
// the end of run base + slot[i] - 1
hipError_t launch_bai_emit(const uint64_t* voff, uint64_t n, const BaiWindow& w, uint64_t base, uint64_t ord0,
                           uint64_t* run_key, uint64_t* run_start, uint64_t* run_end, uint64_t* run_ord,
                           hipStream_t s);

// The stable sort of r runs by key (bits [0, end_bit)): perm = file-order
// index of the k-th run in index order.
hipError_t bai_sort_bytes(uint64_t r, size_t* bytes);
hipError_t launch_bai_sort(void* tmp, size_t tmp_bytes, const uint64_t* run_key, uint64_t* key_sorted,
                           uint32_t* iota, uint32_t* perm, uint64_t r, int end_bit, hipStream_t s);
// the runs in index order: start, end and records (to the next run's ordinal;
// the last run's to `records`)
hipError_t launch_bai_gather(const uint32_t* perm, const uint64_t* run_start, const uint64_t* run_end,
                             const uint64_t* run_ord, uint64_t r, uint64_t records, uint64_t* start, uint64_t* end,
                             uint64_t* count, hipStream_t s);
// Gap fill of the linear tables (total = lin_off[n_ref] windows): last[w] = 1 +
// the last touched window at or before w (0: none; a max-scan of window
// ordinals), filled[w] = that window's entry when it lies in w's contig, else 0
hipError_t bai_fill_bytes(uint64_t total, size_t* bytes);
hipError_t launch_bai_fill(void* tmp, size_t tmp_bytes, const BaiTables& t, uint64_t total, uint32_t* ord,
                           uint32_t* last, uint64_t* filled, hipStream_t s);

}  // namespace hbam
