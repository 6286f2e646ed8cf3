// hbam_query.h -- launch wrappers of the bounded-traversal kernels (hbam_query.hip):
// the record filter of BAMRecordReader.initialize's interval and unmapped
// branches (BAMRecordReader.java:170-178) over one decoded window.
//
// htsjdk's filter ([htsjdk] BAMQueryMultipleIntervalsIteratorFilter.
// compareIntervalToRecord) keeps one interval index for the whole query and,
// per record, skips the intervals that lie BEFORE it.  The intervals are
// sorted and disjoint, so BEFORE holds for a prefix of them and the loop is
//   p_i   = intervals BEFORE record i          (binary search, k_query_classify)
//   idx_i = max(idx_{i-1}, p_i)                (inclusive max-scan, carry across windows)
//   keep  = idx_i < L and intervals[idx_i] is not AFTER record i   (k_query_select)
// with the iteration ending at the first record whose idx_i == L.  The kept
// records' columns and rests are then gathered into a compact buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbam_device.h"

namespace hbam {

// L optimized intervals on the device (SoA): end = the effective end
// (INT32_MAX for "to the end of the reference").
struct QueryIntervals {
  const int32_t *ref, *start, *end;
  uint32_t n;
};

// Per-window results the host reads back (u64 each).
enum : int {
  kQueryStop = 0,   // min record index with idx == L (unmapped mode: first refID == -1); ~0 = none
  kQueryCarry = 1,  // idx of the last record: the next window's carry-in
  kQueryKept = 2,   // records kept
  kQueryBytes = 3,  // their rest bytes
  kQueryStateWords = 4,
};

// alignment end + p of records [0, n) of a decoded window (u = the stream
// col.rest_off indexes); record 0's p takes the carry-in
hipError_t launch_query_classify(const uint8_t* u, const Columns& col, uint64_t n, const QueryIntervals& iv,
                                 uint32_t carry, int32_t* aend, uint32_t* p, hipStream_t s);
// temp bytes of the scans over n items
hipError_t query_scan_bytes(uint64_t n, size_t* bytes);
// idx = inclusive max-scan of p
hipError_t launch_query_scan(void* tmp, size_t tmp_bytes, const uint32_t* p, uint32_t* idx, uint64_t n,
                             hipStream_t s);
// keep flags + kept rest lengths (n + 1 entries each, the last 0);
// state[kQueryStop] (= ~0 before) and state[kQueryCarry]
hipError_t launch_query_select(const Columns& col, const int32_t* aend, const uint32_t* idx, uint64_t n,
                               const QueryIntervals& iv, uint32_t* flag, uint64_t* klen, uint64_t* state,
                               hipStream_t s);
// unmapped-only: keep = i >= the first record with refID == -1 (found_before:
// an earlier window held it); state[kQueryStop] (= ~0 before) = that index
hipError_t launch_query_unmapped(const Columns& col, uint64_t n, bool found_before, uint32_t* flag, uint64_t* klen,
                                 uint64_t* state, hipStream_t s);
// slot / roff = exclusive sums of flag / klen over n + 1 entries;
// state[kQueryKept], state[kQueryBytes]
hipError_t launch_query_offsets(void* tmp, size_t tmp_bytes, const uint32_t* flag, uint32_t* slot,
                                const uint64_t* klen, uint64_t* roff, uint64_t n, uint64_t* state, hipStream_t s);
// the kept records' columns -> dst at their slots (rest_off = roff: into
// `rests`), then their rest bytes back to back into rests (16 B-aligned, room
// for the kept bytes + 16; u readable 32 bytes past the last rest);
// src_off: scratch, one entry per kept record
hipError_t launch_query_compact(const uint8_t* u, const Columns& src, uint64_t n, const uint32_t* flag,
                                const uint32_t* slot, const uint64_t* roff, const Columns& dst, uint64_t kept,
                                uint64_t* src_off, uint8_t* rests, hipStream_t s);

}  // namespace hbam
