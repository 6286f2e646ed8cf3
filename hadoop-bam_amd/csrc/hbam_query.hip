// hbam_query.hip -- gfx950 kernels of bounded traversal: the record filter of
// BAMRecordReader.initialize's interval and unmapped-only branches
// (BAMRecordReader.java:170-178; [htsjdk] BAMFileReader.BAMFileIndexIterator,
// BAMQueryFilteringIterator, BAMQueryMultipleIntervalsIteratorFilter,
// BAMFileIndexUnmappedIterator) over the records of one decoded window.
//
//   query_classify   per record: alignment end from the CIGAR (a lane for
//        cigars of <= kWaveCigarOps operators, the whole wave for a longer
//        one) and p = the intervals BEFORE the record (binary search, the
//        intervals in LDS when they fit)
//   (hipcub)         idx = inclusive max-scan of p, carry-in folded into p[0]
//   query_select     keep flags, kept rest lengths, the stop record (one
//        atomic per wave), the carry-out
//   query_unmapped   the unmapped-only predicate instead of the three above
//   (hipcub)         exclusive sums of the flags (slots) and of the kept rest
//        lengths (rest offsets, 64-bit)
//   query_gather / query_pack   the kept records' columns and rest bytes into
//        a compact buffer (ColLayout + rests back to back)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_align_end.h"
#include "hbam_device.h"
#include "hbam_query.h"

namespace hbam {

namespace {

constexpr uint32_t kLdsIntervals = 1024;      // intervals held in LDS (8 KiB: ref + end)
constexpr uint32_t kQueryThreads = 256;

// One lane per record (the cigar walk: cigar_ref_len, hbam_align_end.h).
template <bool kLds>
__global__ __launch_bounds__(kQueryThreads) void k_query_classify(const uint8_t* __restrict__ u, Columns c,
                                                                  uint64_t n, QueryIntervals iv, uint32_t carry,
                                                                  int32_t* __restrict__ aend,
                                                                  uint32_t* __restrict__ p) {
  __shared__ int32_t s_ref[kLds ? kLdsIntervals : 1], s_end[kLds ? kLdsIntervals : 1];
  if (kLds) {
    for (uint32_t t = threadIdx.x; t < iv.n; t += kQueryThreads) {
      s_ref[t] = iv.ref[t];
      s_end[t] = iv.end[t];
    }
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  const bool in = i < n;
  int32_t ref = -1, start = 0;
  bool mapped = false;
  if (in) {
    ref = c.ref_id[i];
    start = (int32_t)((uint32_t)c.pos[i] + 1u);
    mapped = !(c.flag[i] & 4u);
  }
  const uint32_t rl = cigar_ref_len(u, c, i, mapped);  // reference length, wrapping like a Java int
  if (!in) return;
  // [htsjdk] getAlignmentEnd: an unmapped record ends where it starts
  aend[i] = mapped ? (int32_t)((uint32_t)start + rl - 1u) : start;
  // BEFORE: the interval's contig precedes the record's, or it ends before
  // the record starts; true for a prefix of the sorted, disjoint intervals
  const int32_t* ivr = kLds ? s_ref : iv.ref;
  const int32_t* ive = kLds ? s_end : iv.end;
  uint32_t lo = 0, hi = iv.n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const int32_t r = ivr[mid];
    if (r < ref || (r == ref && ive[mid] < start)) lo = mid + 1; else hi = mid;
  }
  p[i] = i == 0 ? max(lo, carry) : lo;
}

__global__ __launch_bounds__(kQueryThreads) void k_query_select(const int32_t* __restrict__ ref_id,
                                                                const uint32_t* __restrict__ rest_len,
                                                                const int32_t* __restrict__ aend,
                                                                const uint32_t* __restrict__ idx, uint64_t n,
                                                                QueryIntervals iv, uint32_t* __restrict__ flag,
                                                                uint64_t* __restrict__ klen,
                                                                unsigned long long* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  bool stopped = false;
  if (i < n) {
    const uint32_t id = idx[i];
    bool keep = false;
    if (id >= iv.n) {
      stopped = true;
    } else {
      // AFTER: the interval's contig follows the record's, or it starts past the record's end
      keep = !(iv.ref[id] > ref_id[i] || aend[i] < iv.start[id]);
    }
    flag[i] = keep;
    klen[i] = keep ? rest_len[i] : 0;
    if (i == n - 1) state[kQueryCarry] = id;
  }
  if (i == 0) {
    flag[n] = 0;
    klen[n] = 0;
  }
  // the stop record: the lowest stopped lane of the wave holds the wave's
  // minimum (lanes are consecutive records), one atomic per wave
  const unsigned long long b = __ballot(stopped);
  if (b && (int)(threadIdx.x & 63u) == __ffsll((long long)b) - 1) atomicMin(&state[kQueryStop], (unsigned long long)i);
}

// unmapped-only: the first record with refID == -1 of the window ...
__global__ __launch_bounds__(kQueryThreads) void k_query_first_unplaced(const int32_t* __restrict__ ref_id,
                                                                        uint64_t n,
                                                                        unsigned long long* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  const unsigned long long b = __ballot(i < n && ref_id[i] == -1);
  if (b && (int)(threadIdx.x & 63u) == __ffsll((long long)b) - 1) atomicMin(&state[kQueryStop], (unsigned long long)i);
}
// ... and every record from it on (from record 0 when an earlier window held it)
__global__ __launch_bounds__(kQueryThreads) void k_query_unmapped_flags(const uint32_t* __restrict__ rest_len,
                                                                        uint64_t n, uint32_t found_before,
                                                                        uint32_t* __restrict__ flag,
                                                                        uint64_t* __restrict__ klen,
                                                                        const unsigned long long* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  const unsigned long long first = found_before ? 0ull : state[kQueryStop];
  if (i < n) {
    const bool keep = i >= first;
    flag[i] = keep;
    klen[i] = keep ? rest_len[i] : 0;
  }
  if (i == 0) {
    flag[n] = 0;
    klen[n] = 0;
  }
}

__global__ void k_query_totals(const uint32_t* __restrict__ slot, const uint64_t* __restrict__ roff, uint64_t n,
                               unsigned long long* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  state[kQueryKept] = slot[n];
  state[kQueryBytes] = roff[n];
}

// kept record i -> slot[i] of the compact columns; key and voff carried over
__global__ __launch_bounds__(kQueryThreads) void k_query_gather(Columns s, uint64_t n,
                                                                const uint32_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ slot,
                                                                const uint64_t* __restrict__ roff, Columns d,
                                                                uint64_t* __restrict__ src_off) {
  const uint64_t i = (uint64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint32_t j = slot[i];
  d.ref_id[j] = s.ref_id[i];
  d.pos[j] = s.pos[i];
  d.l_seq[j] = s.l_seq[i];
  d.next_ref_id[j] = s.next_ref_id[i];
  d.next_pos[j] = s.next_pos[i];
  d.tlen[j] = s.tlen[i];
  d.l_read_name[j] = s.l_read_name[i];
  d.mapq[j] = s.mapq[i];
  d.bin[j] = s.bin[i];
  d.n_cigar[j] = s.n_cigar[i];
  d.flag[j] = s.flag[i];
  d.key[j] = s.key[i];
  d.voff[j] = s.voff[i];
  d.rest_off[j] = roff[i];
  d.rest_len[j] = s.rest_len[i];
  src_off[j] = s.rest_off[i];
}

// The kept records' rests back to back.  k_pack_rests (hbam_records.hip) computes a record's
// source from its slot (contiguous records); kept records are scattered, so
// here a workgroup takes 256 kept records with their destination (cp) and
// source (sp) offsets in LDS and writes 16-byte output chunks: a shifted 16 B
// load when the chunk lies in one rest (most of them), bytes otherwise.
constexpr uint32_t kQPackRecs = 256;
__global__ __launch_bounds__(256) void k_query_pack(const uint8_t* __restrict__ u,
                                                    const uint64_t* __restrict__ rest_off,
                                                    const uint32_t* __restrict__ rest_len,
                                                    const uint64_t* __restrict__ src_off, uint64_t m,
                                                    uint8_t* __restrict__ dst) {
  __shared__ uint64_t cp[kQPackRecs + 1], sp[kQPackRecs];
  const uint64_t r0 = (uint64_t)blockIdx.x * kQPackRecs;
  if (r0 >= m) return;
  const uint32_t cnt = (uint32_t)min<uint64_t>(kQPackRecs, m - r0), t = threadIdx.x;
  if (t < cnt) {
    const uint64_t c = rest_off[r0 + t];
    cp[t] = c;
    sp[t] = src_off[r0 + t];
    if (t == cnt - 1) cp[cnt] = c + rest_len[r0 + t];
  }
  __syncthreads();
  const uint64_t lo = cp[0], hi = cp[cnt];
  for (uint64_t c = (lo & ~15ull) + 16ull * t; c < hi; c += 16ull * blockDim.x) {
    const uint64_t o0 = max(c, lo), o1 = min(c + 16, hi);
    uint32_t a = 0, b = cnt - 1;  // the last record with cp <= o0
    while (a < b) {
      const uint32_t mid = (a + b + 1) >> 1;
      if (cp[mid] <= o0) a = mid; else b = mid - 1;
    }
    if (o0 == c && o1 == c + 16 && cp[a + 1] >= c + 16) {
      const uint64_t src = sp[a] + (c - cp[a]);
      const uint4* q = reinterpret_cast<const uint4*>(u + (src & ~15ull));
      *reinterpret_cast<uint4*>(dst + c) = shift16(q[0], q[1], (uint32_t)(src & 15));
    } else {
      for (uint64_t o = o0; o < o1; ++o) {
        while (cp[a + 1] <= o) ++a;
        dst[o] = u[sp[a] + (o - cp[a])];
      }
    }
  }
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kQueryThreads - 1) / kQueryThreads); }

}  // namespace

hipError_t launch_query_classify(const uint8_t* u, const Columns& col, uint64_t n, const QueryIntervals& iv,
                                 uint32_t carry, int32_t* aend, uint32_t* p, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (iv.n <= kLdsIntervals)
    hipLaunchKernelGGL(k_query_classify<true>, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, u, col, n, iv, carry,
                       aend, p);
  else
    hipLaunchKernelGGL(k_query_classify<false>, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, u, col, n, iv, carry,
                       aend, p);
  return hipGetLastError();
}

hipError_t query_scan_bytes(uint64_t n, size_t* bytes) {
  size_t a = 0, b = 0, c = 0;
  const uint32_t* p32 = nullptr;
  uint32_t* o32 = nullptr;
  const uint64_t* p64 = nullptr;
  uint64_t* o64 = nullptr;
  hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, a, p32, o32, hipcub::Max(), (int)n, (hipStream_t)0);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, b, p32, o32, (int)n, (hipStream_t)0)) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, c, p64, o64, (int)n, (hipStream_t)0)) != hipSuccess) return e;
  *bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return hipSuccess;
}

hipError_t launch_query_scan(void* tmp, size_t tmp_bytes, const uint32_t* p, uint32_t* idx, uint64_t n,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  return hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, p, idx, hipcub::Max(), (int)n, s);
}

hipError_t launch_query_select(const Columns& col, const int32_t* aend, const uint32_t* idx, uint64_t n,
                               const QueryIntervals& iv, uint32_t* flag, uint64_t* klen, uint64_t* state,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_query_select, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, col.ref_id, col.rest_len, aend,
                     idx, n, iv, flag, klen, reinterpret_cast<unsigned long long*>(state));
  return hipGetLastError();
}

hipError_t launch_query_unmapped(const Columns& col, uint64_t n, bool found_before, uint32_t* flag, uint64_t* klen,
                                 uint64_t* state, hipStream_t s) {
  if (n == 0) return hipSuccess;
  unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
  hipLaunchKernelGGL(k_query_first_unplaced, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, col.ref_id, n, st);
  hipLaunchKernelGGL(k_query_unmapped_flags, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, col.rest_len, n,
                     found_before ? 1u : 0u, flag, klen, st);
  return hipGetLastError();
}

hipError_t launch_query_offsets(void* tmp, size_t tmp_bytes, const uint32_t* flag, uint32_t* slot,
                                const uint64_t* klen, uint64_t* roff, uint64_t n, uint64_t* state, hipStream_t s) {
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flag, slot, (int)(n + 1), s);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, klen, roff, (int)(n + 1), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_query_totals, dim3(1), dim3(64), 0, s, slot, roff, n,
                     reinterpret_cast<unsigned long long*>(state));
  return hipGetLastError();
}

hipError_t launch_query_compact(const uint8_t* u, const Columns& src, uint64_t n, const uint32_t* flag,
                                const uint32_t* slot, const uint64_t* roff, const Columns& dst, uint64_t kept,
                                uint64_t* src_off, uint8_t* rests, hipStream_t s) {
  if (n == 0 || kept == 0) return hipSuccess;
  hipLaunchKernelGGL(k_query_gather, dim3(blocks_for(n)), dim3(kQueryThreads), 0, s, src, n, flag, slot, roff, dst,
                     src_off);
  hipLaunchKernelGGL(k_query_pack, dim3((unsigned)((kept + kQPackRecs - 1) / kQPackRecs)), dim3(256), 0, s, u,
                     dst.rest_off, dst.rest_len, src_off, kept, rests);
  return hipGetLastError();
}

}  // namespace hbam
