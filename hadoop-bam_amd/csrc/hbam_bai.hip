// hbam_bai.hip -- gfx950 kernels of the BAM indexer (.bai, SAM spec 5.2) over
// the records of one decoded window, and the passes that finish the index.
//
//   bai_classify  per record: the end from the CIGAR (cigar_ref_len, shared
//        with the bounded-traversal filter), the bin (reg2bin, computed), the
//        16 kbp windows touched, the key refID << 16 | bin and the sort key
//        (refID, pos); end > 2^29, a window beyond the contig's table and a
//        refID beyond the header are reported
//   (hipcub)      skmax = inclusive max-scan of the sort keys
//   bai_link      the order check against skmax, the boundary flags (key
//        differs from the predecessor's; the last key of the window before is
//        carried in), the linear entries (64-bit min, only for windows the
//        predecessor does not touch), the per-contig 0x4 counts (one atomic
//        per wave and contig)
//   (hipcub)      slot = exclusive sum of the boundary flags
//   bai_emit      the boundaries into the run list; each also ends the run
//        before it (possibly a run of an earlier window)
//   at the end    (hipcub) stable radix sort of the runs by key, bai_gather of
//        their starts, ends and record counts; bai_lin_ord + (hipcub) max-scan
//        + bai_lin_fill for the untouched linear windows
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_align_end.h"
#include "hbam_bai.h"
#include "hbam_device.h"

namespace hbam {

namespace {

constexpr uint32_t kBaiThreads = 256;

// SAM spec 5.3 reg2bin over the 0-based half-open [beg, end)
__device__ __forceinline__ uint32_t reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return ((1u << 15) - 1) / 7 + (beg >> 14);
  if (beg >> 17 == end >> 17) return ((1u << 12) - 1) / 7 + (beg >> 17);
  if (beg >> 20 == end >> 20) return ((1u << 9) - 1) / 7 + (beg >> 20);
  if (beg >> 23 == end >> 23) return ((1u << 6) - 1) / 7 + (beg >> 23);
  if (beg >> 26 == end >> 26) return ((1u << 3) - 1) / 7 + (beg >> 26);
  return 0;
}

__device__ __forceinline__ void report(unsigned long long* state, uint64_t i, int code) {
  atomicMin(&state[kBaiErr], (unsigned long long)((i << 2) | (uint64_t)code));
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_classify(const uint8_t* __restrict__ u, Columns c, uint64_t n,
                                                              BaiTables t, BaiWindow w,
                                                              unsigned long long* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  const bool in = i < n;
  int32_t ref = -1, pos = -1;
  bool unm = false;
  if (in) {
    ref = c.ref_id[i];
    pos = c.pos[i];
    unm = (c.flag[i] & 4u) != 0;
  }
  bool indexed = in && ref >= 0 && pos >= 0;
  if (indexed && ref >= t.n_ref) {
    report(state, i, kBaiErrRef);
    indexed = false;
  }
  const uint32_t rl = cigar_ref_len(u, c, i, indexed && !unm);  // (every lane: the long cigars take the wave)
  if (!in) return;
  uint64_t key = (uint64_t)(uint32_t)t.n_ref << 16, sk = 0;
  uint2 ws = make_uint2(1u, 0u);
  if (indexed) {
    int64_t end;
    uint32_t w0, w1;
    if (unm) {  // a placed unmapped read: one position, the window of the base before it
      end = (int64_t)pos + 1;
      w0 = w1 = (uint32_t)max(pos - 1, 0) >> kBaiLinShift;
    } else {
      end = (int64_t)pos + max((int32_t)rl, 1);
      w0 = (uint32_t)pos >> kBaiLinShift;
      w1 = (uint32_t)((end - 1) >> kBaiLinShift);  // (end <= 2^32: fits; checked next)
    }
    if (end > kBaiMaxEnd) {
      report(state, i, kBaiErrEnd);
    } else if (w1 >= t.lin_off[ref + 1] - t.lin_off[ref]) {
      report(state, i, kBaiErrWindow);
    } else {
      key = ((uint64_t)(uint32_t)ref << 16) | reg2bin((uint32_t)pos, (uint32_t)end);
      sk = (((uint64_t)(uint32_t)ref << 32) | (uint32_t)pos) + 1;
      ws = make_uint2(w0, w1);
    }
  }
  w.key[i] = key;
  w.sk[i] = sk;
  w.wspan[i] = ws;
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_link(const uint64_t* __restrict__ voff,
                                                          const uint16_t* __restrict__ flag, uint64_t n,
                                                          uint64_t carry_key, uint64_t carry_sk, BaiTables t,
                                                          BaiWindow w, unsigned long long* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t none = (uint64_t)(uint32_t)t.n_ref << 16;
  bool count = false;  // an indexed record with flag 0x4
  uint32_t ref = 0;
  if (i < n) {
    const uint64_t key = w.key[i], pk = i ? w.key[i - 1] : carry_key;
    w.bflag[i] = key != pk;
    if (key != none) {
      ref = (uint32_t)(key >> 16);
      const uint64_t before = i ? max(w.skmax[i - 1], carry_sk) : carry_sk;
      if (w.sk[i] < before) report(state, i, kBaiErrOrder);
      // the linear entries: a window the record before touches too has a smaller voff already
      const uint2 ws = w.wspan[i];
      uint32_t p0 = 1, p1 = 0;
      if (i && pk != none && (uint32_t)(pk >> 16) == ref) {
        const uint2 pw = w.wspan[i - 1];
        p0 = pw.x;
        p1 = pw.y;
      }
      unsigned long long* lin = reinterpret_cast<unsigned long long*>(t.lin) + t.lin_off[ref];
      const unsigned long long v = voff[i];
      for (uint32_t k = ws.x; k <= ws.y; ++k) {
        if (k >= p0 && k <= p1) {
          k = p1;
          continue;
        }
        atomicMin(&lin[k], v);
      }
      count = t.unm && (flag[i] & 4u);
    }
    if (i == n - 1) {
      state[kBaiLastKey] = key;
      state[kBaiSkMax] = max(w.skmax[i], carry_sk);
    }
  }
  if (i == 0) w.bflag[n] = 0;
  // the 0x4 counts: the lanes of one contig add once (uniform loop over the wave's contigs)
  for (unsigned long long m = __ballot(count); m;) {
    const int src = __ffsll((long long)m) - 1;
    const uint32_t r = (uint32_t)__shfl((int)ref, src, 64);
    const unsigned long long same = __ballot(count && ref == r);
    if ((int)lane == src) atomicAdd(reinterpret_cast<unsigned long long*>(&t.unm[r]), (unsigned long long)__popcll(same));
    m &= ~same;
  }
}

__global__ void k_bai_heads(const uint32_t* __restrict__ slot, uint64_t n, unsigned long long* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[kBaiHeads] = slot[n];
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_emit(const uint64_t* __restrict__ voff, uint64_t n, BaiWindow w,
                                                          uint64_t base, uint64_t ord0,
                                                          uint64_t* __restrict__ run_key,
                                                          uint64_t* __restrict__ run_start,
                                                          uint64_t* __restrict__ run_end,
                                                          uint64_t* __restrict__ run_ord) {
  const uint64_t i = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  if (i >= n || !w.bflag[i]) return;
  const uint64_t j = base + w.slot[i], v = voff[i];
  run_key[j] = w.key[i];
  run_start[j] = v;
  run_ord[j] = ord0 + i;
  if (j) run_end[j - 1] = v;
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_iota(uint32_t* __restrict__ a, uint64_t r) {
  const uint64_t i = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  if (i < r) a[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_gather(const uint32_t* __restrict__ perm,
                                                            const uint64_t* __restrict__ run_start,
                                                            const uint64_t* __restrict__ run_end,
                                                            const uint64_t* __restrict__ run_ord, uint64_t r,
                                                            uint64_t records, uint64_t* __restrict__ start,
                                                            uint64_t* __restrict__ end,
                                                            uint64_t* __restrict__ count) {
  const uint64_t k = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  if (k >= r) return;
  const uint64_t j = perm[k];
  start[k] = run_start[j];
  end[k] = run_end[j];
  count[k] = (j + 1 < r ? run_ord[j + 1] : records) - run_ord[j];
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_lin_ord(const uint64_t* __restrict__ lin, uint64_t total,
                                                             uint32_t* __restrict__ ord) {
  const uint64_t k = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  if (k < total) ord[k] = lin[k] != ~0ull ? (uint32_t)k + 1u : 0u;
}

__global__ __launch_bounds__(kBaiThreads) void k_bai_lin_fill(BaiTables t, uint64_t total,
                                                              const uint32_t* __restrict__ last,
                                                              uint64_t* __restrict__ filled) {
  const uint64_t k = (uint64_t)blockIdx.x * kBaiThreads + threadIdx.x;
  if (k >= total) return;
  uint32_t lo = 0, hi = (uint32_t)t.n_ref;  // the contig of window k: the last with lin_off <= k
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (t.lin_off[mid] <= k) lo = mid; else hi = mid;
  }
  const uint32_t m = last[k];
  filled[k] = m > t.lin_off[lo] ? t.lin[m - 1] : 0;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kBaiThreads - 1) / kBaiThreads); }

}  // namespace

hipError_t bai_scan_bytes(uint64_t n, size_t* bytes) {
  size_t a = 0, b = 0;
  const uint64_t* p64 = nullptr;
  uint64_t* o64 = nullptr;
  const uint32_t* p32 = nullptr;
  uint32_t* o32 = nullptr;
  hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, a, p64, o64, hipcub::Max(), (int)n, (hipStream_t)0);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, b, p32, o32, (int)(n + 1), (hipStream_t)0)) != hipSuccess)
    return e;
  *bytes = a > b ? a : b;
  return hipSuccess;
}

hipError_t launch_bai_classify(const uint8_t* u, const Columns& col, uint64_t n, const BaiTables& t,
                               const BaiWindow& w, uint64_t* state, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_classify, dim3(blocks_for(n)), dim3(kBaiThreads), 0, s, u, col, n, t, w,
                     reinterpret_cast<unsigned long long*>(state));
  return hipGetLastError();
}

hipError_t launch_bai_link(void* tmp, size_t tmp_bytes, const Columns& col, uint64_t n, uint64_t carry_key,
                           uint64_t carry_sk, const BaiTables& t, const BaiWindow& w, uint64_t* state,
                           hipStream_t s) {
  if (n == 0) return hipSuccess;
  unsigned long long* st = reinterpret_cast<unsigned long long*>(state);
  hipError_t e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, w.sk, w.skmax, hipcub::Max(), (int)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bai_link, dim3(blocks_for(n)), dim3(kBaiThreads), 0, s, col.voff, col.flag, n, carry_key,
                     carry_sk, t, w, st);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, w.bflag, w.slot, (int)(n + 1), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_bai_heads, dim3(1), dim3(64), 0, s, w.slot, n, st);
  return hipGetLastError();
}

hipError_t launch_bai_emit(const uint64_t* voff, uint64_t n, const BaiWindow& w, uint64_t base, uint64_t ord0,
                           uint64_t* run_key, uint64_t* run_start, uint64_t* run_end, uint64_t* run_ord,
                           hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_emit, dim3(blocks_for(n)), dim3(kBaiThreads), 0, s, voff, n, w, base, ord0, run_key,
                     run_start, run_end, run_ord);
  return hipGetLastError();
}

hipError_t bai_sort_bytes(uint64_t r, size_t* bytes) {
  const uint64_t* k = nullptr;
  uint64_t* ko = nullptr;
  const uint32_t* v = nullptr;
  uint32_t* vo = nullptr;
  return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, k, ko, v, vo, (int)r, 0, 64, (hipStream_t)0);
}

hipError_t launch_bai_sort(void* tmp, size_t tmp_bytes, const uint64_t* run_key, uint64_t* key_sorted,
                           uint32_t* iota, uint32_t* perm, uint64_t r, int end_bit, hipStream_t s) {
  if (r == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_iota, dim3(blocks_for(r)), dim3(kBaiThreads), 0, s, iota, r);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, run_key, key_sorted, iota, perm, (int)r, 0, end_bit, s);
}

hipError_t launch_bai_gather(const uint32_t* perm, const uint64_t* run_start, const uint64_t* run_end,
                             const uint64_t* run_ord, uint64_t r, uint64_t records, uint64_t* start, uint64_t* end,
                             uint64_t* count, hipStream_t s) {
  if (r == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_gather, dim3(blocks_for(r)), dim3(kBaiThreads), 0, s, perm, run_start, run_end, run_ord,
                     r, records, start, end, count);
  return hipGetLastError();
}

hipError_t bai_fill_bytes(uint64_t total, size_t* bytes) {
  const uint32_t* p = nullptr;
  uint32_t* o = nullptr;
  return hipcub::DeviceScan::InclusiveScan(nullptr, *bytes, p, o, hipcub::Max(), (int)total, (hipStream_t)0);
}

hipError_t launch_bai_fill(void* tmp, size_t tmp_bytes, const BaiTables& t, uint64_t total, uint32_t* ord,
                           uint32_t* last, uint64_t* filled, hipStream_t s) {
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bai_lin_ord, dim3(blocks_for(total)), dim3(kBaiThreads), 0, s, t.lin, total, ord);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::InclusiveScan(tmp, tmp_bytes, ord, last, hipcub::Max(), (int)total, s)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(k_bai_lin_fill, dim3(blocks_for(total)), dim3(kBaiThreads), 0, s, t, total, last, filled);
  return hipGetLastError();
}

}  // namespace hbam
