// hbam_merge.hip -- gfx950 kernels that plan the merge of k sorted runs of
// SAMRecordWritable encodings (hbam_merge_*: the reduce side of the reference's
// sort job, Hadoop's merge of the sorted map outputs) and build each output
// part's source table.  The run bytes stay in host memory; only the sort word,
// the framing and the order of every record live in HBM.  A record's global
// index g is run-major: run r's record i has g = run_base[r] + i, so the
// stable radix sort of (word, g) gives Hadoop's tie rule -- the earlier run,
// then the earlier record -- with no comparison code.
//
//   k_merge_check   per run: the framing (increasing offsets, records of >= 36
//        bytes inside len) and the words (non-decreasing); the first bad index
//        of either kind by atomicMin, the records' lengths as a by-product
//   k_merge_iota    idx[g] = g
//   (hipcub)        stable radix sort of (word, g): perm[j] = the global index
//        of the j-th output record
//   (launch_sort_offsets of hbam_sort.hip)  doff = the output starts
//   k_merge_heads   flag[j] = record j starts in another part than record j - 1
//        (part = doff / part_bytes: parts without a record start do not exist)
//   (hipcub)        exclusive sum of the flags: the kept parts' numbers
//   k_merge_parts   part_first[p] / part_start[p] = the first record / byte of part p
//   k_merge_rank    rank[perm[j]] = j, the inverse order
//   k_merge_cuts    cut[p][r] = the records of run r that precede part p: the
//        rank of a sorted run's records increases, one binary search per pair
//   k_merge_src     per part: record j's position in the staged slices, its
//        (run, record) name and its output start relative to the part
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_launch.h"

namespace hbam {

namespace {

constexpr uint32_t kMergeThreads = 256;

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kMergeThreads - 1) / kMergeThreads); }

// offs: the run's n + 1 offsets; bad[0] / bad[1] = the first record with bad
// framing / the first record whose word is below its predecessor's (preset ~0)
__global__ __launch_bounds__(kMergeThreads) void k_merge_check(const uint64_t* __restrict__ offs, uint64_t n,
                                                               uint64_t len, const uint64_t* __restrict__ word,
                                                               uint32_t* __restrict__ rlen,
                                                               unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t o0 = offs[i], o1 = offs[i + 1];
  const bool ok = o1 > o0 && o1 - o0 >= kMergeMinRecord && o1 - o0 <= 0xffffffffull && o1 <= len;
  rlen[i] = ok ? (uint32_t)(o1 - o0) : 0;
  if (!ok) atomicMin(&bad[0], (unsigned long long)i);
  if (word && i > 0 && word[i] < word[i - 1]) atomicMin(&bad[1], (unsigned long long)i);
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_iota(uint32_t* __restrict__ idx, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (i < n) idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_heads(const uint64_t* __restrict__ doff, uint64_t n,
                                                               uint64_t part_bytes, uint32_t* __restrict__ flag) {
  const uint64_t j = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j < n) flag[j] = (j == 0 || doff[j] / part_bytes != doff[j - 1] / part_bytes) ? 1u : 0u;
  else if (j == n) flag[j] = 0;
}

// num[j] = the exclusive sum of flag (num[n] = the parts); entry num[n] of both tables closes the last part
__global__ __launch_bounds__(kMergeThreads) void k_merge_parts(const uint32_t* __restrict__ flag,
                                                               const uint32_t* __restrict__ num,
                                                               const uint64_t* __restrict__ doff, uint64_t n,
                                                               uint32_t* __restrict__ part_first,
                                                               uint64_t* __restrict__ part_start) {
  const uint64_t j = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j > n || (j < n && !flag[j])) return;
  part_first[num[j]] = (uint32_t)j;
  part_start[num[j]] = doff[j];
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_rank(const uint32_t* __restrict__ perm, uint64_t n,
                                                              uint32_t* __restrict__ rank) {
  const uint64_t j = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j < n) rank[perm[j]] = (uint32_t)j;
}

// cut[p * k + r] for p in [0, parts], r in [0, k): the first record of run r
// whose output index is >= part_first[p] (row `parts`: the run's records), and
// cut_off = that record's offset in its run (the run's length past its last)
__global__ __launch_bounds__(kMergeThreads) void k_merge_cuts(const uint32_t* __restrict__ rank,
                                                              const uint64_t* __restrict__ run_base, uint32_t k,
                                                              const uint32_t* __restrict__ part_first,
                                                              const uint64_t* __restrict__ off, uint64_t pairs,
                                                              uint32_t* __restrict__ cut,
                                                              uint64_t* __restrict__ cut_off) {
  const uint64_t t = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (t >= pairs) return;
  const uint32_t r = (uint32_t)(t % k);
  const uint32_t target = part_first[t / k];
  const uint64_t b = run_base[r];
  uint64_t lo = 0, hi = run_base[r + 1] - b;  // the first i in [0, hi] with rank[b + i] >= target
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (rank[b + mid] < target) lo = mid + 1; else hi = mid;
  }
  cut[t] = (uint32_t)lo;
  cut_off[t] = off[b + r + lo];  // (the run's n + 1 checked offsets: the host stages slices by these)
}

// perm, doff: the part's first entries (perm + j0, doff + j0); off: every
// run's n + 1 offsets back to back (run r's at run_base[r] + r); slice_base[r]
// = where offset 0 of run r would lie in the staging buffer (modulo 2^64)
__global__ __launch_bounds__(kMergeThreads) void k_merge_src(const uint32_t* __restrict__ perm,
                                                             const uint64_t* __restrict__ doff, uint32_t n,
                                                             uint64_t dbase, const uint64_t* __restrict__ run_base,
                                                             uint32_t k, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ slice_base,
                                                             uint64_t* __restrict__ src_pos,
                                                             uint64_t* __restrict__ src_id,
                                                             uint64_t* __restrict__ part_offs) {
  const uint32_t j = blockIdx.x * kMergeThreads + threadIdx.x;
  if (j > n) return;
  part_offs[j] = doff[j] - dbase;
  if (j == n) return;
  const uint64_t g = perm[j];
  uint32_t lo = 0, hi = k;  // the last run with run_base <= g (an empty run shares its base with the next one)
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (run_base[mid] <= g) lo = mid; else hi = mid;
  }
  src_pos[j] = slice_base[lo] + off[g + lo];
  src_id[j] = ((uint64_t)lo << 32) | (g - run_base[lo]);
}

}  // namespace

hipError_t merge_tmp_bytes(uint64_t n, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = sort_tmp_bytes(n, &a);
  if (e != hipSuccess) return e;
  const uint32_t* f = nullptr;
  uint32_t* fo = nullptr;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, b, f, fo, (int)(n + 1), (hipStream_t)0)) != hipSuccess) return e;
  *bytes = a > b ? a : b;
  return hipSuccess;
}

hipError_t launch_merge_check(const uint64_t* offs, uint64_t n, uint64_t len, const uint64_t* word, uint32_t* rlen,
                              unsigned long long* bad, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_check, dim3(blocks_for(n)), dim3(kMergeThreads), 0, s, offs, n, len, word, rlen, bad);
  return hipGetLastError();
}

hipError_t launch_merge_perm(void* tmp, size_t tmp_bytes, const uint64_t* word, uint64_t* word_sorted, uint32_t* idx,
                             uint32_t* perm, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_iota, dim3(blocks_for(n)), dim3(kMergeThreads), 0, s, idx, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, word, word_sorted, idx, perm, (int)n, 0, 64, s);
}

hipError_t launch_merge_heads(void* tmp, size_t tmp_bytes, const uint64_t* doff, uint64_t n, uint64_t part_bytes,
                              uint32_t* flag, uint32_t* num, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_heads, dim3(blocks_for(n + 1)), dim3(kMergeThreads), 0, s, doff, n, part_bytes, flag);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flag, num, (int)(n + 1), s);
}

hipError_t launch_merge_cuts(const uint32_t* flag, const uint32_t* num, const uint64_t* doff, const uint32_t* perm,
                             uint64_t n, const uint64_t* run_base, uint32_t k, uint64_t parts, uint32_t* part_first,
                             uint64_t* part_start, uint32_t* rank, const uint64_t* off, uint32_t* cut,
                             uint64_t* cut_off, hipStream_t s) {
  if (n == 0 || k == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_parts, dim3(blocks_for(n + 1)), dim3(kMergeThreads), 0, s, flag, num, doff, n, part_first,
                     part_start);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_merge_rank, dim3(blocks_for(n)), dim3(kMergeThreads), 0, s, perm, n, rank);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint64_t pairs = (parts + 1) * k;
  hipLaunchKernelGGL(k_merge_cuts, dim3(blocks_for(pairs)), dim3(kMergeThreads), 0, s, rank, run_base, k, part_first,
                     off, pairs, cut, cut_off);
  return hipGetLastError();
}

hipError_t launch_merge_src(const uint32_t* perm, const uint64_t* doff, uint64_t n, uint64_t dbase,
                            const uint64_t* run_base, uint32_t k, const uint64_t* off, const uint64_t* slice_base,
                            uint64_t* src_pos, uint64_t* src_id, uint64_t* part_offs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merge_src, dim3(blocks_for(n + 1)), dim3(kMergeThreads), 0, s, perm, doff, (uint32_t)n, dbase,
                     run_base, k, off, slice_base, src_pos, src_id, part_offs);
  return hipGetLastError();
}

}  // namespace hbam
