// hbam_sort.hip -- gfx950 kernels that put the records of one decoded span in
// sorted order (hbam_sort_writables: SAMRecordWritable.write of every record,
// ordered by the BAMRecordReader key or by coordinate).
//
//   k_sort_words  per record: the 64-bit sort word of the chosen order, the
//        record's encoded length (36 + rest_len) and a u32 iota
//   (hipcub)      stable radix sort of (word, iota): perm[j] = the batch index
//        of the j-th output record
//   k_sort_lens   slen[j] = len[perm[j]] (slen[n] = 0)
//   (hipcub)      doff = exclusive sum of slen over n + 1 entries: the output
//        starts, doff[n] = the output's bytes
//   k_sort_gather the record bytes, divided by output bytes: a workgroup owns
//        one 32 KiB output tile, whatever the records' lengths
//        (k_sort_gather<true>: the same gather for one part of a merge of
//        sorted runs, hbam_merge.hip, from a per-record source table)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_dev_util.h"  // shift16
#include "hbam_launch.h"

namespace hbam {

namespace {

constexpr uint32_t kSortThreads = 256;

__global__ __launch_bounds__(kSortThreads) void k_sort_words(const int64_t* __restrict__ key,
                                                             const int32_t* __restrict__ ref_id,
                                                             const int32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ rest_len, uint64_t n,
                                                             int order, uint64_t* __restrict__ word,
                                                             uint32_t* __restrict__ len, uint32_t* __restrict__ iota) {
  const uint64_t i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x;
  if (i >= n) return;
  uint64_t w;
  if (order == kSortKey)  // LongWritable.compareTo: signed; the sign bit flipped sorts the same unsigned
    w = (uint64_t)key[i] ^ (1ull << 63);
  else  // refID -1 last (0xffffffff), pos -1 first in its contig (0)
    w = ((uint64_t)(uint32_t)ref_id[i] << 32) | (uint32_t)(pos[i] + 1);
  word[i] = w;
  len[i] = 36u + rest_len[i];
  iota[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kSortThreads) void k_sort_lens(const uint32_t* __restrict__ len,
                                                            const uint32_t* __restrict__ perm, uint64_t n,
                                                            uint64_t* __restrict__ slen) {
  const uint64_t j = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x;
  if (j < n) slen[j] = len[perm[j]];
  else if (j == n) slen[j] = 0;
}

// dst[doff[j], doff[j + 1]) = the bytes of record perm[j] (u + rec_pos[perm[j]]),
// indexBin (bytes 14-15) written as 0 when its refID < 0.
//
// Workgroup b owns output bytes [b * kSortTile, (b + 1) * kSortTile).  The
// records that overlap the tile -- at most 911 + 1, a record has >= 36 bytes --
// go into an LDS table of kSortTable entries: the record's output start and its
// source position with the refID < 0 flag in bit 63.  Entries past the tile's
// last record hold ~0, so "the last entry with start <= o" is a fixed ten-step
// search.  Each lane then forms 16-byte output chunks: a chunk inside one
// record is two aligned 16 B loads shifted together (one when the source is
// aligned: the read then stays inside the record) and one coalesced 16 B
// store; a chunk that crosses a record boundary, or the output's last partial
// chunk, goes byte by byte.  The source is readable 16 bytes past its last
// record.
constexpr uint32_t kSortTile = 32768;
constexpr uint32_t kSortTable = 1024;
constexpr uint64_t kSortUnplaced = 1ull << 63;
static_assert(kSortTile / 36 + 2 < kSortTable, "every record of a tile and the next one's start fit the table");

// kMerge (one part of hbam_merge_next): rec_pos[j] is the j-th output record's
// own source position (k_merge_src's table: no perm), the encodings already
// carry indexBin = 0 (no ref_id, no patch), and doff holds the part's n + 1
// global output starts, dbase = the part's first: the tile is relative to it.
template <bool kMerge>
__global__ __launch_bounds__(kSortThreads) void k_sort_gather(const uint8_t* __restrict__ u,
                                                              const uint64_t* __restrict__ rec_pos,
                                                              const int32_t* __restrict__ ref_id,
                                                              const uint32_t* __restrict__ perm,
                                                              const uint64_t* __restrict__ doff, uint32_t n,
                                                              uint64_t total, uint8_t* __restrict__ dst,
                                                              uint64_t dbase) {
  __shared__ uint64_t t_off[kSortTable];
  __shared__ uint64_t t_src[kSortTable];
  const uint64_t t0 = (uint64_t)blockIdx.x * kSortTile;
  if (t0 >= total) return;
  const uint64_t t1 = min(t0 + kSortTile, total);
  // the tile's first record: the last j with doff[j] <= t0 (doff[0] = 0, doff[n] = total > t0)
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (doff[mid] - (kMerge ? dbase : 0) <= t0) lo = mid; else hi = mid;
  }
  const uint32_t j0 = lo;
  for (uint32_t k = threadIdx.x; k < kSortTable; k += kSortThreads) {
    const uint64_t j = (uint64_t)j0 + k;
    uint64_t o = ~0ull, s = 0;
    if (j <= n) {
      o = doff[j] - (kMerge ? dbase : 0);  // (a start at or past t1 ends the tile's last record; later ones are never searched for)
      if (j < n && o < t1) {
        if constexpr (kMerge) {
          s = rec_pos[j];
        } else {
          const uint32_t r = perm[j];
          s = rec_pos[r] | (ref_id[r] < 0 ? kSortUnplaced : 0);
        }
      }
    }
    t_off[k] = o;
    t_src[k] = s;
  }
  __syncthreads();
  for (uint64_t c = t0 + 16ull * threadIdx.x; c < t1; c += 16ull * kSortThreads) {
    uint32_t a = 0;  // the last entry with t_off <= c
#pragma unroll
    for (uint32_t step = kSortTable >> 1; step; step >>= 1)
      if (t_off[a + step] <= c) a += step;
    const uint64_t ro = t_off[a], rs = t_src[a];
    const uint64_t c1 = min(c + 16, t1);
    if (c1 == c + 16 && t_off[a + 1] >= c1) {
      const uint64_t src = (rs & ~kSortUnplaced) + (c - ro);
      const uint32_t sh = (uint32_t)(src & 15);
      const uint4* q = reinterpret_cast<const uint4*>(u + (src & ~15ull));
      uint4 v = q[0];
      // (sh differs from lane to lane here: shift16's four cases are selects, not a table)
      if (sh) v = shift16(v, q[1], sh);
      // indexBin = 0: record bytes 14-15, at chunk byte rel (-1: byte 15 alone is chunk byte 0)
      const int64_t rel = (int64_t)(ro + 14) - (int64_t)c;
      if ((rs & kSortUnplaced) && rel >= -1 && rel <= 15) {
        uint64_t mlo = 0, mhi = 0;
        if (rel < 0) {
          mlo = 0xffull;
        } else if (rel < 8) {
          mlo = 0xffffull << (8 * rel);
          if (rel == 7) mhi = 0xffull;
        } else {
          mhi = 0xffffull << (8 * (rel - 8));
        }
        v.x &= ~(uint32_t)mlo;
        v.y &= ~(uint32_t)(mlo >> 32);
        v.z &= ~(uint32_t)mhi;
        v.w &= ~(uint32_t)(mhi >> 32);
      }
      *reinterpret_cast<uint4*>(dst + c) = v;
    } else {
      for (uint64_t o = c; o < c1; ++o) {
        while (t_off[a + 1] <= o) ++a;
        const uint64_t s = t_src[a], at = o - t_off[a];
        uint8_t b = u[(s & ~kSortUnplaced) + at];
        if ((s & kSortUnplaced) && (at == 14 || at == 15)) b = 0;
        dst[o] = b;
      }
    }
  }
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kSortThreads - 1) / kSortThreads); }

}  // namespace

hipError_t sort_tmp_bytes(uint64_t n, size_t* bytes) {
  size_t a = 0, b = 0;
  const uint64_t* k = nullptr;
  uint64_t* ko = nullptr;
  const uint32_t* v = nullptr;
  uint32_t* vo = nullptr;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, ko, v, vo, (int)n, 0, 64, (hipStream_t)0);
  if (e != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, b, k, ko, (int)(n + 1), (hipStream_t)0)) != hipSuccess) return e;
  *bytes = a > b ? a : b;
  return hipSuccess;
}

hipError_t launch_sort_perm(void* tmp, size_t tmp_bytes, const Columns& col, uint64_t n, int order, uint64_t* word,
                            uint64_t* word_sorted, uint32_t* len, uint32_t* iota, uint32_t* perm, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sort_words, dim3(blocks_for(n)), dim3(kSortThreads), 0, s, col.key, col.ref_id, col.pos,
                     col.rest_len, n, order, word, len, iota);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, word, word_sorted, iota, perm, (int)n, 0, 64, s);
}

hipError_t launch_sort_offsets(void* tmp, size_t tmp_bytes, const uint32_t* len, const uint32_t* perm, uint64_t n,
                               uint64_t* slen, uint64_t* doff, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sort_lens, dim3(blocks_for(n + 1)), dim3(kSortThreads), 0, s, len, perm, n, slen);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, slen, doff, (int)(n + 1), s);
}

hipError_t launch_sort_gather(const uint8_t* u, const uint64_t* rec_pos, const int32_t* ref_id, const uint32_t* perm,
                              const uint64_t* doff, uint64_t n, uint64_t total, uint8_t* dst, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint64_t tiles = (total + kSortTile - 1) / kSortTile;
  hipLaunchKernelGGL(k_sort_gather<false>, dim3((unsigned)tiles), dim3(kSortThreads), 0, s, u, rec_pos, ref_id, perm,
                     doff, (uint32_t)n, total, dst, (uint64_t)0);
  return hipGetLastError();
}

hipError_t launch_sort_words(const Columns& col, uint64_t n, int order, uint64_t* word, uint32_t* len, uint32_t* iota,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sort_words, dim3(blocks_for(n)), dim3(kSortThreads), 0, s, col.key, col.ref_id, col.pos,
                     col.rest_len, n, order, word, len, iota);
  return hipGetLastError();
}

hipError_t launch_merge_gather(const uint8_t* u, const uint64_t* src_pos, const uint64_t* doff, uint64_t n,
                               uint64_t dbase, uint64_t total, uint8_t* dst, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint64_t tiles = (total + kSortTile - 1) / kSortTile;
  hipLaunchKernelGGL(k_sort_gather<true>, dim3((unsigned)tiles), dim3(kSortThreads), 0, s, u, src_pos, nullptr,
                     nullptr, doff, (uint32_t)n, total, dst, dbase);
  return hipGetLastError();
}

}  // namespace hbam
