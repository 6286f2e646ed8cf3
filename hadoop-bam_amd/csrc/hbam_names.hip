// hbam_names.hip -- gfx950 kernels that order records by read name
// (HBAM_SORT_QUERYNAME): the name's bytes zero-extended and compared as
// unsigned bytes, then the tie word from the flag, then the input order.  The
// key is a byte string of up to 255 bytes at any alignment, so the order is an
// LSD radix sort over its 8-byte big-endian chunks, least significant key
// first, each pass stable:
//
//   k_name_refs    per record: where its name starts (rec_pos + 36), its length
//        min(l_read_name, rest_len) and its tie word (the window sort and the
//        merge's runs both start from decoded columns); the window sort also
//        takes the encoded length, 36 + rest_len, from it
//   k_name_census  per chunk index: the OR and the AND of every record's chunk
//        word (a record that ends before the chunk counts as the zero word),
//        the same for the tie word, and the fewest / most chunks of a record.
//        Reduced in the wave, then in LDS, then one global atomic per word and
//        workgroup.  or ^ and = the bits in which the records differ.
//   (host)         one read-back of the census: a chunk whose records do not
//        differ is skipped (a stable sort of equal keys is the identity), the
//        others sort only bits [ctz(diff), 64 - clz(diff))
//   k_name_iota    perm = 0 .. n - 1
//   k_name_words   word[j] = the tie word / chunk c of record perm[j]
//   (hipcub)       SortPairs(word, perm) on the pass's bit range
//
// launch_name_order takes per-record references (base, name_pos, name_len, tie),
// not a pipeline span, so hbam_sort_writables and hbam_merge_plan share it.
// k_name_sorted is the merge's check that a run is in this order.
//
// Loads: a chunk is read as one or two aligned 8-byte words, each of which holds
// at least one byte of the name, so no load leaves the record by more than the
// 7 bytes after its last byte (the sources are readable >= 16 bytes past their
// last record; the merge's packed names are padded by 8).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_launch.h"

namespace hbam {

namespace {

constexpr uint32_t kNameThreads = 256;
constexpr uint32_t kNameWave = 64;
constexpr uint32_t kNameMaxBlocks = 2048;  // the census strides: its global atomics do not grow with n past this

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kNameThreads - 1) / kNameThreads); }

// chunk c of the name at p: bytes [8c, 8c + 8) big-endian, zero past len
__device__ __forceinline__ uint64_t name_chunk(const uint8_t* p, uint32_t len, uint32_t c) {
  const uint32_t at = 8 * c;
  if (at >= len) return 0;
  const uint32_t valid = min(len - at, 8u);
  const uintptr_t a = reinterpret_cast<uintptr_t>(p + at);
  const uint32_t sh = (uint32_t)(a & 7);
  const uint64_t* q = reinterpret_cast<const uint64_t*>(a - sh);
  uint64_t v = q[0] >> (8 * sh);
  if (sh + valid > 8) v |= q[1] << (64 - 8 * sh);  // (sh > 0 here)
  if (valid < 8) v &= (1ull << (8 * valid)) - 1;
  return __builtin_bswap64(v);
}

__device__ __forceinline__ uint32_t tie_word(uint32_t flag) {
  uint32_t m = 3;
  if (flag & 0x1) {
    const uint32_t ends = flag & 0xc0;
    m = ends == 0x40 ? 0 : ends == 0x80 ? 2 : 1;
  }
  return 2 * m + ((flag & 0x900) ? 1u : 0u);
}

__global__ __launch_bounds__(kNameThreads) void k_name_refs(const uint64_t* __restrict__ rec_pos,
                                                            const uint8_t* __restrict__ l_read_name,
                                                            const uint32_t* __restrict__ rest_len,
                                                            const uint16_t* __restrict__ flag, uint64_t n,
                                                            uint64_t* __restrict__ name_pos,
                                                            uint8_t* __restrict__ name_len,
                                                            uint8_t* __restrict__ tie, uint32_t* __restrict__ len) {
  const uint64_t i = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x;
  if (i >= n) return;
  if (len) len[i] = 36u + rest_len[i];
  name_pos[i] = rec_pos[i] + 36;
  name_len[i] = (uint8_t)min((uint32_t)l_read_name[i], rest_len[i]);
  tie[i] = (uint8_t)tie_word(flag[i]);
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
  for (uint32_t d = kNameWave / 2; d; d >>= 1) v |= __shfl_xor(v, d, kNameWave);
  return v;
}
__device__ __forceinline__ uint64_t wave_and(uint64_t v) {
#pragma unroll
  for (uint32_t d = kNameWave / 2; d; d >>= 1) v &= __shfl_xor(v, d, kNameWave);
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (uint32_t d = kNameWave / 2; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d, kNameWave));
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (uint32_t d = kNameWave / 2; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, kNameWave));
  return v;
}

// census (kNameCensusWords u64, preset by the launch), two halves of
// kNameCensusHalf words: [c] = OR and [half + c] = AND of chunk c over the
// records that reach it; [kNameCensusTie] of each half = the tie words' OR /
// AND; [kNameCensusChunks] = the most / the fewest chunks of a record.  A record
// that ends before chunk c holds the zero word there: its AND is applied by
// the host from the fewest-chunks word (every chunk index at or past it has a
// record that ends before it), and by the lanes here while their wave is still
// walking.
__global__ __launch_bounds__(kNameThreads) void k_name_census(const uint8_t* __restrict__ base,
                                                              const uint64_t* __restrict__ name_pos,
                                                              const uint8_t* __restrict__ name_len,
                                                              const uint8_t* __restrict__ tie, uint64_t n,
                                                              unsigned long long* __restrict__ census) {
  __shared__ unsigned long long s_or[kNameChunks], s_and[kNameChunks];
  __shared__ uint32_t s_misc[4];  // tie OR, tie AND, fewest chunks, most chunks
  if (threadIdx.x < kNameChunks) {
    s_or[threadIdx.x] = 0;
    s_and[threadIdx.x] = ~0ull;
  }
  if (threadIdx.x == 0) {
    s_misc[0] = 0;
    s_misc[1] = ~0u;
    s_misc[2] = ~0u;
    s_misc[3] = 0;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & (kNameWave - 1);
  uint32_t t_or = 0, t_and = ~0u, c_min = ~0u, c_max = 0;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kNameThreads; i0 < n; i0 += (uint64_t)gridDim.x * kNameThreads) {
    const uint64_t i = i0 + threadIdx.x;
    const bool live = i < n;
    const uint32_t len = live ? name_len[i] : 0;
    const uint32_t chunks = (len + 7) >> 3;
    const uint8_t* p = base + (live ? name_pos[i] : 0);
    if (live) {
      const uint32_t t = tie[i];
      t_or |= t;
      t_and &= t;
      c_min = min(c_min, chunks);
      c_max = max(c_max, chunks);
    }
    const uint32_t w_max = wave_max(chunks);  // (wave-uniform: the shuffles below see every lane)
    for (uint32_t c = 0; c < w_max; ++c) {
      const uint64_t w = name_chunk(p, len, c);  // 0 past the record's own chunks (and for a lane past n: len 0)
      const uint64_t o = wave_or(w);
      const uint64_t a = wave_and(live ? w : ~0ull);
      if (lane == 0) {
        atomicOr(&s_or[c], (unsigned long long)o);
        atomicAnd(&s_and[c], (unsigned long long)a);
      }
    }
  }
  t_or = (uint32_t)wave_or(t_or);
  t_and = (uint32_t)wave_and(t_and);
  c_min = wave_min(c_min);
  c_max = wave_max(c_max);
  if (lane == 0) {
    atomicOr(&s_misc[0], t_or);
    atomicAnd(&s_misc[1], t_and);
    atomicMin(&s_misc[2], c_min);
    atomicMax(&s_misc[3], c_max);
  }
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t < kNameChunks) {
    if (t < s_misc[3]) {  // one OR and one AND per chunk the workgroup's records reach
      atomicOr(&census[t], s_or[t]);
      atomicAnd(&census[kNameCensusHalf + t], s_and[t]);
    }
  } else if (t == kNameChunks) {
    atomicOr(&census[kNameCensusTie], (unsigned long long)s_misc[0]);
  } else if (t == kNameChunks + 1) {
    atomicAnd(&census[kNameCensusHalf + kNameCensusTie], (unsigned long long)s_misc[1]);
  } else if (t == kNameChunks + 2) {
    atomicMin(&census[kNameCensusHalf + kNameCensusChunks], (unsigned long long)s_misc[2]);
  } else if (t == kNameChunks + 3) {
    atomicMax(&census[kNameCensusChunks], (unsigned long long)s_misc[3]);
  }
}

__global__ __launch_bounds__(kNameThreads) void k_name_iota(uint32_t* __restrict__ perm, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x;
  if (i < n) perm[i] = (uint32_t)i;
}

// word[j] = chunk c of record perm[j]; c < 0: its tie word
__global__ __launch_bounds__(kNameThreads) void k_name_words(const uint8_t* __restrict__ base,
                                                             const uint64_t* __restrict__ name_pos,
                                                             const uint8_t* __restrict__ name_len,
                                                             const uint8_t* __restrict__ tie,
                                                             const uint32_t* __restrict__ perm, uint64_t n, int c,
                                                             uint64_t* __restrict__ word) {
  const uint64_t j = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = perm[j];
  word[j] = c < 0 ? (uint64_t)tie[r] : name_chunk(base + name_pos[r], name_len[r], (uint32_t)c);
}

// bad = the first record i > 0 whose (name, tie) is below record i - 1's (preset ~0)
__global__ __launch_bounds__(kNameThreads) void k_name_sorted(const uint8_t* __restrict__ base,
                                                              const uint64_t* __restrict__ name_pos,
                                                              const uint8_t* __restrict__ name_len,
                                                              const uint8_t* __restrict__ tie, uint64_t n,
                                                              unsigned long long* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x + 1;
  if (i >= n) return;
  const uint32_t la = name_len[i - 1], lb = name_len[i];
  const uint8_t* pa = base + name_pos[i - 1];
  const uint8_t* pb = base + name_pos[i];
  const uint32_t chunks = (max(la, lb) + 7) >> 3;
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint64_t a = name_chunk(pa, la, c), b = name_chunk(pb, lb, c);
    if (a < b) return;
    if (a > b) {
      atomicMin(bad, (unsigned long long)i);
      return;
    }
  }
  if (tie[i - 1] > tie[i]) atomicMin(bad, (unsigned long long)i);
}

// dst[at[i], at[i] + name_len[i]) = the name at src + name_pos[i]; name_pos[i] = dst_base + at[i]
__global__ __launch_bounds__(kNameThreads) void k_name_pack(const uint8_t* __restrict__ src,
                                                            uint64_t* __restrict__ name_pos,
                                                            const uint8_t* __restrict__ name_len,
                                                            const uint64_t* __restrict__ at, uint64_t n,
                                                            uint8_t* __restrict__ dst, uint64_t dst_base) {
  const uint64_t i = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = src + name_pos[i];
  uint8_t* q = dst + dst_base + at[i];
  const uint32_t len = name_len[i];
  for (uint32_t k = 0; k < len; ++k) q[k] = p[k];
  name_pos[i] = dst_base + at[i];
}

// len64[i] = name_len[i] (len64[n] = 0): the scan's input
__global__ __launch_bounds__(kNameThreads) void k_name_lens(const uint8_t* __restrict__ name_len, uint64_t n,
                                                            uint64_t* __restrict__ len64) {
  const uint64_t i = (uint64_t)blockIdx.x * kNameThreads + threadIdx.x;
  if (i < n) len64[i] = name_len[i];
  else if (i == n) len64[i] = 0;
}

}  // namespace

hipError_t launch_name_refs(const uint64_t* rec_pos, const Columns& col, uint64_t n, uint64_t* name_pos,
                            uint8_t* name_len, uint8_t* tie, uint32_t* len, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_name_refs, dim3(blocks_for(n)), dim3(kNameThreads), 0, s, rec_pos, col.l_read_name,
                     col.rest_len, col.flag, n, name_pos, name_len, tie, len);
  return hipGetLastError();
}

hipError_t launch_name_order(void* tmp, size_t tmp_bytes, const uint8_t* base, const uint64_t* name_pos,
                             const uint8_t* name_len, const uint8_t* tie, uint64_t n, uint64_t* word,
                             uint64_t* word2, uint32_t* scratch, uint32_t* perm, uint64_t* census,
                             NameReadback rb, void* rb_ctx, NameOrderStats* stats, hipStream_t s, bool full,
                             hipEvent_t after_census, hipEvent_t after_tie) {
  *stats = NameOrderStats();
  if (n == 0) return hipSuccess;
  // the OR words, the tie OR and the most-chunks word start at 0; the AND words, the tie AND and the
  // fewest-chunks word at all ones
  hipError_t e = hipMemsetAsync(census, 0, kNameCensusHalf * 8, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(census + kNameCensusHalf, 0xff, kNameCensusHalf * 8, s)) != hipSuccess) return e;
  const unsigned grid = blocks_for(n) < kNameMaxBlocks ? blocks_for(n) : kNameMaxBlocks;
  hipLaunchKernelGGL(k_name_census, dim3(grid), dim3(kNameThreads), 0, s, base, name_pos, name_len, tie, n,
                     reinterpret_cast<unsigned long long*>(census));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint64_t h[kNameCensusWords];
  if ((e = rb(rb_ctx, h, census, sizeof h, s)) != hipSuccess) return e;
  if (after_census && (e = hipEventRecord(after_census, s)) != hipSuccess) return e;
  const uint64_t* h_or = h;
  const uint64_t* h_and = h + kNameCensusHalf;
  const uint32_t most = (uint32_t)h_or[kNameCensusChunks], fewest = (uint32_t)h_and[kNameCensusChunks];
  if (most > kNameChunks || fewest > most) return hipErrorUnknown;  // (a name has at most 255 bytes)
  struct Pass {
    int c, lo, hi;
  } pass[kNameChunks + 1];
  uint32_t passes = 0;
  stats->chunks_present = most;
  // least significant key first: the tie word (c = -1), then the chunks from the last one down
  for (int k = 0; k <= (int)most; ++k) {
    const int c = k == 0 ? -1 : (int)most - k;
    uint64_t diff;
    if (c < 0) diff = (h_or[kNameCensusTie] ^ h_and[kNameCensusTie]) & 7;
    else diff = h_or[c] ^ ((uint32_t)c >= fewest ? 0 : h_and[c]);  // a record that ends before c: the zero word
    if (full && c >= 0) diff = ~0ull;  // (measurement: every chunk present, all 64 bits)
    if (!diff) continue;
    pass[passes].c = c;
    pass[passes].lo = __builtin_ctzll(diff);
    pass[passes].hi = 64 - __builtin_clzll(diff);
    ++passes;
  }
  // the passes ping-pong between scratch and perm and end in perm
  uint32_t* cur = (passes & 1) ? scratch : perm;
  uint32_t* other = (passes & 1) ? perm : scratch;
  hipLaunchKernelGGL(k_name_iota, dim3(blocks_for(n)), dim3(kNameThreads), 0, s, cur, n);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (after_tie && (passes == 0 || pass[0].c >= 0) && (e = hipEventRecord(after_tie, s)) != hipSuccess) return e;
  for (uint32_t k = 0; k < passes; ++k) {
    const Pass& ps = pass[k];
    hipLaunchKernelGGL(k_name_words, dim3(blocks_for(n)), dim3(kNameThreads), 0, s, base, name_pos, name_len, tie,
                       cur, n, ps.c, word);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, word, word2, cur, other, (int)n, ps.lo, ps.hi, s);
    if (e != hipSuccess) return e;
    uint32_t* t = cur;
    cur = other;
    other = t;
    if (after_tie && ps.c < 0 && (e = hipEventRecord(after_tie, s)) != hipSuccess) return e;
    if (ps.c >= 0) {
      ++stats->chunks_sorted;
      stats->bits_sorted += (uint64_t)(ps.hi - ps.lo);
    }
  }
  return hipSuccess;
}

hipError_t launch_name_sorted(const uint8_t* base, const uint64_t* name_pos, const uint8_t* name_len,
                              const uint8_t* tie, uint64_t n, unsigned long long* bad, hipStream_t s) {
  if (n < 2) return hipSuccess;
  hipLaunchKernelGGL(k_name_sorted, dim3(blocks_for(n - 1)), dim3(kNameThreads), 0, s, base, name_pos, name_len, tie,
                     n, bad);
  return hipGetLastError();
}

hipError_t launch_name_starts(void* tmp, size_t tmp_bytes, const uint8_t* name_len, uint64_t n, uint64_t* len64,
                              uint64_t* at, hipStream_t s) {
  hipLaunchKernelGGL(k_name_lens, dim3(blocks_for(n + 1)), dim3(kNameThreads), 0, s, name_len, n, len64);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, len64, at, (int)(n + 1), s);
}

hipError_t launch_name_pack(const uint8_t* src, uint64_t* name_pos, const uint8_t* name_len, const uint64_t* at,
                            uint64_t n, uint8_t* dst, uint64_t dst_base, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_name_pack, dim3(blocks_for(n)), dim3(kNameThreads), 0, s, src, name_pos, name_len, at, n, dst,
                     dst_base);
  return hipGetLastError();
}

}  // namespace hbam
