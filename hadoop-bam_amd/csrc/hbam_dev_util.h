// hbam_dev_util.h -- device helpers the kernel files share: unaligned loads,
// the record head, wave primitives, the 16-byte shifted load, and the
// launchers' grid_for.  Device code only, but for grid_for: a static inline host
// helper that also reaches the files that include this through hbam_align_end.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbam {

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// unaligned little-endian u32 from a 4-aligned base (reads 8 bytes: pad!)
__device__ __forceinline__ uint32_t ldu32(const uint8_t* base, uint64_t off) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(base + (off & ~3ull));
  uint32_t lo = p[0], hi = p[1];
  return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(off & 3));
}
__device__ __forceinline__ uint64_t ldu64(const uint8_t* base, uint64_t off) {
  return (uint64_t)ldu32(base, off) | ((uint64_t)ldu32(base, off + 4) << 32);
}

// A record's block_size and 32 fixed-field bytes (q .. q + 36) from three
// dword-aligned loads (two dwordx4, one dwordx2) instead of one ldu32 (two
// dword loads) per field: the record walks and the check/output pass issue
// ~6x fewer load instructions per record.  at(k) = the u32 at q + 4k, k <= 8.
// Reads up to 3 bytes past q + 36 (the stream is padded).
struct __attribute__((aligned(4))) U32x4 { uint32_t x, y, z, w; };
struct __attribute__((aligned(4))) U32x2 { uint32_t x, y; };
struct RecHead {
  uint32_t w[10];
  uint32_t sh;
  __device__ __forceinline__ uint32_t at(int k) const { return __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh); }
};
__device__ __forceinline__ RecHead load_head(const uint8_t* base, uint64_t q) {
  const uint8_t* b = base + (q & ~3ull);
  const U32x4 a = *reinterpret_cast<const U32x4*>(b);
  const U32x4 c = *reinterpret_cast<const U32x4*>(b + 16);
  const U32x2 d = *reinterpret_cast<const U32x2*>(b + 32);
  RecHead h;
  h.w[0] = a.x; h.w[1] = a.y; h.w[2] = a.z; h.w[3] = a.w;
  h.w[4] = c.x; h.w[5] = c.y; h.w[6] = c.z; h.w[7] = c.w;
  h.w[8] = d.x; h.w[9] = d.y;
  h.sh = (uint32_t)(q & 3);
  return h;
}

// ---- wave primitives
// Inclusive wave scan on DPP (VALU lane moves, no LDS round trip): Hillis-Steele
// inside each 16-lane row, then row_bcast:15 / row_bcast:31 carry the row totals.
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
  return v;
}

// Inclusive wave max-scan on DPP (as wave_incl_scan_dpp; 0 is the identity).
__device__ __forceinline__ uint32_t wave_incl_max_dpp(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));   // row_shr:1
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));   // row_shr:2
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));   // row_shr:4
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));   // row_shr:8
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));  // row_bcast:15
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += t;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint32_t l2 = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t h2 = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    const uint64_t v2 = ((uint64_t)h2 << 32) | l2;
    v = v2 < v ? v2 : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_incl_sum64(uint64_t v) {
  const uint32_t lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ int64_t wave_max_i64(int64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d, 64);
    v = max(v, (int64_t)(((uint64_t)hi << 32) | lo));
  }
  return v;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// a cigar longer than this many operators is walked by a whole wave
// (record_invalid_wave, hbam_chain.hip; cigar_ref_len, hbam_align_end.h)
constexpr uint32_t kWaveCigarOps = 32;

// 16 bytes starting sh bytes into the 32-byte pair (a, b)
__device__ __forceinline__ uint4 shift16(const uint4 a, const uint4 b, uint32_t sh) {
  const uint32_t r = sh & 3;
  uint32_t w0, w1, w2, w3, w4;
  switch (sh >> 2) {
    case 0: w0 = a.x; w1 = a.y; w2 = a.z; w3 = a.w; w4 = b.x; break;
    case 1: w0 = a.y; w1 = a.z; w2 = a.w; w3 = b.x; w4 = b.y; break;
    case 2: w0 = a.z; w1 = a.w; w2 = b.x; w3 = b.y; w4 = b.z; break;
    default: w0 = a.w; w1 = b.x; w2 = b.y; w3 = b.z; w4 = b.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r),
                    __builtin_amdgcn_alignbyte(w3, w2, r), __builtin_amdgcn_alignbyte(w4, w3, r));
}

// host: the grid of a launch of bs threads per workgroup over n items
static inline unsigned grid_for(uint64_t n, unsigned bs, unsigned cap = 65535u * 4) {
  uint64_t g = (n + bs - 1) / bs;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

}  // namespace hbam
