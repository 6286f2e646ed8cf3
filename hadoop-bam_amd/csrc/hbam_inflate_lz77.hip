// hbam_inflate_lz77.hip -- gfx950 kernel of inflate phase B: LZ77 tokens -> bytes.
//
//   inflate_lz77   (phase B) one 1024-thread workgroup per BGZF block: tokens
//        -> a u16 LDS map (literal or source position), resolved by pointer
//        chasing with path compression, 16 B coalesced stores into the
//        contiguous inflated stream.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "hbam_dev_util.h"
#include "hbam_device.h"
#include "hbam_launch.h"

namespace hbam {

// Inflate phase B: tokens -> bytes, one 1024-thread workgroup per BGZF block
// Every output position p gets a u16 entry in an LDS map: 0xFF00|byte for a
// literal, else the position its byte is copied from (p - dist, strictly
// smaller; for an overlapping match this is the periodic extension, so every
// match is expanded in one parallel step).  Bytes are then resolved by
// following entries back to a literal and writing the result in place (path
// compression); positions are visited in increasing order so chains are
// short (measured on BAM data: mean depth 7.5, max ~40 without compression).
// The map needs ISIZE <= 65280 (positions below the 0xFF00 tag space: the
// BGZF maximum htsjdk/bgzip write); larger blocks take the dependency-round
// path over a byte image in the same LDS.
constexpr int kLzThreads = 1024;
constexpr int kLzWaves = kLzThreads / 64;
constexpr uint32_t kMapMax = 65280;
constexpr uint32_t kLitTag = 0xFF00u;
// map entries: 128 KiB, so that the 16 waves' 8 rows of 64 eight-entry chunks
// (step 3) cover it exactly and need no bounds (o0 + ISIZE <= 65295)
constexpr uint32_t kMapEntries = 65536;
static_assert(kMapEntries == kLzWaves * 8 * 64 * 8 && kMapMax + 15 < kMapEntries, "phase-B map geometry");
constexpr int kLzRing = 4;  // phase-B fill: 64-token groups loaded ahead (4 vs 8 measured equal)
constexpr int kLzTokGroups = 32;  // token groups a wave keeps in registers (32 K tokens per block)
#ifndef HBAM_LZ_CHASE
#define HBAM_LZ_CHASE 2
#endif
constexpr int kLzChase = HBAM_LZ_CHASE;  // positions chased together per thread (4: slower before pointer jumping)

// exclusive scan over the workgroup; returns the prefix, *total = sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
  const uint32_t lane = lane_id(), wid = threadIdx.x >> 6;
  const uint32_t inc = wave_incl_scan(v);
  if (lane == 63) scratch[wid] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kLzWaves; ++w) {
    const uint32_t x = scratch[w];
    off += (uint32_t)w < wid ? x : 0u;
    tot += x;
  }
  *total = tot;
  __syncthreads();
  return off + inc - v;
}

__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* scratch) {
  const uint32_t lane = lane_id(), wid = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  uint32_t r = 0xffffffffu;
#pragma unroll
  for (int w = 0; w < kLzWaves; ++w) r = min(r, scratch[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ uint32_t tok_len(uint32_t t) { return (t >> 31) ? (t & 0xffffu) : ((t >> 24) & 3u); }

// Rare path (ISIZE > 65280): byte image, matches resolve in dependency rounds.
__device__ void lz77_rounds(uint8_t* out, uint32_t* scratch, const uint32_t* tk, uint32_t ntok, uint32_t isize,
                            uint32_t o0) {
  uint32_t P = 0;
  for (uint32_t c = 0; c < ntok; c += kLzThreads) {
    const uint32_t i = c + threadIdx.x;
    const uint32_t t = i < ntok ? tk[i] : 0u;
    const bool ismatch = (t >> 31) != 0;
    const uint32_t len = i < ntok ? tok_len(t) : 0u;
    uint32_t total;
    const uint32_t pos = P + block_excl_scan(len, scratch, &total);
    P += total;
    if (!ismatch) {
      for (uint32_t j = 0; j < len; ++j)
        if (pos + j < isize) out[o0 + pos + j] = (uint8_t)(t >> (8 * j));
    }
    const uint32_t dist = ((t >> 16) & 0x7fffu) + 1;
    bool pending = ismatch && pos < isize;
    __syncthreads();
    for (;;) {
      const uint32_t first = block_min(pending ? pos : 0xffffffffu, scratch);
      if (first == 0xffffffffu) break;
      if (pending && (pos == first || pos - dist + min(len, dist) <= first)) {
        const uint32_t n = min(len, isize - pos);
        uint8_t* dst = out + o0 + pos;
        for (uint32_t k = 0; k < n; ++k) dst[k] = dst[(int)k - (int)dist];
        pending = false;
      }
      __syncthreads();
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kLzThreads) void k_inflate_lz77(const BlockInfo* __restrict__ blocks, uint32_t b0,
                                                             uint64_t chunk_ustart,
                                                             const uint32_t* __restrict__ tokens,
                                                             const HuffOut* __restrict__ hout,
                                                             uint8_t* __restrict__ u) {
  // map index = o0 + position, so 16-byte output segments read 32 B-aligned LDS
  __shared__ __attribute__((aligned(16))) uint16_t map[kMapEntries];
  __shared__ uint32_t scratch[kLzWaves];
  const BlockInfo blk = blocks[b0 + blockIdx.x];
  const HuffOut ho = hout[b0 + blockIdx.x];
  if (ho.status != kOk || blk.isize == 0) return;
  const uint32_t isize = blk.isize;
  const uint32_t o0 = (uint32_t)(blk.ustart & 15);
  const uint32_t* tk = tokens + (blk.ustart - chunk_ustart);
  const uint32_t ntok = ho.ntok;
  const uint32_t tid = threadIdx.x;
  const uint64_t g0 = blk.ustart & ~15ull;
  const uint64_t gend = blk.ustart + isize;
  const uint32_t nseg = (uint32_t)((gend - g0 + 15) >> 4);

  if (isize > kMapMax) {  // uniform per workgroup
    uint8_t* img = reinterpret_cast<uint8_t*>(map);
    lz77_rounds(img, scratch, tk, ntok, isize, o0);
    for (uint32_t s = tid; s < nseg; s += kLzThreads) {
      const uint64_t ga = g0 + 16ull * s;
      if (ga >= blk.ustart && ga + 16 <= gend) {
        *reinterpret_cast<uint4*>(u + ga) = *reinterpret_cast<const uint4*>(img + 16 * s);
      } else {
        for (int j = 0; j < 16; ++j) {
          const uint64_t g = ga + j;
          if (g >= blk.ustart && g < gend) u[g] = img[16 * s + j];
        }
      }
    }
    return;
  }

  // 1. wave w expands tokens [w*TW, (w+1)*TW); its output range starts at
  //    the byte total of the waves before it.  Up to kLzTokGroups groups of
  //    64 tokens stay in registers from this load to step 2 (all loads in
  //    flight at once); a wave with more re-reads them (L2) through a ring.
  const uint32_t wid = tid >> 6, lane = tid & 63;
  // 0. empty map: 0 marks a position no token writes (inside a match)
  auto zero_map = [&]() {
    for (uint32_t c = tid; c < kMapEntries / 8; c += kLzThreads)
      reinterpret_cast<uint4*>(map)[c] = make_uint4(0u, 0u, 0u, 0u);
  };
  const uint32_t TW = (ntok + kLzWaves - 1) / kLzWaves;
  const uint32_t tw0 = min(wid * TW, ntok), tw1 = min(tw0 + TW, ntok);
  const bool inreg = TW <= 64u * kLzTokGroups;  // uniform over the workgroup
  uint32_t tr[kLzTokGroups];
  uint32_t wsum = 0;
  if (inreg) {
#pragma unroll
    for (int k = 0; k < kLzTokGroups; ++k) {
      const uint32_t i = tw0 + lane + 64u * k;
      tr[k] = i < tw1 ? tk[i] : 0u;  // 0 = a literal token of length 0
    }
    zero_map();  // (while the loads are in flight)
#pragma unroll
    for (int k = 0; k < kLzTokGroups; ++k) wsum += tok_len(tr[k]);
  } else {
    zero_map();
    for (uint32_t i0 = tw0 + lane; i0 < tw1 + lane; i0 += 8 * 64) {  // 8 loads in flight
      uint32_t tv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) tv[k] = i0 + 64 * k < tw1 ? tk[i0 + 64 * k] : 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) wsum += tok_len(tv[k]);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) wsum += __shfl_xor(wsum, d, 64);
  if (lane == 0) scratch[wid] = wsum;
  __syncthreads();
  uint32_t P = 0;
#pragma unroll
  for (int w = 0; w < kLzWaves; ++w) P += (uint32_t)w < wid ? scratch[w] : 0u;
  const uint32_t whi = min(P + wsum, isize);  // end of this wave's range (the last token may run past ISIZE)

  // 2. token heads, 64 tokens (one per lane) at a time: a literal writes its
  //    1-2 entries (tag | byte), a match only its distance at its first
  //    position.  Every lane stores at most two entries, whatever the
  //    match lengths of its wave.
  uint16_t* m = map + o0;
  auto head = [&](uint32_t t) {
    const uint32_t len = tok_len(t);
    const uint32_t incl = wave_incl_scan_dpp(len);
    const uint32_t pos = P + incl - len;
    P += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (len != 0 && pos < whi) {
      if (t >> 31) {
        m[pos] = (uint16_t)(((t >> 16) & 0x7fffu) + 1);  // dist <= pos: checked in phase A
      } else {
        m[pos] = (uint16_t)(kLitTag | (t & 0xffu));
        if (len == 2 && pos + 1 < whi) m[pos + 1] = (uint16_t)(kLitTag | ((t >> 8) & 0xffu));
      }
    }
  };
  // one token's entries, branch-free selects and two predicated stores
  auto head_at = [&](uint32_t t, uint32_t len, uint32_t pos) {
    const bool mt = (t >> 31) != 0;
    const uint32_t e0 = mt ? ((t >> 16) & 0x7fffu) + 1u : (kLitTag | (t & 0xffu));  // dist <= pos: checked in phase A
    if ((len != 0) & (pos < whi)) m[pos] = (uint16_t)e0;
    if ((len == 2) & !mt & (pos + 1 < whi)) m[pos + 1] = (uint16_t)(kLitTag | ((t >> 8) & 0xffu));
  };
  if (inreg) {
    // two groups of 64 tokens per scan: their lengths packed in 16-bit
    // halves (a group's bytes <= 64 x 258 < 2^16)
#pragma unroll
    for (int j = 0; j < kLzTokGroups / 2; ++j) {
      if (tw0 + 128u * j >= tw1) break;  // wave-uniform
      const uint32_t t0 = tr[2 * j], t1 = tr[2 * j + 1];
      const uint32_t l0 = tok_len(t0), l1 = tok_len(t1);
      const uint32_t incl = wave_incl_scan_dpp(l0 | (l1 << 16));
      const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      const uint32_t p0 = P + (incl & 0xffffu) - l0;
      const uint32_t p1 = P + (tot & 0xffffu) + (incl >> 16) - l1;
      P += (tot & 0xffffu) + (tot >> 16);
      head_at(t0, l0, p0);
      head_at(t1, l1, p1);
    }
  } else {
    uint32_t ring[kLzRing];  // tokens of the next kLzRing groups (L2 hits after step 1)
#pragma unroll
    for (int k = 0; k < kLzRing; ++k) ring[k] = tw0 + lane + 64 * k < tw1 ? tk[tw0 + lane + 64 * k] : 0u;
    for (uint32_t gi = tw0; gi < tw1 && P < whi; gi += 64) {  // wave-uniform
      const uint32_t i = gi + lane;
      const uint32_t t = ring[0];
#pragma unroll
      for (int k = 0; k + 1 < kLzRing; ++k) ring[k] = ring[k + 1];
      ring[kLzRing - 1] = i + 64 * kLzRing < tw1 ? tk[i + 64 * kLzRing] : 0u;
      head(i < tw1 ? t : 0u);
    }
  }
  __syncthreads();

  // 3. match bodies: every 0 entry belongs to the match whose distance is the
  //    nearest non-zero entry before it that is not a literal, so a
  //    carry-forward over the map turns distances into source positions
  //    (q - dist).  Wave w owns 8-entry chunks [512w, 512w + 512), eight
  //    coalesced rows of 64 chunks held in registers.  The carry is a running
  //    max of keys (chunk + 1) << 16 | last non-zero entry of the chunk:
  //    keys grow with the position, so max-scans over rows, lanes (DPP) and
  //    waves (LDS) find the nearest non-zero entry before each chunk.
  {
    constexpr uint32_t kRowChunks = 64, kWaveChunks = 8 * kRowChunks;
    uint4* mc = reinterpret_cast<uint4*>(map);
    uint4 rows[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t c = wid * kWaveChunks + r * kRowChunks + lane;
      rows[r] = mc[c];  // (every chunk: entries past the block are zero or unused)
    }
    uint32_t key[8], kmax = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t w4[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
      uint32_t rl = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rl = (w4[j] & 0xffffu) ? (w4[j] & 0xffffu) : rl;
        rl = (w4[j] >> 16) ? (w4[j] >> 16) : rl;
      }
      const uint32_t c = wid * kWaveChunks + r * kRowChunks + lane;
      key[r] = rl ? ((c + 1u) << 16) | rl : 0u;
      kmax = max(kmax, key[r]);
    }
    const uint32_t wmax = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max_dpp(kmax), 63);
    if (lane == 0) scratch[wid] = wmax;
    __syncthreads();
    uint32_t carry = 0;  // key of the last non-zero entry before this wave's chunks
    for (uint32_t w = 0; w < wid; ++w) carry = max(carry, scratch[w]);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t incl = wave_incl_max_dpp(key[r]);
      const uint32_t excl = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x138, 0xf, 0xf, true);  // wave_shr:1
      uint32_t cur = max(carry, excl) & 0xffffu;
      carry = max(carry, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
      const uint32_t c = wid * kWaveChunks + r * kRowChunks + lane;
      // position of entry 0 of this chunk, relative to the block (index - o0)
      const uint32_t q0 = 8u * c - o0;
      uint32_t w4[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // inside the block a 0 entry follows its match's head, so a literal
        // stays and every other entry (a head's distance, or 0 in its body)
        // becomes q - cur, cur = the last non-zero entry (past the block the
        // values are unused)
        const uint32_t lo = w4[j] & 0xffffu, hi = w4[j] >> 16;
        cur = lo ? lo : cur;
        const uint32_t olo = lo < kLitTag ? q0 + 2u * j - cur : lo;
        cur = hi ? hi : cur;
        const uint32_t ohi = hi < kLitTag ? q0 + 2u * j + 1u - cur : hi;
        w4[j] = (olo & 0xffffu) | (ohi << 16);
      }
      mc[c] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
  }
  __syncthreads();

  // 4. resolve, increasing positions first; results written back in place
  //    (path compression).  Each chase step is one dependent LDS load, so a
  //    thread chases kLzChase positions 1024 apart at once (their loads
  //    overlap).  Any visiting order is correct: entries always point to
  //    smaller positions and a chase ends at a literal, resolved or not.
  // Branch-free steps: a resolved lane re-reads its own entry (no select,
  // no exec-masked read).
  for (uint32_t q = tid; q < isize; q += kLzChase * kLzThreads) {
    uint32_t v[kLzChase], at[kLzChase];
#pragma unroll
    for (int k = 0; k < kLzChase; ++k) {
      at[k] = q + k * kLzThreads < isize ? q + k * kLzThreads : q;
      v[k] = m[at[k]];
    }
    for (;;) {
      bool more = false;
#pragma unroll
      for (int k = 0; k < kLzChase; ++k) more |= v[k] < kLitTag;
      if (!__builtin_amdgcn_ballot_w64(more)) break;
      // min(v, at): an unresolved v is a smaller position than at; a
      // resolved lane (v >= kLitTag > at) re-reads its own entry, which
      // holds v (the literal it first read, or its last store below: only
      // this lane writes m[at]) -- so the value read is the new v either way
#pragma unroll
      for (int k = 0; k < kLzChase; ++k) v[k] = m[min(v[k], at[k])];
      // pointer jumping: every step stores how far the chase got, so a lane
      // whose chain runs through this position skips the hops already made
      // (a run of dist-1 matches resolves in ~log2(len) steps instead of
      // len).  Any stored value is a position holding the same byte, or the
      // byte itself, so racing stores keep every entry valid.  The last step
      // of a chase stores its byte, so nothing is written after the loop.
      // Every lane stores, branch-free (exec-masked stores of only the lanes
      // still chasing: 5.70 vs 5.43 ms per C2 pass).
#pragma unroll
      for (int k = 0; k < kLzChase; ++k) m[at[k]] = (uint16_t)v[k];
    }
  }
  __syncthreads();

  // 5. 16 B stores; low bytes of 16 entries packed with v_perm
  for (uint32_t s = tid; s < nseg; s += kLzThreads) {
    const uint64_t ga = g0 + 16ull * s;
    if (ga >= blk.ustart && ga + 16 <= gend) {
      const uint4 e0 = *reinterpret_cast<const uint4*>(map + 16 * s);
      const uint4 e1 = *reinterpret_cast<const uint4*>(map + 16 * s + 8);
      uint4 o;
      o.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x06040200u);
      o.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x06040200u);
      o.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x06040200u);
      o.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x06040200u);
      *reinterpret_cast<uint4*>(u + ga) = o;
    } else {
      for (int j = 0; j < 16; ++j) {
        const uint64_t g = ga + j;
        if (g >= blk.ustart && g < gend) u[g] = (uint8_t)map[16 * s + j];
      }
    }
  }
}

// ---- host launch wrappers (hbam_launch.h)
hipError_t launch_inflate_lz77(const BlockInfo* blocks, uint32_t b0, uint32_t nb, uint64_t chunk_ustart,
                               const uint32_t* tokens, const HuffOut* hout, uint8_t* u, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_inflate_lz77, dim3(nb), dim3(kLzThreads), 0, s, blocks, b0, chunk_ustart, tokens, hout, u);
  return hipGetLastError();
}

}  // namespace hbam
