// hbam_records.hip -- gfx950 kernels of record output and the SAMRecordWritable codec.
//
//   rec_out        fused field decode + sort key + voff
//        (LazyBAMRecordFactory.java:37-50; BAMRecordReader.java:81-121;
//         util/MurmurHash3.java:32-102); long_hash for rests > 2 KiB
//   sbi_emit       .splitting-bai entries (SplittingBAMIndexer.java:262-287)
//   wr_copy / wr_bin_patch / wr_decode   SAMRecordWritable.write / readFields
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hbam_dev_util.h"
#include "hbam_device.h"
#include "hbam_launch.h"
#include "hbam_record_dev.h"

namespace hbam {

// Murmur keys of long unmapped records (C4-like reads: the rest is tens of
// KB), one wave per record.  The per-block input mixing (k1*c1, rotl, *c2 and
// the k2 twin) is independent across 16 B blocks, so the 64 lanes do it for
// 64 consecutive blocks from one coalesced 1 KB load; only the h1/h2 chain is
// serial, and it runs on wave-uniform values (scalar ALU) fed by readlane.
__global__ __launch_bounds__(64) void k_long_hash(const uint8_t* __restrict__ u, const uint64_t* __restrict__ rec_pos,
                                                  Columns col, SpecGate gate) {
  if (gate_closed(gate)) return;
  const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
  const uint32_t lane = lane_id();
  const uint32_t nrec = min(*col.long_n, col.long_cap);
  for (uint32_t li = blockIdx.x; li < nrec; li += gridDim.x) {
    const uint64_t i = col.long_rec[li];
    const uint64_t q = rec_pos[i];
    const uint32_t len = ldu32(u, q) - 32u;
    const uint64_t off = q + 36;
    uint64_t h1 = 0, h2 = 0;  // seed 0 (BAMRecordReader.java:101)
    const uint32_t nblocks = len / 16;
    // the next 64 blocks are loaded while the serial chain runs over these
    uint64_t n1 = 0, n2 = 0;
    if (lane < nblocks) {
      n1 = ldu64(u, off + 16ull * lane);
      n2 = ldu64(u, off + 16ull * lane + 8);
    }
    for (uint32_t c = 0; c < nblocks; c += 64) {
      uint64_t k1 = n1, k2 = n2;
      const uint32_t nb = c + 64 + lane;
      n1 = n2 = 0;
      if (nb < nblocks) {
        n1 = ldu64(u, off + 16ull * nb);
        n2 = ldu64(u, off + 16ull * nb + 8);
      }
      k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2;
      k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1;
      const uint32_t k1lo = (uint32_t)k1, k1hi = (uint32_t)(k1 >> 32);
      const uint32_t k2lo = (uint32_t)k2, k2hi = (uint32_t)(k2 >> 32);
      const uint32_t m = min(64u, nblocks - c);
      for (uint32_t j = 0; j < m; ++j) {  // util/MurmurHash3.java:48-60, :59 quirk
        const uint64_t K1 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)k1hi, (int)j) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)k1lo, (int)j);
        const uint64_t K2 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)k2hi, (int)j) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)k2lo, (int)j);
        h1 ^= K1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        h2 ^= K2;
        h2 = (h2 << 31) | (h1 >> 33); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
      }
    }
    const uint64_t t = off + 16ull * nblocks;
    const uint32_t r = len & 15;
    if (r) {  // tail (:62-88), as murmur3_dev
      const uint64_t lo = ldu64(u, t), hi = ldu64(u, t + 8);
      if (r > 8) {
        uint64_t k2 = hi & (~0ull >> (64 - 8 * (r - 8)));
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
      }
      uint64_t k1 = r >= 8 ? lo : (lo & (~0ull >> (64 - 8 * r)));
      k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    }
    h1 ^= (uint64_t)len;
    h2 ^= (uint64_t)len;
    h1 += h2;
    h2 += h1;
    h1 = fmix64(h1);
    h2 = fmix64(h2);
    h1 += h2;
    if (lane == 0) col.key[i] = (int64_t)((0x7fffffffull << 32) | (uint64_t)(int64_t)(int32_t)h1);
  }
}

__global__ void k_rec_decode(const uint8_t* __restrict__ u, const uint64_t* __restrict__ rec_pos, uint64_t n,
                             Columns col) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    decode_record(u, rec_pos[i], i, col);
}

// .splitting-bai (SplittingBAMIndexer.java:273-277): the voff of every record
// whose global ordinal go = o0 + o satisfies (go + 1) % g == 0, at index
// (go + 1) / g - 1 - o0 / g (entries of earlier windows come before).
__global__ void k_sbi_emit(const uint64_t* __restrict__ voff, uint64_t n, uint32_t g, uint64_t o0,
                           uint64_t* __restrict__ ent) {
  const uint64_t k0 = o0 / g;
  for (uint64_t o = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; o < n;
       o += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t go = o0 + o;
    if ((go + 1) % g == 0) ent[(go + 1) / g - 1 - k0] = voff[o];
  }
}

// the chain successor of the last record of a span: where the next window
// (or the next batch of a split) resumes
__global__ void k_next_pos(const uint8_t* __restrict__ u, const uint64_t* __restrict__ rec_pos, uint64_t n,
                           uint64_t p0, int mode, uint64_t* __restrict__ out, SpecGate gate) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (gate_closed(gate)) return;
  if (n == 0) {
    *out = p0;
    return;
  }
  const uint64_t q = rec_pos[n - 1];
  const int32_t bs = (int32_t)ldu32(u, q);
  *out = q + 4 + (uint64_t)(mode == kReader ? bs : (bs > 0 ? bs : 0));
}

// Digests of a span (bench / test parity checks, not on the timed path):
// out[0] xor of the keys, out[1] sum of the voffs (order-independent), and
// the order-sensitive out[2] / out[3] = sum_i dmix(x_i) * P^(n-1-i) mod 2^64
// over keys / voffs (oracle/hbam_oracle.h ORC_DIGEST_P; composable across
// windows and ranks: D(A ++ B) = D(A) * P^|B| + D(B)).  Each thread takes a
// contiguous run of records (Horner), weighted by P^(records after the run).
__device__ __forceinline__ uint64_t dig_mix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
__device__ __forceinline__ uint64_t dig_pow(uint64_t b, uint64_t e) {
  uint64_t r = 1;
  for (; e; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}
constexpr uint64_t kDigestP = 0x100000001b3ull;

__global__ __launch_bounds__(256) void k_digest(const int64_t* __restrict__ keys, const uint64_t* __restrict__ voffs,
                                                uint64_t n, unsigned long long* __restrict__ out) {
  const uint64_t nt = (uint64_t)gridDim.x * blockDim.x, t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t per = (n + nt - 1) / nt;
  const uint64_t i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
  uint64_t kx = 0, vs = 0, kd = 0, vd = 0;
  for (uint64_t i = i0; i < i1; ++i) {
    const uint64_t v = voffs[i];
    vs += v;
    vd = vd * kDigestP + dig_mix(v);
    if (keys) {
      const uint64_t k = (uint64_t)keys[i];
      kx ^= k;
      kd = kd * kDigestP + dig_mix(k);
    }
  }
  const uint64_t w = dig_pow(kDigestP, n - i1);
  kd *= w;
  vd *= w;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    kx ^= (uint64_t)__shfl_xor((unsigned long long)kx, d, 64);
    vs += (uint64_t)__shfl_xor((unsigned long long)vs, d, 64);
    kd += (uint64_t)__shfl_xor((unsigned long long)kd, d, 64);
    vd += (uint64_t)__shfl_xor((unsigned long long)vd, d, 64);
  }
  if (lane_id() == 0) {
    atomicXor(&out[0], (unsigned long long)kx);
    atomicAdd(&out[1], (unsigned long long)vs);
    atomicAdd(&out[2], (unsigned long long)kd);
    atomicAdd(&out[3], (unsigned long long)vd);
  }
}

// ---------------------------------------------------------------------------
// Drop-in batch path (hbam_decode_span): a decoded window's records leave the
// pipeline's buffers for an export slot (so the next window decodes while
// this one's batches cross PCIe; the batches go to the host by SDMA copies
// of column slices).  HBM-bound copy, one thread per record: every column's
// stores coalesce across the wave.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void copy_record_fields(const Columns& s, uint64_t i, const Columns& d, uint64_t j,
                                                   uint64_t rest_base) {
  d.key[j] = s.key[i];
  d.rest_off[j] = s.rest_off[i] - rest_base;
  d.voff[j] = s.voff[i];
  d.ref_id[j] = s.ref_id[i];
  d.pos[j] = s.pos[i];
  d.l_seq[j] = s.l_seq[i];
  d.next_ref_id[j] = s.next_ref_id[i];
  d.next_pos[j] = s.next_pos[i];
  d.tlen[j] = s.tlen[i];
  d.rest_len[j] = s.rest_len[i];
  d.bin[j] = s.bin[i];
  d.n_cigar[j] = s.n_cigar[i];
  d.flag[j] = s.flag[i];
  d.l_read_name[j] = s.l_read_name[i];
  d.mapq[j] = s.mapq[i];
}

// Device -> page-locked host bytes written by the shader engines: a host
// read-back that never waits behind copy-engine traffic of other streams (a
// pageable hipMemcpy D2H of the block table queued ~13 ms behind a drop-in
// batch's D2H on another stream).
__global__ __launch_bounds__(256) void k_readback(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                                  uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    const uint64_t n16 = n >> 4;
    for (uint64_t i = t; i < n16; i += stride)
      reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    for (uint64_t i = (n16 << 4) + t; i < n; i += stride) dst[i] = src[i];
  } else {
    for (uint64_t i = t; i < n; i += stride) dst[i] = src[i];
  }
}

// host[i] <- *src[i] for i < n (n <= kGatherMax): a few scattered values read
// back by one launch, with no DMA-engine copy to queue behind larger ones
struct U64Srcs {
  const uint64_t* p[kGatherMax];
};
__global__ __launch_bounds__(64) void k_gather_u64(uint64_t* __restrict__ dst, U64Srcs src, int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = *src.p[i];
}

// slot <- records [0, n) of a span; positions rebased so that window position
// `base` (the first record's start) is slot byte 0; dpos[n] = the slot's bytes
// Also (packed != nullptr) the columns once more, batch-major: the records
// [b*m, b*m + m) of batch b as one ColLayout(m) block at packed + b * lf.bytes
// (the last, shorter batch as ColLayout(n - b*m) = ll), with rest_off counted
// in the packed rests (k_pack_rests) from the batch's first record -- exactly
// a drop-in host slot's column area, so a batch's columns cross PCIe as one
// copy instead of fifteen.
__global__ __launch_bounds__(256) void k_export_records(Columns s, const uint64_t* __restrict__ spos, Columns d,
                                                        uint64_t* __restrict__ dpos, uint64_t n, uint64_t base,
                                                        uint64_t nbytes, uint8_t* __restrict__ packed, ColLayout lf,
                                                        ColLayout ll, uint64_t m) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    copy_record_fields(s, i, d, i, base);
    dpos[i] = spos[i] - base;
    if (packed) {
      const uint64_t b = i / m, j = i - b * m;
      const bool last = (b + 1) * m > n;
      const Columns c = (last ? ll : lf).at(packed + b * lf.bytes, nullptr);
      copy_record_fields(s, i, c, j, spos[b * m]);
      c.rest_off[j] -= 36 * (j + 1);  // into the batch's packed rests (k_pack_rests)
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) dpos[n] = nbytes;
}

// ---------------------------------------------------------------------------
// SAMRecordWritable codec (SAMRecordWritable.java:55-68)
// ---------------------------------------------------------------------------
// write(): [htsjdk] BAMRecordCodec.encode of an unmodified BAMRecord emits
// block_size (= 32 + rest length), the fixed fields and the undecoded rest --
// the record's own bytes, except that indexBin is written as 0 when refID < 0.
// The records of a span lie back to back in the inflated stream, so the
// encodings of a span are u[p0, p0+n) copied into a 16 B-aligned buffer
// (k_wr_copy: HBM-bound, 2 B of traffic per byte) followed by the sparse bin
// patches (k_wr_bin_patch: 6 B of columns per record).

// Drop-in batches carry each record's rest only (read name .. aux): the 36
// bytes of block_size + fixed fields are in the columns already, and leaving
// them out cuts a batch's D2H by ~10 % (the drop-in loop is PCIe-bound).
// dst <- the rests of records [0, n) of a span, back to back: record i's rest
// lands at cp(i) = rest_off[i] - p0 - 36 (i + 1) (records are contiguous from
// p0, so cp(i + 1) = cp(i) + rest_len[i]).  A workgroup takes 256 records:
// their cp() in LDS, then 16-byte output chunks, each a shifted 16 B load
// when the chunk lies in one rest (most of them) and bytes otherwise.
constexpr uint32_t kPackRecs = 256;
__global__ __launch_bounds__(256) void k_pack_rests(const uint8_t* __restrict__ u,
                                                    const uint64_t* __restrict__ rest_off,
                                                    const uint32_t* __restrict__ rest_len, uint64_t n, uint64_t p0,
                                                    uint8_t* __restrict__ dst) {
  __shared__ uint64_t cp[kPackRecs + 1];
  const uint64_t r0 = (uint64_t)blockIdx.x * kPackRecs;
  if (r0 >= n) return;
  const uint32_t cnt = (uint32_t)min<uint64_t>(kPackRecs, n - r0), t = threadIdx.x;
  if (t < cnt) {
    const uint64_t c = rest_off[r0 + t] - p0 - 36 * (r0 + t + 1);
    cp[t] = c;
    if (t == cnt - 1) cp[cnt] = c + rest_len[r0 + t];
  }
  __syncthreads();
  const uint64_t lo = cp[0], hi = cp[cnt];
  const uint64_t skew = p0 + 36 * (r0 + 1);  // source = output + skew + 36 * (local record)
  for (uint64_t c = (lo & ~15ull) + 16ull * t; c < hi; c += 16ull * blockDim.x) {
    const uint64_t o0 = max(c, lo), o1 = min(c + 16, hi);
    uint32_t a = 0, b = cnt - 1;  // the last record with cp <= o0
    while (a < b) {
      const uint32_t mid = (a + b + 1) >> 1;
      if (cp[mid] <= o0) a = mid; else b = mid - 1;
    }
    if (o0 == c && o1 == c + 16 && cp[a + 1] >= c + 16) {
      const uint64_t src = c + skew + 36ull * a;
      const uint4* q = reinterpret_cast<const uint4*>(u + (src & ~15ull));
      *reinterpret_cast<uint4*>(dst + c) = shift16(q[0], q[1], (uint32_t)(src & 15));
    } else {
      for (uint64_t o = o0; o < o1; ++o) {
        while (cp[a + 1] <= o) ++a;
        dst[o] = u[o + skew + 36ull * a];
      }
    }
  }
}

constexpr int kWrUnroll = 4;  // 16 B chunks in flight per thread
// dst[0, 16*ceil(n/16)) = u[p0, ...): chunk c of the destination comes from
// the aligned source chunks c and c+1 (the stream is padded past its end).
__global__ __launch_bounds__(256) void k_wr_copy(const uint8_t* __restrict__ u, uint64_t p0, uint64_t n,
                                                 uint8_t* __restrict__ dst) {
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(u + (p0 & ~15ull));
  uint4* __restrict__ d = reinterpret_cast<uint4*>(dst);
  const uint32_t sh = (uint32_t)(p0 & 15);  // uniform: shift16 takes one of its four cases for the whole launch
  const uint64_t nch = (n + 15) >> 4;
  const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
  uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (; c + (kWrUnroll - 1) * T < nch; c += kWrUnroll * T) {  // kWrUnroll coalesced chunks per thread
    uint4 a[kWrUnroll], b[kWrUnroll];
#pragma unroll
    for (int k = 0; k < kWrUnroll; ++k) {
      a[k] = src[c + k * T];
      b[k] = src[c + k * T + 1];
    }
#pragma unroll
    for (int k = 0; k < kWrUnroll; ++k) d[c + k * T] = shift16(a[k], b[k], sh);
  }
  for (; c < nch; c += T) d[c] = shift16(src[c], src[c + 1], sh);
}

__global__ void k_wr_bin_patch(const uint64_t* __restrict__ rec_pos, const int32_t* __restrict__ ref_id,
                               const uint16_t* __restrict__ bin, uint64_t n, uint64_t p0, uint8_t* __restrict__ dst) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (ref_id[i] < 0 && bin[i] != 0) {  // [htsjdk] encode: indexBin = 0 unless refIndex >= 0
      const uint64_t q = rec_pos[i] - p0 + 14;
      dst[q] = 0;
      dst[q + 1] = 0;
    }
  }
}

// readFields(): [htsjdk] BAMRecordCodec.decode (LazyBAMRecordFactory, no
// header) once per framed value buf[offs[i], offs[i+1]) (the last ends at
// len).  The first failing value's index and status go to *bad
// ((i << 8) | status, atomicMin); values decode independently.
__global__ void k_wr_decode(const uint8_t* __restrict__ buf, uint64_t len, const uint64_t* __restrict__ offs,
                            uint64_t n, Columns col, uint64_t* __restrict__ rec_pos,
                            unsigned long long* __restrict__ bad) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = offs[i], e = i + 1 < n ? offs[i + 1] : len;
    uint32_t code = kOk;
    if (e < p || e > len) {
      code = kErrArg;
    } else if (e - p < 4) {
      code = kErrTrunc;  // readInt at EOF: decode() returns null
    } else {
      const int32_t bs = (int32_t)ldu32(buf, p);
      if (bs < 32) code = kErrFormat;                         // "Invalid record length"
      else if (e - p - 4 < (uint64_t)bs) code = kErrTrunc;    // readFully short: RuntimeEOFException
    }
    if (code != kOk) {
      atomicMin(bad, (unsigned long long)((i << 8) | code));
      continue;
    }
    decode_record(buf, p, i, col);
    col.voff[i] = kNone;  // a shuffled record has no file position
    rec_pos[i] = p;
  }
}

// ---- host launch wrappers (hbam_launch.h)
hipError_t launch_rec_decode(const uint8_t* u, const uint64_t* rec_pos, uint64_t n, const Columns& col,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_rec_decode, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, u, rec_pos, n, col);
  return hipGetLastError();
}
hipError_t launch_sbi_emit(const uint64_t* voff, uint64_t n, uint32_t g, uint64_t o0, uint64_t* ent, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sbi_emit, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, voff, n, g, o0, ent);
  return hipGetLastError();
}
hipError_t launch_next_pos(const uint8_t* u, const uint64_t* rec_pos, uint64_t n, uint64_t p0, int mode,
                           uint64_t* out, hipStream_t s, const unsigned long long* gate_bad,
                           const unsigned long long* gate_need, uint64_t gate_e_inf) {
  const SpecGate g{gate_bad, gate_need, gate_e_inf};
  hipLaunchKernelGGL(k_next_pos, dim3(1), dim3(64), 0, s, u, rec_pos, n, p0, mode, out, g);
  return hipGetLastError();
}
hipError_t launch_readback(void* dst, const void* src, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_readback, dim3(grid_for((n + 15) / 16, 256, 64)), dim3(256), 0, s,
                     static_cast<uint8_t*>(dst), static_cast<const uint8_t*>(src), n);
  return hipGetLastError();
}
hipError_t launch_pack_rests(const uint8_t* u, const uint64_t* rest_off, const uint32_t* rest_len, uint64_t n,
                             uint64_t p0, uint8_t* dst, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_rests, dim3((unsigned)((n + kPackRecs - 1) / kPackRecs)), dim3(256), 0, s, u, rest_off,
                     rest_len, n, p0, dst);
  return hipGetLastError();
}
hipError_t launch_gather_u64(uint64_t* dst, const uint64_t* const* src, int n, hipStream_t s) {
  if (n <= 0 || n > kGatherMax) return n == 0 ? hipSuccess : hipErrorInvalidValue;
  U64Srcs g{};
  for (int i = 0; i < n; ++i) g.p[i] = src[i];
  hipLaunchKernelGGL(k_gather_u64, dim3(1), dim3(64), 0, s, dst, g, n);
  return hipGetLastError();
}
hipError_t launch_export_records(const Columns& src, const uint64_t* src_pos, const Columns& dst, uint64_t* dst_pos,
                                 uint64_t n, uint64_t base, uint64_t nbytes, uint8_t* packed, uint64_t m,
                                 hipStream_t s) {
  const ColLayout lf(m ? m : 1, false), ll(m ? n - (n ? (n - 1) / m : 0) * m : 1, false);
  hipLaunchKernelGGL(k_export_records, dim3(grid_for(std::max<uint64_t>(n, 1), 256, 8192)), dim3(256), 0, s, src,
                     src_pos, dst, dst_pos, n, base, nbytes, m ? packed : nullptr, lf, ll, m ? m : 1);
  return hipGetLastError();
}
hipError_t launch_digest(const int64_t* keys, const uint64_t* voffs, uint64_t n, uint64_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_digest, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, keys, voffs, n,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}
hipError_t launch_wr_encode(const uint8_t* u, uint64_t p0, uint64_t nbytes, const uint64_t* rec_pos,
                            const int32_t* ref_id, const uint16_t* bin, uint64_t n, uint8_t* dst, hipStream_t s) {
  if (nbytes) {
    const uint64_t nch = (nbytes + 15) >> 4;
    // 8 workgroups of 256 per CU (2048 lanes x kWrUnroll chunks in flight each)
    const uint64_t grid = std::min<uint64_t>((nch + 255) / 256, 256ull * 8);
    hipLaunchKernelGGL(k_wr_copy, dim3((unsigned)std::max<uint64_t>(grid, 1)), dim3(256), 0, s, u, p0, nbytes, dst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wr_bin_patch, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, rec_pos, ref_id, bin, n, p0,
                     dst);
  return hipGetLastError();
}
hipError_t launch_long_hash(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, hipStream_t s,
                            const unsigned long long* gate_bad, const unsigned long long* gate_need,
                            uint64_t gate_e_inf) {
  if (!col.long_rec || col.long_cap == 0) return hipSuccess;
  const uint32_t grid = std::min<uint32_t>(col.long_cap, 256u * 16u);
  const SpecGate g{gate_bad, gate_need, gate_e_inf};
  hipLaunchKernelGGL(k_long_hash, dim3(grid), dim3(64), 0, s, u, rec_pos, col, g);
  return hipGetLastError();
}
hipError_t launch_wr_decode(const uint8_t* buf, uint64_t len, const uint64_t* offs, uint64_t n, const Columns& col,
                            uint64_t* rec_pos, unsigned long long* bad, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wr_decode, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, buf, len, offs, n, col, rec_pos,
                     bad);
  return hipGetLastError();
}

}  // namespace hbam
