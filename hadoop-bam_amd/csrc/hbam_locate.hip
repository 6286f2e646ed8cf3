// hbam_locate.hip -- gfx950 kernels of BGZF block discovery.
//
//   bgzf_scan -> sort -> bgzf_verify (bgzf_walk fallback)   BGZF block discovery
//        ([htsjdk] BlockCompressedInputStream.readBlock; heuristic twin
//         BaseSplitGuesser.java:31-108)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "hbam_dev_util.h"
#include "hbam_device.h"
#include "hbam_launch.h"

namespace hbam {

// BGZF block discovery
// A candidate is a position whose 16 header bytes read 1f 8b 08 04 .. .. .. ..
// .. .. 06 00 'B' 'C' 02 00 (ID1 ID2 CM FLG, XLEN=6, BC subfield, SLEN=2): the
// exact framing htsjdk writes and requires (XLEN==6), plus the BC subfield id
// for selectivity.  Candidates are appended unordered, sorted, then the BSIZE
// chain is verified; any break falls back to the serial walk (bgzf_walk).
__global__ __launch_bounds__(256) void k_bgzf_scan(const uint8_t* __restrict__ buf, uint64_t len, uint64_t base,
                                                   uint64_t from, uint64_t* __restrict__ cand, uint32_t cap,
                                                   uint32_t* __restrict__ count) {
  // buf = first byte of the loaded range (16 B aligned, zero padded past
  // len).  Lane i of a wave step reads 16 B chunk c = step + i: one coalesced
  // 1 KiB load per wave (64 B per lane, as before, strided the wave's loads
  // 64 B apart and ran at 2.2 TB/s).  The 4 bytes after a chunk, which a
  // header starting in its last 3 bytes needs, come from the next lane's
  // chunk (a lane shuffle; the wave's last lane loads them).  A word without
  // a 0x1f byte (nearly all of them) costs three VALU operations; the rare
  // 0x1f bytes get the full header test.  Candidates are reported in file
  // coordinates (base + offset).
  // Four such wave steps per iteration (4 KiB per wave), their loads issued
  // together: one load in flight per wave left the scan latency-bound.  The
  // last lane's 4 bytes past the iteration's last chunk are loaded with them
  // (loaded at their use, they cost a second memory latency per iteration).
#ifndef HBAM_SCAN_U
#define HBAM_SCAN_U 4
#endif
#ifndef HBAM_SCAN_PIPE
#define HBAM_SCAN_PIPE 1
#endif
#ifndef HBAM_SCAN_GRID
#define HBAM_SCAN_GRID 8192
#endif
  constexpr int kU = HBAM_SCAN_U;
  // Candidates are collected per workgroup in LDS and reserved in cand[] by
  // one global atomic per workgroup: every candidate's own atomicAdd on one
  // device-scope counter serialized across the 8 XCDs.
  constexpr uint32_t kWgCand = 256;
  __shared__ uint64_t s_cand[kWgCand];
  __shared__ uint32_t s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint64_t nc = (len + 15) / 16;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * kU;
  const uint32_t lane = lane_id();
  const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) * kU;
  // the iteration's kU chunks per lane and the last lane's 4 bytes past them
  // (buf is zero padded past len)
  auto fetch = [&](uint64_t c0, uint4* vv, uint32_t& tail) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const uint64_t c = c0 + 64 * u + lane;
      vv[u] = c < nc ? reinterpret_cast<const uint4*>(buf)[c] : make_uint4(0, 0, 0, 0);
    }
    const uint64_t clast = c0 + 64 * (kU - 1) + 63;
    tail = lane == 63 && clast < nc ? *reinterpret_cast<const uint32_t*>(buf + 16 * clast + 16) : 0u;
  };
#if HBAM_SCAN_PIPE
  // software-pipelined: the next iteration's loads are in flight while this
  // one's chunks are tested
  uint4 nv[kU];
  uint32_t ntail = 0;
  if (wave0 < nc) fetch(wave0, nv, ntail);
#endif
  for (uint64_t c0 = wave0; c0 < nc; c0 += stride) {
    uint4 vv[kU];
    uint32_t tail;
#if HBAM_SCAN_PIPE
#pragma unroll
    for (int u = 0; u < kU; ++u) vv[u] = nv[u];
    tail = ntail;
    if (c0 + stride < nc) fetch(c0 + stride, nv, ntail);
#else
    fetch(c0, vv, tail);
#endif
#pragma unroll
    for (int u = 0; u < kU; ++u) {
    const uint64_t c = c0 + 64 * u + lane;  // the wave stays converged through the shuffle
    const uint4 v = vv[u];
    uint32_t nx = (uint32_t)__shfl_down((int)v.x, 1, 64);
    // the wave's last lane: the next step's first chunk (lane 0), or the tail
    const uint32_t next0 = u + 1 < kU ? (uint32_t)__shfl((int)vv[u + 1 < kU ? u + 1 : u].x, 0, 64) : 0u;
    if (lane == 63) nx = u + 1 < kU ? next0 : tail;
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, nx};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = w[k] ^ 0x1f1f1f1fu;
      uint32_t hz = (x - 0x01010101u) & ~x & 0x80808080u;  // a byte of w[k] may be 0x1f (superset)
      while (hz) {
        const uint32_t byte = (uint32_t)__builtin_ctz(hz) >> 3;
        hz &= hz - 1;
        const uint32_t magic = __builtin_amdgcn_alignbyte(w[k + 1], w[k], byte);
        if (magic != 0x04088b1fu) continue;
        const uint64_t p = 16 * c + 4 * k + byte;
        if (p + 18 > len || base + p < from) continue;
        const uint32_t xlen = ldu32(buf, p + 10) & 0xffffu;
        const uint32_t sub = ldu32(buf, p + 12);
        if (xlen != 6 || sub != 0x00024342u) continue;
        const uint32_t j = atomicAdd(&s_n, 1u);
        if (j < kWgCand) {
          s_cand[j] = base + p;
        } else {  // (more than kWgCand block headers in one workgroup's range: tiny blocks)
          const uint32_t i = atomicAdd(count, 1u);
          if (i < cap) cand[i] = base + p;
        }
      }
    }
    }
  }
  __syncthreads();
  const uint32_t nw = min(s_n, kWgCand);
  if (threadIdx.x == 0) s_base = nw ? atomicAdd(count, nw) : 0u;
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < nw; t += blockDim.x)
    if (s_base + t < cap) cand[s_base + t] = s_cand[t];
}

// ---------------------------------------------------------------------------
// Anchored locate: the block table of a range whose start is a known block
// start, from a fraction of its bytes.  The range is cut into segments of
// seg bytes; segment j = [lo + j * seg, min(lo + (j + 1) * seg, hi)).
//   k_bgzf_anchor_walk  one wave per segment: the segment's anchor (the first
//        header match whose successor matches too; lo for segment 0), then
//        the BSIZE walk from it up to the segment's end: block count and exit
//   k_bgzf_link         one workgroup: every walk's exit is the next
//        non-empty segment's anchor and the last exit reaches hi; the
//        exclusive scan of the counts
//   k_bgzf_seg_emit     one lane per segment: the walk again (its loads hit
//        L2), writing the block starts in file order
// Any doubt (a walk step that is no header, a broken link, a range not walked
// to hi) sets res[0]; the caller then runs the scan path.  Every loop is
// bounded: a search covers one segment, a walk step advances >= 26 bytes.
// ---------------------------------------------------------------------------
constexpr uint64_t kNoAnchor = ~0ull;
#ifndef HBAM_ANCHOR_U
#define HBAM_ANCHOR_U 4  // wave steps (1 KiB each) per search iteration
#endif

// the scan's header test at p (p + 18 <= the readable range) plus a BSIZE
// that holds a block: no weaker than k_bgzf_walk's framing rules
__device__ __forceinline__ bool bgzf_header_at(const uint8_t* __restrict__ file, uint64_t p, uint32_t* total) {
  const uint32_t w0 = ldu32(file, p);
  const uint32_t xlen = ldu32(file, p + 10) & 0xffffu;
  const uint32_t sub = ldu32(file, p + 12);
  *total = (ldu32(file, p + 16) & 0xffffu) + 1;
  return w0 == 0x04088b1fu && xlen == 6 && sub == 0x00024342u && *total >= 26;
}

// file: absolute file coordinates, 16 B aligned at offset 0 (as the scan).
// res[0] |= 1: declined.
__global__ __launch_bounds__(256) void k_bgzf_anchor_walk(const uint8_t* __restrict__ file, uint64_t lo, uint64_t hi,
                                                          uint64_t seg, uint32_t nseg, uint32_t partial,
                                                          uint64_t* __restrict__ anchor, uint64_t* __restrict__ exitp,
                                                          uint32_t* __restrict__ cnt, uint32_t* __restrict__ res) {
  const uint32_t j = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;  // wave-uniform
  if (j >= nseg) return;
  const uint32_t lane = lane_id();
  const uint64_t s0 = lo + (uint64_t)j * seg;
  const uint64_t end = s0 + seg < hi ? s0 + seg : hi;
  uint64_t a = j == 0 ? lo : kNoAnchor;
  if (j != 0) {
    // The scan's wave step: lane i reads 16 B chunk c0 + i (one coalesced
    // 1 KiB load), four steps per iteration, the next iteration's loads in
    // flight while this one's chunks are tested.  The first iteration with
    // an anchor holds the segment's first one: iterations are in file order.
    constexpr int kU = HBAM_ANCHOR_U;
    const uint4* chunks = reinterpret_cast<const uint4*>(file);
    const uint64_t cend = (end + 15) / 16;
    auto fetch = [&](uint64_t c0, uint4* vv, uint32_t& tail) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint64_t c = c0 + 64 * u + lane;
        vv[u] = c < cend ? chunks[c] : make_uint4(0, 0, 0, 0);
      }
      const uint64_t clast = c0 + 64 * (kU - 1) + 63;  // (the file is padded past hi)
      tail = lane == 63 && clast < cend ? *reinterpret_cast<const uint32_t*>(file + 16 * clast + 16) : 0u;
    };
    uint4 nv[kU];
    uint32_t ntail = 0;
    const uint64_t cfirst = s0 / 16;
    fetch(cfirst, nv, ntail);
    for (uint64_t c0 = cfirst; c0 < cend && a == kNoAnchor; c0 += 64 * kU) {
      uint4 vv[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) vv[u] = nv[u];
      const uint32_t tail = ntail;
      if (c0 + 64 * kU < cend) fetch(c0 + 64 * kU, nv, ntail);
      uint64_t best = kNoAnchor;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const uint64_t c = c0 + 64 * u + lane;
        const uint4 v = vv[u];
        uint32_t nx = (uint32_t)__shfl_down((int)v.x, 1, 64);
        const uint32_t next0 = u + 1 < kU ? (uint32_t)__shfl((int)vv[u + 1 < kU ? u + 1 : u].x, 0, 64) : 0u;
        if (lane == 63) nx = u + 1 < kU ? next0 : tail;
        const uint32_t w[5] = {v.x, v.y, v.z, v.w, nx};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t x = w[k] ^ 0x1f1f1f1fu;
          uint32_t hz = (x - 0x01010101u) & ~x & 0x80808080u;  // a byte of w[k] may be 0x1f (superset)
          while (hz) {
            const uint32_t byte = (uint32_t)__builtin_ctz(hz) >> 3;
            hz &= hz - 1;
            if (__builtin_amdgcn_alignbyte(w[k + 1], w[k], byte) != 0x04088b1fu) continue;
            const uint64_t p = 16 * c + 4 * k + byte;
            if (p < s0 || p >= end || p + 18 > hi || p >= best) continue;
            uint32_t total, t2;
            if (!bgzf_header_at(file, p, &total)) continue;
            const uint64_t q = p + total;  // the successor: a header too, or past the range
            if (q < hi && (q + 18 > hi || !bgzf_header_at(file, q, &t2))) continue;
            best = p;
          }
        }
      }
      if (__any(best != kNoAnchor)) a = wave_min_u64(best);
    }
  }
  if (lane != 0) return;
  // the BSIZE walk from the anchor to the segment's end.  The last block of
  // the range may be cut by hi: it is counted (k_bgzf_verify's partial rule
  // sees it) and ends the walk.
  uint64_t p = a;
  uint32_t n = 0;
  if (a != kNoAnchor) {
    while (p < end) {
      uint32_t total;
      if (p + 18 > hi || !bgzf_header_at(file, p, &total)) {
        atomicOr(&res[0], 1u);
        break;
      }
      ++n;
      p += total;
      if (p > hi) {
        if (!partial) atomicOr(&res[0], 1u);
        break;
      }
    }
  }
  anchor[j] = a;
  exitp[j] = a != kNoAnchor ? p : kNoAnchor;
  cnt[j] = n;
}

// One workgroup over all segments, thread t on a contiguous run of them.
// res[0] |= 1 on a broken link or a range not walked to hi, res[1] = the
// blocks of the range (saturated), offs[j] = the blocks before segment j.
constexpr int kLinkThreads = 1024;
struct LastExitOp {
  __device__ __forceinline__ uint64_t operator()(uint64_t x, uint64_t y) const { return y != kNoAnchor ? y : x; }
};
__global__ __launch_bounds__(kLinkThreads) void k_bgzf_link(const uint64_t* __restrict__ anchor,
                                                            const uint64_t* __restrict__ exitp,
                                                            const uint32_t* __restrict__ cnt, uint32_t nseg,
                                                            uint64_t hi, uint32_t* __restrict__ offs,
                                                            uint32_t* __restrict__ res) {
  using ScanSum = hipcub::BlockScan<uint64_t, kLinkThreads>;
  __shared__ typename ScanSum::TempStorage tmp;
  const uint32_t per = (nseg + kLinkThreads - 1) / kLinkThreads;
  const uint32_t j0 = min(threadIdx.x * per, nseg), j1 = min(j0 + per, nseg);
  uint64_t sum = 0, last = kNoAnchor;
  for (uint32_t j = j0; j < j1; ++j) {
    sum += cnt[j];
    if (anchor[j] != kNoAnchor) last = exitp[j];
  }
  uint64_t before = 0, prev = kNoAnchor, total = 0;
  ScanSum(tmp).ExclusiveSum(sum, before, total);
  __syncthreads();
  ScanSum(tmp).ExclusiveScan(last, prev, kNoAnchor, LastExitOp());
  bool bad = false;
  for (uint32_t j = j0; j < j1; ++j) {
    offs[j] = before < 0xffffffffull ? (uint32_t)before : 0xffffffffu;
    before += cnt[j];
    const uint64_t a = anchor[j];
    if (a == kNoAnchor) continue;
    if (prev != kNoAnchor && prev != a) bad = true;  // (segment 0's anchor is lo itself)
    prev = exitp[j];
  }
  // the chain's last exit: hi, or past it (a cut block, which the walk judged)
  if (threadIdx.x == kLinkThreads - 1 && (prev == kNoAnchor || prev < hi)) bad = true;
  if (bad) atomicOr(&res[0], 1u);
  if (threadIdx.x == 0) res[1] = total < 0xffffffffull ? (uint32_t)total : 0xffffffffu;
}

// The block starts of every segment at its offset: the checked walk again.
__global__ void k_bgzf_seg_emit(const uint8_t* __restrict__ file, const uint64_t* __restrict__ anchor,
                                const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offs, uint32_t nseg,
                                uint32_t cap, uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nseg) return;
  uint64_t p = anchor[j];
  const uint32_t n = cnt[j], o = offs[j];
  for (uint32_t i = 0; i < n && o + i < cap; ++i) {
    out[o + i] = p;
    p += (ldu32(file, p + 16) & 0xffffu) + 1;
  }
}

// Verify the sorted candidate chain and fill BlockInfo.  flags[0] |= 1 on any
// break (fallback), flags[1] = first block index with ISIZE > 64 KiB,
// flags[3] += the empty blocks (ISIZE 0: candidates for dead positions).
// partial (streamed upload, bytes past hi not there yet): a last candidate
// whose block runs past hi is the incomplete tail -> flags[2] = 1, not a break.
__global__ void k_bgzf_verify(const uint8_t* __restrict__ file, uint64_t lo, uint64_t hi,
                              const uint64_t* __restrict__ cand, uint32_t n,
                              BlockInfo* __restrict__ blocks, uint32_t* __restrict__ flags, uint32_t partial) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t c = cand[i];
  if (i == 0 && c != lo) atomicOr(&flags[0], 1u);
  uint32_t total = (ldu32(file, c + 16) & 0xffffu) + 1;
  uint64_t next = c + total;
  uint64_t expect = (i + 1 < n) ? cand[i + 1] : hi;
  if (partial && i + 1 == n && next > hi && total >= 26) {
    flags[2] = 1u;
    return;
  }
  if (next != expect || total < 26) {
    atomicOr(&flags[0], 1u);
    return;
  }
  BlockInfo b;
  b.coff = c;
  b.ustart = 0;
  b.csize = total;
  b.crc = ldu32(file, next - 8);
  b.isize = ldu32(file, next - 4);
  b.flags = 0;
  if (b.isize > kMaxIsize) atomicMin(&flags[1], i);
  if (b.isize == 0) atomicAdd(&flags[3], 1u);
  blocks[i] = b;
}

// Serial fallback: walk BSIZE from lo with htsjdk's framing rules.
// out[0] = nblocks, out[1] = status, out[2] = failing offset (low 32), out[3] = hi 32.
// partial: a block cut by hi ends the walk cleanly (out[2..3] = its start).
__global__ void k_bgzf_walk(const uint8_t* __restrict__ file, uint64_t lo, uint64_t hi,
                            BlockInfo* __restrict__ blocks, uint32_t cap, uint32_t* __restrict__ out,
                            uint32_t partial) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint64_t p = lo;
  uint32_t n = 0;
  int st = kOk;
  while (p < hi) {
    if (hi - p < 18) { st = partial ? kOk : kErrIO; break; }
    uint32_t total = (ldu32(file, p + 16) & 0xffffu) + 1;
    if (total < 18) { st = kErrIO; break; }
    if (p + total > hi) { st = partial ? kOk : kErrTrunc; break; }
    uint32_t w0 = ldu32(file, p);
    uint32_t xlen = ldu32(file, p + 10) & 0xffffu;
    if (w0 != 0x04088b1fu || xlen != 6 || total < 26) { st = kErrFormat; break; }
    if (n >= cap) { st = kErrState; break; }
    BlockInfo b;
    b.coff = p;
    b.ustart = 0;
    b.csize = total;
    b.crc = ldu32(file, p + total - 8);
    b.isize = ldu32(file, p + total - 4);
    b.flags = 0;
    if (b.isize > kMaxIsize) { st = kErrFormat; break; }
    blocks[n++] = b;
    p += total;
  }
  out[0] = n;
  out[1] = (uint32_t)st;
  out[2] = (uint32_t)p;
  out[3] = (uint32_t)(p >> 32);
}

__global__ void k_block_isize(const BlockInfo* __restrict__ blocks, uint32_t n, uint64_t* __restrict__ isz) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) isz[i] = blocks[i].isize;
}
__global__ void k_block_ustart(BlockInfo* __restrict__ blocks, uint32_t n, const uint64_t* __restrict__ us,
                               uint64_t base) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) blocks[i].ustart = base + us[i];
}

// ---- host launch wrappers (hbam_launch.h)
hipError_t launch_bgzf_scan(const uint8_t* file, uint64_t buf_base, uint64_t lo, uint64_t hi, uint64_t* cand,
                            uint32_t cap, uint32_t* count, hipStream_t s) {
  // scan from the 16 B aligned file offset at or below lo (windows are placed
  // so that file offsets keep their alignment; the bytes below buf_base are
  // allocated); candidates below lo are dropped
  (void)buf_base;
  const uint64_t a = lo & ~15ull;
  const uint64_t nc = (hi - a + 15) / 16;  // 16 B per lane and step, 4 steps per iteration
  hipLaunchKernelGGL(k_bgzf_scan, dim3(grid_for((nc + 3) / 4, 256, HBAM_SCAN_GRID)), dim3(256), 0, s, file + a, hi - a, a, lo,
                     cand, cap, count);
  return hipGetLastError();
}
hipError_t launch_bgzf_anchor_walk(const uint8_t* file, uint64_t lo, uint64_t hi, uint64_t seg, uint32_t nseg,
                                   uint32_t partial, uint64_t* anchor, uint64_t* exitp, uint32_t* cnt, uint32_t* offs,
                                   uint32_t* res, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_anchor_walk, dim3((nseg + 3) / 4), dim3(256), 0, s, file, lo, hi, seg, nseg, partial,
                     anchor, exitp, cnt, res);
  hipLaunchKernelGGL(k_bgzf_link, dim3(1), dim3(kLinkThreads), 0, s, anchor, exitp, cnt, nseg, hi, offs, res);
  return hipGetLastError();
}
hipError_t launch_bgzf_seg_emit(const uint8_t* file, const uint64_t* anchor, const uint32_t* cnt,
                                const uint32_t* offs, uint32_t nseg, uint32_t n, uint64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_seg_emit, dim3((nseg + 63) / 64), dim3(64), 0, s, file, anchor, cnt, offs, nseg, n, out);
  return hipGetLastError();
}
hipError_t launch_bgzf_verify(const uint8_t* file, uint64_t lo, uint64_t hi, const uint64_t* cand, uint32_t n,
                              BlockInfo* blocks, uint32_t* flags, uint32_t partial, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_bgzf_verify, dim3((n + 255) / 256), dim3(256), 0, s, file, lo, hi, cand, n, blocks, flags,
                     partial);
  return hipGetLastError();
}
hipError_t launch_bgzf_walk(const uint8_t* file, uint64_t lo, uint64_t hi, BlockInfo* blocks, uint32_t cap,
                            uint32_t* out, uint32_t partial, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf_walk, dim3(1), dim3(64), 0, s, file, lo, hi, blocks, cap, out, partial);
  return hipGetLastError();
}
hipError_t launch_block_ustart(BlockInfo* blocks, uint32_t n, uint64_t* tmp_isize, uint64_t* tmp_ustart,
                               void* scan_tmp, size_t* scan_bytes, uint64_t base, hipStream_t s) {
  if (scan_tmp == nullptr) {  // size query
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, tmp_isize, tmp_ustart, (int)n, s);
  }
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_block_isize, dim3((n + 255) / 256), dim3(256), 0, s, blocks, n, tmp_isize);
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, *scan_bytes, tmp_isize, tmp_ustart, (int)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_block_ustart, dim3((n + 255) / 256), dim3(256), 0, s, blocks, n, tmp_ustart, base);
  return hipGetLastError();
}
hipError_t sort_u64(void* tmp, size_t* tmp_bytes, uint64_t* keys_in, uint64_t* keys_out, uint32_t n,
                    hipStream_t s) {
  return hipcub::DeviceRadixSort::SortKeys(tmp, *tmp_bytes, keys_in, keys_out, (int)n, 0, 64, s);
}
hipError_t scan_u32_to_u64(void* tmp, size_t* tmp_bytes, const uint32_t* in, uint64_t* out, uint32_t n,
                           hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, (int)n, s);
}

}  // namespace hbam
