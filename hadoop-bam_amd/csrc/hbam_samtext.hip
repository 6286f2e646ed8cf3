// hbam_samtext.hip -- gfx950 kernels that write the records of one decoded span
// as SAM text (hbam_format_sam: one line per record, the rules in include/hbam.h).
//
//   k_sam_measure  one wave per record: the line's length, the length of its
//        head (QNAME .. TLEN and the tab behind it) and the malformed-aux flag
//   (hipcub)       doff = exclusive sum of the lengths over n + 1 entries: the
//        line starts, doff[n] = the text's bytes
//   k_sam_write    the text, divided by output bytes as k_sort_gather divides
//        its output: a workgroup owns one 16 KiB tile of the text, formats it in
//        LDS and stores it in 16-byte chunks
//
// Both kernels run the same segment functions (sam_head, sam_seq_qual,
// sam_aux), the measuring one with the puts compiled out, so a line is as long
// as what is written into it.  A segment function is run by one wave whose
// lanes share the bytes: name and reference bytes, bases and qualities are
// dealt to the lanes by output byte; CIGAR operations and the elements of a B
// array are dealt 64 at a time, a wave prefix sum of their widths placing each
// lane's characters.  Only the aux tag chain is walked in turn, one tag per
// step, and every step is bounded by the record's end.  A record of at most
// kSamStage bytes is first copied into its wave's LDS stage (sam_stage), and what
// is the same in every lane is marked so (uni) and computed on the scalar unit.
//
// A line shorter than kSamLong belongs to one wave of its tile's workgroup (the
// lines of a tile go round the four waves); a longer one is worked on by the
// whole workgroup: bases and qualities by all four waves, the head by wave 0,
// the aux fields by wave 1.  A line that crosses tiles is formatted by each of
// them, every put clipped to the tile; a CIGAR or a B array that starts before
// the tile is measured again from its start and left once it has passed the
// tile's end.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hbam_fmt.h"
#include "hbam_launch.h"

namespace hbam {

namespace {

constexpr uint32_t kSamThreads = 256;
constexpr uint32_t kSamWaves = kSamThreads / 64;
constexpr uint32_t kSamTile = 16384;
constexpr uint64_t kSamLong = 4096;
// A record of at most kSamStage bytes (36 + rest) is copied into LDS by its
// wave in one round of 16-byte loads before any field is read: the fields and
// the aux chain are a dozen dependent reads, each a trip to HBM otherwise.
constexpr uint32_t kSamStage = 1024;
constexpr uint32_t kSamStageQuads = (kSamStage + 15 + 15) / 16 + 1;

// the tile a write pass fills: LDS bytes for text offsets [t0, t0 + len)
struct SamSink {
  uint8_t* tile;
  uint64_t t0;
  uint32_t len;
  __device__ __forceinline__ void put(uint64_t o, uint32_t c) const {
    const uint64_t d = o - t0;
    if (d < len) tile[d] = (uint8_t)c;
  }
  __device__ __forceinline__ uint64_t end() const { return t0 + len; }
};

// one record as its wave sees it (the same in every lane)
struct SamRec {
  const uint8_t* r;  // the encoding: block_size, the 32 fixed bytes, the rest
  uint32_t rest_len, lrn, ncig, flag, mapq;
  int32_t lseq, ref, pos, nref, npos, tlen;
};

struct SamRefs {
  const uint32_t* off;  // n + 1 starts into bytes
  const uint8_t* bytes;
  int32_t n;
};

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { return ld_u16(p) | (ld_u16(p + 2) << 16); }

// A value that is the same in every lane, told to the compiler: what is computed
// from it (digit counts, the branches of the aux walk, addresses) then runs on the
// scalar unit instead of 64 idle-but-for-one vector lanes.
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int32_t uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) {
  return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(x, d, 64);
    if (lane >= d) x += t;
  }
  return x;
}

__device__ __forceinline__ uint32_t char_of(uint64_t lo, uint64_t hi, uint32_t k) {  // byte k of 16 packed ones
  return (uint32_t)((k < 8 ? lo : hi) >> (8 * (k & 7))) & 0xffu;
}

// the decimal of v at o, one digit per lane; returns its length
template <bool W>
__device__ __forceinline__ uint32_t put_u32(const SamSink& s, uint64_t o, uint32_t v, uint32_t lane) {
  const uint32_t nd = fmt::ndigits_u32(v);
  if (W) {  // v is uniform: the digits come off its end one by one, lane nd - 1 - d keeps digit d
    uint32_t c = 0, x = v;
    for (uint32_t d = 0; d < nd; ++d) {
      const uint32_t r = x % 10u;
      x /= 10u;
      if (lane == nd - 1 - d) c = r;
    }
    if (lane < nd) s.put(o + lane, '0' + c);
  }
  return nd;
}

template <bool W>
__device__ __forceinline__ uint32_t put_i32(const SamSink& s, uint64_t o, int32_t v, uint32_t lane) {
  if (v >= 0) return put_u32<W>(s, o, (uint32_t)v, lane);
  if (W && lane == 0) s.put(o, '-');
  return 1 + put_u32<W>(s, o + 1, fmt::abs_i32(v), lane);
}

template <bool W>
__device__ __forceinline__ void put_1(const SamSink& s, uint64_t o, uint32_t c, uint32_t lane) {
  if (W && lane == 0) s.put(o, c);
}

// len source bytes (+ add) at o, dealt to the lanes; only the part inside the tile is visited
__device__ __forceinline__ void copy_clipped(const SamSink& s, uint64_t o, const uint8_t* src, uint64_t len,
                                             uint32_t add, uint32_t lane, uint32_t part = 0, uint32_t nparts = 1) {
  const uint64_t lo = o < s.t0 ? s.t0 - o : 0;
  const uint64_t hi = s.end() > o ? min(len, s.end() - o) : 0;
  for (uint64_t k = lo + 64ull * part + lane; k < hi; k += 64ull * nparts) s.put(o + k, (src[k] + add) & 0xffu);
}

template <bool W>
__device__ __forceinline__ uint32_t put_ref(const SamSink& s, uint64_t o, int32_t id, const SamRefs& refs,
                                            uint32_t lane) {
  if (id < 0 || id >= refs.n) {  // -1; any other value cannot leave hbam_decode_span
    put_1<W>(s, o, '*', lane);
    return 1;
  }
  const uint32_t a = uni(refs.off[id]), len = uni(refs.off[id + 1]) - a;
  if (W) copy_clipped(s, o, refs.bytes + a, len, 0, lane);
  return len;
}

// QNAME .. TLEN and the tab behind it, from o on; returns the offset behind it
// (a write pass may return early, past the tile's end: its caller knows the head's length)
template <bool W>
__device__ uint64_t sam_head(const SamSink& s, uint64_t o, const SamRec& R, const SamRefs& refs, uint32_t lane) {
  if (R.lrn <= 1) {
    put_1<W>(s, o, '*', lane);
    o += 1;
  } else {
    if (W) copy_clipped(s, o, R.r + 36, R.lrn - 1, 0, lane);
    o += R.lrn - 1;
  }
  put_1<W>(s, o++, '\t', lane);
  o += put_u32<W>(s, o, R.flag, lane);
  put_1<W>(s, o++, '\t', lane);
  o += put_ref<W>(s, o, R.ref, refs, lane);
  put_1<W>(s, o++, '\t', lane);
  o += put_i32<W>(s, o, (int32_t)((uint32_t)R.pos + 1u), lane);
  put_1<W>(s, o++, '\t', lane);
  o += put_u32<W>(s, o, R.mapq, lane);
  put_1<W>(s, o++, '\t', lane);
  if (R.ncig == 0) {
    put_1<W>(s, o++, '*', lane);
  } else {
    const uint8_t* cg = R.r + 36 + R.lrn;
    for (uint32_t c0 = 0; c0 < R.ncig; c0 += 64) {
      const uint32_t k = c0 + lane;
      const bool valid = k < R.ncig;
      const uint32_t v = valid ? ld_u32(cg + 4ull * k) : 0;
      const uint32_t nd = fmt::ndigits_u32(v >> 4);
      const uint32_t w = valid ? nd + 1 : 0;
      const uint32_t incl = wave_incl_sum(w, lane);
      if (W && valid) {
        const uint64_t at = o + (incl - w);
        fmt::fmt_u32(v >> 4, [&](uint32_t i, char ch) { s.put(at + i, (uint8_t)ch); });
        const uint32_t op = v & 15u;
        s.put(at + nd, op < 8 ? char_of(0x3d5048534e44494dull, 0, op) : op == 8 ? 'X' : '?');  // "MIDNSHP="
      }
      o += uni(__shfl(incl, 63, 64));
      if (W && o >= s.end()) return o;
    }
  }
  put_1<W>(s, o++, '\t', lane);
  if (R.nref < 0 || R.nref >= refs.n) {
    put_1<W>(s, o++, '*', lane);
  } else if (R.nref == R.ref) {
    put_1<W>(s, o++, '=', lane);
  } else {
    o += put_ref<W>(s, o, R.nref, refs, lane);
  }
  put_1<W>(s, o++, '\t', lane);
  o += put_i32<W>(s, o, (int32_t)((uint32_t)R.npos + 1u), lane);
  put_1<W>(s, o++, '\t', lane);
  o += put_i32<W>(s, o, R.tlen, lane);
  put_1<W>(s, o++, '\t', lane);
  return o;
}

__device__ __forceinline__ const uint8_t* sam_seq_ptr(const SamRec& R) { return R.r + 36 + R.lrn + 4ull * R.ncig; }
__device__ __forceinline__ const uint8_t* sam_qual_ptr(const SamRec& R) {
  return sam_seq_ptr(R) + (((uint64_t)R.lseq + 1) >> 1);
}
// QUAL prints as '*'
__device__ __forceinline__ bool sam_qual_star(const SamRec& R) {
  return R.lseq == 0 || uni((uint32_t)sam_qual_ptr(R)[0]) == 0xffu;
}

// SEQ, the tab, QUAL at o (write pass only): share `part` of `nparts` of the bases and qualities
__device__ void sam_seq_qual(const SamSink& s, uint64_t o, const SamRec& R, bool qstar, uint32_t part,
                             uint32_t nparts, uint32_t lane) {
  const uint64_t sl = (uint64_t)R.lseq;
  if (sl == 0) {
    if (part == 0 && lane < 3) s.put(o + lane, lane == 1 ? '\t' : '*');
    return;
  }
  const uint8_t* sq = sam_seq_ptr(R);
  {
    const uint64_t lo = o < s.t0 ? s.t0 - o : 0;
    const uint64_t hi = s.end() > o ? min(sl, s.end() - o) : 0;
    for (uint64_t k = lo + 64ull * part + lane; k < hi; k += 64ull * nparts) {
      const uint32_t b = sq[k >> 1];
      // "=ACMGRSV" "TWYHKDBN"
      s.put(o + k, char_of(0x565352474d43413dull, 0x4e42444b48595754ull, (k & 1) ? (b & 15u) : (b >> 4)));
    }
  }
  if (part == 0 && lane == 0) s.put(o + sl, '\t');
  if (qstar) {
    if (part == 0 && lane == 0) s.put(o + sl + 1, '*');
  } else {
    copy_clipped(s, o + sl + 1, sam_qual_ptr(R), sl, 33, lane, part, nparts);
  }
}

__device__ __forceinline__ uint32_t aux_int_size(uint32_t t) {
  return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0;
}

// an element of `type` at p as the value put_i32 / put_u32 takes (*neg: print it signed)
__device__ __forceinline__ uint32_t aux_int(const uint8_t* p, uint32_t type, bool* is_signed) {
  *is_signed = type == 'c' || type == 's' || type == 'i';
  switch (type) {
    case 'c': return (uint32_t)(int32_t)(int8_t)p[0];
    case 'C': return p[0];
    case 's': return (uint32_t)(int32_t)(int16_t)ld_u16(p);
    case 'S': return ld_u16(p);
    default: return ld_u32(p);
  }
}

// The aux fields [a, end) from o on, each with its tab in front; o moves behind
// them.  false: malformed (a step would leave the record).  A write pass may
// return early, past the tile's end.
template <bool W>
__device__ bool sam_aux(const SamSink& s, uint64_t& o, const uint8_t* a, const uint8_t* end, uint32_t lane) {
  while (a < end) {
    if (end - a < 3) return false;  // a tag header cut by the end
    const uint32_t type = uni((uint32_t)a[2]);
    const bool is_int = type == 'c' || type == 'C' || type == 's' || type == 'S' || type == 'i' || type == 'I';
    if (W && lane < 6)
      s.put(o + lane, lane == 0 ? '\t' : lane == 1 ? a[0] : lane == 2 ? a[1] : lane == 4 ? (is_int ? 'i' : type) : ':');
    o += 6;
    a += 3;
    if (is_int || type == 'f' || type == 'A') {
      const uint32_t sz = type == 'A' ? 1 : aux_int_size(type);
      if ((uint64_t)(end - a) < sz) return false;
      if (type == 'A') {
        put_1<W>(s, o++, a[0], lane);
      } else if (type == 'f') {
        uint64_t lo = 0, hi = 0;
        const uint32_t len = fmt::fmt_g(uni(ld_u32(a)), [&](uint32_t i, char ch) {
          if (i < 8) lo |= (uint64_t)(uint8_t)ch << (8 * i); else hi |= (uint64_t)(uint8_t)ch << (8 * (i - 8));
        });
        if (W && lane < len) s.put(o + lane, char_of(lo, hi, lane));
        o += len;
      } else {
        bool sg;
        const uint32_t v = uni(aux_int(a, type, &sg));
        o += sg ? put_i32<W>(s, o, (int32_t)v, lane) : put_u32<W>(s, o, v, lane);
      }
      a += sz;
    } else if (type == 'Z' || type == 'H') {
      uint64_t len = 0;
      for (;;) {  // the NUL, 64 bytes a step, never past the end
        const uint64_t rem = (uint64_t)(end - a) - len;
        if (rem == 0) return false;
        const bool in = lane < rem;
        const uint32_t c = in ? a[len + lane] : 1u;
        const uint64_t m = __ballot(in && c == 0);
        if (m) {  // (a ballot is uniform already)
          len += (uint64_t)__builtin_ctzll(m);
          break;
        }
        if (rem <= 64) return false;
        len += 64;
      }
      if (W) copy_clipped(s, o, a, len, 0, lane);
      o += len;
      a += len + 1;
    } else if (type == 'B') {
      if (end - a < 5) return false;
      const uint32_t sub = uni((uint32_t)a[0]), cnt = uni(ld_u32(a + 1));
      const uint32_t sz = aux_int_size(sub);
      if (sz == 0) return false;
      if ((uint64_t)(end - a - 5) / sz < cnt) return false;
      put_1<W>(s, o++, sub, lane);
      a += 5;
      for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
        const uint32_t k = c0 + lane < cnt ? c0 + lane : cnt - 1;  // (idle lanes re-read the last element)
        const bool valid = c0 + lane < cnt;
        const uint8_t* p = a + (uint64_t)k * sz;
        uint32_t len;
        uint64_t lo = 0, hi = 0;
        bool sg = false;
        uint32_t v = 0;
        if (sub == 'f') {
          len = fmt::fmt_g(ld_u32(p), [&](uint32_t i, char ch) {
            if (i < 8) lo |= (uint64_t)(uint8_t)ch << (8 * i); else hi |= (uint64_t)(uint8_t)ch << (8 * (i - 8));
          });
        } else {
          v = aux_int(p, sub, &sg);
          len = sg ? fmt::len_i32((int32_t)v) : fmt::ndigits_u32(v);
        }
        const uint32_t w = valid ? len + 1 : 0;
        const uint32_t incl = wave_incl_sum(w, lane);
        if (W && valid) {
          const uint64_t at = o + (incl - w);
          s.put(at, ',');
          if (sub == 'f') {
            for (uint32_t i = 0; i < len; ++i) s.put(at + 1 + i, char_of(lo, hi, i));
          } else if (sg) {
            fmt::fmt_i32((int32_t)v, [&](uint32_t i, char ch) { s.put(at + 1 + i, (uint8_t)ch); });
          } else {
            fmt::fmt_u32(v, [&](uint32_t i, char ch) { s.put(at + 1 + i, (uint8_t)ch); });
          }
        }
        o += uni(__shfl(incl, 63, 64));
        if (W && o >= s.end()) return true;
      }
      a += (uint64_t)cnt * sz;
    } else {
      return false;  // an unknown type ('d' among them)
    }
    if (W && o >= s.end()) return true;
  }
  return true;
}

struct SamCols {
  const uint64_t* rec_pos;
  const int32_t *ref_id, *pos, *l_seq, *next_ref_id, *next_pos, *tlen;
  const uint8_t *l_read_name, *mapq;
  const uint16_t *n_cigar, *flag;
  const uint32_t* rest_len;
};

__device__ __forceinline__ SamRec sam_load(const uint8_t* u, const SamCols& c, uint64_t i) {
  SamRec R;
  R.r = u + uni(c.rec_pos[i]);
  R.rest_len = uni(c.rest_len[i]);
  R.lrn = uni((uint32_t)c.l_read_name[i]);
  R.ncig = uni((uint32_t)c.n_cigar[i]);
  R.flag = uni((uint32_t)c.flag[i]);
  R.mapq = uni((uint32_t)c.mapq[i]);
  R.lseq = uni(c.l_seq[i]);
  R.ref = uni(c.ref_id[i]);
  R.pos = uni(c.pos[i]);
  R.nref = uni(c.next_ref_id[i]);
  R.npos = uni(c.next_pos[i]);
  R.tlen = uni(c.tlen[i]);
  return R;
}

// The record's bytes in the wave's LDS stage, if they fit: R.r then points there.
// Aligned 16-byte loads: up to 15 bytes before the record (still inside the
// source, whose start is 16 B-aligned) and after it (the source is readable 16
// bytes past its last record, as k_sort_gather needs it).
__device__ __forceinline__ void sam_stage(SamRec& R, uint4* stage, uint32_t lane) {
  const uint64_t bytes = 36ull + R.rest_len;
  if (bytes > kSamStage) return;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(R.r) & 15u);
  const uint4* q = reinterpret_cast<const uint4*>(R.r - sh);
  const uint32_t nq = (sh + (uint32_t)bytes + 15u) >> 4;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the lanes' reads of the record before)
  __builtin_amdgcn_wave_barrier();
  for (uint32_t k = lane; k < nq; k += 64) stage[k] = q[k];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  R.r = reinterpret_cast<const uint8_t*>(stage) + sh;
}

// the name, the CIGAR, the bases and the qualities fit the rest (bytes they take; ~0: they do not)
__device__ __forceinline__ uint64_t sam_fixed_bytes(const SamRec& R) {
  if (R.lseq < 0) return ~0ull;
  const uint64_t need = (uint64_t)R.lrn + 4ull * R.ncig + (((uint64_t)R.lseq + 1) >> 1) + (uint64_t)R.lseq;
  return need <= R.rest_len ? need : ~0ull;
}

__global__ __launch_bounds__(kSamThreads) void k_sam_measure(const uint8_t* __restrict__ u, SamCols c, uint64_t n,
                                                             SamRefs refs, uint32_t* __restrict__ head_len,
                                                             uint64_t* __restrict__ llen,
                                                             unsigned long long* __restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  __shared__ uint4 stage[kSamWaves][kSamStageQuads];
  if (blockIdx.x == 0 && threadIdx.x == 0) llen[n] = 0;
  const SamSink none{nullptr, 0, 0};
  for (uint64_t i = (uint64_t)blockIdx.x * kSamWaves + wave; i < n; i += (uint64_t)gridDim.x * kSamWaves) {
    SamRec R = sam_load(u, c, i);
    sam_stage(R, stage[wave], lane);
    const uint64_t fixed = sam_fixed_bytes(R);
    uint64_t o = 0;
    uint32_t hl = 0;
    bool ok = fixed != ~0ull;
    if (ok) {
      o = sam_head<false>(none, 0, R, refs, lane);
      hl = (uint32_t)o;
      o += (R.lseq ? (uint64_t)R.lseq : 1) + 1 + (sam_qual_star(R) ? 1 : (uint64_t)R.lseq);
      ok = sam_aux<false>(none, o, R.r + 36 + fixed, R.r + 36 + R.rest_len, lane);
      o += 1;  // '\n'
    }
    if (lane == 0) {
      head_len[i] = hl;
      llen[i] = ok ? o : 0;
      if (!ok) atomicMin(bad, (unsigned long long)i);
    }
  }
}

__global__ __launch_bounds__(kSamThreads) void k_sam_write(const uint8_t* __restrict__ u, SamCols c, uint32_t n,
                                                           SamRefs refs, const uint32_t* __restrict__ head_len,
                                                           const uint64_t* __restrict__ doff, uint64_t total,
                                                           uint8_t* __restrict__ dst) {
  __shared__ uint4 tile4[kSamTile / 16];
  __shared__ uint4 stage[kSamWaves][kSamStageQuads];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t t0 = (uint64_t)blockIdx.x * kSamTile;
  if (t0 >= total) return;
  const uint64_t t1 = min(t0 + kSamTile, total);
  const SamSink s{reinterpret_cast<uint8_t*>(tile4), t0, (uint32_t)(t1 - t0)};
  // the tile's first line: the last j with doff[j] <= t0 (doff[0] = 0, doff[n] = total > t0; no line is empty)
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (doff[mid] <= t0) lo = mid; else hi = mid;
  }
  const uint32_t j0 = lo;
  for (uint32_t j = j0; j < n; ++j) {
    const uint64_t l0 = uni(doff[j]);
    if (l0 >= t1) break;
    const uint64_t l1 = uni(doff[j + 1]);
    const bool big = l1 - l0 >= kSamLong;
    if (!big && ((j - j0) & (kSamWaves - 1)) != wave) continue;
    SamRec R = sam_load(u, c, j);
    sam_stage(R, stage[wave], lane);
    const uint64_t o_seq = l0 + uni(head_len[j]);
    const bool qstar = sam_qual_star(R);
    const uint64_t sl = R.lseq ? (uint64_t)R.lseq : 1;
    uint64_t o_aux = o_seq + sl + 1 + (qstar ? 1 : sl);
    if (o_seq > t0 && (!big || wave == 0)) sam_head<true>(s, l0, R, refs, lane);
    if (o_aux > t0 && o_seq < t1) sam_seq_qual(s, o_seq, R, qstar, big ? wave : 0, big ? kSamWaves : 1, lane);
    if (o_aux < t1 && (!big || wave == 1)) {
      sam_aux<true>(s, o_aux, R.r + 36 + sam_fixed_bytes(R), R.r + 36 + R.rest_len, lane);
      if (lane == 0) s.put(l1 - 1, '\n');
    }
  }
  __syncthreads();
  const uint32_t len = s.len;
  for (uint32_t b = 16u * threadIdx.x; b < len; b += 16u * kSamThreads) {
    if (b + 16 <= len) {
      *reinterpret_cast<uint4*>(dst + t0 + b) = tile4[b >> 4];
    } else {
      for (uint32_t k = b; k < len; ++k) dst[t0 + k] = s.tile[k];
    }
  }
}

SamCols cols_of(const uint64_t* rec_pos, const Columns& col) {
  return SamCols{rec_pos,      col.ref_id,      col.pos,  col.l_seq,   col.next_ref_id, col.next_pos,
                 col.tlen,     col.l_read_name, col.mapq, col.n_cigar, col.flag,        col.rest_len};
}

}  // namespace

hipError_t sam_tmp_bytes(uint64_t n, size_t* bytes) {
  const uint64_t* in = nullptr;
  uint64_t* out = nullptr;
  *bytes = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, in, out, (int)(n + 1), (hipStream_t)0);
}

hipError_t launch_sam_measure(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, uint64_t n,
                              const uint32_t* ref_off, const uint8_t* ref_bytes, int32_t n_ref, uint32_t* head_len,
                              uint64_t* llen, unsigned long long* bad, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = std::min<uint64_t>((n + kSamWaves - 1) / kSamWaves, 1u << 16);
  hipLaunchKernelGGL(k_sam_measure, dim3((unsigned)blocks), dim3(kSamThreads), 0, s, u, cols_of(rec_pos, col), n,
                     SamRefs{ref_off, ref_bytes, n_ref}, head_len, llen, bad);
  return hipGetLastError();
}

hipError_t launch_sam_offsets(void* tmp, size_t tmp_bytes, const uint64_t* llen, uint64_t n, uint64_t* doff,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, llen, doff, (int)(n + 1), s);
}

hipError_t launch_sam_write(const uint8_t* u, const uint64_t* rec_pos, const Columns& col, uint64_t n,
                            const uint32_t* ref_off, const uint8_t* ref_bytes, int32_t n_ref,
                            const uint32_t* head_len, const uint64_t* doff, uint64_t total, uint8_t* dst,
                            hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint64_t tiles = (total + kSamTile - 1) / kSamTile;
  hipLaunchKernelGGL(k_sam_write, dim3((unsigned)tiles), dim3(kSamThreads), 0, s, u, cols_of(rec_pos, col),
                     (uint32_t)n, SamRefs{ref_off, ref_bytes, n_ref}, head_len, doff, total, dst);
  return hipGetLastError();
}

}  // namespace hbam
