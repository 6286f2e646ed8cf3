// hbam_samparse.hip -- gfx950 kernels that parse SAM text into BAM records
// (hbam_parse_sam: one record per line, the rules in include/hbam.h).
//
//   k_samp_count   a workgroup per 4 KiB of the text, 16 aligned bytes per lane:
//        the '\n's of its piece
//   (hipcub)       the exclusive sum of those counts: the line index each piece
//        starts at, the last = the number of lines
//   k_samp_starts  the same loads again: start[k + 1] = the byte behind the
//        k-th '\n' (start[0] = 0), placed by a block prefix sum
//   k_samp_measure one wave per line: every field and aux tag validated, the
//        record's size, the first bad line and its field (atomicMin)
//   (hipcub)       roff = the exclusive sum of the sizes over n + 1 entries: the
//        record starts, roff[n] = the encodings' bytes
//   k_samp_write   the records
//
// Both passes run the same function (samp_line) over a line, the measuring one
// with the stores compiled out, so a record is exactly as long as measured.
// The lanes of a wave share a line's bytes: tabs are found by ballots over
// 16-byte loads per lane (find_byte: 1 KiB a step), name, bases (two per lane
// into one byte) and qualities are dealt by output byte, CIGAR operators and
// the commas of a B array are found 64 bytes at a time by ballot, each
// operator's or element's index is the count of those before it (a popcount
// of the ballot below the lane plus the running total) and its lane reads its
// number; a scalar number has one digit per lane.  What is the same in every
// lane is marked so (uni).  A line of at most kSpStage bytes is first copied
// into its wave's LDS stage and read from there.  Every step is bounded by the
// line's end; no byte outside [text, text + len) rounded up to 16 is read, and
// the upload zeroes that padding.
//
// A line shorter than kSpLong belongs to one wave (the lines of a group of four
// go to the four waves of a workgroup); a longer one is worked on by all four:
// each runs samp_line with its part number, walks the field structure itself
// (that costs no byte-sized step) and takes every fourth 64-byte step of the
// bases, the qualities, a Z or H string and a B array's elements.  The waves
// need no barrier: sizes follow from the structure alone, a wave flags what is
// wrong in its share with the same atomicMin, and their stores are disjoint.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hbam_align_end.h"  // consumes_ref
#include "hbam_dev_util.h"
#include "hbam_fmt.h"
#include "hbam_launch.h"

namespace hbam {

namespace {

constexpr uint32_t kSpThreads = 256;
constexpr uint32_t kSpWaves = kSpThreads / 64;
constexpr uint32_t kSpPiece = 16 * kSpThreads;  // text bytes per workgroup of the line passes
constexpr uint64_t kSpLong = 4096;
constexpr uint64_t kSpHuge = 1ull << 40;        // what a number too large for any field saturates to
// A line of at most kSpStage bytes is copied into its wave's LDS stage in one
// round of 16-byte loads before any field is read: the tab searches, the
// digits and the aux walk are some sixty dependent reads, each a trip to L2 or
// HBM otherwise (measured: DESIGN.md 4.11).
constexpr uint32_t kSpStage = 2048;
constexpr uint32_t kSpStageQuads = (kSpStage + 15 + 15) / 16 + 1;

// one line as its wave sees it (the same in every lane)
struct SpLine {
  const uint8_t* T;         // the text, or the stage that holds the line (16 B-aligned)
  unsigned long long* bad;  // line << 8 | field of the first violation (measure pass)
  uint64_t line;
  uint8_t* rec;             // where the record goes (write pass)
  uint32_t lane, part, nparts;
};

struct SpDict {
  const uint32_t* off;  // n + 1 starts into bytes, the names sorted as unsigned bytes
  const uint8_t* bytes;
  const int32_t* idx;   // the sorted name's (lowest) index in the dictionary
  int32_t n;
};

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) {
  return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | uni((uint32_t)x);
}
__device__ __forceinline__ uint32_t ldc(const uint8_t* T, uint64_t p) { return uni((uint32_t)T[p]); }  // p uniform

__device__ __forceinline__ void sp_bad(const SpLine& c, uint32_t field) {
  if (c.bad && c.lane == 0) atomicMin(c.bad, (unsigned long long)(c.line << 8 | field));
}

// bit k set: byte k of the 4 in w equals the byte rep is made of
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t rep) {
  const uint32_t x = w ^ rep;
  const uint32_t y = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 where a byte of x is 0
  return (((y >> 7) * 0x00204081u) >> 21) & 0xfu;
}
__device__ __forceinline__ uint32_t eq16(const uint4 q, uint32_t ch) {
  const uint32_t rep = ch * 0x01010101u;
  return eq4(q.x, rep) | (eq4(q.y, rep) << 4) | (eq4(q.z, rep) << 8) | (eq4(q.w, rep) << 12);
}

// the first byte equal to ch in [pos, end), or end: 16 aligned bytes per lane, 1 KiB a step
__device__ __forceinline__ uint64_t find_byte(const uint8_t* T, uint64_t pos, uint64_t end, uint32_t ch,
                                              uint32_t lane) {
  for (uint64_t base = pos & ~15ull; base < end; base += 1024) {
    const uint64_t p = base + 16ull * lane;
    uint32_t m = 0;
    if (p < end) {
      m = eq16(*reinterpret_cast<const uint4*>(T + p), ch);
      if (p < pos) m &= ~0u << (uint32_t)(pos - p);
      if (end - p < 16) m &= (1u << (uint32_t)(end - p)) - 1u;
    }
    const uint64_t any = __ballot(m != 0);
    if (any) {
      const uint32_t src = (uint32_t)__builtin_ctzll(any);
      return base + 16ull * src + (uint32_t)__builtin_ctz(uni((uint32_t)__shfl((int)m, (int)src, 64)));
    }
  }
  return end;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

__device__ __forceinline__ void st_u32(uint8_t* p, uint32_t v) {  // (records start at any byte)
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

// A decimal field [a, b): an optional '-', then one or more digits, leading
// zeros allowed.  Every byte is looked at, 64 a step; the value is summed from
// one digit per lane and saturates to kSpHuge past ten significant digits.
struct SpDec {
  bool ok, neg;
  uint64_t mag;
};
__device__ SpDec sp_dec(const uint8_t* T, uint64_t a, uint64_t b, uint32_t lane) {
  SpDec r{false, false, 0};
  if (a < b && ldc(T, a) == '-') {
    r.neg = true;
    ++a;
  }
  if (a >= b) return r;
  uint64_t z = b;  // the first nonzero digit
  for (uint64_t p = a; p < b; p += 64) {
    const bool in = p + lane < b;
    const uint32_t dg = (in ? (uint32_t)T[p + lane] : (uint32_t)'0') - '0';
    if (__ballot(dg > 9u)) return r;
    const uint64_t nz = __ballot(dg != 0);
    if (nz && z == b) z = p + (uint32_t)__builtin_ctzll(nz);
  }
  r.ok = true;
  const uint64_t sd = b - z;
  if (sd > 10) {
    r.mag = kSpHuge;
    return r;
  }
  uint64_t v = 0;
  if (lane < sd) v = (uint64_t)((uint32_t)T[z + lane] - '0') * fmt::pow10_u32((uint32_t)sd - 1u - lane);
  r.mag = uni(wave_sum_u64(v));
  return r;
}

// the field as a signed value in [lo, hi]
__device__ __forceinline__ bool sp_int(const uint8_t* T, uint64_t a, uint64_t b, int64_t lo, int64_t hi,
                                       uint32_t lane, int64_t* v) {
  const SpDec d = sp_dec(T, a, b, lane);
  *v = d.neg ? -(int64_t)d.mag : (int64_t)d.mag;
  return d.ok && *v >= lo && *v <= hi;
}

// The dictionary index of the name [a, b), -1: not a name.  A binary search,
// each comparison by the wave; *hint = the sorted position the wave found last
// (-1: none) is tried first: neighbouring lines mostly name the same reference.
__device__ int32_t sp_dict_find(const SpDict& d, const uint8_t* T, uint64_t a, uint64_t b, uint32_t lane,
                                int32_t* hint) {
  const uint64_t klen = b - a;
  int32_t lo = 0, hi = d.n;
  bool hinted = *hint >= 0;
  while (lo < hi) {
    const int32_t mid = hinted ? *hint : lo + ((hi - lo) >> 1);
    const uint32_t n0 = uni(d.off[mid]), nlen = uni(d.off[mid + 1]) - n0;
    const uint64_t m = klen < nlen ? klen : nlen;
    int cmp = 0;
    for (uint64_t p = 0; p < m && cmp == 0; p += 64) {
      const bool in = p + lane < m;
      const uint32_t kc = in ? T[a + p + lane] : 0u, nc = in ? d.bytes[n0 + p + lane] : 0u;
      const uint64_t ne = __ballot(kc != nc);
      if (ne) {
        const int src = __builtin_ctzll(ne);
        cmp = (int)uni((uint32_t)__shfl((int)kc, src, 64)) - (int)uni((uint32_t)__shfl((int)nc, src, 64));
      }
    }
    if (cmp == 0) cmp = klen < nlen ? -1 : klen > nlen ? 1 : 0;
    if (cmp == 0) {
      *hint = mid;
      return (int32_t)uni((uint32_t)d.idx[mid]);
    }
    if (cmp < 0) hi = mid; else lo = mid + 1;  // (a hint that misses halves the range like any other probe)
    hinted = false;
  }
  return -1;
}

// RNAME / RNEXT [a, b): false = unknown name.  same: what '=' means (-2: '=' is not allowed here)
__device__ __forceinline__ bool sp_ref(const SpDict& d, const uint8_t* T, uint64_t a, uint64_t b, int32_t same,
                                       uint32_t lane, int32_t* hint, int32_t* id) {
  if (b - a == 1) {
    const uint32_t ch = ldc(T, a);
    if (ch == '*' || (ch == '=' && same != -2)) {
      *id = ch == '*' ? -1 : same;
      return true;
    }
  }
  *id = sp_dict_find(d, T, a, b, lane, hint);
  return *id >= 0;
}

__device__ __forceinline__ uint32_t cigar_op_of(uint32_t ch) {  // "MIDNSHP=X" -> 0..8, else 15
  switch (ch) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return 15;
  }
}

// The CIGAR [a, b), not "*": number-then-operator pairs.  The operators of 64
// bytes are found by ballot; an operator's lane reads its number backwards to
// the operator before it (or the field's start).  *ncig, *ref_len = the sum of
// the lengths that consume the reference.
template <bool W>
__device__ bool sp_cigar(const SpLine& c, uint64_t a, uint64_t b, uint8_t* dst, uint32_t* ncig, uint64_t* ref_len) {
  const uint8_t* T = c.T;
  const uint32_t lane = c.lane;
  uint64_t n = 0, rl = 0;
  bool err = false;
  for (uint64_t p = a; p < b; p += 64) {
    const bool in = p + lane < b;
    const uint32_t ch = in ? (uint32_t)T[p + lane] : (uint32_t)'0';
    const bool isop = ch - '0' > 9u;
    const uint64_t mask = __ballot(isop);
    if (isop) {
      const uint32_t op = cigar_op_of(ch);
      uint32_t v = 0, nd = 0, mul = 1;
      bool over = false;
      for (uint64_t q = p + lane; q > a; --q) {  // the digits, the last one first
        const uint32_t dg = (uint32_t)T[q - 1] - '0';
        if (dg > 9u) break;
        if (nd < 9) {
          v += dg * mul;
          mul *= 10u;
        } else {
          over |= dg != 0;
        }
        ++nd;
      }
      err |= op > 8u || nd == 0 || over || v >= (1u << 28);
      if (W && c.part == 0) st_u32(dst + 4ull * (n + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull))), (v << 4) | op);
      if (op <= 8u && consumes_ref(op)) rl += v;
    }
    n += (uint64_t)__popcll(mask);
  }
  err |= ldc(T, b - 1) - '0' <= 9u;  // digits with no operator behind them
  *ncig = (uint32_t)(n < 0x10000 ? n : 0x10000);
  *ref_len = uni(wave_sum_u64(rl));
  return !__ballot(err) && n <= 65535;
}

// nibble codes of the letters by (letter & 31): "=ACMGRSVTWYHKDBN", 16 = not a base
constexpr uint64_t seq_table(bool high) {
  const char* s = "=ACMGRSVTWYHKDBN";
  uint64_t t = 0;
  for (int k = 1; k < 16; ++k) {
    const int i = s[k] & 31;
    if ((i >= 16) == high) t |= (uint64_t)k << (4 * (i & 15));
  }
  return t;
}
constexpr uint32_t seq_valid() {
  const char* s = "=ACMGRSVTWYHKDBN";
  uint32_t m = 0;
  for (int k = 1; k < 16; ++k) m |= 1u << (s[k] & 31);
  return m;
}
__device__ __forceinline__ uint32_t nibble_of(uint32_t ch) {
  if (ch == '=') return 0;
  if (ch == '.') return 15;
  const uint32_t i = ch & 31u;
  if ((ch & 0xc0u) != 0x40u || !((seq_valid() >> i) & 1u)) return 16;
  return (uint32_t)((i < 16 ? seq_table(false) : seq_table(true)) >> (4 * (i & 15))) & 15u;
}

// SEQ [a, a + lseq), not "*": by output byte, this wave's share
template <bool W>
__device__ bool sp_seq(const SpLine& c, uint64_t a, uint64_t lseq, uint8_t* dst) {
  const uint64_t nb = (lseq + 1) >> 1;
  bool err = false;
  for (uint64_t k = 64ull * c.part + c.lane; k < nb; k += 64ull * c.nparts) {
    const uint32_t hi = nibble_of(c.T[a + 2 * k]);
    const uint32_t lo = 2 * k + 1 < lseq ? nibble_of(c.T[a + 2 * k + 1]) : 0u;
    err |= (hi | lo) > 15u;
    if (W) dst[k] = (uint8_t)((hi << 4) | lo);
  }
  return !__ballot(err);
}

// QUAL: lseq bytes at a (star: 0xFF each)
template <bool W>
__device__ bool sp_qual(const SpLine& c, uint64_t a, uint64_t lseq, bool star, uint8_t* dst) {
  bool err = false;
  for (uint64_t k = 64ull * c.part + c.lane; k < lseq; k += 64ull * c.nparts) {
    const uint32_t q = star ? 0xffu + 33u : (uint32_t)c.T[a + k];
    err |= !star && (q < 33u || q > 126u);
    if (W) dst[k] = (uint8_t)(q - 33u);
  }
  return !__ballot(err);
}

__device__ __forceinline__ uint32_t aux_size(uint32_t t) {
  return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : 0;
}
__device__ __forceinline__ bool aux_in_range(uint32_t t, int64_t v) {
  switch (t) {
    case 'c': return v >= -128 && v <= 127;
    case 'C': return v >= 0 && v <= 255;
    case 's': return v >= -32768 && v <= 32767;
    case 'S': return v >= 0 && v <= 65535;
    case 'i': return v >= -2147483648ll && v <= 2147483647ll;
    default: return v >= 0 && v <= 4294967295ll;
  }
}

// one lane's integer element [q, the next ',' or end)
__device__ __forceinline__ bool lane_int(const uint8_t* T, uint64_t q, uint64_t end, int64_t* v) {
  bool neg = false;
  if (q < end && T[q] == '-') {
    neg = true;
    ++q;
  }
  uint64_t mag = 0;
  uint32_t nd = 0;
  for (; q < end; ++q, ++nd) {
    const uint32_t ch = T[q];
    if (ch == ',') break;
    if (ch - '0' > 9u) return false;
    if (mag < kSpHuge) mag = mag * 10u + (ch - '0');
  }
  *v = neg ? -(int64_t)mag : (int64_t)mag;
  return nd != 0;
}

// One aux field [a, b) ("TG:t:value") into dst; *size = its bytes in the record.
template <bool W>
__device__ bool sp_aux(const SpLine& c, uint64_t a, uint64_t b, uint8_t* dst, uint64_t* size) {
  const uint8_t* T = c.T;
  const uint32_t lane = c.lane;
  const uint64_t len = b - a;
  if (len < 5) return false;
  const uint32_t h = lane < 6 && lane < len ? (uint32_t)T[a + lane] : 0u;
  const uint32_t t0 = uni((uint32_t)__shfl((int)h, 0, 64)), t1 = uni((uint32_t)__shfl((int)h, 1, 64));
  const uint32_t type = uni((uint32_t)__shfl((int)h, 3, 64)), sub = uni((uint32_t)__shfl((int)h, 5, 64));
  if (uni((uint32_t)__shfl((int)h, 2, 64)) != ':' || uni((uint32_t)__shfl((int)h, 4, 64)) != ':') return false;
  const uint64_t va = a + 5, vlen = len - 5;
  const bool put = W && c.part == 0;
  uint32_t stored = type;  // the type byte in the record
  if (type == 'A') {
    if (vlen != 1) return false;
    if (put && lane == 0) dst[3] = (uint8_t)sub;
    *size = 4;
  } else if (type == 'i') {
    int64_t v;
    if (!sp_int(T, va, b, -2147483648ll, 4294967295ll, lane, &v)) return false;
    stored = v >= -128 && v <= 127 ? 'c' : v >= 0 && v <= 255 ? 'C' : v >= -32768 && v <= 32767 ? 's'
             : v >= 0 && v <= 65535 ? 'S' : v <= 2147483647ll ? 'i' : 'I';
    const uint32_t sz = aux_size(stored);
    if (put && lane < sz) dst[3 + lane] = (uint8_t)((uint64_t)v >> (8 * lane));
    *size = 3 + sz;
  } else if (type == 'f') {
    if (vlen >= (1ull << 31)) return false;
    uint32_t bits = 0;
    if (!fmt::parse_f32([&](uint32_t i) { return (char)ldc(T, va + i); }, (uint32_t)vlen, &bits)) return false;
    if (put && lane < 4) dst[3 + lane] = (uint8_t)(bits >> (8 * lane));
    *size = 7;
  } else if (type == 'Z' || type == 'H') {
    if (W)
      for (uint64_t k = 64ull * c.part + lane; k < vlen; k += 64ull * c.nparts) dst[3 + k] = T[va + k];
    if (put && lane == 0) dst[3 + vlen] = 0;
    *size = 3 + vlen + 1;
  } else if (type == 'B') {
    const uint32_t sz = vlen ? aux_size(sub) : 0;
    if (sz == 0) return false;
    const uint64_t ea = va + 1;  // ",v,v,v" or nothing
    if (ea < b && ldc(T, ea) != ',') return false;
    uint64_t cnt = 0, step = 0;
    bool err = false;
    for (uint64_t p = ea; p < b; p += 64, ++step) {
      const bool comma = p + lane < b && T[p + lane] == ',';
      const uint64_t mask = __ballot(comma);
      if (comma && step % c.nparts == c.part) {  // this wave's share: the element behind the comma
        const uint64_t q = p + lane + 1;
        uint8_t* at = dst + 8 + (uint64_t)sz * (cnt + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull)));
        if (sub == 'f') {
          uint64_t e = q;
          while (e < b && T[e] != ',') ++e;
          uint32_t bits = 0;
          err |= e - q >= (1ull << 31) ||
                 !fmt::parse_f32([&](uint32_t i) { return (char)T[q + i]; }, (uint32_t)(e - q), &bits);
          if (W) st_u32(at, bits);
        } else {
          int64_t v = 0;
          err |= !lane_int(T, q, b, &v) || !aux_in_range(sub, v);
          if (W)
            for (uint32_t k = 0; k < sz; ++k) at[k] = (uint8_t)((uint64_t)v >> (8 * k));
        }
      }
      cnt += (uint64_t)__popcll(mask);
    }
    if (__ballot(err) || cnt > 0xffffffffull) return false;
    if (put && lane < 5) dst[3 + lane] = lane == 0 ? (uint8_t)sub : (uint8_t)(cnt >> (8 * (lane - 1)));
    *size = 8 + sz * cnt;
  } else {
    return false;
  }
  if (put && lane < 3) dst[lane] = (uint8_t)(lane == 0 ? t0 : lane == 1 ? t1 : stored);
  return true;
}

__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {  // arithmetic shifts, as oracle/bai.py
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

enum : uint32_t {
  kSpEmpty, kSpCount, kSpQname, kSpFlag, kSpRname, kSpPos, kSpMapq, kSpCigar, kSpRnext, kSpPnext, kSpTlen, kSpSeq,
  kSpQual, kSpAux, kSpTooLong, kSpFields
};

// The line [l0, l1) of c.T (l1 = its '\n'; c.T is the text, or the wave's stage
// with l0 < 16: nothing below needs a position in the whole text, only c.T
// 16 B-aligned).  Returns the record's bytes, 0 when the line is malformed (the
// measure pass has then recorded it).
template <bool W>
__device__ uint64_t samp_line(const SpLine& c, uint64_t l0, uint64_t l1, const SpDict& d, int32_t* hint) {
  const uint8_t* T = c.T;
  const uint32_t lane = c.lane;
#define SP_FAIL(field)  \
  do {                  \
    sp_bad(c, (field)); \
    return 0;           \
  } while (0)
  // the next field [a, b); one of the first ten must end at a tab
#define SP_NEXT(field, last)                  \
  a = b + 1;                                  \
  b = find_byte(T, a, l1, '\t', lane);        \
  if (!(last) && b == l1) SP_FAIL(kSpCount);  \
  if (a == b) SP_FAIL(field)
  if (l1 > l0 && ldc(T, l1 - 1) == '\r') --l1;
  if (l1 == l0) SP_FAIL(kSpEmpty);
  if (l1 - l0 >= (1ull << 31)) SP_FAIL(kSpTooLong);
  int64_t v;
  uint64_t a = l0, b = find_byte(T, a, l1, '\t', lane);
  if (b == l1) SP_FAIL(kSpCount);
  // QNAME
  const uint64_t nlen = b - a;
  if (nlen < 1 || nlen > 254) SP_FAIL(kSpQname);
  if (W && c.part == 0) {
    for (uint32_t k = lane; k < nlen; k += 64) c.rec[36 + k] = T[a + k];
    if (lane == 0) c.rec[36 + nlen] = 0;
  }
  const uint32_t lrn = (uint32_t)nlen + 1;
  SP_NEXT(kSpFlag, false);
  if (!sp_int(T, a, b, 0, 65535, lane, &v)) SP_FAIL(kSpFlag);
  const uint32_t flag = (uint32_t)v;
  SP_NEXT(kSpRname, false);
  int32_t ref, nref;
  if (!sp_ref(d, T, a, b, -2, lane, hint, &ref)) SP_FAIL(kSpRname);
  SP_NEXT(kSpPos, false);
  if (!sp_int(T, a, b, -2147483648ll, 2147483647ll, lane, &v)) SP_FAIL(kSpPos);
  const int32_t pos = (int32_t)((uint32_t)v - 1u);
  SP_NEXT(kSpMapq, false);
  if (!sp_int(T, a, b, 0, 255, lane, &v)) SP_FAIL(kSpMapq);
  const uint32_t mapq = (uint32_t)v;
  SP_NEXT(kSpCigar, false);
  uint32_t ncig = 0;
  uint64_t ref_len = 0;
  if (!(b - a == 1 && ldc(T, a) == '*') && !sp_cigar<W>(c, a, b, c.rec + 36 + lrn, &ncig, &ref_len)) SP_FAIL(kSpCigar);
  SP_NEXT(kSpRnext, false);
  if (!sp_ref(d, T, a, b, ref, lane, hint, &nref)) SP_FAIL(kSpRnext);
  SP_NEXT(kSpPnext, false);
  if (!sp_int(T, a, b, -2147483648ll, 2147483647ll, lane, &v)) SP_FAIL(kSpPnext);
  const int32_t npos = (int32_t)((uint32_t)v - 1u);
  SP_NEXT(kSpTlen, false);
  if (!sp_int(T, a, b, -2147483648ll, 2147483647ll, lane, &v)) SP_FAIL(kSpTlen);
  const int32_t tlen = (int32_t)v;
  SP_NEXT(kSpSeq, false);
  const uint64_t sa = a;
  const uint64_t lseq = b - a == 1 && ldc(T, a) == '*' ? 0 : b - a;
  SP_NEXT(kSpQual, true);
  const bool qstar = b - a == 1 && ldc(T, a) == '*';
  if (!qstar && b - a != lseq) SP_FAIL(kSpQual);  // (lseq 0: QUAL must be "*")
  const uint64_t o_seq = 36ull + lrn + 4ull * ncig, o_qual = o_seq + ((lseq + 1) >> 1);
  if (lseq && !sp_seq<W>(c, sa, lseq, c.rec + o_seq)) sp_bad(c, kSpSeq);
  if (!sp_qual<W>(c, a, lseq, qstar, c.rec + o_qual)) sp_bad(c, kSpQual);
  uint64_t o = o_qual + lseq;
  while (b < l1) {
    a = b + 1;
    b = find_byte(T, a, l1, '\t', lane);
    uint64_t sz = 0;
    if (!sp_aux<W>(c, a, b, c.rec + o, &sz)) SP_FAIL(kSpAux);
    o += sz;
  }
  if (o - 4 > 0x7fffffffull) SP_FAIL(kSpTooLong);
  if (W && c.part == 0 && lane < 36) {
    uint32_t bin = 0;
    if (ref >= 0) bin = reg2bin(pos, (int64_t)pos + (((flag & 4u) || ref_len == 0) ? 1 : (int64_t)ref_len)) & 0xffffu;
    const uint32_t k = lane >> 2;
    const uint32_t w = k == 0 ? (uint32_t)(o - 4) : k == 1 ? (uint32_t)ref : k == 2 ? (uint32_t)pos
                       : k == 3 ? (lrn | (mapq << 8) | (bin << 16)) : k == 4 ? (ncig | (flag << 16))
                       : k == 5 ? (uint32_t)lseq : k == 6 ? (uint32_t)nref : k == 7 ? (uint32_t)npos : (uint32_t)tlen;
    c.rec[lane] = (uint8_t)(w >> (8 * (lane & 3)));
  }
#undef SP_NEXT
#undef SP_FAIL
  return o;
}

// the lines of the grid's groups of four: each wave its short line, all four every long one
template <bool W>
__device__ __forceinline__ void samp_lines(const uint8_t* T, const uint64_t* __restrict__ start, uint64_t n,
                                           const SpDict& d, uint64_t* rlen, const uint64_t* roff, uint8_t* dst,
                                           unsigned long long* bad) {
  __shared__ uint4 stage[kSpWaves][kSpStageQuads];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  int32_t hint = -1;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kSpWaves; i0 < n; i0 += (uint64_t)gridDim.x * kSpWaves) {
    for (uint32_t k = 0; k < kSpWaves && i0 + k < n; ++k) {
      const uint64_t i = i0 + k;
      const uint64_t l0 = uni(start[i]), l1 = uni(start[i + 1]) - 1;
      const bool big = l1 - l0 >= kSpLong;
      if (!big && k != wave) continue;
      const uint8_t* Tl = T;
      uint64_t base = 0;  // samp_line's positions count from T + base
      if (l1 - l0 <= kSpStage) {
        // the aligned 16-byte pieces that hold [l0, l1) into the stage: byte p's copy is stage byte p - base
        base = l0 & ~15ull;
        const uint32_t nq = (uint32_t)((l1 - base + 15) >> 4);
        const uint4* q = reinterpret_cast<const uint4*>(T + base);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the lanes' reads of the line before)
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j = lane; j < nq; j += 64) stage[wave][j] = q[j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        Tl = reinterpret_cast<const uint8_t*>(stage[wave]);
      }
      const SpLine c{Tl, bad, i, W ? dst + uni(roff[i]) : nullptr, lane, big ? wave : 0u, big ? kSpWaves : 1u};
      const uint64_t size = samp_line<W>(c, l0 - base, l1 - base, d, &hint);
      if (!W && lane == 0 && c.part == 0) rlen[i] = size;
    }
  }
}

__global__ __launch_bounds__(kSpThreads) void k_samp_measure(const uint8_t* __restrict__ T,
                                                             const uint64_t* __restrict__ start, uint64_t n, SpDict d,
                                                             uint64_t* __restrict__ rlen,
                                                             unsigned long long* __restrict__ bad) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rlen[n] = 0;
  samp_lines<false>(T, start, n, d, rlen, nullptr, nullptr, bad);
}

__global__ __launch_bounds__(kSpThreads) void k_samp_write(const uint8_t* __restrict__ T,
                                                           const uint64_t* __restrict__ start, uint64_t n, SpDict d,
                                                           const uint64_t* __restrict__ roff,
                                                           uint8_t* __restrict__ dst) {
  samp_lines<true>(T, start, n, d, nullptr, roff, dst, nullptr);
}

// ---- line finding
__device__ __forceinline__ uint32_t piece_newlines(const uint8_t* T, uint64_t len, uint64_t p) {  // bit k: T[p + k] is '\n'
  if (p >= len) return 0;
  uint32_t m = eq16(*reinterpret_cast<const uint4*>(T + p), '\n');
  if (len - p < 16) m &= (1u << (uint32_t)(len - p)) - 1u;
  return m;
}

__global__ __launch_bounds__(kSpThreads) void k_samp_count(const uint8_t* __restrict__ T, uint64_t len,
                                                           uint64_t npiece, uint64_t* __restrict__ cnt) {
  __shared__ uint32_t part[kSpWaves];
  const uint64_t p = (uint64_t)blockIdx.x * kSpPiece + 16ull * threadIdx.x;
  const uint32_t c = wave_sum_u32((uint32_t)__popc(piece_newlines(T, len, p)));
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = (uint64_t)part[0] + part[1] + part[2] + part[3];
    if (blockIdx.x == 0) cnt[npiece] = 0;
  }
}

__global__ __launch_bounds__(kSpThreads) void k_samp_starts(const uint8_t* __restrict__ T, uint64_t len,
                                                            const uint64_t* __restrict__ first,
                                                            uint64_t* __restrict__ start) {
  __shared__ uint32_t part[kSpWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t p = (uint64_t)blockIdx.x * kSpPiece + 16ull * threadIdx.x;
  uint32_t m = piece_newlines(T, len, p);
  const uint32_t c = (uint32_t)__popc(m);
  const uint32_t incl = wave_incl_scan_dpp(c);
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  uint64_t k = first[blockIdx.x] + (incl - c);
  for (uint32_t w = 0; w < wave; ++w) k += part[w];
  if (blockIdx.x == 0 && threadIdx.x == 0) start[0] = 0;
  for (; m; m &= m - 1) start[++k] = p + (uint32_t)__builtin_ctz(m) + 1;
}

}  // namespace

const char* samp_field_name(uint32_t field) {
  static const char* const names[kSpFields] = {"is empty",     "has fewer than 11 fields", "QNAME", "FLAG", "RNAME",
                                               "POS",          "MAPQ",                     "CIGAR", "RNEXT", "PNEXT",
                                               "TLEN",         "SEQ",                      "QUAL",  "aux field",
                                               "is too long"};
  return field < kSpFields ? names[field] : "?";
}

uint64_t samp_pieces(uint64_t len) { return (len + kSpPiece - 1) / kSpPiece; }

hipError_t samp_scan_bytes(uint64_t m, size_t* bytes) {
  const uint64_t* in = nullptr;
  uint64_t* out = nullptr;
  *bytes = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, in, out, (int)m, (hipStream_t)0);
}

hipError_t launch_samp_scan(void* tmp, size_t tmp_bytes, const uint64_t* in, uint64_t m, uint64_t* out,
                            hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, (int)m, s);
}

hipError_t launch_samp_count(const uint8_t* text, uint64_t len, uint64_t* cnt, hipStream_t s) {
  const uint64_t np = samp_pieces(len);
  if (np == 0) return hipSuccess;
  hipLaunchKernelGGL(k_samp_count, dim3((unsigned)np), dim3(kSpThreads), 0, s, text, len, np, cnt);
  return hipGetLastError();
}

hipError_t launch_samp_starts(const uint8_t* text, uint64_t len, const uint64_t* first, uint64_t* start,
                              hipStream_t s) {
  const uint64_t np = samp_pieces(len);
  if (np == 0) return hipSuccess;
  hipLaunchKernelGGL(k_samp_starts, dim3((unsigned)np), dim3(kSpThreads), 0, s, text, len, first, start);
  return hipGetLastError();
}

static unsigned samp_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + kSpWaves - 1) / kSpWaves, 1u << 16); }

hipError_t launch_samp_measure(const uint8_t* text, const uint64_t* start, uint64_t n, const uint32_t* dict_off,
                               const uint8_t* dict_bytes, const int32_t* dict_idx, int32_t dict_n, uint64_t* rlen,
                               unsigned long long* bad, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_samp_measure, dim3(samp_grid(n)), dim3(kSpThreads), 0, s, text, start, n,
                     SpDict{dict_off, dict_bytes, dict_idx, dict_n}, rlen, bad);
  return hipGetLastError();
}

hipError_t launch_samp_write(const uint8_t* text, const uint64_t* start, uint64_t n, const uint32_t* dict_off,
                             const uint8_t* dict_bytes, const int32_t* dict_idx, int32_t dict_n, const uint64_t* roff,
                             uint8_t* dst, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_samp_write, dim3(samp_grid(n)), dim3(kSpThreads), 0, s, text, start, n,
                     SpDict{dict_off, dict_bytes, dict_idx, dict_n}, roff, dst);
  return hipGetLastError();
}

}  // namespace hbam
