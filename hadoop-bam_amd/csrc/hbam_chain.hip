// hbam_chain.hip -- gfx950 kernels of the BAM record-boundary chain ([htsjdk]
// BAMRecordCodec.decode; SplittingBAMIndexer.java:340-368).  In file order:
//   the record rules    SAMRecord.isValid under STRICT / LENIENT (one rule
//                       list around a lane's or a wave's pass over the cigar),
//                       the dead positions, plausible() for the guesses
//   k_rec_link          the exact serial link (fallback)
//   k_rec_emit          positions + voffs by walking (count path)
//   the walk stage      k_rec_walk_wave (or k_rec_cand + k_rec_walk), then
//                       k_rec_search: a guessed chain and a record list per block
//   k_rec_linkfix       the parallel link check; k_rec_walk re-walks what it forces
//   check_listed_h      the reader / indexer rules per record, for
//   k_rec_count           the count path (a list overflowed) and
//   k_rec_check_out       the list path: check + output in one launch
//   launch_*            the host wrappers (hbam_launch.h)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "hbam_dev_util.h"
#include "hbam_device.h"
#include "hbam_launch.h"
#include "hbam_record_dev.h"

namespace hbam {

struct ChainEnv {  // (the device's part of ChainArgs: chain_env below)
  const uint8_t* u;        // inflated stream
  const BlockInfo* blocks;
  uint64_t e_inf;          // end of inflated (available) data
  uint64_t e_true;         // end of the logical stream (all blocks)
  uint64_t p0;             // span start position (first record, read after seek)
  uint64_t q_end;          // records with position >= q_end are outside the span
  const uint64_t* dead;    // sorted dead positions (empty block after exhausted one)
  uint32_t ndead;
  int32_t n_ref;
  uint32_t k0, k1;         // block range [k0, k1)
  int validate;            // reader mode: 0 SILENT (none), 1 LENIENT (decode structure), 2 STRICT (SAMRecord.isValid)
  const int32_t* ref_len;  // n_ref reference lengths, or nullptr
};

// ---------------------------------------------------------------------------
// [htsjdk] SAMRecord.isValid under ValidationStringency.STRICT.  BAMFileReader's
// iterator validates every record it returns unless the stringency is SILENT
// (BAMRecordReader.java:142,192-194 pass hadoopbam.samheaderreader.
// validation-stringency through; htsjdk's default is STRICT) and STRICT turns
// the first error into a SAMFormatException.  Restated subset (DESIGN.md
// §2.1; oracle/hbam_oracle.c orc_strict_invalid is the same rule list):
//   structure  read name, cigar, seq, qual inside the record; cigar op <= 8
//   unpaired   no proper-pair / mate-unmapped / mate-reverse / first / second
//              flag, mate refID == -1
//   paired     mate refID/pos consistent (isValidReferenceIndexAndPosition),
//              mate refID set unless mate-unmapped, first or second flag
//   unmapped   not secondary / supplementary, MAPQ 0, no cigar
//   mapped     cigar present, non-empty sequence dictionary
//   position   refID/pos consistent, pos+1 <= reference length
//   cigar      Cigar.isValid (zero-length ops, H/S/P placement, I/D pairs,
//              a real operator) and M/=/X blocks inside the reference
//   bin        == reg2bin(alignmentStart-1, alignmentEnd)
//   seq        cigar read length == l_seq when both are non-zero;
//              l_seq == 0 needs FZ, or CQ + CS (unless secondary)
// The reader's IllegalArgumentException (refID out of range) is checked
// before this, as the record factory raises it first.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int reg2bin_dev(int beg, int end) {  // GenomicIndexUtil.regionToBin
  --end;
  if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
  if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
  if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
  if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
  if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
  return 0;
}

// aux tag t present (an l_seq == 0 record's FZ / CQ / CS lookup); *zlen = Z
// string length
__device__ bool aux_find(const uint8_t* u, uint64_t a, uint64_t e, uint16_t tag, int64_t* zlen) {
  while (a + 3 <= e) {
    const uint16_t t = (uint16_t)(u[a] | (u[a + 1] << 8));
    const uint8_t ty = u[a + 2];
    a += 3;
    int64_t sz;
    switch (ty) {
      case 'A': case 'c': case 'C': sz = 1; break;
      case 's': case 'S': sz = 2; break;
      case 'i': case 'I': case 'f': sz = 4; break;
      case 'Z': case 'H': {
        uint64_t j = a;
        while (j < e && u[j]) ++j;
        if (t == tag) *zlen = (int64_t)(j - a);
        sz = (int64_t)(j - a) + 1;
        break;
      }
      case 'B': {
        if (a + 5 > e) return false;
        const uint8_t sub = u[a];
        const int32_t cnt = (int32_t)ldu32(u, a + 1);
        const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
        if (cnt < 0) return false;
        sz = 5 + (int64_t)cnt * es;
        break;
      }
      default: return false;
    }
    if (t == tag) return true;
    if ((uint64_t)sz > e - a) return false;  // a malformed aux block ends the lookup
    a += (uint64_t)sz;
  }
  return false;
}

// The rule list, each rule once: the rules that read only the record's head
// (record_structure_invalid, head_rules_invalid), what a pass over the cigar
// establishes (CigarFacts; one lane's serial loop or a wave's scans fill it,
// with one placement rule for both: cigar_op_misplaced), and the rules that
// consume it (cigar_rules_invalid).  Verdicts are booleans, so the order of
// the rules is free; what is loaded is not: nothing reads past q + 4 + bs.
struct RecFields {  // the fixed fields the rules read, off the record's head
  int32_t ref, pos, lseq, nref, npos;
  uint32_t lrn, mapq, bin, ncig, flag;
};
__device__ __forceinline__ RecFields rec_fields(const RecHead& h) {
  const uint32_t w12 = h.at(3), w16 = h.at(4);
  RecFields f;
  f.ref = (int32_t)h.at(1);
  f.pos = (int32_t)h.at(2);
  f.lrn = w12 & 0xffu;
  f.mapq = (w12 >> 8) & 0xffu;
  f.bin = w12 >> 16;
  f.ncig = w16 & 0xffffu;
  f.flag = w16 >> 16;
  f.lseq = (int32_t)h.at(5);
  f.nref = (int32_t)h.at(6);
  f.npos = (int32_t)h.at(7);
  return f;
}

// structure: the lazy fields isValid decodes must lie inside the record
__device__ __forceinline__ bool record_structure_invalid(const RecFields& f, int32_t bs) {
  if (f.lrn < 1 || f.lseq < 0) return true;
  const int64_t need = 32 + (int64_t)f.lrn + 4 * (int64_t)f.ncig + ((int64_t)f.lseq + 1) / 2 + (int64_t)f.lseq;
  return need > (int64_t)bs;
}

// STRICT: unpaired / paired, unmapped / mapped, position, mate position
__device__ __forceinline__ bool head_rules_invalid(const ChainEnv& E, const RecFields& f) {
  const uint32_t flag = f.flag;
  if (!(flag & 0x1)) {
    if (flag & (0x2 | 0x8 | 0x20 | 0x40 | 0x80)) return true;
    if (f.nref != -1) return true;
  } else {
    if (f.nref == -1) {
      if (f.npos != -1) return true;
      if (!(flag & 0x8)) return true;  // "Mapped mate should have mate reference name"
    } else {
      if (f.npos == -1) return true;
      if (E.ref_len && (int64_t)f.npos + 1 > (int64_t)E.ref_len[f.nref]) return true;
    }
    if (!(flag & 0xC0)) return true;  // neither first nor second of pair
  }
  if (flag & 0x4) {
    if (flag & (0x100 | 0x800)) return true;
    if (f.mapq != 0) return true;  // (a cigar on an unmapped read is allowed: test.bam has them)
  } else {
    if (f.ncig == 0) return true;
    if (E.n_ref == 0) return true;  // MISSING_SEQUENCE_DICTIONARY
  }
  if (f.ref == -1) {
    if (f.pos != -1) return true;
  } else {
    if (f.pos == -1) return true;
    if (E.ref_len && (int64_t)f.pos + 1 > (int64_t)E.ref_len[f.ref]) return true;
  }
  return false;
}

// What a pass over the cigar establishes.  bad: an operator above 8 (all a
// LENIENT pass looks for), or under STRICT a broken Cigar.isValid rule of a
// mapped read; real: an operator other than S / H / P seen; qlen / rlen: read
// and reference bases (wrapping u32 sums); maxend: the furthest end of an
// M / = / X block.
struct CigarFacts {
  bool bad, real;
  uint32_t qlen, rlen;
  int64_t maxend;
};
__device__ __forceinline__ bool op_consumes_read(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
__device__ __forceinline__ bool op_consumes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// Cigar.isValid's rules for operator k by itself: a zero length, an H not at
// an end, an S with more than an H between it and an end, a P at the end or
// next to an operator that is not M I D N = X.  op_at(j) = operator j (called
// for a P's two neighbours only).
template <typename OpAt>
__device__ __forceinline__ bool cigar_op_misplaced(uint32_t k, uint32_t op, uint32_t len, uint32_t ncig, uint32_t first_op,
                                                   uint32_t last_op, OpAt op_at) {
  if (len == 0) return true;
  if (op == 5) return k != 0 && k != ncig - 1;
  if (op == 4) {
    if (k == 0 || k == ncig - 1) return false;
    if (k == 1) return !(ncig == 3 && last_op == 5) && first_op != 5;
    if (k == ncig - 2) return last_op != 5;
    return true;
  }
  if (op == 6 && k != 0) {
    if (k == ncig - 1) return true;
    const uint32_t pv = op_at(k - 1), nx = op_at(k + 1);
    const bool pr = pv <= 3 || pv == 7 || pv == 8, nr = nx <= 3 || nx == 7 || nx == 8;
    return !pr || !nr;
  }
  return false;
}

// CigarFacts by one lane's serial loop (cigars up to kWaveCigarOps operators
// in k_rec_check_out; any length in k_rec_count)
__device__ __forceinline__ CigarFacts cigar_facts_lane(const uint8_t* u, uint64_t c0, const RecFields& f, bool strict) {
  const uint32_t ncig = f.ncig;
  CigarFacts c{false, false, 0, 0, 0};
  for (uint32_t k = 0; k < ncig; ++k) {
    if ((ldu32(u, c0 + 4ull * k) & 0xfu) > 8) {
      c.bad = true;
      return c;
    }
  }
  if (!strict) return c;
  const bool unmapped = f.flag & 0x4;
  const auto op_at = [&](uint32_t j) { return ldu32(u, c0 + 4ull * j) & 0xfu; };
  const uint32_t first_op = ncig ? op_at(0) : 99u, last_op = ncig ? op_at(ncig - 1) : 99u;
  int64_t rpos = (int64_t)f.pos + 1;
  // Cigar.isValid: between two separators (M/=/X/N or P) an I or a D may
  // appear only once ("No M or N operator between pair of I/D operators")
  bool seen_i = false, seen_d = false;
  for (uint32_t k = 0; k < ncig; ++k) {
    const uint32_t w = ldu32(u, c0 + 4ull * k), op = w & 0xfu, len = w >> 4;
    if (op_consumes_read(op)) c.qlen += len;
    if (op_consumes_ref(op)) c.rlen += len;
    if (!unmapped) {
      c.bad = cigar_op_misplaced(k, op, len, ncig, first_op, last_op, op_at) || (op == 1 && seen_i) || (op == 2 && seen_d);
      if (c.bad) return c;
      if (op == 6) {
        seen_i = seen_d = false;
      } else if (op != 4 && op != 5) {  // real operator
        c.real = true;
        if (op == 1) seen_i = true;
        else if (op == 2) seen_d = true;
        else seen_i = seen_d = false;
        if (op == 0 || op == 7 || op == 8) c.maxend = max(c.maxend, rpos + (int64_t)len - 1);
      }
    }
    if (op_consumes_ref(op)) rpos += len;
  }
  return c;
}

// CigarFacts by a whole wave, for records with long cigars (ONT-like reads
// carry thousands of operators; one lane walking them serially set the pace
// of the record check: 2.0 ms per C4 pass).  Same facts: the per-operator
// rules become a lane-per-operator pass over chunks of 64, the running state
// becomes scans --
//   qlen / rlen            wrapping u32 sums (as the serial u32 accumulators)
//   alignment block ends   exclusive 64-bit sum of reference lengths before k
//   Cigar.isValid I/D pairs   an I (D) is invalid when the previous I (D)
//                          comes after the last separator (M N = X P) before it:
//                          two running max-scans of 1-based indices.
// Wave-uniform arguments; returns the same facts on every lane.
__device__ __forceinline__ CigarFacts cigar_facts_wave(const uint8_t* u, uint64_t c0, const RecFields& f, bool strict) {
  const uint32_t lane = lane_id(), ncig = f.ncig;
  CigarFacts c{false, false, 0, 0, 0};
  bool bad = false;
  for (uint32_t k = lane; k < ncig; k += 64) bad |= (ldu32(u, c0 + 4ull * k) & 0xfu) > 8;
  c.bad = __ballot(bad) != 0;
  if (c.bad || !strict) return c;
  const bool unmapped = f.flag & 0x4;
  const auto op_at = [&](uint32_t j) { return ldu32(u, c0 + 4ull * j) & 0xfu; };
  const uint32_t first_op = ncig ? op_at(0) : 99u, last_op = ncig ? op_at(ncig - 1) : 99u;
  uint32_t qlen = 0, rlen = 0;          // lane partial sums (wrapping, as the serial code)
  uint64_t rcarry = 0;                  // reference bases of the chunks before
  uint32_t sep_carry = 0, i_carry = 0, d_carry = 0;  // 1-based indices of the last separator / I / D
  bool real = false;
  int64_t maxend = 0;
  for (uint32_t k0 = 0; k0 < ncig; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool in = k < ncig;
    const uint32_t w = in ? ldu32(u, c0 + 4ull * k) : 0u, op = in ? w & 0xfu : 15u, len = w >> 4;
    if (op_consumes_read(op)) qlen += len;
    if (op_consumes_ref(op)) rlen += len;
    const uint64_t rl = op_consumes_ref(op) ? (uint64_t)len : 0ull;
    const uint64_t rincl = wave_incl_sum64(rl);
    const int64_t rpos = (int64_t)f.pos + 1 + (int64_t)(rcarry + rincl - rl);  // before op k
    rcarry += (uint64_t)__builtin_amdgcn_readlane((int)(uint32_t)rincl, 63) |
              ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rincl >> 32), 63) << 32);
    // running 1-based indices (0 = none) up to and including op k
    const bool sep = op == 0 || op == 3 || op == 6 || op == 7 || op == 8;
    const uint32_t sep_i = max(sep_carry, wave_incl_max_dpp(sep ? k + 1 : 0u));
    const uint32_t i_i = max(i_carry, wave_incl_max_dpp(op == 1 ? k + 1 : 0u));
    const uint32_t d_i = max(d_carry, wave_incl_max_dpp(op == 2 ? k + 1 : 0u));
    // the same before op k (exclusive): one lane up, the carry on lane 0
    uint32_t sep_x = (uint32_t)__shfl_up((int)sep_i, 1, 64), i_x = (uint32_t)__shfl_up((int)i_i, 1, 64),
             d_x = (uint32_t)__shfl_up((int)d_i, 1, 64);
    if (lane == 0) {
      sep_x = sep_carry;
      i_x = i_carry;
      d_x = d_carry;
    }
    sep_carry = (uint32_t)__builtin_amdgcn_readlane((int)sep_i, 63);
    i_carry = (uint32_t)__builtin_amdgcn_readlane((int)i_i, 63);
    d_carry = (uint32_t)__builtin_amdgcn_readlane((int)d_i, 63);
    if (in && !unmapped) {
      if (cigar_op_misplaced(k, op, len, ncig, first_op, last_op, op_at)) bad = true;
      if (op != 4 && op != 5 && op != 6) {  // real operator
        real = true;
        if (op == 1 && i_x > sep_x) bad = true;  // a second I since the last separator
        if (op == 2 && d_x > sep_x) bad = true;
        if (op == 0 || op == 7 || op == 8) maxend = max(maxend, rpos + (int64_t)len - 1);
      }
    }
  }
  c.bad = __ballot(bad) != 0;
  c.real = __ballot(real) != 0;
  c.qlen = wave_sum_u32(qlen);
  c.rlen = wave_sum_u32(rlen);
  c.maxend = wave_max_i64(maxend);
  return c;
}

// STRICT: the rules on what the cigar pass found
__device__ __forceinline__ bool cigar_rules_invalid(const ChainEnv& E, uint64_t q, int32_t bs, const RecFields& f,
                                                    const CigarFacts& c) {
  const bool unmapped = f.flag & 0x4;
  if (!unmapped) {
    if (!c.real) return true;
    if (f.ref >= 0 && E.ref_len && c.maxend > (int64_t)E.ref_len[f.ref]) return true;  // CIGAR_MAPS_OFF_REFERENCE
  }
  // bin: computeIndexingBin()
  {
    const int start0 = f.pos;  // getAlignmentStart() - 1
    int end = unmapped ? 0 : (int)((int64_t)f.pos + 1 + (int64_t)c.rlen - 1);
    if (end <= 0) end = start0 + 1;
    if ((uint32_t)reg2bin_dev(start0, end) != f.bin) return true;
  }
  if (f.lseq != 0 && f.ncig != 0 && (int64_t)c.qlen != (int64_t)f.lseq) return true;  // MISMATCH_CIGAR_SEQ_LENGTH
  if (f.lseq == 0 && !(f.flag & 0x100)) {  // EMPTY_READ unless FZ, or CQ and CS
    const uint64_t a0 = q + 36 + f.lrn + 4ull * f.ncig, ae = q + 4 + (uint64_t)bs;
    int64_t zl = -1;
    if (!aux_find(E.u, a0, ae, (uint16_t)('F' | ('Z' << 8)), &zl)) {
      int64_t cq = -1, cs = -1;
      const bool hq = aux_find(E.u, a0, ae, (uint16_t)('C' | ('Q' << 8)), &cq);
      const bool hs = aux_find(E.u, a0, ae, (uint16_t)('C' | ('S' << 8)), &cs);
      if (!hq || !hs || cq <= 0 || cs <= 0) return true;
    }
  }
  return false;
}

// true when the (fully inflated) record at q fails validation: the rules
// above around the given pass over the cigar.  strict = false keeps only the
// structural decode failures (LENIENT still decodes the cigar for isValid and
// logs the rest).
template <typename Facts>
__device__ __forceinline__ bool record_invalid_by(const ChainEnv& E, uint64_t q, int32_t bs, bool strict, const RecFields& f,
                                                  Facts cigar_facts) {
  if (record_structure_invalid(f, bs)) return true;
  if (strict && head_rules_invalid(E, f)) return true;
  const CigarFacts c = cigar_facts(E.u, q + 36 + f.lrn, f, strict);
  if (c.bad) return true;
  return strict && cigar_rules_invalid(E, q, bs, f, c);
}

// One lane's verdict.  *defer (when given): a cigar longer than kWaveCigarOps
// operators is not checked here (false returned, *defer set) --
// record_invalid_wave takes it.
// (h: the record's head, load_head(E.u, q), already in registers)
__device__ __forceinline__ bool record_invalid_h(const ChainEnv& E, uint64_t q, int32_t bs, bool strict, bool* defer,
                                                 const RecHead& h) {
  const RecFields f = rec_fields(h);
  if (defer && f.ncig > kWaveCigarOps) {
    *defer = true;
    return false;
  }
  return record_invalid_by(E, q, bs, strict, f, [](const uint8_t* u, uint64_t c0, const RecFields& f, bool strict) {
    return cigar_facts_lane(u, c0, f, strict);
  });
}

__device__ __forceinline__ uint64_t rfl_u64(uint64_t v) {
  return (uint64_t)rfl((uint32_t)v) | ((uint64_t)rfl((uint32_t)(v >> 32)) << 32);
}

// A whole wave's verdict on one record (wave-uniform arguments, taken as
// scalars: the record's fields then live in SGPRs beside the caller's
// per-lane state; the same value on every lane).
__device__ bool record_invalid_wave(const ChainEnv& E, uint64_t q, int32_t bs, bool strict) {
  q = rfl_u64(q);
  bs = (int32_t)rfl((uint32_t)bs);
  return record_invalid_by(E, q, bs, strict, rec_fields(load_head(E.u, q)),
                           [](const uint8_t* u, uint64_t c0, const RecFields& f, bool strict) {
                             return cigar_facts_wave(u, c0, f, strict);
                           });
}

__device__ __forceinline__ bool is_dead(const ChainEnv& E, uint64_t q) {
  uint32_t lo = 0, hi = E.ndead;  // sorted; usually 0 or 1 entries (the EOF marker)
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (E.dead[mid] < q) lo = mid + 1; else hi = mid;
  }
  return lo < E.ndead && E.dead[lo] == q;
}
__device__ __forceinline__ bool dead_in_record(const ChainEnv& E, uint64_t q, int32_t bs) {
  if (E.ndead == 0) return false;
  const uint8_t offs[11] = {4, 8, 12, 13, 14, 16, 18, 20, 24, 28, 32};
  for (int i = 0; i < 11; ++i)
    if (is_dead(E, q + offs[i])) return true;
  return bs > 32 && is_dead(E, q + 36);
}

// Is any dead position within [q, q + 40] (header fields + first rest byte)?
__device__ __forceinline__ bool dead_near(const ChainEnv& E, uint64_t q) {
  uint32_t lo = 0, hi = E.ndead;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (E.dead[mid] < q) lo = mid + 1; else hi = mid;
  }
  return lo < E.ndead && E.dead[lo] <= q + 40;
}

// Necessary conditions for a record of a well-formed BAM (guess only; the
// true chain is fixed by the link step, never by this test).  Bytes past the
// inflated range of a stream that goes on (an open window, or blocks not yet
// inflated) cannot refute a record: it stays plausible when its block_size
// can be read and is >= 32 (so a walk through it still moves forward).
// (Taken as implausible, the record straddling a window's end within its
// first 36 + l_read_name bytes failed every candidate walk of its block, and
// the block's search walked from every later candidate: ~7 ms on one 256 MiB
// drop-in window.)
// The rules split for a software-pipelined walk: plausible_head decides from
// q's head h alone (1: plausible, 0: not, 2: the read-name end byte at
// q + 36 + lrn - 1 decides: *name_at = its position), so that a walk can
// load that byte together with the next record's head (q + 4 + block_size):
// one dependent memory round trip per record instead of two.  h =
// load_head(E.u, q); it is not looked at when q + 4 > e_inf.
__device__ __forceinline__ int plausible_head(const ChainEnv& E, uint64_t q, const RecHead& h, uint64_t* name_at) {
  if (q + 36 > E.e_inf) return E.e_inf < E.e_true && q + 4 <= E.e_inf && (int32_t)h.at(0) >= 32;
  int32_t bs = (int32_t)h.at(0);
  int32_t ref = (int32_t)h.at(1);
  int32_t pos = (int32_t)h.at(2);
  uint32_t lrn = h.at(3) & 0xffu;
  uint32_t ncig = h.at(4) & 0xffffu;
  int32_t lseq = (int32_t)h.at(5);
  int32_t nref = (int32_t)h.at(6);
  int32_t npos = (int32_t)h.at(7);
  if (ref < -1 || ref >= E.n_ref || nref < -1 || nref >= E.n_ref) return 0;
  if (pos < -1 || npos < -1 || lrn < 1 || lseq < 0) return 0;
  int64_t need = 32 + (int64_t)lrn + 4 * (int64_t)ncig + (int64_t)lseq + ((int64_t)lseq + 1) / 2;
  if ((int64_t)bs < need) return 0;
  if (q + 4 + (uint64_t)bs > E.e_true) return 0;
  if (q + 36 + lrn > E.e_inf) return E.e_inf < E.e_true;
  *name_at = q + 36 + lrn - 1;
  return 2;
}
// the head of the record at q for plausible_head (a q whose block_size is
// not inflated is not read: q0's bytes instead, which it does not look at)
__device__ __forceinline__ RecHead plausible_load(const ChainEnv& E, uint64_t q, uint64_t q0) {
  return load_head(E.u, q + 4 <= E.e_inf ? q : q0);
}
__device__ __forceinline__ bool plausible(const ChainEnv& E, uint64_t q) {
  uint64_t name_at = 0;
  const int ph = plausible_head(E, q, plausible_load(E, q, 0), &name_at);
  return ph == 2 ? E.u[name_at] == 0 : ph != 0;
}

// plausible() at q and at the record after it (or the end / unreadable data):
// a cheap second check that removes most false candidates inside long records.
__device__ __forceinline__ bool plausible2(const ChainEnv& E, uint64_t q) {
  if (!plausible(E, q)) return false;
  const uint64_t q2 = q + 4 + (uint64_t)(int32_t)ldu32(E.u, q);
  return q2 == E.e_true || q2 + 36 > E.e_inf || plausible(E, q2);
}

// A necessary condition of plausible() that reads 8 bytes: refID and mate
// refID in range (random bytes pass with probability ~(n_ref / 2^32)^2), or
// data past the inflated range, which plausible() judges itself.  Candidate
// scans test it first and run plausible2 only when a lane of the wave passes.
// (ref, nref: the dwords at q + 4 and q + 24, however the scan came by them;
// branch-free, a scan evaluates it for 8 positions a lane)
__device__ __forceinline__ bool refs_prefilter(const ChainEnv& E, int32_t ref, int32_t nref, uint64_t q) {
  return (q + 36 > E.e_inf) | ((ref >= -1) & (ref < E.n_ref) & (nref >= -1) & (nref < E.n_ref));
}
__device__ __forceinline__ bool cand_prefilter(const ChainEnv& E, uint64_t q) {
  const bool inflated = q + 36 <= E.e_inf;  // (nothing is read past the inflated range)
  return refs_prefilter(E, inflated ? (int32_t)ldu32(E.u, q + 4) : 0, inflated ? (int32_t)ldu32(E.u, q + 24) : 0, q);
}

// One chain step from q under the given rules.  Returns false if the walk
// cannot continue (data unavailable or malformed record); *nq = next position.
template <int MODE>
__device__ __forceinline__ bool chain_step(const ChainEnv& E, uint64_t q, uint64_t* nq) {
  if (q + 4 > E.e_inf) return false;
  int32_t bs = (int32_t)ldu32(E.u, q);
  if (MODE == kReader) {
    if (bs < 32) return false;
    *nq = q + 4 + (uint64_t)bs;
  } else {
    *nq = q + 4 + (bs > 0 ? (uint64_t)bs : 0);
  }
  return true;
}

// Link the per-block guesses into the true chain (serial in block order, with
// a 256-block tile fast path when every block of the tile links to the next).
// entry[i] = true first record position of block k0+i, or kNone.
// summary[0] = final chain position, summary[1] = 1 if the chain stopped
// inside a block (malformed record / data unavailable).
template <int MODE>
__global__ __launch_bounds__(256) void k_rec_link(ChainEnv E, const uint64_t* __restrict__ g,
                                                  const uint64_t* __restrict__ x, uint64_t* __restrict__ entry,
                                                  uint64_t* __restrict__ summary) {
  __shared__ uint64_t s_cur;
  __shared__ int s_stop;
  const uint32_t nb = E.k1 - E.k0;
  if (threadIdx.x == 0) { s_cur = E.p0; s_stop = 0; }
  __syncthreads();
  for (uint32_t t0 = 0; t0 < nb; t0 += 256) {
    const uint32_t i = t0 + threadIdx.x;
    const uint64_t cur = s_cur;
    const int stop = s_stop;
    bool fast = true;
    if (i < nb) {
      const BlockInfo b = E.blocks[E.k0 + i];
      const uint64_t bend = b.ustart + b.isize;
      const uint64_t gi = g[i], xi = x[i];
      const uint64_t expect = (threadIdx.x == 0) ? cur : x[i - 1];
      fast = !stop && gi != kNone && gi == expect && gi < E.q_end && xi != kNone && xi >= bend;
    }
    const int all_fast = __syncthreads_and(fast);
    if (all_fast) {
      if (i < nb) entry[i] = g[i];
      __syncthreads();
      if (threadIdx.x == 0) s_cur = x[min(t0 + 255, nb - 1)];
      __syncthreads();
      continue;
    }
    if (threadIdx.x == 0) {
      uint64_t c = cur;
      int st = stop;
      for (uint32_t j = t0; j < min(t0 + 256, nb); ++j) {
        const BlockInfo b = E.blocks[E.k0 + j];
        const uint64_t bend = b.ustart + b.isize;
        if (st || c >= E.q_end || c >= bend || b.isize == 0) {
          entry[j] = kNone;
          continue;
        }
        entry[j] = c;
        if (g[j] == c) {
          c = x[j];
        } else {
          uint64_t q = c, nq;
          while (q < bend && chain_step<MODE>(E, q, &nq)) q = nq;
          c = q;
        }
        if (c < bend) st = 1;
      }
      s_cur = c;
      s_stop = st;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    summary[0] = s_cur;
    summary[1] = (uint64_t)s_stop;
  }
}

// Parallel link.  y[i] = guess exit of block i (0 when the block has no
// guess); in[i] = max(y[0..i-1]) is the position the chain enters block i
// with, IF every guess is on the true chain.  k_rec_link_check verifies that
// claim block by block (entry = guess where the chain enters the block,
// pass-through elsewhere) and counts violations; any violation sends the span
// to the exact serial link (k_rec_link).
__global__ void k_rec_link_y(const uint64_t* __restrict__ g, const uint64_t* __restrict__ x, uint32_t nb,
                             uint64_t* __restrict__ y) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) y[i] = (g[i] != kNone && x[i] != kNone) ? x[i] : 0;
}

// Second walk: write record positions and normalized voffs at base[i].
template <int MODE>
__global__ void k_rec_emit(ChainEnv E, const uint64_t* __restrict__ entry, const uint32_t* __restrict__ cnt,
                           const uint64_t* __restrict__ base, uint64_t* __restrict__ rec_pos,
                           uint64_t* __restrict__ rec_voff) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nb = E.k1 - E.k0;
  if (i >= nb) return;
  const uint32_t n = cnt[i];
  if (n == 0) return;
  const BlockInfo b = E.blocks[E.k0 + i];
  uint64_t q = entry[i];
  uint64_t o = base[i];
  for (uint32_t r = 0; r < n; ++r) {
    rec_pos[o + r] = q;
    rec_voff[o + r] = (b.coff << 16) | (q - b.ustart);
    const int32_t bs = (int32_t)ldu32(E.u, q);
    q += 4 + (uint64_t)(MODE == kReader ? bs : (bs > 0 ? bs : 0));
  }
}

// ---------------------------------------------------------------------------
// The walk stage: a guessed chain and a list of record starts per block
// ---------------------------------------------------------------------------
//   k_rec_walk_wave  one wave per block: the block's first plausible record
//                  start (its candidate), then a lane per 4 KiB segment walks
//                  from the segment's first plausible start, and the lists are
//                  stitched where the chain from the candidate meets them.
//                  Every record start of the block is listed as a u16 offset
//                  (g = the walk's start, x = its exit, wcnt = the count).
//                  The block of the span start has a known entry: one lane
//                  walks it by block_size alone (walk_entry).
//   k_rec_cand + k_rec_walk  the same in two launches, a wave per block for the
//                  candidate and a lane per block for the walk: the A/B of the
//                  above (kStageWalkLane).  k_rec_walk also runs the forced
//                  re-walk rounds of the link check.
//   k_rec_search   blocks whose candidate's walk met an implausible record
//                  (g == kRetry): the later candidates in order.
//   k_rec_linkfix  max-scan link check; blocks whose list is off the chain are
//                  re-walked from their true entry (usually zero or a few).
//   k_rec_check_out  one wave per block: the reader / indexer rules
//                  (check_listed_h) for every listed record at once (the first
//                  stop gives count, status and the bytes still to inflate), then
//                  positions, voffs and (reader) the fused decode + key at the
//                  block's scanned base.
// Shared by the walks: walk_plausible (every record must pass plausible(), to
// a limit or to the block end and kGuessLookahead records beyond), walk_entry
// (from a known entry by chain_step), wave_pull_block (the block into L2
// before one lane's dependent loads).
// k_rec_cand: one wave per block, each lane testing kCandPos consecutive
// positions per step (512 per step): refID and mate refID of its 8 positions
// come from 5 aligned 8 B loads, and only the rare position that passes that
// test runs plausible2; the first hit wins (ballot).  A short-read block
// finishes in its first step, at the cost of the old 64-positions step; a
// long-read block (C4: the first record start lies ~32 KB in on average)
// takes 8x fewer dependent steps (0.74 ms per C4 pass before).
constexpr int kCandPos = 8;
// The scan as a wave-level function: the first plausible2 position of [lo,
// bend), kNone when there is none; wave-uniform arguments, the same result
// on every lane.  STEPS consecutive 512-position steps have their loads in
// flight together (one round trip for STEPS steps; k_rec_walk_wave scans
// long-read blocks 4 steps at a time) and are then tested in order.
template <int STEPS>
__device__ __forceinline__ uint64_t cand_scan_wave(const ChainEnv& E, uint64_t lo, uint64_t bend) {
  const uint32_t lane = lane_id();
  const uint64_t s0 = lo & ~7ull;  // 8-aligned scan origin (positions < lo are masked)
  for (uint64_t c00 = s0; c00 < bend; c00 += (uint64_t)STEPS * 64 * kCandPos) {
    uint32_t passes[STEPS];  // bit j: position p0 + j of that step passes the prefilter
#pragma unroll
    for (int t = 0; t < STEPS; ++t) {
      const uint64_t p0 = c00 + (uint64_t)t * 64 * kCandPos + (uint64_t)lane * kCandPos;
      uint32_t pass = 0;
      uint32_t w[10];
      // (a step past the block end loads the origin's bytes and passes nothing: no
      // branch around the loads, so that the steps' loads go out together)
      const uint2* src = reinterpret_cast<const uint2*>(E.u + (p0 < bend ? p0 : s0));  // du_ is padded past the stream
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const uint2 v = src[i];
        w[2 * i] = v.x;
        w[2 * i + 1] = v.y;
      }
#pragma unroll
      for (int j = 0; j < kCandPos; ++j) {
        const uint64_t q = p0 + j;
        const int32_t ref = (int32_t)__builtin_amdgcn_alignbyte(w[2 + (j >> 2)], w[1 + (j >> 2)], j & 3);
        const int32_t nref = (int32_t)__builtin_amdgcn_alignbyte(w[7 + (j >> 2)], w[6 + (j >> 2)], j & 3);
        const bool ok = (q >= lo) & (q < bend) & refs_prefilter(E, ref, nref, q);
        pass |= ok ? 1u << j : 0u;
      }
      passes[t] = pass;
    }
#pragma unroll
    for (int t = 0; t < STEPS; ++t) {
      const uint64_t c0 = c00 + (uint64_t)t * 64 * kCandPos;
      const uint64_t p0 = c0 + (uint64_t)lane * kCandPos;
      const uint32_t pass = passes[t];
      uint32_t hit = kCandPos;  // the first position of this lane that is plausible2
      if (__ballot(pass != 0)) {
        for (uint32_t m = pass; m; m &= m - 1) {
          const uint32_t j = (uint32_t)__ffs((int)m) - 1;
          if (plausible2(E, p0 + j)) {
            hit = j;
            break;
          }
        }
      }
      const uint64_t hm = __ballot(hit < kCandPos);
      if (hm) {
        const uint32_t f = (uint32_t)__ffsll((long long)hm) - 1;
        return c0 + (uint64_t)f * kCandPos + (uint32_t)__shfl((int)hit, (int)f, 64);
      }
    }
  }
  return kNone;
}

// A start 1-3 bytes before a true record reads that record's block_size
// shifted up by whole bytes (~2^8-2^24 times it) and, with refID 0, its
// fields stay in range: plausible2 passes and the walk leaves the block
// at once -- past the inflated end of a window it cannot be checked, and
// the link check then re-walks the block and the ones its far exit hid
// (one round each; C2 passes took two, drop-in windows fell back to the
// serial link).  When c's record leaves the block, a plausible2 start
// 1-3 bytes later whose record ends inside the block is taken instead.
// (One lane's work; c != kNone.)
__device__ __forceinline__ uint64_t cand_shift(const ChainEnv& E, uint64_t c, uint64_t bend) {
  if (c + 4 + (uint64_t)(int32_t)ldu32(E.u, c) >= bend) {
    for (uint32_t d = 1; d <= 3; ++d) {
      const uint64_t q = c + d;
      if (q + 36 <= E.e_inf && q + 4 + (uint64_t)(int32_t)ldu32(E.u, q) < bend && plausible2(E, q)) return q;
    }
  }
  return c;
}

// the blocks that get a candidate: past the span's first block, inside the span
__device__ __forceinline__ bool cand_wanted(const ChainEnv& E, const BlockInfo& b) {
  return b.ustart + b.isize > E.p0 && b.ustart > E.p0 && b.ustart < E.q_end && b.isize > 0;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_rec_cand(ChainEnv E, uint64_t* __restrict__ cand) {
  const BlockInfo b = E.blocks[E.k0 + blockIdx.x];
  const uint64_t bend = b.ustart + b.isize;
  uint64_t c = kNone;
  if (cand_wanted(E, b)) {
    c = cand_scan_wave<1>(E, b.ustart, bend);
    if (c != kNone && lane_id() == 0) c = cand_shift(E, c, bend);
  }
  if (lane_id() == 0) cand[blockIdx.x] = c;
}

constexpr int kGuessLookahead = 4;  // plausible records required past a guess walk's exit
constexpr uint64_t kRetry = ~0ull - 2;  // g[]: the candidate's walk failed, search on
constexpr uint32_t kListPlausible = 0x80000000u;  // wcnt flag: the list came from a plausible() walk
constexpr uint32_t kListCountMask = 0x7fffffffu;

// The plausible walk from `start`: every record must pass plausible(); the
// records that start before lim are listed (put(index, position)).  With lim
// == bend (the block end) the walk goes on for kGuessLookahead records past
// the block end, or to the end of the stream or of the inflated range; with
// lim < bend it ends at the first record start at or past lim.  exitq = that
// first start at or past lim, n = the records listed.
// Software-pipelined: record q's read-name end byte and the next record's
// head are loaded together (plausible_head), one dependent round trip per
// record.  Loads past the inflated range read the stream's padding and are
// not used (plausible_head's rules).
struct PlausWalk {
  bool valid;
  uint64_t exitq;
  uint32_t n;
};
template <typename Put>
__device__ __forceinline__ PlausWalk walk_plausible(const ChainEnv& E, uint64_t start, uint64_t lim, uint64_t bend,
                                                    Put put) {
  uint64_t q = start, exitq = start;
  uint32_t m = 0;
  bool valid = true;
  // (a start past the inflated range -- an exit handed on for its lookahead --
  // is not read: the loop ends before it looks at h)
  RecHead h = plausible_load(E, start, 0);
  int left = kGuessLookahead;  // plausible records required past the block end
  for (;;) {
    const bool inside = q < lim;
    if (!inside && (lim < bend || left-- <= 0 || q == E.e_true || q + 36 > E.e_inf)) break;
    uint64_t na = q;
    const int ph = plausible_head(E, q, h, &na);
    const uint64_t q2 = q + 4 + (uint64_t)(int32_t)h.at(0);
    const uint8_t nb = E.u[na];
    // (q2 may lie anywhere: its head is loaded when its block_size is
    // inflated; reads reach 40 bytes past it, inside the stream's pad)
    h = plausible_load(E, q2, q);
    if (ph == 0 || (ph == 2 && nb != 0)) { valid = false; break; }
    if (inside) {
      put(m, q);
      ++m;
      exitq = q2;  // the first record start at or past lim (the walk's exit)
    }
    q = q2;
  }
  return PlausWalk{valid, exitq, m};
}

// walk_plausible with nothing listed: is the chain from `start` plausible to
// the block end and kGuessLookahead records beyond?
__device__ __forceinline__ bool plausible_to_block_end(const ChainEnv& E, uint64_t start, uint64_t bend) {
  return walk_plausible(E, start, bend, bend, [](uint32_t, uint64_t) {}).valid;
}

// The walk from a known entry (the span start, a forced entry, a candidate
// whose chain was found plausible): by block_size alone (chain_step), every
// record start before the block end listed in L.  Returns the count (it may
// pass kListCap: the caller raises the overflow word), *exitq = where the
// walk left the block or stopped.  One lane's work.
template <int MODE>
__device__ __forceinline__ uint32_t walk_entry(const ChainEnv& E, uint64_t entry, const BlockInfo& b,
                                               uint16_t* __restrict__ L, uint64_t* exitq) {
  const uint64_t bend = b.ustart + b.isize;
  uint64_t q = entry, nq;
  uint32_t n = 0;
  while (q < bend) {
    if (n < kListCap) L[n] = (uint16_t)(q - b.ustart);
    ++n;
    if (!chain_step<MODE>(E, q, &nq)) break;
    q = nq;
  }
  *exitq = q;
  return n;
}

// A lane's walk through a block is a chain of dependent loads from HBM (~190
// for a short-read block).  The whole wave first pulls the block's inflated
// bytes [lo, hi) and the lookahead past them into L2 with independent loads,
// so that the chain then runs at L2 latency.
__device__ __forceinline__ void wave_pull_block(const ChainEnv& E, uint64_t lo, uint64_t hi, uint32_t* overflow) {
  uint32_t acc = 0;
  const uint64_t end = min(hi + 4096, E.e_inf);
  for (uint64_t a = (lo & ~127ull) + 128ull * lane_id(); a < end; a += 128ull * 64) acc += ldu32(E.u, a);
  if (acc == 0x9e3779b9u && E.k0 == 0xffffffffu) atomicOr(overflow, 0u);  // keeps the loads (never true)
}

template <int MODE>
__global__ __launch_bounds__(256) void k_rec_walk(ChainEnv E, const uint64_t* __restrict__ cand,
                                                  const uint64_t* __restrict__ force, uint64_t* __restrict__ g_out,
                                                  uint64_t* __restrict__ x_out, uint32_t* __restrict__ wcnt,
                                                  uint16_t* __restrict__ list, uint32_t* __restrict__ overflow,
                                                  bool validate) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nb = E.k1 - E.k0;
  if (force) {
    // A re-walk round forces a few blocks, a lane each: the wave first pulls
    // every forced block of the wave into L2.
    const uint64_t fi = i < nb ? force[i] : kNone;
    for (uint64_t todo = __ballot(fi != kNone && fi != kForceEmpty); todo; todo &= todo - 1) {
      const uint32_t src = (uint32_t)__ffsll((long long)todo) - 1;
      const BlockInfo wb = E.blocks[E.k0 + blockIdx.x * blockDim.x + (threadIdx.x & ~63u) + src];
      wave_pull_block(E, wb.ustart, wb.ustart + wb.isize, overflow);
    }
  }
  if (i >= nb) return;
  uint64_t f = kNone;  // guess
  if (force) {
    f = force[i];
    if (f == kNone) return;  // keep this block's walk
  }
  const BlockInfo b = E.blocks[E.k0 + i];
  const uint64_t bend = b.ustart + b.isize;
  if (validate && f != kForceEmpty && f != kNone) {
    // a link-round entry may itself come from a wrong walk upstream (fixed in
    // the same round): re-walk only if the chain from it is plausible to the
    // block end and beyond; otherwise keep the old walk for the next round
    if (!plausible_to_block_end(E, f, bend)) return;
  }
  uint16_t* __restrict__ L = list + (uint64_t)i * kListCap;
  uint64_t g = kNone, x = kNone;
  uint32_t n = 0;
  bool plaus_list = false;  // every listed record passed plausible()
  const bool live = bend > E.p0 && b.ustart < E.q_end && b.isize > 0;
  if (live && f != kForceEmpty) {
    uint64_t entry = f;
    if (f == kNone && b.ustart <= E.p0) entry = E.p0;  // the block of the span start: entry known
    if (entry != kNone) {
      g = entry;
      n = walk_entry<MODE>(E, entry, b, L, &x);
    } else {
      const uint64_t c = cand[i];
      if (c < bend) {  // c == kNone (no candidate): nothing to walk
        const PlausWalk w = walk_plausible(E, c, bend, bend, [&](uint32_t m, uint64_t q) {
          if (m < kListCap) L[m] = (uint16_t)(q - b.ustart);
        });
        if (w.valid) {
          g = c;
          x = w.exitq;
          n = w.n;
          plaus_list = true;
        } else {
          g = kRetry;  // later candidates: k_rec_search (wave per block)
          n = 0;
        }
      }
    }
  }
  if (n > kListCap) atomicOr(overflow, 1u);
  g_out[i] = g;
  x_out[i] = x;
  wcnt[i] = n | (plaus_list ? kListPlausible : 0u);
}

// ---------------------------------------------------------------------------
// k_rec_walk_wave: the unforced round of k_rec_cand + k_rec_walk, one wave per
// block.  The chain from a block's candidate c is deterministic (the record at
// q names the next start), so a walk begun at any record start on it lists
// what the walk from c lists from there on.  The block is cut into kWalkSeg-
// byte segments counted from its start:
//   probe   every lane tests kCandPos positions of the first kWalkProbe bytes
//           of every segment against the refID prefilter (all segments' loads
//           in flight together); lane j then takes the first of segment j's
//           positions that is plausible2: c_j.  c_0 is the block's candidate
//           (cand_scan_wave over the rest of the block when segment 0's
//           window holds none), moved by cand_shift: what k_rec_cand writes.
//   walk    lane j runs walk_plausible from c_j (the segment holding c: from
//           c) up to the next segment's start, listing into its LDS row; the
//           last segment's walker also walks the lookahead past the block.
//   stitch  wave-uniform: cur = c; while cur is inside the block, walker k of
//           the segment holding cur is taken when c_k == cur (kRetry when it
//           met an implausible record: that record is on the chain from c),
//           else the whole wave walks on from cur to the end of segment k.
//           When the last piece did not end at the block end, the lookahead
//           is walked from the exit.
// g, x, wcnt, list, cand and the overflow word are those of the two kernels
// it replaces (tests/walk_wave_model.py restates the stitch; its test and
// tests/test_gpu_walk_wave.py hold the two equal).
// (experiment variants: make EXTRA="-DHBAM_WALK_SEG=... -DHBAM_WALK_WAVES=...")
#ifndef HBAM_WALK_SEG
#define HBAM_WALK_SEG 4096
#endif
#ifndef HBAM_WALK_WAVES
#define HBAM_WALK_WAVES 4
#endif
constexpr uint32_t kWalkSeg = HBAM_WALK_SEG;
constexpr uint32_t kWalkSegs = kMaxIsize / kWalkSeg;  // segments of the largest block
constexpr uint32_t kWalkProbe = 64 * kCandPos;        // positions probed per segment
constexpr uint32_t kSegListCap = kWalkSeg / 32;       // a walker's LDS row: 128 entries
// a plausible record takes at least 36 bytes (block_size >= 32), so a segment holds fewer starts than a row
static_assert(kWalkSeg / 36 + 1 < kSegListCap, "a segment's record starts fit its walker's row");
static_assert(kWalkSegs * kWalkSeg == kMaxIsize && kWalkSegs <= 64 && kWalkSegs % 8 == 0, "a lane per segment");
static_assert(kWalkProbe <= kWalkSeg, "a probe window inside its segment");
constexpr uint32_t kPassRow = 64 + 4;  // a segment's 64 pass bytes (+ a word: rows on different banks)

// (launch bounds: DESIGN.md 4.3, "k_rec_walk_wave")
template <int MODE>
__global__ __launch_bounds__(64, HBAM_WALK_WAVES) void k_rec_walk_wave(ChainEnv E, uint64_t* __restrict__ cand,
                                                         uint64_t* __restrict__ g_out, uint64_t* __restrict__ x_out,
                                                         uint32_t* __restrict__ wcnt, uint16_t* __restrict__ list,
                                                         uint32_t* __restrict__ overflow) {
  __shared__ uint16_t s_list[kWalkSegs][kSegListCap];
  __shared__ __attribute__((aligned(4))) uint8_t s_pass[kWalkSegs][kPassRow];
  const uint32_t i = blockIdx.x, lane = lane_id();
  const BlockInfo b = E.blocks[E.k0 + i];
  const uint64_t bend = b.ustart + b.isize;
  uint16_t* __restrict__ L = list + (uint64_t)i * kListCap;
  uint64_t g = kNone, x = kNone, c = kNone;
  uint32_t n = 0;
  bool plaus_list = false;
  const bool live = bend > E.p0 && b.ustart < E.q_end && b.isize > 0;
  if (live && b.ustart <= E.p0) {
    // the block of the span start: the entry is known, the walk goes by
    // block_size alone (walk_entry).  One lane's chain of dependent loads:
    // the wave pulls the block into L2 first, as a forced re-walk does, so
    // that the other blocks' waves do not wait on it.
    wave_pull_block(E, b.ustart, bend, overflow);
    if (lane == 0) {
      g = E.p0;
      n = walk_entry<MODE>(E, E.p0, b, L, &x);
    }
  } else if (live) {
    const uint32_t nseg = min((b.isize + kWalkSeg - 1) / kWalkSeg, kWalkSegs);
    // ---- probe: the prefilter over every segment's window, 8 segments' loads at a time
#pragma unroll
    for (uint32_t j0 = 0; j0 < kWalkSegs; j0 += 8) {
      U32x4 wa[8], wb[8];
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) {
        const uint64_t p0 = b.ustart + (uint64_t)(j0 + t) * kWalkSeg + (uint64_t)lane * kCandPos;
        const uint8_t* src = E.u + ((p0 < bend ? p0 : b.ustart) & ~3ull);  // (the stream is padded past its end)
        wa[t] = *reinterpret_cast<const U32x4*>(src + 4);   // refID of p0 .. p0 + 7
        wb[t] = *reinterpret_cast<const U32x4*>(src + 24);  // next refID of the same
      }
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) {
        const uint64_t p0 = b.ustart + (uint64_t)(j0 + t) * kWalkSeg + (uint64_t)lane * kCandPos;
        const uint32_t sh = (uint32_t)(p0 & 3);
        // the dwords at p0 + 4 (+ 4, + 8) and at p0 + 24 (+ 4, + 8)
        const uint32_t r0 = __builtin_amdgcn_alignbyte(wa[t].y, wa[t].x, sh), r1 = __builtin_amdgcn_alignbyte(wa[t].z, wa[t].y, sh),
                       r2 = __builtin_amdgcn_alignbyte(wa[t].w, wa[t].z, sh);
        const uint32_t m0 = __builtin_amdgcn_alignbyte(wb[t].y, wb[t].x, sh), m1 = __builtin_amdgcn_alignbyte(wb[t].z, wb[t].y, sh),
                       m2 = __builtin_amdgcn_alignbyte(wb[t].w, wb[t].z, sh);
        uint32_t pass = 0;  // bit k: position p0 + k passes the prefilter
#pragma unroll
        for (int k = 0; k < kCandPos; ++k) {
          const uint64_t q = p0 + k;
          const int32_t ref = (int32_t)__builtin_amdgcn_alignbyte(k < 4 ? r1 : r2, k < 4 ? r0 : r1, k & 3);
          const int32_t nref = (int32_t)__builtin_amdgcn_alignbyte(k < 4 ? m1 : m2, k < 4 ? m0 : m1, k & 3);
          const bool ok = (q < bend) & refs_prefilter(E, ref, nref, q);
          pass |= ok ? 1u << k : 0u;
        }
        s_pass[j0 + t][lane] = (uint8_t)(j0 + t < nseg ? pass : 0u);
      }
    }
    __syncthreads();
    // ---- lane j: the first plausible2 position of segment j's window
    // (every lane first finds its next passing position in LDS, then the
    // lanes run plausible2 together: its dependent loads are in flight for
    // all segments at once.  A lane whose position fails goes round again;
    // with a plausible2 per lane as it met its position, the lanes' three
    // round trips each ran one after another: 0.76 ms per C2 pass.)
    uint64_t cj = kNone;
    {
      const uint64_t sj = b.ustart + (uint64_t)lane * kWalkSeg;
      const uint32_t* row = reinterpret_cast<const uint32_t*>(s_pass[lane < nseg ? lane : 0]);
      bool scanning = lane < nseg;
      uint32_t w = 0, m = 0;  // m: the bits of word w - 1 not looked at yet (bit k: position sj + 32 (w - 1) + k)
      for (;;) {
        uint64_t q = kNone;
        if (scanning) {
          while (m == 0 && w < 16) m = row[w++];
          if (m) {
            q = sj + 32 * (w - 1) + ((uint32_t)__ffs((int)m) - 1);
            m &= m - 1;
          } else {
            scanning = false;
          }
        }
        if (__ballot(q != kNone) == 0) break;
        if (q != kNone && plausible2(E, q)) {
          cj = q;
          scanning = false;
        }
      }
    }
    // ---- the block's candidate (k_rec_cand's)
    c = shfl_u64(cj, 0);
    if (c == kNone && b.isize > kWalkProbe) c = cand_scan_wave<4>(E, b.ustart + kWalkProbe, bend);
    c = rfl_u64(c);
    if (c != kNone) c = rfl_u64(cand_shift(E, c, bend));
    if (c != kNone) {
      // ---- walk: lane j from its segment's start
      const uint32_t k0 = min((uint32_t)((c - b.ustart) / kWalkSeg), nseg - 1);
      const uint64_t start = lane == k0 ? c : lane > k0 && lane < nseg ? cj : kNone;
      const uint64_t lim = lane + 1 < nseg ? b.ustart + (uint64_t)(lane + 1) * kWalkSeg : bend;
      PlausWalk w{false, kNone, 0};
      if (start != kNone) {
        uint16_t* row = s_list[lane];
        w = walk_plausible(E, start, lim, bend, [&](uint32_t m, uint64_t q) {
          if (m < kSegListCap) row[m] = (uint16_t)(q - b.ustart);
        });
      }
      __syncthreads();
      // ---- stitch
      uint64_t cur = c;
      bool ok = true, looked = false;
      while (cur < bend) {
        const uint32_t k = min((uint32_t)((cur - b.ustart) / kWalkSeg), nseg - 1);
        const uint64_t klim = k + 1 < nseg ? b.ustart + (uint64_t)(k + 1) * kWalkSeg : bend;
        uint32_t pn;
        if (rfl_u64(shfl_u64(start, k)) == cur) {  // walker k is on the chain
          ok = rfl((uint32_t)__shfl((int)w.valid, (int)k, 64)) != 0;
          pn = rfl((uint32_t)__shfl((int)w.n, (int)k, 64));
          if (ok) {
            for (uint32_t t = lane; t < min(pn, kSegListCap); t += 64)
              if (n + t < kListCap) L[n + t] = s_list[k][t];
            cur = rfl_u64(shfl_u64(w.exitq, k));
            // (a row too short: only in a block above kMaxIsize, which locate refuses; the count path then)
            if (pn > kSegListCap && lane == 0) atomicOr(overflow, 1u);
          }
        } else {  // off it (or no start in its window): the wave walks on through segment k
          const PlausWalk s = walk_plausible(E, cur, klim, bend, [&](uint32_t m, uint64_t q) {
            if (lane == 0 && n + m < kListCap) L[n + m] = (uint16_t)(q - b.ustart);
          });
          ok = rfl((uint32_t)s.valid) != 0;
          pn = rfl(s.n);
          cur = rfl_u64(s.exitq);
        }
        if (!ok) break;
        n += pn;
        looked = klim == bend;  // that piece walked the lookahead
      }
      if (ok && !looked) ok = rfl((uint32_t)plausible_to_block_end(E, cur, bend)) != 0;
      if (ok) {
        g = c;
        x = cur;
        plaus_list = true;
      } else {
        g = kRetry;  // later candidates: k_rec_search (wave per block)
        n = 0;
      }
    }
  }
  if (lane == 0) {
    if (n > kListCap) atomicOr(overflow, 1u);
    cand[i] = c;
    g_out[i] = g;
    x_out[i] = x;
    wcnt[i] = n | (plaus_list ? kListPlausible : 0u);
  }
}

// Blocks whose first candidate failed (k_rec_walk: g == kRetry): one wave
// per block tries the later candidates in order (64 positions per step, a
// wave-uniform walk per candidate), as BAMSplitGuesser tries candidate after
// candidate; the valid one's records are listed by lane 0.
template <int MODE>
__global__ __launch_bounds__(64) void k_rec_search(ChainEnv E, const uint64_t* __restrict__ cand,
                                                   uint64_t* __restrict__ g_out, uint64_t* __restrict__ x_out,
                                                   uint32_t* __restrict__ wcnt, uint16_t* __restrict__ list,
                                                   uint32_t* __restrict__ overflow, uint32_t* __restrict__ searched) {
  const uint32_t i = blockIdx.x;
  if (g_out[i] != kRetry) return;
  const uint32_t lane = lane_id();
  if (lane == 0) atomicAdd(searched, 1u);  // (hbam_chain_counters)
  const BlockInfo b = E.blocks[E.k0 + i];
  const uint64_t bend = b.ustart + b.isize;
  wave_pull_block(E, b.ustart, bend, overflow);  // the walks below are dependent-load chains
  uint64_t g = kNone;
  for (uint64_t c0 = cand[i] + 1; c0 < bend && g == kNone; c0 += 64) {
    const uint64_t p = c0 + lane;
    const bool pre = p < bend && cand_prefilter(E, p);
    uint64_t m = __ballot(pre) ? __ballot(pre && plausible2(E, p)) : 0ull;
    while (m) {
      const uint64_t c = c0 + (uint64_t)(__ffsll((long long)m) - 1);
      m &= m - 1;
      if (plausible_to_block_end(E, c, bend)) {
        g = c;
        break;
      }
    }
  }
  if (lane == 0) {
    // (every record of a plausible chain has a block_size that can be read
    // and is >= 32: the walk by block_size leaves the block where it did)
    uint32_t n = 0;
    uint64_t x = kNone;
    if (g != kNone) {
      n = walk_entry<MODE>(E, g, b, list + (uint64_t)i * kListCap, &x);
      if (n > kListCap) atomicOr(overflow, 1u);
    }
    g_out[i] = g;
    x_out[i] = x;
    wcnt[i] = n | (g != kNone ? kListPlausible : 0u);
  }
}

// Parallel link check (in = exclusive max-scan of the guess exits).  Entries
// where the chain enters a block; a block whose walk does not start there is
// re-walked from it (force = entry), a stray walk in a pass-through block is
// dropped (force = kForceEmpty).  A chain that breaks before a block is a
// hard violation (serial link).
__global__ void k_rec_linkfix(ChainEnv E, const uint64_t* __restrict__ g, const uint64_t* __restrict__ x,
                              const uint64_t* __restrict__ in_scan, uint64_t* __restrict__ entry,
                              uint64_t* __restrict__ force, uint32_t* __restrict__ counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nb = E.k1 - E.k0;
  if (i >= nb) return;
  if (i == 0) {
    entry[0] = E.p0;
    const BlockInfo b = E.blocks[E.k0];
    if (x[0] < b.ustart + b.isize) atomicAdd(&counters[0], 1u);  // chain stops in the first block
    return;
  }
  const BlockInfo b = E.blocks[E.k0 + i];
  const uint64_t bend = b.ustart + b.isize;
  const uint64_t in = in_scan[i];
  const uint64_t gi = g[i];
  uint64_t e = kNone;
  if (in >= E.q_end) {
    e = kNone;
  } else if (in >= bend || b.isize == 0) {
    if (gi != kNone && x[i] > in) {  // a stray walk would corrupt later in[]
      force[i] = kForceEmpty;
      atomicAdd(&counters[1], 1u);
      atomicAdd(&counters[kChainCtrDropped], 1u);
    }
  } else if (in < b.ustart) {
    atomicAdd(&counters[0], 1u);  // a block before stopped inside itself
  } else {
    e = in;
    if (gi != in) {
      force[i] = in;
      atomicAdd(&counters[1], 1u);
      atomicAdd(&counters[kChainCtrRewalked], 1u);
    }
  }
  entry[i] = e;
}

// force[] off the serial link's entry[]
__global__ void k_force_from_entry(const uint64_t* __restrict__ g, const uint64_t* __restrict__ entry, uint32_t nb,
                                   uint64_t* __restrict__ force) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const uint64_t e = entry[i], gi = g[i];
  force[i] = e == gi ? kNone : (e == kNone ? kForceEmpty : e);
}

// The reader / indexer rules for the record at q (one lane), stated here
// once for the list path (k_rec_check_out) and the count path (k_rec_count):
// *stop = the block's count ends at this record (*counted: the record itself
// counts), *s = its status (kOk: a clean stop -- outside the span, EOF at a
// dead position or at the end of the stream --, or with *nd set bytes still
// to inflate), *nd = the furthest byte the record needs inflated, *long_cigar
// = its cigar was left to a second pass (record_invalid_wave).
// first: the reader's first record follows a seek (no EOF test at q);
// light: the record passed plausible() on fully inflated data, which covers
// every rule that reads it.
template <int MODE>
__device__ __forceinline__ void check_listed_h(const ChainEnv& E, uint64_t q, uint64_t lim, bool first, bool light,
                                               bool* stop, bool* counted, int* s, uint64_t* nd, bool* long_cigar,
                                               const RecHead& h) {
  const uint64_t avail = E.e_true - q;
  if (q >= lim) {
    *stop = true;  // outside the span
  } else if (light && !dead_near(E, q)) {
    // all rules pass without reading the record
  } else if (MODE == kReader) {
    if (!first && is_dead(E, q)) {
      *stop = true;  // readInt at an exhausted block + empty block: EOF
    } else if (avail < 4) {
      *stop = true;
    } else if (q + 4 > E.e_inf) {
      *stop = true;
      *nd = q + 4;
    } else {
      const int32_t bs = (int32_t)h.at(0);
      if (bs < 32) {
        *stop = true;
        *s = kErrFormat;
      } else if (dead_in_record(E, q, bs) || avail - 4 < (uint64_t)bs) {
        *stop = true;
        *s = kErrTrunc;
      } else if (q + 4 + (uint64_t)bs > E.e_inf) {
        *stop = true;
        *nd = q + 4 + (uint64_t)bs;
      } else {
        const int32_t ref = (int32_t)h.at(1), nref = (int32_t)h.at(6);
        if (ref < -1 || ref >= E.n_ref || nref < -1 || nref >= E.n_ref) {
          *stop = true;
          *s = kErrArg;
        } else if (E.validate && record_invalid_h(E, q, bs, E.validate == 2, long_cigar, h)) {
          *stop = true;
          *s = kErrFormat;
        }
      }
    }
  } else {
    if (is_dead(E, q)) {
      *stop = true;
    } else if (avail < 4) {
      *stop = true;
      if (avail > 0) *s = kErrIO;  // "less than 4 bytes long"
    } else if (q + 4 > E.e_inf) {
      *stop = true;
      *nd = q + 4;
    } else {
      const int32_t bs = (int32_t)h.at(0);
      if (bs > 0 && ((uint64_t)bs > avail - 4 || is_dead(E, q + 4))) {
        *stop = true;
        *counted = true;
        *s = kErrIO;  // "Skip failed"
      }
    }
  }
}

// The count path (a list overflowed: indexer-mode records shorter than 36
// bytes): count and validate the records of each block by walking it, one
// thread per block, check_listed_h per record.
//   cnt[i], err[i] = status code (a stop that is no error: kStopClean),
//   *need = furthest byte the span needs inflated (atomicMax).
template <int MODE>
__global__ void k_rec_count(ChainEnv E, const uint64_t* __restrict__ entry, uint32_t* __restrict__ cnt,
                            int32_t* __restrict__ err, unsigned long long* __restrict__ need) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t nb = E.k1 - E.k0;
  if (i >= nb) return;
  uint32_t n = 0;
  int st = kOk;
  const uint64_t e = entry[i];
  if (e != kNone) {
    const BlockInfo b = E.blocks[E.k0 + i];
    const uint64_t lim = min(b.ustart + b.isize, E.q_end);
    uint64_t q = e;
    bool first = (MODE == kReader) && (e == E.p0);  // reader: first record follows a seek
    while (q < lim) {  // (the walk leaves the block: no head is loaded past its end)
      bool stop = false, counted = false, long_cigar = false;
      int s = kOk;
      uint64_t nd = 0;
      const RecHead h = load_head(E.u, q);
      check_listed_h<MODE>(E, q, lim, first, false, &stop, &counted, &s, &nd, &long_cigar, h);
      first = false;
      const int32_t bs = (int32_t)h.at(0);
      // a cigar above kWaveCigarOps operators: one lane's pass takes any length
      if (long_cigar && record_invalid_h(E, q, bs, E.validate == 2, nullptr, h)) {
        stop = true;
        s = kErrFormat;
      }
      if (stop) {
        n += counted;
        if (nd) atomicMax(need, (unsigned long long)nd);
        else st = s == kOk ? kStopClean : s;
        break;
      }
      ++n;
      q += 4 + (uint64_t)(MODE == kReader ? bs : (bs > 0 ? bs : 0));
    }
  }
  cnt[i] = n;
  err[i] = st;
}

// Record check and output in one pass (the list path of decode_span_pos):
// the record rules, the long-cigar validation and the output, one wave per
// block, so a block's records are read from HBM once after inflate and
// written out while they are in L2.  A block writes its records at base[i],
// the exclusive scan of the lists' counts: the true offsets for every block
// up to the first one that stops early, since every block before it keeps
// its whole list.  A stop ends the reader's iteration (a failure, EOF at an
// empty block, the end of the stream or of the span) and the indexer's, so
// the span's records are exactly those up to the first stop, and what later
// blocks write lies past them.  The launch reports:
//   bad[0]   min over blocks that stop early or fail of (i << 40 | base[i] +
//            count): the first such block and the records up to its stop
//   flags[0] the first failing block (its status is the span's when it is
//            the first stop)
//   cnt[] / err[] per block, need = the bytes a stopped record needs past
//            the inflated range.
constexpr int kBadShift = 40;

// (4 / 6 / 8 waves per SIMD: 1.116 / 1.065 / 1.052 ms per C2 pass,
// profiles/r06_late/variants_check_out_waves.log)
template <int MODE, bool DECODE>
__global__ __launch_bounds__(64, 6) void k_rec_check_out(ChainEnv E, const uint64_t* __restrict__ entry,
                                                         const uint32_t* __restrict__ wcnt,
                                                         const uint16_t* __restrict__ list,
                                                         const uint64_t* __restrict__ base, uint32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ err,
                                                         unsigned long long* __restrict__ need,
                                                         unsigned long long* __restrict__ bad,
                                                         uint32_t* __restrict__ flags, uint64_t* __restrict__ rec_pos,
                                                         uint64_t* __restrict__ rec_voff, Columns col, uint64_t cap) {
  const uint32_t lane = lane_id();
  const uint32_t i = blockIdx.x;
  const uint64_t e = entry[i];
  const BlockInfo b = E.blocks[E.k0 + i];
  const uint16_t* __restrict__ L = list + (uint64_t)i * kListCap;
  const uint64_t lim = min(b.ustart + b.isize, E.q_end);
  const uint32_t wc = wcnt[i];
  const uint32_t listed = e == kNone ? 0u : min(wc & kListCountMask, kListCap);
  // (check_listed_h's light) a plausible() list on fully inflated data
  // already satisfies every rule that reads the record
  const bool light = (wc & kListPlausible) && E.e_inf == E.e_true && (MODE != kReader || E.validate == 0);
  const uint64_t o0 = base[i];
  uint32_t count = listed;
  int st = kOk;
  uint64_t nd = 0;
  // 64 records at a time: check them, validate their long cigars, and write
  // the ones before the first stop while their lines are still in L1/L2 (a
  // whole block checked before any output re-fetched every line: 5.9 GB per
  // C2 pass)
  for (uint32_t r0 = 0; r0 < listed; r0 += 64) {
    const uint32_t r = r0 + lane;
    const uint64_t q = r < listed ? b.ustart + L[r] : 0;
    bool stop = false, counted = false, long_cigar = false;
    int s = kOk;
    uint64_t x = 0;
    // the record's head is loaded once for the checks and the output (three
    // passes over it re-fetched its lines from HBM: 5.3 GB per C2 pass)
    RecHead h{};
    if (r < listed) {
      h = load_head(E.u, q);
      check_listed_h<MODE>(E, q, lim, r == 0 && q == E.p0, light, &stop, &counted, &s, &x, &long_cigar, h);
    }
    uint32_t m = min(64u, listed - r0);  // records of this chunk that stand
    const uint64_t sm = __ballot(stop);
    bool halt = sm != 0;  // the block's count ends in this chunk
    if (sm) {
      const uint32_t f = (uint32_t)__ffsll((long long)sm) - 1;
      m = f + (uint32_t)__shfl((int)counted, (int)f, 64);
      st = __shfl(s, (int)f, 64);
      nd = shfl_u64(x, f);
    }
    if (MODE == kReader) {
      // cigars longer than kWaveCigarOps before the stop, a wave each in order
      // (record_invalid_wave): the first invalid one becomes the stop
      const bool lg = lane < m && long_cigar;
      for (uint64_t wm = __ballot(lg); wm; wm &= wm - 1) {
        const uint32_t src = (uint32_t)__ffsll((long long)wm) - 1;
        const uint64_t qq = shfl_u64(q, src);
        if (record_invalid_wave(E, qq, (int32_t)ldu32(E.u, qq), E.validate == 2)) {
          m = src;
          st = kErrFormat;
          nd = 0;
          halt = true;
          break;
        }
      }
    }
    if (lane < m) {
      const uint64_t o = o0 + r;
      if (o < cap) {  // (sized from the lists' counts: always)
        rec_pos[o] = q;
        rec_voff[o] = (b.coff << 16) | (q - b.ustart);
        if (DECODE) decode_record_h(E.u, q, o, col, h);
      }
    }
    if (halt) {
      count = r0 + m;
      break;
    }
  }
  if (lane == 0) {
    if (nd) atomicMax(need, (unsigned long long)nd);
    cnt[i] = count;
    err[i] = st;
    if (count < listed || st != kOk)
      atomicMin(bad, ((unsigned long long)i << kBadShift) | (unsigned long long)(o0 + count));
    if (st != kOk) atomicMin(&flags[0], i);
    // (no per-block atomic on a shared word here: 52 K of them on one address
    // serialize across the XCDs; k_records_after answers for the rare stop)
  }
}

// *flag = 1 when a block after block k has records (a span cut at an early
// stop dropped them: a diagnostic, hbam_pipeline_counters)
__global__ void k_records_after(const uint32_t* __restrict__ cnt, uint32_t nb, uint32_t k, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > k && i < nb && cnt[i]) *flag = 1u;
}
hipError_t launch_records_after(const uint32_t* cnt, uint32_t nb, uint32_t k, uint32_t* flag, hipStream_t s) {
  hipLaunchKernelGGL(k_records_after, dim3((nb + 255) / 256), dim3(256), 0, s, cnt, nb, k, flag);
  return hipGetLastError();
}

// first block (index) whose status is non-zero -> *first (atomicMin), status -> code[]
__global__ void k_first_error_hout(const HuffOut* __restrict__ hout, uint32_t b0, uint32_t nb,
                                   uint32_t* __restrict__ first) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && hout[b0 + i].status != kOk) atomicMin(first, i);
}
__global__ void k_first_error_i32(const int32_t* __restrict__ err, uint32_t nb, uint32_t* __restrict__ first) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && err[i] != kOk) atomicMin(first, i);
}
// zero the counts of blocks after `cut` (the first failing block)
__global__ void k_truncate_counts(uint32_t* __restrict__ cnt, uint32_t nb, const uint32_t* __restrict__ cut) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && i > *cut) cnt[i] = 0;
}

// cnt[i] = the records block i's list holds (0 off the chain): the
// optimistic output counts k_rec_check_out's offsets are scanned from
__global__ void k_list_counts(const uint64_t* __restrict__ entry, const uint32_t* __restrict__ wcnt, uint32_t nb,
                              uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) cnt[i] = entry[i] != kNone ? min(wcnt[i] & kListCountMask, kListCap) : 0u;
}

// ---- host launch wrappers (hbam_launch.h)
static ChainEnv chain_env(const ChainArgs& a) {
  ChainEnv E;
  E.u = a.u;
  E.blocks = a.blocks;
  E.e_inf = a.e_inf;
  E.e_true = a.e_true;
  E.p0 = a.p0;
  E.q_end = a.q_end;
  E.dead = a.dead;
  E.ndead = a.ndead;
  E.n_ref = a.n_ref;
  E.k0 = a.k0;
  E.k1 = a.k1;
  E.validate = a.validate;
  E.ref_len = a.ref_len;
  return E;
}

// f(m) with the run-time mode as the compile-time constant decltype(m)::value
template <typename F>
static void with_mode(int mode, F f) {
  if (mode == kReader) f(std::integral_constant<int, kReader>());
  else f(std::integral_constant<int, kIndexer>());
}

hipError_t launch_chain(const ChainArgs& a, int mode, int stage, hipStream_t s) {
  const ChainEnv E = chain_env(a);
  const uint32_t nb = a.k1 - a.k0;
  if (nb == 0) return hipSuccess;
  const unsigned tb = 64, gb = (nb + tb - 1) / tb;
  switch (stage) {
    case kStageSerialLink:
      with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(k_rec_link<decltype(m)::value>, dim3(1), dim3(256), 0, s, E, a.g, a.x, a.entry, a.summary);
      });
      break;
    case kStageCount:
      with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(k_rec_count<decltype(m)::value>, dim3(gb), dim3(tb), 0, s, E, a.entry, a.cnt, a.err, a.need);
      });
      break;
    case kStageEmit:
      with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(k_rec_emit<decltype(m)::value>, dim3(gb), dim3(tb), 0, s, E, a.entry, a.cnt, a.base,
                           a.rec_pos, a.rec_voff);
      });
      break;
    case kStageWalk:      // candidates + walks, a wave per block
    case kStageWalkLane:  // the same by k_rec_cand + a lane per block (HBAM_CHAIN_WALK=lane)
      with_mode(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (stage == kStageWalk) {
          hipLaunchKernelGGL(k_rec_walk_wave<M>, dim3(nb), dim3(64), 0, s, E, a.cand, a.g, a.x, a.wcnt, a.list,
                             a.counters + 2);
        } else {
          hipLaunchKernelGGL(k_rec_cand<M>, dim3(nb), dim3(64), 0, s, E, a.cand);
          hipLaunchKernelGGL(k_rec_walk<M>, dim3((nb + 255) / 256), dim3(256), 0, s, E, a.cand, nullptr, a.g, a.x,
                             a.wcnt, a.list, a.counters + 2, false);
        }
        hipLaunchKernelGGL(k_rec_search<M>, dim3(nb), dim3(64), 0, s, E, a.cand, a.g, a.x, a.wcnt, a.list,
                           a.counters + 2, a.counters + kChainCtrSearched);
      });
      break;
    case kStageLinkCheck: {  // y, exclusive max-scan, check with re-walk requests
      hipError_t e = hipMemsetAsync(a.force, 0xff, (size_t)nb * 8, s);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_rec_link_y, dim3(gb), dim3(tb), 0, s, a.g, a.x, nb, a.x2);
      size_t sb = a.scan_bytes;
      e = hipcub::DeviceScan::ExclusiveScan(a.scan_tmp, sb, a.x2, a.base, hipcub::Max(), (uint64_t)0, (int)nb, s);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(k_rec_linkfix, dim3(gb), dim3(tb), 0, s, E, a.g, a.x, a.base, a.entry, a.force, a.counters);
      break;
    }
    case kStageRewalk:       // re-walk the requested blocks (entries validated)
    case kStageRewalkAll: {  // force off the serial link's (exact) entry[], then re-walk
      const bool validate = stage == kStageRewalk;
      if (stage == kStageRewalkAll) hipLaunchKernelGGL(k_force_from_entry, dim3(gb), dim3(tb), 0, s, a.g, a.entry, nb, a.force);
      with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(k_rec_walk<decltype(m)::value>, dim3((nb + 255) / 256), dim3(256), 0, s, E, a.cand, a.force,
                           a.g, a.x, a.wcnt, a.list, a.counters + 2, validate);
      });
      break;
    }
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_list_counts(const ChainArgs& a, hipStream_t s) {
  const uint32_t nb = a.k1 - a.k0;
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_list_counts, dim3((nb + 255) / 256), dim3(256), 0, s, a.entry, a.wcnt, nb, a.cnt);
  return hipGetLastError();
}

hipError_t launch_rec_check_out(const ChainArgs& a, int mode, bool decode, const Columns& col, uint64_t cap,
                                hipStream_t s) {
  static_assert(kBadShift == kFusedBadShift, "hbam_launch.h kFusedBadShift");
  const ChainEnv E = chain_env(a);
  const uint32_t nb = a.k1 - a.k0;
  if (nb == 0) return hipSuccess;
  unsigned long long* need = a.need;
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(a.fuse_bad);
#define HBAM_CO(M, D)                                                                                            \
  hipLaunchKernelGGL((k_rec_check_out<M, D>), dim3(nb), dim3(64), 0, s, E, a.entry, a.wcnt, a.list, a.base, a.cnt, \
                     a.err, need, bad, a.fuse_flags, a.rec_pos, a.rec_voff, col, cap)
  if (mode == kReader && decode) HBAM_CO(kReader, true);
  else if (mode == kReader) HBAM_CO(kReader, false);
  else HBAM_CO(kIndexer, false);
#undef HBAM_CO
  return hipGetLastError();
}

hipError_t link_scan_bytes(uint32_t nb, size_t* bytes) {
  uint64_t* p = nullptr;
  return hipcub::DeviceScan::ExclusiveScan(nullptr, *bytes, p, p, hipcub::Max(), (uint64_t)0, (int)nb, (hipStream_t)0);
}

hipError_t launch_first_error_hout(const HuffOut* hout, uint32_t b0, uint32_t nb, uint32_t* first, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_first_error_hout, dim3((nb + 255) / 256), dim3(256), 0, s, hout, b0, nb, first);
  return hipGetLastError();
}
hipError_t launch_first_error_i32(const int32_t* err, uint32_t nb, uint32_t* first, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_first_error_i32, dim3((nb + 255) / 256), dim3(256), 0, s, err, nb, first);
  return hipGetLastError();
}
hipError_t launch_truncate_counts(uint32_t* cnt, uint32_t nb, const uint32_t* cut, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_truncate_counts, dim3((nb + 255) / 256), dim3(256), 0, s, cnt, nb, cut);
  return hipGetLastError();
}

}  // namespace hbam
