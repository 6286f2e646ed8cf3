// hbam_kernels.hip -- gfx950 kernels of inflate phase A: DEFLATE symbols -> LZ77 tokens.
// (What is left of the former all-stages file: the other stages are in hbam_locate,
// hbam_inflate_lz77, hbam_chain and hbam_records.)
//
//   huff_tables    one wave per block: a DEFLATE block's header + Huffman
//        tables, built ahead of the decode at high occupancy (in rounds: the
//        first block of each BGZF block, then the one the decode stopped at)
//   inflate_huff   (phase A) one 256-thread workgroup per BGZF block: the
//        symbol stream -> LZ77 tokens by 256 speculative slices, a sync pass
//        and an emit pass; the compressed block and the tables sit in LDS.
//        ([htsjdk] BlockGunzipper.unzipBlock -> java.util.zip.Inflater)
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "hbam_dev_util.h"
#include "hbam_device.h"
#include "hbam_launch.h"

namespace hbam {

// Inflate phase A: Huffman decode, one 256-thread workgroup per BGZF block
// The block's compressed bytes are staged in LDS (dynamic shared memory sized
// per launch to the largest block of the chunk) by coalesced 16 B loads; the
// Huffman tables (~11 KiB) sit next to them.  Wave 0 parses block headers,
// decodes code lengths and builds the tables (wave-uniform scalar code, the
// other waves wait at a barrier).  A DEFLATE block's symbol stream is then
// decoded by all 256 lanes at once: lane l starts at a guessed bit position
// B0 + l*S and decodes its slice up to the first symbol boundary at or past
// the next slice (its "exit").  Huffman streams self-synchronise, so a lane
// that started off a boundary soon falls onto the true path.  A sync pass
// re-decodes each slice from its predecessor's exit only until it lands on one
// of the first kMergePts boundaries its speculative walk recorded (the walks
// share every symbol from there on), so it costs a few symbols per lane.  A
// last pass re-decodes each slice from its true start and writes tokens at
// workgroup-scanned offsets, four at a time (16 B stores).
//
// Semantics follow zlib's inflate() as driven by [htsjdk] BlockGunzipper
// (one call, all input, ISIZE bytes of output space):
//   * a field whose bits are not all inside the block's CDATA stops decoding
//     ("Did not inflate expected amount" = kErrFormat unless output is full);
//   * invalid codes / distances -> DataFormatException (kErrIO);
//   * once output is exactly full at a symbol boundary, zlib still decodes the
//     next litlen code (and a whole length/distance pair, or the next block
//     header after an end-of-block) before it notices there is no room: those
//     can still raise errors -> the scalar lookahead below.
//
// Table entries (u32):
//   litlen  [15:0] payload  [20:16] bits to consume  [25:24] literal count  [28:26] kind
//           kind 0 LIT : payload = 1 or 2 literal bytes; (e & 0x0300ffff) IS the token
//           kind 1 LEN : payload [8:0] base (3..258), [12:9] extra bits
//           kind 2 EOB, 3 LONG (payload = sub-table base), 4 BAD, 5 SLOW (canonical decode)
//   dist    [14:0] base  [20:16] bits  [24:21] extra  [28:26] kind (0 ok, 3 LONG, 4 BAD, 5 SLOW)
//   codes   [15:0] symbol [20:16] bits (code-length alphabet, root 7: always direct)
// Codes longer than the root index a fixed-size sub-table by the next bits;
// sub-table entries carry the full code length.
// Tokens (u32): literal  bit31=0, [25:24] count (1..2), [15:0] bytes
//               match    bit31=1, [30:16] dist-1, [15:0] length
#ifndef HBAM_HUFF_THREADS
#define HBAM_HUFF_THREADS 256
#endif
constexpr int kHuffThreads = HBAM_HUFF_THREADS;  // lanes per DEFLATE block (a multiple of 64)
constexpr int kHuffWaves = kHuffThreads / 64;
// Phase A runs as two kernels per round.  The lean instance (k_inflate_huff)
// decodes one DEFLATE block per workgroup from prebuilt tables, with only the
// round's window of compressed bits staged in LDS, at kLeanWavesPerSimd waves
// per SIMD (a round after the first: 128 lanes wide, LeanGeom below);
// whatever it does not handle goes to the fallback kernel
// (k_huff_fallback), the full body (huff_block) at 4 waves per SIMD, which
// reads the block from an LDS copy (staged) when the tables + the block fit
// kHuffStageMaxLds, else straight from HBM/L2 (C4: 7.4 -> 3.9 ms; C2: staged
// 7.6 vs 8.0 ms).
// HBAM_HUFF_STAGE_MAX / HBAM_HUFF_WAVES_PER_SIMD: the lean instance's LDS per
// workgroup and its waves per SIMD (A/B knobs; 40 KB and 4 = the fallback's
// own, fixed, geometry).
#ifndef HBAM_HUFF_STAGE_MAX
#define HBAM_HUFF_STAGE_MAX (32 * 1024)
#endif
constexpr uint32_t kLeanLds = HBAM_HUFF_STAGE_MAX;
constexpr uint32_t kHuffStageMaxLds = 40 * 1024;

// Wave-local ordering of LDS traffic (code run by one wave only).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
constexpr int kLitRoot = 10;
constexpr int kDistRoot = 9;
// Variable-size sub-tables (as zlib's inflate_table): the root entry of a
// long-code prefix holds the sub-table base and its index width (= the longest
// code under that prefix - root).  A complete litlen code with a 10-bit root
// needs at most 310 sub entries (zlib ENOUGH_LENS 1334 - 1024), the distance
// code with a 9-bit root at most 80: the largest sum of 2^(longest code under
// a prefix - root) over every complete code of up to 30 symbols and 15 bits,
// by enumeration of their length distributions (zlib's ENOUGH_DISTS 592 is
// the figure for its 6-bit root and says nothing here); case T2 of
// tests/deflate_cases.py reaches 306 and 80.  build_table
// accepts complete codes only (and the one-code case).  Prefixes that would
// not fit fall back to K_SLOW (canonical decode), which valid streams never
// reach.  The caps size the table image every block writes and phase A reads
// back, and the LDS that bounds k_huff_tables' resident waves.
constexpr int kLitSubCap = 320;
constexpr int kDistSubCap = 128;
enum : uint32_t { K_LIT = 0, K_LEN = 1, K_EOB = 2, K_LONG = 3, K_BAD = 4, K_SLOW = 5 };
constexpr uint32_t kBadEntry = K_BAD << 26;
constexpr uint32_t kLongTag = 0xF0000000u;  // build-time mark: kLongTag | (max len - root)
constexpr uint32_t kKindLit = 1u << 26;  // e < kKindLit  <=>  literal entry
// a root entry that points to a sub-table (kind K_LONG) also carries bit 31,
// so the decode loop tests it with one signed compare
constexpr uint32_t kLongEntry = 0x80000000u | (K_LONG << 26);
__device__ __forceinline__ bool is_long(uint32_t e) { return (int32_t)e < 0; }

__constant__ uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                      31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2,
                                      2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,
                                       33,  49,  65,  97,  129, 193,  257,  385,  513,  769,
                                       1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2,  3,  3,  4,  4,  5,  5,  6,
                                       6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// LDS tables of one DEFLATE block.  The leading kTableImage bytes (lit ..
// sort_dist) are everything the symbol decode reads; k_huff_tables writes
// exactly that image to HBM and k_inflate_huff copies it back.
struct HuffLds {
  uint32_t lit[1 << kLitRoot];                      // litlen root table (with literal pairs)
  uint32_t litsub[kLitSubCap];                      // litlen sub-tables
  uint32_t dist[1 << kDistRoot];                    // distance root table (also the code-length table)
  uint32_t distsub[kDistSubCap];                    // distance sub-tables
  uint32_t cnt_lit[16];
  uint32_t cnt_dist[16];
  uint16_t sort_lit[288];
  uint16_t sort_dist[32];
  // ---- build scratch
  uint32_t offs[16];
  uint32_t firstc[16];
  uint32_t base[16];
  uint32_t bt_status;
  uint16_t rev_of[320];
  uint8_t lens[320];
  uint8_t cl_lens[20];
};
constexpr uint32_t kTableImage = offsetof(HuffLds, offs);
// dyn_header_par's per-lane symbol scratch (ClLds) may alias lit[]: the
// litlen table is built only after the code lengths are decoded
static_assert(kTableImage % 16 == 0, "table image is copied in 16 B units");
static_assert(kTableImage == kHuffTableImage, "hbam_device.h kHuffTableImage must match HuffLds");

// A code of length l fills 2^(root - l) root entries: codes with l <= root -
// kFillWave are filled by the whole wave together, longer ones by their lane.
#ifndef HBAM_FILL_WAVE
#define HBAM_FILL_WAVE 6
#endif
constexpr int kFillWave = HBAM_FILL_WAVE;

// mode 0 litlen, 1 distance, 2 code-length codes
__device__ __forceinline__ uint32_t make_entry(int mode, uint32_t s, uint32_t len) {
  if (mode == 0) {
    if (s < 256) return (len << 16) | (1u << 24) | s;
    if (s == 256) return (len << 16) | (K_EOB << 26);
    if (s < 286) {
      const uint32_t i = s - 257;
      return (len << 16) | (K_LEN << 26) | ((uint32_t)kLenExtra[i] << 9) | (uint32_t)kLenBase[i];
    }
    return (len << 16) | kBadEntry;
  }
  if (mode == 1) {
    if (s < 30) return (len << 16) | ((uint32_t)kDistExtra[s] << 21) | (uint32_t)kDistBase[s];
    return (len << 16) | kBadEntry;
  }
  return (len << 16) | s;
}

// Canonical Huffman table build by ONE wave (wave 0 of the workgroup; the
// other waves wait at the caller's barrier).  Validity follows
// zlib inflate_table: over-subscribed -> error; incomplete -> error unless
// the only code has length 1 (LENS/DISTS); no codes -> all-invalid table
// (DISTS) or error (CODES).  Returns 0 on success.  Per-length state lives in
// LDS (not in unrolled SGPR arrays) to keep the decode loop's registers free.
// Callers must rfl() the result: a call's return value is divergent to the
// compiler, and one divergent branch at the call site turns the whole decode
// state into VGPRs with exec-masked control flow.
__device__ __attribute__((noinline)) int build_table(HuffLds& L, const uint8_t* lens, int nsym, int root, int mode,
                                                     uint32_t* tab, uint32_t* cnt, uint16_t* sorted, uint32_t* sub,
                                                     int subcap) {
  const uint32_t lane = lane_id();
  // counts per code length by ballots, then the Kraft check, the canonical
  // offsets and first codes as wave-uniform arithmetic (LDS atomics and a
  // one-lane loop over LDS cost ~3 K cycles per table)
  uint32_t cntv[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) cntv[q] = 0;
  for (int c0 = 0; c0 < nsym; c0 += 64) {
    const int s = c0 + (int)lane;
    const uint32_t l = s < nsym ? lens[s] : 0;
#pragma unroll
    for (uint32_t q = 1; q < 16; ++q) cntv[q] += (uint32_t)__popcll(__ballot(l == q));
  }
  int left = 1, maxl = 0;
  bool over = false;
  uint32_t o = 0, code = 0, prev = 0, my_cnt = 0, my_off = 0, my_first = 0;
#pragma unroll
  for (uint32_t l = 1; l < 16; ++l) {
    const uint32_t c = cntv[l];
    left = (left << 1) - (int)c;
    maxl = c ? (int)l : maxl;
    over = over || left < 0;
    code = (code + prev) << 1;
    my_cnt = lane == l ? c : my_cnt;
    my_off = lane == l ? o : my_off;
    my_first = lane == l ? code : my_first;
    o += c;
    prev = c;
  }
  if (lane < 16) {
    cnt[lane] = my_cnt;
    L.offs[lane] = my_off;
    L.firstc[lane] = my_first;
  }
  uint32_t st = 0;
  if (over) st = 1;
  else if (maxl == 0) st = mode == 2 ? 1 : 2;
  else if (left > 0 && (mode == 2 || maxl != 1)) st = 1;
  for (int i = lane; i < (1 << root); i += 64) tab[i] = kBadEntry;
  wave_sync();
  if (st == 1) return 1;
  if (st == 2) return 0;  // no codes: all-invalid table
  const uint32_t rmask = (1u << root) - 1;
  const uint64_t ltmask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  bool any_long = false;
  // next canonical rank per code length: wave-uniform, kept in registers (an
  // LDS counter costs a dependent LDS round trip per length and group)
  uint32_t basev[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) basev[q] = 0;
  for (int c0 = 0; c0 < nsym; c0 += 64) {
    const int s = c0 + (int)lane;
    const uint32_t l = s < nsym ? lens[s] : 0;
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t q = 1; q < 16; ++q) {
      const uint64_t m = __ballot(l == q);
      rank = l == q ? basev[q] + (uint32_t)__popcll(m & ltmask) : rank;
      basev[q] += (uint32_t)__popcll(m);
    }
    uint32_t rev = 0, e = 0;
    if (l) {
      sorted[L.offs[l] + rank] = (uint16_t)s;
      const uint32_t code = L.firstc[l] + rank;
      rev = __brev(code) >> (32 - l);
      L.rev_of[s] = (uint16_t)rev;
      if ((int)l <= root) {
        e = make_entry(mode, (uint32_t)s, l);
        // a code that fills fewer than 64 root entries fills them itself; the
        // wave fills the wider ones together below (a lane alone took up to
        // 2^(root - l) dependent trips, and the wave waited for the longest)
        if ((int)l > root - kFillWave)
          for (uint32_t i = rev; i < (1u << root); i += (1u << l)) tab[i] = e;
      } else {
        atomicMax(&tab[rev & rmask], kLongTag | (l - (uint32_t)root));  // widest sub-table under the prefix
        any_long = true;
      }
    }
    for (uint64_t wm = __ballot(l != 0 && (int)l <= root - kFillWave); wm; wm &= wm - 1) {
      const int src = __ffsll((long long)wm) - 1;
      const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)l, src);  // src is wave-uniform
      const uint32_t wr = (uint32_t)__builtin_amdgcn_readlane((int)rev, src);
      const uint32_t we = (uint32_t)__builtin_amdgcn_readlane((int)e, src);
      for (uint32_t k = lane; k < (1u << (root - (int)wl)); k += 64) tab[wr + (k << wl)] = we;
    }
  }
  wave_sync();
  if (__ballot(any_long) == 0) return 0;
  // sub-table bases: exclusive scan of the sub-table sizes in root-index order
  uint32_t used = 0;
  for (int c0 = 0; c0 < (1 << root); c0 += 64) {
    const uint32_t i = c0 + lane;
    const uint32_t t = tab[i];
    const bool mk = t >= kLongTag;
    const uint32_t bits = t & 15u;
    const uint32_t sz = mk ? (1u << bits) : 0u;
    uint32_t inc = sz;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t v = __shfl_up(inc, d, 64);
      if (lane >= (uint32_t)d) inc += v;
    }
    const uint32_t base = used + inc - sz;
    if (mk) tab[i] = base + sz <= (uint32_t)subcap ? (kLongEntry | (bits << 16) | base) : (K_SLOW << 26);
    used += (uint32_t)__shfl(inc, 63, 64);
  }
  const uint32_t nused = min(used, (uint32_t)subcap);
  for (uint32_t i = lane; i < nused; i += 64) sub[i] = kBadEntry;
  wave_sync();
  for (int s = lane; s < nsym; s += 64) {
    const uint32_t l = lens[s];
    if ((int)l > root) {
      const uint32_t rev = L.rev_of[s];
      const uint32_t e = tab[rev & rmask];
      if (is_long(e)) {
        const uint32_t b = e & 0xffffu, sb = (e >> 16) & 15u;
        const uint32_t ent = make_entry(mode, (uint32_t)s, l);
        for (uint32_t k = rev >> root; k < (1u << sb); k += 1u << (l - root)) sub[b + k] = ent;
      }
    }
  }
  wave_sync();
  return 0;
}

// The same build with its per-length state and the code lengths in registers
// (k_huff_tables, §7 item 2 of DESIGN.md): ~25 % faster per table, but its
// ~116 VGPRs would spill k_inflate_huff, whose rare inline header path calls
// the LDS-state build_table above.
__device__ __attribute__((noinline)) int build_table_r(HuffLds& L, const uint8_t* lens, int nsym, int root, int mode,
                                                     uint32_t* tab, uint32_t* cnt, uint16_t* sorted, uint32_t* sub,
                                                     int subcap) {
  const uint32_t lane = lane_id();
  // Every symbol's code length stays in registers (nsym <= 320: 5 groups of
  // 64), so do the canonical offsets and first codes (wave-uniform, picked
  // per lane by a select chain): each LDS read on this path is a dependent
  // round trip in a wave that has nothing else to do.
  constexpr int kGroups = 5;
  const int ng = (nsym + 63) >> 6;
  uint32_t lv[kGroups];
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const int s = 64 * g + (int)lane;
    lv[g] = g < ng && s < nsym ? lens[s] : 0u;
  }
  // counts per code length by ballots, then the Kraft check, the canonical
  // offsets and first codes as wave-uniform arithmetic (LDS atomics and a
  // one-lane loop over LDS cost ~3 K cycles per table)
  uint32_t cntv[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) cntv[q] = 0;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    if (g >= ng) break;  // wave-uniform
#pragma unroll
    for (uint32_t q = 1; q < 16; ++q) cntv[q] += (uint32_t)__popcll(__ballot(lv[g] == q));
  }
  int left = 1, maxl = 0;
  bool over = false;
  uint32_t o = 0, code = 0, prev = 0, my_cnt = 0;
  uint32_t offu[16], firstu[16];
  offu[0] = firstu[0] = 0;
#pragma unroll
  for (uint32_t l = 1; l < 16; ++l) {
    const uint32_t c = cntv[l];
    left = (left << 1) - (int)c;
    maxl = c ? (int)l : maxl;
    over = over || left < 0;
    code = (code + prev) << 1;
    my_cnt = lane == l ? c : my_cnt;
    offu[l] = o;
    firstu[l] = code;
    o += c;
    prev = c;
  }
  if (lane < 16) cnt[lane] = my_cnt;
  uint32_t st = 0;
  if (over) st = 1;
  else if (maxl == 0) st = mode == 2 ? 1 : 2;
  else if (left > 0 && (mode == 2 || maxl != 1)) st = 1;
  for (int i = lane; i < (1 << root); i += 64) tab[i] = kBadEntry;
  wave_sync();
  if (st == 1) return 1;
  if (st == 2) return 0;  // no codes: all-invalid table
  const uint32_t rmask = (1u << root) - 1;
  const uint64_t ltmask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  bool any_long = false;
  // next canonical rank per code length: wave-uniform, kept in registers (an
  // LDS counter costs a dependent LDS round trip per length and group)
  uint32_t basev[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) basev[q] = 0;
  uint32_t revv[kGroups];
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    revv[g] = 0;
    if (g >= ng) break;  // wave-uniform
    const int s = 64 * g + (int)lane;
    const uint32_t l = lv[g];
    uint32_t rank = 0, off = 0, first = 0;
#pragma unroll
    for (uint32_t q = 1; q < 16; ++q) {
      const uint64_t m = __ballot(l == q);
      rank = l == q ? basev[q] + (uint32_t)__popcll(m & ltmask) : rank;
      off = l == q ? offu[q] : off;
      first = l == q ? firstu[q] : first;
      basev[q] += (uint32_t)__popcll(m);
    }
    uint32_t rev = 0, e = 0;
    if (l) {
      sorted[off + rank] = (uint16_t)s;
      rev = __brev(first + rank) >> (32 - l);
      revv[g] = rev;
      if ((int)l <= root) {
        e = make_entry(mode, (uint32_t)s, l);
        // a code that fills fewer than 64 root entries fills them itself; the
        // wave fills the wider ones together below (a lane alone took up to
        // 2^(root - l) dependent trips, and the wave waited for the longest)
        if ((int)l > root - kFillWave)
          for (uint32_t i = rev; i < (1u << root); i += (1u << l)) tab[i] = e;
      } else {
        atomicMax(&tab[rev & rmask], kLongTag | (l - (uint32_t)root));  // widest sub-table under the prefix
        any_long = true;
      }
    }
    for (uint64_t wm = __ballot(l != 0 && (int)l <= root - kFillWave); wm; wm &= wm - 1) {
      const int src = __ffsll((long long)wm) - 1;
      const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)l, src);  // src is wave-uniform
      const uint32_t wr = (uint32_t)__builtin_amdgcn_readlane((int)rev, src);
      const uint32_t we = (uint32_t)__builtin_amdgcn_readlane((int)e, src);
      for (uint32_t k = lane; k < (1u << (root - (int)wl)); k += 64) tab[wr + (k << wl)] = we;
    }
  }
  wave_sync();
  if (__ballot(any_long) == 0) {
    return 0;
  }
  // sub-table bases: exclusive sum of the sub-table sizes in root-index
  // order.  A table has a handful of long-code prefixes, so the marked
  // entries of each 64-entry chunk are walked in lane order (a 6-step
  // shuffle scan of every chunk, ds_bpermute each step, took ~12 K cycles);
  // the root entries are read all at once first
  constexpr int kChunks = (1 << kLitRoot) / 64;
  const int nch = (1 << root) >> 6;
  uint32_t tv[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; ++c) tv[c] = c < nch ? tab[64 * c + lane] : 0u;
  uint32_t used = 0;
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const uint32_t t = tv[c];  // 0 past the root table: no marks
    for (uint64_t mm = __ballot(t >= kLongTag); mm; mm &= mm - 1) {
      const int j = __ffsll((long long)mm) - 1;
      const uint32_t bits = (uint32_t)__builtin_amdgcn_readlane((int)t, j) & 15u;
      const uint32_t sz = 1u << bits;
      if ((int)lane == j)
        tab[64 * c + lane] = used + sz <= (uint32_t)subcap ? (kLongEntry | (bits << 16) | used) : (K_SLOW << 26);
      used += sz;
    }
  }
  const uint32_t nused = min(used, (uint32_t)subcap);
  for (uint32_t i = lane; i < nused; i += 64) sub[i] = kBadEntry;
  wave_sync();
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    if (g >= ng) break;  // wave-uniform
    const uint32_t l = lv[g];
    if ((int)l > root) {
      const int s = 64 * g + (int)lane;
      const uint32_t rev = revv[g];
      const uint32_t e = tab[rev & rmask];
      if (is_long(e)) {
        const uint32_t b = e & 0xffffu, sb = (e >> 16) & 15u;
        const uint32_t ent = make_entry(mode, (uint32_t)s, l);
        for (uint32_t k = rev >> root; k < (1u << sb); k += 1u << (l - root)) sub[b + k] = ent;
      }
    }
  }
  wave_sync();
  return 0;
}

// Fold two consecutive literals into one litlen entry when both codes fit in
// the 10-bit index (the common case for quality/sequence bytes).
__device__ __attribute__((noinline)) void pair_literals(HuffLds& L) {
  const uint32_t lane = lane_id();
  uint32_t v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t i = lane + 64u * j;
    const uint32_t e1 = L.lit[i];
    v[j] = e1;
    const uint32_t l1 = (e1 >> 16) & 31;
    if (e1 < kKindLit && l1 < (uint32_t)kLitRoot) {
      const uint32_t e2 = L.lit[i >> l1];
      const uint32_t l2 = (e2 >> 16) & 31;
      if (e2 < kKindLit && l2 + l1 <= (uint32_t)kLitRoot)
        v[j] = ((l1 + l2) << 16) | (2u << 24) | (e1 & 0xffu) | ((e2 & 0xffu) << 8);
    }
  }
  wave_sync();
#pragma unroll
  for (int j = 0; j < 16; ++j) L.lit[lane + 64u * j] = v[j];
  wave_sync();
}

// puff-style canonical decode (sub-table overflow, split literal pairs: rare).
template <bool UNIFORM>
__device__ uint32_t canon_decode(uint64_t bits, const uint32_t* cnt, const uint16_t* sorted, int mode) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len < 16; ++len) {
    code |= (int)(bits & 1);
    bits >>= 1;
    const int count = UNIFORM ? (int)rfl(cnt[len]) : (int)cnt[len];
    if (code - count < first) {
      const uint32_t s = UNIFORM ? rfl(sorted[index + (code - first)]) : sorted[index + (code - first)];
      return make_entry(mode, s, (uint32_t)len);
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return kBadEntry;
}

template <bool UNIFORM>
__device__ __forceinline__ uint32_t lit_lookup(const HuffLds& L, uint64_t b) {
  uint32_t e = L.lit[(uint32_t)b & ((1u << kLitRoot) - 1)];
  if (UNIFORM) e = rfl(e);
  if (is_long(e)) {
    e = L.litsub[(e & 0xffffu) + ((uint32_t)(b >> kLitRoot) & ((1u << ((e >> 16) & 15u)) - 1))];
    if (UNIFORM) e = rfl(e);
  } else if ((e >> 26) == K_SLOW) {
    e = canon_decode<UNIFORM>(b, L.cnt_lit, L.sort_lit, 0);
  }
  return e;
}
template <bool UNIFORM>
__device__ __forceinline__ uint32_t dist_lookup(const HuffLds& L, uint64_t b) {
  uint32_t d = L.dist[(uint32_t)b & ((1u << kDistRoot) - 1)];
  if (UNIFORM) d = rfl(d);
  if (is_long(d)) {
    d = L.distsub[(d & 0xffffu) + ((uint32_t)(b >> kDistRoot) & ((1u << ((d >> 16) & 15u)) - 1))];
    if (UNIFORM) d = rfl(d);
  } else if ((d >> 26) == K_SLOW) {
    d = canon_decode<UNIFORM>(b, L.cnt_dist, L.sort_dist, 1);
  }
  return d;
}

// lane_decode exit events (EV_MERGE: the sync walk reached a boundary of the
// lane's speculative walk)
// (EV_HAND, lean instance only: the symbol needs the canonical decode, which
// the lean instance leaves to the fallback kernel)
enum : uint32_t {
  EV_STOP = 0, EV_EOB = 1, EV_INPUT = 2, EV_ERR = 3, EV_FULLX = 4, EV_FULLO = 5, EV_MERGE = 6, EV_HAND = 7
};
enum { LD_SPEC = 0, LD_SYNC = 1, LD_EMIT = 2 };

// Boundaries of a lane's speculative walk: p[k] = bit position after symbol
// kMergeFirst << k, b[k] = output bytes decoded up to there (~0u = not reached).
#ifndef HBAM_MERGE_FIRST
#define HBAM_MERGE_FIRST 4
#endif
constexpr uint32_t kMergeFirst = HBAM_MERGE_FIRST;  // power of two
static_assert((kMergeFirst & (kMergeFirst - 1)) == 0, "kMergeFirst: a power of two");
// Slices shorter than this many bits (a short last DEFLATE block) take their
// boundaries at kMergeFirst / 2 << k instead (0: never)
#ifndef HBAM_MERGE_SHORT_BITS
#define HBAM_MERGE_SHORT_BITS 400
#endif
constexpr uint32_t kMergeShortBits = HBAM_MERGE_SHORT_BITS;
#ifndef HBAM_MERGE_TINY_BITS
#define HBAM_MERGE_TINY_BITS 0
#endif
constexpr uint32_t kMergeTinyBits = HBAM_MERGE_TINY_BITS;  // ... kMergeFirst / 4 << k below this
// (the first boundary of a short / tiny slice, kMergeFirst / 2 or / 4, is at least one symbol)
static_assert(kMergeShortBits == 0 || kMergeFirst >= 2, "kMergeShortBits needs kMergeFirst >= 2");
static_assert(kMergeTinyBits == 0 || kMergeFirst >= 4, "kMergeTinyBits needs kMergeFirst >= 4");
struct MergePts {
  uint32_t p0, p1, p2, p3;
  uint32_t b0, b1, b2, b3;
};

// 16 B token store with 4 B alignment (global memory; unaligned mode).
struct __attribute__((packed, aligned(4))) Tok4 {
  uint32_t a, b, c, d;
};

// Decode from bit `a` while the position is below `stop` (bit positions are
// relative to the 16 B-aligned LDS image W; E = end of CDATA).  Returns the
// event that ended the walk; x = position reached, nt/nb = tokens/bytes
// decoded.
//   LD_SPEC records the first boundaries in mp;
//   LD_SYNC stops with EV_MERGE (mj = index) when it reaches one of them;
//   LD_EMIT writes tokens to tok[0..nt) and applies the output-space rules with
//           the output position of the first token = out0.
// LEAN: L holds the four decode tables only (no cnt_* / sort_*): a symbol that
// needs the canonical decode ends the walk with EV_HAND.
template <int MODE, bool LEAN = false>
__device__ __forceinline__ uint32_t lane_decode(const HuffLds& L, const uint32_t* __restrict__ W, uint32_t a,
                                                uint32_t stop, uint32_t E, uint32_t& x, uint32_t& nt, uint32_t& nb,
                                                MergePts& mp, uint32_t& mj, uint32_t* __restrict__ tok,
                                                uint32_t out0, uint32_t isize, uint32_t mf = kMergeFirst) {
  constexpr bool EMIT = MODE == LD_EMIT;
  uint32_t wd, cnt, nx;
  uint64_t buf;
#define LSEEK(p)                                                    \
  do {                                                              \
    wd = (p) >> 5;                                                  \
    buf = (((uint64_t)W[wd + 1] << 32) | W[wd]) >> ((p) & 31);      \
    cnt = 64 - ((p) & 31);                                          \
    wd += 2;                                                        \
    nx = W[wd];                                                     \
  } while (0)
  LSEEK(a);
  uint32_t pos = a, ev = EV_STOP;
  uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0, fill = 0;  // EMIT: pending tokens
  nt = 0;
  nb = 0;
  if (MODE == LD_SPEC) {
    mp.p0 = mp.p1 = mp.p2 = mp.p3 = ~0u;
    mp.b0 = mp.b1 = mp.b2 = mp.b3 = ~0u;
  }
#define LREFILL()                        \
  do {                                   \
    if (cnt <= 32) {                     \
      buf |= (uint64_t)nx << cnt;        \
      cnt += 32;                         \
      ++wd;                              \
      nx = W[wd];                        \
    }                                    \
  } while (0)
#define LCONSUME(n)  \
  do {               \
    buf >>= (n);     \
    cnt -= (n);      \
    pos += (n);      \
  } while (0)
#define LCOMMIT(t_, len_)                                                                   \
  do {                                                                                      \
    if (EMIT) {                                                                             \
      q0 = fill == 0 ? (t_) : q0;                                                           \
      q1 = fill == 1 ? (t_) : q1;                                                           \
      q2 = fill == 2 ? (t_) : q2;                                                           \
      q3 = (t_);                                                                            \
      if (++fill == 4) {                                                                    \
        *reinterpret_cast<Tok4*>(tok + nt - 3) = Tok4{q0, q1, q2, q3};                      \
        fill = 0;                                                                           \
      }                                                                                     \
    }                                                                                       \
    ++nt;                                                                                   \
    nb += (len_);                                                                           \
    if (MODE == LD_SPEC && (nt & (nt - 1)) == 0 && nt >= mf && nt <= 8 * mf) {                   \
      /* boundaries after symbols F, 2F, 4F, 8F: the speculative walk has */                \
      /* usually joined the true path by the later ones */                                  \
      mp.p0 = nt == mf ? pos : mp.p0;                                              \
      mp.b0 = nt == mf ? nb : mp.b0;                                               \
      mp.p1 = nt == 2 * mf ? pos : mp.p1;                                          \
      mp.b1 = nt == 2 * mf ? nb : mp.b1;                                           \
      mp.p2 = nt == 4 * mf ? pos : mp.p2;                                          \
      mp.b2 = nt == 4 * mf ? nb : mp.b2;                                           \
      mp.p3 = nt == 8 * mf ? pos : mp.p3;                                          \
      mp.b3 = nt == 8 * mf ? nb : mp.b3;                                           \
    }                                                                                       \
  } while (0)
  // Fast path: while a whole symbol (<= 15+5+15+13 = 48 bits) fits before E,
  // no CDATA-end checks are needed; literal and length/distance symbols are
  // decoded with selects instead of divergent branches (the wave mixes both in
  // nearly every step).  End-of-block, invalid codes and (EMIT) distances
  // beyond the output leave it; the slow path below re-decodes that symbol
  // from `pos` with every zlib check.
  const uint32_t fast_end = E >= 48 ? min(stop, E - 47) : 0u;
  for (;;) {
    bool merged = false;
    // Every lane peeks the 64 bits at `pos` from three words (no bit-buffer
    // refills).  The loop runs with the wave's exec mask unchanged until no
    // lane is active (one scalar branch per symbol): a lane that has left
    // (act = 0) or meets a symbol the fast path does not take (ok = 0) only
    // computes, every update is a select.  The branchy form paid an exec-mask
    // update per branch on the scalar unit that the CU's 16 waves share
    // (SQ_INSTS_SALU ~ 0.8 x SQ_INSTS_VALU, the issue limit of the kernel).
    // go(p): inside the fast region; SYNC: hit = p is a boundary of the lane's
    // speculative walk (the walks share every symbol from there on; the min
    // of the xors is 0 iff one matches).  & rather than &&: no branches.
    auto fast_go = [&](uint32_t p, uint32_t bytes, bool& hit) -> bool {
      hit = false;
      if (MODE == LD_SYNC) hit = min(min(p ^ mp.p0, p ^ mp.p1), min(p ^ mp.p2, p ^ mp.p3)) == 0;
      return (p < fast_end) & (!EMIT | (out0 + bytes < isize));
    };
    bool hit0;
    const bool g0 = fast_go(pos, nb, hit0);
    merged = g0 & hit0;
    bool act = g0 & !hit0;
    uint32_t it = 0, ucp = mf;  // iterations of this loop, next checkpoint iteration (wave-uniform)
    if (__builtin_amdgcn_ballot_w64(act)) do {
      const uint32_t wd = pos >> 5, sh = pos & 31;
      const uint32_t w0 = W[wd], w1 = W[wd + 1], w2 = W[wd + 2];
      const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh);
      const uint32_t hi = __builtin_amdgcn_alignbit(w2, w1, sh);
      uint32_t e = L.lit[lo & ((1u << kLitRoot) - 1)];
      {  // a code longer than the root (rare): every lane reads, long ones keep it
        const bool lg = is_long(e);
        if (__builtin_amdgcn_ballot_w64(lg)) {
          const uint32_t es = L.litsub[min((e & 0xffffu) + __builtin_amdgcn_ubfe(lo, kLitRoot, (e >> 16) & 15u),
                                           (uint32_t)kLitSubCap - 1)];  // in bounds for the lanes that drop it
          e = lg ? es : e;
        }
      }
      // kind 0 literal, 1 length: isl = bit 26; kind > 1 leaves the fast path
      const uint32_t isl = (e >> 26) & 1u;
      const uint32_t n1 = (e >> 16) & 31;
      const uint32_t ex = __builtin_amdgcn_ubfe(e, 9, 4 * isl);
      // literal: e >> 24 bytes; length: base + ex extra bits (ubfe of 0 bits is 0)
      const uint32_t len = (isl ? (e & 511) : (e >> 24)) + __builtin_amdgcn_ubfe(lo, n1, ex);
      const uint32_t c1 = n1 + ex;  // <= 20: the distance code starts inside lo
      const uint32_t b2 = __builtin_amdgcn_alignbit(hi, lo, c1);
      uint32_t d = L.dist[b2 & ((1u << kDistRoot) - 1)];
      {
        const bool lg = is_long(d);
        if (__builtin_amdgcn_ballot_w64(lg)) {
          const uint32_t ds = L.distsub[min((d & 0xffffu) + __builtin_amdgcn_ubfe(b2, kDistRoot, (d >> 16) & 15u),
                                            (uint32_t)kDistSubCap - 1)];
          d = lg ? ds : d;
        }
      }
      const uint32_t dn = (d >> 16) & 31, dx = (d >> 21) & 15;
      const uint32_t dist = (d & 0x7fff) + __builtin_amdgcn_ubfe(b2, dn, dx);
      // not taken here (the slow path decodes that symbol): an EOB / invalid /
      // canonical-decode entry (e >= 2 << 26), an invalid or canonical-decode
      // distance entry for a length (d >= 1 << 26: kinds K_BAD and K_SLOW),
      // (EMIT) a distance before the block start
      bool bad = (e >= (2u << 26)) | ((isl != 0) & (d >= kKindLit));
      if (EMIT) bad |= (isl != 0) & (out0 + nb < dist);
      const bool upd = act & !bad;
      const uint32_t tm = 0x80000000u | ((dist - 1) << 16) | len, tl = e & 0x0300ffffu;
      const uint32_t t = tl ^ ((tm ^ tl) & (0u - isl));
      const uint32_t npos = pos + c1 + ((dn + dx) & (0u - isl));
      pos = upd ? npos : pos;
      nb += upd ? len : 0u;
      if (EMIT) {
        const uint32_t fs = upd ? fill : 7u;  // the queue slot this token takes (7: none)
        q0 = fs == 0 ? t : q0;
        q1 = fs == 1 ? t : q1;
        q2 = fs == 2 ? t : q2;
        q3 = upd ? t : q3;
        if (fs == 3) *reinterpret_cast<Tok4*>(tok + nt - 3) = Tok4{q0, q1, q2, q3};
        fill = upd ? (fill + 1) & 3u : fill;
      }
      nt += upd ? 1u : 0u;
      ++it;
      if (MODE == LD_SPEC && it == ucp) {
        // boundaries after symbols F, 2F, 4F, 8F, tested at the iteration of
        // that number (uniform): a lane that entered this loop with nt = 0 and
        // decoded a symbol in every iteration has nt == it.  A lane that
        // re-entered after the slow path records only where the counts
        // agree; a missing boundary costs its sync walk time, not a result.
        const bool cp = upd & (nt == it);
        if (it == mf) { mp.p0 = cp ? pos : mp.p0; mp.b0 = cp ? nb : mp.b0; }
        if (it == 2 * mf) { mp.p1 = cp ? pos : mp.p1; mp.b1 = cp ? nb : mp.b1; }
        if (it == 4 * mf) { mp.p2 = cp ? pos : mp.p2; mp.b2 = cp ? nb : mp.b2; }
        if (it == 8 * mf) { mp.p3 = cp ? pos : mp.p3; mp.b3 = cp ? nb : mp.b3; }
        ucp = it == 8 * mf ? 0u : 2 * it;
      }
      bool hit;
      const bool g = fast_go(pos, nb, hit);
      merged = merged | (upd & g & hit);
      act = upd & g & !hit;
    } while (__builtin_amdgcn_ballot_w64(act));
    if (MODE == LD_SYNC && merged) {
      const bool h0 = pos == mp.p0, h1 = pos == mp.p1, h2 = pos == mp.p2;
      mj = h0 ? 0u : h1 ? 1u : h2 ? 2u : 3u;
    }
    if (MODE == LD_SYNC && merged) {
      ev = EV_MERGE;
      break;
    }
    // ---- slow path: one symbol with every check (or the end of the slice)
    if (pos >= stop) break;
    LSEEK(pos);
    if (MODE == LD_SYNC) {
      const bool h0 = pos == mp.p0, h1 = pos == mp.p1, h2 = pos == mp.p2, h3 = pos == mp.p3;
      if (h0 | h1 | h2 | h3) {
        mj = h0 ? 0u : h1 ? 1u : h2 ? 2u : 3u;
        ev = EV_MERGE;
        break;
      }
    }
    if (EMIT && out0 + nb >= isize) {
      ev = (out0 + nb == isize) ? EV_FULLX : EV_FULLO;
      break;
    }
    LREFILL();
    uint32_t e;
    if (LEAN) {
      e = L.lit[(uint32_t)buf & ((1u << kLitRoot) - 1)];
      if (is_long(e)) {
        e = L.litsub[(e & 0xffffu) + ((uint32_t)(buf >> kLitRoot) & ((1u << ((e >> 16) & 15u)) - 1))];
      } else if ((e >> 26) == K_SLOW) {
        ev = EV_HAND;
        break;
      }
    } else {
      e = lit_lookup<false>(L, buf);
    }
    uint32_t n1 = (e >> 16) & 31;
    uint32_t t, len;
    if (e < kKindLit) {
      if (pos + n1 > E) {  // a pair may straddle the end: decode the first literal alone
        if ((e >> 24) == 2u) {
          if (LEAN) { ev = EV_HAND; break; }
          e = canon_decode<false>(buf, L.cnt_lit, L.sort_lit, 0);
          n1 = (e >> 16) & 31;
        }
        if (pos + n1 > E) { ev = EV_INPUT; break; }
      }
      t = e & 0x0300ffffu;
      len = e >> 24;
      LCONSUME(n1);
    } else {
      const uint32_t k = e >> 26;
      if (k == K_LEN) {
        const uint32_t ex = (e >> 9) & 15;
        if (pos + n1 + ex > E) { ev = EV_INPUT; break; }
        len = (e & 511) + ((uint32_t)(buf >> n1) & ((1u << ex) - 1));
        LCONSUME(n1 + ex);
        LREFILL();
        uint32_t d;
        if (LEAN) {
          d = L.dist[(uint32_t)buf & ((1u << kDistRoot) - 1)];
          if (is_long(d)) {
            d = L.distsub[(d & 0xffffu) + ((uint32_t)(buf >> kDistRoot) & ((1u << ((d >> 16) & 15u)) - 1))];
          } else if ((d >> 26) == K_SLOW) {
            ev = EV_HAND;
            break;
          }
        } else {
          d = dist_lookup<false>(L, buf);
        }
        const uint32_t dn = (d >> 16) & 31;
        if (d >= kKindLit) {  // invalid distance code
          ev = (pos + max(dn, 1u) > E) ? EV_INPUT : EV_ERR;
          break;
        }
        const uint32_t dx = (d >> 21) & 15;
        if (pos + dn + dx > E) { ev = EV_INPUT; break; }
        const uint32_t dist = (d & 0x7fff) + ((uint32_t)(buf >> dn) & ((1u << dx) - 1));
        LCONSUME(dn + dx);
        if (EMIT && dist > out0 + nb) { ev = EV_ERR; break; }  // invalid distance too far back
        t = 0x80000000u | ((dist - 1) << 16) | len;
      } else if (k == K_EOB) {
        if (pos + n1 > E) { ev = EV_INPUT; break; }
        LCONSUME(n1);
        ev = EV_EOB;
        break;
      } else {  // invalid literal/length code
        ev = (pos + max(n1, 1u) > E) ? EV_INPUT : EV_ERR;
        break;
      }
    }
    LCOMMIT(t, len);
  }
#undef LSEEK
#undef LREFILL
#undef LCONSUME
#undef LCOMMIT
  if (EMIT && fill) {  // the 1..3 tokens not yet stored
    uint32_t* p = tok + nt - fill;
    p[0] = q0;
    if (fill > 1) p[1] = q1;
    if (fill > 2) p[2] = q2;
  }
  x = pos;
  return ev;
}

// Workgroup-wide helpers for the phase-A workgroup (all threads call them in
// uniform control flow; each ends with a barrier so `red` can be reused).
// NW: the workgroup's waves.
template <int NW = kHuffWaves>
__device__ __forceinline__ uint32_t wg_any(bool p, uint32_t* red) {
  const uint32_t w = threadIdx.x >> 6;
  const uint64_t b = __ballot(p);
  if (lane_id() == 0) red[w] = b != 0;
  __syncthreads();
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) r |= red[i];
  __syncthreads();
  return r;
}
template <int NW = kHuffWaves>
__device__ __forceinline__ uint32_t wg_min(uint32_t v, uint32_t* red) {
  const uint32_t w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
  if (lane_id() == 0) red[w] = v;
  __syncthreads();
  uint32_t r = 0xffffffffu;
#pragma unroll
  for (int i = 0; i < NW; ++i) r = min(r, red[i]);
  __syncthreads();
  return r;
}
// exclusive scans of (u, v) over the workgroup
template <int NW = kHuffWaves>
__device__ __forceinline__ void wg_excl_scan2(uint32_t u, uint32_t v, uint32_t* red, uint32_t& eu, uint32_t& ev) {
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t iu = wave_incl_scan(u), iv = wave_incl_scan(v);
  if (lane_id() == 63) {
    red[w] = iu;
    red[NW + w] = iv;
  }
  __syncthreads();
  uint32_t ou = 0, ov = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    ou += (uint32_t)i < w ? red[i] : 0u;
    ov += (uint32_t)i < w ? red[NW + i] : 0u;
  }
  __syncthreads();
  eu = ou + iu - u;
  ev = ov + iv - v;
}

// Wave-uniform bit reader over a 16 B-aligned LDS image (block headers, code
// lengths, lookahead).  Values are readfirstlane'd so the state stays in SGPRs.
struct SReader {
  const uint32_t* W;
  uint64_t buf;
  uint32_t cnt, wd;
  __device__ __forceinline__ void seek(uint32_t p) {
    wd = p >> 5;
    buf = (((uint64_t)rfl(W[wd + 1]) << 32) | rfl(W[wd])) >> (p & 31);
    cnt = 64 - (p & 31);
    wd += 2;
  }
  __device__ __forceinline__ void fill() {
    if (cnt <= 32) {
      buf |= (uint64_t)rfl(W[wd]) << cnt;
      cnt += 32;
      ++wd;
    }
  }
  __device__ __forceinline__ uint32_t pos() const { return 32u * wd - cnt; }
  __device__ __forceinline__ void consume(uint32_t n) {
    buf >>= n;
    cnt -= n;
  }
};

// Dynamic-Huffman block header after BTYPE: code-length code, code lengths,
// litlen / distance tables (+ literal pairing).  Run by one wave.  Returns
// DH_OK, DH_TRUNC (a field does not fit before bit E) or kErrIO
// (DataFormatException: bad counts, over/under-subscribed codes, a repeat with
// no previous length, no end-of-block code).
enum : int { DH_OK = 0, DH_TRUNC = -1 };
__device__ __forceinline__ int dyn_header(HuffLds& L, SReader& R, uint32_t E) {
  const uint32_t lane = lane_id();
  R.fill();
  if (R.pos() + 14 > E) return DH_TRUNC;
  const uint32_t hlit = ((uint32_t)R.buf & 31) + 257;
  const uint32_t hdist = ((uint32_t)(R.buf >> 5) & 31) + 1;
  const uint32_t hclen = ((uint32_t)(R.buf >> 10) & 15) + 4;
  R.consume(14);
  if (hlit > 286 || hdist > 30) return kErrIO;
  if (R.pos() + 3 * hclen > E) return DH_TRUNC;
  if (lane < 20) L.cl_lens[lane] = 0;
  wave_sync();
  for (uint32_t i = 0; i < hclen; ++i) {
    R.fill();
    const uint32_t v = (uint32_t)R.buf & 7;
    R.consume(3);
    if (lane == 0) L.cl_lens[kClOrder[i]] = (uint8_t)v;
  }
  wave_sync();
  if (rfl(build_table(L, L.cl_lens, 19, 7, 2, L.dist, L.cnt_dist, L.sort_dist, nullptr, 0))) return kErrIO;
  const uint32_t ntot = hlit + hdist;
  uint32_t i = 0, last = 0;
  while (i < ntot) {
    R.fill();
    const uint32_t e = rfl(L.dist[(uint32_t)R.buf & 127]);
    const uint32_t nbits = (e >> 16) & 31;
    if (R.pos() + nbits > E) return DH_TRUNC;
    const uint32_t sym = e & 0xffff;
    uint32_t rep, val, xb = 0;
    if (sym < 16) {
      rep = 1;
      val = sym;
    } else if (sym == 16) {
      xb = 2;
      rep = 3 + ((uint32_t)(R.buf >> nbits) & 3);
      val = last;
    } else if (sym == 17) {
      xb = 3;
      rep = 3 + ((uint32_t)(R.buf >> nbits) & 7);
      val = 0;
    } else {
      xb = 7;
      rep = 11 + ((uint32_t)(R.buf >> nbits) & 127);
      val = 0;
    }
    if (R.pos() + nbits + xb > E) return DH_TRUNC;
    if (sym == 16 && i == 0) return kErrIO;  // repeat with no previous length
    R.consume(nbits + xb);
    if (i + rep > ntot) return kErrIO;
    for (uint32_t j = lane; j < rep; j += 64) L.lens[i + j] = (uint8_t)val;
    i += rep;
    last = val;
  }
  wave_sync();
  if (rfl(L.lens[256]) == 0) return kErrIO;
  if (rfl(build_table(L, L.lens, (int)hlit, kLitRoot, 0, L.lit, L.cnt_lit, L.sort_lit, L.litsub, kLitSubCap)) ||
      rfl(build_table(L, L.lens + hlit, (int)hdist, kDistRoot, 1, L.dist, L.cnt_dist, L.sort_dist, L.distsub,
                      kDistSubCap)))
    return kErrIO;
  pair_literals(L);
  return DH_OK;
}

// Expected compressed bits of a non-final DEFLATE block, from its code
// lengths (symbol probabilities taken as 2^-length): zlib ends a block after
// lit_bufsize - 1 = 16383 symbols (deflate.c _tr_tally at the default
// memLevel 8), literals and length/distance pairs alike.  It sizes the first
// all-lane pass over the block, so that the slices do not reach far into the
// next block (decoded there with the wrong tables and thrown away); only the
// speed depends on it -- a short guess continues with another pass.  All 64
// lanes of a wave call it; lens[0..hlit) litlen, lens[hlit..hlit+hdist) dist.
constexpr uint32_t kZlibBlockSymbols = 16383;
__device__ uint32_t block_bits_estimate(const uint8_t* lens, uint32_t hlit, uint32_t hdist) {
  const uint32_t lane = lane_id();
  float wl = 0.f, al = 0.f, wlen = 0.f, wd = 0.f, ad = 0.f;
  for (uint32_t s = lane; s < hlit; s += 64) {
    const uint32_t l = lens[s];
    if (l == 0 || s == 256) continue;
    const float w = ldexpf(1.0f, -(int)l);
    wl += w;
    if (s < 256) {
      al += w * (float)l;
    } else if (s < 286) {
      al += w * (float)(l + kLenExtra[s - 257]);
      wlen += w;
    }
  }
  for (uint32_t d = lane; d < hdist && d < 30; d += 64) {
    const uint32_t l = lens[hlit + d];
    if (l == 0) continue;
    const float w = ldexpf(1.0f, -(int)l);
    wd += w;
    ad += w * (float)(l + kDistExtra[d]);
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    wl += __shfl_xor(wl, k, 64);
    al += __shfl_xor(al, k, 64);
    wlen += __shfl_xor(wlen, k, 64);
    wd += __shfl_xor(wd, k, 64);
    ad += __shfl_xor(ad, k, 64);
  }
  const float edist = wd > 0.f ? ad / wd : 0.f;
  const float per_sym = wl > 0.f ? (al + wlen * edist) / wl : 8.f;
  return rfl((uint32_t)fminf((float)kZlibBlockSymbols * per_sym, 1e9f));
}
// End of the first all-lane pass over a DEFLATE block whose symbols start at
// bit b0: an eighth over the estimate (a final block runs to the end).
__device__ __forceinline__ uint32_t pass_end(uint32_t b0, uint32_t est, bool final_blk, uint32_t E) {
  if (final_blk || est == 0) return E;
  const uint64_t e = (uint64_t)b0 + est + (est >> 3) + 1024;
  return e < E ? (uint32_t)e : E;
}

// Dynamic header with the code-length symbols decoded by all 64 lanes of the
// wave (k_huff_tables): lane l speculatively decodes the kClSlice bits from
// p + l*kClSlice of a window, a sync loop restarts slices from their
// predecessor's exit until every lane starts on a true boundary (code-length
// codes are <= 7 bits and resynchronise within a few symbols), then a wave
// scan of the run lengths places every lane's runs in lens[].  Valid headers
// only: any anomaly (bad counts, a repeat with no previous length, a run past
// HLIT+HDIST, bits beyond the staged window) returns DH_TRUNC and the decode
// kernel parses the block inline with dyn_header (the zlib semantics).
constexpr uint32_t kClSlice = 16;
constexpr uint32_t kClMaxSym = kClSlice;  // a slice holds at most one symbol per bit
struct ClLds {
  uint16_t ent[64][kClMaxSym];  // sym | extra << 5 | bits << 12
  uint8_t ex[64][kClSlice];     // k_huff_tables: the slice's exit from each entry offset
};
static_assert(sizeof(ClLds) <= sizeof(HuffLds::lit), "ClLds aliases HuffLds::lit in k_inflate_huff");
static_assert(sizeof(HuffLds::litsub) >= 1024 + 16, "k_huff_tables stages its header bits in litsub");

// Maps of 16 4-bit values (lo: inputs 0-7, hi: 8-15): g <- g o f, i.e.
// g'(e) = g(f(e)).
__device__ __forceinline__ void nib_compose(uint32_t& glo, uint32_t& ghi, uint32_t flo, uint32_t fhi) {
  const uint64_t g = ((uint64_t)ghi << 32) | glo;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    lo |= (uint32_t)(g >> (4u * ((flo >> (4 * e)) & 15u)) & 15u) << (4 * e);
    hi |= (uint32_t)(g >> (4u * ((fhi >> (4 * e)) & 15u)) & 15u) << (4 * e);
  }
  glo = lo;
  ghi = hi;
}

__device__ __forceinline__ uint32_t peek32(const uint32_t* W, uint32_t p) {
  return __builtin_amdgcn_alignbit(W[(p >> 5) + 1], W[p >> 5], p & 31);
}

// build_table_r for k_huff_tables (REG), build_table for k_inflate_huff's inline path
template <bool REG, typename... A>
__device__ __forceinline__ int build_tab(A&&... a) {
  if constexpr (REG) return build_table_r(static_cast<A&&>(a)...);
  else return build_table(static_cast<A&&>(a)...);
}

template <bool REG>
__device__ int dyn_header_par(HuffLds& L, ClLds& C, const uint32_t* __restrict__ W, uint32_t p, uint32_t E,
                              uint32_t* end_pos) {
  const uint32_t lane = lane_id();
  if (p + 14 > E) return DH_TRUNC;
  const uint32_t h = rfl(peek32(W, p));
  const uint32_t hlit = (h & 31) + 257, hdist = ((h >> 5) & 31) + 1, hclen = ((h >> 10) & 15) + 4;
  if (hlit > 286 || hdist > 30) return DH_TRUNC;
  p += 14;
  if (p + 3 * hclen > E) return DH_TRUNC;
  if (lane < 20) L.cl_lens[lane] = 0;
  wave_sync();
  if (lane < hclen) L.cl_lens[kClOrder[lane]] = (uint8_t)(peek32(W, p + 3 * lane) & 7);
  wave_sync();
  p += 3 * hclen;
  if (rfl(build_tab<REG>(L, L.cl_lens, 19, 7, 2, L.dist, L.cnt_dist, L.sort_dist, nullptr, 0))) return DH_TRUNC;
  const uint32_t ntot = hlit + hdist;
  uint32_t done = 0, prevv = 0, have_prev = 0;
  for (;;) {  // windows of 64 * kClSlice bits
    const uint32_t a0 = p + lane * kClSlice, stop = a0 + kClSlice;
    uint32_t a = a0, x = a0, ns = 0;
    if constexpr (REG) {
      // k_huff_tables: the symbol at EVERY bit offset of the slice (16
      // independent lookups), the slice's exit from every entry offset (a
      // backward pass), then the entries of the 64 slices chained on the
      // scalar unit.  The speculative decode + sync loop it replaces
      // restarted 62 of 64 lanes per window, ~21 K cycles per header.
      const bool live0 = a0 + 14 <= E;  // the decode stops at a field that may cross E (monotone in the offset)
      uint64_t win = 0;
      if (live0) win = (((uint64_t)W[(a0 >> 5) + 1] << 32) | W[a0 >> 5]) >> (a0 & 31);
      uint32_t lenv[kClSlice];
#pragma unroll
      for (uint32_t j = 0; j < kClSlice; ++j) {
        const uint32_t b = (uint32_t)(win >> j);
        const uint32_t e = L.dist[b & 127];
        const uint32_t nb = (e >> 16) & 31, sym = e & 0xffff;
        const uint32_t xb = sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u;
        const uint32_t ext = (b >> nb) & ((1u << xb) - 1);
        lenv[j] = nb + xb;
        C.ent[lane][j] = (uint16_t)(sym | (ext << 5) | ((nb + xb) << 12));
      }
      // exit offset (from the slice start) when the decode enters at j; the
      // next slice's entry is exit - kClSlice (<= 14), 15 = stopped at E
      uint32_t glo = 0, ghi = 0;
#pragma unroll
      for (int j = (int)kClSlice - 1; j >= 0; --j) {
        const uint32_t nx = (uint32_t)j + lenv[j];
        uint32_t exj = nx >= kClSlice ? nx : (uint32_t)C.ex[lane][min(nx, kClSlice - 1)];
        if (a0 + (uint32_t)j + 14 > E) exj = (uint32_t)j;
        C.ex[lane][j] = (uint8_t)exj;
        const uint32_t g = exj >= kClSlice ? exj - kClSlice : 15u;
        if (j < 8) glo |= g << (4 * j);
        else ghi |= g << (4 * (j - 8));
      }
      // entry of slice l = F_{l-1}(0), F_l = g_l o ... o g_0: an inclusive
      // DPP scan under composition (15 = stopped stays stopped; a lane with
      // no DPP source takes the identity).  A 64-step scalar chain of
      // readlanes took ~12.8 K cycles per header.
      ghi = (ghi & 0x0fffffffu) | 0xf0000000u;
      constexpr uint32_t kIdLo = 0x76543210u, kIdHi = 0xfedcba98u;
#define CL_SCAN_STEP(ctrl, rmask)                                                                        \
  do {                                                                                                     \
    const uint32_t plo_ = (uint32_t)__builtin_amdgcn_update_dpp((int)kIdLo, (int)glo, ctrl, rmask, 0xf, false); \
    const uint32_t phi_ = (uint32_t)__builtin_amdgcn_update_dpp((int)kIdHi, (int)ghi, ctrl, rmask, 0xf, false); \
    nib_compose(glo, ghi, plo_, phi_); /* g <- g o p: the earlier slices first */                         \
  } while (0)
      CL_SCAN_STEP(0x111, 0xf);  // row_shr:1
      CL_SCAN_STEP(0x112, 0xf);  // row_shr:2
      CL_SCAN_STEP(0x114, 0xf);  // row_shr:4
      CL_SCAN_STEP(0x118, 0xf);  // row_shr:8
      CL_SCAN_STEP(0x142, 0xa);  // row_bcast:15 -> rows 1, 3
      CL_SCAN_STEP(0x143, 0xc);  // row_bcast:31 -> rows 2, 3
#undef CL_SCAN_STEP
      const uint32_t my_e =
          (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(glo & 15u), 0x138, 0xf, 0xf, false);  // wave_shr:1; lane 0: 0
      // walk the true symbols from the entry, compacting them to ent[lane][0..ns)
      if (my_e != 15) {
        uint32_t q = my_e;
        a = a0 + q;
        while (q < kClSlice && a0 + q + 14 <= E) {
          const uint32_t en = C.ent[lane][q];
          C.ent[lane][ns++] = (uint16_t)en;
          q += en >> 12;
        }
        x = a0 + q;
      }
      // slices after the one that stopped at E start (and end) where it stopped
      const uint64_t stopped = __ballot(my_e != 15 && x < stop);
      if (stopped) {
        const uint32_t sl = (uint32_t)__ffsll((unsigned long long)stopped) - 1;
        const uint32_t xs = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)sl);
        if (lane > sl) {
          a = x = xs;
          ns = 0;
        }
      }
    } else {
    auto decode_slice = [&]() {
      x = a;
      ns = 0;
      while (x < stop && x + 14 <= E) {
        const uint32_t b = peek32(W, x);
        const uint32_t e = L.dist[b & 127];
        const uint32_t nb = (e >> 16) & 31, sym = e & 0xffff;
        const uint32_t xb = sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u;
        const uint32_t ext = (b >> nb) & ((1u << xb) - 1);
        if (ns < kClMaxSym) C.ent[lane][ns] = (uint16_t)(sym | (ext << 5) | ((nb + xb) << 12));
        ++ns;
        x += nb + xb;
      }
    };
    decode_slice();
    for (;;) {  // sync: restart each slice from its predecessor's exit
      uint32_t px = __shfl_up(x, 1, 64);
      if (lane == 0) px = a0;
      const bool need = px != a;
      if (__ballot(need) == 0) break;
      if (need) {
        a = px;
        decode_slice();
      }
    }
    }
    // run lengths of this lane's symbols and its last defined value
    uint32_t cnt = 0, own = 0, has = 0;
    for (uint32_t j = 0; j < ns && j < kClMaxSym; ++j) {
      const uint32_t en = C.ent[lane][j], sym = en & 31, ext = (en >> 5) & 127;
      cnt += sym < 16 ? 1u : sym == 18 ? 11u + ext : 3u + ext;
      if (sym != 16) {
        own = sym < 16 ? sym : 0u;
        has = 1;
      }
    }
    const bool bad_lane = ns > kClMaxSym;
    const uint32_t incl = wave_incl_scan_dpp(cnt);  // DPP: no LDS round trips
    const uint32_t base = done + incl - cnt;
    const uint64_t reach = __ballot(done + incl >= ntot);
    const uint32_t lend = reach ? (uint32_t)__ffsll((unsigned long long)reach) - 1 : 63u;
    // value entering each lane (for repeat codes): last defined value before
    // it, as a max-scan of (lane + 1) << 8 | value over the defining lanes
    const uint32_t key = wave_incl_max_dpp(has ? ((lane + 1u) << 8) | own : 0u);
    const uint32_t in_key = __shfl_up(key, 1, 64);
    uint32_t in_v = in_key & 0xffu, in_h = in_key != 0;
    if (lane == 0 || !in_h) {
      in_v = prevv;
      in_h = have_prev;
    }
    // write this lane's runs
    uint32_t i = base, last = in_v, hl = in_h, xe = a;
    bool bad = bad_lane;
    if (lane <= lend) {
      for (uint32_t j = 0; j < ns && j < kClMaxSym && i < ntot; ++j) {
        const uint32_t en = C.ent[lane][j], sym = en & 31, ext = (en >> 5) & 127;
        uint32_t val, rep;
        if (sym < 16) { val = sym; rep = 1; }
        else if (sym == 16) { val = last; rep = 3 + ext; bad |= !hl; }
        else if (sym == 17) { val = 0; rep = 3 + ext; }
        else { val = 0; rep = 11 + ext; }
        if (i + rep > ntot) { bad = true; break; }
        for (uint32_t k = 0; k < rep; ++k) L.lens[i + k] = (uint8_t)val;
        i += rep;
        last = val;
        hl = 1;
        xe += en >> 12;
      }
    }
    if (__ballot(bad)) return DH_TRUNC;
    if (reach) {  // this window completes the header: end = after lane lend's last used symbol
      const uint32_t end = (uint32_t)__builtin_amdgcn_readlane((int)xe, (int)lend);  // lend is wave-uniform
      if (end > E) return DH_TRUNC;
      *end_pos = rfl(end);
      break;
    }
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (tot == 0) return DH_TRUNC;  // no progress (ran past the staged window)
    done += tot;
    const uint32_t k63 = (uint32_t)__builtin_amdgcn_readlane((int)key, 63);
    if (k63) {
      prevv = k63 & 0xffu;
      have_prev = 1;
    }
    p = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
  }
  wave_sync();
  if (rfl(L.lens[256]) == 0) return DH_TRUNC;
  if (rfl(build_tab<REG>(L, L.lens, (int)hlit, kLitRoot, 0, L.lit, L.cnt_lit, L.sort_lit, L.litsub, kLitSubCap)))
    return DH_TRUNC;
  if (rfl(build_tab<REG>(L, L.lens + hlit, (int)hdist, kDistRoot, 1, L.dist, L.cnt_dist, L.sort_dist, L.distsub,
                      kDistSubCap)))
    return DH_TRUNC;
  pair_literals(L);
  return DH_OK;
}

// First DEFLATE block of every BGZF block: header + tables built ahead of the
// decode kernel, one wave per block at high occupancy, so the serial header
// work of one block overlaps the others instead of idling a decode workgroup.
// status 0: tables[blockIdx.x] holds the table image and the symbols start at
// bit B0; anything else (stored / fixed block, malformed or long header) is
// left to k_inflate_huff's inline path, which owns the error semantics.
constexpr uint32_t kTabStageBytes = 1024;
// Round 0 parses the header at the start of the block; later rounds the one
// where the previous decode round stopped (hout kHuffPending); blocks with
// nothing pending get status 2.
__global__ __launch_bounds__(64) void k_huff_tables(const uint8_t* __restrict__ file,
                                                    const BlockInfo* __restrict__ blocks, uint32_t b0,
                                                    uint8_t* __restrict__ tables,
                                                    HuffTableInfo* __restrict__ tinfo,
                                                    const HuffOut* __restrict__ hout, uint32_t round) {
  __shared__ __attribute__((aligned(16))) HuffLds L;
  ClLds& C = *reinterpret_cast<ClLds*>(L.lit);  // code-length symbols: done before lit[] is built
  // the staged header bits alias litsub[], which is written only after the
  // code lengths are decoded: 11.3 -> 9.9 KB of LDS, 14 -> 16 waves per CU
  uint4* s_in = reinterpret_cast<uint4*>(L.litsub);
  const uint32_t lane = lane_id();
  const uint32_t bi = b0 + blockIdx.x;
  const BlockInfo blk = blocks[bi];
  HuffTableInfo ti{1u, 0u, 0u, 0u};
  const uint64_t sbyte = blk.coff + 18;
  const uint64_t abase = sbyte & ~15ull;
  uint32_t hbit = 8u * (uint32_t)(sbyte - abase);  // the header, relative to abase
  bool todo = blk.isize != 0;
  if (round > 0) {
    const HuffOut ho = hout[bi];
    todo = todo && ho.status == kHuffPending;
    hbit = ho.resume_bit;
    if (!todo) ti.status = 2u;
  }
  if (todo) {
    // stage 1 KiB from the 16 B unit holding the header
    const uint32_t sb = (hbit >> 3) & ~15u;
    const uint32_t cend = (uint32_t)(blk.coff + blk.csize - abase);  // block end, relative to abase
    const uint32_t nreal = min((cend - sb + 15) >> 4, kTabStageBytes / 16);
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(file + abase + sb);
    for (uint32_t i = lane; i <= nreal; i += 64) s_in[i] = src[i];  // +1 pad chunk (file is padded)
    wave_sync();
    SReader R;
    R.W = reinterpret_cast<const uint32_t*>(s_in);
    const uint32_t Ereal = 8u * ((uint32_t)(sbyte - abase) + (blk.csize - 26)) - 8u * sb;
    const uint32_t E = min(Ereal, 128u * nreal);
    R.seek(hbit - 8u * sb);
    R.fill();
    if (R.pos() + 3 <= E && (((uint32_t)R.buf >> 1) & 3u) == 2u) {
      const uint32_t fin = (uint32_t)R.buf & 1u;
      R.consume(3);
      uint32_t b0pos = 0;
      const uint32_t hp = R.pos();
      const uint32_t h = rfl(peek32(R.W, hp));  // (read before the table build overwrites the staged bits)
      if (dyn_header_par<true>(L, C, R.W, hp, E, &b0pos) == DH_OK) {
        wave_sync();
        const uint32_t est = block_bits_estimate(L.lens, (h & 31) + 257, ((h >> 5) & 31) + 1);
        uint4* __restrict__ dst = reinterpret_cast<uint4*>(tables + (uint64_t)blockIdx.x * kTableImage);
        const uint4* img = reinterpret_cast<const uint4*>(&L);
        for (uint32_t i = lane; i < kTableImage / 16; i += 64) dst[i] = img[i];
        ti = HuffTableInfo{0u, b0pos + 8u * sb, fin, est};
      }
    }
  }
  if (lane == 0) tinfo[blockIdx.x] = ti;
}

// Control block: wave 0 -> workgroup (pass parameters) and back (results).
template <int NW>
struct HuffCtlT {
  uint32_t act;                 // kActDecode / kActDone
  uint32_t B0, out0, tok0;      // all-lane pass: first symbol bit, output / token position
  uint32_t Bend;                // its region end (pass_end; E for a final block)
  uint32_t fe, fx, ftok, fbytes, m3any;  // its result
  uint32_t xx[NW], xe[NW];  // exit / event of each wave's last lane
  uint32_t red[2 * NW];
};
using HuffCtl = HuffCtlT<kHuffWaves>;
enum : uint32_t { kActDecode = 1, kActDone = 2 };
constexpr uint32_t kHuffLdsBytes = (sizeof(HuffLds) + 15) & ~15u;
constexpr uint32_t kHuffCtlBytes = (sizeof(HuffCtl) + 15) & ~15u;
constexpr uint32_t kHuffStaticBytes = kHuffLdsBytes + kHuffCtlBytes;
// LDS of a phase-A workgroup (static, kHuffStageMaxLds): the staged block at
// offset 0 (its word addresses need no base add, and the three-word peek fits
// the ds_read2 offsets), then the tables and the control block.
constexpr uint32_t kHuffStageCap = kHuffStageMaxLds - kHuffStaticBytes;
static_assert(kHuffStageCap % 16 == 0 && kHuffStageCap >= 16 * 1024, "phase-A LDS budget");

constexpr int kHuffWavesPerSimd = 4;  // VGPR cap 128; LDS admits 4 staged workgroups per CU
// One decode round of block bx of the chunk (the body of k_huff_fallback),
// reading the compressed bits from an LDS copy of the block (STAGE) or from
// HBM/L2.
template <bool STAGE>
__device__ __forceinline__ void huff_block(uint8_t* smem, const uint8_t* __restrict__ file,
                                           const BlockInfo* __restrict__ blocks, uint32_t b0, uint64_t chunk_ustart,
                                           uint32_t* __restrict__ tokens, HuffOut* __restrict__ hout,
                                           const uint8_t* __restrict__ tables, const HuffTableInfo* __restrict__ tinfo,
                                           uint32_t round, uint32_t defer, uint32_t bx) {
  HuffLds& L = *reinterpret_cast<HuffLds*>(smem + kHuffStageCap);
  HuffCtl& C = *reinterpret_cast<HuffCtl*>(smem + kHuffStageCap + kHuffLdsBytes);
  uint4* s_in = reinterpret_cast<uint4*>(smem);
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t bi = b0 + bx;
  const BlockInfo blk = blocks[bi];
  const uint32_t isize = blk.isize;
  if (isize == 0) {  // inflate(buf,off,0) returns 0 without reading: nothing to validate
    if (tid == 0 && round == 0) { hout[bi].ntok = 0; hout[bi].status = kOk; }
    return;
  }
  HuffOut h0{0u, kOk, 0u, 0u};
  if (round > 0) {  // only blocks a previous round left pending
    h0 = hout[bi];
    if (h0.status != kHuffPending) return;
  }
  uint32_t* tok_out = tokens + (blk.ustart - chunk_ustart);
  const uint64_t sbyte = blk.coff + 18;  // cdata start
  const uint64_t abase = sbyte & ~15ull;
  const HuffTableInfo ti = tinfo[bx];
  {  // stage the block (+16 B of zero-padded file) and its prebuilt tables in LDS
    // One index space over both copies ([0, nq): block, [nq, nq + nt): table
    // image), kStageBatch 16 B loads in flight per thread before their LDS
    // stores: the copy costs about one memory latency instead of one per
    // loop trip.
    // A later round reads nothing before the bit where the last one stopped,
    // so only the 16 B units from there on are staged.
    const uint32_t nq_all = STAGE ? (uint32_t)((blk.coff + blk.csize - abase + 15) >> 4) + 1 : 0u;
    const uint32_t q0 = round > 0 ? min(h0.resume_bit >> 7, nq_all) : 0u;
    const uint32_t nq = nq_all - q0;
    const uint32_t nt = ti.status == 0 ? kTableImage / 16 : 0u;
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(file + abase) + q0;
    const uint4* __restrict__ tsrc = reinterpret_cast<const uint4*>(tables + (uint64_t)bx * kTableImage);
    uint4* sdst = s_in + q0;
    uint4* tdst = reinterpret_cast<uint4*>(&L);
    // global -> LDS without registers (global_load_lds_dwordx4): each wave
    // instruction moves 64 consecutive 16 B units to LDS base + lane x 16, all
    // of a workgroup's copies in flight at once (__syncthreads drains them;
    // phase A 8.52 -> 8.00 ms per C2 pass against register staging with 4-10
    // loads in flight per thread)
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef __attribute__((address_space(1))) void* gbl_vp;
    const uint32_t wv = tid >> 6, ln = tid & 63;
    for (uint32_t u0 = 64 * wv; u0 < nq; u0 += kHuffThreads)
      if (u0 + ln < nq) __builtin_amdgcn_global_load_lds((gbl_vp)(src + u0 + ln), (lds_vp)(sdst + u0), 16, 0, 0);
    for (uint32_t u0 = 64 * wv; u0 < nt; u0 += kHuffThreads)
      if (u0 + ln < nt) __builtin_amdgcn_global_load_lds((gbl_vp)(tsrc + u0 + ln), (lds_vp)(tdst + u0), 16, 0, 0);
  }
  __syncthreads();
  // compressed bits: the LDS copy, or (unstaged) the file in HBM
  const uint32_t* __restrict__ W =
      STAGE ? reinterpret_cast<const uint32_t*>(s_in) : reinterpret_cast<const uint32_t*>(file + abase);
  const uint32_t E = 8u * ((uint32_t)(sbyte - abase) + (blk.csize - 26));  // end of CDATA (bits from W)

  SReader R;  // wave 0's reader
  R.W = W;
  R.buf = 0;
  R.cnt = R.wd = 0;

  uint32_t outpos = h0.outpos, ntok = h0.ntok;
  bool pending = false;  // stopped before the next DEFLATE block's header (defer)
  uint32_t resume_bit = 0;
  int err = kOk;
  bool look = false;       // output exactly full: zlib's lookahead
  bool final_blk = false;  // BFINAL of the current DEFLATE block
  bool resume = false;     // an all-lane pass result waits in C
  bool pre = ti.status == 0;  // first DEFLATE block's header + tables come from k_huff_tables
  uint32_t est = 0, bend = E;  // wave 0: the current block's size estimate, the pass region end

  // zlib's lookahead once the output is exactly full: decode on until a
  // symbol needs room; returns true when it ends at a (non-final) EOB so the
  // next block header must be examined too.
  auto lookahead = [&]() -> bool {
    for (;;) {
      R.fill();
      const uint32_t p = R.pos();
      const uint32_t e = lit_lookup<true>(L, R.buf);
      const uint32_t n1 = (e >> 16) & 31;
      if (e < kKindLit) return false;  // literal: no room (a pair's first code is checked by n1 >= its length)
      const uint32_t k = e >> 26;
      if (k == K_LEN) {
        const uint32_t ex = (e >> 9) & 15;
        if (p + n1 + ex > E) return false;
        R.consume(n1 + ex);
        R.fill();
        const uint32_t d = dist_lookup<true>(L, R.buf);
        const uint32_t dn = (d >> 16) & 31;
        if (d >= kKindLit) {
          if (R.pos() + max(dn, 1u) <= E) err = kErrIO;
          return false;
        }
        const uint32_t dx = (d >> 21) & 15;
        if (R.pos() + dn + dx > E) return false;
        const uint32_t dist = (d & 0x7fff) + ((uint32_t)(R.buf >> dn) & ((1u << dx) - 1));
        if (dist > outpos) err = kErrIO;
        return false;
      }
      if (k == K_EOB) {
        if (p + n1 > E) return false;
        R.consume(n1);
        return !final_blk;
      }
      if (p + max(n1, 1u) <= E) err = kErrIO;  // invalid literal/length code
      return false;
    }
  };

  if (wave == 0) R.seek(round > 0 ? h0.resume_bit : 8u * (uint32_t)(sbyte - abase));
  for (;;) {
    if (wave == 0) {
      uint32_t act = kActDone;
      for (;;) {  // wave-uniform: advance to the next all-lane pass or to the end
        bool do_look = false;
        if (resume) {  // ---- result of the all-lane pass
          resume = false;
          const uint32_t fe = rfl(C.fe), fxs = rfl(C.fx), m3any = rfl(C.m3any);
          ntok = rfl(ntok + C.ftok);
          outpos = rfl(outpos + C.fbytes);
          if (!m3any && bend < E && fxs < E && outpos < isize) {
            // the pass ended at its region end inside the block: go on with
            // the same tables over the next stretch
            bend = min(E, fxs + (est >> 2) + 4096u);
            if (lane == 0) {
              C.B0 = fxs;
              C.Bend = bend;
              C.out0 = outpos;
              C.tok0 = ntok;
            }
            act = kActDecode;
            resume = true;
            break;
          }
          if (!m3any) {  // walked to the end of CDATA without an end-of-block
            if (outpos < isize) err = kErrFormat;
            else if (outpos == isize) { look = true; R.seek(fxs); }
            else break;
            if (err != kOk || fxs >= E) break;
            do_look = true;
          } else if (fe == EV_EOB) {
            R.seek(fxs);
            if (final_blk) { err = kErrFormat; break; }  // EOB before ISIZE bytes
            if (defer) {  // the next header is the next round's (k_huff_tables)
              pending = true;
              resume_bit = fxs;
              break;
            }
            continue;
          } else if (fe == EV_FULLX) {
            look = true;
            R.seek(fxs);
            do_look = true;
          } else if (fe == EV_FULLO) {
            break;
          } else {
            err = fe == EV_ERR ? kErrIO : kErrFormat;
            break;
          }
        } else if (pre) {  // ---- first DEFLATE block: prebuilt tables already in LDS
          pre = false;
          final_blk = ti.final_blk != 0;
          R.seek(ti.B0);
          est = ti.est_bits;
          bend = pass_end(ti.B0, est, final_blk, E);
          if (lane == 0) {
            C.B0 = ti.B0;
            C.Bend = bend;
            C.out0 = outpos;
            C.tok0 = ntok;
          }
          act = kActDecode;
          resume = true;
          break;
        } else {  // ---- next DEFLATE block header
          if (err != kOk) break;
          R.fill();
          if (R.pos() + 3 > E) { if (!look) err = kErrFormat; break; }
          const uint32_t hdr = (uint32_t)R.buf & 7;
          R.consume(3);
          final_blk = hdr & 1;
          const uint32_t type = hdr >> 1;
          if (type == 0) {  // stored
            R.consume((8u - (R.pos() & 7u)) & 7u);  // to the byte boundary
            R.fill();
            if (R.pos() + 32 > E) { if (!look) err = kErrFormat; break; }
            const uint32_t len = (uint32_t)R.buf & 0xffff, nlen = (uint32_t)(R.buf >> 16) & 0xffff;
            R.consume(32);
            if (len != (~nlen & 0xffffu)) { err = kErrIO; break; }
            const uint32_t p = R.pos();  // byte aligned
            if (look) {
              if (len != 0) break;  // COPY with no room: zlib stops here
              if (final_blk) break;
              continue;
            }
            const uint32_t n = min(min(len, isize - outpos), (E - p) >> 3);
            const uint8_t* src = reinterpret_cast<const uint8_t*>(W) + (p >> 3);
            for (uint32_t j = lane; j < n; j += 64) tok_out[ntok + j] = (1u << 24) | src[j];
            ntok += n;
            outpos += n;
            R.seek(p + 8 * n);
            if (n < len) {
              if (outpos < isize) err = kErrFormat;  // ran out of input
              break;
            }
            if (final_blk) {
              if (outpos < isize) err = kErrFormat;
              break;
            }
            if (outpos == isize) look = true;
            continue;
          }
          if (type == 3) { err = kErrIO; break; }
          const uint32_t hp = R.pos();
          if (type == 1) {  // fixed Huffman
            for (int s = lane; s < 320; s += 64) {
              uint8_t l;
              if (s < 144) l = 8; else if (s < 256) l = 9; else if (s < 280) l = 7; else if (s < 288) l = 8; else l = 5;
              L.lens[s] = l;
            }
            wave_sync();
            if (rfl(build_table(L, L.lens, 288, kLitRoot, 0, L.lit, L.cnt_lit, L.sort_lit, L.litsub, kLitSubCap)) ||
                rfl(build_table(L, L.lens + 288, 32, kDistRoot, 1, L.dist, L.cnt_dist, L.sort_dist, L.distsub,
                                kDistSubCap))) {
              err = kErrIO;
              break;
            }
            pair_literals(L);
            est = block_bits_estimate(L.lens, 288, 32);
          } else {  // dynamic Huffman: code lengths decoded by the 64 lanes of the wave
            uint32_t endp = 0;
            int dh = dyn_header_par<false>(L, *reinterpret_cast<ClLds*>(L.lit), W, R.pos(), E, &endp);
            if (rfl(dh) == DH_OK) {
              R.seek(endp);
            } else {  // an anomaly: the serial parse owns zlib's error semantics
              dh = dyn_header(L, R, E);
              if (dh == DH_TRUNC) { if (!look) err = kErrFormat; break; }
              if (dh != DH_OK) { err = kErrIO; break; }
            }
            const uint32_t h = rfl(peek32(W, hp));
            est = block_bits_estimate(L.lens, (h & 31) + 257, ((h >> 5) & 31) + 1);
          }
          if (!look) {  // hand the symbol stream to the workgroup
            bend = pass_end(R.pos(), est, final_blk, E);
            if (lane == 0) {
              C.Bend = bend;
              C.B0 = R.pos();
              C.out0 = outpos;
              C.tok0 = ntok;
            }
            act = kActDecode;
            resume = true;
            break;
          }
          do_look = true;
        }
        if (do_look) {
          if (!lookahead()) break;
        }
      }
      if (lane == 0) C.act = act;
    }
    __syncthreads();
    if (C.act != kActDecode) break;

    // ---- all-lane decode of this DEFLATE block's symbols
    const uint32_t B0 = C.B0, out0 = C.out0, tok0 = C.tok0, Bend = C.Bend;
    const uint32_t R = Bend > B0 ? Bend - B0 : 0u;
    const uint32_t S = (R + kHuffThreads - 1) / kHuffThreads;
    uint32_t a = min(B0 + tid * S, Bend);
    const uint32_t stop = tid == kHuffThreads - 1 ? Bend : min(B0 + (tid + 1) * S, Bend);
    MergePts mp;
    uint32_t mj = 0, x, nt, nb;
    const uint32_t mf = S < kMergeTinyBits ? kMergeFirst / 4 : S < kMergeShortBits ? kMergeFirst / 2 : kMergeFirst;
    uint32_t ev = lane_decode<LD_SPEC>(L, W, a, stop, E, x, nt, nb, mp, mj, nullptr, 0, 0, mf);
    const uint32_t sx = x, snt = nt, snb = nb, sev = ev;
    for (;;) {  // sync: restart each slice from its predecessor's exit
      if (lane == 63) {
        C.xx[wave] = x;
        C.xe[wave] = ev;
      }
      __syncthreads();
      uint32_t px = __shfl_up(x, 1, 64), pev = __shfl_up(ev, 1, 64);
      if (lane == 0 && wave > 0) {
        px = C.xx[wave - 1];
        pev = C.xe[wave - 1];
      }
      const bool need = tid > 0 && pev == EV_STOP && px != a;
      if (!wg_any(need, C.red)) break;
      if (need) {
        a = px;
        uint32_t rx, rnt, rnb;
        const uint32_t rev = lane_decode<LD_SYNC>(L, W, a, stop, E, rx, rnt, rnb, mp, mj, nullptr, 0, 0, mf);
        if (rev == EV_MERGE) {  // shares the speculative walk from boundary mj on
          const uint32_t bj = mj == 0 ? mp.b0 : mj == 1 ? mp.b1 : mj == 2 ? mp.b2 : mp.b3;
          x = sx;
          ev = sev;
          nt = rnt + snt - (mf << mj);
          nb = rnb + snb - bj;
        } else {
          x = rx;
          ev = rev;
          nt = rnt;
          nb = rnb;
        }
      }
    }
    const uint32_t lend0 = wg_min(ev != EV_STOP ? tid : 0xffffffffu, C.red);
    const uint32_t lend = lend0 == 0xffffffffu ? (uint32_t)kHuffThreads - 1 : lend0;
    const bool valid = tid <= lend;
    uint32_t toff, boff;
    wg_excl_scan2(valid ? nt : 0u, valid ? nb : 0u, C.red, toff, boff);
    uint32_t x3 = a, nt3 = 0, nb3 = 0, ev3 = EV_STOP;
    if (valid)
      ev3 = lane_decode<LD_EMIT>(L, W, a, stop, E, x3, nt3, nb3, mp, mj, tok_out + tok0 + toff, out0 + boff, isize);
    const uint32_t m3 = wg_min((valid && ev3 != EV_STOP) ? tid : 0xffffffffu, C.red);
    const uint32_t f = m3 != 0xffffffffu ? m3 : lend;
    if (tid == f) {
      C.fe = ev3;
      C.fx = x3;
      C.ftok = toff + nt3;
      C.fbytes = boff + nb3;
      C.m3any = m3 != 0xffffffffu;
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (wave == 0 && pending && err == kOk) {
      hout[bi] = HuffOut{ntok, kHuffPending, resume_bit, outpos};
    } else {
      if (err == kOk && outpos < isize) err = kErrFormat;  // "Did not inflate expected amount"
      hout[bi] = HuffOut{ntok, err, 0u, outpos};
    }
  }
}

// Phase A fallback: the blocks of the chunk that the round's lean launch
// handed over (flist: [round] = their count, [kHuffListHdr ..) = their indices
// in the chunk), a fixed grid striding over the list.  Each block's round is
// redone from hout as it was at round entry, so the same token range is
// rewritten.  A workgroup stages its compressed block in LDS when it fits
// kHuffStageCap, else it reads the bits from HBM/L2.
__global__ __launch_bounds__(kHuffThreads, kHuffWavesPerSimd) void k_huff_fallback(
    const uint8_t* __restrict__ file, const BlockInfo* __restrict__ blocks, uint32_t b0, uint64_t chunk_ustart,
    uint32_t* __restrict__ tokens, HuffOut* __restrict__ hout, const uint8_t* __restrict__ tables,
    const HuffTableInfo* __restrict__ tinfo, uint32_t round, uint32_t defer, const uint32_t* flist, uint32_t nb,
    uint32_t* pstats) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kHuffStageCap + kHuffStaticBytes];
  const uint32_t n = min(flist[round], nb);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t bx = flist[kHuffListHdr + i];
    if (bx >= nb) continue;
    const BlockInfo& b = blocks[b0 + bx];
    const uint64_t abase = (b.coff + 18) & ~15ull;
    const uint32_t need = (uint32_t)(((b.coff + b.csize - abase + 15) >> 4) + 1) * 16u;  // huff_stage_bytes
    if (need <= kHuffStageCap)
      huff_block<true>(smem, file, blocks, b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, bx);
    else
      huff_block<false>(smem, file, blocks, b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, bx);
    __syncthreads();  // the next block's staging overwrites this one's LDS
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(&pstats[kPathStatFallback], n);
}

// ---- the lean instance
// LDS of a lean workgroup (static, kLeanLds): the staged window at offset 0,
// the four decode tables (the leading kLeanTableBytes of the table image),
// the control block.
#ifndef HBAM_HUFF_WAVES_PER_SIMD
#define HBAM_HUFF_WAVES_PER_SIMD 5
#endif
constexpr int kLeanWavesPerSimd = HBAM_HUFF_WAVES_PER_SIMD;  // 5: VGPR cap 96, 5 workgroups of <= 32 KB per CU
constexpr uint32_t kLeanTableBytes = offsetof(HuffLds, cnt_lit);  // lit, litsub, dist, distsub
// The lean body runs at two widths.  NT = kHuffThreads: kLeanLds per
// workgroup, every round 0 and the later rounds' hand-up list.  NT =
// kNarrowThreads: the later rounds' first launch.  A second DEFLATE block is
// a third of the first one's bits (C2: ~7.3 KB against ~19.5 KB); cut 256
// ways its slices (~230 bits) are shorter than the 16-32 symbols a walk
// needs to join the true path, so sync dominates, and two waves pay it
// instead of four.  Its window fits kNarrowLds, which keeps 20 waves per CU.
#ifndef HBAM_HUFF_NARROW_LDS
#define HBAM_HUFF_NARROW_LDS (16 * 1024)
#endif
constexpr int kNarrowThreads = 128;
constexpr uint32_t kNarrowLds = HBAM_HUFF_NARROW_LDS;
// HBAM_HUFF_NARROW=0: every round at 256 lanes (A/B knob)
#ifndef HBAM_HUFF_NARROW
#define HBAM_HUFF_NARROW 1
#endif
constexpr bool kHuffNarrow = HBAM_HUFF_NARROW != 0;
// HBAM_HUFF_MIN_SLICE_BITS: a floor under the slice size (A/B knob: fewer
// active lanes inside the same workgroup; 0 = off)
#ifndef HBAM_HUFF_MIN_SLICE_BITS
#define HBAM_HUFF_MIN_SLICE_BITS 0
#endif
constexpr uint32_t kHuffMinSliceBits = HBAM_HUFF_MIN_SLICE_BITS;
template <int NT>
struct LeanGeom {
  static_assert(NT == kHuffThreads || NT == kNarrowThreads, "lean widths");
  static constexpr int kWaves = NT / 64;
  static constexpr uint32_t kLds = NT == kHuffThreads ? kLeanLds : kNarrowLds;
  static constexpr uint32_t kCtlBytes = (sizeof(HuffCtlT<kWaves>) + 15) & ~15u;
  static constexpr uint32_t kStageCap = kLds - kLeanTableBytes - kCtlBytes;
};
constexpr uint32_t kLeanStageCap = LeanGeom<kHuffThreads>::kStageCap;
constexpr uint32_t kNarrowStageCap = LeanGeom<kNarrowThreads>::kStageCap;
static_assert(kLeanTableBytes % 16 == 0 && kLeanTableBytes <= kTableImage, "lean tables: a prefix of the table image");
static_assert(kLeanLds <= 64 * 1024 && kLeanStageCap % 16 == 0 && kLeanStageCap >= 8 * 1024, "lean LDS budget");
static_assert(kNarrowStageCap % 16 == 0 && kNarrowStageCap >= 8 * 1024 && kNarrowStageCap <= kLeanStageCap,
              "narrow LDS budget");
// bits a walk may read past its region end: a lane's exit lies up to one
// symbol (48 bits) past its stop, and the slow path's reader holds four
// words from the word of that position on
constexpr uint32_t kLeanReadPast = 48 + 128;

// One round of the block passed in (blk, ti, timg) from its prebuilt tables: the passes
// of huff_block over one DEFLATE block (stage, speculate, sync, emit, and the
// same-tables continuation), every lane taking the (uniform) decisions wave 0
// takes there.  Handled inline: the end-of-block that leaves the block
// pending (defer), output overfull (EV_FULLO), and output exactly full
// (EV_FULLX) where the next code is an end-of-block inside CDATA of a final
// block -- the end of every well-formed BGZF block.  Returns kLeanDone; or,
// with hout untouched, kLeanWide (the round's window is larger than this
// width's stage: a function of blk and ti alone, decided before anything is
// read) or kLeanOther for everything else: the fallback redoes the round.
// Bit positions are relative to the 16 B unit the staged window starts at.
enum : int { kLeanDone = 0, kLeanWide = 1, kLeanOther = 2 };
template <int NT>
__device__ __forceinline__ int lean_block(uint8_t* smem, const uint8_t* __restrict__ file, const BlockInfo& blk,
                                           uint32_t* __restrict__ tok_out, HuffOut& h, const uint8_t* __restrict__ timg,
                                           const HuffTableInfo& ti, uint32_t isize, uint32_t defer) {
  using G = LeanGeom<NT>;
  using Ctl = HuffCtlT<G::kWaves>;
  if (ti.status != 0) return kLeanOther;  // no prebuilt tables: stored / fixed block, an anomalous header
  HuffLds& L = *reinterpret_cast<HuffLds*>(smem + G::kStageCap);  // (only its leading kLeanTableBytes exist)
  Ctl& C = *reinterpret_cast<Ctl*>(smem + G::kStageCap + kLeanTableBytes);
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint64_t sbyte = blk.coff + 18;  // cdata start
  const uint64_t abase = sbyte & ~15ull;
  const uint32_t Eabs = 8u * ((uint32_t)(sbyte - abase) + (blk.csize - 26));  // end of CDATA
  if (ti.B0 > Eabs) return kLeanOther;
  const bool final_blk = ti.final_blk != 0;
  const uint32_t est = ti.est_bits;
  const uint32_t bend_abs = pass_end(ti.B0, est, final_blk, Eabs);
  // the round's window, in 16 B units of the block (+16 B of zero-padded file)
  const uint32_t nq_all = (uint32_t)((blk.coff + blk.csize - abase + 15) >> 4) + 1;
  const uint32_t q0 = min(ti.B0 >> 7, nq_all);
  const uint32_t q1 = min(((bend_abs + kLeanReadPast) >> 7) + 1, nq_all);
  const uint32_t nq = q1 > q0 ? q1 - q0 : 0u;
  if (nq * 16u > G::kStageCap) return NT == kNarrowThreads ? kLeanWide : kLeanOther;  // a window larger than the stage
  {  // stage the window and the tables (global -> LDS without registers, as huff_block)
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(file + abase) + q0;
    const uint4* __restrict__ tsrc = reinterpret_cast<const uint4*>(timg);
    uint4* sdst = reinterpret_cast<uint4*>(smem);
    uint4* tdst = reinterpret_cast<uint4*>(&L);
    constexpr uint32_t nt = kLeanTableBytes / 16;
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef __attribute__((address_space(1))) void* gbl_vp;
    for (uint32_t u0 = 64 * wave; u0 < nq; u0 += NT)
      if (u0 + lane < nq) __builtin_amdgcn_global_load_lds((gbl_vp)(src + u0 + lane), (lds_vp)(sdst + u0), 16, 0, 0);
    for (uint32_t u0 = 64 * wave; u0 < nt; u0 += NT)
      if (u0 + lane < nt) __builtin_amdgcn_global_load_lds((gbl_vp)(tsrc + u0 + lane), (lds_vp)(tdst + u0), 16, 0, 0);
  }
  __syncthreads();
  const uint32_t* __restrict__ W = reinterpret_cast<const uint32_t*>(smem);
  const uint32_t bias = q0 << 7;
  const uint32_t E = Eabs - bias;
  // bits a later pass may read: everything staged, or (the block's end is
  // staged) whatever huff_block reads
  const uint32_t read_end = q1 == nq_all ? 0xffffffffu : nq << 7;
  uint32_t B0 = ti.B0 - bias, Bend = bend_abs - bias;
  uint32_t outpos = h.outpos, ntok = h.ntok;
  for (;;) {
    // ---- all-lane decode of [B0, Bend)
    const uint32_t R = Bend > B0 ? Bend - B0 : 0u;
    const uint32_t S = max((R + NT - 1) / NT, kHuffMinSliceBits);
    uint32_t a = min(B0 + tid * S, Bend);
    const uint32_t stop = tid == NT - 1 ? Bend : min(B0 + (tid + 1) * S, Bend);
    MergePts mp;
    uint32_t mj = 0, x, nt, nb;
    const uint32_t mf = S < kMergeTinyBits ? kMergeFirst / 4 : S < kMergeShortBits ? kMergeFirst / 2 : kMergeFirst;
    uint32_t ev = lane_decode<LD_SPEC, true>(L, W, a, stop, E, x, nt, nb, mp, mj, nullptr, 0, 0, mf);
    const uint32_t sx = x, snt = nt, snb = nb, sev = ev;
    for (;;) {  // sync: restart each slice from its predecessor's exit
      if (lane == 63) {
        C.xx[wave] = x;
        C.xe[wave] = ev;
      }
      __syncthreads();
      uint32_t px = __shfl_up(x, 1, 64), pev = __shfl_up(ev, 1, 64);
      if (lane == 0 && wave > 0) {
        px = C.xx[wave - 1];
        pev = C.xe[wave - 1];
      }
      const bool need = tid > 0 && pev == EV_STOP && px != a;
      if (!wg_any<G::kWaves>(need, C.red)) break;
      if (need) {
        a = px;
        uint32_t rx, rnt, rnb;
        const uint32_t rev = lane_decode<LD_SYNC, true>(L, W, a, stop, E, rx, rnt, rnb, mp, mj, nullptr, 0, 0, mf);
        if (rev == EV_MERGE) {  // shares the speculative walk from boundary mj on
          const uint32_t bj = mj == 0 ? mp.b0 : mj == 1 ? mp.b1 : mj == 2 ? mp.b2 : mp.b3;
          x = sx;
          ev = sev;
          nt = rnt + snt - (mf << mj);
          nb = rnb + snb - bj;
        } else {
          x = rx;
          ev = rev;
          nt = rnt;
          nb = rnb;
        }
      }
    }
    const uint32_t lend0 = wg_min<G::kWaves>(ev != EV_STOP ? tid : 0xffffffffu, C.red);
    const uint32_t lend = lend0 == 0xffffffffu ? (uint32_t)NT - 1 : lend0;
    const bool valid = tid <= lend;
    uint32_t toff, boff;
    wg_excl_scan2<G::kWaves>(valid ? nt : 0u, valid ? nb : 0u, C.red, toff, boff);
    uint32_t x3 = a, nt3 = 0, nb3 = 0, ev3 = EV_STOP;
    if (valid)
      ev3 = lane_decode<LD_EMIT, true>(L, W, a, stop, E, x3, nt3, nb3, mp, mj, tok_out + ntok + toff, outpos + boff,
                                       isize);
    const uint32_t m3 = wg_min<G::kWaves>((valid && ev3 != EV_STOP) ? tid : 0xffffffffu, C.red);
    const uint32_t f = m3 != 0xffffffffu ? m3 : lend;
    if (tid == f) {
      C.fe = ev3;
      C.fx = x3;
      C.ftok = toff + nt3;
      C.fbytes = boff + nb3;
      C.m3any = m3 != 0xffffffffu;
    }
    __syncthreads();
    // ---- the pass's result (uniform)
    const uint32_t fe = rfl(C.fe), fxs = rfl(C.fx), m3any = rfl(C.m3any);
    ntok = rfl(ntok + C.ftok);
    outpos = rfl(outpos + C.fbytes);
    if (!m3any) {
      // the pass ended at its region end inside the block: go on with the
      // same tables over the next stretch, if it is staged
      if (!(Bend < E && fxs < E && outpos < isize)) return kLeanOther;
      const uint32_t bnext = min(E, fxs + (est >> 2) + 4096u);
      if (bnext + kLeanReadPast > read_end) return kLeanOther;
      B0 = fxs;
      Bend = bnext;
      continue;
    }
    if (fe == EV_EOB) {
      if (final_blk || !defer) return kLeanOther;  // an early end (error), or a header for this round
      h = HuffOut{ntok, kHuffPending, fxs + bias, outpos};  // the next header is the next round's
      return kLeanDone;
    }
    if (fe == EV_FULLX) {  // zlib's lookahead: the final block's end-of-block, inside CDATA
      const uint32_t wd = fxs >> 5;
      const uint32_t lo = __builtin_amdgcn_alignbit(W[wd + 1], W[wd], fxs & 31);
      uint32_t e = L.lit[lo & ((1u << kLitRoot) - 1)];
      if (is_long(e))
        e = L.litsub[min((e & 0xffffu) + __builtin_amdgcn_ubfe(lo, kLitRoot, (e >> 16) & 15u),
                         (uint32_t)kLitSubCap - 1)];
      e = rfl(e);
      if (!final_blk || (e >> 26) != K_EOB || fxs + ((e >> 16) & 31) > E) return kLeanOther;
    } else if (fe != EV_FULLO) {
      return kLeanOther;  // an error event, input exhausted, a canonical-decode entry
    }
    h = HuffOut{ntok, kOk, 0u, outpos};
    return kLeanDone;
  }
}

// One round of block bx of the chunk by the lean body at width NT.  A block
// whose round it does not handle is appended to flist for k_huff_fallback
// (launched behind it); the narrow width appends one whose window is larger
// than its stage to the hand-up list instead (nb: blocks of the chunk).
// pstats counts the rounds completed, spread over kPathStatSlots words.
template <int NT>
__device__ __forceinline__ void lean_round(uint8_t* smem, const uint8_t* __restrict__ file,
                                           const BlockInfo* __restrict__ blocks, uint32_t b0, uint64_t chunk_ustart,
                                           uint32_t* __restrict__ tokens, HuffOut* __restrict__ hout,
                                           const uint8_t* __restrict__ tables, const HuffTableInfo* __restrict__ tinfo,
                                           uint32_t round, uint32_t defer, uint32_t* flist, uint32_t* pstats,
                                           uint32_t bx, uint32_t nb) {
  const uint32_t bi = b0 + bx;
  const BlockInfo blk = blocks[bi];
  const uint32_t isize = blk.isize;
  if (isize == 0) {  // inflate(buf,off,0) returns 0 without reading: nothing to validate
    if (threadIdx.x == 0 && round == 0) { hout[bi].ntok = 0; hout[bi].status = kOk; }
    return;
  }
  HuffOut h{0u, kOk, 0u, 0u};
  if (round > 0) {  // only blocks a previous round left pending
    h = hout[bi];
    if (h.status != kHuffPending) return;
  }
  const HuffTableInfo ti = tinfo[bx];
  const int res = lean_block<NT>(smem, file, blk, tokens + (blk.ustart - chunk_ustart), h,
                                 tables + (uint64_t)bx * kTableImage, ti, isize, defer);
  if (threadIdx.x == 0) {
    constexpr uint32_t stat = NT == kNarrowThreads ? kPathStatNarrow : kPathStatLean;
    if (res == kLeanDone) {
      hout[bi] = h;
      atomicAdd(&pstats[stat + (bx % kPathStatSlots) * kPathStatStride], 1u);
    } else if (NT == kNarrowThreads && res == kLeanWide) {
      const uint32_t k = bx % kHuffUpSlots, cap = (nb + kHuffUpSlots - 1) / kHuffUpSlots;
      const uint32_t i = atomicAdd(&flist[kHuffUpCtr + k * kHuffUpStride + round], 1u);
      if (i < cap) flist[kHuffListHdr + nb + k * cap + i] = bx;
    } else {
      flist[kHuffListHdr + atomicAdd(&flist[round], 1u)] = bx;
    }
  }
}

// Phase A, lean instance: one workgroup of NT lanes per BGZF block, one
// DEFLATE block per round.  NT = 256 over the chunk in round 0; in a later
// round NT = 128 over the chunk, then NT = 256, LIST, a fixed grid striding
// over the blocks the narrow launch handed up (grid x = nb otherwise).
template <int NT, bool LIST>
__global__ __launch_bounds__(NT, kLeanWavesPerSimd) void k_inflate_huff(
    const uint8_t* __restrict__ file, const BlockInfo* __restrict__ blocks, uint32_t b0, uint64_t chunk_ustart,
    uint32_t* __restrict__ tokens, HuffOut* __restrict__ hout, const uint8_t* __restrict__ tables,
    const HuffTableInfo* __restrict__ tinfo, uint32_t round, uint32_t defer, uint32_t* flist, uint32_t* pstats,
    uint32_t nb) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[LeanGeom<NT>::kLds];
  if (!LIST) {
    lean_round<NT>(smem, file, blocks, b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, pstats,
                   blockIdx.x, nb);
    return;
  }
  // one index space over the sub-lists, entry i of sub-list k at i * slots + k
  // (the sub-lists are about equally long), so the grid shares the blocks evenly
  const uint32_t cap = (nb + kHuffUpSlots - 1) / kHuffUpSlots;
  uint32_t nmax = 0;
  for (uint32_t k = 0; k < kHuffUpSlots; ++k) nmax = max(nmax, flist[kHuffUpCtr + k * kHuffUpStride + round]);
  nmax = min(rfl(nmax), cap);
  for (uint32_t j = blockIdx.x; j < nmax * kHuffUpSlots; j += gridDim.x) {
    const uint32_t k = j % kHuffUpSlots, i = j / kHuffUpSlots;
    if (i >= rfl(flist[kHuffUpCtr + k * kHuffUpStride + round])) continue;
    const uint32_t bx = rfl(flist[kHuffListHdr + nb + k * cap + i]);
    if (bx < nb)
      lean_round<NT>(smem, file, blocks, b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, pstats,
                     bx, nb);
    __syncthreads();  // the next block's staging overwrites this one's LDS
  }
}

// ---- host launch wrappers (hbam_launch.h)
hipError_t launch_huff_tables(const uint8_t* file, const BlockInfo* blocks, uint32_t b0, uint32_t nb,
                              uint8_t* tables, HuffTableInfo* tinfo, const HuffOut* hout, uint32_t round,
                              hipStream_t s) {
  if (nb == 0) return hipSuccess;
  hipLaunchKernelGGL(k_huff_tables, dim3(nb), dim3(64), 0, s, file, blocks, b0, tables, tinfo, hout, round);
  return hipGetLastError();
}
// phase A proper; the chunk's tables must be built (launch_huff_tables).
hipError_t launch_inflate_huff_prebuilt(const uint8_t* file, const BlockInfo* blocks, uint32_t b0, uint32_t nb,
                                        uint64_t chunk_ustart, uint32_t* tokens, HuffOut* hout,
                                        const uint8_t* tables, const HuffTableInfo* tinfo, uint32_t round,
                                        uint32_t defer, uint32_t* flist, uint32_t* pstats, hipStream_t s) {
  if (nb == 0) return hipSuccess;
  // the lean instance over the chunk (a later round: 128 lanes wide, then the
  // 256-lane one over the blocks handed up, a grid under half the chunk's so
  // that a profile shows one full-size launch per round), then the fallback
  // over the blocks handed over
  if (round == 0 || !kHuffNarrow) {
    hipLaunchKernelGGL((k_inflate_huff<kHuffThreads, false>), dim3(nb), dim3(kHuffThreads), 0, s, file, blocks, b0,
                       chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, pstats, nb);
  } else {
    hipLaunchKernelGGL((k_inflate_huff<kNarrowThreads, false>), dim3(nb), dim3(kNarrowThreads), 0, s, file, blocks,
                       b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, pstats, nb);
    const uint32_t up_grid = std::max(1u, std::min((nb - 1) / 2, kHuffUpGrid));
    hipLaunchKernelGGL((k_inflate_huff<kHuffThreads, true>), dim3(up_grid), dim3(kHuffThreads), 0, s, file, blocks,
                       b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, pstats, nb);
  }
  hipLaunchKernelGGL(k_huff_fallback, dim3(std::min(nb, kHuffFallbackGrid)), dim3(kHuffThreads), 0, s, file, blocks,
                     b0, chunk_ustart, tokens, hout, tables, tinfo, round, defer, flist, nb, pstats);
  return hipGetLastError();
}
hipError_t huff_lean_occupancy(int* workgroups_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(workgroups_per_cu, k_inflate_huff<kHuffThreads, false>,
                                                      kHuffThreads, 0);
}
hipError_t huff_narrow_occupancy(int* workgroups_per_cu, uint32_t* stage_cap_bytes) {
  *stage_cap_bytes = kNarrowStageCap;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(workgroups_per_cu, k_inflate_huff<kNarrowThreads, false>,
                                                      kNarrowThreads, 0);
}

}  // namespace hbam
