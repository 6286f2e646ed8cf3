// hbam_record_dev.h -- device routines the record chain (hbam_chain.hip) and
// the record output kernels (hbam_records.hip) both use: a record's fields and
// sort key into the columns, and the gate of a speculative launch.  Device
// code only (included by .hip files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbam_dev_util.h"
#include "hbam_device.h"

namespace hbam {

// ---------------------------------------------------------------------------
// Fused record decode: SoA columns + BAMRecordReader.getKey
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// MurmurHash3.murmurhash3(byte[], seed) (util/MurmurHash3.java:32-102) over
// len bytes of u at off.
__device__ inline uint64_t murmur3_dev(const uint8_t* u, uint64_t off, uint32_t len, int32_t seed) {
  const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
  uint64_t h1 = (uint64_t)(int64_t)seed, h2 = h1;
  const uint32_t nblocks = len / 16;
  for (uint32_t i = 0; i < nblocks; ++i) {
    uint64_t k1 = ldu64(u, off + 16ull * i), k2 = ldu64(u, off + 16ull * i + 8);
    k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = (h2 << 31) | (h1 >> 33); h2 += h1; h2 = h2 * 5 + 0x38495ab5;  // :59
  }
  const uint64_t t = off + 16ull * nblocks;
  const uint32_t r = len & 15;
  if (r) {
    // tail bytes via two 8-byte loads (padding makes the over-read safe), masked
    uint64_t lo = ldu64(u, t), hi = ldu64(u, t + 8);
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
  return h1;
}

// Fields + key of the record at q into slot i of the columns.
__device__ __forceinline__ void decode_record_h(const uint8_t* __restrict__ u, uint64_t q, uint64_t i,
                                                const Columns& col, const RecHead& h) {
  const int32_t bs = (int32_t)h.at(0);
  const int32_t ref = (int32_t)h.at(1);
  const int32_t pos = (int32_t)h.at(2);
  const uint32_t w12 = h.at(3);
  const uint32_t w16 = h.at(4);
  const int32_t lseq = (int32_t)h.at(5);
  const int32_t nref = (int32_t)h.at(6);
  const int32_t npos = (int32_t)h.at(7);
  const int32_t tlen = (int32_t)h.at(8);
  const uint16_t flag = (uint16_t)(w16 >> 16);
  col.ref_id[i] = ref;
  col.pos[i] = pos;
  col.l_read_name[i] = (uint8_t)w12;
  col.mapq[i] = (uint8_t)(w12 >> 8);
  col.bin[i] = (uint16_t)(w12 >> 16);
  col.n_cigar[i] = (uint16_t)w16;
  col.flag[i] = flag;
  col.l_seq[i] = lseq;
  col.next_ref_id[i] = nref;
  col.next_pos[i] = npos;
  col.tlen[i] = tlen;
  col.rest_off[i] = q + 36;
  col.rest_len[i] = (uint32_t)(bs - 32);
  // BAMRecordReader.getKey (:81-121): alignmentStart = pos+1
  const int32_t start = (int32_t)((uint32_t)pos + 1u);
  int64_t key;
  if (!((flag & 4) || ref < 0 || start < 0)) {
    key = (int64_t)(((uint64_t)(int64_t)ref << 32) | (uint64_t)(int64_t)(int32_t)(start - 1));
  } else {
    if (col.long_rec && (uint32_t)(bs - 32) > kLongHash) {  // long rest: k_long_hash
      const uint32_t slot = atomicAdd(col.long_n, 1u);
      if (slot < col.long_cap) {
        col.long_rec[slot] = i;
        return;
      }
    }
    const int32_t mh = (int32_t)murmur3_dev(u, q + 36, (uint32_t)(bs - 32), 0);
    key = (int64_t)((0x7fffffffull << 32) | (uint64_t)(int64_t)mh);
  }
  col.key[i] = key;
}
__device__ __forceinline__ void decode_record(const uint8_t* __restrict__ u, uint64_t q, uint64_t i,
                                              const Columns& col) {
  decode_record_h(u, q, i, col, load_head(u, q));
}

// The gate of a speculative launch (queued before the host has read
// k_rec_check_out's verdict): it runs only if no block stopped the span
// (*bad == ~0) and no record needs bytes past the inflated range; otherwise
// rec_pos past the stop may be stale and the host launches it again.
struct SpecGate {
  const unsigned long long* bad = nullptr;  // nullptr: no gate
  const unsigned long long* need = nullptr;
  uint64_t e_inf = 0;
};
__device__ __forceinline__ bool gate_closed(const SpecGate& g) {
  return g.bad && (*g.bad != ~0ull || *g.need > g.e_inf);
}

}  // namespace hbam
