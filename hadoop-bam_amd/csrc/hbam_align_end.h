// hbam_align_end.h -- device routine shared by the bounded-traversal filter
// (hbam_query.hip) and the BAM indexer (hbam_bai.hip): the reference length of
// a record's CIGAR, the quantity [htsjdk] getAlignmentEnd and the index's
// record end are made of.  Device code only (included by .hip files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbam_dev_util.h"  // ldu32, wave_sum_u32, kWaveCigarOps
#include "hbam_device.h"

namespace hbam {

// M, D, N, =, X (op codes 0, 2, 3, 7, 8) consume the reference
__device__ __forceinline__ bool consumes_ref(uint32_t op) { return (0x18du >> op) & 1u; }

// Reference length of record i's cigar, wrapping like a Java int; 0 for a
// lane with want == false.  One lane per record; a record whose cigar is
// longer than kWaveCigarOps is summed by its whole wave (the lanes' records of
// that kind one after the other: the loop is uniform, driven by the ballot),
// so EVERY lane of the wave must call this, want or not.
// (a cigar that SILENT let run past its record is read to the record's end only)
__device__ __forceinline__ uint32_t cigar_ref_len(const uint8_t* __restrict__ u, const Columns& c, uint64_t i,
                                                  bool want) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t ncig = 0;
  uint64_t c0 = 0;
  if (want) {
    const uint32_t lrn = c.l_read_name[i], rest = c.rest_len[i];
    ncig = min((uint32_t)c.n_cigar[i], rest > lrn ? (rest - lrn) >> 2 : 0u);
    c0 = c.rest_off[i] + lrn;
  }
  const bool lng = want && ncig > kWaveCigarOps;
  uint32_t rl = 0;
  if (want && !lng) {
    for (uint32_t k = 0; k < ncig; ++k) {
      const uint32_t w = ldu32(u, c0 + 4ull * k);
      if (consumes_ref(w & 0xfu)) rl += w >> 4;
    }
  }
  for (unsigned long long m = __ballot(lng); m; m &= m - 1) {
    const int src = __ffsll((long long)m) - 1;
    const uint64_t b = (uint64_t)(uint32_t)__shfl((int)(uint32_t)c0, src, 64) |
                       ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(c0 >> 32), src, 64) << 32);
    const uint32_t nc = (uint32_t)__shfl((int)ncig, src, 64);
    uint32_t part = 0;
    for (uint32_t k = lane; k < nc; k += 64) {
      const uint32_t w = ldu32(u, b + 4ull * k);
      if (consumes_ref(w & 0xfu)) part += w >> 4;
    }
    part = wave_sum_u32(part);
    if ((int)lane == src) rl = part;
  }
  return rl;
}

}  // namespace hbam
