// hbam_abi_util.h -- what the two halves of the extern "C" boundary share:
// hbam_abi.cpp (the product API on hbam_ctx) and hbam_abi_gpu.cpp (the
// device-resident decode on hbam_gpu, include/hbam.h's benchmark block).
#pragma once
#include "../../include/hbam.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hbam_host.h"

namespace hbam_abi {
using hadoop_bam::BamFile;

// the last error of a call with no ctx (open, compress, codec): per thread,
// as JNI callers from many executor threads read it right after their call
extern thread_local std::string g_open_err;

// hipEventCreate x 2 ... hipEventDestroy x 2 around one timed stretch of a stream
struct EventPair {
  hipEvent_t e0{}, e1{};
  EventPair() {
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
  }
  ~EventPair() {
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  void start(hipStream_t s) { (void)hipEventRecord(e0, s); }
  // records the end, waits for it: the milliseconds since start (0 if the events failed)
  float stop_ms(hipStream_t s) {
    float ms = 0;
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
  }
};

// A malloc'ed copy of v for the caller (hbam_free): at least one byte, so
// that an empty result is not NULL.  *n = v's elements.
template <class T>
int copy_out(const std::vector<T>& v, T** buf, uint64_t* n) {
  *buf = static_cast<T*>(malloc(v.empty() ? 1 : v.size() * sizeof(T)));
  if (!*buf) return HBAM_E_NOMEM;
  if (!v.empty()) memcpy(*buf, v.data(), v.size() * sizeof(T));
  *n = v.size();
  return HBAM_OK;
}

inline int check_device(int device) {
  if (device >= 0 && device < hbam_device_count()) return HBAM_OK;
  g_open_err = "no HIP device " + std::to_string(device);
  return HBAM_E_DEVICE;
}

// hbam_set_locate / hbam_gpu_set_locate and the counter getters of both handles, over the file or its pipeline
inline void set_locate(BamFile& f, uint64_t seg_bytes, uint32_t cap_limit) {
  hbam::Pipeline& p = f.pipe();
  if (seg_bytes == HBAM_LOCATE_SEG_DEFAULT) {
    seg_bytes = hbam::kLocateSegBytes;
    if (const char* e = getenv("HBAM_LOCATE_SEG")) seg_bytes = strtoull(e, nullptr, 0);
  }
  p.set_locate(seg_bytes, cap_limit);
  f.invalidate_window();
}

inline void locate_counters(const hbam::Pipeline& p, uint64_t out[2]) {
  out[0] = p.locate_anchored();
  out[1] = p.locate_declined();
}

inline void sort_name_counters(const hbam::Pipeline& p, uint64_t out[3]) {
  for (int i = 0; i < 3; ++i) out[i] = p.name_counters()[i];
}

// hbam_decode_span_device / hbam_gpu_run (hbam_abi_gpu.cpp)
int decode_device(BamFile& f, uint64_t vstart, uint64_t vend, int32_t flags, hbam_gpu_stats* st, hbam::SpanDev* last,
                  std::string* err);
// hbam_chain_lists (hbam_abi_gpu.cpp, with the measurement-only entry points)
int chain_lists(BamFile& f, uint64_t** g, uint64_t** x, uint32_t** wcnt, uint16_t** list, uint64_t* n_blocks,
                uint64_t* n_list, uint32_t* stage);
}  // namespace hbam_abi
