// Device side of the zstd decode (zstdec.hip): the call behind
// tsg_inflate_zstd_device.  No HIP types here: capi.cpp includes it.
#pragma once
#include <cstdint>
#include <mutex>
#include <string>

#include "zstdec.h"

namespace tsg {

// Kernel times and counts of one call (tools/zstd_probe.py)
struct ZstdStats {
  double decode_ms = 0, hash_ms = 0;
  uint64_t frames = 0, blocks = 0;
};

// The literal scratch: 128 KiB of device memory per stream of the largest
// call so far, kept on the engine from call to call.  A call holds mu while
// its kernels run.
struct ZstdScratch {
  std::mutex mu;
  void* lits = nullptr;
  size_t bytes = 0;
  int device = -1;
  ZstdScratch() = default;
  ZstdScratch(const ZstdScratch&) = delete;
  ZstdScratch& operator=(const ZstdScratch&) = delete;
  ~ZstdScratch();
};

// Decode nstreams zstd streams d_z[z_off[i], z_off[i + 1]) into the slots
// d_dst[dst_off[i], dst_off[i + 1]) on the device that holds d_z; out_lens and
// status (host arrays of nstreams) are filled for every stream.  Synchronous.
// false: the call itself failed -- *err starts with "zstd:" when an argument
// is at fault, else a HIP error; a stream that fails is not a failed call.
bool inflate_zstd_device(ZstdScratch* keep, const void* d_z, const uint64_t* z_off, uint32_t nstreams, void* d_dst,
                         const uint64_t* dst_off, uint64_t* out_lens, int32_t* status, ZstdStats* st, std::string* err);

}  // namespace tsg
