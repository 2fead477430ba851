// Device side of the gzip inflate (inflate.hip): the call behind
// tsg_inflate_gzip_device.  No HIP types here: capi.cpp includes it.
#pragma once
#include <cstdint>
#include <string>

#include "inflate.h"

namespace tsg {

// Kernel times and counts of one call (tools/inflate_probe.py)
struct InflateStats {
  double inflate_ms = 0, crc_ms = 0;
  uint64_t members = 0, slices = 0;
};

// Inflate nstreams gzip streams d_gz[gz_off[i], gz_off[i + 1]) into the slots
// d_dst[dst_off[i], dst_off[i + 1]) on the device that holds d_gz; out_lens and
// status (host arrays of nstreams) are filled for every stream.  Synchronous.
// false: the call itself failed -- *err starts with "inflate:" when an
// argument is at fault, else a HIP error; a stream that fails is not a failed
// call.
bool inflate_gzip_device(const void* d_gz, const uint64_t* gz_off, uint32_t nstreams, void* d_dst,
                         const uint64_t* dst_off, uint64_t* out_lens, int32_t* status, InflateStats* st,
                         std::string* err);

}  // namespace tsg
