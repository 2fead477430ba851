// Device side of the layer-tar walk (tarscan.hip): scratch layout and launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "tarscan.h"

namespace tsg {

// Where the pass keeps its arrays in one device scratch buffer (zeroed by the
// launch).  The host reads total after it.
struct TarScanScratch {
  uint64_t* total;        // marked blocks
  uint64_t* pad;          // two words the shared scan kernel takes as an empty batch's offsets / new starts
  uint64_t* region_base;  // per region of 128 blocks (64 KiB): marked blocks before it
  uint32_t* region_n;     // per region: its marked blocks
  uint8_t* marks;         // per block (padded to whole regions): plan_tar_marks' byte
};
size_t tar_scan_scratch_bytes(uint64_t len);
TarScanScratch tar_scan_scratch_layout(void* scratch, uint64_t len);

// Enqueue on `s`: mark, count, scan, compact over the whole blocks of
// tar[0, len) (16-byte aligned device memory; nothing at or past len is
// read).  The marked blocks go in order to out_blocks (512 bytes each) and
// their block numbers to out_idx, both of cap_blocks entries (device-visible
// memory); when there are more than cap_blocks, neither is written
// (sc.total still tells the count).
bool tar_scan_launch(const uint8_t* tar, uint64_t len, const TarScanScratch& sc, uint8_t* out_blocks,
                     uint64_t* out_idx, uint64_t cap_blocks, hipStream_t s, std::string* err);

}  // namespace tsg
