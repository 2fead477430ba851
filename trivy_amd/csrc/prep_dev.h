// Device side of the raw-batch preparation (prep.hip): scratch layout and launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "prep.h"

namespace tsg {

// Where the pass keeps its arrays in one device scratch buffer.  The host
// uploads offsets (nfiles + 1), flags (nfiles) and the printable table (8
// dwords) before the launch and reads total, new_off and kinds after it.
struct PrepScratch {
  uint64_t* total;        // prepared bytes
  uint32_t* print_tab;    // 8 dwords
  uint64_t* offsets;      // nfiles + 1
  uint64_t* new_off;      // nfiles + 1
  uint64_t* region_base;  // per 64 KiB region: output position of its first byte
  uint32_t* region_n;     // per region: bytes it emits
  uint32_t* first;        // per region: the first file that starts after its first byte
  uint8_t* flags;         // nfiles
  uint8_t* kinds;         // nfiles
};
size_t prep_scratch_bytes(uint64_t total, uint32_t nfiles);
PrepScratch prep_scratch_layout(void* scratch, uint64_t total, uint32_t nfiles);

// Enqueue on `s`: classify, count, scan, compact.  src, dst: 16-byte aligned
// device buffers, src read only below `total` (= offsets[nfiles]), dst of
// dst_cap bytes.  dst receives the prepared bytes and 64 zero bytes behind
// them; when they do not fit, dst is not written at all (sc.total still tells
// the size).  The offsets are the host's, checked there (nondecreasing from
// 0).  pass_ev (may be NULL): 5 events recorded around the four passes.
bool prep_launch(const uint8_t* src, uint64_t total, uint32_t nfiles, uint8_t* dst, uint64_t dst_cap,
                 const PrepScratch& sc, hipStream_t s, hipEvent_t* pass_ev, std::string* err);

// The skeleton's middle pass for another compaction (tarscan.hip): region_base[r]
// = region_n[0] + ... + region_n[r - 1], *total = the sum.  pad: two device
// words, pad[0] = 0 (the scan takes them as an empty batch's offsets and new
// starts and sets pad[1] = 0).
void region_scan_launch(const uint32_t* region_n, uint32_t nregions, uint64_t* region_base, uint64_t* total,
                        uint64_t* pad, hipStream_t s);

}  // namespace tsg
