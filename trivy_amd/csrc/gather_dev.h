// Device side of the device-only scan's gather (gather.hip): launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "gather.h"

namespace tsg {

// meta: two uint64 on the device -- [0] the number of runs, [1] gather_total.
constexpr uint32_t kGatherTile = 4096;     // destination bytes per workgroup step of tsg_gather_copy

// Enqueue on `s`, behind the segment's final K2: need[] from K2's candidate
// list (16-byte records whose first dword is the file; *ncands of them, at
// most cand_cap stored), the file flags and `all` (a mode-1 rule: every
// file); then the run layout (goff, runs, meta) as plan_gather gives it.
// need: nfiles bytes; goff: nfiles uint64; runs: room for (nfiles + 1) / 2 + 1.
bool gather_plan_launch(const void* cands, const uint32_t* ncands, uint32_t cand_cap, const uint32_t* fflags,
                        const uint64_t* offsets, uint32_t nfiles, uint32_t lead, bool all, uint32_t chunk,
                        uint8_t* need, uint64_t* goff, GatherRun* runs, uint64_t* meta, hipStream_t s,
                        std::string* err);

// Enqueue on `s`: the runs' bytes from the segment's frame (src, 16-byte
// aligned, 16 readable bytes past its end) into dst (host-mapped, cap bytes).
// Writes nothing when gather_total exceeds cap.  blocks_max: the grid's limit.
bool gather_copy_launch(const uint8_t* src, const GatherRun* runs, const uint64_t* meta, uint8_t* dst, uint64_t cap,
                        uint32_t blocks_max, hipStream_t s, std::string* err);

}  // namespace tsg
