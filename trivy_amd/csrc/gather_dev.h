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

// With windows (gather.h plan_gather_windows).  The scratch: one device
// allocation of gather_windows_scratch_bytes, laid out by
// gather_windows_scratch_layout (the launch zeroes it).
struct GatherWindowScratch {
  uint64_t *tot_m, *pad_m, *tot_s, *pad_s;   // marked chunks and run starts in all, and the scans' pad words
  uint8_t *any, *whole;                      // per file
  uint32_t* cnt;                             // per file: marked chunks under a windowed file
  uint64_t *base_m, *base_s;                 // per region: marked chunks / run starts in front of it
  uint32_t *region_m, *region_s;
  uint8_t* marks;                            // per chunk, whole regions and one region of zeros behind them
};
size_t gather_windows_scratch_bytes(uint64_t nchunks, uint32_t nfiles);
GatherWindowScratch gather_windows_scratch_layout(void* scratch, uint64_t nchunks, uint32_t nfiles);

// Enqueue on `s`, behind the segment's final K2: the files' classes (cls:
// nfiles bytes), the run table (runs: room for runs_cap) and meta as
// gather_plan_launch's, from K2's candidate list, the file flags, `all`, the
// windowable byte per rule-table row (wrows, nrows) and the window options.
// total: the segment's bytes.  A table of more than runs_cap runs stores
// nothing past it and sets meta[1] to UINT64_MAX (the copy then writes nothing).
// Here meta has four words: with o.line_cap != 0 (gather.h line_window)
// tsg_gw_lines leaves in [2] the candidates it widened and in [3] those that
// ended at the cap; both are zero otherwise.  That pass reads the segment's
// frame (data: 16-byte aligned, 16 readable bytes past its end, chunk 0 at
// byte 0) and K1's '\n' count per chunk (nl), and is timed between
// lines_begin and lines_end where given.  It needs no scratch of its own.
bool gather_windows_launch(const void* cands, const uint32_t* ncands, uint32_t cand_cap, const uint32_t* fflags,
                           const uint64_t* offsets, uint32_t nfiles, uint32_t lead, bool all, const uint8_t* wrows,
                           uint32_t nrows, uint32_t chunk, uint64_t total, const GatherWindowOpts& o,
                           const GatherWindowScratch& sc, uint8_t* cls, GatherRun* runs, uint64_t runs_cap,
                           uint64_t* meta, hipStream_t s, std::string* err, const uint8_t* data = nullptr,
                           const uint16_t* nl = nullptr, hipEvent_t lines_begin = nullptr,
                           hipEvent_t lines_end = nullptr);

// Enqueue on `s`: the runs' bytes from the segment's frame (src, 16-byte
// aligned, 16 readable bytes past its end) into dst (host-mapped, cap bytes).
// Writes nothing when gather_total exceeds cap.  blocks_max: the grid's limit.
bool gather_copy_launch(const uint8_t* src, const GatherRun* runs, const uint64_t* meta, uint8_t* dst, uint64_t cap,
                        uint32_t blocks_max, hipStream_t s, std::string* err);

}  // namespace tsg
