// The device-only scan's gather layout: which bytes of a segment the host
// confirmer must see, and where they land in the gather buffer.  Pure
// arithmetic on the offsets array and the per-file need flags -- no HIP, no
// device -- so it is the CPU model the device scan (gather.hip:
// tsg_gather_scan) is compared with (tsg_test_plan_gather,
// tests/test_gather_plan.py).
//
// A run is a maximal sequence of consecutive non-lead files with need = 1.
// Its source span starts at the K1 chunk boundary at or below its first file
// (the confirmer's line numbers count '\n' from that boundary:
// CensoredView::prefix_at) and ends with its last file.  Runs land one after
// the other, each on a 64-byte boundary; the copy moves whole 16-byte words.
#pragma once
#include <cstdint>
#include <vector>

namespace tsg {

constexpr uint64_t kGatherNone = ~uint64_t(0);   // goff of a file that is not gathered
constexpr uint64_t kGatherAlign = 64;            // a run's destination alignment

// One run: bytes [src, src + len) of the segment's frame (byte 0 = the K1
// chunk grid's origin) go to [dst, dst + len) of the gather buffer; the copy
// itself moves len rounded up to 16 bytes.
struct GatherRun { uint64_t src, dst, len; };

struct GatherPlan {
  std::vector<uint64_t> goff;        // per file: its first byte in the gather buffer, or kGatherNone
  std::vector<GatherRun> runs;
  uint64_t total = 0;                // bytes of the buffer the runs take (a multiple of 64)
};

// (constexpr: the device scan calls it too)
constexpr uint64_t gather_round(uint64_t n) { return (n + kGatherAlign - 1) & ~(kGatherAlign - 1); }

// offsets: nfiles + 1 frame offsets; files below `lead` are never gathered;
// need: one byte per file (non-zero = gather); chunk: the segment's K1 chunk bytes.
inline void plan_gather(const uint64_t* offsets, uint32_t nfiles, uint32_t lead, const uint8_t* need, uint32_t chunk,
                        GatherPlan* out) {
  out->goff.assign(nfiles, kGatherNone);
  out->runs.clear();
  uint64_t dst = 0;
  for (uint32_t f = lead; f < nfiles;) {
    if (!need[f]) { ++f; continue; }
    uint32_t e = f;
    while (e + 1 < nfiles && need[e + 1]) ++e;
    const uint64_t src = offsets[f] / chunk * chunk;
    const uint64_t len = offsets[e + 1] - src;
    for (uint32_t k = f; k <= e; ++k) out->goff[k] = dst + (offsets[k] - src);
    out->runs.push_back(GatherRun{src, dst, len});
    dst += gather_round(len);
    f = e + 1;
  }
  out->total = dst;
}

}  // namespace tsg
