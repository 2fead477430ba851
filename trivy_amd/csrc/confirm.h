// What the host confirmation (confirm.cpp) takes from a segment's GPU passes,
// in plain host types: no HIP here, so the confirmation builds with the host
// compiler alone and runs under the host sanitizers (tools/asan_check.py).
#pragma once
#include <chrono>
#include <cstdint>
#include <memory>
#include <vector>

#include "gather.h"
#include "threadpool.h"

namespace tsg {

// A candidate as the host sees it (the device's record of the same layout
// becomes one in GpuOut::finish_copy, engine.hip, and nowhere else).
struct Cand { uint32_t file, rule; uint64_t start; };

// GPU results of one segment as the host confirmer reads them (the engine's
// GpuOut adds what belongs to the lane and the device).
struct SegmentOut {
  std::vector<Cand> cands;      // (file, rule, start) candidates, unsorted
  std::vector<uint16_t> nl;     // '\n' count per K1 chunk
  std::vector<uint32_t> ff;     // per-file flags (fold-special content)
  uint32_t chunk = 0;           // K1 chunk bytes of this segment (nl[] granularity)
  // device-only scans: where each file's bytes are in the gather buffer, and
  // what the gather took.  gbase: the buffer's host address (the CPU model
  // sets one of its own).
  const uint8_t* gbase = nullptr;
  bool gathered = false;
  uint64_t gather_total = 0, gather_files = 0;
  std::vector<uint64_t> goff;
  // ... with windows (tsg_device_scan_opts; gather.h plan_gather_windows): the
  // run table and the files' classes instead of goff, which confirm_segment
  // derives for the whole files.  run_base (the CPU model only): run k's
  // bytes are at run_base[k], an allocation of their own, not at gbase + dst.
  // insufficient (out): the windowed files whose confirmation would have read
  // outside their runs, ascending; they have no result yet.
  bool windowed = false;
  std::vector<uint8_t> gcls;
  std::vector<GatherRun> wruns;
  std::vector<const uint8_t*> run_base;
  std::vector<uint32_t> insufficient;
  uint64_t window_files = 0;
  // the confirmation's plan (plan_confirm): candidates grouped per file, the
  // files to confirm (largest first) and the rest.  (Built on the driver
  // thread it delayed the next piece's launch by as much as it saved the
  // confirming thread: profiles/rd4q_bench_c3prof.log; it is now built while
  // the next piece's passes run.)
  bool planned = false;
  std::vector<uint32_t> per_file, work, light;
  std::vector<Cand> sorted;
};

// One call's host confirm resources.
// The pool is created at the call's first confirmation that needs it: per-file
// Scan batches (a few files, confirmed inline on the calling thread) never
// start one, so the queue's up to max_inflight concurrent batches hold a lane
// each but no idle confirm threads.
struct CallCtx {
  std::unique_ptr<ThreadPool> pool;
  int nt = 1;
  ThreadPool& get() {
    if (!pool || pool->size() != nt) pool.reset(new ThreadPool(nt));
    return *pool;
  }
};

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace tsg
