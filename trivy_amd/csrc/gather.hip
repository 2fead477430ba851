// Device-only scans (the batch exists only in HBM): after a segment's final K2
// the GPU decides which files the host confirmer must see and compacts exactly
// those into host-mapped memory, so nothing else of the batch crosses the link.
//
//   tsg_gather_mark   need[f] = 1 for every file of K2's candidate list, every
//                     file with a flag word (fold-special content), or every
//                     file (a mode-1 rule); leads never
//   tsg_gather_scan   one workgroup over the files: the runs of needed files,
//                     their 64-byte aligned destinations, goff[f], the totals
//                     (gather.h plan_gather is its CPU model)
//   tsg_gather_copy   the runs' bytes, 16 bytes per load and store, one 4 KiB
//                     destination tile per workgroup step: a tile finds its run
//                     by binary search, so a 64 MB file among ten-byte files is
//                     spread over the whole grid
// The destination is host-mapped coherent memory; the stores go over the link
// themselves (as tsg_readback's), with no copy engine and no second round trip.
#include "gather_dev.h"

namespace tsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void tsg_gather_mark(const uint4* __restrict__ cands,
                                                       const uint32_t* __restrict__ ncands, uint32_t cand_cap,
                                                       const uint32_t* __restrict__ fflags, uint32_t nfiles,
                                                       uint32_t lead, uint32_t all, uint8_t* __restrict__ need) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  const uint32_t n = min(*ncands, cand_cap);       // (K2 counts past a full list; an overflow is run again)
  for (uint32_t i = tid; i < n; i += step) {
    const uint32_t f = cands[i].x;
    if (f >= lead && f < nfiles) need[f] = 1;      // (several threads may store the same 1)
  }
  for (uint32_t f = lead + tid; f < nfiles; f += step)
    if (all || fflags[f] != 0) need[f] = 1;        // (any flag word makes a file one the confirmer reads: plan_confirm)
}

// inclusive prefix sum of v over the workgroup's 1024 threads
__device__ __forceinline__ uint64_t block_incl_scan(uint64_t v, uint64_t* part) {
  const uint32_t t = threadIdx.x;
  part[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t u = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += u;
    __syncthreads();
  }
  return part[t];
}

// One workgroup; thread t owns a contiguous range of files, then of runs.
// Run k is the k-th run start in file order, so a thread knows the index of
// the run a file belongs to from the run starts before its range.
__global__ __launch_bounds__(1024) void tsg_gather_scan(const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                        const uint8_t* __restrict__ need, uint32_t chunk,
                                                        uint64_t* __restrict__ goff, GatherRun* runs,
                                                        uint64_t* __restrict__ meta) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nfiles + 1023u) / 1024u;
  const uint32_t b = min(nfiles, t * per), e = min(nfiles, b + per);
  auto needed = [&](uint32_t f) { return f >= lead && f < nfiles && need[f] != 0; };
  uint32_t ns = 0;
  for (uint32_t f = b; f < e; ++f) ns += needed(f) && (f == 0 || !needed(f - 1));
  const uint32_t base = static_cast<uint32_t>(block_incl_scan(ns, part)) - ns;
  const uint32_t nruns = static_cast<uint32_t>(part[1023]);
  __syncthreads();
  // each run's source start, and (in len, for now) its end
  uint32_t c = base;
  for (uint32_t f = b; f < e; ++f) {
    if (!needed(f)) continue;
    if (f == 0 || !needed(f - 1)) runs[c++].src = off[f] / chunk * chunk;
    if (!needed(f + 1)) runs[c - 1].len = off[f + 1];
  }
  __syncthreads();
  // destinations: the prefix of the runs' sizes rounded up to 64 bytes
  const uint32_t rper = (nruns + 1023u) / 1024u;
  const uint32_t rb = min(nruns, t * rper), re = min(nruns, rb + rper);
  uint64_t sz = 0;
  for (uint32_t k = rb; k < re; ++k) sz += gather_round(runs[k].len - runs[k].src);
  uint64_t dst = block_incl_scan(sz, part) - sz;
  const uint64_t total = part[1023];
  for (uint32_t k = rb; k < re; ++k) {
    const uint64_t len = runs[k].len - runs[k].src;
    runs[k].dst = dst;
    runs[k].len = len;
    dst += gather_round(len);
  }
  __syncthreads();
  c = base;
  for (uint32_t f = b; f < e; ++f) {
    if (!needed(f)) { goff[f] = kGatherNone; continue; }
    if (f == 0 || !needed(f - 1)) ++c;
    goff[f] = runs[c - 1].dst + (off[f] - runs[c - 1].src);
  }
  if (t == 0) { meta[0] = nruns; meta[1] = total; }
}

__global__ __launch_bounds__(256) void tsg_gather_copy(const uint8_t* __restrict__ src,
                                                       const GatherRun* __restrict__ runs,
                                                       const uint64_t* __restrict__ meta, uint8_t* __restrict__ dst,
                                                       uint64_t cap) {
  const uint32_t nruns = static_cast<uint32_t>(meta[0]);
  const uint64_t total = meta[1];
  if (nruns == 0 || total > cap) return;          // (too small a buffer: the host grows it and launches again)
  const uint64_t ntiles = (total + kGatherTile - 1) / kGatherTile;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = tile * kGatherTile;
    // the last run that starts at or below the tile (the same for every thread)
    uint32_t lo = 0, hi = nruns;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (runs[mid].dst <= t0) lo = mid; else hi = mid;
    }
    const uint64_t d = t0 + threadIdx.x * 16u;
    if (d >= total) continue;                      // (total is a multiple of 64: d + 16 <= total <= cap)
    // and at or below this thread's 16 bytes: that run unless another starts in the tile
    if (lo + 1 < nruns && runs[lo + 1].dst <= d) {
      hi = nruns;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (runs[mid].dst <= d) lo = mid; else hi = mid;
      }
    }
    const uint64_t r_src = runs[lo].src, r_dst = runs[lo].dst, r_len = runs[lo].len;
    const uint64_t o = d - r_dst;
    if (o >= r_len) continue;                      // the padding between two runs
    // (o is a multiple of 16 below len: at most 15 bytes past the run's end are read)
    const v4u w = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(src + r_src + o));
    *reinterpret_cast<v4u*>(dst + d) = w;
  }
}

}  // namespace

bool gather_plan_launch(const void* cands, const uint32_t* ncands, uint32_t cand_cap, const uint32_t* fflags,
                        const uint64_t* offsets, uint32_t nfiles, uint32_t lead, bool all, uint32_t chunk,
                        uint8_t* need, uint64_t* goff, GatherRun* runs, uint64_t* meta, hipStream_t s,
                        std::string* err) {
  hipError_t e = hipMemsetAsync(need, 0, nfiles ? nfiles : 1, s);
  if (e == hipSuccess) {
    const uint32_t n = nfiles > cand_cap ? nfiles : cand_cap;
    const uint32_t blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
    hipLaunchKernelGGL(tsg_gather_mark, dim3(blocks ? blocks : 1), dim3(256), 0, s, static_cast<const uint4*>(cands),
                       ncands, cand_cap, fflags, nfiles, lead, all ? 1u : 0u, need);
    hipLaunchKernelGGL(tsg_gather_scan, dim3(1), dim3(1024), 0, s, offsets, nfiles, lead,
                       static_cast<const uint8_t*>(need), chunk, goff, runs, meta);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { *err = std::string("gather launch: ") + hipGetErrorString(e); return false; }
  return true;
}

bool gather_copy_launch(const uint8_t* src, const GatherRun* runs, const uint64_t* meta, uint8_t* dst, uint64_t cap,
                        uint32_t blocks_max, hipStream_t s, std::string* err) {
  const uint64_t tiles = (cap + kGatherTile - 1) / kGatherTile;
  const uint32_t blocks = static_cast<uint32_t>(tiles < blocks_max ? tiles : blocks_max);
  hipLaunchKernelGGL(tsg_gather_copy, dim3(blocks ? blocks : 1), dim3(256), 0, s, src, runs, meta, dst, cap);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("gather copy launch: ") + hipGetErrorString(e); return false; }
  return true;
}

}  // namespace tsg
