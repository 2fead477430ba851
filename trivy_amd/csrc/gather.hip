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
//
// With windows (tsg_device_scan_opts; gather.h plan_gather_windows is the CPU
// model, pass for pass) the layout is made on the segment's K1 chunk grid:
//   tsg_gw_flags     per candidate: its file has one; it needs the whole file
//                    (a row that is not windowable, a start at or past the
//                    file's length -- kFullScanStart among them)
//   tsg_gw_class     per file: none / whole / windowed before the windows are
//                    counted; a windowed file's head chunk is marked
//   tsg_gw_windows   per candidate of a windowed file: its window's chunks
//   tsg_gw_lines     in its place with a line cap: a wave per candidate widens
//                    the window to the lines the confirmer reads, from the
//                    bytes at the window's ends and K1's per-chunk '\n' counts
//   tsg_gw_count     per marked chunk: one more for every windowed file on it
//   tsg_gw_demote    per file: windows on more than half of its chunks -> whole
//   tsg_gw_fill      per chunk: marked when a whole file lies on it
//   tsg_gw_regions   per region of 128 chunks: its marked chunks and run starts
//   tsg_prep_scan    twice (region_scan_launch): the regions' prefixes
//   tsg_gw_runs      one wave per region: each run start's (src, dst), each
//                    run end's last byte
//   tsg_gw_finish    per run: its length; the totals
// and the copy is tsg_gather_copy over that run table.  Every index that
// comes from a candidate is bounded before it is used: the file by [lead,
// nfiles), the start by the file's length, the chunks by the file's own.
#include "gather_dev.h"
#include "prep_dev.h"

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


// ---------------------------------------------------------------- windows
constexpr uint32_t kGwRegion = 128;          // chunks per region (one wave, two chunks per lane)
constexpr uint32_t kGwWaves = 4;

__global__ __launch_bounds__(256) void tsg_gw_flags(const uint4* __restrict__ cands, const uint32_t* __restrict__ ncands,
                                                    uint32_t cand_cap, const uint64_t* __restrict__ off,
                                                    uint32_t nfiles, uint32_t lead,
                                                    const uint8_t* __restrict__ wrows, uint32_t nrows,
                                                    uint8_t* __restrict__ any, uint8_t* __restrict__ whole) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  const uint32_t n = min(*ncands, cand_cap);       // (as tsg_gather_mark: an overflowed list is run again)
  for (uint32_t i = tid; i < n; i += step) {
    const uint4 c = cands[i];
    const uint32_t f = c.x, rule = c.y;
    if (f < lead || f >= nfiles) continue;
    any[f] = 1;
    const uint64_t start = c.z | (static_cast<uint64_t>(c.w) << 32);
    const uint64_t len = off[f + 1] - off[f];
    if (rule >= nrows || wrows[rule] == 0 || start >= len) whole[f] = 1;
  }
}

__global__ __launch_bounds__(256) void tsg_gw_class(const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                    const uint32_t* __restrict__ fflags, uint32_t all,
                                                    uint64_t min_file, const uint8_t* __restrict__ any,
                                                    const uint8_t* __restrict__ whole, uint8_t* __restrict__ cls,
                                                    uint8_t* __restrict__ marks, uint32_t chunk, uint64_t nchunks) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (uint32_t f = lead + tid; f < nfiles; f += step) {
    const uint64_t o = off[f], len = off[f + 1] - o;
    const bool special = all || fflags[f] != 0;
    uint8_t c = kGatherClassNone;
    if (special || any[f]) {
      const bool w = special || whole[f] || len < min_file || len == 0;
      c = w ? kGatherClassWhole : kGatherClassWindow;
      if (!w && o / chunk < nchunks) marks[o / chunk] = 1;     // (len > 0: the chunk exists)
    }
    cls[f] = c;
  }
}

__global__ __launch_bounds__(256) void tsg_gw_windows(const uint4* __restrict__ cands,
                                                      const uint32_t* __restrict__ ncands, uint32_t cand_cap,
                                                      const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                      const uint8_t* __restrict__ cls, uint8_t* __restrict__ whole,
                                                      uint8_t* __restrict__ marks, uint32_t chunk, uint64_t nchunks,
                                                      uint32_t before, uint32_t after) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  const uint32_t n = min(*ncands, cand_cap);
  for (uint32_t i = tid; i < n; i += step) {
    const uint4 c = cands[i];
    const uint32_t f = c.x;
    if (f < lead || f >= nfiles || cls[f] != kGatherClassWindow) continue;
    const uint64_t start = c.z | (static_cast<uint64_t>(c.w) << 32);
    const uint64_t o = off[f], len = off[f + 1] - o;
    if (start >= len) continue;                    // (tsg_gw_flags made such a file whole: never reached)
    uint64_t lo, hi;
    window_chunks(o, len, start, before, after, chunk, &lo, &hi);
    const uint64_t c0 = o / chunk, c1 = (o + len - 1) / chunk;
    // (window_chunks clips to the file: c0 <= lo <= hi <= c1 < nchunks; checked all the same)
    if (lo < c0 || hi > c1 || hi >= nchunks || lo > hi) { whole[f] = 1; continue; }
    if (2 * (hi - lo + 1) > c1 - c0 + 1) { whole[f] = 1; continue; }
    for (uint64_t k = lo; k <= hi; ++k) marks[k] = 1;
  }
}

// '\n' among the frame's bytes [p0, p1), counted by the whole wave: lane l
// takes the aligned 16-byte words l, l + 64, ... of the span, a SWAR compare
// per dword, the bytes outside [p0, p1) masked off; a butterfly of __shfl_xor
// leaves the sum in every lane.  The callers keep the span inside one K1
// chunk (at most 32 KiB: 32 words a lane).  The first word starts at p0
// rounded down -- the frame is 16-byte aligned, so at or above byte 0 -- and
// the last ends below p1 + 16: p1 is at most the segment's bytes, behind
// which the frame guarantees 16 readable bytes (the guarantee
// gather_copy_launch's whole-word copy relies on, gather_dev.h).
__device__ __forceinline__ uint32_t wave_count_nl(const uint8_t* __restrict__ data, uint64_t p0, uint64_t p1,
                                                  uint32_t lane) {
  uint32_t c = 0;
  if (p1 > p0) {
    const uint64_t w1 = (p1 + 15) >> 4;
    for (uint64_t w = (p0 >> 4) + lane; w < w1; w += 64) {
      const uint64_t wb = w << 4;
      const v4u x = *reinterpret_cast<const v4u*>(data + wb);
      const uint32_t cut_lo = p0 > wb ? static_cast<uint32_t>(p0 - wb) : 0u;             // 0 .. 15
      const uint32_t cut_hi = p1 - wb < 16 ? static_cast<uint32_t>(p1 - wb) : 16u;       // 1 .. 16
      const uint32_t valid = ((1u << cut_hi) - 1u) & ~((1u << cut_lo) - 1u);             // one bit per byte
      const uint32_t d[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t y = d[k] ^ 0x0a0a0a0au;                                           // a zero byte where '\n' stood
        const uint32_t z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);       // 0x80 per zero byte, exact
        const uint32_t v = (valid >> (4 * k)) & 15u;
        const uint32_t keep = ((v & 1u) << 7) | ((v & 2u) << 14) | ((v & 4u) << 21) | ((v & 8u) << 28);
        c += __popc(z & keep);
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
  return __builtin_amdgcn_readfirstlane(c);
}

// Line windows (gather.h: line_window is the byte model, line_window_chunks
// the walk run here): in place of tsg_gw_windows when line_cap != 0.  One wave
// per candidate of a windowed file: a wave reads 64 records, a lane each, and
// then takes the eligible ones in turn, every lane running the same walk --
// bytes are counted by the whole wave (wave_count_nl) only in the partial
// chunks at s and t and over [s, t); in between, K1's per-chunk counts (nl) of
// chunks that lie wholly inside the file are summed.  Every nl index lies
// strictly between two chunks of the file, [c0, c1] with c1 < nchunks checked
// first; every byte read lies in [file start, file end) but for the aligned
// words at its ends (wave_count_nl).
// stats: [0] candidates whose chunks exceed the byte window's, [1] candidates
// whose walk ended at the cap.
__global__ __launch_bounds__(256) void tsg_gw_lines(const uint4* __restrict__ cands,
                                                    const uint32_t* __restrict__ ncands, uint32_t cand_cap,
                                                    const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                    const uint8_t* __restrict__ cls, uint8_t* __restrict__ whole,
                                                    uint8_t* __restrict__ marks, uint32_t chunk, uint64_t nchunks,
                                                    uint32_t before, uint32_t after, uint32_t line_cap,
                                                    const uint8_t* __restrict__ data,
                                                    const uint16_t* __restrict__ nl,
                                                    unsigned long long* __restrict__ stats) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * kGwWaves + (threadIdx.x >> 6);
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kGwWaves;
  const uint32_t n = min(*ncands, cand_cap);
  uint32_t widened = 0, capped = 0;
  for (uint64_t base = wave * 64; base < n; base += nwaves * 64) {
    const uint64_t i = base + lane;
    uint32_t f = 0, s_lo = 0, s_hi = 0;
    bool ok = false;
    if (i < n) {
      const uint4 c = cands[i];
      f = c.x; s_lo = c.z; s_hi = c.w;
      if (f >= lead && f < nfiles && cls[f] == kGatherClassWindow) {
        const uint64_t start = s_lo | (static_cast<uint64_t>(s_hi) << 32);
        ok = start < off[f + 1] - off[f];          // (tsg_gw_flags made a file with a start past it whole)
      }
    }
    uint64_t todo = __ballot(ok);
    while (todo) {
      const int src = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1;
      const uint32_t cf = __builtin_amdgcn_readlane(f, src);
      const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readlane(s_lo, src)) |
                         (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(s_hi, src))) << 32);
      const uint64_t o = off[cf], len = off[cf + 1] - o;
      const uint64_t c0 = o / chunk, c1 = (o + len - 1) / chunk;
      if (c1 >= nchunks || c1 < c0) { if (lane == 0) whole[cf] = 1; continue; }
      // the byte window, as tsg_gw_windows, and the line window's chunks (gather.h: the model runs the same walk)
      uint64_t plo, phi, lo, hi;
      bool cap_hit;
      window_chunks(o, len, s, before, after, chunk, &plo, &phi);
      line_window_chunks(o, len, s, before, after, line_cap, chunk, nl,
                         [data, lane](uint64_t p0, uint64_t p1) { return wave_count_nl(data, p0, p1, lane); }, &lo, &hi,
                         &cap_hit);
      // (every chunk above is one of the file's: c0 <= lo <= hi <= c1 < nchunks; checked all the same)
      if (lo < c0 || hi > c1 || hi >= nchunks || lo > hi) { if (lane == 0) whole[cf] = 1; continue; }
      widened += lo < plo || hi > phi;
      capped += cap_hit;
      if (2 * (hi - lo + 1) > c1 - c0 + 1) { if (lane == 0) whole[cf] = 1; continue; }
      for (uint64_t k = lo + lane; k <= hi; k += 64) marks[k] = 1;
    }
  }
  if (lane == 0) {
    if (widened) atomicAdd(stats, static_cast<unsigned long long>(widened));
    if (capped) atomicAdd(stats + 1, static_cast<unsigned long long>(capped));
  }
}

// the first file at or above lead that ends above byte b (nfiles: none)
__device__ __forceinline__ uint32_t first_file_ending_above(const uint64_t* __restrict__ off, uint32_t nfiles,
                                                            uint32_t lead, uint64_t b) {
  uint32_t lo = lead, hi = nfiles;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid + 1] > b) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void tsg_gw_count(const uint8_t* __restrict__ marks, uint64_t nchunks,
                                                    const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                    const uint8_t* __restrict__ cls, uint32_t* __restrict__ cnt,
                                                    uint32_t chunk) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x, step = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t c = tid; c < nchunks; c += step) {
    if (!marks[c]) continue;
    const uint64_t b0 = c * chunk, b1 = b0 + chunk;
    for (uint32_t f = first_file_ending_above(off, nfiles, lead, b0); f < nfiles && off[f] < b1; ++f)
      if (cls[f] == kGatherClassWindow && off[f + 1] > off[f]) atomicAdd(cnt + f, 1u);
  }
}

__global__ __launch_bounds__(256) void tsg_gw_demote(const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                     uint8_t* __restrict__ cls, const uint8_t* __restrict__ whole,
                                                     const uint32_t* __restrict__ cnt, uint8_t* __restrict__ marks,
                                                     uint32_t chunk, uint64_t nchunks) {
  const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (uint32_t f = lead + tid; f < nfiles; f += step) {
    const uint64_t o = off[f], len = off[f + 1] - o;
    uint8_t c = cls[f];
    if (c == kGatherClassWindow) {
      const uint64_t nfc = (o + len - 1) / chunk - o / chunk + 1;
      if (whole[f] || 2 * static_cast<uint64_t>(cnt[f]) > nfc) cls[f] = c = kGatherClassWhole;
    }
    // an empty whole file: the chunk it lies in (tsg_gw_fill sees only files with bytes)
    if (c == kGatherClassWhole && len == 0 && o / chunk < nchunks) marks[o / chunk] = 1;
  }
}

__global__ __launch_bounds__(256) void tsg_gw_fill(uint8_t* __restrict__ marks, uint64_t nchunks,
                                                   const uint64_t* __restrict__ off, uint32_t nfiles, uint32_t lead,
                                                   const uint8_t* __restrict__ cls, uint32_t chunk) {
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x, step = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t c = tid; c < nchunks; c += step) {
    if (marks[c]) continue;
    const uint64_t b0 = c * chunk, b1 = b0 + chunk;
    for (uint32_t f = first_file_ending_above(off, nfiles, lead, b0); f < nfiles && off[f] < b1; ++f)
      if (cls[f] == kGatherClassWhole && off[f + 1] > off[f]) { marks[c] = 1; break; }
  }
}

// one thread per region: its 128 mark bytes (0 or 1), and the run starts among them
__global__ __launch_bounds__(256) void tsg_gw_regions(const uint8_t* __restrict__ marks, uint32_t nregions,
                                                      uint32_t* __restrict__ region_m, uint32_t* __restrict__ region_s) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nregions) return;
  const uint64_t b0 = static_cast<uint64_t>(r) * kGwRegion;
  const v4u* p = reinterpret_cast<const v4u*>(marks + b0);
  uint32_t prev = r ? marks[b0 - 1] : 0u, m = 0, s = 0;
#pragma unroll
  for (uint32_t q = 0; q < kGwRegion / 16; ++q) {
    const v4u w = p[q];
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = d[k] & 0x01010101u;
      // a start: a marked byte whose predecessor is not (bytes shifted up by one, the carry from the word before)
      const uint32_t pred = (x << 8) | prev;
      m += __popc(x);
      s += __popc(x & ~pred);
      prev = x >> 24;
    }
  }
  region_m[r] = m;
  region_s[r] = s;
}

// One wave per region, lane l on chunks 2l and 2l + 1 of it.  Run k is the
// k-th run start in chunk order; it lands behind the marked chunks in front
// of it.  A run's end stores its last byte + 1 into len (tsg_gw_finish
// subtracts src).  Nothing is stored at or past runs_cap.
__global__ __launch_bounds__(256) void tsg_gw_runs(const uint8_t* __restrict__ marks, uint32_t nregions,
                                                   const uint64_t* __restrict__ base_m,
                                                   const uint64_t* __restrict__ base_s, GatherRun* __restrict__ runs,
                                                   uint64_t runs_cap, uint32_t chunk, uint64_t total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x * kGwWaves + wv;
  if (r >= nregions) return;                 // whole waves only; no workgroup barrier below
  const uint64_t b0 = static_cast<uint64_t>(r) * kGwRegion;
  const uint32_t m = reinterpret_cast<const uint16_t*>(marks + b0)[lane];
  const uint32_t m0 = m & 1u, m1 = (m >> 8) & 1u;
  // (the marks array ends with a region of zeros: b0 + 128 is readable)
  const uint32_t before = r ? marks[b0 - 1] & 1u : 0u, behind = marks[b0 + kGwRegion] & 1u;
  const uint32_t up = __shfl_up(m1, 1), down = __shfl_down(m0, 1);
  const uint32_t prev = lane ? up : before, next = lane < 63 ? down : behind;
  const uint32_t s0 = m0 & ~prev & 1u, s1 = m1 & ~m0 & 1u;
  const uint32_t e0 = m0 & ~m1 & 1u, e1 = m1 & ~next & 1u;
  uint32_t im = m0 + m1, is = s0 + s1;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t um = __shfl_up(im, d), us = __shfl_up(is, d);
    if (lane >= d) { im += um; is += us; }
  }
  const uint64_t xm = base_m[r] + (im - m0 - m1), xs = base_s[r] + (is - s0 - s1);
  const uint64_t c0 = b0 + 2u * lane;
  if (s0 && xs < runs_cap) { runs[xs].src = c0 * chunk; runs[xs].dst = xm * chunk; }
  if (s1 && xs + s0 < runs_cap) { runs[xs + s0].src = (c0 + 1) * chunk; runs[xs + s0].dst = (xm + m0) * chunk; }
  if (e0 && xs + s0 - 1 < runs_cap) runs[xs + s0 - 1].len = min((c0 + 1) * chunk, total);
  if (e1 && xs + s0 + s1 - 1 < runs_cap) runs[xs + s0 + s1 - 1].len = min((c0 + 2) * chunk, total);
}

__global__ __launch_bounds__(256) void tsg_gw_finish(GatherRun* __restrict__ runs, const uint64_t* __restrict__ tot_m,
                                                     const uint64_t* __restrict__ tot_s, uint64_t runs_cap,
                                                     const uint8_t* __restrict__ marks, uint64_t nchunks,
                                                     uint32_t chunk, uint64_t total, uint64_t* __restrict__ meta) {
  const uint64_t nruns = *tot_s;
  const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x, step = static_cast<uint64_t>(gridDim.x) * 256;
  if (nruns <= runs_cap)
    for (uint64_t k = tid; k < nruns; k += step) runs[k].len -= runs[k].src;
  if (tid == 0) {
    // (the last chunk may be short; a run table that did not fit: a total no buffer holds, so the copy stores nothing)
    uint64_t bytes = *tot_m * chunk;
    if (nchunks && marks[nchunks - 1]) bytes -= nchunks * chunk - total;
    meta[0] = nruns;
    meta[1] = nruns <= runs_cap ? gather_round(bytes) : ~uint64_t(0);
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

namespace {
size_t gw_align(size_t n) { return (n + 63) & ~size_t(63); }
uint64_t gw_regions(uint64_t nchunks) { return (nchunks + kGwRegion - 1) / kGwRegion; }
}  // namespace

size_t gather_windows_scratch_bytes(uint64_t nchunks, uint32_t nfiles) {
  const uint64_t nreg = gw_regions(nchunks);
  return 128 + gw_align(nfiles) * 2 + gw_align(static_cast<size_t>(nfiles) * 4) + gw_align(nreg * 8) * 2 +
         gw_align(nreg * 4) * 2 + (nreg + 1) * kGwRegion + 64;
}

GatherWindowScratch gather_windows_scratch_layout(void* scratch, uint64_t nchunks, uint32_t nfiles) {
  const uint64_t nreg = gw_regions(nchunks);
  uint8_t* sp = static_cast<uint8_t*>(scratch);
  GatherWindowScratch sc;
  sc.tot_m = reinterpret_cast<uint64_t*>(sp);
  sc.pad_m = reinterpret_cast<uint64_t*>(sp + 16);
  sc.tot_s = reinterpret_cast<uint64_t*>(sp + 64);
  sc.pad_s = reinterpret_cast<uint64_t*>(sp + 80);
  sp += 128;
  sc.any = sp; sp += gw_align(nfiles);
  sc.whole = sp; sp += gw_align(nfiles);
  sc.cnt = reinterpret_cast<uint32_t*>(sp); sp += gw_align(static_cast<size_t>(nfiles) * 4);
  sc.base_m = reinterpret_cast<uint64_t*>(sp); sp += gw_align(nreg * 8);
  sc.base_s = reinterpret_cast<uint64_t*>(sp); sp += gw_align(nreg * 8);
  sc.region_m = reinterpret_cast<uint32_t*>(sp); sp += gw_align(nreg * 4);
  sc.region_s = reinterpret_cast<uint32_t*>(sp); sp += gw_align(nreg * 4);
  sc.marks = sp;
  return sc;
}

bool gather_windows_launch(const void* cands, const uint32_t* ncands, uint32_t cand_cap, const uint32_t* fflags,
                           const uint64_t* offsets, uint32_t nfiles, uint32_t lead, bool all, const uint8_t* wrows,
                           uint32_t nrows, uint32_t chunk, uint64_t total, const GatherWindowOpts& o,
                           const GatherWindowScratch& sc, uint8_t* cls, GatherRun* runs, uint64_t runs_cap,
                           uint64_t* meta, hipStream_t s, std::string* err, const uint8_t* data, const uint16_t* nl,
                           hipEvent_t lines_begin, hipEvent_t lines_end) {
  const uint64_t nchunks = (total + chunk - 1) / chunk, nreg64 = gw_regions(nchunks);
  if (o.line_cap != 0 && (!data || !nl)) { *err = "gather windows: line windows need the frame and K1's newline counts"; return false; }
  if (chunk == 0 || chunk % 128 != 0 || nreg64 > 0xffffffffull / kGwWaves) { *err = "gather windows: chunk grid out of range"; return false; }
  const uint32_t nreg = static_cast<uint32_t>(nreg64);
  hipError_t e = hipMemsetAsync(sc.tot_m, 0, gather_windows_scratch_bytes(nchunks, nfiles), s);
  if (e == hipSuccess && nfiles) e = hipMemsetAsync(cls, 0, nfiles, s);
  if (e == hipSuccess) e = hipMemsetAsync(meta + 2, 0, 16, s);          // tsg_gw_lines' counters
  if (e != hipSuccess) { *err = std::string("gather windows: ") + hipGetErrorString(e); return false; }
  // (grid-stride kernels: at most 1024 workgroups, as tsg_gather_mark's; the candidate passes cannot know the
  // list's length on the host and take the capacity's grid)
  auto grid = [](uint64_t n) { const uint64_t b = (n + 255) / 256; return dim3(static_cast<uint32_t>(b < 1 ? 1 : b > 1024 ? 1024 : b)); };
  const uint4* cd = static_cast<const uint4*>(cands);
  hipLaunchKernelGGL(tsg_gw_flags, grid(cand_cap), dim3(256), 0, s, cd, ncands, cand_cap, offsets, nfiles, lead, wrows,
                     nrows, sc.any, sc.whole);
  hipLaunchKernelGGL(tsg_gw_class, grid(nfiles), dim3(256), 0, s, offsets, nfiles, lead, fflags, all ? 1u : 0u,
                     o.min_file, static_cast<const uint8_t*>(sc.any), static_cast<const uint8_t*>(sc.whole), cls,
                     sc.marks, chunk, nchunks);
  if (o.line_cap != 0) {
    if (lines_begin && (e = hipEventRecord(lines_begin, s)) != hipSuccess) { *err = std::string("gather windows: ") + hipGetErrorString(e); return false; }
    hipLaunchKernelGGL(tsg_gw_lines, grid(cand_cap), dim3(256), 0, s, cd, ncands, cand_cap, offsets, nfiles, lead,
                       static_cast<const uint8_t*>(cls), sc.whole, sc.marks, chunk, nchunks, o.before, o.after, o.line_cap,
                       data, nl, reinterpret_cast<unsigned long long*>(meta + 2));
    if (lines_end && (e = hipEventRecord(lines_end, s)) != hipSuccess) { *err = std::string("gather windows: ") + hipGetErrorString(e); return false; }
  } else {
    hipLaunchKernelGGL(tsg_gw_windows, grid(cand_cap), dim3(256), 0, s, cd, ncands, cand_cap, offsets, nfiles, lead,
                       static_cast<const uint8_t*>(cls), sc.whole, sc.marks, chunk, nchunks, o.before, o.after);
  }
  hipLaunchKernelGGL(tsg_gw_count, grid(nchunks), dim3(256), 0, s, static_cast<const uint8_t*>(sc.marks), nchunks,
                     offsets, nfiles, lead, static_cast<const uint8_t*>(cls), sc.cnt, chunk);
  hipLaunchKernelGGL(tsg_gw_demote, grid(nfiles), dim3(256), 0, s, offsets, nfiles, lead, cls,
                     static_cast<const uint8_t*>(sc.whole), static_cast<const uint32_t*>(sc.cnt), sc.marks, chunk,
                     nchunks);
  hipLaunchKernelGGL(tsg_gw_fill, grid(nchunks), dim3(256), 0, s, sc.marks, nchunks, offsets, nfiles, lead,
                     static_cast<const uint8_t*>(cls), chunk);
  if (nreg)
    hipLaunchKernelGGL(tsg_gw_regions, dim3((nreg + 255u) / 256u), dim3(256), 0, s,
                       static_cast<const uint8_t*>(sc.marks), nreg, sc.region_m, sc.region_s);
  region_scan_launch(sc.region_m, nreg, sc.base_m, sc.tot_m, sc.pad_m, s);
  region_scan_launch(sc.region_s, nreg, sc.base_s, sc.tot_s, sc.pad_s, s);
  if (nreg)
    hipLaunchKernelGGL(tsg_gw_runs, dim3((nreg + kGwWaves - 1) / kGwWaves), dim3(256), 0, s,
                       static_cast<const uint8_t*>(sc.marks), nreg, static_cast<const uint64_t*>(sc.base_m),
                       static_cast<const uint64_t*>(sc.base_s), runs, runs_cap, chunk, total);
  hipLaunchKernelGGL(tsg_gw_finish, grid(runs_cap), dim3(256), 0, s, runs, static_cast<const uint64_t*>(sc.tot_m),
                     static_cast<const uint64_t*>(sc.tot_s), runs_cap, static_cast<const uint8_t*>(sc.marks), nchunks,
                     chunk, total, meta);
  e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("gather windows launch: ") + hipGetErrorString(e); return false; }
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
