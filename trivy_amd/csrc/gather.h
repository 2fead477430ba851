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

// ---------------------------------------------------------------- windows
// The opt-in layout that gathers windows around candidate starts instead of
// whole files (tsg_scan_batch_device_opts).  Everything lives on the segment's
// K1 chunk grid: a chunk is gathered or it is not (marks), maximal sequences of
// marked chunks are the runs, and a run lands at chunk * (marked chunks in
// front of it) -- chunk is a multiple of 128, so every destination is 64-byte
// aligned as plan_gather's are.  plan_gather_windows is the CPU model of the
// device passes (gather.hip: tsg_gw_*), pass for pass.
//
// A file is gathered whole when the confirmer may read any of it: fold-special
// content, a mode-1 rule in the set, a candidate of a row that is not
// windowable (mode-3 presence, host-gated keywords, exclude-block pseudo-rules),
// a kFullScanStart or out-of-file start, a file below min_file bytes, or
// windows that mark more than half of its chunks.  Otherwise it contributes
// its head chunk (CensoredView::prefix_at counts '\n' from that boundary) and,
// per candidate start s, the chunks of [s - before, s + after) clipped to the
// file.
constexpr uint8_t kGatherClassNone = 0, kGatherClassWhole = 1, kGatherClassWindow = 2;
constexpr uint32_t kGatherNoRun = ~uint32_t(0);

struct GatherWindowOpts {
  uint32_t before = 0, after = 0;
  uint64_t min_file = 0;
  bool on() const { return before != 0 || after != 0; }
};

// (the host's Cand and the device's candidate record have this layout)
struct GatherCand { uint32_t file, rule; uint64_t start; };

struct GatherWindowPlan {
  std::vector<uint8_t> cls;          // per file: kGatherClass*
  std::vector<uint32_t> first_run;   // per file: the run holding its first chunk, or kGatherNoRun
  std::vector<GatherRun> runs;
  std::vector<uint8_t> marks;        // per chunk of the segment
  uint64_t total = 0;
};

// The chunks [*lo, *hi] of the segment's grid that the window of start s (s <
// len) of the file at frame offset off marks.  (constexpr: the device calls it)
constexpr void window_chunks(uint64_t off, uint64_t len, uint64_t s, uint32_t before, uint32_t after, uint32_t chunk,
                             uint64_t* lo, uint64_t* hi) {
  const uint64_t a = s > before ? s - before : 0;
  uint64_t b = s + after < len ? s + after : len;
  if (b <= s) b = s + 1;
  *lo = (off + a) / chunk;
  *hi = (off + b - 1) / chunk;
}

// The run holding chunk c (runs sorted by src, every src and all lens but the
// last multiples of chunk), or kGatherNoRun.
inline uint32_t gather_run_of(const GatherRun* runs, size_t nruns, uint64_t byte) {
  size_t lo = 0, hi = nruns;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (runs[mid].src <= byte) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return kGatherNoRun;
  const GatherRun& r = runs[lo - 1];
  return byte - r.src < r.len ? static_cast<uint32_t>(lo - 1) : kGatherNoRun;
}

// cands: K2's list (duplicates allowed, any order); fflags: per-file flag words;
// all: the rule set has a mode-1 rule; windowable: one byte per plan row.
inline void plan_gather_windows(const uint64_t* offsets, uint32_t nfiles, uint32_t lead, const GatherCand* cands,
                                size_t ncands, const uint32_t* fflags, bool all, const uint8_t* windowable,
                                uint32_t nrows, uint32_t chunk, const GatherWindowOpts& o, GatherWindowPlan* out) {
  const uint64_t total = nfiles ? offsets[nfiles] : 0;
  const uint64_t nchunks = (total + chunk - 1) / chunk;
  out->cls.assign(nfiles, kGatherClassNone);
  out->first_run.assign(nfiles, kGatherNoRun);
  out->marks.assign(nchunks, 0);
  out->runs.clear();
  std::vector<uint8_t> any(nfiles, 0), whole(nfiles, 0);
  // pass 1, per candidate: which files have one, which need the whole file
  for (size_t i = 0; i < ncands; ++i) {
    const GatherCand& c = cands[i];
    if (c.file < lead || c.file >= nfiles) continue;
    any[c.file] = 1;
    const uint64_t len = offsets[c.file + 1] - offsets[c.file];
    if (c.rule >= nrows || !windowable[c.rule] || c.start >= len) whole[c.file] = 1;   // (kFullScanStart >= len)
  }
  // pass 2, per file: the class before the windows are counted; heads
  for (uint32_t f = lead; f < nfiles; ++f) {
    const uint64_t len = offsets[f + 1] - offsets[f];
    if (!(all || fflags[f] != 0 || any[f])) continue;
    const bool w = all || fflags[f] != 0 || whole[f] || len < o.min_file || len == 0;
    out->cls[f] = w ? kGatherClassWhole : kGatherClassWindow;
    if (!w) out->marks[offsets[f] / chunk] = 1;
  }
  // pass 3, per candidate of a windowed file: its window's chunks (a window
  // that alone spans more than half of the file's chunks marks nothing)
  for (size_t i = 0; i < ncands; ++i) {
    const GatherCand& c = cands[i];
    if (c.file < lead || c.file >= nfiles || out->cls[c.file] != kGatherClassWindow) continue;
    const uint64_t off = offsets[c.file], len = offsets[c.file + 1] - off;
    uint64_t lo, hi;
    window_chunks(off, len, c.start, o.before, o.after, chunk, &lo, &hi);
    const uint64_t nfc = (off + len - 1) / chunk - off / chunk + 1;
    if (2 * (hi - lo + 1) > nfc) { whole[c.file] = 1; continue; }
    for (uint64_t k = lo; k <= hi; ++k) out->marks[k] = 1;
  }
  // passes 4 and 5: marked chunks per file (a chunk two files share counts
  // for both); windows over more than half of a file's chunks make it whole
  for (uint32_t f = lead; f < nfiles; ++f) {
    if (out->cls[f] != kGatherClassWindow) continue;
    const uint64_t off = offsets[f], len = offsets[f + 1] - off;
    const uint64_t c0 = off / chunk, c1 = (off + len - 1) / chunk;
    uint64_t cnt = 0;
    for (uint64_t k = c0; k <= c1; ++k) cnt += out->marks[k];
    if (whole[f] || 2 * cnt > c1 - c0 + 1) out->cls[f] = kGatherClassWhole;
  }
  // pass 6: every chunk of a whole file (an empty one: the chunk it lies in)
  for (uint32_t f = lead; f < nfiles; ++f) {
    if (out->cls[f] != kGatherClassWhole) continue;
    const uint64_t off = offsets[f], len = offsets[f + 1] - off;
    if (len == 0) { if (off / chunk < nchunks) out->marks[off / chunk] = 1; continue; }
    for (uint64_t k = off / chunk; k <= (off + len - 1) / chunk; ++k) out->marks[k] = 1;
  }
  // the compaction: runs of marked chunks
  uint64_t before = 0;
  for (uint64_t k = 0; k < nchunks;) {
    if (!out->marks[k]) { ++k; continue; }
    uint64_t e = k;
    while (e + 1 < nchunks && out->marks[e + 1]) ++e;
    const uint64_t src = k * chunk, end = (e + 1) * chunk < total ? (e + 1) * chunk : total;
    out->runs.push_back(GatherRun{src, before * chunk, end - src});
    before += e - k + 1;
    k = e + 1;
  }
  out->total = out->runs.empty() ? 0 : gather_round(out->runs.back().dst + out->runs.back().len);
  for (uint32_t f = lead; f < nfiles; ++f)
    if (out->cls[f] != kGatherClassNone && offsets[f] / chunk < nchunks)
      out->first_run[f] = gather_run_of(out->runs.data(), out->runs.size(), offsets[f] / chunk * chunk);
}

}  // namespace tsg
