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
  uint32_t line_cap = 0;             // line windows (below); 0: the byte window alone
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
  // line windows: candidates whose window covers more chunks than [s - before, s + after) does, and
  // candidates whose walk ended at the line cap on either side (duplicates in the list count again)
  uint64_t widened = 0, capped = 0;
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

// ---------------------------------------------------------------- line windows
// The confirmer reads lines, not a span: to_finding (scanner.cpp:726-765) asks
// for
//   prev_nl(start)                      the start of the match's own line,
//   prev_nl once per line above it,     at most two (code_start = start_line - 2),
// and each call must find its '\n' inside a gathered run (WindowView::prev_nl:
// a search that meets a run's lower edge above byte 0 makes the file
// insufficient), so the 3rd '\n' met walking back from start - 1 is the
// lowest byte it reads (kLineBack) -- the '\n' itself, one byte below the
// line's first, which matters when it is a chunk's last byte; and forward for
//   next_nl(start)                      the end of the match's line,
//   next_nl once per line up to         end_line + 1 (code_end = end_line + 2),
// where end_line = start_line + m for a match holding m '\n'.  Those m are
// censored, and a censored '\n' is no line end, so 2 + m uncensored ones lie
// behind the match's first byte.  K2 reports no match end; while the window
// is sufficient at all the match lies in [s, t), t = min(len, s + after), so
// m is at most the '\n' of [s, t) and the walk takes kLineFwd + that many
// from t on.  Both walks stop after line_cap bytes.  The confirmer can need
// more (an earlier match censoring a '\n' in front of s); such a file is
// insufficient and fetched whole, as with byte windows.
constexpr uint32_t kLineBack = 3, kLineFwd = 2;

// File bytes [*a, *b) of the line window of start s (s < len) in the file p[0, len).
// capped: a walk ended at line_cap bytes, short of its newlines and of the file's edge.
inline void line_window(const uint8_t* p, uint64_t len, uint64_t s, const GatherWindowOpts& o, uint64_t* a, uint64_t* b,
                        bool* capped) {
  const uint64_t t = s + o.after < len ? s + o.after : len;
  const uint64_t lower = s > o.line_cap ? s - o.line_cap : 0;
  uint64_t back = lower;
  uint32_t nb = 0;
  for (uint64_t q = s; q > lower; --q)
    if (p[q - 1] == '\n' && ++nb == kLineBack) { back = q - 1; break; }
  uint64_t need = kLineFwd;
  for (uint64_t q = s; q < t; ++q) need += p[q] == '\n';
  const uint64_t upper = t + o.line_cap < len ? t + o.line_cap : len;
  uint64_t fwd = upper, nf = 0;
  for (uint64_t q = t; q < upper; ++q)
    if (p[q] == '\n' && ++nf == need) { fwd = q + 1; break; }
  const uint64_t a0 = s > o.before ? s - o.before : 0;
  *a = a0 < back ? a0 : back;
  *b = t > fwd ? t : fwd;
  if (*b <= s) *b = s + 1;
  *capped = (nb < kLineBack && lower > 0) || (nf < need && t + o.line_cap < len);
}

#ifdef __HIPCC__
#define TSG_GATHER_HD __host__ __device__
#else
#define TSG_GATHER_HD
#endif

// The same window on the chunk grid, from the bytes at its ends and a table of
// '\n' per chunk (K1's nl_count) in between: what the device pass
// (gather.hip tsg_gw_lines) runs, a wave per candidate, with count(p0, p1) =
// the '\n' among the frame's bytes [p0, p1), p0 <= p1 inside one chunk.  o:
// the file's frame offset.  *lo .. *hi are the chunks of line_window's [a, b),
// *capped its flag.  Only chunks strictly between two chunks of the file are
// looked up, so each lies wholly inside the file: the file's first and last
// chunk, which neighbours may share, never are -- reaching the chunk of
// s - line_cap (the file's first when s <= line_cap) or of the upper end ends
// a walk whatever that chunk holds, as in the byte model, where the edge lies
// in it.  A walk takes at most line_cap / chunk + 1 steps.  The bytes of an
// edge chunk are counted for `capped` alone.
template <class CountFn>
TSG_GATHER_HD inline void line_window_chunks(uint64_t o, uint64_t len, uint64_t s, uint32_t before, uint32_t after,
                                             uint32_t line_cap, uint32_t chunk, const uint16_t* nl, CountFn count,
                                             uint64_t* lo, uint64_t* hi, bool* capped) {
  const uint32_t max_steps = line_cap / chunk + 2;
  bool cap_hit = false;
  // backward: the chunk of the kLineBack-th '\n' behind s, no lower than the chunk of s - line_cap
  const uint64_t lower = s > line_cap ? s - line_cap : 0;
  const uint64_t kl = (o + lower) / chunk, ks = (o + s) / chunk;
  uint64_t lo_b = kl, sum = 0;
  if (kl < ks) {
    sum = count(ks * chunk, o + s);
    if (sum >= kLineBack) {
      lo_b = ks;
    } else {
      uint32_t steps = 0;
      for (uint64_t k = ks - 1; k > kl && steps < max_steps; --k, ++steps) {
        sum += nl[k];
        if (sum >= kLineBack) { lo_b = k; break; }
      }
    }
  }
  if (sum < kLineBack && lower > 0) {
    const uint64_t e = (kl + 1) * chunk < o + s ? (kl + 1) * chunk : o + s;
    cap_hit = sum + count(o + lower, e) < kLineBack;
  }
  // forward: N = kLineFwd + the '\n' of [s, t); the chunk of the N-th from t on
  const uint64_t t = s + after < len ? s + after : len;
  uint64_t hi_e = (o + (t > s ? t : s + 1) - 1) / chunk;
  if (t < len) {
    uint64_t need = kLineFwd;
    const uint64_t q0 = o + s, q1 = o + t;
    if (q1 > q0) {
      const uint64_t k0 = q0 / chunk, k1 = (q1 - 1) / chunk;
      if (k0 == k1) {
        need += count(q0, q1);
      } else {
        need += count(q0, (k0 + 1) * chunk) + count(k1 * chunk, q1);
        const uint64_t lim = static_cast<uint64_t>(after) / chunk + 2;     // (k1 - k0 - 1 is below it)
        for (uint64_t k = k0 + 1; k < k1 && k - k0 <= lim; ++k) need += nl[k];
      }
    }
    const uint64_t upper = t + line_cap < len ? t + line_cap : len;
    const uint64_t kt = (o + t) / chunk, ku = (o + upper - 1) / chunk;
    hi_e = ku;
    uint64_t got = 0;
    if (kt < ku) {
      got = count(o + t, (kt + 1) * chunk);
      if (got >= need) {
        hi_e = kt;
      } else {
        uint32_t steps = 0;
        for (uint64_t k = kt + 1; k < ku && steps < max_steps; ++k, ++steps) {
          got += nl[k];
          if (got >= need) { hi_e = k; break; }
        }
      }
    }
    if (got < need && t + line_cap < len) {
      const uint64_t b = ku * chunk > o + t ? ku * chunk : o + t;
      cap_hit = cap_hit || got + count(b, o + upper) < need;
    }
  }
  uint64_t plo = 0, phi = 0;
  window_chunks(o, len, s, before, after, chunk, &plo, &phi);
  *lo = plo < lo_b ? plo : lo_b;
  *hi = phi > hi_e ? phi : hi_e;
  *capped = cap_hit;
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
// all: the rule set has a mode-1 rule; windowable: one byte per plan row;
// data: the frame's bytes, read only with o.line_cap != 0; nl (tests): with it
// the windows come from line_window_chunks on that table, as on the device,
// instead of from line_window on the bytes -- the plans must be equal.
inline void plan_gather_windows(const uint64_t* offsets, uint32_t nfiles, uint32_t lead, const GatherCand* cands,
                                size_t ncands, const uint32_t* fflags, bool all, const uint8_t* windowable,
                                uint32_t nrows, uint32_t chunk, const GatherWindowOpts& o, GatherWindowPlan* out,
                                const uint8_t* data = nullptr, const uint16_t* nl = nullptr) {
  const uint64_t total = nfiles ? offsets[nfiles] : 0;
  const uint64_t nchunks = (total + chunk - 1) / chunk;
  out->cls.assign(nfiles, kGatherClassNone);
  out->first_run.assign(nfiles, kGatherNoRun);
  out->marks.assign(nchunks, 0);
  out->runs.clear();
  out->widened = out->capped = 0;
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
    if (o.line_cap != 0 && data) {
      uint64_t a, b, llo, lhi;
      bool capped;
      if (nl) {
        line_window_chunks(off, len, c.start, o.before, o.after, o.line_cap, chunk, nl,
                           [data](uint64_t p0, uint64_t p1) {
                             uint64_t n = 0;
                             for (uint64_t q = p0; q < p1; ++q) n += data[q] == '\n';
                             return n;
                           },
                           &llo, &lhi, &capped);
      } else {
        line_window(data + off, len, c.start, o, &a, &b, &capped);
        llo = (off + a) / chunk;
        lhi = (off + b - 1) / chunk;
      }
      out->widened += llo < lo || lhi > hi;
      out->capped += capped;
      lo = llo;
      hi = lhi;
    }
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
