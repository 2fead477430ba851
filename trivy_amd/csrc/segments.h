// Where Engine::scan cuts a batch: upload segments (host data) or resident
// pieces (device data).  Pure arithmetic on the offsets array -- no HIP, no
// device -- so the policy behind every step time in the README is tested on
// the CPU (tsg_test_plan_segments, tests/test_segments.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tsg {

struct BatchInput {
  const uint8_t* h_data = nullptr;     // host copy for the exact confirmer; nullptr with d_data set: a
                                       // device-only scan (the confirmer reads the GPU's gather of the batch)
  const void* d_data = nullptr;        // device copy; nullptr -> engine uploads h_data
  const uint64_t* offsets = nullptr;   // nfiles + 1 byte offsets into data
  uint32_t nfiles = 0;
  const char* const* paths = nullptr;  // nfiles NUL-terminated paths (ScanArgs.FilePath)
  const uint32_t* path_lens = nullptr; // optional explicit lengths
  const uint8_t* binary = nullptr;     // optional ScanArgs.Binary flags
};

// The cut policy (TSG_* environment knobs, read once at Engine::create).
struct SegmentPolicy {
  // resident data: pipeline pieces (TSG_PIECES; r3za config 2: 4 pieces,
  // first 10%: 1286 GB/s, 2 at 70/30: 919), the first piece's share
  // (TSG_FIRST_PIECE) and a short last piece's (TSG_LAST_PIECE, 0: none; used
  // from 5 pieces on).  Round 5, K2 beside the next K1 (K1Chain): 5 pieces
  // with an 8% last piece 1921 GB/s vs 4 pieces 1796 on config 2 -- the last
  // piece's K2 and host confirmation are the step's tail; 1 GB of config-1
  // files gains nothing from more pieces (profiles/r5t_resident_pieces.log)
  uint32_t pieces = 5;
  double first_piece = 0.1;
  double first_piece_few = 0.2;        // the first piece's share when a batch makes 3 pieces (TSG_FIRST_PIECE_FEW)
  double last_piece = 0.08;
  uint64_t min_piece = 256ull << 20;   // resident data: smaller batches run as one piece (TSG_MIN_PIECE_BYTES)
  uint64_t segment_min = 64ull << 20;  // uploaded data: smallest segment of the geometric tail (TSG_SEGMENT_MIN; r3s: 128 MB 51.5 vs 256 MB 48.8 GB/s on config 1; r4p: 64 MB 53.2 vs 128 MB 52.5)
  bool balanced = true;                // uploaded large-file data: equal segments of <= segment (TSG_SEGMENT_BALANCED)
  uint64_t segment = 4ull << 30;       // uploaded data: bytes per pipeline segment (TSG_SEGMENT_BYTES);
                                       // 1 GB = one full K1 round (256 CUs x 1024 lanes x 4 KiB chunks)
  double dense_files_per_gb = 8000.0;  // "many small files" (image layers: ~48k/GB); the engine sets it from kDenseFilesPerGB
};

// A batch whose bound is host confirmation, not the link or K1: it gets the
// halving tail below and no wire packing (the packers would take its CPUs).
inline bool dense_batch(uint32_t nfiles, uint64_t total, const SegmentPolicy& p) {
  return static_cast<double>(nfiles) * 1e9 > p.dense_files_per_gb * static_cast<double>(total);
}

// A self-contained sub-batch: files [f0, f0 + in.nfiles) of the call's
// batch, offsets rebased to 0, data pointers advanced to its first byte.
struct Segment {
  BatchInput in;
  std::vector<uint64_t> off;
  uint32_t f0 = 0;
  uint64_t b0 = 0, bytes = 0;
  // resident pieces: file 0 of `in` is a lead of the bytes between the
  // 256-byte boundary below the piece's first file and that file (the tail of
  // the previous piece), so K1's lines are aligned as on the pinned path; its
  // results are dropped.  lead_* hold the shifted path / length / binary arrays.
  uint32_t lead = 0;
  std::vector<const char*> lead_paths;
  std::vector<uint32_t> lead_lens;
  std::vector<uint8_t> lead_bin;
};

// Files at which a resident batch is cut into pieces (without 0 and nfiles).
inline void resident_cuts(const BatchInput& in, const SegmentPolicy& p, std::vector<uint32_t>* cut) {
  const uint64_t total = in.offsets[in.nfiles];
  const uint32_t want = static_cast<uint32_t>(std::min<uint64_t>(p.pieces, std::max<uint64_t>(1, total / p.min_piece)));
  // piece 0 takes first_piece of the bytes; with last_piece a short
  // last piece of that share follows the others (its confirmation is the
  // tail left after the GPU's last pass); the rest share what remains
  const bool short_last = p.last_piece > 0.0 && want >= 5;
  // batches of 3 pieces (0.75-1 GB) start with a larger piece
  // (TSG_FIRST_PIECE_FEW; 1 GB of config-1 files: 1.49-1.50 ms per step
  // at 10%, 1.43-1.46 at 20%, 1.45-1.46 at 30%, profiles/r8d_*)
  const double first = want == 3 ? p.first_piece_few : p.first_piece;
  const double mid = 1.0 - first - (short_last ? p.last_piece : 0.0);
  const uint32_t nmid = want - 1 - (short_last ? 1 : 0);
  for (uint32_t k = 1; k < want; ++k) {
    const double share = k <= nmid ? first + mid * (k - 1) / nmid : 1.0 - p.last_piece;
    const uint64_t target = static_cast<uint64_t>(share * static_cast<double>(total));
    const uint32_t f = static_cast<uint32_t>(std::lower_bound(in.offsets, in.offsets + in.nfiles, target) - in.offsets);
    if (f > cut->back() && f < in.nfiles) cut->push_back(f);
  }
}

// Files at which an uploaded batch is cut into segments (without 0 and nfiles).
// Geometric tail: the work left after the last upload is the last
// segment's K1/K2 and host confirmation.  For batches whose confirm
// cost per byte is high (many small files: image layers, config 5) or
// that are too small for several full segments, the rest after the full
// segments is cut in halves down to segment_min, so the last segment
// is small and every upload overlaps the previous segment's work.
// Large-file batches keep full segments (K1 runs at its large-launch
// rate and their confirmation is cheap).
inline void upload_cuts(const BatchInput& in, const SegmentPolicy& p, std::vector<uint32_t>* cut) {
  const uint64_t total = in.offsets[in.nfiles];
  const bool geometric = dense_batch(in.nfiles, total, p) || total < 2 * p.segment;
  for (uint32_t f = 0; f < in.nfiles;) {
    // next cut: the first file boundary at or past the target
    const uint64_t rest = total - in.offsets[f];
    uint64_t target;
    // (geometric batches start halving once less than two full segments
    // are left: a full segment's confirmation then hides behind the next
    // half-size upload; r3t config 5: 4.3+4.3+0.7+... GB left 16 ms after
    // the last upload, the second segment's 25 ms confirmation)
    // (large-file batches: the rest is cut into ceil(rest / segment)
    // equal segments instead of full segments plus a short remainder, so
    // every K1 launch runs at its large-launch rate: a 10 GB batch is
    // 3 x 3.33 GB, not 4 + 4 + 1.4 GB whose last launch ran at ~2.3 TB/s;
    // TSG_SEGMENT_BALANCED=0 keeps full segments)
    const uint64_t kleft = (rest + p.segment - 1) / p.segment;
    if (!geometric && p.balanced && kleft >= 2) target = in.offsets[f] + rest / kleft;
    else if (geometric ? rest >= 2 * p.segment : rest > p.segment) target = in.offsets[f] + p.segment;
    else if (geometric && rest / 2 >= p.segment_min) target = in.offsets[f] + rest / 2;
    else break;
    uint32_t g = static_cast<uint32_t>(std::lower_bound(in.offsets + f, in.offsets + in.nfiles, target) - in.offsets);
    if (g <= f) g = f + 1;
    if (g >= in.nfiles) break;
    cut->push_back(g);
    f = g;
  }
}

// Cuts a validated, non-empty batch (offsets from 0, non-decreasing, some
// bytes) into *segs.  `resident`: in.d_data is the device copy.  The segments
// point into `in`'s arrays and into their own vectors: *segs must not be
// resized while they are in use.
inline void plan_segments(const BatchInput& in, bool resident, const SegmentPolicy& p, std::vector<Segment>* segs) {
  std::vector<uint32_t> cut{0};
  if (resident) resident_cuts(in, p, &cut);
  else upload_cuts(in, p, &cut);
  cut.push_back(in.nfiles);
  segs->clear();
  segs->resize(cut.size() - 1);
  for (size_t k = 0; k < segs->size(); ++k) {
    const uint32_t a = cut[k], b = cut[k + 1];
    Segment& sg = (*segs)[k];
    BatchInput& q = sg.in;
    q = in;
    sg.f0 = a;
    sg.b0 = in.offsets[a];
    sg.bytes = in.offsets[b] - in.offsets[a];
    if (segs->size() > 1) {
      sg.off.resize(b - a + 1);
      for (uint32_t f = a; f <= b; ++f) sg.off[f - a] = in.offsets[f] - sg.b0;
      q.offsets = sg.off.data();
    }
    q.nfiles = b - a;
    q.h_data = in.h_data ? in.h_data + sg.b0 : nullptr;
    q.d_data = resident ? static_cast<const uint8_t*>(in.d_data) + sg.b0 : nullptr;
    q.paths = in.paths ? in.paths + a : nullptr;
    q.path_lens = in.path_lens ? in.path_lens + a : nullptr;
    q.binary = in.binary ? in.binary + a : nullptr;
    // a resident piece after the first starts at an arbitrary file offset:
    // K1 reads 64-byte lines from the piece's base, and a base off the
    // 128-byte L2 line grid made it fetch 2.4 HBM bytes per content byte
    // (aligned pieces 1.5, profiles/rd4k traffic runs).  Start it at the
    // 256-byte boundary below, the bytes in between a lead file.
    const uint64_t delta = resident && k > 0 ? (reinterpret_cast<uintptr_t>(in.d_data) + sg.b0) & 255u : 0;
    if (delta && in.paths) {               // (h_data is null in a device-only scan)
      sg.lead = 1;
      sg.off.insert(sg.off.begin(), 0);
      for (size_t i = 1; i < sg.off.size(); ++i) sg.off[i] += delta;
      q.offsets = sg.off.data();
      q.nfiles = b - a + 1;
      if (q.h_data) q.h_data -= delta;
      q.d_data = static_cast<const uint8_t*>(q.d_data) - delta;
      sg.lead_paths.assign(1, "");
      sg.lead_paths.insert(sg.lead_paths.end(), in.paths + a, in.paths + b);
      q.paths = sg.lead_paths.data();
      if (in.path_lens) {
        sg.lead_lens.assign(1, 0);
        sg.lead_lens.insert(sg.lead_lens.end(), in.path_lens + a, in.path_lens + b);
        q.path_lens = sg.lead_lens.data();
      }
      if (in.binary) {
        sg.lead_bin.assign(1, 0);
        sg.lead_bin.insert(sg.lead_bin.end(), in.binary + a, in.binary + b);
        q.binary = sg.lead_bin.data();
      }
    }
  }
}

}  // namespace tsg
