// K1's guided work schedule, restated on the host: plain C++, no HIP.
//
// tsg_k1_scan_v3 (engine.hip, "Guided work schedule") cuts a launch's nchunks
// into levels of 8-, 4-, 2- and 1-chunk lane ranges, in that order through the
// batch, and into wave items of 64 lanes each.  Wave w of the grid takes item
// w without an atomic; the rest come from eight counters, one per XCD, that
// the workgroups with blockIdx.x % 8 == xc share.  The kernel keeps its own
// arithmetic (it belongs to K1's build hash); this file states the same
// schedule a second way, level by level from the short ranges up, for
//  - the host's guard that every item of a launch has a taker (k1_grid_ok,
//    Engine::seg_prologue), and
//  - the tests that pin the kernel to it (tsg_test_k1_schedule,
//    tests/test_schedule_corpus.py on the CPU, tests/test_gpu_k1_schedule.py
//    on the GPU).
#ifndef TSG_K1_SCHEDULE_H_
#define TSG_K1_SCHEDULE_H_

#include <algorithm>
#include <cstdint>

namespace tsg {

constexpr uint32_t kK1ItemLanes = 64;        // lanes of a wave item
constexpr uint32_t kK1WavesPerBlock = 16;    // a K1 workgroup: 1024 threads
constexpr uint32_t kK1Counters = 8;          // per-XCD item counters of a launch

// Level l holds the lane ranges of (1 << l) chunks: level[0] = kU 1 .. level[3] = kU 8.
struct K1Levels {
  uint64_t chunks[4] = {0, 0, 0, 0};   // chunks of the launch in the level
  uint64_t items[4] = {0, 0, 0, 0};    // wave items of the level (the last may be partial)
  uint64_t nitems = 0;
  // first chunk of the level: the levels lie in the batch from kU 8 down to kU 1
  uint64_t first_chunk(int l) const {
    uint64_t c = 0;
    for (int k = 3; k > l; --k) c += chunks[k];
    return c;
  }
  // first item of the level: items are numbered in batch order
  uint64_t first_item(int l) const {
    uint64_t i = 0;
    for (int k = 3; k > l; --k) i += items[k];
    return i;
  }
};

// The levels of a launch of nchunks chunks on W waves (gridDim.x * 16):
// `rounds` grid-wide rounds (W items) of 1-chunk ranges, as many of 2-chunk
// ranges, the rest in 4-chunk ranges -- or, with top8, `rounds` rounds of
// those too and the rest in 8-chunk ranges.  The short levels are filled
// first, so a small launch has only them.
inline K1Levels k1_levels(uint64_t nchunks, uint64_t W, uint32_t rounds, bool top8) {
  K1Levels lv;
  const int top = top8 ? 3 : 2;
  uint64_t left = nchunks;
  for (int l = 0; l <= top; ++l) {
    const uint64_t per_item = static_cast<uint64_t>(kK1ItemLanes) << l;
    const uint64_t take = l == top ? left : std::min(left, W * per_item * rounds);
    lv.chunks[l] = take;
    lv.items[l] = (take + per_item - 1) / per_item;
    lv.nitems += lv.items[l];
    left -= take;
  }
  return lv;
}

// Item `item` < nitems: its lanes' range length kU, its first chunk c0 (lane
// j walks chunks [c0 + j * kU, min(c0 + (j + 1) * kU, rend)), none if that is
// empty) and its level's end rend.
struct K1Item {
  uint32_t kU = 0;
  uint64_t c0 = 0, rend = 0;
};
inline K1Item k1_item(const K1Levels& lv, uint64_t item) {
  K1Item it;
  for (int l = 3; l >= 0; --l) {
    const uint64_t i0 = lv.first_item(l);
    if (item < i0 + lv.items[l]) {
      it.kU = 1u << l;
      it.c0 = lv.first_chunk(l) + (item - i0) * (static_cast<uint64_t>(kK1ItemLanes) << l);
      it.rend = lv.first_chunk(l) + lv.chunks[l];
      return it;
    }
  }
  return it;                           // (item >= nitems: kU 0)
}

// The k-th item counter xc (< kK1Counters) hands out, k = 0, 1, ...: the
// items past the static round, dealt round-robin to the counters.
inline uint64_t k1_counter_item(uint64_t W, uint32_t xc, uint64_t k) { return W + xc + kK1Counters * k; }

// Whether every item of a launch has a taker: counter xc is read only by the
// workgroups with blockIdx.x % 8 == xc, so a grid of fewer than 8 workgroups
// must hold all its items in the static round.
inline bool k1_grid_ok(uint64_t blocks, uint64_t nitems, uint64_t W) { return blocks >= kK1Counters || nitems <= W; }

}  // namespace tsg

#endif  // TSG_K1_SCHEDULE_H_
