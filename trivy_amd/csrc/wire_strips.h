// Where the wire feeder (WireFeed, engine.hip) cuts a segment into strips:
// one strip is what one packer packs and one copy carries.  Pure arithmetic --
// no HIP, no device -- so the cut is tested on the CPU
// (tsg_test_plan_wire_strips, tests/test_wire_strips.py).
//
// The rules of every plan:
//   * the strips cover [0, segment_bytes) in order, no holes, no overlap;
//   * no strip is longer than `strip`, and only a segment's last strip may
//     have a length that is no multiple of kWireBlock;
//   * where `strip` is a multiple of kWireStripAlign, every offset is: the 6-bit
//     codec's alphabet regions (kWire2Region bytes from the strip's start)
//     then cover the same bytes whatever the cut, so a block's packed bytes do
//     not depend on it.
//
// The uniform cut is strip k = [k strip, (k + 1) strip).  A scan's first
// segment gets a ramp instead: the packers start with the scan, and until
// their first strips are ready the feeder sends strips unpacked from the
// segment's back.  With whole strips at both ends that was ten raw 64 MiB
// strips per scan (7-9 ms per packer for the first strip).  Tiers of equal
// small strips (npackers of strip / 16, then of strip / 4) did not help: the
// packers still finish each tier together, a tier takes four times as long to
// pack as the one before it to send, and while 14 strips wait to be sent only
// the three spare staging slots are free to pack into.  The ramp:
//
//   front   m = kWireRampRounds x npackers strips, strip i of (i + 1) / m of
//           `strip` (down to a multiple of kWireStripAlign): the first is
//           ready after 1 / m of a whole strip's time, and the packers, which
//           take them in order, finish one after the other from then on, not
//           all at once: what the link is offered grows as fast as the
//           packers can make it grow, and a packer never waits for one of the
//           lane's staging slots behind a pile of strips that became ready
//           together;
//   middle  whole strips (the last one short: a multiple of kWireStripAlign);
//   back    kWireRampBack pieces of strip / 16 (from the kWireStripAlign
//           boundary at or below): what goes raw while the packers ramp up is
//           taken in small pieces, and so are the copies the feeder queues
//           ahead before anything is packed.
//
// No ramp (the uniform cut) for a later segment -- the packers work one
// segment ahead, its first strips are ready when the feeder gets there --,
// without packers, for strips under kWireRampMinStrip or no multiple of it
// (the tests' 64 KiB strips: their counts are pinned), and for a segment too
// short for the front and the back.
#pragma once
#include <cstdint>
#include <vector>

namespace tsg {

struct WireStrip { uint64_t offset, bytes; };

constexpr uint64_t kWireStripAlign = 65536;          // = kWire2Region (wirepack.h)
constexpr uint64_t kWireRampMinStrip = 1ull << 20;   // 16 alignment units: strip / 16 stays aligned
// (measured, DESIGN section 8: one round against two and three, and against tiers of equal strips)
constexpr uint32_t kWireRampRounds = 1;
constexpr uint32_t kWireRampBack = 32;
constexpr uint32_t kWireRampBackDiv = 16;

// bytes of front strip i of m
inline uint64_t wire_ramp_front(uint64_t strip, uint64_t i, uint64_t m) {
  const uint64_t b = strip / kWireStripAlign * (i + 1) / m * kWireStripAlign;
  return b ? b : kWireStripAlign;
}

inline std::vector<WireStrip> plan_wire_strips(uint64_t segment_bytes, uint64_t strip, bool first_segment, int npackers) {
  std::vector<WireStrip> plan;
  if (segment_bytes == 0 || strip == 0) return plan;
  auto run = [&](uint64_t from, uint64_t to, uint64_t step) {
    for (uint64_t o = from; o < to; o += step) plan.push_back({o, to - o < step ? to - o : step});
  };
  const uint64_t m = static_cast<uint64_t>(kWireRampRounds) * static_cast<uint64_t>(npackers > 0 ? npackers : 0);
  bool ramp = first_segment && m > 0 && strip >= kWireRampMinStrip && strip % kWireRampMinStrip == 0;
  uint64_t front = 0;
  if (ramp) for (uint64_t i = 0; i < m; ++i) front += wire_ramp_front(strip, i, m);
  const uint64_t back_bytes = kWireRampBack * (strip / kWireRampBackDiv);
  ramp = ramp && segment_bytes >= front + back_bytes;
  if (!ramp) {
    run(0, segment_bytes, strip);
    return plan;
  }
  uint64_t o = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const uint64_t b = wire_ramp_front(strip, i, m);
    plan.push_back({o, b});
    o += b;
  }
  const uint64_t back = (segment_bytes - back_bytes) / kWireStripAlign * kWireStripAlign;   // >= front, which is aligned
  run(front, back, strip);
  run(back, segment_bytes, strip / kWireRampBackDiv);
  return plan;
}

}  // namespace tsg
