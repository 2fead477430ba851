// Device-side content preparation of a raw batch (prep.hip): what it
// computes, stated sequentially on the CPU.  No HIP here.
//
// Analyze's preparation (pkg/fanal/analyzer/secret/secret.go:103-150) per
// file: IsBinary on the first 300 bytes (utils.go:68-86); a binary that is
// not allowed (.pyc) is dropped; text loses every '\r'; an allowed binary
// becomes ExtractPrintableBytes (utils.go:111-143).  The last is local: byte
// i of such a file is kept iff it is printable and some window of 5
// consecutive printable bytes of the same file contains it, and a '\n'
// follows it iff it is kept and byte i + 1 is not printable or is the file's
// end.  So every input byte emits 0, 1 or 2 output bytes, decided from the
// bytes i - 4 ... i + 4 of its file and the file's kind, and the prepared
// batch is one stream compaction of the raw one.
#pragma once
#include <cstdint>
#include <vector>

#include "goregexp.h"

namespace tsg {

// per-file flags the host's gate hands to the device pass
constexpr uint8_t kPrepGate = 1;      // filePatternMatch || Required (feed.cpp: wants)
constexpr uint8_t kPrepAllowed = 2;   // allowedBinary: filepath.Ext(path) == ".pyc"
// what the pass makes of a file
constexpr uint8_t kPrepDropped = 0, kPrepText = 1, kPrepPrintable = 2;
constexpr uint32_t kPrepHead = 300;   // IsBinary looks at the first 300 bytes

// IsBinary's per-byte test (utils.go:74-80)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool prep_trigger(uint32_t b) {
  return b < 7 || b == 11 || (13 < b && b < 27) || (27 < b && b < 0x20) || b == 0x7f;
}

// unicode.IsPrint(rune(b)) for the 256 byte values, one bit each (re::is_print)
inline void prep_print_table(uint32_t tab[8]) {
  for (int w = 0; w < 8; ++w) tab[w] = 0;
  for (uint32_t b = 0; b < 256; ++b)
    if (re::is_print(b)) tab[b >> 5] |= 1u << (b & 31);
}

inline uint8_t prep_kind(uint8_t flags, const uint8_t* c, uint64_t n) {
  if (!(flags & kPrepGate)) return kPrepDropped;
  bool binary = false;
  for (uint64_t i = 0; i < n && i < kPrepHead && !binary; ++i) binary = prep_trigger(c[i]);
  if (!binary) return kPrepText;
  return (flags & kPrepAllowed) ? kPrepPrintable : kPrepDropped;
}

struct PrepPlan {
  std::vector<uint8_t> kinds;      // nfiles
  std::vector<uint64_t> new_off;   // nfiles + 1: every file's start in out (a dropped file has zero length)
  std::vector<uint8_t> out;        // the prepared bytes
};

// The device pass on the host: kinds, new starts and output bytes of the raw
// batch raw[0, off[nfiles]) with the per-byte emit rule above.
inline void plan_prep(const uint8_t* raw, const uint64_t* off, uint32_t nfiles, const uint8_t* flags, PrepPlan* p) {
  uint32_t tab[8];
  prep_print_table(tab);
  auto pr = [&](uint8_t b) { return (tab[b >> 5] >> (b & 31)) & 1u; };
  p->kinds.assign(nfiles, 0);
  p->new_off.assign(nfiles + 1, 0);
  p->out.clear();
  for (uint32_t f = 0; f < nfiles; ++f) {
    const uint64_t s = off[f], e = off[f + 1];
    p->new_off[f] = p->out.size();
    const uint8_t kind = prep_kind(flags[f], raw + s, e - s);
    p->kinds[f] = kind;
    if (kind == kPrepText) {
      for (uint64_t i = s; i < e; ++i) if (raw[i] != '\r') p->out.push_back(raw[i]);
    } else if (kind == kPrepPrintable) {
      for (uint64_t i = s; i < e; ++i) {
        if (!pr(raw[i])) continue;
        bool kept = false;
        for (uint64_t a = i >= s + 4 ? i - 4 : s; a <= i && a + 5 <= e && !kept; ++a)   // windows [a, a + 5) holding i
          kept = pr(raw[a]) && pr(raw[a + 1]) && pr(raw[a + 2]) && pr(raw[a + 3]) && pr(raw[a + 4]);
        if (!kept) continue;
        p->out.push_back(raw[i]);
        if (i + 1 == e || !pr(raw[i + 1])) p->out.push_back('\n');
      }
    }
  }
  p->new_off[nfiles] = p->out.size();
}

}  // namespace tsg
