// Decoding zstd layer blobs (zstdec.hip): RFC 8878 frames, stated once for the
// host and the device, and the sequential CPU model of the device pass.  No
// HIP here.
//
// The reference opens a layer with layer.Uncompressed()
// (pkg/fanal/artifact/image/image.go:464-492); go-containerregistry v0.20.3
// peeks the first bytes and wraps a zstd reader (klauspost/compress) around a
// blob that starts 28 b5 2f fd.  That decoder's source is not at hand, so the
// rules below are RFC 8878's, checked against libzstd on valid streams, and
// the statuses are this project's own:
//   frames      concatenated frames decode one behind the other; skippable
//               frames (50..5f 2a 4d 18 + a 4-byte size) are stepped over; no
//               bytes left ends the stream, fewer than four is an unexpected end
//   header      descriptor: FCS flag, single segment, reserved bit 3 (a header
//               error), checksum flag, dictionary-ID flag; window descriptor
//               (10 + exponent, mantissa in eighths; above 2^31 is a header
//               error); a non-zero Dictionary_ID is kZsDict; a
//               Frame_Content_Size that is not what was decoded is corrupt
//   blocks      raw, RLE, compressed; type 3 is corrupt, as is a block above
//               Block_Maximum_Size = min(Window_Size, 128 KiB) -- in its size
//               field or in what a compressed block regenerates -- and a
//               compressed block below 3 bytes or of 128 KiB (libzstd's limits)
//   literals    raw, RLE, Huffman with one or four streams, treeless (corrupt
//               without an earlier tree in the frame); weights direct or
//               FSE-compressed (accuracy <= 6), the last weight implied, codes
//               of at most 11 bits; every stream read backwards from its last
//               set bit and consumed exactly
//   sequences   count of 1, 2 or 3 bytes; predefined, RLE, FSE and repeat mode
//               per table (repeat without a table and reserved bits are
//               corrupt); accuracy <= 9 / 8 / 9; repeat offsets 1, 4, 8 per
//               frame; offset codes above 31 and an offset reaching before the
//               frame's first output byte are corrupt; the bitstream is
//               consumed exactly
//   checksum    the low 32 bits of XXH64 (seed 0) of the frame's content
// zstd_decode is the decoder both sides run: input bytes, table stores,
// literal stores, the literal copy, the match copy and the frame record go
// through an Io policy (ZsHostIo below; WaveIo in zstdec.hip), so the bounds
// logic the wavefront executes is the logic the sanitizers see on the host.
// The decoder checks no checksum: it records every frame's output range with
// the checksum that follows it, a second pass hashes each range
// (zs_xxh64; tsg_zstd_hash_frames on the device) and zs_check_frames compares.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// The decoder is inlined into the kernel whole: the Io policy then lives in
// registers, not in scratch memory behind a reference
#if defined(__HIPCC__)
#define TSG_ZS_HD __host__ __device__ __attribute__((always_inline))
#else
#define TSG_ZS_HD
#endif
// A value every lane of the wavefront holds alike, moved to a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
#define TSG_ZS_UNIFORM(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#else
#define TSG_ZS_UNIFORM(x) static_cast<uint32_t>(x)
#endif

namespace tsg {

// per-stream status (TSG_ZSTD_* of trivy_secret.h)
enum : int32_t { kZsOk = 0, kZsHeader = 1, kZsCorrupt = 2, kZsEof = 3, kZsChecksum = 4, kZsDict = 5, kZsDstFull = 6 };

inline const char* zstd_status_text(int32_t st) {
  switch (st) {
    case kZsHeader: return "zstd: invalid frame header";
    case kZsCorrupt: return "zstd: corrupt input";
    case kZsEof: return "zstd: unexpected end of input";
    case kZsChecksum: return "zstd: invalid checksum";
    case kZsDict: return "zstd: a dictionary is required";
    default: return "";                            // kZsOk; kZsDstFull is no error of the stream's
  }
}

constexpr uint32_t kZsMagic = 0xfd2fb528u;
constexpr uint32_t kZsSkipMagic = 0x184d2a50u;     // low nibble free
constexpr uint32_t kZsBlockMax = 128u * 1024u;
constexpr uint32_t kZsMinFrame = 9;                // magic 4, descriptor 1, window or FCS 1, one block header 3
constexpr uint32_t kZsHufLogMax = 11;
constexpr uint32_t kZsLLMax = 35, kZsMLMax = 52, kZsOFMax = 31;

// What a stream exercised: counters of the CPU model (tools/gen_zstd_corpus.py
// asserts that a fixture holds what it was built for).  The device ignores them.
enum : uint32_t {
  kEvFrame, kEvSkippable, kEvSingleSegment, kEvChecksum, kEvFcs0, kEvFcs1, kEvFcs2, kEvFcs4, kEvFcs8,
  kEvBlockRaw, kEvBlockRle, kEvBlockCompressed,
  kEvLitRaw, kEvLitRle, kEvLitHuf1, kEvLitHuf4, kEvLitTreeless, kEvLitFmt0, kEvLitFmt1, kEvLitFmt3,
  kEvWeightsDirect, kEvWeightsFse, kEvHufBits11,
  kEvLLPredef, kEvLLRle, kEvLLFse, kEvLLRepeat, kEvOFPredef, kEvOFRle, kEvOFFse, kEvOFRepeat,
  kEvMLPredef, kEvMLRle, kEvMLFse, kEvMLRepeat,
  kEvRep1, kEvRep2, kEvRep3, kEvRep1LL0, kEvRep2LL0, kEvRep3LL0,
  kEvSeq0, kEvSeq127, kEvSeq128, kEvSeqLong,
  kEvOff32768, kEvOff32769, kEvOffFar, kEvFarSameLine, kEvStraddle, kEvLongOverlap, kEvEmptyFrame,
  kEvOffRingEdge, kEvOffRingEdge1,
  kEvCount
};

// LDS on the device: the three sequence tables, the Huffman table and what
// building them needs.  A sequence / weight entry is symbol | bits << 8 |
// base << 16, a Huffman entry symbol | bits << 8.
struct ZsTables {
  uint32_t ll[512], ml[512], of[256];
  uint32_t wfse[64];
  uint16_t huf[1u << kZsHufLogMax];
  int16_t norm[256];
  uint16_t next[256];
  uint8_t weights[256];
  uint32_t ok, huf_log;
};
// A frame's output range inside its stream's slot and the checksum behind it
struct ZsFrameRec {
  uint64_t out_begin, out_end;
  uint32_t has_sum, sum;
};
inline uint32_t zstd_frame_cap(uint64_t len) { return static_cast<uint32_t>(len / kZsMinFrame + 1); }

// What persists from block to block inside a frame; all of it uniform
struct ZsFrameState {
  uint32_t rep[3];
  uint32_t ll_log, ml_log, of_log;
  bool have_ll, have_ml, have_of, have_huf;
  uint32_t huf_log;
};
// Where a block's literals lie
struct ZsLit {
  uint32_t kind;                                   // 0: in the input at pos; 1: the byte val repeated; 2: the literal scratch
  uint32_t size;
  uint64_t pos;
  uint32_t val;
};

TSG_ZS_HD inline uint32_t zs_highbit(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v)); }   // v != 0

// ---- XXH64 ----
constexpr uint64_t kXxP1 = 0x9E3779B185EBCA87ull, kXxP2 = 0xC2B2AE3D27D4EB4Full, kXxP3 = 0x165667B19E3779F9ull,
                   kXxP4 = 0x85EBCA77C2B2AE63ull, kXxP5 = 0x27D4EB2F165667C5ull;
TSG_ZS_HD inline uint64_t zs_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64 - r)); }
TSG_ZS_HD inline uint64_t zs_xx_round(uint64_t acc, uint64_t v) { return zs_rotl(acc + v * kXxP2, 31) * kXxP1; }
TSG_ZS_HD inline uint64_t zs_xx_merge(uint64_t h, uint64_t v) { return (h ^ zs_xx_round(0, v)) * kXxP1 + kXxP4; }
// XXH64 of n bytes, seed 0; ld.w64(i) / ld.w32(i) / ld.w8(i) read little-endian at byte i
template <class Ld>
TSG_ZS_HD inline uint64_t zs_xxh64(Ld ld, uint64_t n) {
  uint64_t i = 0, h;
  if (n >= 32) {
    uint64_t v1 = kXxP1 + kXxP2, v2 = kXxP2, v3 = 0, v4 = 0 - kXxP1;
    for (; n - i >= 128; i += 128) {               // sixteen loads in flight, then four stripes
      uint64_t w[16];
      for (uint32_t k = 0; k < 16; ++k) w[k] = ld.w64(i + 8 * k);
      for (uint32_t k = 0; k < 16; k += 4) {
        v1 = zs_xx_round(v1, w[k]);
        v2 = zs_xx_round(v2, w[k + 1]);
        v3 = zs_xx_round(v3, w[k + 2]);
        v4 = zs_xx_round(v4, w[k + 3]);
      }
    }
    for (; n - i >= 32; i += 32) {
      v1 = zs_xx_round(v1, ld.w64(i));
      v2 = zs_xx_round(v2, ld.w64(i + 8));
      v3 = zs_xx_round(v3, ld.w64(i + 16));
      v4 = zs_xx_round(v4, ld.w64(i + 24));
    }
    h = zs_rotl(v1, 1) + zs_rotl(v2, 7) + zs_rotl(v3, 12) + zs_rotl(v4, 18);
    h = zs_xx_merge(h, v1);
    h = zs_xx_merge(h, v2);
    h = zs_xx_merge(h, v3);
    h = zs_xx_merge(h, v4);
  } else {
    h = kXxP5;
  }
  h += n;
  for (; n - i >= 8; i += 8) h = zs_rotl(h ^ zs_xx_round(0, ld.w64(i)), 27) * kXxP1 + kXxP4;
  if (n - i >= 4) {
    h = zs_rotl(h ^ (static_cast<uint64_t>(ld.w32(i)) * kXxP1), 23) * kXxP2 + kXxP3;
    i += 4;
  }
  for (; i < n; ++i) h = zs_rotl(h ^ (static_cast<uint64_t>(ld.w8(i)) * kXxP5), 11) * kXxP1;
  h ^= h >> 33;
  h *= kXxP2;
  h ^= h >> 29;
  h *= kXxP3;
  h ^= h >> 32;
  return h;
}
struct ZsByteLd {                                  // little-endian from single bytes: any alignment
  const uint8_t* p;
  TSG_ZS_HD uint32_t w8(uint64_t i) const { return p[i]; }
  TSG_ZS_HD uint32_t w32(uint64_t i) const { return p[i] | p[i + 1] << 8 | p[i + 2] << 16 | static_cast<uint32_t>(p[i + 3]) << 24; }
  TSG_ZS_HD uint64_t w64(uint64_t i) const { return w32(i) | static_cast<uint64_t>(w32(i + 4)) << 32; }
};

// ---- bit readers ----
// Forward, least significant bit first, over the input bytes [ip, end): the
// FSE table descriptions.  Bits past end read as zero and set over.
struct ZsFwd {
  uint64_t ip = 0, end = 0, bb = 0;
  uint32_t nb = 0;
  bool over = false;
  template <class Io>
  TSG_ZS_HD uint32_t peek(Io& io, uint32_t k) {    // k <= 24
    while (nb < k && ip < end) {
      bb |= static_cast<uint64_t>(io.in(ip)) << nb;
      ++ip;
      nb += 8;
    }
    return static_cast<uint32_t>(bb) & ((1u << k) - 1u);
  }
  TSG_ZS_HD void drop(uint32_t k) {
    if (k > nb) { over = true; bb = 0; nb = 0; return; }
    bb >>= k;
    nb -= k;
  }
  TSG_ZS_HD uint64_t byte_end() const { return ip - (nb >> 3); }   // the first byte no bit was taken from
};
// Backward over the input bytes [lo, end), from the bit below the last set bit
// of byte end - 1 down to bit 0 of byte lo, most significant first.  rd(pos)
// reads a byte and rd.w32(pos) four, little-endian (ZsRdBack: the uniform
// window; ZsRdLane: a lane's own loads).  Taking more than
// is left pads with zeros and sets over.
template <class Io>
struct ZsRdBack {
  Io* io;
  TSG_ZS_HD uint32_t operator()(uint64_t p) const { return io->in_back(p); }
  TSG_ZS_HD uint32_t w32(uint64_t p) const { return io->in_back32(p); }
};
template <class Io>
struct ZsRdLane {
  Io* io;
  TSG_ZS_HD uint32_t operator()(uint64_t p) const { return io->in_lane(p); }
  TSG_ZS_HD uint32_t w32(uint64_t p) const { return io->in_lane32(p); }
};
struct ZsBack {
  uint64_t lo = 0, ip = 0, bb = 0;
  uint32_t nb = 0;
  bool over = false;
  template <class Rd>
  TSG_ZS_HD bool init(Rd rd, uint64_t begin, uint64_t end) {
    if (end <= begin) return false;
    const uint32_t last = rd(end - 1) & 0xffu;
    if (!last) return false;
    nb = zs_highbit(last);
    bb = last & ((1u << nb) - 1u);
    ip = end - 1;
    lo = begin;
    return true;
  }
  template <class Rd>
  TSG_ZS_HD uint32_t peek(Rd rd, uint32_t k) {     // k <= 32
    if (k == 0) return 0;
    if (nb < k) {
      if (nb <= 32 && ip - lo >= 4) {              // four bytes at once: their loads do not wait for one another
        ip -= 4;
        bb = (bb << 32) | rd.w32(ip);
        nb += 32;
      }
      while (nb < k && ip > lo) {
        --ip;
        bb = (bb << 8) | (rd(ip) & 0xffu);
        nb += 8;
      }
    }
    const uint64_t m = (uint64_t(1) << k) - 1u;
    return static_cast<uint32_t>((nb >= k ? bb >> (nb - k) : bb << (k - nb)) & m);
  }
  TSG_ZS_HD void drop(uint32_t k) {
    if (k > nb) { over = true; nb = 0; bb = 0; return; }
    nb -= k;
  }
  template <class Rd>
  TSG_ZS_HD uint32_t take(Rd rd, uint32_t k) {
    const uint32_t v = peek(rd, k);
    drop(k);
    return v;
  }
  TSG_ZS_HD bool done() const { return !over && nb == 0 && ip == lo; }
};

// ---- FSE ----
// A table description from [ip, end) into t->norm[0, *nsyms): the accuracy in
// *log (at most max_log), *next = the first byte behind it.
template <class Io>
TSG_ZS_HD inline bool zs_read_ncount(Io& io, ZsTables* t, uint64_t ip, uint64_t end, uint32_t max_sym, uint32_t max_log,
                                     uint32_t* log, uint32_t* nsyms, uint64_t* next) {
  ZsFwd f;
  f.ip = ip;
  f.end = end;
  const uint32_t lg = f.peek(io, 4) + 5u;
  f.drop(4);
  if (lg > max_log || f.over) return false;
  int32_t remaining = (1 << lg) + 1, threshold = 1 << lg;
  uint32_t nbits = lg + 1, sym = 0;
  bool prev0 = false;
  io.sync();
  while (remaining > 1 && sym <= max_sym) {
    if (prev0) {
      uint32_t n0 = sym;
      for (;;) {
        const uint32_t r = f.peek(io, 2);
        f.drop(2);
        if (f.over) return false;
        n0 += r;
        if (r != 3) break;
        if (n0 > max_sym) return false;
      }
      if (n0 > max_sym) return false;
      for (; sym < n0; ++sym)
        if (io.leader()) t->norm[sym] = 0;
    }
    const int32_t max = (2 * threshold - 1) - remaining;
    const int32_t v = static_cast<int32_t>(f.peek(io, nbits));
    int32_t count;
    if ((v & (threshold - 1)) < max) {
      count = v & (threshold - 1);
      f.drop(nbits - 1);
    } else {
      count = v & (2 * threshold - 1);
      if (count >= threshold) count -= max;
      f.drop(nbits);
    }
    if (f.over) return false;
    --count;
    remaining -= count < 0 ? -count : count;
    if (io.leader()) t->norm[sym] = static_cast<int16_t>(count);
    ++sym;
    prev0 = count == 0;
    while (remaining < threshold) {
      --nbits;
      threshold >>= 1;
    }
  }
  if (remaining != 1) return false;
  *log = lg;
  *nsyms = sym;
  *next = f.byte_end();
  return true;
}

// The decoding table of norm[0, nsyms) at accuracy log, run by one lane
TSG_ZS_HD inline void zs_fse_build_serial(const int16_t* norm, uint32_t nsyms, uint32_t log, uint32_t* tab, uint16_t* next) {
  const uint32_t size = 1u << log, mask = size - 1;
  uint32_t high = size - 1;
  for (uint32_t s = 0; s < nsyms; ++s) {
    if (norm[s] == -1) {
      tab[high--] = s;
      next[s] = 1;
    } else {
      next[s] = static_cast<uint16_t>(norm[s]);
    }
  }
  const uint32_t step = (size >> 1) + (size >> 3) + 3;
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsyms; ++s)
    for (int32_t i = 0; i < norm[s]; ++i) {
      tab[pos] = s;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = tab[u] & 0xffu, ns = next[s]++;
    const uint32_t nb = log - zs_highbit(ns);
    tab[u] = s | nb << 8 | ((ns << nb) - size) << 16;
  }
}
template <class Io>
TSG_ZS_HD inline void zs_fse_build(Io& io, ZsTables* t, uint32_t nsyms, uint32_t log, uint32_t* tab) {
  io.sync();                                       // the counts the leader wrote
  if (io.leader()) zs_fse_build_serial(t->norm, nsyms, log, tab, t->next);
  io.sync();
}

// One of the three sequence tables by its mode; *ip advances over what it read
template <class Io>
TSG_ZS_HD inline int32_t zs_seq_table(Io& io, ZsTables* t, uint32_t mode, uint32_t which, uint64_t* ip, uint64_t end,
                                      uint32_t* tab, uint32_t* log, bool* have) {
  constexpr int8_t ll_def[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  constexpr int8_t ml_def[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  constexpr int8_t of_def[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  const uint32_t max_sym = which == 0 ? kZsLLMax : which == 1 ? kZsOFMax : kZsMLMax;
  const uint32_t max_log = which == 1 ? 8u : 9u;
  io.note(kEvLLPredef + which * 4 + mode);
  if (mode == 0) {                                 // predefined
    const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
    io.sync();
    if (io.leader())
      for (uint32_t s = 0; s < n; ++s) t->norm[s] = which == 0 ? ll_def[s] : which == 1 ? of_def[s] : ml_def[s];
    *log = which == 1 ? 5u : 6u;
    zs_fse_build(io, t, n, *log, tab);
  } else if (mode == 1) {                          // RLE: one symbol, no bits
    if (*ip >= end) return kZsCorrupt;
    const uint32_t s = io.in(*ip);
    ++*ip;
    if (s > max_sym) return kZsCorrupt;
    io.sync();
    if (io.leader()) tab[0] = s;
    io.sync();
    *log = 0;
  } else if (mode == 2) {                          // FSE-compressed
    uint32_t nsyms = 0;
    if (!zs_read_ncount(io, t, *ip, end, max_sym, max_log, log, &nsyms, ip)) return kZsCorrupt;
    zs_fse_build(io, t, nsyms, *log, tab);
  } else if (!*have) {                             // repeat
    return kZsCorrupt;
  }
  *have = true;
  return kZsOk;
}

// ---- Huffman ----
// The table of t->weights[0, n) (the implied last weight included) into
// t->huf, run by one lane; false when the weights form no complete code of at
// most kZsHufLogMax bits
TSG_ZS_HD inline bool zs_huf_build_serial(ZsTables* t, uint32_t n) {
  uint32_t total = 0;
  for (uint32_t i = 0; i + 1 < n; ++i) {
    const uint32_t w = t->weights[i];
    if (w > kZsHufLogMax) return false;
    total += (1u << w) >> 1;
  }
  if (total == 0) return false;
  const uint32_t log = zs_highbit(total) + 1;
  if (log > kZsHufLogMax) return false;
  const uint32_t rest = (1u << log) - total;
  if (rest & (rest - 1)) return false;             // the last symbol fills what is left: a power of two
  t->weights[n - 1] = static_cast<uint8_t>(zs_highbit(rest) + 1);
  uint32_t rank[kZsHufLogMax + 2];
  for (uint32_t w = 0; w <= kZsHufLogMax + 1; ++w) rank[w] = 0;
  for (uint32_t i = 0; i < n; ++i) ++rank[t->weights[i]];
  if (rank[1] < 2 || (rank[1] & 1u)) return false;
  uint32_t start = 0;
  for (uint32_t w = 1; w <= log; ++w) {
    const uint32_t cur = start;
    start += rank[w] << (w - 1);
    rank[w] = cur;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t w = t->weights[i];
    if (!w) continue;
    const uint32_t len = (1u << w) >> 1, e = i | (log + 1 - w) << 8;
    for (uint32_t u = rank[w]; u < rank[w] + len; ++u) t->huf[u] = static_cast<uint16_t>(e);
    rank[w] += len;
  }
  t->huf_log = log;
  return true;
}

// A Huffman tree description at [ip, end): the weights, then the table.
// *next = the first byte behind it.
template <class Io>
TSG_ZS_HD inline bool zs_huf_tree(Io& io, ZsTables* t, uint64_t ip, uint64_t end, uint64_t* next, uint32_t* huf_log) {
  if (ip >= end) return false;
  const uint32_t hb = io.in(ip);
  ++ip;
  uint32_t n = 0;                                  // weights read
  io.sync();
  if (hb >= 128) {                                 // direct: 4 bits each
    n = hb - 127;
    const uint32_t bytes = (n + 1) / 2;
    if (end - ip < bytes) return false;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t b = io.in(ip + k / 2);
      if (io.leader()) t->weights[k] = static_cast<uint8_t>((k & 1u) ? b & 15u : b >> 4);
    }
    ip += bytes;
    io.note(kEvWeightsDirect);
  } else {                                         // FSE-compressed, two interleaved states
    if (hb == 0 || end - ip < hb) return false;
    const uint64_t wend = ip + hb;
    uint32_t log = 0, nsyms = 0;
    uint64_t bs = 0;
    if (!zs_read_ncount(io, t, ip, wend, 255, 6, &log, &nsyms, &bs)) return false;
    zs_fse_build(io, t, nsyms, log, t->wfse);
    const ZsRdBack<Io> rd{&io};
    ZsBack b;
    if (!b.init(rd, bs, wend)) return false;
    uint32_t s1 = b.take(rd, log), s2 = b.take(rd, log);
    if (b.over) return false;
    for (;;) {
      if (n > 253) return false;
      const uint32_t e1 = TSG_ZS_UNIFORM(t->wfse[s1]);
      if (io.leader()) t->weights[n] = static_cast<uint8_t>(e1);
      ++n;
      s1 = (e1 >> 16) + b.take(rd, (e1 >> 8) & 0xffu);
      if (b.over) {
        if (io.leader()) t->weights[n] = static_cast<uint8_t>(t->wfse[s2]);
        ++n;
        break;
      }
      const uint32_t e2 = TSG_ZS_UNIFORM(t->wfse[s2]);
      if (io.leader()) t->weights[n] = static_cast<uint8_t>(e2);
      ++n;
      s2 = (e2 >> 16) + b.take(rd, (e2 >> 8) & 0xffu);
      if (b.over) {
        if (io.leader()) t->weights[n] = static_cast<uint8_t>(t->wfse[s1]);
        ++n;
        break;
      }
    }
    ip = wend;
    io.note(kEvWeightsFse);
  }
  if (n == 0 || n > 255) return false;
  io.sync();
  if (io.leader()) t->ok = zs_huf_build_serial(t, n + 1) ? 1u : 0u;
  io.sync();
  if (!TSG_ZS_UNIFORM(t->ok)) return false;
  *huf_log = TSG_ZS_UNIFORM(t->huf_log);
  if (*huf_log == kZsHufLogMax) io.note(kEvHufBits11);
  *next = ip;
  return true;
}

// One Huffman stream, input bytes [sb, se), into literals [lb, lb + cnt): run
// by the lane that owns the stream (io.in_lane and io.lit_put are per lane)
template <class Io>
TSG_ZS_HD inline bool zs_huf_stream(Io& io, const ZsTables* t, uint32_t log, uint64_t sb, uint64_t se, uint32_t lb, uint32_t cnt) {
  const ZsRdLane<Io> rd{&io};
  ZsBack b;
  if (!b.init(rd, sb, se)) return false;
  for (uint32_t i = 0; i < cnt; ++i) {
    const uint32_t e = t->huf[b.peek(rd, log)];
    b.drop(e >> 8);
    if (b.over) return false;
    io.lit_put(lb + i, e & 0xffu);
  }
  return b.done();
}

// The literals section of a compressed block at [ip, end): *lit says where the
// literals lie, *next = the first byte of the sequences section
template <class Io>
TSG_ZS_HD inline int32_t zs_literals(Io& io, ZsTables* t, ZsFrameState* fs, uint64_t ip, uint64_t end, ZsLit* lit, uint64_t* next) {
  if (ip >= end) return kZsCorrupt;
  const uint32_t b0 = io.in(ip), type = b0 & 3u, fmt = (b0 >> 2) & 3u;
  if (type < 2) {
    uint32_t hs, size;
    if (fmt == 0 || fmt == 2) {
      hs = 1;
      size = b0 >> 3;
      io.note(kEvLitFmt0);
    } else if (fmt == 1) {
      if (end - ip < 2) return kZsCorrupt;
      hs = 2;
      size = (b0 | io.in(ip + 1) << 8) >> 4;
      io.note(kEvLitFmt1);
    } else {
      if (end - ip < 3) return kZsCorrupt;
      hs = 3;
      size = (b0 | io.in(ip + 1) << 8 | io.in(ip + 2) << 16) >> 4;
      io.note(kEvLitFmt3);
    }
    if (size > kZsBlockMax) return kZsCorrupt;
    ip += hs;
    lit->size = size;
    if (type == 0) {
      if (end - ip < size) return kZsCorrupt;
      lit->kind = 0;
      lit->pos = ip;
      *next = ip + size;
      io.note(kEvLitRaw);
    } else {
      if (ip >= end) return kZsCorrupt;
      lit->kind = 1;
      lit->val = io.in(ip);
      *next = ip + 1;
      io.note(kEvLitRle);
    }
    return kZsOk;
  }
  // Huffman: sizes, [tree,] one or four streams
  uint32_t hs, regen, comp, nstreams = fmt == 0 ? 1u : 4u;
  if (end - ip < 3) return kZsCorrupt;
  const uint32_t h3 = b0 | io.in(ip + 1) << 8 | io.in(ip + 2) << 16;
  if (fmt < 2) {
    hs = 3;
    regen = (h3 >> 4) & 0x3ffu;
    comp = h3 >> 14;
  } else if (fmt == 2) {
    if (end - ip < 4) return kZsCorrupt;
    hs = 4;
    const uint32_t h4 = h3 | io.in(ip + 3) << 24;
    regen = (h4 >> 4) & 0x3fffu;
    comp = h4 >> 18;
  } else {
    if (end - ip < 5) return kZsCorrupt;
    hs = 5;
    const uint32_t h4 = h3 | io.in(ip + 3) << 24;
    regen = (h4 >> 4) & 0x3ffffu;
    comp = (h4 >> 22) | io.in(ip + 4) << 10;
  }
  ip += hs;
  if (regen == 0 || regen > kZsBlockMax || comp == 0 || end - ip < comp) return kZsCorrupt;
  const uint64_t lend = ip + comp;
  if (type == 2) {
    if (!zs_huf_tree(io, t, ip, lend, &ip, &fs->huf_log)) return kZsCorrupt;
    fs->have_huf = true;
  } else {
    if (!fs->have_huf) return kZsCorrupt;
    io.note(kEvLitTreeless);
  }
  if (ip >= lend) return kZsCorrupt;
  const uint32_t log = fs->huf_log;
  bool ok;
  if (nstreams == 1) {
    io.note(kEvLitHuf1);
    const uint64_t sb = ip;
    ok = io.huf_run(1, [&io, t, log, sb, lend, regen](uint32_t) { return zs_huf_stream(io, t, log, sb, lend, 0, regen); });
  } else {
    io.note(kEvLitHuf4);
    if (lend - ip < 10) return kZsCorrupt;
    const uint32_t l1 = io.in(ip) | io.in(ip + 1) << 8, l2 = io.in(ip + 2) | io.in(ip + 3) << 8,
                   l3 = io.in(ip + 4) | io.in(ip + 5) << 8;
    const uint64_t s1 = ip + 6;
    if (lend - s1 < uint64_t(l1) + l2 + l3 + 1) return kZsCorrupt;
    const uint32_t seg = (regen + 3) / 4;
    if (3 * seg > regen) return kZsCorrupt;
    const uint32_t last = regen - 3 * seg;
    ok = io.huf_run(4, [&io, t, log, s1, l1, l2, l3, lend, seg, last](uint32_t k) {
      const uint64_t sb = s1 + (k > 0 ? l1 : 0u) + (k > 1 ? l2 : 0u) + (k > 2 ? l3 : 0u);
      const uint64_t se = k == 0 ? s1 + l1 : k == 1 ? s1 + l1 + l2 : k == 2 ? s1 + l1 + l2 + l3 : lend;
      return zs_huf_stream(io, t, log, sb, se, k * seg, k == 3 ? last : seg);
    });
  }
  if (!ok) return kZsCorrupt;
  lit->kind = 2;
  lit->size = regen;
  lit->pos = 0;
  *next = lend;
  return kZsOk;
}

// ll literals from lit at *lpos to the output at op
template <class Io>
TSG_ZS_HD inline void zs_put_literals(Io& io, const ZsLit& lit, uint32_t lpos, uint64_t op, uint32_t ll) {
  if (!ll) return;
  if (lit.kind == 0) io.copy_in(op, lit.pos + lpos, ll);
  else if (lit.kind == 1) io.fill(op, lit.val, ll);
  else io.copy_lit(op, lpos, ll);
}

// The sequences section [ip, end) of a compressed block, executed
template <class Io>
TSG_ZS_HD inline int32_t zs_sequences(Io& io, ZsTables* t, ZsFrameState* fs, uint64_t ip, uint64_t end, const ZsLit& lit,
                                      uint64_t fbegin, uint64_t block_max, uint64_t cap, uint64_t* op_io) {
  constexpr uint8_t ll_bits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                   1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  constexpr uint32_t ll_base[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,   15,    16,    18,
                                    20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
  constexpr uint8_t ml_bits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                   0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  constexpr uint32_t ml_base[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,  17,  18,  19,   20,
                                    21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,  35,  37,  39,   41,
                                    43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
  uint64_t& op = *op_io;                           // what is written, whichever way the block ends
  const uint64_t bbegin = op;                      // the block may regenerate at most block_max bytes from here
  if (ip >= end) return kZsCorrupt;
  uint32_t nseq = io.in(ip);
  ++ip;
  if (nseq == 0) {
    io.note(kEvSeq0);
    if (ip != end || lit.size > block_max) return kZsCorrupt;
    if (lit.size > cap - op) return kZsDstFull;
    zs_put_literals(io, lit, 0, op, lit.size);
    op += lit.size;
    return kZsOk;
  }
  if (nseq >= 128) {
    if (nseq == 255) {
      if (end - ip < 2) return kZsCorrupt;
      nseq = (io.in(ip) | io.in(ip + 1) << 8) + 0x7f00u;
      ip += 2;
      io.note(kEvSeqLong);
    } else {
      if (ip >= end) return kZsCorrupt;
      nseq = ((nseq - 128) << 8) + io.in(ip);
      ++ip;
      if (nseq == 128) io.note(kEvSeq128);
    }
  } else if (nseq == 127) {
    io.note(kEvSeq127);
  }
  if (ip >= end) return kZsCorrupt;
  const uint32_t modes = io.in(ip);
  ++ip;
  if (modes & 3u) return kZsCorrupt;
  int32_t st = zs_seq_table(io, t, modes >> 6, 0, &ip, end, t->ll, &fs->ll_log, &fs->have_ll);
  if (st == kZsOk) st = zs_seq_table(io, t, (modes >> 4) & 3u, 1, &ip, end, t->of, &fs->of_log, &fs->have_of);
  if (st == kZsOk) st = zs_seq_table(io, t, (modes >> 2) & 3u, 2, &ip, end, t->ml, &fs->ml_log, &fs->have_ml);
  if (st != kZsOk) return st;
  const ZsRdBack<Io> rd{&io};
  ZsBack b;
  if (!b.init(rd, ip, end)) return kZsCorrupt;
  uint32_t sl = b.take(rd, fs->ll_log), so = b.take(rd, fs->of_log), sm = b.take(rd, fs->ml_log);
  if (b.over) return kZsCorrupt;
  uint32_t lpos = 0;
  for (uint32_t k = 0; k < nseq; ++k) {
    const uint32_t el = TSG_ZS_UNIFORM(t->ll[sl]), eo = TSG_ZS_UNIFORM(t->of[so]), em = TSG_ZS_UNIFORM(t->ml[sm]);
    const uint32_t cl = el & 0xffu, co = eo & 0xffu, cm = em & 0xffu;
    if (cl > kZsLLMax || co > kZsOFMax || cm > kZsMLMax) return kZsCorrupt;
    const uint32_t ov = (1u << co) + b.take(rd, co);
    const uint32_t ml = ml_base[cm] + b.take(rd, ml_bits[cm]);
    const uint32_t ll = ll_base[cl] + b.take(rd, ll_bits[cl]);
    if (b.over) return kZsCorrupt;
    uint32_t off;
    if (ov > 3) {
      off = ov - 3;
      fs->rep[2] = fs->rep[1];
      fs->rep[1] = fs->rep[0];
      fs->rep[0] = off;
    } else {
      const uint32_t idx = ov - 1 + (ll == 0 ? 1u : 0u);     // 0..3; 3 = rep1 - 1
      io.note((ll == 0 ? kEvRep1LL0 : kEvRep1) + ov - 1);
      if (idx == 0) {
        off = fs->rep[0];
      } else {
        off = idx == 3 ? fs->rep[0] - 1 : fs->rep[idx];
        if (off == 0) return kZsCorrupt;
        if (idx != 1) fs->rep[2] = fs->rep[1];
        fs->rep[1] = fs->rep[0];
        fs->rep[0] = off;
      }
    }
    if (k + 1 < nseq) {
      sl = (el >> 16) + b.take(rd, (el >> 8) & 0xffu);
      sm = (em >> 16) + b.take(rd, (em >> 8) & 0xffu);
      so = (eo >> 16) + b.take(rd, (eo >> 8) & 0xffu);
      if (b.over) return kZsCorrupt;
    }
    if (ll > lit.size - lpos) return kZsCorrupt;
    if (ll > block_max - (op - bbegin)) return kZsCorrupt;       // more than Block_Maximum_Size from one block
    if (ll > cap - op) return kZsDstFull;
    zs_put_literals(io, lit, lpos, op, ll);
    lpos += ll;
    op += ll;
    if (off > op - fbegin) return kZsCorrupt;                    // before the frame's first output byte
    if (ml > block_max - (op - bbegin)) return kZsCorrupt;
    if (ml > cap - op) return kZsDstFull;
    io.seq_note(op, off, ml);
    io.copy(op, off, ml);
    op += ml;
  }
  if (!b.done()) return kZsCorrupt;
  const uint32_t rest = lit.size - lpos;
  if (rest > block_max - (op - bbegin)) return kZsCorrupt;
  if (rest > cap - op) return kZsDstFull;
  zs_put_literals(io, lit, lpos, op, rest);
  op += rest;
  return kZsOk;
}

// What a frame header says
struct ZsHeader {
  uint64_t window, fcs;
  bool has_fcs, has_sum, single;
  uint32_t fcs_bytes;
};
// A frame header behind its magic, from *ip on (n = the stream's length)
template <class In>
TSG_ZS_HD inline int32_t zs_frame_header(In in, uint64_t n, uint64_t* ip_io, ZsHeader* h) {
  uint64_t ip = *ip_io;
  if (ip >= n) return kZsEof;
  const uint32_t d = in(ip);
  ++ip;
  if (d & 8u) return kZsHeader;
  h->single = (d & 32u) != 0;
  h->has_sum = (d & 4u) != 0;
  const uint32_t fcs_flag = d >> 6, did_flag = d & 3u;
  h->window = 0;
  if (!h->single) {
    if (ip >= n) return kZsEof;
    const uint32_t w = in(ip);
    ++ip;
    const uint32_t log = 10 + (w >> 3);
    if (log > 31) return kZsHeader;
    h->window = (uint64_t(1) << log) + ((uint64_t(1) << log) >> 3) * (w & 7u);
  }
  const uint32_t did_bytes = did_flag == 3 ? 4u : did_flag;
  if (n - ip < did_bytes) return kZsEof;
  uint32_t did = 0;
  for (uint32_t k = 0; k < did_bytes; ++k) did |= in(ip + k) << (8 * k);
  ip += did_bytes;
  if (did) return kZsDict;
  h->fcs_bytes = fcs_flag == 0 ? (h->single ? 1u : 0u) : fcs_flag == 1 ? 2u : fcs_flag == 2 ? 4u : 8u;
  h->has_fcs = h->fcs_bytes != 0;
  h->fcs = 0;
  if (n - ip < h->fcs_bytes) return kZsEof;
  for (uint32_t k = 0; k < h->fcs_bytes; ++k) h->fcs |= static_cast<uint64_t>(in(ip + k)) << (8 * k);
  if (h->fcs_bytes == 2) h->fcs += 256;
  ip += h->fcs_bytes;
  if (h->single) h->window = h->fcs;
  *ip_io = ip;
  return kZsOk;
}

// The whole stream [0, n): every frame decoded into the slot [0, cap), its
// record stored (io.rec) while there is room for it: *nrecs counts all
// frames, those from rec_cap on have no record (zstd_frame_cap(n) never
// overflows).  Returns the first error in stream order, checksums apart;
// *out_len = the bytes written (all of them inside the slot) when it stopped.
template <class Io>
TSG_ZS_HD inline int32_t zstd_decode(Io& io, ZsTables* t, uint64_t n, uint64_t cap, uint32_t rec_cap, uint32_t* nrecs,
                                     uint32_t* nblocks, uint64_t* out_len) {
  uint64_t ip = 0, op = 0;
  uint32_t nf = 0, nb = 0;
  int32_t st = n ? kZsOk : kZsEof;
  auto in = [&io](uint64_t p) { return io.in(p); };
  while (st == kZsOk && ip < n) {
    if (n - ip < 4) { st = kZsEof; break; }
    const uint32_t magic = io.in(ip) | io.in(ip + 1) << 8 | io.in(ip + 2) << 16 | io.in(ip + 3) << 24;
    ip += 4;
    if ((magic & 0xfffffff0u) == kZsSkipMagic) {
      if (n - ip < 4) { st = kZsEof; break; }
      const uint64_t size = io.in(ip) | io.in(ip + 1) << 8 | io.in(ip + 2) << 16 | static_cast<uint64_t>(io.in(ip + 3)) << 24;
      ip += 4;
      if (n - ip < size) { st = kZsEof; break; }
      ip += size;
      io.note(kEvSkippable);
      continue;
    }
    if (magic != kZsMagic) { st = kZsHeader; break; }
    ZsHeader h;
    st = zs_frame_header(in, n, &ip, &h);
    if (st != kZsOk) break;
    io.note(kEvFrame);
    if (h.single) io.note(kEvSingleSegment);
    io.note(h.fcs_bytes == 0 ? kEvFcs0 : h.fcs_bytes == 1 ? kEvFcs1 : h.fcs_bytes == 2 ? kEvFcs2 : h.fcs_bytes == 4 ? kEvFcs4 : kEvFcs8);
    const uint64_t block_max = h.window < kZsBlockMax ? h.window : kZsBlockMax;
    const uint64_t fbegin = op;
    ZsFrameState fs;
    fs.rep[0] = 1;
    fs.rep[1] = 4;
    fs.rep[2] = 8;
    fs.ll_log = fs.ml_log = fs.of_log = fs.huf_log = 0;
    fs.have_ll = fs.have_ml = fs.have_of = fs.have_huf = false;
    for (bool last = false; !last;) {
      if (n - ip < 3) { st = kZsEof; break; }
      const uint32_t bh = io.in(ip) | io.in(ip + 1) << 8 | io.in(ip + 2) << 16;
      ip += 3;
      last = (bh & 1u) != 0;
      const uint32_t type = (bh >> 1) & 3u, size = bh >> 3;
      if (type == 3 || size > block_max) { st = kZsCorrupt; break; }
      ++nb;
      if (type == 0) {
        if (n - ip < size) { st = kZsEof; break; }
        if (size > cap - op) { st = kZsDstFull; break; }
        if (size) io.copy_in(op, ip, size);
        ip += size;
        op += size;
        io.note(kEvBlockRaw);
      } else if (type == 1) {
        if (ip >= n) { st = kZsEof; break; }
        if (size > cap - op) { st = kZsDstFull; break; }
        if (size) io.fill(op, io.in(ip), size);
        ++ip;
        op += size;
        io.note(kEvBlockRle);
      } else {
        if (n - ip < size) { st = kZsEof; break; }
        if (size < 3 || size >= kZsBlockMax) { st = kZsCorrupt; break; }
        const uint64_t bend = ip + size;
        ZsLit lit;
        lit.kind = 0;
        lit.size = 0;
        lit.pos = 0;
        lit.val = 0;
        uint64_t sp = 0;
        st = zs_literals(io, t, &fs, ip, bend, &lit, &sp);
        if (st != kZsOk) break;
        st = zs_sequences(io, t, &fs, sp, bend, lit, fbegin, block_max, cap, &op);
        if (st != kZsOk) break;
        ip = bend;
        io.note(kEvBlockCompressed);
      }
    }
    if (st != kZsOk) break;
    if (h.has_fcs && op - fbegin != h.fcs) { st = kZsCorrupt; break; }
    ZsFrameRec r;
    r.out_begin = fbegin;
    r.out_end = op;
    r.has_sum = h.has_sum ? 1u : 0u;
    r.sum = 0;
    if (h.has_sum) {
      if (n - ip < 4) { st = kZsEof; break; }
      r.sum = io.in(ip) | io.in(ip + 1) << 8 | io.in(ip + 2) << 16 | io.in(ip + 3) << 24;
      ip += 4;
      io.note(kEvChecksum);
    }
    if (op == fbegin) io.note(kEvEmptyFrame);
    if (nf < rec_cap) io.rec(nf, r);
    ++nf;
  }
  io.flush(op);
  *nrecs = nf;
  *nblocks = nb;
  *out_len = op;
  return st;
}

// The decoder's status and the frames' checksums -> the stream's status:
// sums[k] = the low 32 bits of XXH64 over record k's range (unused where the
// record has no checksum).  A frame that fails its checksum precedes whatever
// ended the decode behind it.
inline int32_t zs_check_frames(int32_t st, const ZsFrameRec* recs, uint32_t nrecs, const uint32_t* sums) {
  for (uint32_t k = 0; k < nrecs; ++k)
    if (recs[k].has_sum && recs[k].sum != sums[k]) return kZsChecksum;
  return st;
}

// ---- the CPU model ----
constexpr uint32_t kZsNear = 28672;                // zstdec.hip's ring serves a source this near; older bytes come from HBM
template <class Get>
struct ZsHostIo {
  Get get;
  uint8_t* dst;
  uint8_t* lits;                                   // kZsBlockMax bytes
  ZsFrameRec* recs;
  uint64_t* ev;                                    // kEvCount counters, or null
  uint64_t far_line = ~uint64_t(0);
  bool leader() const { return true; }
  void sync() {}
  uint32_t in(uint64_t pos) { return get(pos); }
  uint32_t in_back(uint64_t pos) { return get(pos); }
  uint32_t in_lane(uint64_t pos) { return get(pos); }
  uint32_t in_back32(uint64_t pos) { return get(pos) | get(pos + 1) << 8 | get(pos + 2) << 16 | get(pos + 3) << 24; }
  uint32_t in_lane32(uint64_t pos) { return in_back32(pos); }
  void lit_put(uint32_t k, uint32_t b) { lits[k] = static_cast<uint8_t>(b); }
  template <class F>
  bool huf_run(uint32_t n, F f) {
    bool ok = true;
    for (uint32_t k = 0; k < n; ++k) ok = f(k) && ok;
    return ok;
  }
  void copy_in(uint64_t op, uint64_t pos, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) dst[op + i] = static_cast<uint8_t>(get(pos + i));
  }
  void copy_lit(uint64_t op, uint32_t k, uint32_t len) { std::memcpy(dst + op, lits + k, len); }
  void fill(uint64_t op, uint32_t b, uint32_t len) { std::memset(dst + op, static_cast<int>(b), len); }
  void copy(uint64_t op, uint32_t off, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) dst[op + i] = dst[op + i - off];
  }
  void rec(uint32_t k, const ZsFrameRec& r) { recs[k] = r; }
  void flush(uint64_t) {}
  void note(uint32_t e) {
    if (ev) ++ev[e];
  }
  void seq_note(uint64_t op, uint32_t off, uint32_t len) {
    if (!ev) return;
    if (off == 32768) ++ev[kEvOff32768];
    if (off == 32769) ++ev[kEvOff32769];
    if (off == kZsNear) ++ev[kEvOffRingEdge];      // the last distance zstdec.hip's ring serves, and the first it does not
    if (off == kZsNear + 1) ++ev[kEvOffRingEdge1];
    if (off > kZsNear) {
      ++ev[kEvOffFar];
      // the source starts in the 128-byte line in which an earlier far match's source ended
      if ((op - off) / 128 == far_line) ++ev[kEvFarSameLine];
      far_line = (op - off + std::min(len, off) - 1) / 128;
      if (len <= off && off < kZsNear + len) ++ev[kEvStraddle];   // starts in HBM, ends in the ring
    }
    if (off == 1 && len >= 65539) ++ev[kEvLongOverlap];
  }
};

struct ZsModelStats {
  uint64_t frames = 0, blocks = 0;
};

// One stream of n bytes (byte i = get(i), i < n) into dst[0, cap): the status
// tsg_inflate_zstd_device gives it, *out_len as the device leaves it.
template <class Get>
inline int32_t zstd_model(Get get, uint64_t n, uint8_t* dst, uint64_t cap, uint64_t* out_len, uint64_t* ev = nullptr,
                          ZsModelStats* stats = nullptr) {
  std::vector<ZsFrameRec> recs(zstd_frame_cap(n));
  std::vector<ZsTables> t(1);
  std::vector<uint8_t> lits(kZsBlockMax);
  ZsHostIo<Get> io{get, dst, lits.data(), recs.data(), ev};
  uint32_t nrecs = 0, nblocks = 0;
  int32_t st = zstd_decode(io, t.data(), n, cap, static_cast<uint32_t>(recs.size()), &nrecs, &nblocks, out_len);
  std::vector<uint32_t> sums(nrecs, 0);
  for (uint32_t k = 0; k < nrecs; ++k)
    if (recs[k].has_sum)
      sums[k] = static_cast<uint32_t>(zs_xxh64(ZsByteLd{dst + recs[k].out_begin}, recs[k].out_end - recs[k].out_begin));
  st = zs_check_frames(st, recs.data(), nrecs, sums.data());
  if (stats) {
    stats->frames = nrecs;
    stats->blocks = nblocks;
  }
  return st;
}

// An upper bound of a stream's decoded size from its frame and block headers
// alone: a frame with a Frame_Content_Size counts it (but no more than its
// blocks allow), another counts a raw or RLE block's size and
// Block_Maximum_Size per compressed block.  *exact = every frame states its
// size.  false: the walk met a malformed or truncated header; *bound then
// covers what precedes it.
inline bool zstd_size_bound(const uint8_t* z, size_t len, uint64_t* bound, int* exact) {
  uint64_t ip = 0, total = 0;
  bool all_fcs = true, clean = true;
  auto in = [z](uint64_t p) { return static_cast<uint32_t>(z[p]); };
  while (ip < len) {
    if (len - ip < 4) { clean = false; break; }
    const uint32_t magic = in(ip) | in(ip + 1) << 8 | in(ip + 2) << 16 | in(ip + 3) << 24;
    ip += 4;
    if ((magic & 0xfffffff0u) == kZsSkipMagic) {
      if (len - ip < 4) { clean = false; break; }
      const uint64_t size = in(ip) | in(ip + 1) << 8 | in(ip + 2) << 16 | static_cast<uint64_t>(in(ip + 3)) << 24;
      ip += 4;
      if (len - ip < size) { clean = false; break; }
      ip += size;
      continue;
    }
    ZsHeader h;
    if (magic != kZsMagic || zs_frame_header(in, len, &ip, &h) != kZsOk) { clean = false; break; }
    const uint64_t block_max = h.window < kZsBlockMax ? h.window : kZsBlockMax;
    uint64_t walk = 0;
    for (bool last = false; !last;) {
      if (len - ip < 3) { clean = false; break; }
      const uint32_t bh = in(ip) | in(ip + 1) << 8 | in(ip + 2) << 16;
      ip += 3;
      last = (bh & 1u) != 0;
      const uint32_t type = (bh >> 1) & 3u, size = bh >> 3;
      if (type == 3) { clean = false; break; }
      const uint64_t take = type == 1 ? 1 : size;
      if (len - ip < take) { clean = false; break; }
      ip += take;
      walk += type == 2 ? block_max : size;
    }
    if (h.has_fcs) total += std::min(h.fcs, walk);
    else { total += walk; all_fcs = false; }
    if (!clean) break;
    if (h.has_sum) {
      if (len - ip < 4) { clean = false; break; }
      ip += 4;
    }
  }
  *bound = total;
  *exact = clean && all_fcs ? 1 : 0;
  return clean;
}

enum : int { kLayerNone = 0, kLayerGzip = 1, kLayerZstd = 2 };
// go-containerregistry's peek: gzip by 1f 8b, zstd by 28 b5 2f fd
inline int layer_compression(const uint8_t* blob, size_t len) {
  if (len >= 2 && blob[0] == 0x1f && blob[1] == 0x8b) return kLayerGzip;
  if (len >= 4 && blob[0] == 0x28 && blob[1] == 0xb5 && blob[2] == 0x2f && blob[3] == 0xfd) return kLayerZstd;
  return kLayerNone;
}

}  // namespace tsg
