// Inflating gzip layer blobs (inflate.hip): RFC 1952 members over RFC 1951
// DEFLATE, stated once for the host and the device, and the sequential CPU
// model of the device pass.  No HIP here.
//
// The reference opens a layer with layer.Uncompressed()
// (pkg/fanal/artifact/image/image.go:464-492), i.e. Go's compress/gzip over
// compress/flate; the rules and the error texts below are theirs:
//   member header  1f 8b, CM = 8, reserved FLG bits (0xE0) zero; FEXTRA, FNAME,
//                  FCOMMENT skipped (a name / comment whose NUL is not among
//                  its first 512 bytes is a header error, gunzip.go readString);
//                  FHCRC's 16 bits = the low half of the header's CRC32
//   blocks         stored (LEN == ~NLEN), fixed, dynamic (HLIT <= 286,
//                  HDIST <= 30, repeat 16 needs a previous length, no repeat
//                  past HLIT + HDIST); literal/length symbols 286 / 287 and
//                  distance symbols 30 / 31 are corrupt, as is a distance
//                  reaching before the member's first output byte
//   code tables    huffmanDecoder.init: the code is complete (Kraft sum 1), or
//                  it is the single code of length 1, or it has no code at all
//                  (accepted; decoding a symbol from it is corrupt)
//   trailer        CRC32 and ISIZE (mod 2^32)
//   multistream    after a member, no bytes left is the end; anything else is
//                  the next header (fewer than 10 bytes: unexpected EOF)
// inflate_decode is the decoder both sides run: its input, output, table
// stores and the copy of a match go through an Io policy (HostIo below;
// WaveIo in inflate.hip), so the bounds logic the wavefront executes is the
// logic the sanitizers see on the host.  The decoder checks no CRC: it records
// every member's output range with the trailer's CRC32 and ISIZE, the CRC32 of
// the output is taken in slices (crc32_slices; tsg_crc32_slices on the
// device) and inf_check_members folds the slices per member with the GF(2)
// shift operator and compares.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define TSG_INF_HD __host__ __device__
#else
#define TSG_INF_HD
#endif
// A value every lane of the wavefront holds alike, moved to a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
#define TSG_INF_UNIFORM(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#else
#define TSG_INF_UNIFORM(x) static_cast<uint32_t>(x)
#endif

namespace tsg {

// per-stream status (TSG_INFLATE_* of trivy_secret.h)
enum : int32_t { kInfOk = 0, kInfHeader = 1, kInfCorrupt = 2, kInfEof = 3, kInfChecksum = 4, kInfDstFull = 5 };

inline const char* inflate_status_text(int32_t st) {
  switch (st) {
    case kInfHeader: return "gzip: invalid header";           // gzip.ErrHeader
    case kInfCorrupt: return "flate: corrupt input";          // flate.CorruptInputError, without its offset
    case kInfEof: return "unexpected EOF";                    // io.ErrUnexpectedEOF
    case kInfChecksum: return "gzip: invalid checksum";       // gzip.ErrChecksum
    default: return "";                                       // kInfOk; kInfDstFull is no error of the stream's
  }
}

constexpr uint32_t kInfWindow = 32768;           // DEFLATE's largest distance
constexpr uint32_t kInfPrimaryBits = 10;
constexpr uint32_t kInfLong = 0xffffu;           // primary entry of a code longer than kInfPrimaryBits
constexpr uint32_t kInfMinMember = 20;           // header 10 + empty fixed block 2 + trailer 8
constexpr uint32_t kCrcSlice = 4096;             // bytes per CRC slice, counted from a member's first output byte
constexpr uint32_t kCrcPoly = 0xedb88320u;

// One decode table: primary[low kInfPrimaryBits bits of the stream] =
// symbol << 4 | code length for the codes that fit, kInfLong for the prefix of
// longer ones, 0 where no code starts; count / sym (symbols in canonical
// order) decode a long code bit by bit (the overflow).
struct InfTable {
  uint16_t primary[1u << kInfPrimaryBits];
  uint16_t sym[288];
  uint16_t count[16];
  uint16_t offs[16];
  uint32_t ok;
};
struct InfTables {
  InfTable lit, dist;                            // dist also serves the code-length code of a dynamic header
  uint8_t lens[320];
};
// A member's output range inside its stream's slot and its trailer
struct InfMember {
  uint64_t out_begin, out_end;
  uint32_t crc32, isize;
};
inline uint32_t inflate_member_cap(uint64_t gz_len) { return static_cast<uint32_t>(gz_len / kInfMinMember + 1); }

// huffmanDecoder.init (inflate.go) for lens[0, n), run by one lane.
TSG_INF_HD inline bool inf_build_serial(const uint8_t* lens, uint32_t n, InfTable* t) {
  constexpr uint32_t P = 1u << kInfPrimaryBits;
  for (uint32_t i = 0; i < P; ++i) t->primary[i] = 0;
  for (uint32_t l = 0; l < 16; ++l) t->count[l] = 0;
  uint32_t total = 0;
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15u;
    if (l) { ++t->count[l]; ++total; }
  }
  if (total == 0) return true;                   // no code: fails when a symbol is decoded
  int32_t left = 1;
  for (uint32_t l = 1; l < 16; ++l) {
    left = left * 2 - static_cast<int32_t>(t->count[l]);
    if (left < 0) return false;                  // oversubscribed
  }
  if (left > 0 && !(total == 1 && t->count[1] == 1)) return false;   // incomplete
  uint32_t o = 0;
  for (uint32_t l = 1; l < 16; ++l) { t->offs[l] = static_cast<uint16_t>(o); o += t->count[l]; }
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15u;
    if (l) t->sym[t->offs[l]++] = static_cast<uint16_t>(s);
  }
  uint32_t code = 0;
  t->offs[0] = 0;
  for (uint32_t l = 1; l < 16; ++l) {            // offs[l] = the first code of length l
    code = (code + (l > 1 ? t->count[l - 1] : 0u)) << 1;
    t->offs[l] = static_cast<uint16_t>(code);
  }
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15u;
    if (!l) continue;
    const uint32_t c = t->offs[l]++;
    uint32_t rev = 0;
    for (uint32_t k = 0; k < l; ++k) rev |= ((c >> k) & 1u) << (l - 1 - k);
    if (l <= kInfPrimaryBits) {
      for (uint32_t j = rev; j < P; j += 1u << l) t->primary[j] = static_cast<uint16_t>(s << 4 | l);
    } else {
      t->primary[rev & (P - 1)] = kInfLong;
    }
  }
  return true;
}

template <class Io>
TSG_INF_HD inline bool inf_build(Io& io, const uint8_t* lens, uint32_t n, InfTable* t) {
  io.sync();                                     // the lengths the other lanes' leader wrote
  if (io.leader()) t->ok = inf_build_serial(lens, n, t) ? 1u : 0u;
  io.sync();
  return TSG_INF_UNIFORM(t->ok) != 0;
}

// The bit reader: bb holds nb bits, the next unread stream byte is ip.
struct InfBits {
  uint64_t bb = 0;
  uint32_t nb = 0;
  uint64_t ip = 0, n = 0;
  template <class Io>
  TSG_INF_HD void fill(Io& io) {
    while (nb <= 56 && ip < n) {
      bb |= static_cast<uint64_t>(io.in(ip)) << nb;
      ++ip;
      nb += 8;
    }
  }
  TSG_INF_HD void drop(uint32_t k) { bb >>= k; nb -= k; }
  // k <= 16 bits; false at the end of the stream
  template <class Io>
  TSG_INF_HD bool take(Io& io, uint32_t k, uint32_t* v) {
    if (nb < k) fill(io);
    if (nb < k) return false;
    *v = static_cast<uint32_t>(bb) & ((1u << k) - 1u);
    drop(k);
    return true;
  }
  // to the next byte boundary, the whole bytes still in bb handed back
  TSG_INF_HD void align() {
    ip -= nb >> 3;
    bb = 0;
    nb = 0;
  }
};

// One symbol of table t: kInfOk, kInfCorrupt (no code matches) or kInfEof (the
// code that matches the zero-padded rest is longer than what is left).
template <class Io>
TSG_INF_HD inline int32_t inf_sym(Io& io, InfBits& b, const InfTable& t, uint32_t* sym) {
  if (b.nb < 15) b.fill(io);
  const uint32_t v = static_cast<uint32_t>(b.bb);
  const uint32_t e = TSG_INF_UNIFORM(t.primary[v & ((1u << kInfPrimaryBits) - 1u)]);
  uint32_t len = e & 15u, s = e >> 4;
  if (e == kInfLong) {
    uint32_t code = 0, first = 0, index = 0;
    len = 0;
    for (uint32_t l = 1; l < 16; ++l) {
      code |= (v >> (l - 1)) & 1u;
      const uint32_t cnt = TSG_INF_UNIFORM(t.count[l]);
      if (code < first + cnt) {
        const uint32_t at = index + (code - first);
        s = TSG_INF_UNIFORM(t.sym[at < 288u ? at : 287u]);
        len = l;
        break;
      }
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
  }
  if (len == 0) return kInfCorrupt;
  if (len > b.nb) return kInfEof;
  b.drop(len);
  *sym = s;
  return kInfOk;
}

TSG_INF_HD inline uint32_t inf_crc_byte(uint32_t crc, uint32_t c) {
  crc ^= c;
  for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (kCrcPoly & (0u - (crc & 1u)));
  return crc;
}

// RFC 1951 3.2.5
TSG_INF_HD inline uint32_t inf_len_base(uint32_t s) {      // s = symbol - 257, 0..28
  return s < 8 ? s + 3 : s == 28 ? 258u : ((4u + (s & 3u)) << ((s >> 2) - 1)) + 3u;
}
TSG_INF_HD inline uint32_t inf_len_extra(uint32_t s) { return s < 8 || s == 28 ? 0u : (s >> 2) - 1; }
TSG_INF_HD inline uint32_t inf_dist_base(uint32_t s) {     // s = 0..29
  return s < 4 ? s + 1 : ((2u + (s & 1u)) << ((s >> 1) - 1)) + 1u;
}
TSG_INF_HD inline uint32_t inf_dist_extra(uint32_t s) { return s < 4 ? 0u : (s >> 1) - 1; }

// A dynamic block's header (flate readHuffman) into t->lit / t->dist
template <class Io>
TSG_INF_HD inline int32_t inf_dynamic_header(Io& io, InfBits& b, InfTables* t) {
  uint32_t v = 0;
  if (!b.take(io, 14, &v)) return kInfEof;
  const uint32_t nlit = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, nclen = ((v >> 10) & 15u) + 4u;
  if (nlit > 286u || ndist > 30u) return kInfCorrupt;
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};   // codeOrder
  io.sync();
  if (io.leader())
    for (uint32_t i = 0; i < 19; ++i) t->lens[i] = 0;
  for (uint32_t i = 0; i < nclen; ++i) {
    if (!b.take(io, 3, &v)) return kInfEof;
    if (io.leader()) t->lens[order[i]] = static_cast<uint8_t>(v);
  }
  if (!inf_build(io, t->lens, 19, &t->dist)) return kInfCorrupt;
  const uint32_t n = nlit + ndist;
  uint32_t prev = 0;
  for (uint32_t i = 0; i < n;) {
    uint32_t x = 0;
    const int32_t st = inf_sym(io, b, t->dist, &x);
    if (st != kInfOk) return st;
    if (x < 16) {
      if (io.leader()) t->lens[i] = static_cast<uint8_t>(x);
      prev = x;
      ++i;
      continue;
    }
    uint32_t rep, nb, fillv = 0;
    if (x == 16) {
      if (i == 0) return kInfCorrupt;
      rep = 3; nb = 2; fillv = prev;
    } else if (x == 17) {
      rep = 3; nb = 3;
    } else {
      rep = 11; nb = 7;
    }
    if (!b.take(io, nb, &v)) return kInfEof;
    rep += v;
    if (i + rep > n) return kInfCorrupt;
    if (io.leader())
      for (uint32_t k = 0; k < rep; ++k) t->lens[i + k] = static_cast<uint8_t>(fillv);
    prev = fillv;
    i += rep;
  }
  // the distance lengths first: building the literal table needs only lens[0, nlit)
  if (!inf_build(io, t->lens + nlit, ndist, &t->dist)) return kInfCorrupt;
  if (!inf_build(io, t->lens, nlit, &t->lit)) return kInfCorrupt;
  return kInfOk;
}

template <class Io>
TSG_INF_HD inline void inf_fixed_tables(Io& io, InfTables* t) {
  io.sync();
  if (io.leader()) {
    for (uint32_t s = 0; s < 288; ++s) t->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    for (uint32_t s = 288; s < 320; ++s) t->lens[s] = 5;
  }
  inf_build(io, t->lens, 288, &t->lit);
  inf_build(io, t->lens + 288, 32, &t->dist);
}

// The blocks of one member from b on; *op advances (never past cap).
template <class Io>
TSG_INF_HD inline int32_t inf_blocks(Io& io, InfBits& b, InfTables* t, uint64_t mbegin, uint64_t cap, uint64_t* op_io) {
  uint64_t op = *op_io;
  int32_t st = kInfOk;
  for (bool last = false; !last && st == kInfOk;) {
    uint32_t v = 0;
    if (!b.take(io, 3, &v)) { st = kInfEof; break; }
    last = (v & 1u) != 0;
    const uint32_t type = v >> 1;
    if (type == 3) { st = kInfCorrupt; break; }
    if (type == 0) {
      b.align();
      if (b.n - b.ip < 4) { st = kInfEof; break; }
      const uint32_t len = io.in(b.ip) | io.in(b.ip + 1) << 8, nlen = io.in(b.ip + 2) | io.in(b.ip + 3) << 8;
      b.ip += 4;
      if (len != (nlen ^ 0xffffu)) { st = kInfCorrupt; break; }
      for (uint32_t k = 0; k < len; ++k) {
        if (b.ip >= b.n) { st = kInfEof; break; }
        if (op >= cap) { st = kInfDstFull; break; }
        io.lit(op, io.in(b.ip));
        ++b.ip;
        ++op;
      }
      continue;
    }
    if (type == 1) {
      inf_fixed_tables(io, t);
    } else {
      st = inf_dynamic_header(io, b, t);
      if (st != kInfOk) break;
    }
    for (;;) {                                   // every turn consumes at least one bit or ends the block
      uint32_t s = 0;
      st = inf_sym(io, b, t->lit, &s);
      if (st != kInfOk) break;
      if (s < 256) {
        if (op >= cap) { st = kInfDstFull; break; }
        io.lit(op, s);
        ++op;
        continue;
      }
      if (s == 256) break;
      if (s >= 286) { st = kInfCorrupt; break; }
      s -= 257;
      uint32_t len = inf_len_base(s), x = 0;
      if (inf_len_extra(s)) {
        if (!b.take(io, inf_len_extra(s), &x)) { st = kInfEof; break; }
        len += x;
      }
      uint32_t d = 0;
      st = inf_sym(io, b, t->dist, &d);
      if (st != kInfOk) break;
      if (d >= 30) { st = kInfCorrupt; break; }
      uint32_t dist = inf_dist_base(d);
      if (inf_dist_extra(d)) {
        if (!b.take(io, inf_dist_extra(d), &x)) { st = kInfEof; break; }
        dist += x;
      }
      if (dist > op - mbegin) { st = kInfCorrupt; break; }      // before the member's first output byte
      if (len > cap - op) { st = kInfDstFull; break; }
      io.copy(op, dist, len);
      op += len;
    }
  }
  *op_io = op;
  return st;
}

// A member's header from *ip on (gunzip.go readHeader); kInfOk leaves *ip at the first block
template <class Io>
TSG_INF_HD inline int32_t inf_member_header(Io& io, uint64_t n, uint64_t* ip_io) {
  uint64_t ip = *ip_io;
  if (n - ip < 10) return kInfEof;
  const uint32_t flg = io.in(ip + 3);
  if (io.in(ip) != 0x1fu || io.in(ip + 1) != 0x8bu || io.in(ip + 2) != 8u || (flg & 0xe0u)) return kInfHeader;
  const bool want_crc = (flg & 2u) != 0;
  uint32_t crc = 0xffffffffu;
  if (want_crc)
    for (uint32_t k = 0; k < 10; ++k) crc = inf_crc_byte(crc, io.in(ip + k));
  ip += 10;
  if (flg & 4u) {                                // FEXTRA
    if (n - ip < 2) return kInfEof;
    const uint32_t xlen = io.in(ip) | io.in(ip + 1) << 8;
    if (n - ip - 2 < xlen) return kInfEof;
    if (want_crc)
      for (uint32_t k = 0; k < xlen + 2; ++k) crc = inf_crc_byte(crc, io.in(ip + k));
    ip += 2 + xlen;
  }
  for (uint32_t f = 8u; f <= 16u; f <<= 1) {     // FNAME, FCOMMENT
    if (!(flg & f)) continue;
    for (uint32_t i = 0;; ++i) {
      if (i >= 512) return kInfHeader;
      if (ip >= n) return kInfEof;
      const uint32_t c = io.in(ip);
      ++ip;
      if (want_crc) crc = inf_crc_byte(crc, c);
      if (c == 0) break;
    }
  }
  if (want_crc) {
    if (n - ip < 2) return kInfEof;
    const uint32_t got = io.in(ip) | io.in(ip + 1) << 8;
    ip += 2;
    if (got != (~crc & 0xffffu)) return kInfHeader;
  }
  *ip_io = ip;
  return kInfOk;
}

// The whole stream [0, n): every member decoded into the slot [0, cap), its
// record stored (io.rec; at most rec_cap of them, inflate_member_cap(n) never
// overflows).  Returns the first error in stream order, checksums apart;
// *out_len = the bytes written (all of them inside the slot) when it stopped.
template <class Io>
TSG_INF_HD inline int32_t inflate_decode(Io& io, InfTables* t, uint64_t n, uint64_t cap, uint32_t rec_cap,
                                         uint32_t* nrecs, uint64_t* out_len) {
  InfBits b;
  b.n = n;
  uint64_t op = 0;
  uint32_t nm = 0;
  int32_t st = n ? kInfOk : kInfEof;
  while (st == kInfOk && b.ip < n) {
    st = inf_member_header(io, n, &b.ip);
    if (st != kInfOk) break;
    const uint64_t mbegin = op;
    st = inf_blocks(io, b, t, mbegin, cap, &op);
    if (st != kInfOk) break;
    b.align();
    if (n - b.ip < 8) { st = kInfEof; break; }
    InfMember m;
    m.out_begin = mbegin;
    m.out_end = op;
    m.crc32 = io.in(b.ip) | io.in(b.ip + 1) << 8 | io.in(b.ip + 2) << 16 | io.in(b.ip + 3) << 24;
    m.isize = io.in(b.ip + 4) | io.in(b.ip + 5) << 8 | io.in(b.ip + 6) << 16 | io.in(b.ip + 7) << 24;
    b.ip += 8;
    if (nm < rec_cap) io.rec(nm, m);
    ++nm;
  }
  io.flush(op);
  *nrecs = nm < rec_cap ? nm : rec_cap;
  *out_len = op;
  return st;
}

// ---- CRC32 in slices ----
struct Crc32Table {
  uint32_t t[256];
  Crc32Table() {
    for (uint32_t i = 0; i < 256; ++i) t[i] = inf_crc_byte(0, i);
  }
};
inline uint32_t crc32_bytes(const uint8_t* p, uint64_t n) {
  static const Crc32Table tab;
  uint32_t c = 0xffffffffu;
  for (uint64_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return ~c;
}
inline uint64_t crc32_nslices(uint64_t len) { return (len + kCrcSlice - 1) / kCrcSlice; }
// out[k] = CRC32 of data[k * kCrcSlice, min(len, (k + 1) * kCrcSlice)), each on its own
inline void crc32_slices(const uint8_t* data, uint64_t len, uint32_t* out) {
  for (uint64_t k = 0; k * kCrcSlice < len; ++k)
    out[k] = crc32_bytes(data + k * kCrcSlice, std::min<uint64_t>(kCrcSlice, len - k * kCrcSlice));
}
// a(x) b(x) mod p(x), bit-reflected (zlib's multmodp)
inline uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 nbytes) mod p(x): the operator that shifts a CRC over nbytes more bytes
inline uint32_t crc32_shift_op(uint64_t nbytes) {
  uint32_t sq = crc32_mulmod(1u << 30, 1u << 30), op = 1u << 31;   // x^2; sq runs x^8, x^16, ...
  sq = crc32_mulmod(sq, sq);
  sq = crc32_mulmod(sq, sq);
  for (; nbytes; nbytes >>= 1) {
    if (nbytes & 1u) op = crc32_mulmod(sq, op);
    sq = crc32_mulmod(sq, sq);
  }
  return op;
}
// CRC32 of len bytes from the CRCs of their slices: crc <- shift(crc) ^ next
inline uint32_t crc32_combine(const uint32_t* slices, uint64_t len) {
  static const uint32_t whole = crc32_shift_op(kCrcSlice);
  const uint64_t ns = crc32_nslices(len);
  uint32_t c = 0;
  for (uint64_t k = 0; k < ns; ++k) {
    const uint64_t l = std::min<uint64_t>(kCrcSlice, len - k * kCrcSlice);
    c = crc32_mulmod(l == kCrcSlice ? whole : crc32_shift_op(l), c) ^ slices[k];
  }
  return c;
}

// The decoder's status and the members' checksums -> the stream's status:
// slices = the members' slice CRCs one member after the other.  A member that
// fails its trailer precedes whatever ended the decode behind it.
inline int32_t inf_check_members(int32_t st, const InfMember* recs, uint32_t nrecs, const uint32_t* slices) {
  for (uint32_t k = 0; k < nrecs; ++k) {
    const uint64_t len = recs[k].out_end - recs[k].out_begin;
    if (crc32_combine(slices, len) != recs[k].crc32 || static_cast<uint32_t>(len) != recs[k].isize) return kInfChecksum;
    slices += crc32_nslices(len);
  }
  return st;
}

// ---- the CPU model ----
template <class Get>
struct HostIo {
  Get get;
  uint8_t* dst;
  InfMember* recs;
  bool leader() const { return true; }
  void sync() {}
  uint32_t in(uint64_t pos) { return get(pos); }
  void lit(uint64_t op, uint32_t b) { dst[op] = static_cast<uint8_t>(b); }
  void copy(uint64_t op, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) dst[op + i] = dst[op - dist + i % dist];
  }
  void rec(uint32_t k, const InfMember& m) { recs[k] = m; }
  void flush(uint64_t) {}
};

// One stream of n bytes (byte i = get(i), i < n) into dst[0, cap): the status
// tsg_inflate_gzip_device gives it, *out_len as the device leaves it.
template <class Get>
inline int32_t inflate_model(Get get, uint64_t n, uint8_t* dst, uint64_t cap, uint64_t* out_len,
                             std::vector<InfMember>* members = nullptr) {
  std::vector<InfMember> recs(inflate_member_cap(n));
  std::vector<InfTables> t(1);
  HostIo<Get> io{get, dst, recs.data()};
  uint32_t nrecs = 0;
  int32_t st = inflate_decode(io, t.data(), n, cap, static_cast<uint32_t>(recs.size()), &nrecs, out_len);
  recs.resize(nrecs);
  std::vector<uint32_t> slices;
  for (const InfMember& m : recs) {
    const size_t at = slices.size();
    slices.resize(at + crc32_nslices(m.out_end - m.out_begin));
    crc32_slices(dst + m.out_begin, m.out_end - m.out_begin, slices.data() + at);
  }
  st = inf_check_members(st, recs.data(), nrecs, slices.data());
  if (members) *members = recs;
  return st;
}

// ISIZE of the last member: a hint for the slot's size, no more
inline bool gzip_size_hint(const uint8_t* gz, size_t len, uint64_t* isize) {
  if (len < 18 || gz[0] != 0x1f || gz[1] != 0x8b) return false;
  const uint8_t* p = gz + len - 4;
  *isize = p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
  return true;
}

}  // namespace tsg
