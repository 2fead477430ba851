// Host side of the wire packing (wirepack.h).  The 7-bit codec: a scalar 64-bit
// SWAR path and an AVX2 path, chosen at run time, and the reference unpack.  The
// 6-bit codec with escapes: scalar, AVX2 and AVX-512 VBMI paths and its unpack;
// its split blocks: scalar, AVX2 (lookup only) and AVX-512 VBMI2 paths.
#include "wirepack.h"

#include <algorithm>
#include <cstring>
#include <memory>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace tsg {

namespace {

constexpr uint64_t kHigh = 0x8080808080808080ull;

// 8 bytes < 0x80 (little-endian in x) -> their 56 bits
inline uint64_t squeeze(uint64_t x) {
  x = (x & 0x007F007F007F007Full) | ((x & 0x7F007F007F007F00ull) >> 1);
  x = (x & 0x00003FFF00003FFFull) | ((x & 0x3FFF00003FFF0000ull) >> 2);
  return (x & 0x000000000FFFFFFFull) | ((x & 0x0FFFFFFF00000000ull) >> 4);
}

inline uint64_t spread(uint64_t v) {
  uint64_t x = (v & 0x000000000FFFFFFFull) | ((v << 4) & 0x0FFFFFFF00000000ull);
  x = (x & 0x00003FFF00003FFFull) | ((x << 2) & 0x3FFF00003FFF0000ull);
  return (x & 0x007F007F007F007Full) | ((x << 1) & 0x7F007F007F007F00ull);
}

// Packs the groups [g0, whole groups of n) and the trailing partial group of
// one block; returns the OR of the bytes seen.  Each whole group is written as
// 8 bytes (the top one zero, overwritten by the next group or left in the
// destination's slack).
inline uint64_t pack_groups_scalar(const uint8_t* src, size_t n, size_t g0, uint8_t* dst) {
  uint64_t acc = 0;
  const size_t ng = n / 8;
  for (size_t g = g0; g < ng; ++g) {
    uint64_t x;
    std::memcpy(&x, src + 8 * g, 8);
    acc |= x;
    x = squeeze(x & ~kHigh);
    std::memcpy(dst + 7 * g, &x, 8);
  }
  if (n % 8) {
    uint64_t x = 0;
    std::memcpy(&x, src + 8 * ng, n % 8);
    acc |= x;
    x = squeeze(x & ~kHigh);
    std::memcpy(dst + 7 * ng, &x, 8);
  }
  return acc;
}

uint64_t pack_block_scalar(const uint8_t* src, size_t n, uint8_t* dst) { return pack_groups_scalar(src, n, 0, dst); }

#if defined(__x86_64__)
__attribute__((target("avx2"))) uint64_t pack_block_avx2(const uint8_t* src, size_t n, uint8_t* dst) {
  const __m256i m1 = _mm256_set1_epi64x(0x007F007F007F007Fll), m1h = _mm256_set1_epi64x(0x7F007F007F007F00ll);
  const __m256i m2 = _mm256_set1_epi64x(0x00003FFF00003FFFll), m2h = _mm256_set1_epi64x(0x3FFF00003FFF0000ll);
  const __m256i m3 = _mm256_set1_epi64x(0x000000000FFFFFFFll), m3h = _mm256_set1_epi64x(0x0FFFFFFF00000000ll);
  // the 7 low bytes of both quadwords of a 128-bit lane, side by side
  const __m256i shuf = _mm256_setr_epi8(0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, -1, -1,
                                        0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, -1, -1);
  __m256i acc = _mm256_setzero_si256();
  const size_t nv = n / 32;
  for (size_t i = 0; i < nv; ++i) {
    __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + 32 * i));
    acc = _mm256_or_si256(acc, x);
    x = _mm256_or_si256(_mm256_and_si256(x, m1), _mm256_srli_epi64(_mm256_and_si256(x, m1h), 1));
    x = _mm256_or_si256(_mm256_and_si256(x, m2), _mm256_srli_epi64(_mm256_and_si256(x, m2h), 2));
    x = _mm256_or_si256(_mm256_and_si256(x, m3), _mm256_srli_epi64(_mm256_and_si256(x, m3h), 4));
    x = _mm256_shuffle_epi8(x, shuf);
    // (two 16-byte stores of 14 packed bytes each: the second's two zero
    // bytes are overwritten by the next store or lie in the slack)
    _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + 28 * i), _mm256_castsi256_si128(x));
    _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + 28 * i + 14), _mm256_extracti128_si256(x, 1));
  }
  const __m128i a = _mm_or_si128(_mm256_castsi256_si128(acc), _mm256_extracti128_si256(acc, 1));
  uint64_t r = static_cast<uint64_t>(_mm_cvtsi128_si64(a)) | static_cast<uint64_t>(_mm_extract_epi64(a, 1));
  return r | pack_groups_scalar(src, n, nv * 4, dst);
}
#endif

}  // namespace

bool wire_have_avx2() {
#if defined(__x86_64__)
  static const bool have = __builtin_cpu_supports("avx2");
  return have;
#else
  return false;
#endif
}

size_t wire_pack(const uint8_t* src, size_t n, uint8_t* dst, uint32_t* table, int path) {
  uint64_t (*pack_block)(const uint8_t*, size_t, uint8_t*) = pack_block_scalar;
#if defined(__x86_64__)
  if (path != kWireScalar && wire_have_avx2()) pack_block = pack_block_avx2;
#endif
  size_t o = 0;
  const size_t nb = wire_blocks(n);
  for (size_t b = 0; b < nb; ++b) {
    const uint8_t* s = src + b * kWireBlock;
    const size_t len = n - b * kWireBlock < kWireBlock ? n - b * kWireBlock : kWireBlock;
    if (pack_block(s, len, dst + o) & kHigh) {
      std::memcpy(dst + o, s, len);
      table[b] = static_cast<uint32_t>(o) | kWireRawBit;
      o += len;
    } else {
      table[b] = static_cast<uint32_t>(o);
      o += wire_packed_len(len);
    }
  }
  return o;
}

namespace {

void unpack7_block(const uint8_t* s, size_t len, uint8_t* d) {
  for (size_t g = 0; 8 * g < len; ++g) {
    uint64_t v = 0;
    std::memcpy(&v, s + 7 * g, 7);
    const uint64_t x = spread(v);
    std::memcpy(d + 8 * g, &x, len - 8 * g < 8 ? len - 8 * g : 8);
  }
}

}  // namespace

void wire_unpack(const uint8_t* packed, const uint32_t* table, size_t n, uint8_t* dst) {
  const size_t nb = wire_blocks(n);
  for (size_t b = 0; b < nb; ++b) {
    const size_t len = n - b * kWireBlock < kWireBlock ? n - b * kWireBlock : kWireBlock;
    const uint8_t* s = packed + (table[b] & ~kWireRawBit);
    uint8_t* d = dst + b * kWireBlock;
    if (table[b] & kWireRawBit) {
      std::memcpy(d, s, len);
      continue;
    }
    unpack7_block(s, len, d);
  }
}

// ---- v2: 6-bit codes with escapes (wirepack.h)

namespace {

constexpr uint32_t kAbort = ~0u;

// What the packers look bytes up in, per region: code[v] for the scalar path,
// and inv[v] = 63 - code[v] for v < 0x80 (zero for a byte that escapes), which
// the AVX2 path reads as eight 16-entry tables and the VBMI path as two
// 64-entry ones.
struct Alphabet {
  uint8_t code[256];
  alignas(64) uint8_t inv[128];
};

void choose_alphabet(const uint8_t* p, size_t len, uint8_t* vals, Alphabet* a) {
  uint32_t key[128];
  for (uint32_t v = 0; v < 128; ++v) key[v] = 127 - v;
  for (size_t i = 0; i < len; i += kWire2Sample)
    if (p[i] < 0x80) key[p[i]] += 256;             // (at most 1024 samples: the count stays above the value)
  // larger count first, then lower value
  std::partial_sort(key, key + kWire2Escape, key + 128, [](uint32_t x, uint32_t y) { return x > y; });
  std::memset(a->code, kWire2Escape, sizeof a->code);
  std::memset(a->inv, 0, sizeof a->inv);
  for (uint32_t c = 0; c < kWire2Escape; ++c) {
    const uint8_t v = static_cast<uint8_t>(127 - (key[c] & 0xFF));
    vals[c] = v;
    a->code[v] = static_cast<uint8_t>(c);
    a->inv[v] = static_cast<uint8_t>(kWire2Escape - c);
  }
  vals[kWire2Escape] = 0;
}

// The 6-bit codes of groups [g0, ...) of a block of len bytes (4 bytes -> 3),
// escaped bytes appended to esc; returns the new escape count, or kAbort once
// it reaches `limit`.  *acc gathers the OR of the bytes.
inline uint32_t pack6_groups_scalar(const uint8_t* src, size_t len, size_t g0, const Alphabet& a, uint8_t* dst,
                                    uint8_t* esc, uint32_t nesc, uint32_t limit, uint32_t* acc) {
  const size_t ng = (len + 3) / 4;
  for (size_t g = g0; g < ng; ++g) {
    uint32_t v = 0;
    const size_t k = len - 4 * g < 4 ? len - 4 * g : 4;
    for (size_t j = 0; j < k; ++j) {
      const uint8_t x = src[4 * g + j];
      const uint32_t c = a.code[x];
      *acc |= x;
      v |= c << (6 * j);
      if (c == kWire2Escape) esc[nesc++] = x;
    }
    dst[3 * g] = static_cast<uint8_t>(v);
    dst[3 * g + 1] = static_cast<uint8_t>(v >> 8);
    dst[3 * g + 2] = static_cast<uint8_t>(v >> 16);
    if (nesc >= limit) return kAbort;
  }
  return nesc;
}

uint32_t pack6_scalar(const uint8_t* src, size_t len, const Alphabet& a, uint8_t* dst, uint8_t* esc, uint32_t limit,
                      uint32_t* acc) {
  return pack6_groups_scalar(src, len, 0, a, dst, esc, 0, limit, acc);
}

#if defined(__x86_64__)
// (the stores of both vector paths run up to 16 bytes past the codes they
// hold: over the codes that follow, or into what is written after them)
__attribute__((target("avx2"))) uint32_t pack6_avx2(const uint8_t* src, size_t len, const Alphabet& a, uint8_t* dst,
                                                     uint8_t* esc, uint32_t limit, uint32_t* acc) {
  __m256i T[8], X[8];
  for (int k = 0; k < 8; ++k) {
    T[k] = _mm256_broadcastsi128_si256(_mm_load_si128(reinterpret_cast<const __m128i*>(a.inv + 16 * k)));
    X[k] = _mm256_set1_epi8(static_cast<char>(16 * k));
  }
  const __m256i k70 = _mm256_set1_epi8(0x70), k63 = _mm256_set1_epi8(63);
  const __m256i mul1 = _mm256_set1_epi16(0x4001), mul2 = _mm256_set1_epi32(0x10000001);
  const __m256i shuf = _mm256_setr_epi8(0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, -1, -1, -1, -1,
                                        0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, -1, -1, -1, -1);
  __m256i vacc = _mm256_setzero_si256();
  uint32_t nesc = 0;
  const size_t nv = len / 32;
  for (size_t i = 0; i < nv; ++i) {
    const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + 32 * i));
    vacc = _mm256_or_si256(vacc, x);
    // table k answers for the bytes whose high nibble is k: the saturating
    // add leaves their low nibble and sets bit 7 of every other byte
    __m256i r = _mm256_shuffle_epi8(T[0], _mm256_adds_epu8(x, k70));
    for (int k = 1; k < 8; ++k)
      r = _mm256_or_si256(r, _mm256_shuffle_epi8(T[k], _mm256_adds_epu8(_mm256_xor_si256(x, X[k]), k70)));
    const __m256i c = _mm256_sub_epi8(k63, r);
    uint32_t m = static_cast<uint32_t>(_mm256_movemask_epi8(_mm256_cmpeq_epi8(c, k63)));
    __m256i p = _mm256_madd_epi16(_mm256_maddubs_epi16(c, mul1), mul2);
    p = _mm256_shuffle_epi8(p, shuf);
    _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + 24 * i), _mm256_castsi256_si128(p));
    _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + 24 * i + 12), _mm256_extracti128_si256(p, 1));
    if (m) {
      for (; m; m &= m - 1) esc[nesc++] = src[32 * i + static_cast<unsigned>(__builtin_ctz(m))];
      if (nesc >= limit) return kAbort;
    }
  }
  const __m128i v = _mm_or_si128(_mm256_castsi256_si128(vacc), _mm256_extracti128_si256(vacc, 1));
  const uint64_t r = static_cast<uint64_t>(_mm_cvtsi128_si64(v)) | static_cast<uint64_t>(_mm_extract_epi64(v, 1));
  *acc |= (r & kHigh) ? 0x80u : 0u;
  return pack6_groups_scalar(src, len, nv * 8, a, dst, esc, nesc, limit, acc);
}

__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi"))) uint32_t pack6_vbmi(const uint8_t* src, size_t len,
                                                                                     const Alphabet& a, uint8_t* dst,
                                                                                     uint8_t* esc, uint32_t limit,
                                                                                     uint32_t* acc) {
  const __m512i t0 = _mm512_load_si512(a.inv), t1 = _mm512_load_si512(a.inv + 64);
  const __m512i k63 = _mm512_set1_epi8(63);
  const __m512i mul1 = _mm512_set1_epi16(0x4001), mul2 = _mm512_set1_epi32(0x10000001);
  alignas(64) uint8_t idx[64];
  for (int j = 0; j < 64; ++j) idx[j] = static_cast<uint8_t>(j < 48 ? j / 3 * 4 + j % 3 : 0);
  const __m512i gather = _mm512_load_si512(idx);
  __mmask64 high = 0;
  uint32_t nesc = 0;
  const size_t nv = len / 64;
  for (size_t i = 0; i < nv; ++i) {
    const __m512i x = _mm512_loadu_si512(src + 64 * i);
    const __mmask64 hi = _mm512_movepi8_mask(x);
    high |= hi;
    // (the permute reads index bits 0..6: bytes >= 0x80 are set to the escape code after it)
    const __m512i r = _mm512_permutex2var_epi8(t0, x, t1);
    const __m512i c = _mm512_mask_mov_epi8(_mm512_sub_epi8(k63, r), hi, k63);
    uint64_t m = _mm512_cmpeq_epi8_mask(c, k63);
    __m512i p = _mm512_madd_epi16(_mm512_maddubs_epi16(c, mul1), mul2);
    p = _mm512_permutexvar_epi8(gather, p);
    _mm512_storeu_si512(dst + 48 * i, p);
    if (m) {
      for (; m; m &= m - 1) esc[nesc++] = src[64 * i + static_cast<unsigned>(__builtin_ctzll(m))];
      if (nesc >= limit) return kAbort;
    }
  }
  *acc |= high ? 0x80u : 0u;
  return pack6_groups_scalar(src, len, nv * 16, a, dst, esc, nesc, limit, acc);
}

// pack6_vbmi with the escaped bytes of a vector gathered by one register-form
// byte compress (the store runs up to 63 bytes past them, inside esc)
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi,avx512vbmi2"))) uint32_t pack6_vbmi2(
    const uint8_t* src, size_t len, const Alphabet& a, uint8_t* dst, uint8_t* esc, uint32_t limit, uint32_t* acc) {
  const __m512i t0 = _mm512_load_si512(a.inv), t1 = _mm512_load_si512(a.inv + 64);
  const __m512i k63 = _mm512_set1_epi8(63);
  const __m512i mul1 = _mm512_set1_epi16(0x4001), mul2 = _mm512_set1_epi32(0x10000001);
  alignas(64) uint8_t idx[64];
  for (int j = 0; j < 64; ++j) idx[j] = static_cast<uint8_t>(j < 48 ? j / 3 * 4 + j % 3 : 0);
  const __m512i gather = _mm512_load_si512(idx);
  __mmask64 high = 0;
  uint32_t nesc = 0;
  const size_t nv = len / 64;
  for (size_t i = 0; i < nv; ++i) {
    const __m512i x = _mm512_loadu_si512(src + 64 * i);
    const __mmask64 hi = _mm512_movepi8_mask(x);
    high |= hi;
    const __m512i r = _mm512_permutex2var_epi8(t0, x, t1);
    const __m512i c = _mm512_mask_mov_epi8(_mm512_sub_epi8(k63, r), hi, k63);
    const __mmask64 m = _mm512_cmpeq_epi8_mask(c, k63);
    __m512i p = _mm512_madd_epi16(_mm512_maddubs_epi16(c, mul1), mul2);
    p = _mm512_permutexvar_epi8(gather, p);
    _mm512_storeu_si512(dst + 48 * i, p);
    if (m) {
      _mm512_storeu_si512(esc + nesc, _mm512_maskz_compress_epi8(m, x));
      nesc += static_cast<uint32_t>(__builtin_popcountll(m));
      if (nesc >= limit) return kAbort;
    }
  }
  *acc |= high ? 0x80u : 0u;
  return pack6_groups_scalar(src, len, nv * 16, a, dst, esc, nesc, limit, acc);
}
#endif

// ---- split blocks (wirepack.h).  A block is first taken apart into one value
// per byte of each stream (scan), which also gives every mode's size; the
// streams are packed into the destination (emit) only once split is chosen.

struct Split {
  alignas(64) uint8_t mask[kWireBlock / 8 + 64];
  alignas(64) uint8_t nib[kWireBlock + 128];     // the hot codes
  alignas(64) uint8_t five[kWireBlock + 128];    // the 5-bit values
  alignas(64) uint8_t esc[kWireBlock + 128];     // the escaping bytes
  uint32_t h = 0, e = 0;
  uint32_t e6 = 0;                               // bytes the 6-bit mode would escape
  bool high = false;                             // a byte >= 0x80 was seen
};

// (the vector emit reads whole vectors of values: zeros follow the last one)
inline void split_finish(Split* s, size_t len, uint32_t h, uint32_t e, uint32_t e6, bool high) {
  std::memset(s->nib + h, 0, 64);
  std::memset(s->five + (len - h), 0, 64);
  s->h = h; s->e = e; s->e6 = e6; s->high = high;
}

// bytes [i0, len) of a block whose 6-bit codes are in code[]
inline void split_scan_codes(const uint8_t* src, const uint8_t* code, size_t i0, size_t len, Split* s, uint32_t h,
                             uint32_t e, uint32_t e6, uint32_t acc) {
  uint32_t w = static_cast<uint32_t>(i0) - h;
  for (size_t i = i0; i < len; ++i) {
    const uint8_t x = src[i], c = code[i];
    acc |= x;
    if (i % 8 == 0) s->mask[i / 8] = 0;
    if (c < kWire2Hot) {
      s->mask[i / 8] |= static_cast<uint8_t>(1u << (i % 8));
      s->nib[h++] = c;
    } else if (c < kWire2Warm) {
      s->five[w++] = static_cast<uint8_t>(c - kWire2Hot);
    } else {
      s->five[w++] = kWire2Escape5;
      s->esc[e++] = x;
      e6 += c == kWire2Escape;
    }
  }
  split_finish(s, len, h, e, e6, (acc & 0x80) != 0);
}

void split_scan_scalar(const uint8_t* src, size_t len, const Alphabet& a, Split* s) {
  uint8_t code[kWireBlock];
  for (size_t i = 0; i < len; ++i) code[i] = a.code[src[i]];
  split_scan_codes(src, code, 0, len, s, 0, 0, 0, 0);
}

void split_emit_scalar(const Split& s, size_t len, uint8_t* d) {
  const size_t M = (len + 7) / 8, N = (s.h + 1) / 2, nf = len - s.h, F = (5 * nf + 7) / 8;
  std::memcpy(d, s.mask, M);
  d += M;
  for (size_t j = 0; j < N; ++j) d[j] = static_cast<uint8_t>(s.nib[2 * j] | s.nib[2 * j + 1] << 4);
  d += N;
  for (size_t g = 0; 5 * g < F; ++g) {
    uint64_t v = 0;
    for (int j = 0; j < 8; ++j) v |= static_cast<uint64_t>(s.five[8 * g + j]) << (5 * j);
    for (size_t j = 0; j < 5 && 5 * g + j < F; ++j) d[5 * g + j] = static_cast<uint8_t>(v >> (8 * j));
  }
  d += F;
  std::memcpy(d, s.esc, s.e);
  std::memset(d + s.e, 0, wire2_split_bytes(len, s.h, s.e) - (M + N + F + s.e));
}

#if defined(__x86_64__)
// the codes by the lookup of pack6_avx2, the streams by the scalar loop
__attribute__((target("avx2"))) void split_scan_avx2(const uint8_t* src, size_t len, const Alphabet& a, Split* s) {
  __m256i T[8], X[8];
  for (int k = 0; k < 8; ++k) {
    T[k] = _mm256_broadcastsi128_si256(_mm_load_si128(reinterpret_cast<const __m128i*>(a.inv + 16 * k)));
    X[k] = _mm256_set1_epi8(static_cast<char>(16 * k));
  }
  const __m256i k70 = _mm256_set1_epi8(0x70), k63 = _mm256_set1_epi8(63);
  alignas(32) uint8_t code[kWireBlock];
  const size_t nv = len / 32;
  for (size_t i = 0; i < nv; ++i) {
    const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + 32 * i));
    __m256i r = _mm256_shuffle_epi8(T[0], _mm256_adds_epu8(x, k70));
    for (int k = 1; k < 8; ++k)
      r = _mm256_or_si256(r, _mm256_shuffle_epi8(T[k], _mm256_adds_epu8(_mm256_xor_si256(x, X[k]), k70)));
    _mm256_store_si256(reinterpret_cast<__m256i*>(code + 32 * i), _mm256_sub_epi8(k63, r));
  }
  for (size_t i = 32 * nv; i < len; ++i) code[i] = a.code[src[i]];
  split_scan_codes(src, code, 0, len, s, 0, 0, 0, 0);
}

// Per 64 bytes: the lookup of pack6_vbmi, the hot mask, and one register-form
// byte compress per stream, each stored whole at the stream's end (so up to
// 63 bytes past it, inside the scratch).  A short last vector is loaded under
// a mask.
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi,avx512vbmi2"))) void split_scan_vbmi2(
    const uint8_t* src, size_t len, const Alphabet& a, Split* s) {
  const __m512i t0 = _mm512_load_si512(a.inv), t1 = _mm512_load_si512(a.inv + 64);
  const __m512i k63 = _mm512_set1_epi8(63), khot = _mm512_set1_epi8(static_cast<char>(kWire2Hot));
  const __m512i kwarm = _mm512_set1_epi8(static_cast<char>(kWire2Warm)), k31 = _mm512_set1_epi8(kWire2Escape5);
  uint32_t h = 0, w = 0, e = 0, e6 = 0;
  __mmask64 high = 0;
  for (size_t i = 0; i < len; i += 64) {
    const __mmask64 valid = len - i >= 64 ? ~0ull : (1ull << (len - i)) - 1;
    const __m512i x = _mm512_maskz_loadu_epi8(valid, src + i);
    const __mmask64 hi = _mm512_movepi8_mask(x);
    high |= hi;
    const __m512i r = _mm512_permutex2var_epi8(t0, x, t1);
    const __m512i c = _mm512_mask_mov_epi8(_mm512_sub_epi8(k63, r), hi, k63);
    const __mmask64 hot = _mm512_cmplt_epu8_mask(c, khot) & valid, rest = ~hot & valid;
    const uint64_t hot_bits = hot;
    std::memcpy(s->mask + i / 8, &hot_bits, 8);
    _mm512_storeu_si512(s->nib + h, _mm512_maskz_compress_epi8(hot, c));
    h += static_cast<uint32_t>(__builtin_popcountll(hot));
    const __m512i f = _mm512_min_epu8(_mm512_sub_epi8(c, khot), k31);
    _mm512_storeu_si512(s->five + w, _mm512_maskz_compress_epi8(rest, f));
    w += static_cast<uint32_t>(__builtin_popcountll(rest));
    const __mmask64 out = _mm512_cmpge_epu8_mask(c, kwarm) & valid;
    if (out) {
      _mm512_storeu_si512(s->esc + e, _mm512_maskz_compress_epi8(out, x));
      e += static_cast<uint32_t>(__builtin_popcountll(out));
      e6 += static_cast<uint32_t>(__builtin_popcountll(_mm512_cmpeq_epi8_mask(c, k63) & valid));
    }
  }
  split_finish(s, len, h, e, e6, high != 0);
}

// The fixed 2 -> 1 and 8 -> 5 packs of the two runs of values, whole vectors at
// a time: every store runs past its stream (by at most 63 bytes) into what is
// written after it, the last one past the block into the next block's bytes or
// the destination's slack.
__attribute__((target("avx512f,avx512bw,avx512vl,avx512vbmi"))) void split_emit_vbmi(const Split& s, size_t len,
                                                                                     uint8_t* d) {
  const size_t M = (len + 7) / 8, N = (s.h + 1) / 2, nf = len - s.h, F = (5 * nf + 7) / 8;
  std::memcpy(d, s.mask, M);
  d += M;
  const __m512i two = _mm512_set1_epi16(0x1001);
  for (size_t j = 0; j < s.h; j += 64) {
    const __m512i v = _mm512_load_si512(s.nib + j);
    _mm256_storeu_si256(reinterpret_cast<__m256i*>(d + j / 2), _mm512_cvtepi16_epi8(_mm512_maddubs_epi16(v, two)));
  }
  d += N;
  alignas(64) uint8_t idx[64];
  for (int j = 0; j < 64; ++j) idx[j] = static_cast<uint8_t>(j < 40 ? j / 5 * 8 + j % 5 : 5);   // (byte 5 is zero)
  const __m512i gather = _mm512_load_si512(idx);
  const __m512i mul1 = _mm512_set1_epi16(0x2001), mul2 = _mm512_set1_epi32(0x04000001);
  const __m512i lo20 = _mm512_set1_epi64(0xFFFFF), hi20 = _mm512_set1_epi64(0xFFFFF00000ll);
  for (size_t j = 0; j < nf; j += 64) {
    const __m512i v = _mm512_load_si512(s.five + j);
    // 8 values -> four 10-bit words -> two 20-bit dwords -> 40 bits of a qword
    const __m512i q = _mm512_madd_epi16(_mm512_maddubs_epi16(v, mul1), mul2);
    const __m512i p = _mm512_or_si512(_mm512_and_si512(q, lo20), _mm512_and_si512(_mm512_srli_epi64(q, 12), hi20));
    _mm512_storeu_si512(d + j / 8 * 5, _mm512_permutexvar_epi8(gather, p));
  }
  d += F;
  std::memcpy(d, s.esc, s.e);
  std::memset(d + s.e, 0, wire2_split_bytes(len, s.h, s.e) - (M + N + F + s.e));
}
#endif

}  // namespace

bool wire_have_vbmi() {
#if defined(__x86_64__)
  static const bool have = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw") &&
                           __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("avx512vbmi");
  return have;
#else
  return false;
#endif
}

bool wire_have_vbmi2() {
#if defined(__x86_64__)
  static const bool have = wire_have_vbmi() && __builtin_cpu_supports("avx512vbmi2");
  return have;
#else
  return false;
#endif
}

int wire2_path(int path) {
  if (path == kWireScalar) return kWireScalar;
  if (path != kWireAvx2 && wire_have_vbmi()) return kWireVbmi;
  return wire_have_avx2() ? kWireAvx2 : kWireScalar;
}

size_t wire_pack2(const uint8_t* src, size_t n, uint8_t* dst, uint32_t* table, uint8_t* alpha, int path,
                  Wire2Stats* stats, bool split) {
  uint32_t (*pack6)(const uint8_t*, size_t, const Alphabet&, uint8_t*, uint8_t*, uint32_t, uint32_t*) = pack6_scalar;
  uint64_t (*pack7)(const uint8_t*, size_t, uint8_t*) = pack_block_scalar;
  void (*split_scan)(const uint8_t*, size_t, const Alphabet&, Split*) = split_scan_scalar;
  void (*split_emit)(const Split&, size_t, uint8_t*) = split_emit_scalar;
#if defined(__x86_64__)
  const int used = wire2_path(path);
  if (used != kWireScalar) pack7 = pack_block_avx2;
  if (used == kWireAvx2) pack6 = pack6_avx2;
  if (used == kWireVbmi) pack6 = wire_have_vbmi2() ? pack6_vbmi2 : pack6_vbmi;
  if (used != kWireScalar) { split_scan = split_scan_avx2; }
  if (used == kWireVbmi) split_emit = split_emit_vbmi;
  if (used == kWireVbmi && wire_have_vbmi2()) split_scan = split_scan_vbmi2;
#endif
  if (n) std::memset(alpha, 0, wire2_alpha_bytes(n));
  Wire2Stats st;
  Alphabet a;
  uint8_t esc[kWireBlock + 64];
  std::unique_ptr<Split> sp(split ? new Split : nullptr);
  size_t o = 0;
  const size_t nb = wire_blocks(n);
  for (size_t b = 0; b < nb; ++b) {
    const size_t at = b * kWireBlock;
    if (at % kWire2Region == 0)
      choose_alphabet(src + at, n - at < kWire2Region ? n - at : kWire2Region, alpha + at / kWire2Region * kWire2Alpha, &a);
    const uint8_t* s = src + at;
    const size_t len = n - at < kWireBlock ? n - at : kWireBlock;
    const size_t cb = wire2_code_bytes(len);
    // 6-bit is chosen only below the raw size: once cb + escapes reach len it is out
    const uint32_t limit = len > cb ? static_cast<uint32_t>(len - cb) : 0;
    uint32_t acc = 0;
    bool no6 = false;
    if (split) {
      // every mode's size from one scan; 6-bit and 7-bit blocks are then packed as without split
      split_scan(s, len, a, sp.get());
      const size_t size7 = sp->high ? len : wire_packed_len(len), size6 = cb + ((sp->e6 + 15) & ~size_t(15));
      const size_t sizes = wire2_split_bytes(len, sp->h, sp->e);
      if (sizes < len && sizes < size7 && sizes < size6) {
        split_emit(*sp, len, dst + o);
        table[b] = static_cast<uint32_t>(o) | kWireRawBit | kWire6Bit;
        o += sizes;
        ++st.blocks_split;
        st.escaped += sp->e;
        continue;
      }
      no6 = !(size6 < len && size6 < size7);
    }
    const uint32_t nesc = limit && !no6 ? pack6(s, len, a, dst + o, esc, limit, &acc) : kAbort;
    if (nesc != kAbort) {
      const size_t size6 = cb + ((nesc + 15) & ~size_t(15));
      const bool ascii = !(acc & 0x80);
      if (size6 < len && !(ascii && wire_packed_len(len) <= size6)) {
        const size_t codes = (len + 3) / 4 * 3;
        std::memset(dst + o + codes, 0, cb - codes);
        std::memcpy(dst + o + cb, esc, nesc);
        std::memset(dst + o + cb + nesc, 0, size6 - cb - nesc);
        table[b] = static_cast<uint32_t>(o) | kWire6Bit;
        o += size6;
        ++st.blocks6;
        st.escaped += nesc;
        continue;
      }
    }
    // 7-bit if the block is ASCII and that is below the raw size, else raw
    if (wire_packed_len(len) < len && !(pack7(s, len, dst + o) & kHigh)) {
      table[b] = static_cast<uint32_t>(o);
      o += wire_packed_len(len);
      ++st.blocks7;
    } else {
      std::memcpy(dst + o, s, len);
      table[b] = static_cast<uint32_t>(o) | kWireRawBit;
      o += len;
      ++st.blocks_raw;
    }
  }
  if (stats) *stats = st;
  return o;
}

void wire_unpack2(const uint8_t* packed, const uint32_t* table, const uint8_t* alpha, size_t n, uint8_t* dst) {
  const size_t nb = wire_blocks(n);
  for (size_t b = 0; b < nb; ++b) {
    const size_t at = b * kWireBlock;
    const size_t len = n - at < kWireBlock ? n - at : kWireBlock;
    const uint8_t* s = packed + (table[b] & ~(kWireRawBit | kWire6Bit));
    uint8_t* d = dst + at;
    if ((table[b] & kWireRawBit) && (table[b] & kWire6Bit)) {
      const uint8_t* al = alpha + at / kWire2Region * kWire2Alpha;
      size_t h = 0;
      for (size_t i = 0; i < len; ++i) h += s[i / 8] >> (i % 8) & 1;
      const uint8_t* nib = s + (len + 7) / 8;
      const uint8_t* five = nib + (h + 1) / 2;
      const uint8_t* e = five + (5 * (len - h) + 7) / 8;
      size_t jn = 0, jf = 0;
      for (size_t i = 0; i < len; ++i) {
        if (s[i / 8] >> (i % 8) & 1) {
          d[i] = al[nib[jn / 2] >> (4 * (jn % 2)) & 15];
          ++jn;
        } else {
          const size_t bit = 5 * jf++;
          const uint32_t lo = five[bit >> 3], hi = (bit & 7) > 3 ? five[(bit >> 3) + 1] : 0;
          const uint32_t c = ((lo | hi << 8) >> (bit & 7)) & 31;
          d[i] = c == kWire2Escape5 ? *e++ : al[kWire2Hot + c];
        }
      }
    } else if (table[b] & kWireRawBit) {
      std::memcpy(d, s, len);
    } else if (table[b] & kWire6Bit) {
      const uint8_t* al = alpha + at / kWire2Region * kWire2Alpha;
      const uint8_t* e = s + wire2_code_bytes(len);
      for (size_t i = 0; i < len; ++i) {
        const size_t bit = 6 * i;
        const uint32_t lo = s[bit >> 3], hi = (bit & 7) > 2 ? s[(bit >> 3) + 1] : 0;
        const uint32_t c = ((lo | hi << 8) >> (bit & 7)) & 63;
        d[i] = c == kWire2Escape ? *e++ : al[c];
      }
    } else {
      unpack7_block(s, len, d);
    }
  }
}

}  // namespace tsg
