// Host side of the wire packing (wirepack.h): a scalar 64-bit SWAR path and an
// AVX2 path, chosen at run time, and the reference unpack.
#include "wirepack.h"

#include <cstring>

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
    for (size_t g = 0; 8 * g < len; ++g) {
      uint64_t v = 0;
      std::memcpy(&v, s + 7 * g, 7);
      const uint64_t x = spread(v);
      std::memcpy(d + 8 * g, &x, len - 8 * g < 8 ? len - 8 * g : 8);
    }
  }
}

}  // namespace tsg
