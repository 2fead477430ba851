// Walking a layer tar that lives in device memory (tarscan.hip): what the
// device marks, stated sequentially on the CPU, and the TarInput that runs
// walk_layer (tar.h; walker/tar.go:35-103) over the marked blocks.  No HIP here.
//
// walk_layer reads only 512-byte header blocks, the payload of 'x' / 'g' /
// 'L' / 'K' entries (at most 1 MiB each) and the second block of the end
// marker; everything else it skips.  Every header it accepts passes the
// checksum test, so the device tests every 512-byte block of the tar on its
// own with that test, marks the ones that pass and, behind a marked block of
// one of the four special types, the blocks of its payload.  The marked
// blocks travel to the host and the walk runs there, unchanged.  A block that
// passes without being a header (a tar stored inside the layer) only costs
// bytes; a block the walk reads that is not marked is fetched on its own
// (SparseTarInput's fallback).  A walk needs at most two such reads of at most
// 512 bytes each -- the zero block of the end marker and its successor, or
// the one block at which a malformed tar fails, or the partial tail of a
// truncated one.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "tar.h"

#if defined(__HIPCC__)
#define TSG_TAR_HD __host__ __device__
#define TSG_TAR_UNROLL _Pragma("unroll")
#else
#define TSG_TAR_HD
#define TSG_TAR_UNROLL
#endif

namespace tsg {

constexpr uint32_t kTarBlock = 512;
constexpr int64_t kTarMaxSpecial = 1 << 20;   // archive/tar maxSpecialFileSize

// archive/tar parseNumeric of an N-byte field (tar.cpp parse_numeric), byte i
// = get(i), written without a data-dependent index so that the device keeps
// the field in registers: base-256 when the first byte's high bit is set,
// else octal between leading and trailing spaces / NULs.
template <int N, class Get>
TSG_TAR_HD inline bool tar_numeric(Get get, int64_t* out) {
  const uint32_t b0 = get(0);
  if (b0 & 0x80u) {
    const uint32_t inv = (b0 & 0x40u) ? 0xffu : 0u;        // negative numbers are two's complement
    uint64_t x = 0;
TSG_TAR_UNROLL
    for (int i = 0; i < N; ++i) {
      uint32_t c = (get(i) ^ inv) & 0xffu;
      if (i == 0) c &= 0x7fu;
      if ((x >> 56) != 0) return false;                     // overflow
      x = (x << 8) | c;
    }
    if (x >> 63) return false;
    *out = inv ? ~static_cast<int64_t>(x) : static_cast<int64_t>(x);
    return true;
  }
  int st = 0;                                               // 0 leading trim, 1 digits, 2 trailing trim
  int64_t x = 0;
TSG_TAR_UNROLL
  for (int i = 0; i < N; ++i) {
    const uint32_t c = get(i);
    const bool pad = c == ' ' || c == 0, dig = c >= '0' && c <= '7';
    if (st == 0) {
      if (pad) continue;
      if (!dig) return false;
      st = 1;
      x = c - '0';
    } else if (st == 1) {
      if (dig) {
        if (x > (INT64_MAX >> 3)) return false;
        x = x * 8 + (c - '0');
      } else if (pad) {
        st = 2;
      } else {
        return false;
      }
    } else if (!pad) {
      return false;                                         // a digit behind an inner space or NUL
    }
  }
  *out = x;
  return true;
}

// tar.cpp checksum_ok: the checksum field parses and equals the block's sum
// with that field read as spaces, bytes unsigned or signed
TSG_TAR_HD inline bool tar_block_is_header(const uint8_t* h) {
  int64_t want = 0;
  if (!tar_numeric<8>([h](int i) { return static_cast<uint32_t>(h[148 + i]); }, &want)) return false;
  int64_t u = 0, sg = 0;
  for (uint32_t i = 0; i < kTarBlock; ++i) {
    const uint8_t c = (i >= 148 && i < 156) ? ' ' : h[i];
    u += c;
    sg += static_cast<int8_t>(c);
  }
  return want == u || want == sg;
}

// Blocks of payload the walk reads behind header h: ceil(size / 512) for the
// types 'x', 'g', 'L', 'K' with 0 <= size <= 1 MiB, else 0
TSG_TAR_HD inline uint32_t tar_special_blocks(const uint8_t* h) {
  const uint8_t t = h[156];
  if (t != 'x' && t != 'g' && t != 'L' && t != 'K') return 0;
  int64_t size = 0;
  if (!tar_numeric<12>([h](int i) { return static_cast<uint32_t>(h[124 + i]); }, &size)) return 0;
  if (size < 0 || size > kTarMaxSpecial) return 0;
  return static_cast<uint32_t>((size + kTarBlock - 1) / kTarBlock);
}

// What the device marks: marks[b] (b < len / 512) = 1 for every whole block
// that passes tar_block_is_header and for the payload blocks behind a special
// one, clipped to the whole blocks that exist; 0 elsewhere.
inline void plan_tar_marks(const uint8_t* tar, uint64_t len, uint8_t* marks) {
  const uint64_t nb = len / kTarBlock;
  if (nb) std::memset(marks, 0, nb);
  for (uint64_t b = 0; b < nb; ++b) {
    const uint8_t* h = tar + b * kTarBlock;
    if (!tar_block_is_header(h)) continue;
    marks[b] = 1;
    const uint64_t k = tar_special_blocks(h);
    for (uint64_t j = 1; j <= k && b + j < nb; ++j) marks[b + j] = 1;
  }
}

// A tar of `len` bytes of which only the blocks idx[0..n) (ascending block
// numbers, block k's bytes at blocks + 512 k) are at hand.  read serves from
// them; a range that is not among them comes from `fallback` (one call per
// maximal run inside a read), which is counted.  skip only moves pos.
class SparseTarInput : public TarInput {
 public:
  using Fallback = std::function<bool(uint64_t off, uint8_t* dst, size_t n, std::string* err)>;
  SparseTarInput(const uint64_t* idx, const uint8_t* blocks, size_t n, uint64_t len, Fallback fallback)
      : idx_(idx), blocks_(blocks), n_(n), len_(len), fallback_(std::move(fallback)) {}
  bool read(uint8_t* dst, size_t n, size_t* got, std::string* err) override {
    const uint64_t end = pos + std::min<uint64_t>(n, len_ - pos);
    size_t done = 0;
    while (pos < end) {
      const uint8_t* g = find(pos / kTarBlock);
      uint64_t e = std::min<uint64_t>(end, (pos / kTarBlock + 1) * kTarBlock);
      if (g) {
        std::memcpy(dst + done, g + pos % kTarBlock, e - pos);
      } else {
        while (e < end && !find(e / kTarBlock)) e = std::min<uint64_t>(end, e + kTarBlock);
        if (!fallback_(pos, dst + done, static_cast<size_t>(e - pos), err)) return false;
        ++fallback_reads;
        fallback_bytes += e - pos;
      }
      done += static_cast<size_t>(e - pos);
      pos = e;
    }
    *got = done;
    return true;
  }
  bool skip(uint64_t n, uint64_t* got, std::string*) override {
    *got = std::min<uint64_t>(n, len_ - pos);
    pos += *got;
    return true;
  }
  uint32_t fallback_reads = 0;
  uint64_t fallback_bytes = 0;

 private:
  const uint8_t* find(uint64_t b) const {
    const uint64_t* p = std::lower_bound(idx_, idx_ + n_, b);
    return p != idx_ + n_ && *p == b ? blocks_ + static_cast<size_t>(p - idx_) * kTarBlock : nullptr;
  }
  const uint64_t* idx_;
  const uint8_t* blocks_;
  size_t n_;
  uint64_t len_;
  Fallback fallback_;
};

// The content pass (prep.h) over the tar itself: 2n + 1 entries -- gap, file
// 0, gap, file 1, ..., tail gap -- where a gap covers headers, padding and
// the entries the walk did not hand on, and has flags 0, so it is dropped and
// emits nothing.  off: 2n + 2, flags: 2n + 1.
inline void tar_interleave(const std::vector<TarFile>& files, uint64_t len, const uint8_t* file_flags,
                           std::vector<uint64_t>* off, std::vector<uint8_t>* flags) {
  const size_t n = files.size();
  off->assign(2 * n + 2, 0);
  flags->assign(2 * n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    (*off)[2 * i + 1] = files[i].offset;
    (*off)[2 * i + 2] = files[i].offset + files[i].size;
    (*flags)[2 * i + 1] = file_flags[i];
  }
  (*off)[2 * n + 1] = len;
}

// ... and back: kinds and new starts of the n files from those of the 2n + 1 entries
inline void tar_uninterleave(const std::vector<uint8_t>& kinds2, const std::vector<uint64_t>& new_off2,
                             std::vector<uint8_t>* kinds, std::vector<uint64_t>* new_off) {
  const size_t n = kinds2.size() / 2;
  kinds->resize(n);
  new_off->resize(n + 1);
  for (size_t i = 0; i < n; ++i) {
    (*kinds)[i] = kinds2[2 * i + 1];
    (*new_off)[i] = new_off2[2 * i + 1];
  }
  (*new_off)[n] = new_off2[2 * n + 1];
}

// Statistics of one device walk (tsg_prepared_tar_stats)
struct TarScanStats {
  uint64_t blocks = 0, marked = 0, gathered_bytes = 0;
  uint32_t fallback_reads = 0, retries = 0;
  double scan_ms = 0;        // kernel time of the mark / count / scan / compact pass (the last try)
};

}  // namespace tsg
