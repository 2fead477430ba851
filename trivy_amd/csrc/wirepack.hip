// Device side of the wire packing (wirepack.h): restores a packed strip that
// the copy engine landed in a device buffer to its original bytes in the
// upload ring, before K1 reads them; one kernel per codec.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "wirepack.h"

namespace tsg {

namespace {

__device__ __forceinline__ unsigned long long wire_spread(unsigned long long v) {
  unsigned long long x = (v & 0x000000000FFFFFFFull) | ((v << 4) & 0x0FFFFFFF00000000ull);
  x = (x & 0x00003FFF00003FFFull) | ((x << 2) & 0x3FFF00003FFF0000ull);
  return (x & 0x007F007F007F007Full) | ((x << 1) & 0x7F007F007F007F00ull);
}

// Lane t's 16 bytes of a 7-bit block of len bytes whose packed form is in sh:
// its 14 bytes (two groups) from the four dwords that hold them, stored as one
// 16-byte word (single bytes where the block ends inside them).
__device__ __forceinline__ void unpack7_lane(const uint4* sh, uint32_t t, uint32_t len, uint8_t* __restrict__ out) {
  if (16 * t >= len) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(sh) + ((14 * t) >> 2);
  const unsigned long long lo = w[0] | (static_cast<unsigned long long>(w[1]) << 32);
  const unsigned long long hi = w[2] | (static_cast<unsigned long long>(w[3]) << 32);
  const unsigned long long m56 = (1ull << 56) - 1;
  // the lane's 112 bits start at bit 0 or bit 16 of lo:hi
  const bool odd = (14 * t) & 2;
  const unsigned long long g0 = (odd ? (lo >> 16) | (hi << 48) : lo) & m56;
  const unsigned long long g1 = (odd ? hi >> 8 : (lo >> 56) | (hi << 8)) & m56;
  const unsigned long long x0 = wire_spread(g0), x1 = wire_spread(g1);
  if (16 * t + 16 <= len) {
    uint4 v;
    v.x = static_cast<uint32_t>(x0); v.y = static_cast<uint32_t>(x0 >> 32);
    v.z = static_cast<uint32_t>(x1); v.w = static_cast<uint32_t>(x1 >> 32);
    reinterpret_cast<uint4*>(out)[t] = v;
  } else {
    for (uint32_t i = 16 * t; i < len; ++i) {
      const uint32_t k = i - 16 * t;
      out[i] = static_cast<uint8_t>((k < 8 ? x0 : x1) >> (8 * (k & 7)));
    }
  }
}

__device__ __forceinline__ void copy_raw_lane(const uint8_t* __restrict__ src, uint32_t t, uint32_t len,
                                              uint8_t* __restrict__ out) {
  if (16 * t + 16 <= len) {
    reinterpret_cast<uint4*>(out)[t] = reinterpret_cast<const uint4*>(src)[t];
  } else {
    for (uint32_t i = 16 * t; i < len; ++i) out[i] = src[i];
  }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// A split block (wirepack.h) of len bytes at src, by the whole workgroup; lane
// t owns output bytes 16t .. 16t+15.
//   1. The lane reads its 16 mask bits from global memory; an exclusive scan
//      of their popcounts over the workgroup (a wave scan and the four wave
//      totals in LDS) gives its first hot code and, as 16t less that, its
//      first 5-bit value; the total gives the block's hot count, hence the
//      size of the three streams in front of the escaped bytes.
//   2. Exactly those streams (rounded up to 16 bytes, which the block's own
//      padding covers) and the region's alphabet go to LDS.
//   3. The lane takes the three dwords that hold its hot codes and the four
//      that hold its 5-bit values (reads of LDS may run past the streams, never
//      past sh; what they bring is not used), counts the escapes among its
//      values, and a second scan gives its first escaped byte, read from
//      global memory.
//   4. One 16-byte store; single bytes only in a strip's short last block.
__device__ __forceinline__ void unpack_split_block(const uint8_t* __restrict__ src, const uint8_t* __restrict__ alpha,
                                                   uint32_t len, uint8_t* __restrict__ out, uint4* sh, uint4* sh_alpha,
                                                   uint32_t* sh_wave, uint32_t* sh_wave2) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t mine = 16 * t < len ? min(16u, len - 16 * t) : 0u;   // output bytes of this lane
  const uint32_t mb = (len + 7) / 8;
  uint32_t m = 0;
  if (mine > 8) m = reinterpret_cast<const uint16_t*>(src)[t];
  else if (mine) m = src[2 * t];
  const uint32_t hot = __popc(m), warm = mine - hot;                   // (mask bits past len are zero)
  const uint32_t incl = wave_incl_scan(hot, lane);
  if (lane == 63) sh_wave[wave] = incl;
  if (t < kWire2Alpha / 16) sh_alpha[t] = reinterpret_cast<const uint4*>(alpha)[t];
  __syncthreads();
  uint32_t ni = incl - hot, h = 0;
  for (uint32_t v = 0; v < 4; ++v) {
    const uint32_t x = sh_wave[v];
    ni += v < wave ? x : 0u;
    h += x;
  }
  h = min(h, len);                                                     // (no more than a well-formed mask has)
  const uint32_t fb = mb + (h + 1) / 2;                                // the 5-bit values' first byte
  const uint32_t sbytes = fb + (5 * (len - h) + 7) / 8;                // <= 3073 < sizeof sh
  if (16 * t < sbytes) sh[t] = reinterpret_cast<const uint4*>(src)[t];
  __syncthreads();
  const uint32_t* w = reinterpret_cast<const uint32_t*>(sh);
  unsigned long long nibs = 0, f0 = 0, f1 = 0;
  uint32_t nesc = 0;
  if (mine) {
    {
      const uint32_t at = mb + (ni >> 1), d = at >> 2, sft = (at & 3u) * 8 + (ni & 1u) * 4;
      const unsigned long long lo = w[d] | (static_cast<unsigned long long>(w[d + 1]) << 32);
      nibs = sft ? (lo >> sft) | (static_cast<unsigned long long>(w[d + 2]) << (64 - sft)) : lo;
    }
    {
      const uint32_t bit = 8 * fb + 5 * (16 * t - ni), d = bit >> 5, sft = bit & 31u;
      const unsigned long long lo = w[d] | (static_cast<unsigned long long>(w[d + 1]) << 32);
      const unsigned long long hi = w[d + 2] | (static_cast<unsigned long long>(w[d + 3]) << 32);
      f0 = sft ? (lo >> sft) | (hi << (64 - sft)) : lo;
      f1 = hi >> sft;
    }
    unsigned long long g0 = f0, g1 = f1;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      nesc += (j < warm && (g0 & 31u) == kWire2Escape5) ? 1u : 0u;
      g0 = (g0 >> 5) | (g1 << 59);
      g1 >>= 5;
    }
  }
  const uint32_t incl2 = wave_incl_scan(nesc, lane);
  if (lane == 63) sh_wave2[wave] = incl2;
  __syncthreads();
  uint32_t e = incl2 - nesc;                                           // index of the lane's first escaped byte
  for (uint32_t v = 0; v < wave; ++v) e += sh_wave2[v];
  if (mine) {
    const uint8_t* __restrict__ esc = src + sbytes;
    const uint8_t* al = reinterpret_cast<const uint8_t*>(sh_alpha);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      uint32_t v;
      if ((m >> k) & 1u) {
        v = al[nibs & 15u];
        nibs >>= 4;
      } else {
        const uint32_t c = static_cast<uint32_t>(f0) & 31u;
        f0 = (f0 >> 5) | (f1 << 59);
        f1 >>= 5;
        v = al[kWire2Hot + c];
        if (c == kWire2Escape5) v = k < mine ? esc[e++] : 0u;
      }
      o[k >> 2] |= v << (8 * (k & 3));
    }
    if (mine == 16) {
      reinterpret_cast<uint4*>(out)[t] = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
      for (uint32_t k = 0; k < mine; ++k) out[16 * t + k] = static_cast<uint8_t>(o[k >> 2] >> (8 * (k & 3)));
    }
  }
  __syncthreads();                       // sh, sh_alpha and the wave totals are rewritten by the next block
}

}  // namespace

// One workgroup of 256 lanes per block of kWireBlock bytes (grid-stride over
// the strip's blocks).  land = the block table (tab_bytes) followed by the
// packed bytes; block offsets are multiples of 16 and land, dst are 16-byte
// aligned.  A packed block's 3584 bytes go to LDS with one 16-byte load per
// lane; each lane then takes its 14 bytes (two groups) from the four dwords
// that hold them and stores 16 restored bytes.  A raw block is a 16-byte copy
// per lane.  Only a strip's short last block has lanes that store single
// bytes (fewer than 16 of them).  Loads may run up to 15 bytes past the packed
// bytes (kWireSlack); nothing is stored at or past dst + n.
__global__ __launch_bounds__(256) void tsg_wire_unpack(const uint8_t* __restrict__ land, uint32_t tab_bytes,
                                                        uint8_t* __restrict__ dst, uint32_t n) {
  __shared__ uint4 sh[kWireBlockPacked / 16];
  const uint32_t* __restrict__ tab = reinterpret_cast<const uint32_t*>(land);
  const uint8_t* __restrict__ data = land + tab_bytes;
  const uint32_t nb = (n + kWireBlock - 1) / kWireBlock;
  const uint32_t t = threadIdx.x;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t ent = tab[b];
    const uint32_t len = min(kWireBlock, n - b * kWireBlock);
    const uint8_t* __restrict__ src = data + (ent & ~kWireRawBit);
    uint8_t* __restrict__ out = dst + static_cast<size_t>(b) * kWireBlock;
    if (ent & kWireRawBit) {             // (uniform over the workgroup)
      copy_raw_lane(src, t, len, out);
      continue;
    }
    const uint32_t pl = (len + 7) / 8 * 7;
    if (16 * t < pl) sh[t] = reinterpret_cast<const uint4*>(src)[t];
    __syncthreads();
    unpack7_lane(sh, t, len, out);
    __syncthreads();                     // sh is reloaded by the next block
  }
}

// The v2 unpack (wirepack.h): the same grid and blocks, four modes (a split
// block goes through unpack_split_block above).  land =
// the block table (tab_bytes), the alphabets (alpha_bytes, 64 bytes per region
// of 16 blocks) and the packed bytes.  Raw and 7-bit blocks go as in
// tsg_wire_unpack.  A 6-bit block's codes (at most 3072 bytes, a multiple of
// 16) and its region's alphabet go to LDS; lane t owns code bytes 12t..12t+11
// (three dwords), that is 16 codes and 16 output bytes.  Each lane counts the
// escape codes among its codes below len, an exclusive scan over the workgroup
// (a wave scan and the four wave totals in LDS) gives its first escaped byte,
// and it reads those from the block's tail in global memory.  Loads of a 6-bit
// block stay inside its payload; a short 7-bit block's may run up to 15 bytes
// past it (kWireSlack).  A split block's loads stay inside its payload too:
// the mask bits a lane owns, the three streams rounded up to 16 bytes (which
// the block's own pad to 16 covers) and its escaped bytes one by one.  Nothing
// is stored at or past dst + n.
__global__ __launch_bounds__(256) void tsg_wire_unpack2(const uint8_t* __restrict__ land, uint32_t tab_bytes,
                                                         uint32_t alpha_bytes, uint8_t* __restrict__ dst, uint32_t n) {
  __shared__ uint4 sh[kWireBlockPacked / 16];
  __shared__ uint4 sh_alpha[kWire2Alpha / 16];
  __shared__ uint32_t sh_wave[4], sh_wave2[4];
  const uint32_t* __restrict__ tab = reinterpret_cast<const uint32_t*>(land);
  const uint8_t* __restrict__ alphas = land + tab_bytes;
  const uint8_t* __restrict__ data = alphas + alpha_bytes;
  const uint32_t nb = (n + kWireBlock - 1) / kWireBlock;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const uint32_t ent = tab[b];
    const uint32_t len = min(kWireBlock, n - b * kWireBlock);
    const uint8_t* __restrict__ src = data + (ent & ~(kWireRawBit | kWire6Bit));
    uint8_t* __restrict__ out = dst + static_cast<size_t>(b) * kWireBlock;
    if ((ent & kWireRawBit) && (ent & kWire6Bit)) {   // (the mode is uniform over the workgroup)
      unpack_split_block(src, alphas + static_cast<size_t>(b / (kWire2Region / kWireBlock)) * kWire2Alpha, len, out, sh,
                         sh_alpha, sh_wave, sh_wave2);
      continue;
    }
    if (ent & kWireRawBit) {
      copy_raw_lane(src, t, len, out);
      continue;
    }
    if (!(ent & kWire6Bit)) {
      const uint32_t pl = (len + 7) / 8 * 7;
      if (16 * t < pl) sh[t] = reinterpret_cast<const uint4*>(src)[t];
      __syncthreads();
      unpack7_lane(sh, t, len, out);
      __syncthreads();
      continue;
    }
    const uint32_t cb = ((len + 3) / 4 * 3 + 15u) & ~15u;
    if (16 * t < cb) sh[t] = reinterpret_cast<const uint4*>(src)[t];
    if (t < kWire2Alpha / 16)
      sh_alpha[t] = reinterpret_cast<const uint4*>(alphas + static_cast<size_t>(b / (kWire2Region / kWireBlock)) * kWire2Alpha)[t];
    __syncthreads();
    const uint32_t mine = 16 * t < len ? min(16u, len - 16 * t) : 0u;   // output bytes of this lane
    uint32_t g[4] = {0, 0, 0, 0};        // four codes (24 bits) each
    uint32_t nesc = 0;
    if (mine) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(sh) + 3 * t;
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      g[0] = w0 & 0xFFFFFFu;
      g[1] = ((w0 >> 24) | (w1 << 8)) & 0xFFFFFFu;
      g[2] = ((w1 >> 16) | (w2 << 16)) & 0xFFFFFFu;
      g[3] = w2 >> 8;
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k)
        nesc += (k < mine && ((g[k >> 2] >> (6 * (k & 3))) & 63u) == kWire2Escape) ? 1u : 0u;
    }
    const uint32_t incl = wave_incl_scan(nesc, lane);
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    uint32_t e = incl - nesc;            // index of the lane's first escaped byte
    for (uint32_t v = 0; v < wave; ++v) e += sh_wave[v];
    if (mine) {
      const uint8_t* __restrict__ esc = src + cb;
      const uint8_t* al = reinterpret_cast<const uint8_t*>(sh_alpha);
      uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t c = (g[k >> 2] >> (6 * (k & 3))) & 63u;
        uint32_t v = al[c];
        if (c == kWire2Escape && k < mine) v = esc[e++];
        o[k >> 2] |= v << (8 * (k & 3));
      }
      if (mine == 16) {
        reinterpret_cast<uint4*>(out)[t] = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        for (uint32_t k = 0; k < mine; ++k) out[16 * t + k] = static_cast<uint8_t>(o[k >> 2] >> (8 * (k & 3)));
      }
    }
    __syncthreads();                     // sh, sh_alpha and sh_wave are rewritten by the next block
  }
}

void wire_unpack_launch(const uint8_t* land, uint32_t tab_bytes, uint8_t* dst, uint32_t n, hipStream_t stream) {
  const uint32_t nb = static_cast<uint32_t>(wire_blocks(n));
  if (nb == 0) return;
  hipLaunchKernelGGL(tsg_wire_unpack, dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, stream, land, tab_bytes, dst, n);
}

void wire_unpack2_launch(const uint8_t* land, uint32_t tab_bytes, uint32_t alpha_bytes, uint8_t* dst, uint32_t n,
                         hipStream_t stream) {
  const uint32_t nb = static_cast<uint32_t>(wire_blocks(n));
  if (nb == 0) return;
  hipLaunchKernelGGL(tsg_wire_unpack2, dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, stream, land, tab_bytes, alpha_bytes,
                     dst, n);
}

namespace {

// Lands a packed strip (the table, for v2 the alphabets, the packed bytes) on
// device 0, runs the codec's unpack kernel and reads the n bytes back.
bool unpack_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, const uint8_t* alpha, size_t n,
                  uint8_t* out, const char** err) {
  *err = "";
  if (n == 0) return true;
  if (n > kWireMaxStrip) { *err = "strip too large"; return false; }
  const size_t tab = wire_table_bytes(n), al = alpha ? wire2_alpha_bytes(n) : 0, guard = 64;
  std::vector<uint8_t> h(tab + al + packed_len + kWireSlack, 0);
  std::memcpy(h.data(), table, wire_blocks(n) * sizeof(uint32_t));
  if (alpha) std::memcpy(h.data() + tab, alpha, al);
  std::memcpy(h.data() + tab + al, packed, packed_len);
  std::vector<uint8_t> back(n + guard);
  uint8_t *d_land = nullptr, *d_out = nullptr;
  bool ok = hipSetDevice(0) == hipSuccess && hipMalloc(&d_land, h.size()) == hipSuccess &&
            hipMalloc(&d_out, n + guard) == hipSuccess &&
            hipMemcpy(d_land, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemset(d_out, 0xA5, n + guard) == hipSuccess;
  if (ok) {
    if (alpha) {
      wire_unpack2_launch(d_land, static_cast<uint32_t>(tab), static_cast<uint32_t>(al), d_out, static_cast<uint32_t>(n),
                          nullptr);
    } else {
      wire_unpack_launch(d_land, static_cast<uint32_t>(tab), d_out, static_cast<uint32_t>(n), nullptr);
    }
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(back.data(), d_out, n + guard, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (d_land) hipFree(d_land);
  if (d_out) hipFree(d_out);
  if (!ok) { *err = "HIP call failed in the wire unpack probe"; (void)hipGetLastError(); return false; }
  // the kernel stores nothing past the strip
  for (size_t i = 0; i < guard; ++i)
    if (back[n + i] != 0xA5) { *err = "the unpack kernel wrote past the strip"; return false; }
  std::memcpy(out, back.data(), n);
  return true;
}

}  // namespace

bool wire_unpack_device_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, size_t n, uint8_t* out,
                              const char** err) {
  return unpack_probe(packed, packed_len, table, nullptr, n, out, err);
}

bool wire_unpack2_device_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, const uint8_t* alpha,
                               size_t n, uint8_t* out, const char** err) {
  return unpack_probe(packed, packed_len, table, alpha, n, out, err);
}

}  // namespace tsg
