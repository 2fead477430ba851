// Device side of the wire packing (wirepack.h): restores a packed strip that
// the copy engine landed in a device buffer to its original bytes in the
// upload ring, before K1 reads them.
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
      if (16 * t + 16 <= len) {
        reinterpret_cast<uint4*>(out)[t] = reinterpret_cast<const uint4*>(src)[t];
      } else {
        for (uint32_t i = 16 * t; i < len; ++i) out[i] = src[i];
      }
      continue;
    }
    const uint32_t pl = (len + 7) / 8 * 7;
    if (16 * t < pl) sh[t] = reinterpret_cast<const uint4*>(src)[t];
    __syncthreads();
    if (16 * t < len) {
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
    __syncthreads();                     // sh is reloaded by the next block
  }
}

void wire_unpack_launch(const uint8_t* land, uint32_t tab_bytes, uint8_t* dst, uint32_t n, hipStream_t stream) {
  const uint32_t nb = static_cast<uint32_t>(wire_blocks(n));
  if (nb == 0) return;
  hipLaunchKernelGGL(tsg_wire_unpack, dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, stream, land, tab_bytes, dst, n);
}

bool wire_unpack_device_probe(const uint8_t* packed, size_t packed_len, const uint32_t* table, size_t n, uint8_t* out,
                              const char** err) {
  *err = "";
  if (n == 0) return true;
  if (n > kWireMaxStrip) { *err = "strip too large"; return false; }
  const size_t tab = wire_table_bytes(n), guard = 64;
  std::vector<uint8_t> h(tab + packed_len + kWireSlack, 0);
  std::memcpy(h.data(), table, wire_blocks(n) * sizeof(uint32_t));
  std::memcpy(h.data() + tab, packed, packed_len);
  std::vector<uint8_t> back(n + guard);
  uint8_t *d_land = nullptr, *d_out = nullptr;
  bool ok = hipSetDevice(0) == hipSuccess && hipMalloc(&d_land, h.size()) == hipSuccess &&
            hipMalloc(&d_out, n + guard) == hipSuccess &&
            hipMemcpy(d_land, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemset(d_out, 0xA5, n + guard) == hipSuccess;
  if (ok) {
    wire_unpack_launch(d_land, static_cast<uint32_t>(tab), d_out, static_cast<uint32_t>(n), nullptr);
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

}  // namespace tsg
