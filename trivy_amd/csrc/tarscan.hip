// Device side of the layer-tar walk: the blocks of a tar in device memory
// that walk_layer (tar.cpp; walker/tar.go:35-103) may read -- every 512-byte
// block that passes the header checksum, and the payload blocks behind an
// 'x' / 'g' / 'L' / 'K' header -- compacted, each with its block number, into
// memory the host reads.  tarscan.h states what is marked (plan_tar_marks is
// the CPU model of this file) and why the walk stays exact whatever is marked.
//
// Reduce / scan / compact over regions of 128 blocks (64 KiB, prep.hip's
// region; one wave each), the scan being prep.hip's own kernel:
//   tsg_tar_mark      marks[b] = 1 for a header and for a special header's payload   reads N/32 + the candidates
//   tsg_tar_count     region_n[r] = marked blocks of region r
//   tsg_prep_scan     exclusive prefix and the total (region_scan_launch)
//   tsg_tar_compact   the marked blocks and their numbers to their place            reads, writes 512 B per mark
//
// tsg_tar_mark: lane l of a wave step holds block l's bytes 144..159, one
// 16-byte load: the checksum field (148..155) and the type flag (156).  A
// field that does not parse -- most file content -- ends the block there.
// The blocks whose field parses (all-NUL = 0 among them: the signed sum can
// be 0) are summed two at a time, one per half wave, lane j of the half
// taking bytes [16j, 16j + 16) as one load: byte sum by v_sad_u8, the signed
// sum from it and the count of bytes >= 0x80.  Only a special header reads
// its size field.  A payload's marks may lie in other regions, so they are
// stores of 1 into an array zeroed before the launch, and the count is a
// kernel of its own behind it.
#include "prep_dev.h"
#include "tarscan_dev.h"

namespace tsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kRegionBlocks = 128;      // blocks per wave (one 64 KiB region)
constexpr uint32_t kWaves = 4;               // waves per workgroup

__device__ __forceinline__ uint32_t byte_sum(uint32_t d, uint32_t acc) { return __builtin_amdgcn_sad_u8(d, 0u, acc); }

__global__ __launch_bounds__(256) void tsg_tar_mark(const uint8_t* __restrict__ tar, uint64_t nblocks,
                                                    uint8_t* __restrict__ marks) {
  const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, l32 = lane & 31u;
  const uint64_t b0 = (static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * kRegionBlocks;
  if (b0 >= nblocks) return;                 // whole waves only
  for (uint32_t step = 0; step < kRegionBlocks / 64; ++step) {
    const uint64_t s0 = b0 + step * 64u;
    if (s0 >= nblocks) break;
    const uint64_t b = s0 + lane;
    bool cand = false;
    int64_t want = 0;
    uint32_t type = 0;
    if (b < nblocks) {
      const v4u f = *reinterpret_cast<const v4u*>(tar + b * kTarBlock + 144);
      const uint64_t v = f.y | (static_cast<uint64_t>(f.z) << 32);
      cand = tar_numeric<8>([v](int i) { return static_cast<uint32_t>(v >> (8 * i)) & 0xffu; }, &want);
      type = f.w & 0xffu;
    }
    uint64_t bal = __ballot(cand);
    bool hdr = false;
    while (bal) {                            // wave-uniform: two candidates per turn, one per half wave
      const uint32_t k0 = static_cast<uint32_t>(__builtin_ctzll(bal));
      bal &= bal - 1;
      uint32_t k1 = k0;
      if (bal) {
        k1 = static_cast<uint32_t>(__builtin_ctzll(bal));
        bal &= bal - 1;
      }
      const uint32_t k = half ? k1 : k0;
      v4u w = *reinterpret_cast<const v4u*>(tar + (s0 + k) * kTarBlock + 16u * l32);
      if (l32 == 9) w.y = w.z = 0x20202020u;  // the checksum field reads as spaces
      uint32_t u = byte_sum(w.x, byte_sum(w.y, byte_sum(w.z, byte_sum(w.w, 0u))));
      uint32_t neg = __popc(w.x & 0x80808080u) + __popc(w.y & 0x80808080u) + __popc(w.z & 0x80808080u) +
                     __popc(w.w & 0x80808080u);
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) {     // within each half
        u += __shfl_xor(u, d);
        neg += __shfl_xor(neg, d);
      }
      const int64_t us = u, sg = static_cast<int64_t>(u) - 256 * static_cast<int64_t>(neg);
      // lane k's own half may not be the half that summed it: ask that half
      const uint32_t from0 = 0, from1 = 32;
      const int64_t u0 = __shfl(us, from0), g0 = __shfl(sg, from0), u1 = __shfl(us, from1), g1 = __shfl(sg, from1);
      if (lane == k0) hdr = want == u0 || want == g0;
      if (k1 != k0 && lane == k1) hdr = want == u1 || want == g1;
    }
    uint32_t nb = 0;
    if (hdr) {
      marks[b] = 1;
      if (type == 'x' || type == 'g' || type == 'L' || type == 'K') {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(tar + b * kTarBlock + 124);
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
        int64_t size = 0;
        const bool ok = tar_numeric<12>([d0, d1, d2](int i) {
          return ((i < 4 ? d0 : i < 8 ? d1 : d2) >> (8 * (i & 3))) & 0xffu;
        }, &size);
        if (ok && size >= 0 && size <= kTarMaxSpecial) nb = static_cast<uint32_t>((size + kTarBlock - 1) / kTarBlock);
      }
    }
    uint64_t sp = __ballot(nb != 0);
    while (sp) {                             // a special header's payload: the wave stores its marks
      const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(sp));
      sp &= sp - 1;
      const uint64_t first = s0 + k + 1;
      const uint64_t end = min(first + __shfl(nb, k), nblocks);
      for (uint64_t j = first + lane; j < end; j += 64) marks[j] = 1;
    }
  }
}

// one thread per region: its 128 mark bytes (0 or 1) as eight 16-byte loads
__global__ __launch_bounds__(256) void tsg_tar_count(const uint8_t* __restrict__ marks, uint32_t nregions,
                                                     uint32_t* __restrict__ region_n) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nregions) return;
  const v4u* p = reinterpret_cast<const v4u*>(marks + static_cast<uint64_t>(r) * kRegionBlocks);
  uint32_t n = 0;
#pragma unroll
  for (uint32_t q = 0; q < kRegionBlocks / 16; ++q) {
    const v4u w = p[q];
    n += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
  }
  region_n[r] = n;
}

// The marked blocks of region r to out_blocks from entry region_base[r] on,
// two at a time (one per half wave, 16 bytes per lane), and their block
// numbers to out_idx.  Nothing is written when they do not all fit.
__global__ __launch_bounds__(256) void tsg_tar_compact(const uint8_t* __restrict__ tar,
                                                       const uint8_t* __restrict__ marks, uint32_t nregions,
                                                       const uint64_t* __restrict__ region_base,
                                                       const uint64_t* __restrict__ total,
                                                       uint8_t* __restrict__ out_blocks, uint64_t* __restrict__ out_idx,
                                                       uint64_t cap_blocks) {
  __shared__ uint8_t list[kWaves][kRegionBlocks];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31u;
  const uint32_t r = blockIdx.x * kWaves + wv;
  if (r >= nregions) return;                 // whole waves only; no workgroup barrier below
  if (*total > cap_blocks) return;
  const uint64_t b0 = static_cast<uint64_t>(r) * kRegionBlocks;
  const uint32_t m = reinterpret_cast<const uint16_t*>(marks + b0)[lane];
  const uint32_t m0 = m & 1u, m1 = (m >> 8) & 1u;
  uint32_t incl = m0 + m1;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  const uint32_t excl = incl - m0 - m1, K = __shfl(incl, 63);
  if (K == 0) return;
  uint8_t* lb = list[wv];
  if (m0) lb[excl] = static_cast<uint8_t>(2 * lane);
  if (m1) lb[excl + m0] = static_cast<uint8_t>(2 * lane + 1);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint64_t base = region_base[r];
  for (uint32_t k = half; k < K; k += 2) {
    const uint64_t blk = b0 + lb[k];
    const v4u w = *reinterpret_cast<const v4u*>(tar + blk * kTarBlock + 16u * l32);
    *reinterpret_cast<v4u*>(out_blocks + (base + k) * kTarBlock + 16u * l32) = w;
    if (l32 == 0) out_idx[base + k] = blk;
  }
}

size_t align64(size_t n) { return (n + 63) & ~size_t(63); }
uint64_t tar_regions(uint64_t len) { return (len / kTarBlock + kRegionBlocks - 1) / kRegionBlocks; }

}  // namespace

size_t tar_scan_scratch_bytes(uint64_t len) {
  const uint64_t nreg = tar_regions(len);
  return 64 + align64(nreg * 8) + align64(nreg * 4) + nreg * kRegionBlocks + 64;
}

TarScanScratch tar_scan_scratch_layout(void* scratch, uint64_t len) {
  const uint64_t nreg = tar_regions(len);
  uint8_t* sp = static_cast<uint8_t*>(scratch);
  TarScanScratch sc;
  sc.total = reinterpret_cast<uint64_t*>(sp);
  sc.pad = reinterpret_cast<uint64_t*>(sp + 16);
  sp += 64;
  sc.region_base = reinterpret_cast<uint64_t*>(sp); sp += align64(nreg * 8);
  sc.region_n = reinterpret_cast<uint32_t*>(sp); sp += align64(nreg * 4);
  sc.marks = sp;
  return sc;
}

bool tar_scan_launch(const uint8_t* tar, uint64_t len, const TarScanScratch& sc, uint8_t* out_blocks,
                     uint64_t* out_idx, uint64_t cap_blocks, hipStream_t s, std::string* err) {
  const uint64_t nblocks = len / kTarBlock, nreg64 = tar_regions(len);
  if (nreg64 > 0xffffffffull / kWaves) { *err = "layer tar too large for the device walk"; return false; }
  const uint32_t nreg = static_cast<uint32_t>(nreg64);
  const uint32_t blocks = (nreg + kWaves - 1) / kWaves;
  if (hipMemsetAsync(sc.total, 0, tar_scan_scratch_bytes(len), s) != hipSuccess) {
    *err = std::string("device tar walk: ") + hipGetErrorString(hipGetLastError());
    return false;
  }
  if (nreg) {
    hipLaunchKernelGGL(tsg_tar_mark, dim3(blocks), dim3(256), 0, s, tar, nblocks, sc.marks);
    hipLaunchKernelGGL(tsg_tar_count, dim3((nreg + 255u) / 256u), dim3(256), 0, s, sc.marks, nreg, sc.region_n);
  }
  region_scan_launch(sc.region_n, nreg, sc.region_base, sc.total, sc.pad, s);
  if (nreg)
    hipLaunchKernelGGL(tsg_tar_compact, dim3(blocks), dim3(256), 0, s, tar, sc.marks, nreg, sc.region_base, sc.total,
                       out_blocks, out_idx, cap_blocks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("device tar walk launch: ") + hipGetErrorString(e); return false; }
  return true;
}

}  // namespace tsg
