// Device-side content preparation of a raw batch: the whole of Analyze's
// preparation (pkg/fanal/analyzer/secret/secret.go:103-150) as one stream
// compaction -- IsBinary on every file's head, binaries that are not allowed
// dropped, '\r' stripped from text, ExtractPrintableBytes for allowed binaries
// (prep.h states the per-byte rule and is the CPU model of this file) -- and
// its special case, the CR strip of a batch that is all text (SURVEY.md 8f
// row 1, secret.go:121; crstrip.h).  Neither moves a byte across a file
// boundary, so the batch's image is one stream compaction of the whole batch
// and a file's new start is the output position of its first input byte.
//
// Reduce / scan / compact over 64 KiB regions (one wave each, 1 KiB
// sub-tiles, lane l holds bytes [16l, 16l + 16)); a byte emits 0, 1 or 2:
//   tsg_prep_classify   kind[f] from the host's gate / allowed flags and the file's head
//   tsg_prep_first      per region, the first file that starts after its first byte
//   tsg_prep_pass<0>    bytes each region emits                         reads N
//   tsg_prep_scan       exclusive prefix; the total; the new start (0) of the
//                       files at byte 0; the 64 zero bytes behind the output
//   tsg_prep_pass<1>    the emitted bytes to their place, and the new start
//                       of every file starting in (region start, region end]   reads N, writes N'
// The CR strip runs tsg_cr_count and tsg_cr_compact in place of the two
// passes (no classify, no kinds: 52 VGPRs against 78, 8 waves per SIMD
// against 6, 0.67 ms against 0.76 ms on 1 GB of text in 40k files) and
// shares everything else.  HBM traffic 2N + N' (algorithmic
// N + N').  A single-pass decoupled look-back variant (32 KiB workgroup
// tiles, 512-tile window) was measured slower: 8.1 ms vs 6.1 ms for 10 GB
// (DESIGN.md 4.2).
//
// A sub-tile of text: the kept ("not '\r'") counts' wave prefix sum places
// each lane's bytes, and the sub-tile's output goes to HBM as aligned dwords
// through a per-wave LDS staging line (byte stores only at the two partial
// dwords at its ends, which neighbouring sub-tiles complete); a sub-tile
// that loses nothing and whose output is 16-byte aligned (every one before
// the batch's first '\r') is stored directly.  File boundaries between text
// (or empty) files change nothing.  Inside one allowed binary it is mask
// arithmetic on the 16 printable bits of a lane's word and 4 halo bits from
// each neighbour (the sub-tile's own halo comes from the previous and the
// prefetched next word, loaded only at region edges).  Only a sub-tile with a
// boundary next to a dropped or an allowed-binary file looks files up: each
// lane finds the file of its word's first byte by binary search and walks
// the file pieces of its 16 bytes.
#include "crstrip.h"
#include "prep_dev.h"

namespace tsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kSub = 1024;              // bytes per wave step (64 lanes x 16 B)
constexpr uint32_t kRegion = 64 * 1024;      // bytes per wave (one region)
constexpr uint32_t kWaves = 4;               // waves per workgroup
// A sub-tile emits its kept bytes and one '\n' per kept run that ends in it;
// such ends lie at least 5 bytes apart (<= 205), and the staging line starts
// at the output position's offset within a dword (<= 3).
constexpr uint32_t kStage = kSub + 256 + 16;

// bit k (k < 4): byte k of d is '\r'
__device__ __forceinline__ uint32_t cr_bits(uint32_t d) {
  const uint32_t x = d ^ 0x0d0d0d0du;
  const uint32_t z = ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x)) & 0x80808080u;
  return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

__device__ __forceinline__ uint32_t cr_mask16(v4u w) {
  return cr_bits(w.x) | (cr_bits(w.y) << 4) | (cr_bits(w.z) << 8) | (cr_bits(w.w) << 12);
}

// bit k (k < 4): byte k of d is printable (tab: 256 bits)
__device__ __forceinline__ uint32_t pr_bits(const uint32_t* tab, uint32_t d) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t b = (d >> (8 * k)) & 0xffu;
    m |= ((tab[b >> 5] >> (b & 31u)) & 1u) << k;
  }
  return m;
}

__device__ __forceinline__ uint32_t pr_mask16(const uint32_t* tab, v4u w) {
  return pr_bits(tab, w.x) | (pr_bits(tab, w.y) << 4) | (pr_bits(tab, w.z) << 8) | (pr_bits(tab, w.w) << 12);
}

// 16 bytes at p (a multiple of 16); *valid = mask of the bytes below `total`
// (nothing at or past it is read; the bytes not read are 0)
__device__ __forceinline__ v4u load16(const uint8_t* __restrict__ src, uint64_t p, uint64_t total, uint32_t* valid) {
  if (p + 16 <= total) {
    *valid = 0xffffu;
    return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(src + p));
  }
  uint32_t b[4] = {0, 0, 0, 0}, v = 0;
  for (uint32_t k = 0; k < 16 && p + k < total; ++k) {
    b[k >> 2] |= static_cast<uint32_t>(src[p + k]) << ((k & 3) * 8);
    v |= 1u << k;
  }
  *valid = v;
  return v4u{b[0], b[1], b[2], b[3]};
}

// 16 lanes per file: the file's head is at most 300 bytes, so at most 20
// aligned 16-byte words; lane `sub` of the group takes words sub and sub + 16.
__global__ __launch_bounds__(256) void tsg_prep_classify(const uint8_t* __restrict__ src, uint64_t total,
                                                         const uint64_t* __restrict__ offsets, uint32_t nfiles,
                                                         const uint8_t* __restrict__ flags,
                                                         uint8_t* __restrict__ kinds) {
  const uint32_t f = blockIdx.x * 16u + (threadIdx.x >> 4), sub = threadIdx.x & 15u, lane = threadIdx.x & 63u;
  bool trig = false;
  uint32_t fl = 0;
  if (f < nfiles) {
    fl = flags[f];
    if (fl & kPrepGate) {
      const uint64_t b = offsets[f];
      const uint64_t e = min(min(offsets[f + 1], b + kPrepHead), total);
      const uint64_t a0 = b & ~15ull;
      for (uint32_t k = sub; k < 20; k += 16) {
        const uint64_t p = a0 + 16ull * k;
        if (p >= e) break;
        uint32_t valid;
        const v4u w = load16(src, p, total, &valid);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
          const uint64_t pos = p + j;
          if (pos >= b && pos < e) trig |= prep_trigger((ws[j >> 2] >> ((j & 3) * 8)) & 0xffu);
        }
      }
    }
  }
  const uint64_t bal = __ballot(trig);                       // whole waves get here
  const bool binary = ((bal >> (lane & 48u)) & 0xffffull) != 0;
  if (f < nfiles && sub == 0)
    kinds[f] = !(fl & kPrepGate) ? kPrepDropped : !binary ? kPrepText : (fl & kPrepAllowed) ? kPrepPrintable
                                                                                             : kPrepDropped;
}

// first[r] = the first file whose start is > r * kRegion (file f - 1 holds
// that byte): files f with offsets[f - 1] <= r * kRegion < offsets[f]
__global__ __launch_bounds__(256) void tsg_prep_first(const uint64_t* __restrict__ offsets, uint32_t nfiles,
                                                      uint32_t nregions, uint32_t* __restrict__ first) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f == 0 || f > nfiles || offsets[f] == 0) return;
  const uint64_t rb = (offsets[f - 1] + kRegion - 1) / kRegion;
  const uint64_t re = (offsets[f] - 1) / kRegion;
  for (uint64_t r = rb; r <= re && r < nregions; ++r) first[r] = f;
}

// One workgroup: region_base[r] = bytes emitted before region r; the total;
// new_off of the files that start at byte 0 (every file of an empty batch);
// the 64 zero bytes behind the prepared bytes, when they fit (the CR strip
// gives no dst: it writes no pad).  Each thread sums a contiguous run of
// regions with its loads issued in groups of 8 (a one-at-a-time loop waits
// one L2 round trip per region: 0.29 ms for 10 GB).
__global__ __launch_bounds__(1024) void tsg_prep_scan(const uint32_t* __restrict__ region_n, uint32_t nregions,
                                                      uint64_t* __restrict__ region_base,
                                                      const uint64_t* __restrict__ offsets, uint32_t nfiles,
                                                      uint64_t* __restrict__ new_off, uint64_t* __restrict__ out_total,
                                                      uint8_t* __restrict__ dst, uint64_t dst_cap) {
  __shared__ uint64_t part[1024];
  __shared__ uint32_t s_ub;
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nregions + 1023u) / 1024u;
  const uint32_t b = min(nregions, t * per), e = min(nregions, b + per);
  uint64_t s = 0;
  uint32_t i = b;
  for (; i + 8 <= e; i += 8) {
    uint32_t v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = region_n[i + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  for (; i < e; ++i) s += region_n[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint64_t run = part[t] - s;
  for (i = b; i + 8 <= e; i += 8) {
    uint32_t v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = region_n[i + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      region_base[i + q] = run;
      run += v[q];
    }
  }
  for (; i < e; ++i) {
    region_base[i] = run;
    run += region_n[i];
  }
  const uint64_t prepared = part[1023];
  if (t == 0) {
    uint32_t lo = 0, hi = nfiles + 1;        // the first file that starts after byte 0
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (offsets[mid] > 0) hi = mid; else lo = mid + 1;
    }
    s_ub = lo;
    *out_total = prepared;
  }
  __syncthreads();
  for (uint32_t k = t; k < s_ub; k += 1024) new_off[k] = 0;
  if (t < 64 && prepared + 64 <= dst_cap) dst[prepared + t] = 0;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// Bytes that region [r0, r0 + kRegion) emits as text (in every lane)
__device__ __forceinline__ uint32_t text_region_count(const uint8_t* __restrict__ src, uint64_t r0, uint64_t total,
                                                      uint32_t lane) {
  uint32_t n = 0;
#pragma unroll 8
  for (uint32_t j = 0; j < kRegion / kSub; ++j) {
    uint32_t valid;
    const v4u w = load16(src, r0 + j * kSub + lane * 16u, total, &valid);
    n += __popc(valid & ~cr_mask16(w));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  return n;
}

// The bytes of w that `keep` names, to the staging line from lb[q] on
__device__ __forceinline__ void stage_kept(uint8_t* lb, uint32_t q, v4u w, uint32_t keep) {
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if ((keep >> b) & 1u) {
      lb[q] = static_cast<uint8_t>(ws[b >> 2] >> ((b & 3) * 8));
      ++q;
    }
  }
}

// The wave's staging line (stage byte q holds output byte out - q0 + q, q0 =
// out & 3) to dst[out, out + K): aligned dwords, bytes at the two ragged ends
__device__ __forceinline__ void flush_stage(const uint8_t* lb, uint8_t* __restrict__ dst, uint64_t out, uint32_t q0,
                                            uint32_t K, uint32_t lane) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint64_t a0 = out - q0, e = out + K;
  const uint32_t ndw = static_cast<uint32_t>((e - a0 + 3) >> 2);
  for (uint32_t d = lane; d < ndw; d += 64) {
    const uint64_t g = a0 + 4ull * d;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(lb + 4 * d);
    if (g >= out && g + 4 <= e) {
      *reinterpret_cast<uint32_t*>(dst + g) = v;
    } else {
      for (uint32_t b = 0; b < 4; ++b)
        if (g + b >= out && g + b < e) dst[g + b] = static_cast<uint8_t>(v >> (8 * b));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The files that start in (s0, s1] of a sub-tile at s0 whose output starts at
// `out` (excl, keep, nl: each lane's; K: the sub-tile's bytes): new start =
// output position of their first byte, out + K for a file at s0 + kSub.
// *nf = the first file that starts after s0, *next_start its start; both
// move past the files taken.
template <bool kWrite>
__device__ __forceinline__ void file_starts(const uint64_t* __restrict__ offsets, uint32_t nfiles, uint64_t s0,
                                            uint64_t s1, uint64_t out, uint32_t excl, uint32_t keep, uint32_t nl,
                                            uint32_t K, uint32_t lane, uint32_t* nf, uint64_t* next_start,
                                            uint64_t* __restrict__ new_off) {
  while (*next_start <= s1) {
    const uint32_t idx = *nf + lane;
    const uint64_t o = idx <= nfiles ? offsets[idx] : ~0ull;
    const bool in = o <= s1;                // o > s0: files are sorted and nf is past the earlier ones
    if (kWrite) {
      const uint32_t rel = in ? static_cast<uint32_t>(o - s0) : 0u;
      const bool inside = rel < kSub;
      const uint32_t wi = inside ? rel >> 4 : 0u;
      const uint32_t pe = __shfl(excl, wi), pk = __shfl(keep, wi), pn = __shfl(nl, wi);
      const uint32_t below = (1u << (rel & 15u)) - 1u;
      if (in) new_off[idx] = inside ? out + pe + __popc(pk & below) + __popc(pn & below) : out + K;
    }
    *nf += static_cast<uint32_t>(__popcll(__ballot(in)));
    *next_start = *nf <= nfiles ? offsets[*nf] : ~0ull;
  }
}

// The CR strip's passes: every file is text, so there are no kinds and no
// file lookups.  region_n[r] = bytes region r keeps.
__global__ __launch_bounds__(256) void tsg_cr_count(const uint8_t* __restrict__ src, uint64_t total, uint32_t nregions,
                                                    uint32_t* __restrict__ region_n) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (r >= nregions) return;
  const uint32_t n = text_region_count(src, static_cast<uint64_t>(r) * kRegion, total, lane);
  if (lane == 0) region_n[r] = n;
}

// The kept bytes to dst from region_base[r] on, and new_off of the files that
// start in (r0, r1].
__global__ __launch_bounds__(256) void tsg_cr_compact(const uint8_t* __restrict__ src, uint64_t total,
                                                      uint32_t nregions, const uint64_t* __restrict__ region_base,
                                                      const uint32_t* __restrict__ first,
                                                      const uint64_t* __restrict__ offsets, uint32_t nfiles,
                                                      uint8_t* __restrict__ dst, uint64_t* __restrict__ new_off) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][kSub + 16];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x * kWaves + wv;
  if (r >= nregions) return;                 // whole waves only; no workgroup barrier below
  uint8_t* lb = stage[wv];
  const uint64_t r0 = static_cast<uint64_t>(r) * kRegion;
  const uint64_t r1 = min(r0 + kRegion, total);
  uint64_t out = region_base[r];
  uint32_t nf = first[r];                    // wave-uniform: the first file that starts after the sub-tile's first byte
  uint64_t next_start = offsets[nf];
  uint32_t valid_n;
  v4u wn = load16(src, r0 + lane * 16u, total, &valid_n);
  for (uint64_t s0 = r0; s0 < r1; s0 += kSub) {
    const v4u w = wn;
    const uint32_t valid = valid_n;
    if (s0 + kSub < r1) wn = load16(src, s0 + kSub + lane * 16u, total, &valid_n);   // next sub-tile in flight
    const uint32_t keep = valid & ~cr_mask16(w);
    const uint32_t k = __popc(keep);
    const uint32_t incl = wave_incl_scan(k, lane);
    const uint32_t excl = incl - k;
    const uint32_t K = __shfl(incl, 63);
    const bool plain = __ballot(keep != 0xffffu) == 0;   // full sub-tile without '\r'
    if (plain && (out & 15u) == 0) {
      __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(dst + out + lane * 16u));
    } else if (K) {
      const uint32_t q0 = static_cast<uint32_t>(out & 3u);
      if (plain && q0 == 0) *reinterpret_cast<v4u*>(lb + lane * 16u) = w;
      else stage_kept(lb, q0 + excl, w, keep);
      flush_stage(lb, dst, out, q0, K, lane);
    }
    file_starts<true>(offsets, nfiles, s0, min(s0 + kSub, r1), out, excl, keep, 0u, K, lane, &nf, &next_start, new_off);
    out += K;
  }
}

// The 16 bytes at p taken as bytes of a file [fs, fe) of kind kd: bit b of
// *keep = byte p + b is emitted, of *nl = a '\n' follows it.  P24: printable
// bits of the bytes p - 4 ... p + 19 (bit j = byte p - 4 + j), cr: the '\r'
// bits of the 16.  The caller masks the result to the bytes that are the file's.
__device__ __forceinline__ void file_masks(uint32_t kd, uint32_t P24, uint32_t cr, uint64_t p, uint64_t fs, uint64_t fe,
                                           uint32_t* keep, uint32_t* nl) {
  if (kd == kPrepText) { *keep = ~cr & 0xffffu; *nl = 0; return; }
  if (kd != kPrepPrintable) { *keep = 0; *nl = 0; return; }
  const int64_t base = static_cast<int64_t>(p) - 4;
  int64_t lo = static_cast<int64_t>(fs) - base, hi = static_cast<int64_t>(fe) - base;
  lo = lo < 0 ? 0 : lo > 24 ? 24 : lo;
  hi = hi < 0 ? 0 : hi > 24 ? 24 : hi;
  const uint32_t in_file = hi > lo ? ((1u << (hi - lo)) - 1u) << lo : 0u;   // hi - lo <= 24
  const uint32_t P = P24 & in_file;
  const uint32_t R = P & (P >> 1) & (P >> 2) & (P >> 3) & (P >> 4);          // bit j: bytes j ... j + 4 all printable
  const uint32_t K = R | (R << 1) | (R << 2) | (R << 3) | (R << 4);          // bit j: some such window holds byte j
  *keep = (K >> 4) & 0xffffu;
  *nl = *keep & ~(P >> 5) & 0xffffu;
}

// kWrite false: region_n[r] = bytes region r emits.  kWrite true: the bytes go
// to dst from region_base[r] on (nothing is written when the prepared bytes
// and their 64-byte pad do not fit dst_cap), and new_off of the files that
// start in (r0, r1].
template <bool kWrite>
__global__ __launch_bounds__(256) void tsg_prep_pass(const uint8_t* __restrict__ src, uint64_t total, uint32_t nregions,
                                                     const uint32_t* __restrict__ print_tab,
                                                     const uint32_t* __restrict__ first,
                                                     const uint64_t* __restrict__ offsets, uint32_t nfiles,
                                                     const uint8_t* __restrict__ kinds,
                                                     uint32_t* __restrict__ region_n,
                                                     const uint64_t* __restrict__ region_base,
                                                     const uint64_t* __restrict__ prepared_total,
                                                     uint8_t* __restrict__ dst, uint64_t dst_cap,
                                                     uint64_t* __restrict__ new_off) {
  __shared__ uint32_t tab[8];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWrite ? kWaves : 1][kStage];
  if (threadIdx.x < 8) tab[threadIdx.x] = print_tab[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x * kWaves + wv;
  if (r >= nregions) return;                 // whole waves only; no workgroup barrier below
  if (kWrite && *prepared_total + 64 > dst_cap) return;
  uint8_t* lb = stage[kWrite ? wv : 0];
  const uint64_t r0 = static_cast<uint64_t>(r) * kRegion;
  const uint64_t r1 = min(r0 + kRegion, total);
  // wave-uniform file state: nf = the first file that starts after the
  // sub-tile's first byte, so file kf = nf - 1 (kind kd, start fs) holds that byte
  uint32_t nf = first[r];
  uint64_t next_start = offsets[nf];
  uint32_t kf = nf - 1;
  uint32_t kd = kinds[kf];
  uint64_t fs = offsets[kf];
  if (!kWrite && next_start >= r1 && kd == kPrepText) {      // the region lies in one text file
    const uint32_t n = text_region_count(src, r0, total, lane);
    if (lane == 0) region_n[r] = n;
    return;
  }
  uint64_t out = kWrite ? region_base[r] : 0;
  uint32_t cnt = 0;
  uint32_t valid_n;
  v4u wn = load16(src, r0 + lane * 16u, total, &valid_n);
  uint32_t pw = 0;                            // the previous sub-tile's last dword of each lane
  for (uint64_t s0 = r0; s0 < r1; s0 += kSub) {
    const v4u w = wn;
    const uint32_t valid = valid_n;
    const bool more = s0 + kSub < r1;
    if (more) wn = load16(src, s0 + kSub + lane * 16u, total, &valid_n);   // next sub-tile in flight
    const uint64_t s1 = min(s0 + kSub, r1);
    const uint64_t p = s0 + lane * 16u;
    const bool uniform = next_start >= s1;    // no file starts inside the sub-tile
    uint32_t keep = 0, nl = 0;
    // File boundaries between text files change nothing: when file kf and
    // the (at most 63) files that start inside the sub-tile are all text or
    // empty, it is the CR strip's sub-tile whatever the boundaries.
    bool all_text = false;
    if (!uniform) {
      const uint32_t idx = kf + lane;
      bool other = false;
      if (idx < nfiles && (lane == 0 || offsets[idx] < s1))
        other = kinds[idx] != kPrepText && offsets[idx + 1] != offsets[idx];
      const bool more_files = kf + 64 <= nfiles && offsets[kf + 64] < s1;
      all_text = __ballot(other) == 0 && !more_files;
    }
    if (all_text || (uniform && kd != kPrepPrintable)) {
      if (all_text || kd == kPrepText) keep = valid & ~cr_mask16(w);
    } else {
      const uint32_t P16 = pr_mask16(tab, w) & valid;
      // the sub-tile's halo: 4 bytes before it and 4 behind it
      uint32_t hl = 0, hr = 0;
      if (s0 > r0) hl = pr_bits(tab, __shfl(pw, 63));
      else if (r0 > 0) hl = pr_bits(tab, *reinterpret_cast<const uint32_t*>(src + r0 - 4));
      if (more) {
        hr = pr_bits(tab, __shfl(wn.x, 0)) & __shfl(valid_n, 0) & 15u;
      } else {
        uint32_t d = 0;
        for (uint32_t k = 0; k < 4 && s0 + kSub + k < total; ++k)
          d |= static_cast<uint32_t>(src[s0 + kSub + k]) << (8 * k);
        hr = pr_bits(tab, d);
        for (uint32_t k = 0; k < 4; ++k) if (s0 + kSub + k >= total) hr &= ~(1u << k);
      }
      const uint32_t up = __shfl_up(P16, 1), dn = __shfl_down(P16, 1);
      const uint32_t P24 = (lane ? up >> 12 : hl) | (P16 << 4) | ((lane < 63 ? dn & 15u : hr) << 20);
      const uint32_t cr = cr_mask16(w);
      if (uniform) {
        file_masks(kd, P24, cr, p, fs, next_start, &keep, &nl);
        keep &= valid;
        nl &= valid;
      } else {
        uint64_t pos = p;
        const uint64_t end = min(p + 16, s1);
        if (pos < end) {
          uint32_t lo = nf, hi = nfiles;      // the first file that starts after byte p (offsets[nfiles] = total > p)
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (offsets[mid] > p) hi = mid; else lo = mid + 1;
          }
          uint32_t f = lo - 1;
          while (pos < end) {
            uint64_t fe = offsets[f + 1];
            while (fe <= pos) { ++f; fe = offsets[f + 1]; }   // ends below total: pos < total = offsets[nfiles]
            const uint64_t se = min(fe, end);
            const uint32_t bits = ((1u << (se - p)) - 1u) & ~((1u << (pos - p)) - 1u);
            uint32_t k, n;
            file_masks(kinds[f], P24, cr, p, offsets[f], fe, &k, &n);
            keep |= k & bits;
            nl |= n & bits;
            pos = se;
          }
        }
      }
    }
    pw = w.w;
    const uint32_t k = __popc(keep) + __popc(nl);
    uint32_t excl = 0, K = 0;
    if (!kWrite) {
      cnt += k;
    } else {
      const uint32_t incl = wave_incl_scan(k, lane);
      excl = incl - k;
      K = __shfl(incl, 63);
      const bool plain = __ballot(keep != 0xffffu || nl != 0) == 0;   // full sub-tile, nothing removed or added
      if (plain && (out & 15u) == 0) {
        __builtin_nontemporal_store(w, reinterpret_cast<v4u*>(dst + out + lane * 16u));
      } else if (K) {
        const uint32_t q0 = static_cast<uint32_t>(out & 3u);   // stage byte q holds output byte (out & ~3) + q
        if (plain && q0 == 0) {
          *reinterpret_cast<v4u*>(lb + lane * 16u) = w;
        } else {
          uint32_t q = q0 + excl;
          if (nl == 0) {
            stage_kept(lb, q, w, keep);
          } else {
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
              if ((keep >> b) & 1u) {
                lb[q] = static_cast<uint8_t>(ws[b >> 2] >> ((b & 3) * 8));
                ++q;
              }
              if ((nl >> b) & 1u) {
                lb[q] = '\n';
                ++q;
              }
            }
          }
        }
        flush_stage(lb, dst, out, q0, K, lane);
      }
    }
    file_starts<kWrite>(offsets, nfiles, s0, s1, out, excl, keep, nl, K, lane, &nf, &next_start, new_off);
    if (nf - 1 != kf && nf <= nfiles) {
      kf = nf - 1;
      kd = kinds[kf];
      fs = offsets[kf];
    }
    out += K;
  }
  if (!kWrite) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) region_n[r] = cnt;
  }
}

uint64_t prep_regions(uint64_t total) { return (total + kRegion - 1) / kRegion; }
size_t align64(size_t n) { return (n + 63) & ~size_t(63); }

}  // namespace

size_t cr_strip_scratch_bytes(uint64_t total) { return 64 + prep_regions(total) * (8 + 4 + 4) + 64; }

bool cr_strip_launch(const uint8_t* src, const uint64_t* offsets, uint32_t nfiles, uint64_t total, uint8_t* dst,
                     uint64_t* new_off, void* scratch, hipStream_t s, std::string* err) {
  const uint64_t nreg64 = prep_regions(total);
  if (nreg64 > 0xffffffffull / kWaves) { *err = "batch too large for the CR strip"; return false; }
  const uint32_t nreg = static_cast<uint32_t>(nreg64);
  uint8_t* sp = static_cast<uint8_t*>(scratch);
  uint64_t* d_total = reinterpret_cast<uint64_t*>(sp);
  uint64_t* region_base = reinterpret_cast<uint64_t*>(sp + 64);
  uint32_t* region_n = reinterpret_cast<uint32_t*>(sp + 64 + 8 * nreg64);
  uint32_t* first = region_n + nreg64;
  const uint32_t blocks = (nreg + kWaves - 1) / kWaves;
  if (nreg) {
    hipLaunchKernelGGL(tsg_prep_first, dim3(nfiles / 256u + 1u), dim3(256), 0, s, offsets, nfiles, nreg, first);
    hipLaunchKernelGGL(tsg_cr_count, dim3(blocks), dim3(256), 0, s, src, total, nreg, region_n);
  }
  hipLaunchKernelGGL(tsg_prep_scan, dim3(1), dim3(1024), 0, s, region_n, nreg, region_base, offsets, nfiles, new_off,
                     d_total, static_cast<uint8_t*>(nullptr), uint64_t(0));
  if (nreg)
    hipLaunchKernelGGL(tsg_cr_compact, dim3(blocks), dim3(256), 0, s, src, total, nreg, region_base, first, offsets,
                       nfiles, dst, new_off);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *err = std::string("CR strip launch: ") + hipGetErrorString(e); return false; }
  return true;
}

void region_scan_launch(const uint32_t* region_n, uint32_t nregions, uint64_t* region_base, uint64_t* total,
                        uint64_t* pad, hipStream_t s) {
  hipLaunchKernelGGL(tsg_prep_scan, dim3(1), dim3(1024), 0, s, region_n, nregions, region_base, pad, 0u, pad + 1, total,
                     static_cast<uint8_t*>(nullptr), uint64_t(0));
}

size_t prep_scratch_bytes(uint64_t total, uint32_t nfiles) {
  const uint64_t nreg = prep_regions(total), nf1 = static_cast<uint64_t>(nfiles) + 1;
  return 128 + align64(nf1 * 8) * 2 + align64(nreg * 8) + align64(nreg * 4) * 2 + align64(nfiles) * 2 + 64;
}

PrepScratch prep_scratch_layout(void* scratch, uint64_t total, uint32_t nfiles) {
  const uint64_t nreg = prep_regions(total), nf1 = static_cast<uint64_t>(nfiles) + 1;
  uint8_t* sp = static_cast<uint8_t*>(scratch);
  PrepScratch sc;
  sc.total = reinterpret_cast<uint64_t*>(sp);
  sc.print_tab = reinterpret_cast<uint32_t*>(sp + 64);
  sp += 128;
  sc.offsets = reinterpret_cast<uint64_t*>(sp); sp += align64(nf1 * 8);
  sc.new_off = reinterpret_cast<uint64_t*>(sp); sp += align64(nf1 * 8);
  sc.region_base = reinterpret_cast<uint64_t*>(sp); sp += align64(nreg * 8);
  sc.region_n = reinterpret_cast<uint32_t*>(sp); sp += align64(nreg * 4);
  sc.first = reinterpret_cast<uint32_t*>(sp); sp += align64(nreg * 4);
  sc.flags = sp; sp += align64(nfiles);
  sc.kinds = sp;
  return sc;
}

bool prep_launch(const uint8_t* src, uint64_t total, uint32_t nfiles, uint8_t* dst, uint64_t dst_cap,
                 const PrepScratch& sc, hipStream_t s, hipEvent_t* pass_ev, std::string* err) {
  const uint64_t nreg64 = prep_regions(total);
  if (nreg64 > 0xffffffffull / kWaves) { *err = "batch too large for the device preparation"; return false; }
  const uint32_t nreg = static_cast<uint32_t>(nreg64);
  const uint32_t blocks = (nreg + kWaves - 1) / kWaves;
  auto mark = [&](int i) { return !pass_ev || hipEventRecord(pass_ev[i], s) == hipSuccess; };
  bool ok = mark(0);
  if (nfiles)
    hipLaunchKernelGGL(tsg_prep_classify, dim3((nfiles + 15u) / 16u), dim3(256), 0, s, src, total, sc.offsets, nfiles,
                       sc.flags, sc.kinds);
  ok = mark(1) && ok;
  if (nreg) {
    hipLaunchKernelGGL(tsg_prep_first, dim3(nfiles / 256u + 1u), dim3(256), 0, s, sc.offsets, nfiles, nreg, sc.first);
    hipLaunchKernelGGL(tsg_prep_pass<false>, dim3(blocks), dim3(256), 0, s, src, total, nreg, sc.print_tab, sc.first,
                       sc.offsets, nfiles, sc.kinds, sc.region_n, sc.region_base, sc.total, dst, dst_cap, sc.new_off);
  }
  ok = mark(2) && ok;
  hipLaunchKernelGGL(tsg_prep_scan, dim3(1), dim3(1024), 0, s, sc.region_n, nreg, sc.region_base, sc.offsets, nfiles,
                     sc.new_off, sc.total, dst, dst_cap);
  ok = mark(3) && ok;
  if (nreg)
    hipLaunchKernelGGL(tsg_prep_pass<true>, dim3(blocks), dim3(256), 0, s, src, total, nreg, sc.print_tab, sc.first,
                       sc.offsets, nfiles, sc.kinds, sc.region_n, sc.region_base, sc.total, dst, dst_cap, sc.new_off);
  ok = mark(4) && ok;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !ok) { *err = std::string("device preparation launch: ") + hipGetErrorString(e); return false; }
  return true;
}

}  // namespace tsg
