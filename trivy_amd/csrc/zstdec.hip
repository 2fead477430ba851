// Device side of the zstd decode: a batch of zstd streams in device memory
// decoded there, one wavefront per stream, and the XXH64 of every frame they
// wrote.  zstdec.h states the format rules and holds the decoder itself
// (zstd_decode), which this file runs through WaveIo; zstd_model is the CPU
// model of the whole pass.
//
//   tsg_zstd_streams      one workgroup of one wave per stream, workgroup k
//                         taking the k-th longest stream (the dispatcher starts
//                         workgroups in order, so the long ones start first)
//   tsg_zstd_hash_frames  one thread per frame that carries a checksum: XXH64
//                         is one serial chain per frame (it does not fold across
//                         slices the way CRC32 does), read 128 bytes at a time
//                         so that sixteen loads are in flight per step
//
// A frame is one dependent chain: every lane of the wave runs the decoder on
// the same values (table entries and input bytes pass through readfirstlane,
// so the chain lives in scalar registers and its branches are scalar), lane 0
// alone stores to the tables, and the lanes do what has width: the four
// Huffman literal streams of a block (lane k decodes stream k: its own
// backward bit reader over its own bytes of d_z, its own quarter of the
// literals), the refill of the input window, the literal copy, the match copy
// and the stores to HBM.
//
// Per-wave LDS (46.5 KiB, three waves per CU):
//   win   32 KiB   the newest output at win[pos & 32767]: the near history a
//                  match reads and the token buffer at once
//   inw    2 KiB   the input window, 16-byte aligned in d_z, placed to start at
//                  the byte asked for (forward reads) or to end behind it
//                  (the backward bitstreams); a chunk is loaded only when it
//                  starts below the stream's end, so at most 15 bytes past the
//                  stream are touched, and the decoder never asks for a byte
//                  at or past the end
//   t   12.3 KiB   the LL / ML / OF tables (512 / 512 / 256 entries), the
//                  Huffman table (2^11 entries), the weights and their FSE
//                  table, the counts of a table description
//   stage  2 KiB   the part of the literal scratch the sequences are taking
//                  their literals from
// A block's Huffman-decoded literals (up to 128 KiB) do not fit: they go to the
// stream's 128 KiB of literal scratch in HBM and come back 2 KiB at a time
// (one trip to L2 per 2 KiB, not one per sequence).  Raw literals are read
// from d_z where they lie; RLE literals are one byte.
//
// Output enters the ring in chunks of at most kChunk = 4 KiB, and after every
// chunk the whole 16-byte units below op go to HBM once kFlushAt = 8 KiB are
// pending (the slot starts 16-byte aligned, so unit and ring index are aligned
// alike); the rest goes byte by byte at the end.  Every store lies below
// op <= the slot's capacity.  So at the start of a chunk at p:
//   (a) fewer than kFlushAt + 16 bytes are pending, p - flushed < 8208;
//   (b) the chunk overwrites the ring cells of [p - 32768, p + c - 32768), all
//       below p - kZsNear (kZsNear = 32768 - kChunk) and so, by (a), flushed.
//
// The match copy.  A source byte at distance d = p - src from the chunk's
// start is read from the ring when d <= kZsNear -- its cell is overwritten
// only by the byte 32768 further on, at or past p + kChunk, not in this chunk
// -- and from the slot in HBM otherwise: by (a) src < p - kZsNear < flushed.
// (The ring could serve up to 32768 - c; the fixed kZsNear keeps the rule one
// comparison.)  Lane i writes byte p + i from source p - off + i % off, which
// precedes p: no lane reads what another writes in the same chunk, and a long
// match walks from HBM into the ring byte by byte without a seam.
//
// Visibility of the wave's own stores to its far loads:
//   * they wait for them: store_units and the Huffman literal stores end with
//     s_waitcnt vmcnt(0), so no store of this wave is outstanding when a later
//     load issues (on gfx950 a store counts in vmcnt until L2 has taken it);
//   * they never return a stale L1 line: the vector L1 may hold a line this
//     wave fetched before all its bytes were stored (a far match reads a line
//     the flush had only half filled, or the scratch line of the previous
//     block's literals).  The far loads and the loads that stage the scratch are therefore
//     relaxed agent-scope atomic loads, which compile to global_load ... sc1
//     and are served by L2 past the L1 (on gfx950 an sc1 load bypasses the L1
//     only and is 0-3 % slower than a plain one).  An acquire fence per far
//     match would invalidate the whole L1, the input lines included, at
//     several hundred cycles a time; the sc1 load costs nothing when no far
//     byte is read.  All stores are plain vector stores, which write through
//     to this XCD's L2, the one the loads are served from.
//
// Ordering inside the wave: LDS operations of one wave execute in program
// order, so lane 0's stores are what the next instruction's loads of the other
// lanes see; the wavefront-scope fence + wave barrier (WaveIo::sync) keeps the
// compiler from moving an access across that point (tarscan.hip's idiom).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "zstdec_dev.h"

namespace tsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
// Pointers that say where they point: the accesses compile to global_ and ds_
// instructions, never flat_, wherever the compiler keeps the WaveIo
#define TSG_ZS_GLOBAL __attribute__((address_space(1)))
#define TSG_ZS_LDS __attribute__((address_space(3)))
typedef TSG_ZS_GLOBAL const uint8_t* gcbytes;
typedef TSG_ZS_GLOBAL uint8_t* gbytes;
typedef TSG_ZS_LDS uint8_t* lbytes;

constexpr uint32_t kRing = 32768;
constexpr uint32_t kRingMask = kRing - 1;
constexpr uint32_t kChunk = 4096;                // output bytes that enter the ring between two flush checks
constexpr uint32_t kInWin = 2048;                // input window bytes: 64 lanes x 2 x 16
constexpr uint32_t kFlushAt = 8192;              // pending output that triggers a store to HBM
constexpr uint32_t kStage = 2048;                // literal scratch bytes staged in LDS: 64 lanes x 4 x 8
constexpr uint32_t kRecFirst = 16;               // frame records per stream in the first launch
constexpr uint32_t kNoStage = 0x80000000u;       // no literal index is within kStage of it
static_assert(kZsNear == kRing - kChunk, "zstdec.h's model counts far matches by the same distance");
static_assert(kFlushAt + 16 <= kZsNear, "what the ring no longer serves has been flushed");

struct ZsStream {                                // one stream's place, all offsets in bytes
  uint64_t z_begin, z_end;                       // in d_z
  uint64_t dst_begin, dst_cap;                   // in d_dst
  uint64_t rec_begin;                            // first frame record
  uint32_t rec_cap, pad;
};
struct ZsResult {
  uint64_t out_len;
  int32_t status;
  uint32_t nrecs, nblocks, pad;
};
struct HashDesc {
  uint64_t begin, len;                           // in d_dst
};

struct WaveLds {
  uint8_t win[kRing];
  uint8_t inw[kInWin];
  uint8_t stage[kStage];
  ZsTables t;
};
static_assert(sizeof(WaveLds) < 65536, "one wave's LDS");

// a byte this wave may have stored since the line was last fetched: past the L1
__device__ __forceinline__ uint32_t load_fresh(gbytes p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the input window from d_z[wa, wa + kInWin): out of line, it has many callers
__device__ __noinline__ void load_window(gcbytes z, uint64_t g1, lbytes inw, uint32_t lane, uint64_t wa) {
#pragma unroll
  for (uint32_t c = 0; c < kInWin / 16 / 64; ++c) {
    const uint32_t k = 16u * (lane + 64u * c);
    v4u w = {0u, 0u, 0u, 0u};
    if (wa + k < g1) w = *reinterpret_cast<TSG_ZS_GLOBAL const v4u*>(z + wa + k);
    *reinterpret_cast<TSG_ZS_LDS v4u*>(inw + k) = w;
  }
}

struct WaveIo {
  gcbytes z;                                     // d_z, 16-byte aligned
  uint64_t g0, g1;                               // the stream in d_z
  gbytes out;                                    // the slot, 16-byte aligned
  gbytes lits;                                   // the stream's kZsBlockMax bytes of literal scratch
  ZsFrameRec* recs;
  lbytes win;
  lbytes inw;
  lbytes stage;
  uint32_t lane;
  uint64_t wa = 0;                               // the input window's start in d_z (16-byte aligned)
  uint64_t flushed = 0;                          // output below it is in HBM; a multiple of 16 until the end
  uint32_t sb = kNoStage;                        // stage holds the literal scratch [sb, sb + kStage); a multiple of 8

  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void note(uint32_t) {}
  __device__ __forceinline__ void seq_note(uint64_t, uint32_t, uint32_t) {}

  // ---- input ----
  __device__ __forceinline__ void refill(uint64_t a) {            // a 16-byte aligned
    wa = a;
    sync();
    load_window(z, g1, inw, lane, a);
    sync();
  }
  __device__ __forceinline__ uint32_t in(uint64_t pos) {          // pos < the stream's length
    const uint64_t a = g0 + pos;
    if (a - wa >= kInWin) refill(a & ~uint64_t(15));
    return TSG_ZS_UNIFORM(inw[a - wa]);
  }
  __device__ __forceinline__ uint32_t in_back(uint64_t pos) {     // the same byte; the window ends behind it
    const uint64_t a = g0 + pos;
    if (a - wa >= kInWin) {
      const uint64_t e = (a & ~uint64_t(15)) + 16u;
      refill(e > kInWin ? e - kInWin : 0u);
    }
    return TSG_ZS_UNIFORM(inw[a - wa]);
  }
  __device__ __forceinline__ uint32_t in_back32(uint64_t pos) {   // bytes pos .. pos + 3, all below the stream's length
    const uint64_t a = g0 + pos;
    if (a - wa > kInWin - 4) return in_back(pos) | in_back(pos + 1) << 8 | in_back(pos + 2) << 16 | in_back(pos + 3) << 24;
    const uint32_t k = static_cast<uint32_t>(a - wa);
    return TSG_ZS_UNIFORM(inw[k] | inw[k + 1] << 8 | inw[k + 2] << 16 | inw[k + 3] << 24);
  }
  __device__ __forceinline__ uint32_t in_lane(uint64_t pos) { return z[g0 + pos]; }   // a lane's own byte, pos < the stream's length
  __device__ __forceinline__ uint32_t in_lane32(uint64_t pos) {
    gcbytes p = z + g0 + pos;
    return p[0] | p[1] << 8 | p[2] << 16 | static_cast<uint32_t>(p[3]) << 24;
  }

  // ---- literals ----
  __device__ __forceinline__ void lit_put(uint32_t k, uint32_t b) { lits[k] = static_cast<uint8_t>(b); }   // k < kZsBlockMax
  template <class F>
  __device__ __forceinline__ bool huf_run(uint32_t n, F f) {
    sync();
    sb = kNoStage;                               // the scratch is about to change
    bool ok = true;
    if (lane < n) ok = f(lane);
    drain_stores();
    sync();
    return __all(ok ? 1 : 0) != 0;
  }

  // ---- output ----
  // the whole 16-byte units of [flushed, e) to HBM; e a multiple of 16, e - flushed < 32 KiB
  __device__ __forceinline__ void store_units(uint64_t e) {
    sync();
    for (uint64_t p = flushed + 16u * lane; p < e; p += 16u * 64u)
      *reinterpret_cast<TSG_ZS_GLOBAL v4u*>(out + p) = *reinterpret_cast<TSG_ZS_LDS const v4u*>(win + (p & kRingMask));
    drain_stores();
    flushed = e;
  }
  __device__ __forceinline__ void advance(uint64_t op) {          // op = output bytes so far
    sync();
    if (op - flushed >= kFlushAt) store_units(op & ~uint64_t(15));
  }
  __device__ __forceinline__ void copy_in(uint64_t op, uint64_t pos, uint32_t len) {
    gcbytes src = z + g0 + pos;
    for (uint32_t done = 0; done < len;) {
      const uint32_t c = len - done < kChunk ? len - done : kChunk;
      const uint64_t p = op + done;
      sync();
      for (uint32_t i = lane; i < c; i += 64u) win[(p + i) & kRingMask] = src[done + i];
      done += c;
      advance(p + c);
    }
  }
  // the literal scratch from k & ~7 on into the stage: 8-byte loads past the L1, none past the scratch's end
  __device__ __forceinline__ void load_stage(uint32_t k) {
    sb = k & ~7u;
    sync();
#pragma unroll
    for (uint32_t u = 0; u < kStage / 8 / 64; ++u) {
      const uint32_t i = 8u * (lane + 64u * u);
      uint64_t w = 0;
      if (sb + i < kZsBlockMax)
        w = __hip_atomic_load(reinterpret_cast<TSG_ZS_GLOBAL uint64_t*>(lits + sb + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *reinterpret_cast<TSG_ZS_LDS uint64_t*>(stage + i) = w;
    }
    sync();
  }
  __device__ __forceinline__ void copy_lit(uint64_t op, uint32_t k, uint32_t len) {
    for (uint32_t done = 0; done < len;) {
      const uint32_t kk = k + done;
      if (kk - sb >= kStage) load_stage(kk);
      uint32_t c = len - done < kChunk ? len - done : kChunk;
      if (c > sb + kStage - kk) c = sb + kStage - kk;
      const uint64_t p = op + done;
      sync();
      for (uint32_t i = lane; i < c; i += 64u) win[(p + i) & kRingMask] = stage[kk - sb + i];
      done += c;
      advance(p + c);
    }
  }
  __device__ __forceinline__ void fill(uint64_t op, uint32_t b, uint32_t len) {
    for (uint32_t done = 0; done < len;) {
      const uint32_t c = len - done < kChunk ? len - done : kChunk;
      const uint64_t p = op + done;
      sync();
      for (uint32_t i = lane; i < c; i += 64u) win[(p + i) & kRingMask] = static_cast<uint8_t>(b);
      done += c;
      advance(p + c);
    }
  }
  __device__ __forceinline__ uint32_t history(uint64_t p, uint32_t d) {   // the byte d before the chunk's start p
    const uint64_t src = p - d;
    return d <= kZsNear ? win[src & kRingMask] : load_fresh(out + src);
  }
  __device__ __forceinline__ void copy(uint64_t op, uint32_t off, uint32_t len) {
    for (uint32_t done = 0; done < len;) {
      const uint32_t c = len - done < kChunk ? len - done : kChunk;
      const uint64_t p = op + done;
      sync();
      if (off >= c) {
        for (uint32_t i = lane; i < c; i += 64u) win[(p + i) & kRingMask] = static_cast<uint8_t>(history(p, off - i));
      } else {
        for (uint32_t i = lane; i < c; i += 64u) win[(p + i) & kRingMask] = static_cast<uint8_t>(history(p, off - i % off));
      }
      done += c;
      advance(p + c);
    }
  }
  __device__ __forceinline__ void rec(uint32_t k, const ZsFrameRec& r) {
    if (lane == 0) recs[k] = r;
  }
  __device__ __forceinline__ void flush(uint64_t op) {
    store_units(op & ~uint64_t(15));
    for (uint64_t p = flushed + lane; p < op; p += 64u) out[p] = win[p & kRingMask];
    flushed = op;
  }
};

__global__ __launch_bounds__(64) void tsg_zstd_streams(const uint8_t* __restrict__ z, const ZsStream* __restrict__ streams,
                                                       const uint32_t* __restrict__ order, uint32_t nstreams,
                                                       uint8_t* dst, uint8_t* lits, ZsFrameRec* __restrict__ recs,
                                                       ZsResult* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) WaveLds lds;
  if (blockIdx.x >= nstreams) return;
  const uint32_t s = order[blockIdx.x];
  const ZsStream d = streams[s];
  WaveIo io{(gcbytes)z, d.z_begin, d.z_end, (gbytes)(dst + d.dst_begin),
            (gbytes)(lits + static_cast<uint64_t>(blockIdx.x) * kZsBlockMax), recs + d.rec_begin,
            (lbytes)lds.win, (lbytes)lds.inw, (lbytes)lds.stage, threadIdx.x};
  io.refill(d.z_begin & ~uint64_t(15));
  uint32_t nrecs = 0, nblocks = 0;
  uint64_t out_len = 0;
  const int32_t st = zstd_decode(io, &lds.t, d.z_end - d.z_begin, d.dst_cap, d.rec_cap, &nrecs, &nblocks, &out_len);
  if (threadIdx.x == 0) {
    ZsResult r;
    r.out_len = out_len;
    r.status = st;
    r.nrecs = nrecs;
    r.nblocks = nblocks;
    r.pad = 0;
    res[s] = r;
  }
}

struct DevLd {                                   // 8-byte loads where the range starts 8-byte aligned
  const uint8_t* p;
  bool aligned;
  __device__ __forceinline__ uint32_t w8(uint64_t i) const { return p[i]; }
  __device__ __forceinline__ uint32_t w32(uint64_t i) const {
    return aligned ? *reinterpret_cast<const uint32_t*>(p + i) : ZsByteLd{p}.w32(i);
  }
  __device__ __forceinline__ uint64_t w64(uint64_t i) const {
    return aligned ? *reinterpret_cast<const uint64_t*>(p + i) : ZsByteLd{p}.w64(i);
  }
};

// out[i] = the low 32 bits of XXH64 over dst[d[i].begin, + d[i].len)
__global__ __launch_bounds__(64) void tsg_zstd_hash_frames(const uint8_t* __restrict__ dst, const HashDesc* __restrict__ d,
                                                           uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = dst + d[i].begin;
  out[i] = static_cast<uint32_t>(zs_xxh64(DevLd{p, (reinterpret_cast<uintptr_t>(p) & 7u) == 0}, d[i].len));
}

int device_of_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

// what a call allocates, released whatever way it ends
struct Scratch {
  void* p[2] = {nullptr, nullptr};
  hipStream_t s = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Scratch() {
    for (void* q : p)
      if (q) (void)hipFree(q);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }
};

size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

bool hip_ok(hipError_t e, const char* what, std::string* err) {
  if (e == hipSuccess) return true;
  *err = std::string("device zstd decode: ") + what + ": " + hipGetErrorString(e);
  (void)hipGetLastError();
  return false;
}

}  // namespace

ZstdScratch::~ZstdScratch() {
  if (lits) (void)hipFree(lits);
}

bool inflate_zstd_device(ZstdScratch* keep, const void* d_z, const uint64_t* z_off, uint32_t n, void* d_dst,
                         const uint64_t* dst_off, uint64_t* out_lens, int32_t* status, ZstdStats* stats, std::string* err) {
  if (n == 0) return true;
  if (!keep || !z_off || !dst_off || !out_lens || !status) { *err = "zstd: null argument"; return false; }
  for (uint32_t i = 0; i < n; ++i) {
    if (z_off[i] > z_off[i + 1] || dst_off[i] > dst_off[i + 1]) { *err = "zstd: offsets must not decrease"; return false; }
    if (dst_off[i] & 15u) { *err = "zstd: every slot must start 16-byte aligned"; return false; }
  }
  const uint64_t z_total = z_off[n], dst_total = dst_off[n];
  if ((z_total && !d_z) || (dst_total && !d_dst)) { *err = "zstd: null buffer"; return false; }
  const uintptr_t za = reinterpret_cast<uintptr_t>(d_z), da = reinterpret_cast<uintptr_t>(d_dst);
  if ((za | da) & 15u) { *err = "zstd: buffers must be 16-byte aligned"; return false; }
  if (z_total && dst_total && za < da + dst_total && da < za + z_total) {
    *err = "zstd: d_z and d_dst must not overlap";
    return false;
  }
  const int dev = z_total ? device_of_ptr(d_z) : dst_total ? device_of_ptr(d_dst) : 0;
  if (dev < 0 || (dst_total && device_of_ptr(d_dst) != dev)) {
    *err = "zstd: buffers must be device memory of one device";
    return false;
  }
  Scratch sc;
  if (!hip_ok(hipSetDevice(dev), "set device", err) ||
      !hip_ok(hipStreamCreateWithFlags(&sc.s, hipStreamNonBlocking), "stream", err))
    return false;
  for (hipEvent_t& e : sc.ev)
    if (!hip_ok(hipEventCreate(&e), "event", err)) return false;
  // the literal scratch stays on the engine; this call has it to itself until its kernels are done
  std::lock_guard<std::mutex> hold(keep->mu);
  const size_t lit_bytes = static_cast<size_t>(n) * kZsBlockMax;
  if (keep->device != dev || keep->bytes < lit_bytes) {
    if (keep->lits) (void)hipFree(keep->lits);
    keep->lits = nullptr;
    keep->bytes = 0;
    if (!hip_ok(hipMalloc(&keep->lits, lit_bytes), "literal scratch", err)) return false;
    keep->bytes = lit_bytes;
    keep->device = dev;
  }
  // A layer is one frame, or a few: every stream gets room for kRecFirst frame records, and the streams that hold
  // more frames (the decoder counts them all) run once more with room for exactly their count -- not room for the
  // worst case of one frame per 9 bytes, which would be 2.7 times the compressed batch.
  std::vector<uint32_t> rec_cap(n);
  for (uint32_t i = 0; i < n; ++i) rec_cap[i] = std::min(zstd_frame_cap(z_off[i + 1] - z_off[i]), kRecFirst);
  std::vector<ZsResult> res(n);
  std::vector<std::vector<ZsFrameRec>> frames(n);
  float f_dec = 0;
  // one launch over the streams `which` (longest first); res and frames are filled for them
  auto run = [&](const std::vector<uint32_t>& which) -> bool {
    const uint32_t m = static_cast<uint32_t>(which.size());
    std::vector<ZsStream> streams(m);
    std::vector<uint32_t> order(m);
    uint64_t nrec_total = 0;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t i = which[j];
      ZsStream& st = streams[j];
      st.z_begin = z_off[i];
      st.z_end = z_off[i + 1];
      st.dst_begin = dst_off[i];
      st.dst_cap = dst_off[i + 1] - dst_off[i];
      st.rec_begin = nrec_total;
      st.rec_cap = rec_cap[i];
      st.pad = 0;
      nrec_total += st.rec_cap;
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      return streams[x].z_end - streams[x].z_begin > streams[y].z_end - streams[y].z_begin;
    });
    Scratch tmp;                                 // its stream stays null: the launch runs on sc.s
    const size_t o_streams = 0, o_order = align256(m * sizeof(ZsStream)), o_res = o_order + align256(m * 4),
                 o_recs = o_res + align256(m * sizeof(ZsResult)), bytes = o_recs + nrec_total * sizeof(ZsFrameRec);
    if (!hip_ok(hipMalloc(&tmp.p[0], bytes), "scratch", err)) return false;
    uint8_t* base = static_cast<uint8_t*>(tmp.p[0]);
    ZsStream* d_streams = reinterpret_cast<ZsStream*>(base + o_streams);
    uint32_t* d_order = reinterpret_cast<uint32_t*>(base + o_order);
    ZsResult* d_res = reinterpret_cast<ZsResult*>(base + o_res);
    ZsFrameRec* d_recs = reinterpret_cast<ZsFrameRec*>(base + o_recs);
    std::vector<ZsResult> got(m);
    if (!hip_ok(hipMemcpyAsync(d_streams, streams.data(), m * sizeof(ZsStream), hipMemcpyHostToDevice, sc.s), "upload", err) ||
        !hip_ok(hipMemcpyAsync(d_order, order.data(), m * 4, hipMemcpyHostToDevice, sc.s), "upload", err) ||
        !hip_ok(hipEventRecord(sc.ev[0], sc.s), "event", err))
      return false;
    hipLaunchKernelGGL(tsg_zstd_streams, dim3(m), dim3(64), 0, sc.s, static_cast<const uint8_t*>(d_z), d_streams, d_order, m,
                       static_cast<uint8_t*>(d_dst), static_cast<uint8_t*>(keep->lits), d_recs, d_res);
    float f = 0;
    if (!hip_ok(hipGetLastError(), "launch", err) || !hip_ok(hipEventRecord(sc.ev[1], sc.s), "event", err) ||
        !hip_ok(hipMemcpyAsync(got.data(), d_res, m * sizeof(ZsResult), hipMemcpyDeviceToHost, sc.s), "download", err) ||
        !hip_ok(hipStreamSynchronize(sc.s), "decode kernel", err) ||
        !hip_ok(hipEventElapsedTime(&f, sc.ev[0], sc.ev[1]), "event", err))
      return false;
    f_dec += f;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t i = which[j];
      res[i] = got[j];
      frames[i].clear();
      if (got[j].out_len > streams[j].dst_cap || got[j].nrecs > zstd_frame_cap(streams[j].z_end - streams[j].z_begin)) {
        *err = "device zstd decode: inconsistent result";
        return false;
      }
      if (got[j].nrecs == 0 || got[j].nrecs > streams[j].rec_cap) continue;
      frames[i].resize(got[j].nrecs);
      if (!hip_ok(hipMemcpyAsync(frames[i].data(), d_recs + streams[j].rec_begin, got[j].nrecs * sizeof(ZsFrameRec),
                                 hipMemcpyDeviceToHost, sc.s),
                  "download", err))
        return false;
    }
    return hip_ok(hipStreamSynchronize(sc.s), "download", err);
  };
  std::vector<uint32_t> which(n);
  std::iota(which.begin(), which.end(), 0u);
  if (!run(which)) return false;
  which.clear();
  for (uint32_t i = 0; i < n; ++i)
    if (res[i].nrecs > rec_cap[i]) {
      rec_cap[i] = res[i].nrecs;
      which.push_back(i);
    }
  if (!which.empty() && !run(which)) return false;
  std::vector<uint64_t> hrec(n + 1, 0);
  uint64_t blocks = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (res[i].nrecs != frames[i].size()) { *err = "device zstd decode: inconsistent result"; return false; }
    hrec[i + 1] = hrec[i] + res[i].nrecs;
    blocks += res[i].nblocks;
  }
  std::vector<ZsFrameRec> recs;
  recs.reserve(hrec[n]);
  for (uint32_t i = 0; i < n; ++i) recs.insert(recs.end(), frames[i].begin(), frames[i].end());
  // the frames to hash: those that carry a checksum
  std::vector<HashDesc> todo;
  std::vector<uint64_t> slot_of;                 // todo[k] belongs to record slot_of[k]
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < res[i].nrecs; ++k) {
      const ZsFrameRec& r = recs[hrec[i] + k];
      if (r.out_begin > r.out_end || r.out_end > res[i].out_len) { *err = "device zstd decode: inconsistent frame"; return false; }
      if (!r.has_sum) continue;
      todo.push_back({dst_off[i] + r.out_begin, r.out_end - r.out_begin});
      slot_of.push_back(hrec[i] + k);
    }
  if (todo.size() > 0xffffff00ull) { *err = "zstd: too many frames for one call"; return false; }
  const uint32_t nh = static_cast<uint32_t>(todo.size());
  std::vector<uint32_t> got(nh), sums(recs.size(), 0);
  float f_hash = 0;
  if (nh) {
    const size_t o_sum = align256(nh * sizeof(HashDesc));
    if (!hip_ok(hipMalloc(&sc.p[1], o_sum + nh * 4ull), "scratch", err)) return false;
    uint8_t* b1 = static_cast<uint8_t*>(sc.p[1]);
    if (!hip_ok(hipMemcpyAsync(b1, todo.data(), nh * sizeof(HashDesc), hipMemcpyHostToDevice, sc.s), "upload", err) ||
        !hip_ok(hipEventRecord(sc.ev[2], sc.s), "event", err))
      return false;
    hipLaunchKernelGGL(tsg_zstd_hash_frames, dim3((nh + 63u) / 64u), dim3(64), 0, sc.s, static_cast<const uint8_t*>(d_dst),
                       reinterpret_cast<const HashDesc*>(b1), nh, reinterpret_cast<uint32_t*>(b1 + o_sum));
    if (!hip_ok(hipGetLastError(), "launch", err) || !hip_ok(hipEventRecord(sc.ev[3], sc.s), "event", err) ||
        !hip_ok(hipMemcpyAsync(got.data(), b1 + o_sum, nh * 4ull, hipMemcpyDeviceToHost, sc.s), "download", err) ||
        !hip_ok(hipStreamSynchronize(sc.s), "hash kernel", err) ||
        !hip_ok(hipEventElapsedTime(&f_hash, sc.ev[2], sc.ev[3]), "event", err))
      return false;
    for (uint32_t k = 0; k < nh; ++k) sums[slot_of[k]] = got[k];
  }
  for (uint32_t i = 0; i < n; ++i) {
    status[i] = zs_check_frames(res[i].status, recs.data() + hrec[i], res[i].nrecs, sums.data() + hrec[i]);
    out_lens[i] = res[i].out_len;
  }
  if (stats) {
    stats->decode_ms = f_dec;
    stats->hash_ms = f_hash;
    stats->frames = recs.size();
    stats->blocks = blocks;
  }
  return true;
}

}  // namespace tsg
