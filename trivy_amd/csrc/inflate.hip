// Device side of the gzip inflate: a batch of gzip streams in device memory
// inflated there, one wavefront per stream, and the CRC32 of what they wrote.
// inflate.h states the format rules and holds the decoder itself
// (inflate_decode), which this file runs through WaveIo; inflate_model is the
// CPU model of the whole pass.
//
//   tsg_inflate_streams   one workgroup of one wave per stream, workgroup k
//                         taking the k-th longest stream (the dispatcher starts
//                         workgroups in order, so the long ones start first)
//   tsg_crc32_slices      one thread per 4 KiB slice of a member's output; the
//                         host folds a member's slices with the shift operator
//
// A DEFLATE stream is one dependent chain: every lane of the wave runs the
// decoder on the same values (table entries and input bytes pass through
// readfirstlane, so the chain lives in scalar registers and its branches are
// scalar), lane 0 alone stores to the tables and the window, and all 64 lanes
// do what has width: the refill of the input window (two 16-byte loads per
// lane), the copy of a match, and the stores to HBM.
//
// Per-wave LDS (40.5 KiB, four waves per CU):
//   win   32 KiB   the last 32 KiB of output at win[pos & 32767]: the history a
//                  match reads and the token buffer at once -- a literal is one
//                  LDS store, a match an LDS-to-LDS copy in which lane i writes
//                  win[op + i] = win[op - dist + i % dist], a read of bytes
//                  that all precede op (dist = 1, len = 258 replicates one
//                  byte; no lane reads what another writes in the same copy)
//   inw    2 KiB   the input window, 16-byte aligned in d_gz; a chunk is loaded
//                  only when it starts below the stream's end, so at most 15
//                  bytes past the stream are touched, and the decoder never
//                  asks for a byte at or past the end
//   t    5.6 KiB   the literal/length and distance tables (primary + overflow)
//                  and the code lengths, rebuilt by lane 0 per block
// Output leaves LDS in bulk: when 8 KiB are pending, the whole 16-byte units
// below op go out as one 16-byte store per lane (the slot starts 16-byte
// aligned, so unit and window index are aligned alike); the rest goes byte by
// byte at the end.  Every store lies below op <= the slot's capacity.
//
// Ordering inside the wave: LDS operations of one wave execute in program
// order, so lane 0's stores are what the next instruction's loads of the other
// lanes see; the wavefront-scope fence + wave barrier (WaveIo::sync) keeps the
// compiler from moving an access across that point (tarscan.hip's idiom).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "inflate_dev.h"

namespace tsg {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

constexpr uint32_t kInWin = 2048;                // input window bytes: 64 lanes x 2 x 16
constexpr uint32_t kFlushAt = 8192;              // pending output that triggers a store to HBM
constexpr uint32_t kWinMask = kInfWindow - 1;

struct InfStream {                               // one stream's place, all offsets in bytes
  uint64_t gz_begin, gz_end;                     // in d_gz
  uint64_t dst_begin, dst_cap;                   // in d_dst
  uint64_t rec_begin;                            // first member record
  uint32_t rec_cap, pad;
};
struct InfResult {
  uint64_t out_len;
  int32_t status;
  uint32_t nrecs;
};
struct CrcSliceDesc {
  uint64_t begin;                                // in d_dst
  uint32_t len, pad;
};

struct WaveLds {
  uint8_t win[kInfWindow];
  uint8_t inw[kInWin];
  InfTables t;
};

struct WaveIo {
  const uint8_t* gz;                             // d_gz, 16-byte aligned
  uint64_t g0, g1;                               // the stream in d_gz
  uint8_t* out;                                  // the slot, 16-byte aligned
  InfMember* recs;
  uint8_t* win;
  uint8_t* inw;
  uint32_t lane;
  uint64_t wa = 0;                               // the input window's start in d_gz (16-byte aligned)
  uint64_t flushed = 0;                          // output below it is in HBM; a multiple of 16 until the end

  __device__ bool leader() const { return lane == 0; }
  __device__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ void refill(uint64_t a) {
    wa = a & ~uint64_t(15);
    sync();
#pragma unroll
    for (uint32_t c = 0; c < kInWin / 16 / 64; ++c) {
      const uint32_t k = 16u * (lane + 64u * c);
      v4u w = {0u, 0u, 0u, 0u};
      if (wa + k < g1) w = *reinterpret_cast<const v4u*>(gz + wa + k);
      *reinterpret_cast<v4u*>(inw + k) = w;
    }
    sync();
  }
  __device__ uint32_t in(uint64_t pos) {          // pos < the stream's length
    const uint64_t a = g0 + pos;
    if (a - wa >= kInWin) refill(a);
    return TSG_INF_UNIFORM(inw[a - wa]);
  }
  // the whole 16-byte units of [flushed, e) to HBM; e a multiple of 16, e - flushed < 32 KiB
  __device__ void store_units(uint64_t e) {
    sync();
    for (uint64_t p = flushed + 16u * lane; p < e; p += 16u * 64u)
      *reinterpret_cast<v4u*>(out + p) = *reinterpret_cast<const v4u*>(win + (p & kWinMask));
    flushed = e;
  }
  __device__ void advance(uint64_t op) {          // op = output bytes so far
    if (op - flushed >= kFlushAt) store_units(op & ~uint64_t(15));
  }
  __device__ void lit(uint64_t op, uint32_t b) {
    if (lane == 0) win[op & kWinMask] = static_cast<uint8_t>(b);
    advance(op + 1);
  }
  __device__ void copy(uint64_t op, uint32_t dist, uint32_t len) {
    sync();
    for (uint32_t i = lane; i < len; i += 64u) win[(op + i) & kWinMask] = win[(op - dist + i % dist) & kWinMask];
    sync();
    advance(op + len);
  }
  __device__ void rec(uint32_t k, const InfMember& m) {
    if (lane == 0) recs[k] = m;
  }
  __device__ void flush(uint64_t op) {
    store_units(op & ~uint64_t(15));
    for (uint64_t p = flushed + lane; p < op; p += 64u) out[p] = win[p & kWinMask];
    flushed = op;
  }
};

__global__ __launch_bounds__(64) void tsg_inflate_streams(const uint8_t* __restrict__ gz,
                                                          const InfStream* __restrict__ streams,
                                                          const uint32_t* __restrict__ order, uint32_t nstreams,
                                                          uint8_t* __restrict__ dst, InfMember* __restrict__ recs,
                                                          InfResult* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) WaveLds lds;
  if (blockIdx.x >= nstreams) return;
  const uint32_t s = order[blockIdx.x];
  const InfStream d = streams[s];
  WaveIo io{gz, d.gz_begin, d.gz_end, dst + d.dst_begin, recs + d.rec_begin, lds.win, lds.inw, threadIdx.x};
  io.refill(d.gz_begin);
  uint32_t nrecs = 0;
  uint64_t out_len = 0;
  const int32_t st = inflate_decode(io, &lds.t, d.gz_end - d.gz_begin, d.dst_cap, d.rec_cap, &nrecs, &out_len);
  if (threadIdx.x == 0) {
    InfResult r;
    r.out_len = out_len;
    r.status = st;
    r.nrecs = nrecs;
    res[s] = r;
  }
}

__device__ __forceinline__ uint32_t crc_step(const uint32_t* tab, uint32_t c, uint32_t b) {
  return tab[(c ^ b) & 0xffu] ^ (c >> 8);
}
__device__ __forceinline__ uint32_t crc_word(const uint32_t* tab, uint32_t c, uint32_t w) {
  c = crc_step(tab, c, w);
  c = crc_step(tab, c, w >> 8);
  c = crc_step(tab, c, w >> 16);
  return crc_step(tab, c, w >> 24);
}

// out[i] = CRC32 of dst[sl[i].begin, + sl[i].len): bytes up to a 16-byte
// boundary, 16-byte loads, bytes again
__global__ __launch_bounds__(256) void tsg_crc32_slices(const uint8_t* __restrict__ dst,
                                                        const CrcSliceDesc* __restrict__ sl, uint32_t n,
                                                        uint32_t* __restrict__ out) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = inf_crc_byte(0, threadIdx.x);
  __syncthreads();
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = dst + sl[i].begin;
  uint32_t len = sl[i].len, c = 0xffffffffu;
  for (; len && (reinterpret_cast<uintptr_t>(p) & 15u); --len, ++p) c = crc_step(tab, c, *p);
  for (; len >= 16; len -= 16, p += 16) {
    const v4u w = *reinterpret_cast<const v4u*>(p);
    c = crc_word(tab, crc_word(tab, crc_word(tab, crc_word(tab, c, w.x), w.y), w.z), w.w);
  }
  for (; len; --len, ++p) c = crc_step(tab, c, *p);
  out[i] = ~c;
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
  *err = std::string("device inflate: ") + what + ": " + hipGetErrorString(e);
  (void)hipGetLastError();
  return false;
}

}  // namespace

bool inflate_gzip_device(const void* d_gz, const uint64_t* gz_off, uint32_t n, void* d_dst, const uint64_t* dst_off,
                         uint64_t* out_lens, int32_t* status, InflateStats* stats, std::string* err) {
  if (n == 0) return true;
  if (!gz_off || !dst_off || !out_lens || !status) { *err = "inflate: null argument"; return false; }
  for (uint32_t i = 0; i < n; ++i) {
    if (gz_off[i] > gz_off[i + 1] || dst_off[i] > dst_off[i + 1]) { *err = "inflate: offsets must not decrease"; return false; }
    if (dst_off[i] & 15u) { *err = "inflate: every slot must start 16-byte aligned"; return false; }
  }
  const uint64_t gz_total = gz_off[n], dst_total = dst_off[n];
  if ((gz_total && !d_gz) || (dst_total && !d_dst)) { *err = "inflate: null buffer"; return false; }
  const uintptr_t ga = reinterpret_cast<uintptr_t>(d_gz), da = reinterpret_cast<uintptr_t>(d_dst);
  if ((ga | da) & 15u) { *err = "inflate: buffers must be 16-byte aligned"; return false; }
  if (gz_total && dst_total && ga < da + dst_total && da < ga + gz_total) {
    *err = "inflate: d_gz and d_dst must not overlap";
    return false;
  }
  const int dev = gz_total ? device_of_ptr(d_gz) : dst_total ? device_of_ptr(d_dst) : 0;
  if (dev < 0 || (dst_total && device_of_ptr(d_dst) != dev)) {
    *err = "inflate: buffers must be device memory of one device";
    return false;
  }
  // the streams' places, the order of their start (longest first) and the member records' places
  std::vector<InfStream> streams(n);
  std::vector<uint32_t> order(n);
  uint64_t nrec_total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    InfStream& s = streams[i];
    s.gz_begin = gz_off[i];
    s.gz_end = gz_off[i + 1];
    s.dst_begin = dst_off[i];
    s.dst_cap = dst_off[i + 1] - dst_off[i];
    s.rec_begin = nrec_total;
    s.rec_cap = inflate_member_cap(s.gz_end - s.gz_begin);
    s.pad = 0;
    nrec_total += s.rec_cap;
  }
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return streams[a].gz_end - streams[a].gz_begin > streams[b].gz_end - streams[b].gz_begin;
  });
  Scratch sc;
  if (!hip_ok(hipSetDevice(dev), "set device", err) ||
      !hip_ok(hipStreamCreateWithFlags(&sc.s, hipStreamNonBlocking), "stream", err))
    return false;
  for (hipEvent_t& e : sc.ev)
    if (!hip_ok(hipEventCreate(&e), "event", err)) return false;
  const size_t o_streams = 0, o_order = align256(n * sizeof(InfStream)), o_res = o_order + align256(n * 4),
               o_recs = o_res + align256(n * sizeof(InfResult)), bytes = o_recs + nrec_total * sizeof(InfMember);
  if (!hip_ok(hipMalloc(&sc.p[0], bytes), "scratch", err)) return false;
  uint8_t* base = static_cast<uint8_t*>(sc.p[0]);
  InfStream* d_streams = reinterpret_cast<InfStream*>(base + o_streams);
  uint32_t* d_order = reinterpret_cast<uint32_t*>(base + o_order);
  InfResult* d_res = reinterpret_cast<InfResult*>(base + o_res);
  InfMember* d_recs = reinterpret_cast<InfMember*>(base + o_recs);
  std::vector<InfResult> res(n);
  if (!hip_ok(hipMemcpyAsync(d_streams, streams.data(), n * sizeof(InfStream), hipMemcpyHostToDevice, sc.s), "upload", err) ||
      !hip_ok(hipMemcpyAsync(d_order, order.data(), n * 4, hipMemcpyHostToDevice, sc.s), "upload", err) ||
      !hip_ok(hipEventRecord(sc.ev[0], sc.s), "event", err))
    return false;
  hipLaunchKernelGGL(tsg_inflate_streams, dim3(n), dim3(64), 0, sc.s, static_cast<const uint8_t*>(d_gz), d_streams, d_order,
                     n, static_cast<uint8_t*>(d_dst), d_recs, d_res);
  if (!hip_ok(hipGetLastError(), "launch", err) || !hip_ok(hipEventRecord(sc.ev[1], sc.s), "event", err) ||
      !hip_ok(hipMemcpyAsync(res.data(), d_res, n * sizeof(InfResult), hipMemcpyDeviceToHost, sc.s), "download", err) ||
      !hip_ok(hipStreamSynchronize(sc.s), "inflate kernel", err))
    return false;
  // the records the streams wrote (the device array is sized for the worst case, one member per 20 bytes)
  std::vector<uint64_t> hrec(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (res[i].nrecs > streams[i].rec_cap || res[i].out_len > streams[i].dst_cap) {
      *err = "device inflate: inconsistent result";
      return false;
    }
    hrec[i + 1] = hrec[i] + res[i].nrecs;
  }
  std::vector<InfMember> recs(hrec[n]);
  for (uint32_t i = 0; i < n; ++i)
    if (res[i].nrecs && !hip_ok(hipMemcpyAsync(recs.data() + hrec[i], d_recs + streams[i].rec_begin,
                                               res[i].nrecs * sizeof(InfMember), hipMemcpyDeviceToHost, sc.s),
                                "download", err))
      return false;
  if (!hip_ok(hipStreamSynchronize(sc.s), "download", err)) return false;
  // the members' slices
  std::vector<CrcSliceDesc> slices;
  uint64_t members = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const InfStream& s = streams[i];
    for (uint32_t k = 0; k < res[i].nrecs; ++k) {
      const InfMember& m = recs[hrec[i] + k];
      if (m.out_begin > m.out_end || m.out_end > res[i].out_len) { *err = "device inflate: inconsistent member"; return false; }
      for (uint64_t b = m.out_begin; b < m.out_end; b += kCrcSlice)
        slices.push_back({s.dst_begin + b, static_cast<uint32_t>(std::min<uint64_t>(kCrcSlice, m.out_end - b)), 0});
      ++members;
    }
  }
  if (slices.size() > 0xffffff00ull) { *err = "inflate: too much output for one call"; return false; }
  const uint32_t ns = static_cast<uint32_t>(slices.size());
  std::vector<uint32_t> crcs(ns);
  float f_inf = 0, f_crc = 0;
  if (ns) {
    const size_t o_crc = align256(ns * sizeof(CrcSliceDesc));
    if (!hip_ok(hipMalloc(&sc.p[1], o_crc + ns * 4ull), "scratch", err)) return false;
    uint8_t* b1 = static_cast<uint8_t*>(sc.p[1]);
    if (!hip_ok(hipMemcpyAsync(b1, slices.data(), ns * sizeof(CrcSliceDesc), hipMemcpyHostToDevice, sc.s), "upload", err) ||
        !hip_ok(hipEventRecord(sc.ev[2], sc.s), "event", err))
      return false;
    hipLaunchKernelGGL(tsg_crc32_slices, dim3((ns + 255u) / 256u), dim3(256), 0, sc.s, static_cast<const uint8_t*>(d_dst),
                       reinterpret_cast<const CrcSliceDesc*>(b1), ns, reinterpret_cast<uint32_t*>(b1 + o_crc));
    if (!hip_ok(hipGetLastError(), "launch", err) || !hip_ok(hipEventRecord(sc.ev[3], sc.s), "event", err) ||
        !hip_ok(hipMemcpyAsync(crcs.data(), b1 + o_crc, ns * 4ull, hipMemcpyDeviceToHost, sc.s), "download", err) ||
        !hip_ok(hipStreamSynchronize(sc.s), "checksum kernel", err) ||
        !hip_ok(hipEventElapsedTime(&f_crc, sc.ev[2], sc.ev[3]), "event", err))
      return false;
  }
  if (!hip_ok(hipEventElapsedTime(&f_inf, sc.ev[0], sc.ev[1]), "event", err)) return false;
  const uint32_t* sp = crcs.data();
  for (uint32_t i = 0; i < n; ++i) {
    const InfMember* r = recs.data() + hrec[i];
    status[i] = inf_check_members(res[i].status, r, res[i].nrecs, sp);
    out_lens[i] = res[i].out_len;
    for (uint32_t k = 0; k < res[i].nrecs; ++k) sp += crc32_nslices(r[k].out_end - r[k].out_begin);
  }
  if (stats) {
    stats->inflate_ms = f_inf;
    stats->crc_ms = f_crc;
    stats->members = members;
    stats->slices = ns;
  }
  return true;
}

}  // namespace tsg
