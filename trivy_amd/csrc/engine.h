// GPU engine: device-resident rule tables on one or more MI355X devices and
// the batch pipeline (upload -> K1 -> K2 -> candidates -> exact host confirm).
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gather.h"
#include "prefilter.h"
#include "scanner.h"
#include "segments.h"
#include "wire_strips.h"
#include "wirepack.h"
#ifdef __HIPCC__
#include "gather_dev.h"                 // (the engine's own translation unit: the gather kernels' launches)
#endif

namespace tsg {

struct FeedOpts;       // feed.h
struct LayerWalk;      // tar.h
struct TarScanStats;   // tarscan.h

struct ScanStats {
  double k1_ms = 0, k2_ms = 0, h2d_ms = 0, d2h_ms = 0, host_ms = 0, total_ms = 0;
  double gpu_wall_ms = 0;               // sum over devices of the driver threads' busy time
  uint64_t bytes = 0, files = 0, hits = 0, candidates = 0, confirm_files = 0, findings = 0;
  uint32_t k1_blocks = 0, k1_threads = 0, chunk_bytes = 0, pieces = 1;
  int table_in_lds = 0;
  uint32_t k1_launches = 0;             // K1 launches (segments x scan-DFA groups)
  uint32_t devices = 1;                 // devices that took part
  double feed_ms = 0;                   // wall time from the first upload to the last segment's upload done
  // wire packing (wirepack.h): bytes that crossed the link for the batch's
  // data, strips sent packed / as they are, the packer threads' summed busy time
  uint64_t wire_bytes = 0;
  uint32_t packed_strips = 0, raw_strips = 0;
  double pack_ms = 0;
  // blocks of the strips sent packed by the mode they crossed in, and the
  // bytes the 6-bit blocks escaped
  uint64_t blocks_6bit = 0, blocks_7bit = 0, blocks_raw = 0, escaped_bytes = 0, blocks_split = 0;
  // device-only scans (gather.h): files, bytes and runs the GPU gathered for
  // the confirmer, the gather kernels' time, copy launches repeated with a
  // larger buffer
  uint64_t gather_files = 0, gather_bytes = 0, gather_runs = 0;
  double gather_ms = 0;
  uint32_t gather_retries = 0;
  // ... with windows (tsg_device_scan_opts): files confirmed from windows, the
  // windowed layouts' runs and bytes (whole files' among them), and the files
  // and bytes of the fallback round (files fetched whole after all).
  // gather_bytes and gather_runs hold both rounds.
  uint64_t window_files = 0, window_runs = 0, window_bytes = 0, fallback_files = 0, fallback_bytes = 0;
  // ... with a line cap (gather.h line_window): candidates whose window covers
  // more chunks than the byte window, candidates whose walk ended at the cap,
  // and the line pass's own time (part of gather_ms)
  uint64_t line_widened = 0, line_capped = 0;
  double line_ms = 0;
};

// A batch scan stage: results[i] = Scan(ScanArgs{paths[i], data[off[i]:off[i+1]],
// binary[i]}) -- Engine::scan, or (tests only) the CPU model of its passes.
using BatchScanFn = std::function<bool(const BatchInput& in, SecretVec* results, std::string* err)>;

// Per-file flag word K1 writes (fflags): bit 0 = the file holds U+0130, U+212A
// or U+017F, whose lower / upper case is ASCII (the host re-scans it exactly);
// also set for a file that shares a 16-byte word of the batch with such a
// sequence of a neighbouring file (k1_special: a superset is safe).
constexpr uint32_t kFileFoldSpecial = 1u;

// Test hook (tsg_test_keep_raw): what the GPU passes of one scan() gave, kept
// beside the findings -- one record per segment as Engine::scan cut the batch,
// and every real file's candidates and flag word in batch file indices.
struct RawSegment {
  uint32_t f0 = 0, nfiles = 0, lead = 0;  // first file of the batch, the segment's own files, 1 = it ran with a lead file
  uint64_t b0 = 0, bytes = 0, lead_bytes = 0;
  uint32_t chunk = 0;                   // K1 chunk bytes of this segment
  uint64_t hits = 0;                    // K1 anchor hits (the lead's included)
  std::vector<uint16_t> nl;             // '\n' per chunk; the grid starts at b0 - lead_bytes
  uint32_t lead_flags = 0;              // the lead's flag word
  uint32_t lead_emitted = 0;            // candidates K2 emitted for the lead (duplicates included)
  std::vector<uint32_t> lead_rules;     // the lead's distinct candidates, sorted by (rule, start)
  std::vector<uint64_t> lead_starts;
  // device-only scans with tsg_test_keep_gather on: the gather as it came back
  // from the device, over the segment's files with the lead (segment frame)
  std::vector<uint8_t> need;
  std::vector<uint64_t> goff;
  std::vector<GatherRun> runs;
  uint64_t gather_total = 0;
  std::vector<uint64_t> gather_caps;    // the buffer's capacity at each copy launch
  std::vector<uint8_t> guard_ok;        // per launch: the 0xA5 pattern past that capacity was still whole
  std::vector<uint8_t> gathered;        // gather_total bytes of the buffer
  // ... with windows: the files' classes (gather.h kGatherClass*; goff then
  // holds the whole files' offsets as the host derived them) and the files
  // found insufficient (segment file indices)
  std::vector<uint8_t> cls;
  std::vector<uint32_t> insufficient;
};
// K1's per-chunk and per-file outputs of one prefilter_only call (tests).
struct PrefilterRaw {
  std::vector<uint16_t> nl;             // '\n' count per K1 chunk of the packed batch
  std::vector<uint32_t> ff;             // per-file flag word (kFileFoldSpecial)
  uint32_t chunk = 0;                   // K1 chunk bytes (nl[] granularity)
  // tsg_test_keep_gather on and no host copy given: the device-only scan's
  // gather of this one segment (need ... gathered), without a confirmation
  RawSegment gather;
};
struct RawScan {
  std::vector<RawSegment> segs;
  std::vector<std::vector<std::vector<uint64_t>>> cands;   // [file][rule]; a file without candidates has no rule lists
  std::vector<uint32_t> ff;
  std::string error;                    // a candidate outside its segment's files or the rule table
  // device-only scans with windows and tsg_test_keep_gather on: the fallback
  // round's gather as it came back -- the run table in the batch's frame (src)
  // and the round's one buffer (dst), its bytes, capacity and guard; need and
  // goff over the batch's files (goff: in that buffer)
  bool has_fallback = false;
  RawSegment fallback;
};

struct DeviceTables;
struct Lane;
struct GpuOut;
struct SegmentOut;     // confirm.h
struct CallCtx;        // confirm.h
struct K1Chain;
struct StageIn;
struct WireFeed;
struct SegRun;
struct SegmentDriver;

// One engine = the compiled ruleset's device tables on every selected device.
// scan() is reentrant: each call takes its own lane (HIP streams + scratch
// buffers) on every device it uses and its own host confirm pool.
class Engine {
 public:
  // devices: HIP device ordinals (may repeat one ordinal: replicas on one
  // device, used to exercise the multi-device queue on a one-GPU machine).
  // Fails (nullptr, *err set) when no HIP device is available: the product
  // path has no CPU fallback.
  static std::unique_ptr<Engine> create(std::shared_ptr<const Ruleset> rs, const std::vector<int>& devices,
                                        std::string* err);
  ~Engine();

  // results[i] is Scanner.Scan(ScanArgs{paths[i], data[off[i]:off[i+1]], binary[i]}).
  // raw (tests only, tsg_test_keep_raw): receives the segments' GPU outputs.
  // win (device-only scans): gather windows around candidates (gather.h); NULL or off: whole files.
  bool scan(const BatchInput& in, SecretVec* results, ScanStats* stats, std::string* err, RawScan* raw = nullptr,
            const GatherWindowOpts* win = nullptr);

  // Only the two GPU passes (no host confirmation): used by tests to compare
  // raw candidates ([file][rule], exclude-block pseudo-rules after the rules,
  // as in Prefilter::rules).  Resident data on the engine's first device.
  // raw (optional): K1's other outputs as they came back from the device
  // (and, with tsg_test_keep_gather on and no in.h_data, the gather's).
  bool prefilter_only(const BatchInput& in, std::vector<std::vector<std::vector<uint64_t>>>* cands,
                      ScanStats* stats, std::string* err, PrefilterRaw* raw = nullptr);

  // Host-feed ceiling (no kernels): streams `bytes` of host memory through
  // the first device's upload ring in pieces of the policy's segment bytes,
  // as scan() does, and returns the wall time in ms.
  bool feed_probe(const uint8_t* h_data, uint64_t bytes, double* ms, std::string* err);

  // GPU-side CR strip of a device-resident batch on the first device
  // (crstrip.h, prep.hip): d_dst = d_src without '\r', d_new_off = the files' new
  // starts; *out_total = stripped bytes, *ms = the kernels' time (HIP events).
  bool strip_cr(const void* d_src, const uint64_t* d_off, uint32_t nfiles, uint64_t total, void* d_dst,
                uint64_t* d_new_off, uint64_t* out_total, double* ms, std::string* err);

  // GPU-side content preparation of a raw device-resident batch (prep.hip;
  // prep.h is its CPU model) on the device that owns d_raw: h_off (host,
  // nfiles + 1, nondecreasing from 0) cuts it into files, h_flags (host) are
  // prepare_gate's.  d_dst (dst_cap bytes) receives the prepared bytes and 64
  // zero bytes; h_new_off (nfiles + 1) every file's start in it, h_kinds
  // (nfiles) what became of each file.  Fails, with the size needed in *err
  // and d_dst untouched, when they do not fit.  pass_ms (may be NULL): the
  // kernel time of classify, count, scan, compact; *ms their sum.
  bool prepare_device(const void* d_raw, const uint64_t* h_off, uint32_t nfiles, const uint8_t* h_flags, void* d_dst,
                      uint64_t dst_cap, uint64_t* h_new_off, uint8_t* h_kinds, uint64_t* out_total, double* ms,
                      double* pass_ms, std::string* err);

  // The mark / compact pass of the device tar walk alone (tarscan.hip; test
  // hook): the block numbers plan_tar_marks marks in d_tar[0, len), in order,
  // and those blocks' bytes.
  bool tar_scan_device(const void* d_tar, uint64_t len, std::vector<uint64_t>* idx, std::vector<uint8_t>* blocks,
                       TarScanStats* st, std::string* err);

  // walker.LayerTar.Walk plus the content preparation of a layer tar in
  // device memory: the blocks walk_layer may read are marked and gathered on
  // the device (tarscan.h), the walk runs on the host over them
  // (SparseTarInput; a read they miss is a small copy from d_tar), the walked
  // files pass prepare_gate, and prepare_device takes the tar itself with
  // 2n + 1 interleaved entries (gap, file, gap, ..., tail gap; gaps dropped).
  // kinds / new_off: of the walk's n files.  A malformed tar fails with
  // walk_layer's text before d_dst is touched; pointer checks, capacity
  // failure and times are prepare_device's.
  bool prepare_layer_tar_device(const void* d_tar, uint64_t len, const FeedOpts& fo,
                                const std::vector<std::string>& skip_files, const std::vector<std::string>& skip_dirs,
                                int threads, void* d_dst, uint64_t dst_cap, LayerWalk* walk, std::vector<uint8_t>* kinds,
                                std::vector<uint64_t>* new_off, TarScanStats* st, double* ms, double* pass_ms,
                                std::string* err);

  // Lanes created over all devices, call contexts, and confirm-pool threads
  // started (test hook: the per-file queue's footprint).
  void footprint(uint32_t* lanes, uint32_t* calls, uint32_t* pool_threads);
  // Test hook: the next n run_segment calls fail before their first launch.
  void inject_segment_failures(uint32_t n) { inject_fail_.store(n); }
  // Test hook (tsg_test_keep_raw): the C-ABI's scans pass a RawScan while it is on.
  void set_keep_raw(bool on) { keep_raw_.store(on); }
  bool keep_raw() const { return keep_raw_.load(std::memory_order_relaxed); }
  // Test hook (tsg_test_keep_gather): with keep_raw's record, a device-only
  // scan keeps each segment's gather (RawSegment::need ... gathered).
  void set_keep_gather(bool on) { keep_gather_.store(on); }
  bool keep_gather() const { return keep_gather_.load(std::memory_order_relaxed); }
  // Test hook: gather buffers the devices' pools own, those back in a pool, their bytes.
  void gather_pool(uint32_t* buffers, uint32_t* idle, uint64_t* bytes);
  // CPU model of a device-only scan (tests without a GPU): an engine without
  // devices around a compiled prefilter (copied), and one batch through the table model's candidates, plan_gather,
  // a memcpy gather into a buffer of its own and confirm_segment without
  // h_data.  in.h_data is the batch (read only to build the model's GPU
  // outputs and the gather); chunk: the K1 chunk to model.
  static std::unique_ptr<Engine> create_model(std::shared_ptr<const Ruleset> rs, const Prefilter& pf);
  // before_confirm (optional) runs once the gather is made and before the
  // confirmation: nothing reads in.h_data after it (a sanitizer run frees the
  // batch there).
  // win on: plan_gather_windows' layout, every run copied into an allocation
  // of its own (a read past a run is a read outside an allocation), the
  // windowed confirmation, and the fallback round over the insufficient files
  // (raw->segs[0]: the first round; raw->segs[1]: the fallback's gather).
  bool model_scan_device(const BatchInput& in, uint32_t chunk, SecretVec* results, ScanStats* stats, std::string* err,
                         RawScan* raw = nullptr, const std::function<void()>* before_confirm = nullptr,
                         const GatherWindowOpts* win = nullptr);
  // one byte per row of the prefilter's rule table: a candidate of that row
  // can be confirmed from a window (an anchored or reverse-anchored rule whose
  // keyword gate is exact on the GPU; no exclude-block pseudo-rule)
  std::vector<uint8_t> windowable_rows() const;

  const Prefilter& prefilter() const { return pf_; }
  std::shared_ptr<const Ruleset> ruleset() const { return rs_; }
  const std::vector<int>& devices() const { return devices_; }
  void set_threads(int n) { threads_ = n; }

 private:
  Engine() = default;
  // while_gpu (optional) runs once on the calling thread after the segment's
  // kernels are queued, before their readbacks are; chain (optional) orders
  // the K1 launches of several drivers of one device (K1Chain); defer_copy
  // leaves the readback in the lane's pinned buffers (GpuOut::finish_copy);
  // stage (optional) is a small pinned batch the segment prologue copies in
  // (used by this call only: nothing of it stays on the pooled lane)
  bool run_segment(DeviceTables& dt, Lane& ln, const Segment& sg, const void* d_data, const uint64_t* d_off_up,
                   ScanStats* st, GpuOut* out, std::string* err, const std::function<void()>* while_gpu = nullptr,
                   K1Chain* chain = nullptr, bool defer_copy = false, const StageIn* stage = nullptr,
                   bool gather = false, const GatherWindowOpts* win = nullptr);
  bool fallback_round(const BatchInput& in, const std::vector<Segment>& segs, DeviceTables& dt, CallCtx& cc,
                      std::vector<std::pair<size_t, SegmentOut>>* short_segs, SecretVec* results, ScanStats* st,
                      uint64_t* nconf, uint64_t* nfind, uint64_t* nwindow, RawScan* raw, std::string* err);
  // run_segment's phases (SegRun: what they share)
  bool seg_geometry(SegRun& r, GpuOut* out, std::string* err);
  bool seg_stage_offsets(SegRun& r, std::string* err);
  bool seg_size_scratch(SegRun& r, std::string* err);
  bool seg_prologue(SegRun& r, int attempt, std::string* err);
  bool seg_k1_lds_limits(SegRun& r, std::string* err);
  bool seg_launch_k1(SegRun& r, int attempt, std::string* err);
  bool seg_launch_k2(SegRun& r, int a2, std::string* err);
  bool seg_readback_wait(SegRun& r, int a2, std::string* err);
  bool seg_wait(SegRun& r, std::string* err);
  // device-only scans: the gather kernels behind K2, and the copy again into a larger buffer
  bool seg_launch_gather(SegRun& r, GpuOut* out, std::string* err);
  bool seg_gather_retry(SegRun& r, GpuOut* out, std::string* err);
  void seg_hand_off(SegRun& r, uint32_t ncands, uint32_t nover, bool defer_copy, GpuOut* out);
  bool seg_write_traces(SegRun& r, std::string* err);   // (probe library)
  bool fold_k2_stats(Lane& ln, std::string* err);
  friend struct SegmentDriver;                           // a scan's device driver (engine.hip)
  friend struct WireFeed;                                // takes and returns the engine's packers
  void plan_confirm(const Segment& sg, SegmentOut* g) const;
  void prepare_windows(const Segment& sg, SegmentOut* g) const;
  bool model_scan_windows(const BatchInput& in, uint32_t chunk, SegmentOut& g, bool all, const GatherWindowOpts& win,
                          SecretVec* results, ScanStats* st, std::string* err, RawScan* raw,
                          const std::function<void()>* before_confirm);
  void confirm_segment(CallCtx& cc, const Segment& sg, SegmentOut& g, Secret* results, uint64_t* nconf,
                       uint64_t* nfind, bool gpu_in_flight);
  // g's insufficient files again, from a gather of those whole files
  // (plan_gather's goff over the segment, the buffer at gbase)
  void confirm_fallback(CallCtx& cc, const Segment& sg, SegmentOut& g, const GatherPlan& gp, const uint8_t* gbase,
                        Secret* results, uint64_t* nconf, uint64_t* nfind);
  Lane* acquire_lane(DeviceTables& dt, std::string* err);
  void release_lane(DeviceTables& dt, Lane* ln);
  bool tar_gather(DeviceTables& dt, Lane* ln, const uint8_t* d_tar, uint64_t len, uint64_t* cap_blocks,
                  TarScanStats* st, std::string* err);
  DeviceTables* tables_of(int device);                   // NULL: not one of the engine's devices
  CallCtx* acquire_call();
  void release_call(CallCtx* cc);

  std::shared_ptr<const Ruleset> rs_;
  Prefilter pf_;
  std::vector<int> devices_;
  std::vector<std::unique_ptr<DeviceTables>> dev_;
  int threads_ = 0;
  std::mutex call_mu_;
  std::vector<std::unique_ptr<CallCtx>> calls_;
  std::vector<CallCtx*> free_calls_;
  // tuning (TSG_* environment knobs, read once at create)
  uint32_t chunk_ = 0;                  // K1 bytes per lane chunk (TSG_K1_CHUNK); 0 = by launch size (k1_chunk_for)
  // TSG_K1_ABL: K1 build (kAbl* bits).  Default 4560 = deferred outputs +
  // rolled word loop + 64-byte lines + temporal loads + fast words in boundary
  // lines (layout bits, results valid); the other bits are measurement builds
  // whose results are invalid.
  int k1_abl_ = 4560;
  uint32_t k1_tail_rounds_ = 1;         // v3 guided schedule: grid rounds of 2- and of 1-chunk ranges (TSG_K1_TAIL_ROUNDS)
  // launches of >= 2 GiB: 1 KiB chunks with 8-chunk bulk ranges, then rounds
  // of 4-, 2- and 1-chunk ranges (TSG_K1_TOP8=1; 2: the kU = 8 level in every
  // launch, for tests), instead of 2 KiB chunks
  int k1_top8_ = 1;
  // drivers per device for resident batches (TSG_RESIDENT_DRIVERS; 2 =
  // K1Chain).  Round 4 chained the second driver's K1 behind the first's K2:
  // no gain (config 2 1530 vs 1528 GB/s).  Chained behind the first's K1
  // (TSG_CHAIN_K1, round 5) a piece's K2 runs beside the next piece's K1 and
  // leaves the critical chain: config 2 1632 -> 1862 GB/s, 1 GB of config-1
  // files 482 -> 570 (profiles/r5p_resident_variants.log).
  int resident_drivers_ = 2;
  int chain_k1_ = 1;                    // K1Chain: 0 = next K1 after this K2, 1 = after this K1, 2 = no wait (TSG_CHAIN_K1)
  bool file_index_ = true;              // K1 range starts' files from a per-64-KiB index (TSG_K1_FILE_INDEX)
  // Wire packing of uploaded batches (wirepack.h; TSG_WIRE_PACK 0 = off, 1 =
  // packers race the link, force = every strip waits for a packer, both with
  // the 7-bit codec; 2 and force2 = the same with the 6-bit codec; 3 and
  // force3 = the 6-bit codec with split blocks allowed.  Unset: 2, with split
  // blocks where the CPU packs them with VBMI2 and the scan uploads at least
  // kWireDenseMinBytes -- a smaller one is over before the packers are ahead).  The
  // packer threads belong to the engine: started on the first eligible scan,
  // parked on wire_cv_ between scans, serving one scan at a time (wire_job_).
  int wire_mode_ = 0;                   // 0 off, 1 race, 2 force
  int wire_codec_ = 1;                  // 1 = 7-bit, 2 = 6-bit codes with escapes
  int wire_split_ = 0;                  // split blocks: 0 = never, 1 = allowed, -1 = by the rule for an unset TSG_WIRE_PACK
  int wire_threads_n_ = -1;             // TSG_WIRE_PACK_THREADS; -1 = the engine's threads - 2, at most 16
  // bytes per strip (TSG_WIRE_STRIP_BYTES, a multiple of 4096).  Config 2, 14
  // packers: 4 MiB 198.7 ms per step, 8 MiB 179.2, 16 MiB 169.9-170.2, 32 MiB
  // 165.0, 64 MiB 162.4-163.1 (single copy per segment: 179.0-179.2): every
  // strip copy costs the link about 14 us; 64 MiB with the packers a segment
  // ahead 160.9-161.1 (profiles/wirepack_c2.json).  Each packer holds a pinned
  // staging slot and a device twin of this size.
  uint64_t wire_strip_ = 64ull << 20;
  bool wire_ramp_ = true;               // TSG_WIRE_RAMP=0: the uniform cut for the first segment too (wire_strips.h)
  int wire_copy_streams_ = 2;           // TSG_WIRE_COPY_STREAMS: strip copies alternate over this many copy streams (1 or 2)
  std::mutex wire_mu_;
  std::condition_variable wire_cv_;
  std::vector<std::thread> wire_threads_;
  WireFeed* wire_job_ = nullptr;
  uint64_t wire_gen_ = 0;
  int wire_active_ = 0;                 // packers inside wire_job_
  bool wire_busy_ = false;              // a scan holds the packers
  bool wire_stop_ = false;
  void wire_packer_main();
  // K1Chain drivers poll their readback event yielding instead of sleeping
  // 10 us (TSG_POLL_YIELD), and the confirmer polls the job queue up to
  // pop_spin_us_ before it sleeps (TSG_POP_SPIN_US): a wake-up under the busy
  // confirm pool came 0.1-0.2 ms late; config 2 resident 1838 -> 1920-1945
  // GB/s, config 1 unchanged (profiles/r6a_resident_poll.log)
  bool poll_yield_ = true;
  bool confirm_prefetch_ = true;        // confirm pool: prefetch the next file's result slot and candidate text (TSG_CONFIRM_PREFETCH)
  // confirmations this small run on the calling thread: engine.hip's kInlineConfirm* (a K1 change that re-measures traffic may move them here)
  size_t inline_confirm_files_ = 0;
  uint64_t inline_confirm_bytes_ = 0;
  int pop_spin_us_ = 2000;
  uint32_t k2_hits_per_thread_ = 1;     // K2 grid: hits of the fullest region per thread (TSG_K2_HITS_PER_THREAD)
  bool k2_stats_ = false;               // TSG_K2_STATS=1: per-rule K2 counters, printed to stderr at destruction
  int k2_abl_ = 0;                      // TSG_K2_ABL (probe library): K2 trace / no-walk measurement builds
  bool host_profile_ = false;           // TSG_HOST_PROFILE=1: per-segment host confirm breakdown on stderr
  std::atomic<uint32_t> inject_fail_{0};
  std::atomic<bool> keep_raw_{false};
  std::atomic<bool> keep_gather_{false};
  uint64_t cand_cap0_ = 0;              // a fresh lane's candidate capacity (TSG_CAND_CAP); 0 = the lane's default
  uint64_t tar_gather_cap_ = 0;         // the device tar walk's first gather capacity in bytes (TSG_TAR_GATHER_CAP); 0 = 1/16 of the blocks + 1024
  uint64_t gather_cap_ = 0;             // a gather buffer's first capacity in bytes (TSG_GATHER_CAP); 0 = bytes / 8 + 1 MiB
  std::mutex k2s_mu_;
  std::vector<unsigned long long> k2s_;  // 4 per rule: hits, past the keyword gate, verify starts, bytes walked
  SegmentPolicy seg_;                   // where a batch is cut (segments.h: TSG_PIECES, TSG_SEGMENT_BYTES, ...)
};

int device_count();

// Test hook (tsg_test_readback): tsg_readback of min(nwords, count * per_count)
// dwords of a device buffer holding 1, 2, ... into host-mapped memory on
// device 0; *copied = the dwords that arrived.
bool readback_probe(uint32_t nwords, uint32_t count, uint32_t per_count, uint32_t* copied, std::string* err);

}  // namespace tsg
