// The host confirmation: a segment's GPU candidates into findings, and the
// CPU model of the device-only scan.  It indexes arrays with values that came
// back from the device, so it is host C++ that runs under the host sanitizers.
#include "confirm.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <type_traits>

#include "engine.h"

namespace tsg {

CallCtx* Engine::acquire_call() {
  std::lock_guard<std::mutex> lk(call_mu_);
  const int nt = threads_ > 0 ? threads_ : static_cast<int>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
  CallCtx* cc = nullptr;
  if (!free_calls_.empty()) {
    cc = free_calls_.back();
    free_calls_.pop_back();
  } else {
    calls_.emplace_back(new CallCtx());
    cc = calls_.back().get();
  }
  cc->nt = nt;                                   // (the pool itself starts on first use: CallCtx::get)
  return cc;
}

void Engine::release_call(CallCtx* cc) {
  std::lock_guard<std::mutex> lk(call_mu_);
  free_calls_.push_back(cc);
}

std::vector<uint8_t> Engine::windowable_rows() const {
  std::vector<uint8_t> w(pf_.rules.size(), 0);
  for (size_t r = 0; r < pf_.rules.size() && r < rs_->rules.size(); ++r)
    w[r] = (pf_.rules[r].mode == 0 || pf_.rules[r].mode == 4) && pf_.rules[r].gate_on_gpu;
  return w;
}

static_assert(sizeof(GatherCand) == sizeof(Cand) && offsetof(GatherCand, start) == offsetof(Cand, start) &&
              offsetof(GatherCand, rule) == offsetof(Cand, rule), "plan_gather_windows reads the host's candidates");

bool Engine::model_scan_device(const BatchInput& in, uint32_t chunk, SecretVec* results, ScanStats* st, std::string* err,
                               RawScan* raw, const std::function<void()>* before_confirm, const GatherWindowOpts* win) {
  if (!in.h_data || !in.offsets || !in.paths || chunk == 0) { *err = "model_scan_device: NULL argument"; return false; }
  const uint32_t nfiles = in.nfiles;
  const uint64_t total = nfiles ? in.offsets[nfiles] : 0;
  // the GPU passes' outputs as the table model gives them: candidates, file
  // flags, '\n' per chunk
  SegmentOut g;
  g.chunk = chunk;
  g.ff.assign(nfiles, 0);
  g.nl.assign((total + chunk - 1) / chunk, 0);
  for (uint64_t x = 0; x < total; ++x) g.nl[x / chunk] += in.h_data[x] == '\n';
  bool all = false;
  for (const auto& pr : pf_.rules) all = all || pr.mode == 1;
  std::vector<uint8_t> need(nfiles, 0);
  for (uint32_t f = 0; f < nfiles; ++f) {
    std::vector<std::vector<uint64_t>> cand;
    std::vector<uint8_t> gate;
    if (prefilter_reference_file(pf_, in.h_data + in.offsets[f], in.offsets[f + 1] - in.offsets[f], &cand, &gate))
      g.ff[f] = kFileFoldSpecial;
    for (size_t r = 0; r < cand.size(); ++r)
      for (uint64_t s : cand[r]) g.cands.push_back(Cand{f, static_cast<uint32_t>(r), s});
    need[f] = all || g.ff[f] || std::any_of(cand.begin(), cand.end(), [](const std::vector<uint64_t>& v) { return !v.empty(); });
  }
  if (win && win->on()) return model_scan_windows(in, chunk, g, all, *win, results, st, err, raw, before_confirm);
  // the gather: plan_gather's layout, the runs copied byte for byte into a
  // buffer of exactly gather_total bytes (so a read outside a run is a read
  // outside an allocation)
  GatherPlan gp;
  plan_gather(in.offsets, nfiles, 0, need.data(), chunk, &gp);
  std::vector<uint8_t> buf(gp.total);
  for (const GatherRun& r : gp.runs) std::memcpy(buf.data() + r.dst, in.h_data + r.src, r.len);
  g.gbase = buf.data();
  g.gathered = true;
  g.gather_total = gp.total;
  g.goff = gp.goff;
  // the confirmation of a device-only segment: no host copy of the batch
  Segment sg;
  sg.in = in;
  sg.in.h_data = nullptr;
  sg.bytes = total;
  if (before_confirm && *before_confirm) (*before_confirm)();    // (the caller's batch may be gone from here on)
  results->clear();
  results->resize(nfiles);
  uint64_t nconf = 0, nfind = 0;
  CallCtx* cc = acquire_call();
  try {
    confirm_segment(*cc, sg, g, results->data(), &nconf, &nfind, false);
  } catch (const std::exception& x) {
    release_call(cc);
    *err = x.what();
    return false;
  }
  release_call(cc);
  if (st) {
    *st = ScanStats();
    st->bytes = total;
    st->files = nfiles;
    st->confirm_files = nconf;
    st->findings = nfind;
    st->chunk_bytes = chunk;
    st->gather_files = g.gather_files;
    st->gather_bytes = gp.total;
    st->gather_runs = gp.runs.size();
  }
  if (raw) {
    *raw = RawScan();
    raw->segs.resize(1);
    RawSegment& rec = raw->segs[0];
    rec.nfiles = nfiles;
    rec.bytes = total;
    rec.chunk = chunk;
    rec.need = need;
    rec.goff = gp.goff;
    rec.runs = gp.runs;
    rec.gather_total = gp.total;
    rec.gathered = buf;
  }
  return true;
}

// model_scan_device with windows: g holds the table model's GPU outputs.
bool Engine::model_scan_windows(const BatchInput& in, uint32_t chunk, SegmentOut& g, bool all, const GatherWindowOpts& win,
                                SecretVec* results, ScanStats* st, std::string* err, RawScan* raw,
                                const std::function<void()>* before_confirm) {
  const uint32_t nfiles = in.nfiles;
  const uint64_t total = nfiles ? in.offsets[nfiles] : 0;
  const std::vector<uint8_t> wrows = windowable_rows();
  GatherWindowPlan wp;
  plan_gather_windows(in.offsets, nfiles, 0, reinterpret_cast<const GatherCand*>(g.cands.data()), g.cands.size(),
                      g.ff.data(), all, wrows.data(), static_cast<uint32_t>(wrows.size()), chunk, win, &wp, in.h_data);
  // every run in an allocation of exactly its bytes
  std::vector<std::vector<uint8_t>> run_bytes(wp.runs.size());
  for (size_t k = 0; k < wp.runs.size(); ++k) {
    run_bytes[k].assign(in.h_data + wp.runs[k].src, in.h_data + wp.runs[k].src + wp.runs[k].len);
    g.run_base.push_back(run_bytes[k].data());
  }
  g.gathered = true;
  g.windowed = true;
  g.gather_total = wp.total;
  g.gcls = wp.cls;
  g.wruns = wp.runs;
  // the fallback's gather is planned and copied here, while the batch may
  // still be read: over every windowed file, of which the round takes its own
  std::vector<uint8_t> wneed(nfiles, 0);
  for (uint32_t f = 0; f < nfiles; ++f) wneed[f] = wp.cls[f] == kGatherClassWindow;
  std::vector<std::vector<uint8_t>> whole_bytes(nfiles);
  for (uint32_t f = 0; f < nfiles; ++f)
    if (wneed[f]) {
      const uint64_t src = in.offsets[f] / chunk * chunk;
      whole_bytes[f].assign(in.h_data + src, in.h_data + in.offsets[f + 1]);
    }
  Segment sg;
  sg.in = in;
  sg.in.h_data = nullptr;
  sg.bytes = total;
  if (before_confirm && *before_confirm) (*before_confirm)();
  results->clear();
  results->resize(nfiles);
  uint64_t nconf = 0, nfind = 0;
  GatherPlan fp;
  std::vector<uint8_t> fbuf;
  std::vector<uint32_t> insufficient;
  std::vector<uint64_t> goff1;               // the windowed round's (the fallback round replaces g.goff)
  CallCtx* cc = acquire_call();
  try {
    confirm_segment(*cc, sg, g, results->data(), &nconf, &nfind, false);
    insufficient = g.insufficient;
    goff1 = g.goff;
    if (!insufficient.empty()) {
      std::vector<uint8_t> need(nfiles, 0);
      for (uint32_t f : insufficient) need[f] = 1;
      plan_gather(in.offsets, nfiles, 0, need.data(), chunk, &fp);
      fbuf.assign(fp.total, 0);
      // (a run of adjacent insufficient files: each file's bytes from its own copy)
      for (uint32_t f : insufficient) {
        const uint64_t head = in.offsets[f] % chunk;
        const uint64_t d0 = fp.goff[f] - head;
        // the head bytes only where this file starts a run (else they are the previous file's)
        const bool first = f == 0 || !need[f - 1];
        const uint8_t* sp = whole_bytes[f].data();
        if (first) std::memcpy(fbuf.data() + d0, sp, whole_bytes[f].size());
        else std::memcpy(fbuf.data() + fp.goff[f], sp + head, whole_bytes[f].size() - head);
      }
      confirm_fallback(*cc, sg, g, fp, fbuf.data(), results->data(), &nconf, &nfind);
    }
  } catch (const std::exception& x) {
    release_call(cc);
    *err = x.what();
    return false;
  }
  release_call(cc);
  if (st) {
    *st = ScanStats();
    st->bytes = total;
    st->files = nfiles;
    st->confirm_files = nconf;
    st->findings = nfind;
    st->chunk_bytes = chunk;
    st->gather_files = g.gather_files;
    st->gather_bytes = wp.total + fp.total;
    st->gather_runs = wp.runs.size() + fp.runs.size();
    st->window_files = g.window_files;
    st->window_runs = wp.runs.size();
    st->window_bytes = wp.total;
    st->fallback_files = insufficient.size();
    st->fallback_bytes = fp.total;
    st->line_widened = wp.widened;
    st->line_capped = wp.capped;
  }
  if (raw) {
    *raw = RawScan();
    raw->segs.resize(2);
    RawSegment& rec = raw->segs[0];
    rec.nfiles = nfiles;
    rec.bytes = total;
    rec.chunk = chunk;
    rec.cls = wp.cls;
    rec.need.assign(nfiles, 0);
    for (uint32_t f = 0; f < nfiles; ++f) rec.need[f] = wp.cls[f] != kGatherClassNone;
    rec.goff = goff1;
    rec.runs = wp.runs;
    rec.gather_total = wp.total;
    rec.gathered.assign(wp.total, 0);
    for (size_t k = 0; k < wp.runs.size(); ++k)
      std::memcpy(rec.gathered.data() + wp.runs[k].dst, run_bytes[k].data(), wp.runs[k].len);
    rec.insufficient = insufficient;
    RawSegment& fb = raw->segs[1];
    fb.nfiles = nfiles;
    fb.bytes = total;
    fb.chunk = chunk;
    fb.need.assign(nfiles, 0);
    for (uint32_t f : insufficient) fb.need[f] = 1;
    fb.goff = fp.goff;
    fb.goff.resize(nfiles, kGatherNone);
    fb.runs = fp.runs;
    fb.gather_total = fp.total;
    fb.gathered = fbuf;
  }
  return true;
}

void Engine::confirm_fallback(CallCtx& cc, const Segment& sg, SegmentOut& g, const GatherPlan& gp, const uint8_t* gbase,
                              Secret* results, uint64_t* nconf, uint64_t* nfind) {
  g.work = g.insufficient;
  g.light.clear();
  g.insufficient.clear();
  g.windowed = false;
  g.run_base.clear();
  g.goff = gp.goff;
  g.gbase = gbase;
  g.gather_total = gp.total;
  const uint64_t files = g.gather_files, wfiles = g.window_files;
  confirm_segment(cc, sg, g, results, nconf, nfind, false);
  g.gather_files = files;                  // (the first round's count stands: these files were among them)
  g.window_files = wfiles - g.work.size();
}

// Host confirmation of one segment (files [0, in.nfiles) of sg.in, results
// into results[0..nfiles)) from that segment's GPU output `g`.
void Engine::plan_confirm(const Segment& sg, SegmentOut* gp) const {
  SegmentOut& g = *gp;
  const BatchInput& in = sg.in;
  const size_t nr = rs_->rules.size();
  // group candidates per file (counting sort by file, then sort each file's list)
  g.per_file.assign(in.nfiles + 1, 0);
  for (const Cand& c : g.cands) g.per_file[c.file + 1]++;
  for (uint32_t f = 0; f < in.nfiles; ++f) g.per_file[f + 1] += g.per_file[f];
  g.sorted.resize(g.cands.size());
  {
    std::vector<uint32_t> pos(g.per_file.begin(), g.per_file.end() - 1);
    for (const Cand& c : g.cands) g.sorted[pos[c.file]++] = c;
  }
  bool any_full = false;
  for (size_t r = 0; r < nr; ++r) if (pf_.rules[r].mode == 1) any_full = true;
  // files to confirm (candidates, fold-special content, or host-evaluated
  // rules), largest first (LPT: the per-file confirm cost grows with size);
  // every other file only needs the global allow-path outcome and is handled
  // in blocks after them (image layers: hundreds of thousands of such files)
  g.work.clear();
  g.light.clear();
  g.work.reserve(in.nfiles / 4 + 16);
  for (uint32_t f = sg.lead; f < in.nfiles; ++f) {
    if (any_full || g.ff[f] || g.per_file[f] != g.per_file[f + 1]) g.work.push_back(f);
    else g.light.push_back(f);
  }
  // largest first, by power-of-two size class (a counting sort: a full sort
  // of config 5's 13k files per piece cost ~1 ms on the confirming thread;
  // LPT within a factor of two balances the pool as well)
  {
    uint32_t cnt[65] = {};
    auto cls = [&](uint32_t f) {
      const uint64_t n = in.offsets[f + 1] - in.offsets[f];
      return 63 - __builtin_clzll(n + 1);           // 0..63
    };
    for (uint32_t f : g.work) ++cnt[63 - cls(f) + 1];
    for (int k = 1; k <= 64; ++k) cnt[k] += cnt[k - 1];
    std::vector<uint32_t> by(g.work.size());
    for (uint32_t f : g.work) by[cnt[63 - cls(f)]++] = f;
    g.work.swap(by);
  }
  g.planned = true;
}

namespace {

// Where the confirmer reads a segment's bytes -- the only reader of
// BatchInput::h_data on the confirm path: the caller's host copy
// (std::false_type), or a device-only scan's gather buffer through the
// device's goff (std::true_type).  The confirm worker is instantiated once per
// source, so neither pays a branch per file for the other.
struct FromWindows {};     // a device-only scan's gather with windows: whole files through goff, the rest through runs
struct ConfirmBytes {
  const uint8_t* h;
  const uint64_t* off;
  const uint8_t* gbuf;
  const uint64_t* goff;
  const uint8_t* const* fptr;     // FromWindows, the CPU model: per whole file, its bytes in its run's allocation
  const uint8_t* content(std::false_type, uint32_t f) const { return h + off[f]; }
  const uint8_t* content(std::true_type, uint32_t f) const { return gbuf + goff[f]; }
  const uint8_t* content(FromWindows, uint32_t f) const { return fptr ? fptr[f] : gbuf + goff[f]; }
  // K1's newline counts are per chunk of the segment's frame; prefix_at also
  // reads the bytes between the chunk boundary below the file and the file
  void newlines(std::false_type, uint32_t f, uint32_t, NlSource* n) const {
    n->data = h;
    n->file_off = off[f];
  }
  // (the gather starts every run on that boundary, so the head bytes are in
  // the buffer in front of the file: no pointer outside it is formed)
  void newlines(std::true_type, uint32_t f, uint32_t chunk, NlSource* n) const {
    const uint64_t head = off[f] % chunk;
    n->data = gbuf + (goff[f] - head);
    n->data_off = off[f] - head;
    n->file_off = off[f];
  }
  void newlines(FromWindows, uint32_t f, uint32_t chunk, NlSource* n) const {
    const uint64_t head = off[f] % chunk;
    n->data = content(FromWindows(), f) - head;
    n->data_off = off[f] - head;
    n->file_off = off[f];
  }
};

}  // namespace

void Engine::confirm_segment(CallCtx& cc, const Segment& sg, SegmentOut& g, Secret* results, uint64_t* nconf_out,
                             uint64_t* nfind_out, bool gpu_in_flight) {
  const BatchInput& in = sg.in;
  const Ruleset& rs = *rs_;
  const size_t nplan = pf_.rules.size();   // rules + exclude-block pseudo-rules
  const auto t_begin = std::chrono::steady_clock::now();
  if (!g.planned) plan_confirm(sg, &g);
  if (g.gathered && g.windowed) prepare_windows(sg, &g);
  // (the CPU model's runs live in allocations of their own: a whole file's
  // bytes are then addressed through a per-file pointer into its run's)
  std::vector<const uint8_t*> file_base;
  if (g.gathered && g.windowed && !g.run_base.empty()) {
    file_base.assign(in.nfiles, reinterpret_cast<const uint8_t*>(""));
    for (uint32_t f = sg.lead; f < in.nfiles; ++f) {
      if (g.gcls[f] != kGatherClassWhole) continue;
      const uint32_t k = gather_run_of(g.wruns.data(), g.wruns.size(), in.offsets[f] / g.chunk * g.chunk);
      if (k != kGatherNoRun) file_base[f] = g.run_base[k] + (in.offsets[f] - g.wruns[k].src);   // (else: empty, past the last chunk)
    }
  }
  const ConfirmBytes src{in.h_data, in.offsets, g.gbase, g.goff.data(), file_base.empty() ? nullptr : file_base.data()};
  if (g.gathered && g.windowed) {
    uint64_t nf = 0, nw = 0;
    for (uint32_t f = sg.lead; f < in.nfiles; ++f) { nf += g.gcls[f] != kGatherClassNone; nw += g.gcls[f] == kGatherClassWindow; }
    g.gather_files = nf;
    g.window_files = nw;
    for (uint32_t f : g.work)
      if (g.gcls[f] == kGatherClassNone) throw std::runtime_error("device-only scan: a file the confirmer reads was not gathered");
  } else if (g.gathered) {
    // a file to confirm that the device did not gather (or placed outside
    // what it gathered) fails the call: it is never scanned from wrong bytes
    if (g.goff.size() != in.nfiles || (!g.gbase && g.gather_total)) throw std::runtime_error("device-only scan: no gather for the segment");
    for (uint32_t f : g.work) {
      const uint64_t o = g.goff[f], head = in.offsets[f] % g.chunk;
      if (o == kGatherNone || o < head || o > g.gather_total || in.offsets[f + 1] - in.offsets[f] > g.gather_total - o)
        throw std::runtime_error("device-only scan: a file the confirmer reads was not gathered");
    }
    uint64_t nf = 0;
    for (uint32_t f = sg.lead; f < in.nfiles; ++f) nf += g.goff[f] != kGatherNone;
    g.gather_files = nf;
  } else if (!in.h_data && !g.work.empty()) {
    throw std::runtime_error("scan without a host copy of the batch and without a gather");
  }
  const std::vector<uint32_t>& per_file = g.per_file;
  std::vector<Cand>& sorted = g.sorted;
  const std::vector<uint32_t>& work = g.work;
  const std::vector<uint32_t>& light = g.light;
  // the plan every confirmed file starts from, and its mode-1 rules
  std::vector<uint8_t> kind0(nplan, kPlanNoMatch);
  std::vector<uint32_t> full_rules;
  for (size_t r = 0; r < nplan; ++r) {
    if (pf_.rules[r].mode == 1) {            // (mode 3: only with a presence candidate)
      kind0[r] = kPlanFull;
      full_rules.push_back(static_cast<uint32_t>(r));
    }
  }
  results -= sg.lead;                      // results[f] for the piece's files f >= lead
  constexpr uint32_t kLightBlock = 512;
  const uint32_t nlight_blocks = static_cast<uint32_t>((light.size() + kLightBlock - 1) / kLightBlock);
  std::atomic<uint32_t> next_light{0};
  std::atomic<uint32_t> next{0};
  std::atomic<uint64_t> nfind{0}, nconf{0};
  // TSG_HOST_PROFILE: worker thread-ns in the plan (candidates sorted and
  // grouped), scan_file and storing the result
  std::atomic<uint64_t> ph_plan{0}, ph_scan{0}, ph_store{0};
  const bool prof = host_profile_;
  auto light_files = [&]() {
    for (;;) {
      const uint32_t b = next_light.fetch_add(1);
      if (b >= nlight_blocks) break;
      const size_t e = std::min<size_t>(light.size(), (static_cast<size_t>(b) + 1) * kLightBlock);
      for (size_t k = static_cast<size_t>(b) * kLightBlock; k < e; ++k) {
        const uint32_t f = light[k];
        if (confirm_prefetch_ && k + 8 < e) __builtin_prefetch(in.paths[light[k + 8]]);   // (path strings: scattered)
        // no candidates, no host-evaluated rule: only the global allow-path outcome remains
        const char* p = in.paths[f];
        const size_t pn = in.path_lens ? in.path_lens[f] : std::strlen(p);
        if (global_allow_path(rs, reinterpret_cast<const uint8_t*>(p), pn)) results[f] = Secret::path_only(p, pn);
      }
    }
  };
  std::mutex short_mu;
  g.insufficient.clear();
  // run k's bytes
  auto run_ptr = [&](uint32_t k) { return g.run_base.empty() ? g.gbase + g.wruns[k].dst : g.run_base[k]; };
  auto worker = [&](auto from) {               // from: where the bytes are (ConfirmBytes)
    FilePlan plan;
    std::vector<std::vector<uint64_t>> spare;
    std::vector<WindowRun> wruns;
    std::vector<uint32_t> my_short;            // windowed files found insufficient
    // per-thread counts and work taken a few files at a time: 15 threads
    // hitting shared counters once per file serialised on their cache lines
    uint64_t my_conf = 0, my_find = 0, my_plan = 0, my_scan = 0, my_store = 0;
    constexpr uint32_t kTake = 4;
    uint32_t wi = 0, wend = 0;
    for (;;) {
      if (wi == wend) {
        wi = next.fetch_add(kTake);
        if (wi >= work.size()) break;
        wend = std::min<uint32_t>(wi + kTake, static_cast<uint32_t>(work.size()));
      }
      uint32_t f = work[wi++];
      if (confirm_prefetch_ && wi < wend && !std::is_same<decltype(from), FromWindows>::value) {
        // the next file of this take: its result slot and the text at its
        // first candidate starts, fetched while this file is confirmed (the
        // host has not touched the batch's bytes since they were written):
        // resident config 5 602-611 -> 614-657 GB/s (profiles/r6j_confirm_prefetch_c5.log; two files
        // ahead and a wider window were no better)
        const uint32_t fn = work[wi];
        __builtin_prefetch(results + fn, 1);
        __builtin_prefetch(in.paths[fn]);
        const uint8_t* cn = src.content(from, fn);
        const uint64_t ln = in.offsets[fn + 1] - in.offsets[fn];
        for (uint32_t k = per_file[fn], ke = std::min(per_file[fn + 1], per_file[fn] + 4); k < ke; ++k) {
          const uint64_t st = sorted[k].start;
          if (st < ln) {
            __builtin_prefetch(cn + st);
            if (st + 64 < ln) __builtin_prefetch(cn + st + 64);
          }
        }
      }
      const auto tp0 = prof ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
      const char* path_p = in.paths[f];
      const size_t path_n = in.path_lens ? in.path_lens[f] : std::strlen(path_p);
      const bool in_windows = std::is_same<decltype(from), FromWindows>::value && g.gcls[f] == kGatherClassWindow;
      const uint8_t* content = in_windows ? nullptr : src.content(from, f);
      const size_t len = in.offsets[f + 1] - in.offsets[f];
      const bool binary = in.binary ? in.binary[f] != 0 : false;
      const uint32_t cb = per_file[f], ce = per_file[f + 1];
      if (g.ff[f]) {
        // fold-special file (U+0130/U+212A/U+017F present): the two passes run
        // on the host with the variant scan DFA, then the exact confirmer
        ++my_conf;
        std::vector<std::vector<uint64_t>> vc;
        std::vector<uint8_t> vg;
        prefilter_variant_file(pf_, content, len, &vc, &vg);
        plan_from_candidates(pf_, &vc, &plan);
        Secret s = scan_file(rs, path_p, path_n, content, len, binary, &plan);
        my_find += s.findings().size();
        results[f] = std::move(s);
        continue;
      }
      ++my_conf;
      plan.kind = kind0;                       // mode-1 rules kPlanFull, the rest kPlanNoMatch
      for (RuleCandidates& c : plan.cands) {   // start lists are reused from file to file
        c.starts.clear();
        spare.push_back(std::move(c.starts));
      }
      plan.cands.clear();
      std::sort(sorted.begin() + cb, sorted.begin() + ce, [](const Cand& a, const Cand& b) {
        return a.rule != b.rule ? a.rule < b.rule : a.start < b.start;
      });
      for (uint32_t k = cb; k < ce;) {
        uint32_t r = sorted[k].rule;
        RuleCandidates rc;
        rc.rule = r;
        if (!spare.empty()) {
          rc.starts = std::move(spare.back());
          spare.pop_back();
        }
        while (k < ce && sorted[k].rule == r) {
          if (rc.starts.empty() || rc.starts.back() != sorted[k].start) rc.starts.push_back(sorted[k].start);
          ++k;
        }
        // mode 3 presence candidates, and a mode-4 walk that gave up
        // (kFullScanStart sorts last): the rule in full on the host
        plan.kind[r] = pf_.rules[r].mode == 3 || rc.starts.back() == kFullScanStart ? kPlanFull
                     : pf_.rules[r].gate_on_gpu ? kPlanCandidates : kPlanCandHostGate;
        plan.cands.push_back(std::move(rc));
      }
      // the rules scan_file visits: mode-1 rules and those with candidates, ascending
      plan.active.clear();
      plan.active_set = true;
      {
        size_t a = 0, b = 0;
        while (a < full_rules.size() || b < plan.cands.size()) {
          const uint32_t x = a < full_rules.size() ? full_rules[a] : UINT32_MAX;
          const uint32_t y = b < plan.cands.size() ? plan.cands[b].rule : UINT32_MAX;
          if (x <= y) { plan.active.push_back(x); ++a; if (x == y) ++b; }
          else { plan.active.push_back(y); ++b; }
        }
      }
      if (in_windows) {
        // the file's runs: from the one holding its head chunk on
        wruns.clear();
        const uint64_t o0 = in.offsets[f], o1 = in.offsets[f + 1];
        for (uint32_t k = gather_run_of(g.wruns.data(), g.wruns.size(), o0 / g.chunk * g.chunk);
             k != kGatherNoRun && k < g.wruns.size() && g.wruns[k].src < o1; ++k) {
          const GatherRun& r = g.wruns[k];
          const uint64_t a = std::max(r.src, o0), b = std::min(r.src + r.len, o1);
          if (b <= a) continue;
          wruns.push_back(WindowRun{a - o0, b - o0, run_ptr(k) + (a - r.src)});
        }
        WindowFile wf;
        wf.runs = wruns.data();
        wf.nruns = wruns.size();
        wf.len = len;
        wf.chunk_nl = g.nl.data();
        wf.chunk = g.chunk;
        wf.file_off = o0;
        bool insufficient = wruns.empty() || wruns[0].a != 0;
        Secret s;
        if (!insufficient) s = scan_file_windows(rs, path_p, path_n, wf, binary, plan, &insufficient);
        if (insufficient) { --my_conf; my_short.push_back(f); continue; }
        my_find += s.findings().size();
        results[f] = std::move(s);
        continue;
      }
      NlSource nls;
      nls.chunk_nl = g.nl.data();
      src.newlines(from, f, g.chunk, &nls);
      nls.chunk = g.chunk;
      const auto tp1 = prof ? std::chrono::steady_clock::now() : tp0;
      Secret s = scan_file(rs, path_p, path_n, content, len, binary, &plan, &nls);
      const auto tp2 = prof ? std::chrono::steady_clock::now() : tp0;
      my_find += s.findings().size();
      results[f] = std::move(s);
      if (prof) {
        const auto tp3 = std::chrono::steady_clock::now();
        my_plan += std::chrono::duration_cast<std::chrono::nanoseconds>(tp1 - tp0).count();
        my_scan += std::chrono::duration_cast<std::chrono::nanoseconds>(tp2 - tp1).count();
        my_store += std::chrono::duration_cast<std::chrono::nanoseconds>(tp3 - tp2).count();
      }
    }
    nconf.fetch_add(my_conf);
    nfind.fetch_add(my_find);
    if (!my_short.empty()) {
      std::lock_guard<std::mutex> lk(short_mu);
      g.insufficient.insert(g.insufficient.end(), my_short.begin(), my_short.end());
    }
    if (prof) { ph_plan += my_plan; ph_scan += my_scan; ph_store += my_store; }
  };
  // small confirmations (a few files, little text: per-file Scan batches) run
  // on this thread; waking the pool costs more than the work
  uint64_t work_bytes = 0;
  for (size_t k = 0; k < work.size() && work_bytes <= inline_confirm_bytes_; ++k)
    work_bytes += in.offsets[work[k] + 1] - in.offsets[work[k]];
  const bool inline_confirm = work.size() <= inline_confirm_files_ && work_bytes <= inline_confirm_bytes_ &&
                              light.size() <= kLightBlock;
  const int nt = inline_confirm ? 1 : cc.get().size();
  // while GPU passes are in flight one core stays with each thread driving
  // them (a preempted driver thread stalls its GPU)
  const int active = gpu_in_flight && nt > 1 ? nt - 1 : nt;
  const double t_setup = ms_since(t_begin);
  std::atomic<uint64_t> work_us{0}, light_us{0};
  auto body = [&](int idx) {
    if (idx >= active) return;
    auto a = std::chrono::steady_clock::now();
    if (g.gathered && g.windowed) worker(FromWindows());
    else if (g.gathered) worker(std::true_type());
    else worker(std::false_type());
    auto b = std::chrono::steady_clock::now();
    light_files();
    work_us.fetch_add(std::chrono::duration_cast<std::chrono::microseconds>(b - a).count());
    light_us.fetch_add(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - b).count());
  };
  if (inline_confirm) body(0);
  else cc.get().run(body);
  if (host_profile_) {
    uint64_t ph[5];
    for (int k = 0; k < 5; ++k) ph[k] = g_scan_prof[k].exchange(0);
    std::fprintf(stderr, "[tsg host] files %u (work %zu, light %zu) cands %zu: setup %.2f ms, wall %.2f ms, "
                 "work %.1f + light %.1f thread-ms on %d threads (plan %.1f, scan_file %.1f, store %.1f); scan_file "
                 "thread-ms: keywords %.1f, find %.1f, blocks %.1f, findings %.1f, sort %.1f\n", in.nfiles,
                 work.size(), light.size(), g.cands.size(), t_setup, ms_since(t_begin), work_us.load() / 1e3,
                 light_us.load() / 1e3, active, ph_plan.load() / 1e6, ph_scan.load() / 1e6, ph_store.load() / 1e6,
                 ph[0] / 1e6, ph[1] / 1e6, ph[2] / 1e6, ph[3] / 1e6, ph[4] / 1e6);
  }
  std::sort(g.insufficient.begin(), g.insufficient.end());
  *nconf_out += nconf.load();
  *nfind_out += nfind.load();
}

// The windowed gather's tables as they came from the device, checked before
// anything is indexed with them, and goff for the files gathered whole.
void Engine::prepare_windows(const Segment& sg, SegmentOut* gp) const {
  SegmentOut& g = *gp;
  const BatchInput& in = sg.in;
  const uint64_t total = in.nfiles ? in.offsets[in.nfiles] : 0;
  if (g.gcls.size() != in.nfiles || g.chunk == 0 || (!g.gbase && g.run_base.empty() && g.gather_total))
    throw std::runtime_error("device-only scan: no windowed gather for the segment");
  if (!g.run_base.empty() && g.run_base.size() != g.wruns.size())
    throw std::runtime_error("device-only scan: run allocations do not match the run table");
  uint64_t src_end = 0, dst_end = 0;
  for (const GatherRun& r : g.wruns) {
    if (r.len == 0 || r.src < src_end || r.src % g.chunk != 0 || r.len > total || r.src > total - r.len ||
        r.dst < dst_end || r.dst % kGatherAlign != 0 || r.len > g.gather_total || r.dst > g.gather_total - r.len)
      throw std::runtime_error("device-only scan: a gather run outside the segment or the buffer");
    src_end = r.src + r.len;
    dst_end = r.dst + r.len;
  }
  g.goff.assign(in.nfiles, kGatherNone);
  for (uint32_t f = sg.lead; f < in.nfiles; ++f) {
    if (g.gcls[f] > kGatherClassWindow) throw std::runtime_error("device-only scan: a file class out of range");
    if (g.gcls[f] == kGatherClassNone) continue;
    g.goff[f] = 0;
    if (g.gcls[f] != kGatherClassWhole) continue;
    const uint64_t o0 = in.offsets[f], o1 = in.offsets[f + 1], c0 = o0 / g.chunk * g.chunk;
    const uint32_t k = c0 < total ? gather_run_of(g.wruns.data(), g.wruns.size(), c0) : kGatherNoRun;
    if (k == kGatherNoRun) {
      if (o1 != o0 || c0 < total) throw std::runtime_error("device-only scan: a whole file's run is missing");
      g.goff[f] = g.gather_total;
      continue;
    }
    const GatherRun& r = g.wruns[k];
    if (o1 > r.src + r.len) throw std::runtime_error("device-only scan: a whole file reaches past its run");
    g.goff[f] = r.dst + (o0 - r.src);
  }
}

}  // namespace tsg
