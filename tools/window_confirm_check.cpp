// Stand-alone sanitizer run of the windowed confirmation (host code only; no
// GPU): the CPU model of the device-only scan with windows
// (tsg_scan_device_model_opts) over the corpora tools/window_confirm_check.py
// dumps from tests/_window_corpus.py.  The model copies every gathered run
// into an allocation of exactly its bytes and frees the batch before the
// confirmation, so under AddressSanitizer a read of scan_file_windows,
// WindowView or find_all_windows into a hole, past a run or through the
// batch's old address is a read outside an allocation.  Each corpus must give
// the findings and the insufficient files the dump states.
//
//   window_confirm_check <dump file>
//
// Dump: "WCC1", uint32 ncorpora, then per corpus: string name, string config
// JSON ("" = builtin rules), uint32 chunk, before, after, uint64 min_file,
// uint32 nfiles, per file (string path, uint8 binary, string content), uint32
// n + n x uint32 insufficient files, string findings JSON (tsg_result_json).
// string = uint64 length + bytes; little endian.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <pthread.h>
#include <string>
#include <vector>

#include "../include/trivy_secret.h"
#include "../include/trivy_secret_test.h"

namespace {

struct Reader {
  std::ifstream in;
  bool ok = true;
  template <typename T> T num() {
    T v{};
    if (!in.read(reinterpret_cast<char*>(&v), sizeof(v))) ok = false;
    return v;
  }
  std::string str() {
    const uint64_t n = num<uint64_t>();
    std::string s;
    if (!ok || n > (1ull << 32)) { ok = false; return s; }
    s.resize(n);
    if (n && !in.read(&s[0], static_cast<std::streamsize>(n))) ok = false;
    return s;
  }
};

int fail(const std::string& what) {
  std::fprintf(stderr, "window_confirm_check: %s: %s\n", what.c_str(), tsg_last_error());
  return 1;
}

struct Gone { uint8_t** batch; };
void release_batch(void* user) {
  Gone* g = static_cast<Gone*>(user);
  std::free(*g->batch);            // the confirmation may not read the batch: a stray read is a use after free
  *g->batch = nullptr;
}

}  // namespace

static int run(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: window_confirm_check <dump file>\n"); return 2; }
  Reader r;
  r.in.open(argv[1], std::ios::binary);
  char magic[4] = {};
  if (!r.in.read(magic, 4) || std::memcmp(magic, "WCC1", 4) != 0) { std::fprintf(stderr, "bad dump\n"); return 2; }
  const uint32_t ncorpora = r.num<uint32_t>();
  for (uint32_t c = 0; c < ncorpora && r.ok; ++c) {
    const std::string name = r.str(), cfg = r.str();
    tsg_device_scan_opts opts{};
    const uint32_t chunk = r.num<uint32_t>();
    opts.window_before = r.num<uint32_t>();
    opts.window_after = r.num<uint32_t>();
    opts.window_min_file = r.num<uint64_t>();
    const uint32_t nfiles = r.num<uint32_t>();
    std::vector<std::string> paths(nfiles), contents(nfiles);
    std::vector<uint8_t> binary(nfiles ? nfiles : 1, 0);
    for (uint32_t f = 0; f < nfiles; ++f) { paths[f] = r.str(); binary[f] = r.num<uint8_t>(); contents[f] = r.str(); }
    std::vector<uint32_t> want_short(r.num<uint32_t>());
    for (uint32_t& f : want_short) f = r.num<uint32_t>();
    const std::string want_json = r.str();
    if (!r.ok) break;
    std::vector<uint64_t> off(nfiles + 1, 0);
    for (uint32_t f = 0; f < nfiles; ++f) off[f + 1] = off[f] + contents[f].size();
    // the batch in an allocation of exactly its size
    uint8_t* batch = static_cast<uint8_t*>(std::malloc(off[nfiles] ? off[nfiles] : 1));
    for (uint32_t f = 0; f < nfiles; ++f) std::memcpy(batch + off[f], contents[f].data(), contents[f].size());
    std::vector<const char*> pp(nfiles);
    std::vector<uint32_t> pl(nfiles);
    for (uint32_t f = 0; f < nfiles; ++f) { pp[f] = paths[f].data(); pl[f] = static_cast<uint32_t>(paths[f].size()); }
    tsg_ruleset* rs = nullptr;
    if (tsg_ruleset_compile(cfg.empty() ? nullptr : cfg.data(), cfg.size(), &rs) != 0) return fail(name + ": ruleset");
    Gone gone{&batch};
    tsg_result* res = nullptr;
    if (tsg_scan_device_model_opts(rs, batch, off.data(), nfiles, pp.data(), pl.data(), binary.data(), chunk, &opts,
                                   release_batch, &gone, &res) != 0)
      return fail(name + ": tsg_scan_device_model_opts");
    if (batch) { std::fprintf(stderr, "%s: the batch was not released\n", name.c_str()); return 1; }
    char* json = nullptr;
    size_t jn = 0;
    if (tsg_result_json(res, &json, &jn) != 0) return fail(name + ": tsg_result_json");
    const bool same = std::string(json, jn) == want_json;
    tsg_free(json);
    tsg_window_segment ws{};
    if (tsg_result_window_segment(res, 0, &ws) != 0) return fail(name + ": tsg_result_window_segment");
    const bool same_short = ws.ninsufficient == want_short.size() &&
                            (want_short.empty() || std::memcmp(ws.insufficient, want_short.data(), 4 * want_short.size()) == 0);
    uint64_t wf = 0, wr = 0, wb = 0, ff = 0, fb = 0;
    tsg_result_gather_window_stats(res, &wf, &wr, &wb, &ff, &fb);
    std::printf("%-14s chunk %u window %u/%u/%llu: %u files, %llu windowed in %llu runs, %llu bytes, %llu fell back "
                "(%llu bytes); findings %s, insufficient set %s\n", name.c_str(), chunk, opts.window_before,
                opts.window_after, static_cast<unsigned long long>(opts.window_min_file), nfiles,
                static_cast<unsigned long long>(wf), static_cast<unsigned long long>(wr),
                static_cast<unsigned long long>(wb), static_cast<unsigned long long>(ff),
                static_cast<unsigned long long>(fb), same ? "equal" : "DIFFER", same_short ? "equal" : "DIFFERS");
    tsg_result_free(res);
    tsg_ruleset_free(rs);
    if (!same || !same_short) return 1;
  }
  if (!r.ok) { std::fprintf(stderr, "truncated dump\n"); return 2; }
  std::printf("window_confirm_check: %u corpora, no sanitizer report\n", ncorpora);
  return 0;
}

// Regexp compile recurses once per nesting level (x{0,N} becomes N nested
// quests) and the sanitizer's redzones make each frame several times larger:
// the run gets a 1 GiB stack, as tools/asan_driver.cpp's does.
struct Args { int argc; char** argv; int rc; };
static void* run_thread(void* p) {
  Args* a = static_cast<Args*>(p);
  a->rc = run(a->argc, a->argv);
  return nullptr;
}

int main(int argc, char** argv) {
  Args a{argc, argv, 1};
  pthread_attr_t at;
  pthread_attr_init(&at);
  pthread_attr_setstacksize(&at, size_t(1) << 30);
  pthread_t t;
  if (pthread_create(&t, &at, run_thread, &a) != 0) return 2;
  pthread_join(t, nullptr);
  return a.rc;
}
