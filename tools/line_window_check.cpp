// Stand-alone sanitizer run of the line windows' host code (no GPU): over the
// corpora tools/line_window_check.py dumps from tests/_line_window_corpus.py,
//   tsg_test_plan_gather_lines    the layout with a line cap: gather.h
//                                 line_window on the batch's bytes and, beside
//                                 it, line_window_chunks -- the walk the
//                                 device pass runs -- on the '\n' count per
//                                 chunk; the batch lies in an allocation of
//                                 exactly its size, so a walk that leaves a
//                                 file at the batch's ends is a read outside
//                                 an allocation; the two plans must be equal
//                                 (the hook fails otherwise);
//   tsg_scan_device_model_opts2   the whole-mode model with the cap: every
//                                 gathered run in an allocation of exactly
//                                 its bytes, the batch freed before the
//                                 confirmation, the fallback round.
// Each corpus must give the findings and the insufficient files the dump
// states.
//
//   line_window_check <dump file>
//
// Dump: "LWC1", uint32 ncorpora, then per corpus: string name, string config
// JSON ("" = builtin rules), uint32 chunk, before, after, cap, uint64
// min_file, uint32 nfiles, per file (string path, uint8 binary, string
// content), uint32 n + n x uint32 insufficient files, string findings JSON
// (tsg_result_json), uint32 ncands + per candidate (uint32 file, uint32 rule,
// uint64 start), nfiles x uint32 file flags, uint32 nrows + nrows x uint8
// windowable.  string = uint64 length + bytes; little endian.
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
  std::fprintf(stderr, "line_window_check: %s: %s\n", what.c_str(), tsg_last_error());
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
  if (argc != 2) { std::fprintf(stderr, "usage: line_window_check <dump file>\n"); return 2; }
  Reader r;
  r.in.open(argv[1], std::ios::binary);
  char magic[4] = {};
  if (!r.in.read(magic, 4) || std::memcmp(magic, "LWC1", 4) != 0) { std::fprintf(stderr, "bad dump\n"); return 2; }
  const uint32_t ncorpora = r.num<uint32_t>();
  for (uint32_t c = 0; c < ncorpora && r.ok; ++c) {
    const std::string name = r.str(), cfg = r.str();
    tsg_device_scan_opts2 opts{};
    opts.struct_size = sizeof(opts);
    const uint32_t chunk = r.num<uint32_t>();
    opts.window_before = r.num<uint32_t>();
    opts.window_after = r.num<uint32_t>();
    opts.window_line_cap = r.num<uint32_t>();
    opts.window_min_file = r.num<uint64_t>();
    const uint32_t nfiles = r.num<uint32_t>();
    std::vector<std::string> paths(nfiles), contents(nfiles);
    std::vector<uint8_t> binary(nfiles ? nfiles : 1, 0);
    for (uint32_t f = 0; f < nfiles; ++f) { paths[f] = r.str(); binary[f] = r.num<uint8_t>(); contents[f] = r.str(); }
    std::vector<uint32_t> want_short(r.num<uint32_t>());
    for (uint32_t& f : want_short) f = r.num<uint32_t>();
    const std::string want_json = r.str();
    const uint32_t ncands = r.num<uint32_t>();
    if (!r.ok || ncands > (1u << 24)) { r.ok = false; break; }
    std::vector<uint32_t> cf(ncands ? ncands : 1), cr(ncands ? ncands : 1);
    std::vector<uint64_t> cs(ncands ? ncands : 1);
    for (uint32_t k = 0; k < ncands; ++k) { cf[k] = r.num<uint32_t>(); cr[k] = r.num<uint32_t>(); cs[k] = r.num<uint64_t>(); }
    std::vector<uint32_t> fflags(nfiles ? nfiles : 1, 0);
    for (uint32_t f = 0; f < nfiles; ++f) fflags[f] = r.num<uint32_t>();
    const uint32_t nrows = r.num<uint32_t>();
    if (!r.ok || nrows > (1u << 20)) { r.ok = false; break; }
    std::vector<uint8_t> rows(nrows ? nrows : 1, 0);
    for (uint32_t k = 0; k < nrows; ++k) rows[k] = r.num<uint8_t>();
    if (!r.ok) break;
    std::vector<uint64_t> off(nfiles + 1, 0);
    for (uint32_t f = 0; f < nfiles; ++f) off[f + 1] = off[f] + contents[f].size();
    // the batch in an allocation of exactly its size
    uint8_t* batch = static_cast<uint8_t*>(std::malloc(off[nfiles] ? off[nfiles] : 1));
    for (uint32_t f = 0; f < nfiles; ++f) std::memcpy(batch + off[f], contents[f].data(), contents[f].size());
    // the layout: the byte model and the table walk
    const uint64_t nchunks = (off[nfiles] + chunk - 1) / chunk;
    std::vector<uint8_t> cls(nfiles ? nfiles : 1), marks(nchunks ? nchunks : 1);
    std::vector<uint32_t> first(nfiles ? nfiles : 1);
    std::vector<uint64_t> runs(3 * (nchunks / 2 + 2));
    size_t nruns = 0;
    uint64_t total = 0, widened = 0, capped = 0;
    if (tsg_test_plan_gather_lines(batch, off.data(), nfiles, 0, cf.data(), cr.data(), cs.data(), ncands, fflags.data(), 0,
                                   rows.data(), nrows, chunk, &opts, cls.data(), first.data(), marks.data(), runs.data(),
                                   nchunks / 2 + 2, &nruns, &total, &widened, &capped) != 0)
      return fail(name + ": tsg_test_plan_gather_lines");
    std::vector<const char*> pp(nfiles);
    std::vector<uint32_t> pl(nfiles);
    for (uint32_t f = 0; f < nfiles; ++f) { pp[f] = paths[f].data(); pl[f] = static_cast<uint32_t>(paths[f].size()); }
    tsg_ruleset* rs = nullptr;
    if (tsg_ruleset_compile(cfg.empty() ? nullptr : cfg.data(), cfg.size(), &rs) != 0) return fail(name + ": ruleset");
    Gone gone{&batch};
    tsg_result* res = nullptr;
    if (tsg_scan_device_model_opts2(rs, batch, off.data(), nfiles, pp.data(), pl.data(), binary.data(), chunk, &opts,
                                    release_batch, &gone, &res) != 0)
      return fail(name + ": tsg_scan_device_model_opts2");
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
    uint64_t wf = 0, wr = 0, wb = 0, ff = 0, fb = 0, lw = 0, lc = 0;
    tsg_result_gather_window_stats(res, &wf, &wr, &wb, &ff, &fb);
    tsg_result_gather_line_stats(res, &lw, &lc, nullptr);
    const bool same_plan = wr == nruns && wb == total && lw == widened && lc == capped;
    std::printf("%-17s chunk %u window %u/%u/%llu cap %u: %u files, %llu windowed in %llu runs, %llu bytes, %llu widened, "
                "%llu capped, %llu fell back (%llu bytes); findings %s, insufficient set %s, layout %s\n", name.c_str(),
                chunk, opts.window_before, opts.window_after, static_cast<unsigned long long>(opts.window_min_file),
                opts.window_line_cap, nfiles, static_cast<unsigned long long>(wf), static_cast<unsigned long long>(wr),
                static_cast<unsigned long long>(wb), static_cast<unsigned long long>(lw),
                static_cast<unsigned long long>(lc), static_cast<unsigned long long>(ff),
                static_cast<unsigned long long>(fb), same ? "equal" : "DIFFER", same_short ? "equal" : "DIFFERS",
                same_plan ? "equal" : "DIFFERS");
    tsg_result_free(res);
    tsg_ruleset_free(rs);
    if (!same || !same_short || !same_plan) return 1;
  }
  if (!r.ok) { std::fprintf(stderr, "truncated dump\n"); return 2; }
  std::printf("line_window_check: %u corpus runs, no sanitizer report\n", ncorpora);
  return 0;
}

// Regexp compile recurses once per nesting level and the sanitizer's redzones
// make each frame several times larger: the run gets a 1 GiB stack, as
// tools/window_confirm_check.cpp's does.
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
