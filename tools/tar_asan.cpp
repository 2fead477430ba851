// Host-code sanitizer driver for the device tar walk's CPU side: runs
// plan_tar_marks (tsg_test_tar_marks) and the model of
// tsg_prepare_layer_tar_device (marks -> SparseTarInput -> walk_layer -> gate
// -> interleaved entries -> plan_prep), with the marks and without them, over
// the tars of tests/_tar_corpus.py, and compares them with
// tsg_prepare_layer_tar_opts.  Built by tools/tar_asan_check.py with
// -fsanitize=address,undefined; no GPU is touched.
//
// Usage: tar_asan <dir>; <dir>/index.txt lists one case directory per line,
// each holding tar.bin and opts.txt (line 1: config path; then lines
// "F <skip file>", "D <skip dir>", "P <file pattern>").
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include <pthread.h>

#include "../include/trivy_secret.h"
#include "../include/trivy_secret_test.h"

static std::string slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static std::vector<std::string> lines_of(const std::string& p) {
  std::vector<std::string> out;
  std::ifstream f(p);
  for (std::string l; std::getline(f, l);) out.push_back(l);
  return out;
}

struct View {
  int rc = 0;
  std::string err, data, walk;
  std::vector<uint64_t> off;
  std::vector<uint32_t> idx;
  std::vector<uint8_t> bin;
  std::vector<std::string> paths;
  bool operator==(const View& o) const {
    return rc == o.rc && err == o.err && data == o.data && walk == o.walk && off == o.off && idx == o.idx &&
           bin == o.bin && paths == o.paths;
  }
};

static View view_of(int rc, tsg_prepared* p) {
  View v;
  v.rc = rc;
  if (rc != 0) { v.err = tsg_last_error(); return v; }
  const uint8_t *d, *b;
  const uint64_t* o;
  const uint32_t* ix;
  uint32_t n = 0;
  tsg_prepared_view(p, &d, &o, &ix, &b, &n);
  v.off.assign(o, o + n + 1);
  if (n) {                                         // (an empty vector's data() may be NULL)
    v.idx.assign(ix, ix + n);
    v.bin.assign(b, b + n);
  }
  if (d && o[n]) v.data.assign(reinterpret_cast<const char*>(d), o[n]);
  const char* const* pp;
  const uint32_t* pl;
  tsg_prepared_paths(p, &pp, &pl);
  for (uint32_t k = 0; k < n; ++k) v.paths.emplace_back(pp[k], pl[k]);
  v.walk = tsg_prepared_walk_json(p);
  tsg_prepared_free(p);
  return v;
}

static int run_case(tsg_ruleset* rs, const std::string& dir, uint64_t* bytes, uint64_t* marked, uint32_t* max_fb) {
  const std::string tar_s = slurp(dir + "/tar.bin");
  // exact-size heap copies: a read past the tar or a store past the marks is a report
  const size_t len = tar_s.size();
  std::unique_ptr<uint8_t[]> tar(new uint8_t[len]);
  std::memcpy(tar.get(), tar_s.data(), len);
  std::unique_ptr<uint8_t[]> marks(new uint8_t[len / 512]);
  std::vector<std::string> opts = lines_of(dir + "/opts.txt");
  if (opts.empty()) opts.push_back("");
  std::vector<const char*> sf, sd, pats;
  for (size_t i = 1; i < opts.size(); ++i) {
    if (opts[i].size() < 2) continue;
    (opts[i][0] == 'F' ? sf : opts[i][0] == 'D' ? sd : pats).push_back(opts[i].c_str() + 2);
  }
  tsg_feed_opts fo{};
  fo.config_path = opts[0].c_str();
  fo.file_patterns = pats.data();
  fo.n_file_patterns = static_cast<uint32_t>(pats.size());
  fo.skip_files = sf.data();
  fo.n_skip_files = static_cast<uint32_t>(sf.size());
  fo.skip_dirs = sd.data();
  fo.n_skip_dirs = static_cast<uint32_t>(sd.size());
  fo.threads = 4;
  if (tsg_test_tar_marks(tar.get(), len, marks.get()) != 0) { std::fprintf(stderr, "%s: %s\n", dir.c_str(), tsg_last_error()); return 2; }
  for (size_t b = 0; b < len / 512; ++b) *marked += marks[b];
  tsg_prepared* p = nullptr;
  const int hrc = tsg_prepare_layer_tar_opts(rs, tar.get(), len, &fo, &p);
  const View host = view_of(hrc, p);
  int rc = 0;
  for (int use_marks = 1; use_marks >= 0; --use_marks) {
    uint32_t fb = 0;
    p = nullptr;
    const int mrc = tsg_prepare_layer_tar_device_model(rs, tar.get(), len, &fo, use_marks, &fb, &p);
    const View m = view_of(mrc, p);
    if (!(m == host)) {
      std::fprintf(stderr, "%s: the model (marks %d) and the host call differ\n", dir.c_str(), use_marks);
      rc = 1;
    }
    if (use_marks) {
      if (fb > 2) { std::fprintf(stderr, "%s: %u fallback reads\n", dir.c_str(), fb); rc = 1; }
      if (fb > *max_fb) *max_fb = fb;
    }
  }
  *bytes += len;
  return rc;
}

static int run_all(const std::string& root) {
  tsg_ruleset* rs = nullptr;
  if (tsg_ruleset_compile(nullptr, 0, &rs) != 0) { std::fprintf(stderr, "%s\n", tsg_last_error()); return 2; }
  int rc = 0;
  uint64_t bytes = 0, marked = 0;
  uint32_t max_fb = 0;
  size_t n = 0;
  for (const std::string& c : lines_of(root + "/index.txt")) {
    if (c.empty()) continue;
    rc |= run_case(rs, root + "/" + c, &bytes, &marked, &max_fb);
    ++n;
  }
  tsg_ruleset_free(rs);
  std::printf("tar walk model == host call on %zu cases, %llu tar bytes, %llu blocks marked, at most %u fallback reads: %s\n",
              n, static_cast<unsigned long long>(bytes), static_cast<unsigned long long>(marked), max_fb,
              rc ? "FAILED" : "ok");
  return rc;
}

// The rule set's regexp compile recurses once per nesting level and ASan's
// redzones make each frame several times larger than at -O3, so the run gets
// a 1 GiB stack (as tools/prep_asan.cpp).
struct Args {
  std::string root;
  int rc;
};

static void* run_thread(void* p) {
  auto* a = static_cast<Args*>(p);
  a->rc = run_all(a->root);
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: tar_asan <dir>\n"); return 2; }
  Args a{argv[1], 1};
  pthread_attr_t at;
  pthread_attr_init(&at);
  pthread_attr_setstacksize(&at, size_t(1) << 30);
  pthread_t t;
  if (pthread_create(&t, &at, run_thread, &a) != 0) return 2;
  pthread_join(t, nullptr);
  return a.rc;
}
