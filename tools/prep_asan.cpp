// Host-code sanitizer driver for the device preparation's CPU side: runs
// plan_prep (tsg_prepare_device_model) and prepare_core
// (tsg_prepare_batch_opts) over the corpora of tests/_prep_corpus.py and
// compares them.  Built by tools/prep_asan_check.py with
// -fsanitize=address,undefined; no GPU is touched.
//
// Usage: prep_asan <dir>; <dir>/index.txt lists one case directory per line,
// each holding config.json (may be empty = builtin rules), data.bin,
// offsets.bin (uint64, nfiles + 1), paths.txt (one path per line) and
// opts.txt (line 1: config path; then one file pattern per line).
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

static int run_case(const std::string& dir, uint64_t* bytes_in, uint64_t* bytes_out) {
  const std::string cfg = slurp(dir + "/config.json");
  // exact-size heap copies: a read past the batch or the offsets is a report
  const std::string data_s = slurp(dir + "/data.bin"), off_s = slurp(dir + "/offsets.bin");
  struct Bytes {                                   // new[]: not NULL for an empty batch
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    uint8_t* data() const { return p.get(); }
    size_t size() const { return n; }
  } data{std::unique_ptr<uint8_t[]>(new uint8_t[data_s.size()]), data_s.size()};
  std::memcpy(data.data(), data_s.data(), data_s.size());
  std::vector<uint64_t> off(off_s.size() / 8);
  std::memcpy(off.data(), off_s.data(), off.size() * 8);
  const std::vector<std::string> paths = lines_of(dir + "/paths.txt");
  std::vector<std::string> opts = lines_of(dir + "/opts.txt");
  if (opts.empty()) opts.push_back("");
  const uint32_t nfiles = static_cast<uint32_t>(paths.size());
  if (off.size() != nfiles + 1u || off[nfiles] != data.size()) { std::fprintf(stderr, "%s: bad case\n", dir.c_str()); return 2; }
  std::vector<const char*> pp;
  std::vector<uint32_t> pl;
  for (const auto& p : paths) { pp.push_back(p.c_str()); pl.push_back(static_cast<uint32_t>(p.size())); }
  std::vector<const char*> pats;
  for (size_t i = 1; i < opts.size(); ++i) pats.push_back(opts[i].c_str());
  tsg_feed_opts fo{};
  fo.config_path = opts[0].c_str();
  fo.file_patterns = pats.data();
  fo.n_file_patterns = static_cast<uint32_t>(pats.size());
  fo.threads = 4;
  tsg_ruleset* rs = nullptr;
  if (tsg_ruleset_compile(cfg.empty() ? nullptr : cfg.data(), cfg.size(), &rs) != 0) {
    std::fprintf(stderr, "%s: %s\n", dir.c_str(), tsg_last_error());
    return 2;
  }
  std::vector<uint8_t> kinds(nfiles);
  std::vector<uint64_t> new_off(nfiles + 1u);
  tsg_prepared *m = nullptr, *h = nullptr;
  int rc = 0;
  if (tsg_prepare_device_model(rs, data.data(), off.data(), nfiles, pp.data(), pl.data(), &fo, kinds.data(),
                               new_off.data(), &m) != 0 ||
      tsg_prepare_batch_opts(rs, data.data(), off.data(), nfiles, pp.data(), pl.data(), &fo, &h) != 0) {
    std::fprintf(stderr, "%s: %s\n", dir.c_str(), tsg_last_error());
    rc = 2;
  } else {
    const uint8_t *md, *hd, *mb, *hb;
    const uint64_t *mo, *ho;
    const uint32_t *mi, *hi;
    uint32_t mn = 0, hn = 0;
    tsg_prepared_view(m, &md, &mo, &mi, &mb, &mn);
    tsg_prepared_view(h, &hd, &ho, &hi, &hb, &hn);
    if (mn != hn || std::memcmp(mo, ho, (mn + 1u) * 8) != 0 || (mn && std::memcmp(mi, hi, mn * 4u) != 0) ||
        (mn && std::memcmp(mb, hb, mn) != 0) || std::memcmp(md, hd, mo[mn]) != 0 || new_off[nfiles] != mo[mn]) {
      std::fprintf(stderr, "%s: the model and the host feed differ\n", dir.c_str());
      rc = 1;
    }
    *bytes_in += data.size();
    *bytes_out += mo[mn];
  }
  tsg_prepared_free(m);
  tsg_prepared_free(h);
  tsg_ruleset_free(rs);
  return rc;
}

// The rule set's regexp compile recurses once per nesting level and ASan's
// redzones make each frame several times larger than at -O3, so the run gets
// a 1 GiB stack (as tools/asan_driver.cpp).
struct Args {
  std::string root;
  int rc;
};

static int run_all(const std::string& root);

static void* run_thread(void* p) {
  auto* a = static_cast<Args*>(p);
  a->rc = run_all(a->root);
  return nullptr;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: prep_asan <dir>\n"); return 2; }
  Args a{argv[1], 1};
  pthread_attr_t at;
  pthread_attr_init(&at);
  pthread_attr_setstacksize(&at, size_t(1) << 30);
  pthread_t t;
  if (pthread_create(&t, &at, run_thread, &a) != 0) return 2;
  pthread_join(t, nullptr);
  return a.rc;
}

static int run_all(const std::string& root) {
  int rc = 0;
  uint64_t in = 0, out = 0;
  size_t n = 0;
  for (const std::string& c : lines_of(root + "/index.txt")) {
    if (c.empty()) continue;
    rc |= run_case(root + "/" + c, &in, &out);
    ++n;
  }
  std::printf("prep model == host feed on %zu corpora, %llu raw bytes -> %llu prepared: %s\n", n,
              static_cast<unsigned long long>(in), static_cast<unsigned long long>(out), rc ? "FAILED" : "ok");
  return rc;
}
