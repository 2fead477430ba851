// Sanitizer driver for the zstd decode's CPU side (tools/zstd_asan_check.py):
// zstd_model (zstdec.h) -- the decoder the device runs, behind ZsHostIo -- over
// every stream of tests/_zstd_corpus.py, on exact-size heap copies so that a
// read past the stream or a write past the slot is the sanitizer's to see.
//
//   zstd_asan <dir>        dir/index.txt: one "<name> <status> <cap>" per line,
//                          dir/<name>.zst the stream, dir/<name>.out the payload
//                          of a valid one
// Per stream: the status and, for a valid one, the output are the corpus's;
// a slot one byte short ends TSG_ZSTD_DST_FULL; zstd_size_bound walks it and,
// for a valid one, is no smaller than the output.  Per stream of at most kSmall
// bytes also every single-byte corruption (each byte XOR 0xFF, XOR 0x01, + 1)
// and every truncation: the call returns (every loop turn of the decoder
// consumes input, produces output or stops), the status is one of the table's,
// the output stays in the slot.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "zstdec.h"

using namespace tsg;

namespace {

constexpr size_t kSmall = 400;
long g_runs = 0;

std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// one run on exact-size heap blocks; the output's first *out_len bytes to *out
int32_t run(const uint8_t* z, size_t n, uint64_t cap, std::vector<uint8_t>* out) {
  std::unique_ptr<uint8_t[]> src(new uint8_t[n]), dst(new uint8_t[cap]);
  std::copy(z, z + n, src.get());
  const uint8_t* p = src.get();
  uint64_t out_len = ~0ull, bound = 0;
  int exact = 0;
  const int32_t st = zstd_model([p](uint64_t k) { return static_cast<uint32_t>(p[k]); }, n, dst.get(), cap, &out_len);
  const bool clean = zstd_size_bound(p, n, &bound, &exact);
  ++g_runs;
  if (st < kZsOk || st > kZsDstFull || out_len > cap || (st == kZsOk && (!clean || bound < out_len || (exact && bound != out_len)))) {
    std::printf("FAIL: status %d out_len %llu cap %llu bound %llu\n", st, static_cast<unsigned long long>(out_len),
                static_cast<unsigned long long>(cap), static_cast<unsigned long long>(bound));
    std::exit(1);
  }
  if (out) out->assign(dst.get(), dst.get() + out_len);
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  std::ifstream index(dir + "/index.txt");
  std::string name;
  int want = 0;
  unsigned long long cap = 0;
  long streams = 0, mutated = 0, by_status[7] = {0, 0, 0, 0, 0, 0, 0};
  while (index >> name >> want >> cap) {
    const std::vector<uint8_t> z = slurp(dir + "/" + name + ".zst");
    std::vector<uint8_t> out;
    const int32_t st = run(z.data(), z.size(), cap, &out);
    if (st != want) { std::printf("FAIL %s: status %d, want %d\n", name.c_str(), st, want); return 1; }
    ++streams;
    if (want == kZsOk) {
      if (out != slurp(dir + "/" + name + ".out")) { std::printf("FAIL %s: output differs\n", name.c_str()); return 1; }
      if (!out.empty() && run(z.data(), z.size(), out.size() - 1, nullptr) != kZsDstFull) {
        std::printf("FAIL %s: a slot one byte short\n", name.c_str());
        return 1;
      }
    }
    if (z.size() > kSmall) continue;
    std::vector<uint8_t> m = z;
    for (size_t k = 0; k < z.size(); ++k) {
      for (int how = 0; how < 3; ++how) {
        m[k] = how == 0 ? z[k] ^ 0xff : how == 1 ? z[k] ^ 0x01 : static_cast<uint8_t>(z[k] + 1);
        ++by_status[run(m.data(), m.size(), cap, nullptr)];
      }
      m[k] = z[k];
      ++by_status[run(z.data(), k, cap, nullptr)];
      mutated += 4;
    }
  }
  std::printf("zstd_model: %ld streams as the corpus says; %ld corruptions and truncations of the streams of <= %zu "
              "bytes (status OK %ld, header %ld, corrupt %ld, EOF %ld, checksum %ld, dictionary %ld, slot full %ld); "
              "%ld runs, all returned, every output inside its slot\n",
              streams, mutated, kSmall, by_status[0], by_status[1], by_status[2], by_status[3], by_status[4], by_status[5],
              by_status[6], g_runs);
  return streams > 300 && mutated > 10000 ? 0 : 1;
}
