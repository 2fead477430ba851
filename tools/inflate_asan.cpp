// Sanitizer driver for the gzip inflate's CPU side (tools/inflate_asan_check.py):
// inflate_model (inflate.h) -- the decoder the device runs, behind HostIo --
// over every stream of tests/_gzip_corpus.py, on exact-size heap copies so that
// a read past the stream or a write past the slot is the sanitizer's to see.
//
//   inflate_asan <dir>     dir/index.txt: one "<name> <status> <cap>" per line,
//                          dir/<name>.gz the stream, dir/<name>.out the payload
//                          of a valid one
// Per stream: the status and, for a valid one, the output are the corpus's;
// a slot one byte short ends TSG_INFLATE_DST_FULL.  Per stream of at most
// kSmall bytes also every single-byte corruption (each byte XOR 0xFF) and
// every truncation: the call returns (every loop turn of the decoder consumes
// input or stops), the status is one of the table's, the output stays in the
// slot.  The checksum pass is compared with a bytewise CRC32.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "inflate.h"

using namespace tsg;

namespace {

constexpr size_t kSmall = 400;
long g_runs = 0;

std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// one run on exact-size heap blocks; the output's first *out_len bytes to *out
int32_t run(const uint8_t* gz, size_t n, uint64_t cap, std::vector<uint8_t>* out) {
  std::unique_ptr<uint8_t[]> src(new uint8_t[n]), dst(new uint8_t[cap]);
  std::copy(gz, gz + n, src.get());
  const uint8_t* p = src.get();
  uint64_t out_len = ~0ull;
  const int32_t st = inflate_model([p](uint64_t k) { return static_cast<uint32_t>(p[k]); }, n, dst.get(), cap, &out_len);
  ++g_runs;
  if (st < kInfOk || st > kInfDstFull || out_len > cap) {
    std::printf("FAIL: status %d out_len %llu cap %llu\n", st, static_cast<unsigned long long>(out_len),
                static_cast<unsigned long long>(cap));
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
  long streams = 0, mutated = 0, by_status[6] = {0, 0, 0, 0, 0, 0};
  while (index >> name >> want >> cap) {
    const std::vector<uint8_t> gz = slurp(dir + "/" + name + ".gz");
    std::vector<uint8_t> out;
    const int32_t st = run(gz.data(), gz.size(), cap, &out);
    if (st != want) { std::printf("FAIL %s: status %d, want %d\n", name.c_str(), st, want); return 1; }
    ++streams;
    if (want == kInfOk) {
      if (out != slurp(dir + "/" + name + ".out")) { std::printf("FAIL %s: output differs\n", name.c_str()); return 1; }
      if (crc32_bytes(out.data(), out.size()) != [&] {
            std::vector<uint32_t> s(crc32_nslices(out.size()));
            crc32_slices(out.data(), out.size(), s.data());
            return crc32_combine(s.data(), out.size());
          }()) {
        std::printf("FAIL %s: crc32 slices\n", name.c_str());
        return 1;
      }
      if (!out.empty() && run(gz.data(), gz.size(), out.size() - 1, nullptr) != kInfDstFull) {
        std::printf("FAIL %s: a slot one byte short\n", name.c_str());
        return 1;
      }
    }
    if (gz.size() > kSmall) continue;
    std::vector<uint8_t> m = gz;
    for (size_t k = 0; k < gz.size(); ++k) {
      m[k] ^= 0xff;
      ++by_status[run(m.data(), m.size(), cap, nullptr)];
      m[k] ^= 0xff;
      ++by_status[run(gz.data(), k, cap, nullptr)];
      mutated += 2;
    }
  }
  std::printf("inflate_model: %ld streams as the corpus says; %ld corruptions and truncations of the streams of <= %zu "
              "bytes (status OK %ld, header %ld, corrupt %ld, EOF %ld, checksum %ld, slot full %ld); %ld runs, all "
              "returned, every output inside its slot\n",
              streams, mutated, kSmall, by_status[0], by_status[1], by_status[2], by_status[3], by_status[4],
              by_status[5], g_runs);
  return streams > 300 && mutated > 10000 ? 0 : 1;
}
