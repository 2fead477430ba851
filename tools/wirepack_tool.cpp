// Stand-alone check and host rate measurement of the wire packer
// (trivy_amd/csrc/wirepack.cpp); no GPU, no Python.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I trivy_amd/csrc tools/wirepack_tool.cpp trivy_amd/csrc/wirepack.cpp -o tools/wirepack_tool_asan -lpthread
//   tools/wirepack_tool_asan check        # the cases of tests/test_wirepack.py, exact-size heap buffers
//
//   g++ -O3 -std=c++17 -march=x86-64-v2 -I trivy_amd/csrc tools/wirepack_tool.cpp trivy_amd/csrc/wirepack.cpp \
//       -o tools/wirepack_tool -lpthread
//   tools/wirepack_tool rate [MiB per thread] [threads ...]   # pack GB/s of input against memcpy
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "wirepack.h"

using namespace tsg;

static int g_fail = 0;

static size_t predicted(const uint8_t* p, size_t n) {
  size_t o = 0;
  for (size_t b = 0; b * kWireBlock < n; ++b) {
    const size_t len = n - b * kWireBlock < kWireBlock ? n - b * kWireBlock : kWireBlock;
    bool ascii = true;
    for (size_t i = 0; i < len; ++i) ascii = ascii && p[b * kWireBlock + i] < 0x80;
    o += ascii ? wire_packed_len(len) : len;
  }
  return o;
}

// src is copied to an exact-size heap block at `mis` bytes past an allocation
// start, so the sanitizer sees any read outside [src, src + n)
static void one_case(const char* name, const std::vector<uint8_t>& data, size_t mis) {
  const size_t n = data.size();
  std::unique_ptr<uint8_t[]> raw(new uint8_t[n + mis]);
  uint8_t* src = raw.get() + mis;
  if (n) std::memcpy(src, data.data(), n);
  std::vector<uint8_t> packed[2];
  std::vector<uint32_t> tab[2];
  size_t pl[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    std::unique_ptr<uint8_t[]> dst(new uint8_t[wire_bound(n)]);
    tab[k].assign(wire_blocks(n), 0);
    pl[k] = wire_pack(src, n, dst.get(), tab[k].data(), k == 0 ? kWireScalar : kWireAvx2);
    packed[k].assign(dst.get(), dst.get() + pl[k]);
    std::unique_ptr<uint8_t[]> back(new uint8_t[n]);
    wire_unpack(packed[k].data(), tab[k].data(), n, back.get());
    if (n && std::memcmp(back.get(), src, n) != 0) { std::printf("FAIL %s: round trip (path %d)\n", name, k + 1); ++g_fail; }
    if (pl[k] != predicted(src, n)) { std::printf("FAIL %s: packed size %zu (path %d)\n", name, pl[k], k + 1); ++g_fail; }
  }
  if (pl[0] != pl[1] || packed[0] != packed[1] || tab[0] != tab[1]) { std::printf("FAIL %s: paths differ\n", name); ++g_fail; }
}

static std::vector<uint8_t> text(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    v[i] = static_cast<uint8_t>((seed >> 24) & 0x7F);
  }
  return v;
}

static int check() {
  const size_t B = kWireBlock;
  const size_t lens[] = {0, 1, 7, 8, 9, 31, 32, 33, B - 1, B, B + 1, 2 * B + 5};
  char name[64];
  for (size_t n : lens)
    for (size_t mis : {size_t(0), size_t(1), size_t(3), size_t(13)}) {
      std::snprintf(name, sizeof name, "len %zu mis %zu", n, mis);
      one_case(name, text(n, 7 + static_cast<uint32_t>(n)), mis);
    }
  const uint8_t vals[] = {0x00, 0x7F, 0x80, 0xFF};
  const size_t strip = 4 * B;
  for (uint8_t v : vals)
    for (size_t pos : {size_t(0), B - 1, B, 2 * B - 1, strip - 1}) {
      std::vector<uint8_t> d = text(strip, 99);
      d[pos] = v;
      std::snprintf(name, sizeof name, "value %02x at %zu", v, pos);
      one_case(name, d, 1);
    }
  one_case("all non-ASCII", std::vector<uint8_t>(3 * B + 17, 0xC3), 0);
  std::vector<uint8_t> alt = text(6 * B + 3, 5);
  for (size_t b = 0; b < 6; b += 2) alt[b * B + 100] = 0xE2;
  one_case("alternating blocks", alt, 3);
  std::printf("wirepack check: %s (AVX2 %s)\n", g_fail ? "FAILED" : "ok", wire_have_avx2() ? "yes" : "no: scalar twice");
  return g_fail ? 1 : 0;
}

static double run_threads(int nt, size_t bytes, bool pack, const std::vector<std::vector<uint8_t>>& src,
                          std::vector<std::vector<uint8_t>>& dst) {
  const int reps = 4;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      std::vector<uint32_t> tab(wire_blocks(bytes));
      for (int r = 0; r < reps; ++r) {
        if (pack) wire_pack(src[t].data(), bytes, dst[t].data(), tab.data(), kWireAuto);
        else std::memcpy(dst[t].data(), src[t].data(), bytes);
      }
    });
  for (auto& x : th) x.join();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return static_cast<double>(bytes) * nt * reps / s / 1e9;
}

static int rate(int argc, char** argv) {
  const size_t bytes = static_cast<size_t>(argc > 2 ? std::atoi(argv[2]) : 64) << 20;
  std::vector<int> counts;
  for (int i = 3; i < argc; ++i) counts.push_back(std::atoi(argv[i]));
  if (counts.empty()) counts = {1, 8, 14, 16};
  int maxt = 1;
  for (int c : counts) maxt = c > maxt ? c : maxt;
  std::vector<std::vector<uint8_t>> src(maxt), dst(maxt);
  for (int t = 0; t < maxt; ++t) {
    src[t] = text(bytes, 11 + t);
    dst[t].assign(wire_bound(bytes), 1);
  }
  for (int nt : counts) {
    if (nt < 1) continue;
    run_threads(nt, bytes, true, src, dst);    // warm
    const double p = run_threads(nt, bytes, true, src, dst);
    const double m = run_threads(nt, bytes, false, src, dst);
    std::printf("{\"threads\": %d, \"mib_per_thread\": %zu, \"pack_gbps\": %.2f, \"memcpy_gbps\": %.2f, \"avx2\": %s}\n", nt,
                bytes >> 20, p, m, wire_have_avx2() ? "true" : "false");
    std::fflush(stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "check") == 0) return check();
  if (argc > 1 && std::strcmp(argv[1], "rate") == 0) return rate(argc, argv);
  std::fprintf(stderr, "usage: %s check | rate [MiB per thread] [threads ...]\n", argv[0]);
  return 2;
}
