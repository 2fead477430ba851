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
//   tools/wirepack_tool_asan check2      # the 6-bit codec (v2): the cases of tests/test_wirepack2.py
//   tools/wirepack_tool_asan strips      # the strip planner (wire_strips.h) over the grid of tests/test_wire_strips.py
//   tools/wirepack_tool rate2 FILE [MiB per thread] [threads ...]
//       # v2 on FILE's bytes (repeated to fill 64 MiB strips): GB/s of input, packed / input with the strips'
//       # heads, escaped share, blocks per mode, beside the 7-bit packer on the same bytes
//   tools/wirepack_tool_asan check3      # check2's cases with split blocks allowed
//   tools/wirepack_tool rate3 FILE [MiB per thread] [threads ...]    # rate2 with split blocks allowed
//       # (WIREPACK_PATH=1|2|3 in the environment: the scalar, AVX2 or VBMI path instead of the CPU's best)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <thread>
#include <vector>

#include "wire_strips.h"
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

// ---- v2

static const char* path_name(int p) { return p == kWireVbmi ? "vbmi" : p == kWireAvx2 ? "avx2" : "scalar"; }

// as one_case: every path from an exact-size source into exact-size buffers, the round trip from exact-size
// packed bytes, and the format's invariants; the exact bytes are the Python model's to predict
static bool g_split = false;   // check3: the same cases with split blocks allowed
static unsigned long long g_split_blocks = 0;

static void one_case2(const char* name, const std::vector<uint8_t>& data, size_t mis) {
  const size_t n = data.size();
  std::unique_ptr<uint8_t[]> raw(new uint8_t[n + mis]);
  uint8_t* src = raw.get() + mis;
  if (n) std::memcpy(src, data.data(), n);
  std::vector<uint8_t> packed[3], alpha[3];
  std::vector<uint32_t> tab[3];
  for (int k = 0; k < 3; ++k) {
    std::unique_ptr<uint8_t[]> dst(new uint8_t[wire2_bound(n)]);
    tab[k].assign(wire_blocks(n), 0);
    alpha[k].assign(wire2_alpha_bytes(n), 0xEE);
    Wire2Stats st;
    const size_t pl = wire_pack2(src, n, dst.get(), tab[k].data(), alpha[k].data(), k + 1, &st, g_split);
    packed[k].assign(dst.get(), dst.get() + pl);
    g_split_blocks += st.blocks_split;
    std::unique_ptr<uint8_t[]> back(new uint8_t[n]);
    wire_unpack2(packed[k].data(), tab[k].data(), alpha[k].data(), n, back.get());
    if (n && std::memcmp(back.get(), src, n) != 0) { std::printf("FAIL %s: round trip (path %d)\n", name, k + 1); ++g_fail; }
    if (pl > n + 15) { std::printf("FAIL %s: packed size %zu (path %d)\n", name, pl, k + 1); ++g_fail; }
    if (st.blocks6 + st.blocks7 + st.blocks_raw + st.blocks_split != wire_blocks(n) || (!g_split && st.blocks_split)) { std::printf("FAIL %s: block counts\n", name); ++g_fail; }
    for (uint32_t t : tab[k])
      if ((t & 15u) || (!g_split && (t & kWireRawBit) && (t & kWire6Bit))) { std::printf("FAIL %s: table entry %08x\n", name, t); ++g_fail; }
  }
  for (int k = 1; k < 3; ++k)
    if (packed[0] != packed[k] || tab[0] != tab[k] || alpha[0] != alpha[k]) {
      std::printf("FAIL %s: path %d differs from the scalar path\n", name, k + 1);
      ++g_fail;
    }
}

static std::vector<uint8_t> words(size_t n, uint32_t seed) {
  static const char vals[] = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ";   // 63 values
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    v[i] = static_cast<uint8_t>(vals[i % kWire2Sample == 0 ? i / kWire2Sample % 63 : (seed >> 16) % 63]);
  }
  return v;
}

// 63 values of which a few are far more frequent than the rest: blocks of it go split where that is allowed
static std::vector<uint8_t> skewed(size_t n, uint32_t seed) {
  static const char vals[] = "etaoin shrdlucmfwypvbgkqjxzETAOINSHRDLUCMFWYPVBGKQJXZ0123456789_";
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    const uint32_t a = (seed >> 8) % 63, b = (seed >> 20) % 63;
    v[i] = static_cast<uint8_t>(vals[a * b / 63]);
  }
  return v;
}

static int check2() {
  const size_t B = kWireBlock, R = kWire2Region;
  const size_t lens[] = {0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 100, 1000, 1001, B - 1, B, B + 1, 2 * B + 5, 3 * B + 77};
  char name[64];
  for (size_t n : lens)
    for (size_t mis : {size_t(0), size_t(1), size_t(3), size_t(13)}) {
      std::snprintf(name, sizeof name, "words len %zu mis %zu", n, mis);
      one_case2(name, words(n, 7 + static_cast<uint32_t>(n)), mis);
      std::snprintf(name, sizeof name, "noise len %zu mis %zu", n, mis);
      one_case2(name, text(n, 9 + static_cast<uint32_t>(n)), mis);
      std::snprintf(name, sizeof name, "skewed len %zu mis %zu", n, mis);
      one_case2(name, skewed(n, 13 + static_cast<uint32_t>(n)), mis);
    }
  const uint8_t vals[] = {0x00, 0x7F, 0x80, 0xFF};
  const size_t strip = R + 4 * B;
  for (uint8_t v : vals)
    for (size_t pos : {size_t(0), B - 1, B, R - 1, R, strip - 1}) {
      std::vector<uint8_t> d = words(strip, 99);
      d[pos] = v;
      std::snprintf(name, sizeof name, "value %02x at %zu", v, pos);
      one_case2(name, d, 1);
    }
  // escape counts around the points where 7-bit and raw take over, and far past them
  for (size_t k : {size_t(1), size_t(495), size_t(496), size_t(497), size_t(1008), size_t(1009), size_t(2048), size_t(4096)})
    for (uint8_t v : {uint8_t('#'), uint8_t(0x80)}) {
      std::vector<uint8_t> d = words(B, 5);
      for (size_t i = 0; i < k; ++i) d[i * (B / k) + (k < B / 2 ? 1 : 0)] = v;
      std::snprintf(name, sizeof name, "%zu escapes of %02x", k, v);
      one_case2(name, d, 3);
    }
  for (size_t tail : {size_t(1), size_t(2), size_t(3)}) {
    std::vector<uint8_t> d = words(3 * B + 1028 + tail, 3);
    for (size_t i = d.size() - tail; i < d.size(); ++i) d[i] = '@';
    std::snprintf(name, sizeof name, "escapes in a last group of %zu", tail);
    one_case2(name, d, 13);
  }
  {
    std::vector<uint8_t> d(3 * B + 18);
    for (size_t i = 0; i < d.size(); ++i) d[i] = i % 2 ? 0xA9 : 0xC3;
    one_case2("all non-ASCII", d, 0);
  }
  {
    std::vector<uint8_t> d = words(10 * B, 11), x = text(B, 12), y = words(B + 100, 13);
    d.insert(d.end(), x.begin(), x.end());
    d.insert(d.end(), B, 0xC3);
    d.insert(d.end(), y.begin(), y.end());
    one_case2("three modes", d, 1);
  }
  {
    std::vector<uint8_t> d = words(R, 21), x = text(R / 2 + 7, 22);
    for (uint8_t& c : x) c = static_cast<uint8_t>('!' + c % 15);
    d.insert(d.end(), x.begin(), x.end());
    one_case2("two regions", d, 3);
  }
  // hot and warm values in turn, by byte and by runs that end at the 1024-byte edges; every 16th byte escaping
  {
    std::vector<uint8_t> d = words(3 * B + 333, 31);
    const uint8_t hot = d[0], warm = '%';
    for (size_t i = 0; i < B; ++i) d[i] = i % 2 ? hot : static_cast<uint8_t>('a' + i / 2 % 26);
    for (size_t i = B; i < 2 * B; ++i) d[i] = (i / 1024) % 2 ? hot : static_cast<uint8_t>('A' + i % 26);
    for (size_t i = 2 * B; i < 3 * B; i += 16) d[i + 1] = warm;
    for (size_t i = 2 * B + 32; i < 2 * B + 48; ++i) d[i] = 0x80 + static_cast<uint8_t>(i % 16);
    one_case2("hot and warm patterns", d, 5);
  }
  std::printf("split blocks written: %llu\n", g_split_blocks);
  std::printf("wirepack check%s: %s (AVX2 %s, VBMI %s, VBMI2 %s)\n", g_split ? "3" : "2", g_fail ? "FAILED" : "ok",
              wire_have_avx2() ? "yes" : "no: scalar in its place", wire_have_vbmi() ? "yes" : "no: the path below in its place",
              wire_have_vbmi2() ? "yes" : "no");
  return g_fail ? 1 : 0;
}

static int rate2(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[2], std::ios::binary);
  std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (file.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  const size_t bytes = static_cast<size_t>(argc > 3 ? std::atoi(argv[3]) : 64) << 20;
  std::vector<int> counts;
  for (int i = 4; i < argc; ++i) counts.push_back(std::atoi(argv[i]));
  if (counts.empty()) counts = {1, 8, 14, 16};
  int maxt = 1;
  for (int c : counts) maxt = c > maxt ? c : maxt;
  // thread t packs `bytes` of the file from its own offset (wrapping), as one strip
  std::vector<std::vector<uint8_t>> src(maxt), dst(maxt);
  for (int t = 0; t < maxt; ++t) {
    src[t].resize(bytes);
    size_t at = (file.size() / maxt * t) % file.size();
    for (size_t o = 0; o < bytes;) {
      const size_t k = std::min(bytes - o, file.size() - at);
      std::memcpy(src[t].data() + o, file.data() + at, k);
      o += k;
      at = 0;
    }
    dst[t].assign(wire2_bound(bytes), 1);
  }
  const int reps = 4;
  // WIREPACK_PATH=1|2|3: the scalar, AVX2 or VBMI path instead of the CPU's best
  const int path = std::getenv("WIREPACK_PATH") ? std::atoi(std::getenv("WIREPACK_PATH")) : kWireAuto;
  for (int nt : counts) {
    if (nt < 1) continue;
    double gbps[2] = {0, 0};
    std::vector<Wire2Stats> st(nt);
    std::vector<size_t> pl2(nt), pl1(nt);
    for (int v2 = 1; v2 >= 0; --v2)
      for (int pass = 0; pass < 2; ++pass) {     // (the first pass warms)
        auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t)
          th.emplace_back([&, t] {
            std::vector<uint32_t> tab(wire_blocks(bytes));
            std::vector<uint8_t> alpha(wire2_alpha_bytes(bytes));
            for (int r = 0; r < reps; ++r) {
              if (v2) pl2[t] = wire_pack2(src[t].data(), bytes, dst[t].data(), tab.data(), alpha.data(), path, &st[t], g_split);
              else pl1[t] = wire_pack(src[t].data(), bytes, dst[t].data(), tab.data(), kWireAuto);
            }
          });
        for (auto& x : th) x.join();
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        gbps[v2] = static_cast<double>(bytes) * nt * reps / s / 1e9;
      }
    Wire2Stats a;
    double sent2 = 0, sent1 = 0;
    for (int t = 0; t < nt; ++t) {
      a.blocks6 += st[t].blocks6; a.blocks7 += st[t].blocks7; a.blocks_raw += st[t].blocks_raw; a.escaped += st[t].escaped;
      a.blocks_split += st[t].blocks_split;
      sent2 += static_cast<double>(wire_table_bytes(bytes) + wire2_alpha_bytes(bytes) + pl2[t]);
      sent1 += static_cast<double>(wire_table_bytes(bytes) + pl1[t]);
    }
    const double in = static_cast<double>(bytes) * nt;
    std::printf("{\"file\": \"%s\", \"file_mb\": %.1f, \"threads\": %d, \"mib_per_thread\": %zu, \"path\": \"%s\", "
                "\"pack2_gbps\": %.2f, \"ratio2\": %.4f, \"escaped_share\": %.5f, \"blocks_6bit\": %llu, "
                "\"blocks_7bit\": %llu, \"blocks_raw\": %llu, \"blocks_split\": %llu, \"vbmi2\": %s, \"pack7_gbps\": %.2f, \"ratio7\": %.4f}\n",
                argv[2], file.size() / 1e6, nt, bytes >> 20, path_name(wire2_path(path)), gbps[1], sent2 / in,
                static_cast<double>(a.escaped) / in, static_cast<unsigned long long>(a.blocks6),
                static_cast<unsigned long long>(a.blocks7), static_cast<unsigned long long>(a.blocks_raw),
                static_cast<unsigned long long>(a.blocks_split), wire_have_vbmi2() ? "true" : "false", gbps[0],
                sent1 / in);
    std::fflush(stdout);
  }
  return 0;
}

// ---- the strip planner (wire_strips.h) over the grid of tests/test_wire_strips.py: random segment sizes in
// [1, 2^33), the strip sizes the engine and its tests use, 0..16 packers; every plan is checked for exact cover in
// order, aligned offsets, strip lengths, and the uniform cut where the ramp is off or does not fit

static bool strips_case(uint64_t seg, uint64_t strip, bool first, int np) {
  const std::vector<WireStrip> plan = plan_wire_strips(seg, strip, first, np);
  uint64_t at = 0;
  bool ok = !plan.empty();
  for (size_t i = 0; ok && i < plan.size(); ++i) {
    const WireStrip& s = plan[i];
    ok = s.offset == at && s.bytes > 0 && s.bytes <= strip && (i + 1 == plan.size() || s.bytes % kWireBlock == 0) &&
         (strip % kWireStripAlign != 0 || s.offset % kWireStripAlign == 0);
    at += s.bytes;
  }
  ok = ok && at == seg;
  const uint64_t m = static_cast<uint64_t>(kWireRampRounds) * np;
  uint64_t need = kWireRampBack * (strip / kWireRampBackDiv);
  for (uint64_t i = 0; i < m; ++i) need += wire_ramp_front(strip, i, m);
  const bool ramp = first && np > 0 && strip >= kWireRampMinStrip && strip % kWireRampMinStrip == 0 && seg >= need;
  const size_t nuniform = static_cast<size_t>((seg + strip - 1) / strip);
  if (ok && !ramp) {
    ok = plan.size() == nuniform;
    for (size_t i = 0; ok && i < plan.size(); ++i) ok = plan[i].offset == i * strip;
  }
  if (ok && ramp) ok = plan.size() > nuniform && plan[0].bytes <= std::max(kWireStripAlign, strip / m) &&
                       plan[m - 1].bytes == strip && plan.back().bytes <= strip / kWireRampBackDiv;
  if (!ok) {
    std::printf("FAIL strips: segment %llu strip %llu first %d packers %d\n", static_cast<unsigned long long>(seg),
                static_cast<unsigned long long>(strip), first ? 1 : 0, np);
    ++g_fail;
  }
  return ramp;
}

static int strips() {
  const uint64_t sizes[] = {4096, 65536, 1ull << 20, 64ull << 20, kWireMaxStrip};
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  size_t cases = 0, ramped = 0;
  for (uint64_t strip : sizes) {
    for (int i = 0; i < 400; ++i) {
      // log-uniform sizes; 4096-byte strips stay under 2^28 bytes (65536 strips)
      const int bits = 1 + static_cast<int>(rnd() % (strip >= 65536 ? 33 : 28));
      const uint64_t seg = std::max<uint64_t>(1, rnd() & ((1ull << bits) - 1));
      const int np = static_cast<int>(rnd() % 17);
      for (bool first : {true, false}) { ramped += strips_case(seg, strip, first, np); ++cases; }
    }
    for (int np : {1, 14, 16}) {
      const uint64_t m = static_cast<uint64_t>(kWireRampRounds) * np;
      uint64_t edge = kWireRampBack * (strip / kWireRampBackDiv);
      for (uint64_t i = 0; i < m; ++i) edge += wire_ramp_front(strip, i, m);
      for (uint64_t seg : {edge - 1, edge, edge + 1, edge + kWireStripAlign + 5, (uint64_t(1) << 33) - 1})
        if (seg / strip < (1u << 21)) { ramped += strips_case(seg, strip, true, np); ++cases; }
    }
  }
  std::printf("strips: %zu plans checked, %zu with a ramp, %d failed\n", cases, ramped, g_fail);
  return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "strips") == 0) return strips();
  if (argc > 1 && std::strcmp(argv[1], "check") == 0) return check();
  if (argc > 1 && std::strcmp(argv[1], "rate") == 0) return rate(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "check2") == 0) return check2();
  if (argc > 2 && std::strcmp(argv[1], "rate2") == 0) return rate2(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "check3") == 0) { g_split = true; return check2(); }
  if (argc > 2 && std::strcmp(argv[1], "rate3") == 0) { g_split = true; return rate2(argc, argv); }
  std::fprintf(stderr, "usage: %s check | rate [MiB per thread] [threads ...] | check2 | check3 | strips | "
                       "rate2 FILE [MiB per thread] [threads ...] | rate3 FILE ...\n", argv[0]);
  return 2;
}
