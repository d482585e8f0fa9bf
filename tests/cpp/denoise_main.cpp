// denoise_main.cpp — wbx_denoise.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_denoise_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line (doubles as
// the hex of their bits):
//   t <W>                                      -> "t <status> <fnv-1a 64 of analysis_out's bytes> <of synthesis_out's>"
//   d <W>                                      -> "d <fnv of the device's A> <of the device's Y>", after checking that both are the
//                                                 canonical tables' words in the packed places
//   h <n> <W>                                  -> "h <denoise_hops> <denoise_profile_hops>"
//   b <n> <W> <channels>                       -> "b <denoise_band_hops> <denoise_launches>"
//   s <W>                                      -> "s <K> <G> <hops_wg> <chunk> <pair_tiles>", after checking the LDS bounds
//   q <hops> <strength bits> <count> <sum bits>...  -> "q <status> <out bits>..."
//   c <n> <W> <S> <F> <thr: 0 NULL, 1 given> <channels> <floor bits> <at> <entry bits> -> "c <status of denoise_check_args>"
//                                                 (thr = channels x B entries of 1.0, entry `at` replaced)
//   p <n> <W> <has_sums> <has_hops>            -> "p <status of denoise_profile_check_args>"
// Ends with "denoise ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_denoise.h"

static double from_hex(const std::string& s) {
  const uint64_t u = std::stoull(s, nullptr, 16);
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
static uint64_t fnv(const float* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n * sizeof(float); i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "t") {
      uint32_t W;
      ss >> W;
      const bool ok = wbx::den_window_ok(W);
      const size_t words = ok ? (size_t)2 * (W / 2 + 1) * W : 1;   // exactly the tables' length: ASan sees one word too many
      std::vector<float> a(words, 7.0f), y(words, 7.0f);
      const wbx_status st = wbx::denoise_tables(W, a.data(), y.data());
      if (!ok && (st != WBX_ERR_INVALID || a[0] != 7.0f || y[0] != 7.0f)) return 3;
      if (ok && wbx::denoise_tables(W, nullptr, nullptr) != WBX_ERR_INVALID) return 3;
      std::printf("t %d %016" PRIx64 " %016" PRIx64 "\n", (int)st, fnv(a.data(), words), fnv(y.data(), words));
    } else if (tag == "d") {
      uint32_t W;
      ss >> W;
      const uint32_t B = W / 2 + 1;
      const size_t half = (size_t)B * W;
      std::vector<float> a(2 * half), y(2 * half), A((size_t)W * W), Y((size_t)W * W);
      if (wbx::denoise_tables(W, a.data(), y.data()) != WBX_OK) return 4;
      wbx::denoise_device_tables(W, A.data(), Y.data());
      for (uint32_t k = 0; k < B; k++)
        for (uint32_t j = 0; j < W; j++) {
          const size_t at = (size_t)k * W + j;
          const uint32_t cw = wbx::den_cell_word(W, k), mw = wbx::den_masked_word(W, k);
          if (!same(A[(size_t)j * W + cw], a[at]) || !same(Y[(size_t)mw * W + j], y[at])) return 5;
          if (k == 0 || k == B - 1) {                              // the rows the packing leaves out are all +0.0
            if (!same(a[half + at], 0.0f) || !same(y[half + at], 0.0f)) return 6;
          } else if (!same(A[(size_t)j * W + cw + 1], a[half + at]) || !same(Y[(size_t)(mw + 1) * W + j], y[half + at])) {
            return 7;
          }
        }
      std::printf("d %016" PRIx64 " %016" PRIx64 "\n", fnv(A.data(), A.size()), fnv(Y.data(), Y.size()));
    } else if (tag == "h") {
      uint64_t n;
      uint32_t W;
      ss >> n >> W;
      std::printf("h %" PRIu64 " %" PRIu64 "\n", wbx::denoise_hops(n, W), wbx::denoise_profile_hops(n, W));
    } else if (tag == "b") {
      uint64_t n;
      uint32_t W, channels;
      ss >> n >> W >> channels;
      std::printf("b %u %" PRIu64 "\n", (unsigned)wbx::denoise_band_hops(W, channels), wbx::denoise_launches(n, W, channels));
    } else if (tag == "s") {
      uint32_t W;
      ss >> W;
      const wbx::DenShape s = wbx::denoise_shape(W);
      // what the kernel relies on: 4 waves, the staged rows within the span, 16-byte rows, the pairs covered
      if (s.G * (4u / s.G) != 4u || s.hops_wg != (8u / s.K) * (4u / s.G) || W % s.chunk || s.chunk % 4u || s.stride_shared % 4u) return 8;
      if ((s.hops_wg - 1u) * s.stride_shared + s.chunk > wbx::kDenSpanWords || s.hops_wg * s.stride_own > wbx::kDenSpanWords) return 9;
      if ((uint64_t)s.pair_tiles * 64u * s.K * s.G < W / 2u) return 10;
      if (wbx::kDenStageWords / (W * 2u) <= wbx::kDenBandSlack) return 11;
      std::printf("s %u %u %u %u %u\n", (unsigned)s.K, (unsigned)s.G, (unsigned)s.hops_wg, (unsigned)s.chunk, (unsigned)s.pair_tiles);
    } else if (tag == "q") {
      uint64_t hops;
      std::string strength;
      size_t count;
      ss >> hops >> strength >> count;
      std::vector<double> sums(count), out(count, 7.0);
      for (double& v : sums) {
        std::string w;
        ss >> w;
        v = from_hex(w);
      }
      const wbx_status st = wbx::denoise_threshold(sums.data(), hops, count, from_hex(strength), out.data());
      std::printf("q %d", (int)st);
      for (double v : out) std::printf(" %016" PRIx64, bits(v));
      std::printf("\n");
    } else if (tag == "c") {
      wbx::DenCall k{};
      int has_thr;
      uint32_t channels;
      size_t at;
      std::string floor, entry;
      ss >> k.n_frames >> k.window >> k.smooth_hops >> k.smooth_bins >> has_thr >> channels >> floor >> at >> entry;
      const uint32_t W = wbx::den_window_ok(k.window) ? k.window : 64u;
      std::vector<double> thr((size_t)channels * (W / 2 + 1), 1.0);   // exactly what the check may read
      if (at < thr.size()) thr[at] = from_hex(entry);
      k.thr = has_thr ? thr.data() : nullptr;
      k.floor = from_hex(floor);
      const char* why = "";
      const wbx_status st = wbx::denoise_check_args(k, channels, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 12;              // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "p") {
      uint64_t n;
      uint32_t W;
      int has_sums, has_hops;
      ss >> n >> W >> has_sums >> has_hops;
      const char* why = "";
      const wbx_status st = wbx::denoise_profile_check_args(n, W, has_sums != 0, has_hops != 0, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 13;
      std::printf("p %d\n", (int)st);
    }
  }
  static_assert(sizeof(wbx_denoise_stats) == 32 && wbx::kDenBandSlack == 11, "the header's text names these");
  std::printf("denoise ok\n");
  return 0;
}
