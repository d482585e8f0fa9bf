// f0_main.cpp — wbx_f0.h alone, stand-alone (its own main, g++ only, no device, no library): what tests/test_f0_host.py
// runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   h <n> <W> <H> <tau_max>                              -> "h <f0_hops>"
//   c <n> <W> <H> <tau_min> <tau_max> <threshold> <has_out> <cap> -> "c <status of f0_check>"
//   l <W> <tau_max>                                      -> "l <f0_launch_hops>"
//   n <hops> <W> <tau_max>                               -> "n <f0_launches>"
//   s <W> <H> <tau_max>                                  -> "s <G> <F> <f0_span_words>"
// The threshold is read with strtod, so "nan" and "inf" are cases.  Ends with "f0 ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "../../whitebox_amd/csrc/wbx_f0.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "h") {
      uint64_t n;
      uint32_t W, H, tau_max;
      ss >> n >> W >> H >> tau_max;
      std::printf("h %" PRIu64 "\n", wbx::f0_hops(n, W, H, tau_max));
    } else if (tag == "c") {
      wbx::F0Call k{};
      std::string thr;
      int has_out;
      uint64_t cap;
      ss >> k.n_frames >> k.window >> k.hop >> k.tau_min >> k.tau_max >> thr >> has_out >> cap;
      k.threshold = std::strtod(thr.c_str(), nullptr);
      k.has_out = has_out != 0;
      k.frames_cap = (size_t)cap;
      const char* why = "";
      const wbx_status st = wbx::f0_check(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;             // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "l") {
      uint32_t W, tau_max;
      ss >> W >> tau_max;
      std::printf("l %u\n", (unsigned)wbx::f0_launch_hops(W, tau_max));
    } else if (tag == "n") {
      uint64_t hops;
      uint32_t W, tau_max;
      ss >> hops >> W >> tau_max;
      std::printf("n %" PRIu64 "\n", wbx::f0_launches(hops, W, tau_max));
    } else if (tag == "s") {
      uint32_t W, H, tau_max;
      ss >> W >> H >> tau_max;
      const wbx::F0Shape s = wbx::f0_shape(W, H, tau_max);
      const uint32_t words = wbx::f0_span_words(W, H, s.G, s.F);
      if (words > wbx::kF0SpanWords || s.G * s.F > 8u || s.G * wbx::kF0WaveLags <= tau_max) return 5;   // what the kernel relies on
      std::printf("s %u %u %u\n", (unsigned)s.G, (unsigned)s.F, (unsigned)words);
    }
  }
  static_assert(wbx::kF0MaxHops == 1ull << 20 && wbx::kF0MaxWindow == 8192 && wbx::kF0MaxTauMax == 4095, "the header's text names these");
  static_assert(sizeof(wbx_f0_frame) == 32 && sizeof(wbx_f0_info) == 32, "the header's text names these");
  std::printf("f0 ok\n");
  return 0;
}
