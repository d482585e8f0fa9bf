// stretch_main.cpp — wbx_stretch.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_stretch_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   s <m> <N>                          -> "s <stretch_steps>"
//   a <k> <n> <m> <N>                  -> "a <stretch_anchor>"
//   w <N> <cap>                        -> "w <status> <fnv-1a of the cap doubles' bits> <first> <last>"
//   c <n> <m> <N> <D> <wants> <cap>    -> "c <status of stretch_check_args>"
//   l <n> <N> <D>                      -> "l <stretch_launch_steps>"
//   b <K> <launch_steps>               -> "b <bands> <launches> <steps of all bands> <search launches of all bands>"
// The window's buffer holds exactly <cap> doubles (a table that wrote past N, or into a capacity it should have refused, is
// the sanitizer's to see) and starts as 7.0.  Ends with "stretch ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_stretch.h"

static uint64_t bits_of(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "s") {
      uint64_t m;
      uint32_t N;
      ss >> m >> N;
      std::printf("s %" PRIu64 "\n", wbx::stretch_steps(m, N));
    } else if (tag == "a") {
      uint64_t k, n, m;
      uint32_t N;
      ss >> k >> n >> m >> N;
      std::printf("a %" PRIu64 "\n", wbx::stretch_anchor(k, n, m, N));
    } else if (tag == "w") {
      uint32_t N;
      size_t cap;
      ss >> N >> cap;
      std::vector<double> out(cap, 7.0);
      const wbx_status st = wbx::stretch_window(N, out.data(), cap);
      uint64_t h = 1469598103934665603ull;
      for (double v : out) {
        const uint64_t u = bits_of(v);
        for (int i = 0; i < 8; i++) h = (h ^ ((u >> (8 * i)) & 0xFFu)) * 1099511628211ull;
      }
      std::printf("w %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (int)st, h, cap ? bits_of(out.front()) : 0,
                  cap ? bits_of(out.back()) : 0);
    } else if (tag == "c") {
      wbx::StretchCall k{};
      int wants;
      ss >> k.n_frames >> k.out_frames >> k.window >> k.tolerance >> wants >> k.positions_cap;
      k.wants_positions = wants != 0;
      const char* why = "";
      const wbx_status st = wbx::stretch_check_args(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;           // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "l") {
      uint64_t n;
      uint32_t N, D;
      ss >> n >> N >> D;
      std::printf("l %u\n", (unsigned)wbx::stretch_launch_steps(n, N, D));
    } else if (tag == "b") {
      uint64_t K, steps = 0, searches = 0;
      uint32_t per;
      ss >> K >> per;
      const uint64_t bands = wbx::stretch_bands(K);
      for (uint64_t i = 0; i < bands; i++) {
        const wbx::StretchBand b = wbx::stretch_band(K, per, i);
        if (b.first != i * wbx::kStretchBandSteps || b.steps == 0 || b.steps > wbx::kStretchBandSteps) return 3;
        steps += b.steps, searches += b.searches;
      }
      std::printf("b %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", bands, wbx::stretch_launches(K, per), steps, searches);
    }
  }
  if (wbx::stretch_window(64, nullptr, 64) != WBX_ERR_INVALID) return 5;
  if (wbx::stretch_band(10, 4, 7).steps != 0) return 6;         // a band past the end is empty
  static_assert(wbx::kStretchMaxWindow == 8192 && wbx::kStretchMaxTolerance == 4096 && wbx::kStretchPerLane == 8, "the header's text names these");
  std::printf("stretch ok\n");
  return 0;
}
