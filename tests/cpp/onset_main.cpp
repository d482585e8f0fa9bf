// onset_main.cpp — wbx_onset.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_onsets_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   h <n> <H>                                                        -> "h <onset_hops>"
//   c <n> <H> <floor> <threshold> <delta> <w> <a> <has_out> <cap>    -> "c <status of onset_check>"
//   t <n> <H> <floor> <W> <step> <lag_min> <lag_max> <threshold> <has_out> <cap> -> "t <status of tempo_check>"
//   s <H> <hops>                                                     -> "s <q> <row> <grid> <lds_bytes>"
//   p <threshold> <delta> <w> <a> <N> <o_0> ... <o_N-1>              -> "p <count> <the N onset flags as 0/1>"
// Doubles are read with strtod, so "nan" and "inf" are cases; the o are floats' values in %.9g.  Ends with "onset ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_onset.h"

static double number(std::istringstream& ss) {
  std::string s;
  ss >> s;
  return std::strtod(s.c_str(), nullptr);
}

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
      uint32_t H;
      ss >> n >> H;
      std::printf("h %" PRIu64 "\n", wbx::onset_hops(n, H));
    } else if (tag == "c") {
      wbx::OnsetCall k{};
      int has_out;
      uint64_t cap;
      ss >> k.n_frames >> k.hop;
      k.floor_power = number(ss), k.threshold = number(ss), k.delta = number(ss);
      ss >> k.w >> k.a >> has_out >> cap;
      k.has_out = has_out != 0;
      k.frames_cap = (size_t)cap;
      const char* why = "";
      const wbx_status st = wbx::onset_check(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;             // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "t") {
      wbx::OnsetCall k{};
      wbx::F0Call f{};
      int has_out;
      uint64_t cap;
      ss >> k.n_frames >> k.hop;
      k.floor_power = number(ss);
      ss >> f.window >> f.hop >> f.tau_min >> f.tau_max;
      f.threshold = number(ss);
      ss >> has_out >> cap;
      f.has_out = has_out != 0;
      f.frames_cap = (size_t)cap;
      const char* why = "";
      const wbx_status st = wbx::tempo_check(k, &f, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;
      std::printf("t %d\n", (int)st);
    } else if (tag == "s") {
      uint32_t H;
      uint64_t hops;
      ss >> H >> hops;
      const wbx::OnsetShape s = wbx::onset_shape(H, hops);
      // what the kernel relies on: a wave's chunk holds min(q, 32) columns of 64 rows; every hop has a wave or the grid is full
      const uint32_t C = s.q < wbx::kOnsetChunk ? s.q : wbx::kOnsetChunk;
      if (s.row && (s.row < C || s.row % 2u == 0u || s.lds_bytes != wbx::kOnsetWaves * 64u * s.row * 4u || s.lds_bytes > 65536u)) return 5;
      if (!s.row && (s.lds_bytes || (s.q != 1u && s.q != 2u && s.q != 4u))) return 5;
      if (s.grid > wbx::kOnsetGridMax || (hops && !s.grid) || (s.grid < wbx::kOnsetGridMax && (uint64_t)s.grid * wbx::kOnsetWaves < hops)) return 5;
      std::printf("s %u %u %u %u\n", (unsigned)s.q, (unsigned)s.row, (unsigned)s.grid, (unsigned)s.lds_bytes);
    } else if (tag == "p") {
      const double threshold = number(ss), delta = number(ss);
      uint32_t w, a;
      uint64_t n;
      ss >> w >> a >> n;
      std::vector<wbx_onset_frame> rec((size_t)n);               // (exactly n: the sanitizer sees a step past either end)
      for (auto& r : rec) r.novelty = number(ss), r.onset = 7u;
      const uint64_t count = wbx::onset_pick(rec.data(), n, threshold, delta, w, a);
      std::printf("p %" PRIu64 " ", count);
      for (const auto& r : rec) std::putchar(r.onset ? '1' : '0');
      std::putchar('\n');
    }
  }
  static_assert(wbx::kOnsetMaxHops == 1ull << 20 && wbx::kOnsetMaxHop == 16384 && wbx::kOnsetMaxW == 64 && wbx::kOnsetMaxA == 256,
                "the header's text names these");
  static_assert(sizeof(wbx_onset_frame) == 32 && sizeof(wbx_onset_info) == 24, "the header's text names these");
  std::printf("onset ok\n");
  return 0;
}
