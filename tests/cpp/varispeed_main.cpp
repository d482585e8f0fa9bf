// varispeed_main.cpp — wbx_varispeed.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_varispeed_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   t <quality> <guard_num> <guard_den>   -> "t <status> <H> <T> <P> <fnv-1a 64 of h's bytes> <of d's bytes> <of the device copy's>"
//   k <knot_shift> <n> <knot 0> ... <knot n-1>  -> "k": the current curve (decimal 64-bit integers)
//   p <j>                                 -> "p <position of output frame j on the current curve>"
//   c <n_frames> <out_frames> <quality> <guard_num> <guard_den> <knots: 0 NULL, 1 current>  -> "c <status>"
//   l <n_frames> <out_frames> <quality> <guard_num> <guard_den>  -> "l <n_tiles> <first_out>:<n_out>:<lo_frame>:<span> ..."
// Ends with "varispeed ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_varispeed.h"

static uint64_t fnv(const std::vector<float>& v) {
  uint64_t h = 1469598103934665603ull;
  for (float f : v) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    for (int b = 0; b < 4; b++) h = (h ^ ((u >> (8 * b)) & 0xFFu)) * 1099511628211ull;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  std::vector<int64_t> knots;                                    // exactly the curve's length: ASan sees one knot too many
  uint32_t g = 4;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "t") {
      int quality;
      uint32_t gn, gd;
      ss >> quality >> gn >> gd;
      wbx::VsPlan p;
      const char* why = "";
      const wbx_status st = wbx::varispeed_plan(quality, gn, gd, &p, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 3;
      if (st != WBX_OK) {
        std::printf("t %d\n", (int)st);
        continue;
      }
      if (p.row % 16u || p.row < 2u * p.T || p.row >= 2u * p.T + 16u || (1u << (32u - p.s)) != p.P) return 4;
      std::vector<float> h((size_t)(p.P + 1u) * p.T), d((size_t)p.P * p.T), dev((size_t)p.P * p.row);
      wbx::varispeed_table(p, h.data(), d.data());
      wbx::varispeed_table_device(p, dev.data());
      for (uint32_t ph = 0; ph < p.P; ph++)                      // the device copy is the two tables interleaved, word by word
        for (uint32_t k = 0; k < p.row / 2u; k++) {
          const float wh = k < p.T ? h[(size_t)ph * p.T + k] : 0.0f, wd = k < p.T ? d[(size_t)ph * p.T + k] : 0.0f;
          if (std::memcmp(&dev[(size_t)ph * p.row + 2u * k], &wh, 4) || std::memcmp(&dev[(size_t)ph * p.row + 2u * k + 1u], &wd, 4)) return 5;
        }
      std::printf("t %d %u %u %u %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (int)st, p.H, p.T, p.P, fnv(h), fnv(d), fnv(dev));
    } else if (tag == "k") {
      size_t n;
      ss >> g >> n;
      knots.assign(n, 0);
      for (int64_t& v : knots) ss >> v;
      std::printf("k\n");
    } else if (tag == "p") {
      uint64_t j;
      ss >> j;
      if ((j >> g) >= knots.size()) return 6;
      std::printf("p %" PRId64 "\n", wbx::varispeed_position(knots.data(), g, j));
    } else if (tag == "c" || tag == "l") {
      wbx::VsCall k{};
      int has = 1;
      ss >> k.n_frames >> k.out_frames >> k.quality >> k.guard_num >> k.guard_den;
      if (tag == "c") ss >> has;
      k.knots = has ? knots.data() : nullptr;
      k.n_knots = knots.size();
      k.knot_shift = g;
      wbx::VsPlan p;
      const char* why = "";
      const wbx_status st = wbx::varispeed_check_args(k, &p, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 7;             // a refusal says why, an acceptance nothing
      if (tag == "c") {
        std::printf("c %d\n", (int)st);
        continue;
      }
      if (st != WBX_OK) return 8;
      const uint64_t n = wbx::varispeed_tiles(knots.data(), k.out_frames, g, p, nullptr, 0);
      std::vector<wbx_varispeed_tile> t(n);
      if (wbx::varispeed_tiles(knots.data(), k.out_frames, g, p, t.data(), n) != n) return 9;
      std::printf("l %" PRIu64, n);
      uint64_t next = 0;
      for (const wbx_varispeed_tile& r : t) {
        // what the kernel relies on: the tiles cover the outputs in order, start at a multiple of 16, hold at most 1024
        // outputs and 4096 staged frames, and every position of a tile lies inside its span
        if (r.first_out != next || r.first_out % 16u || r.n_out == 0 || r.n_out > 1024u || r.span > 4096u || r.span < p.T) return 10;
        for (uint64_t j = r.first_out; j < (uint64_t)r.first_out + r.n_out; j++) {
          const int64_t f = wbx::varispeed_position(knots.data(), g, j) >> 32;
          if (f - (int64_t)(p.H - 1u) < r.lo_frame || f + (int64_t)p.H >= r.lo_frame + (int64_t)r.span) return 11;
        }
        next += r.n_out;
        std::printf(" %u:%u:%" PRId64 ":%u", r.first_out, r.n_out, r.lo_frame, r.span);
      }
      if (next != k.out_frames) return 12;
      std::printf("\n");
    }
  }
  static_assert(sizeof(wbx_varispeed_tile) == 24 && sizeof(wbx_varispeed_info) == 32, "the header's text names these");
  std::printf("varispeed ok\n");
  return 0;
}
