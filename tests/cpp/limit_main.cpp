// limit_main.cpp — wbx_limit.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_limit_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   r <A> <H> <R> <cap>                                      -> "r <status> <fnv-1a of the cap doubles' bits> <first> <last>"
//   c <n> <ceiling bits> <drive bits> <A> <H> <R>            -> "c <status of limit_check_args>"
//   b <n> <A>                                                -> "b <bands> <frames, curve_frames, curve_tiles, apply_tiles of every band, summed>"
// doubles travel as the 16 hex digits of their bits, floats as 8.  The table's buffer holds exactly <cap> doubles (a table
// that wrote past A + H + R, or into a capacity it should have refused, is the sanitizer's to see) and starts as 7.0.
// Ends with "limit ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_limit.h"

static double from_bits(const std::string& w) {
  const uint64_t u = std::stoull(w, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}
static float float_from_bits(const std::string& w) {
  const uint32_t u = (uint32_t)std::stoul(w, nullptr, 16);
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}
static uint64_t to_bits(double d) {
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
    if (tag == "r") {
      uint32_t A, H, R;
      size_t cap;
      ss >> A >> H >> R >> cap;
      std::vector<double> out(cap, 7.0);
      const wbx_status st = wbx::limit_ramp(A, H, R, out.data(), cap);
      uint64_t h = 1469598103934665603ull;
      for (double v : out) {
        const uint64_t u = to_bits(v);
        for (int i = 0; i < 8; i++) h = (h ^ ((u >> (8 * i)) & 0xFFu)) * 1099511628211ull;
      }
      std::printf("r %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", (int)st, h, cap ? to_bits(out.front()) : 0, cap ? to_bits(out.back()) : 0);
    } else if (tag == "c") {
      wbx::LimitCall k{};
      std::string ceiling, drive;
      ss >> k.n_frames >> ceiling >> drive >> k.lookahead >> k.hold >> k.release;
      k.ceiling = float_from_bits(ceiling);
      k.drive = from_bits(drive);
      const char* why = "";
      const wbx_status st = wbx::limit_check_args(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 3;           // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "b") {
      uint64_t n;
      uint32_t A;
      ss >> n >> A;
      const uint64_t bands = wbx::limit_bands(n);
      uint64_t frames = 0, curve = 0, ct = 0, at = 0, next = 0;
      for (uint64_t i = 0; i < bands; i++) {
        const wbx::LimitBand b = wbx::limit_band(n, A, i);
        if (b.first != next || b.frames == 0 || b.frames > wbx::kLimitBand) return 4;   // the bands tile [0, n) in order
        if ((size_t)b.curve_frames > wbx::limit_stage_doubles(A)) return 5;             // ... and fit the stage
        next = b.first + b.frames;
        frames += b.frames, curve += b.curve_frames, ct += b.curve_tiles, at += b.apply_tiles;
      }
      if (next != n || wbx::limit_band(n, A, bands).frames != 0) return 6;
      std::printf("b %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", bands, frames, curve, ct, at);
    }
  }
  double one[3];
  if (wbx::limit_ramp(1, 1, 1, nullptr, 3) != WBX_ERR_INVALID) return 7;
  if (wbx::limit_ramp(1, 1, 1, one, 3) != WBX_OK || one[0] != 0.0 || one[2] != 0.0) return 8;
  static_assert(wbx::kLimitTile == 2048 && wbx::kLimitSegment == 2048 && wbx::kLimitBand == (1u << 20), "the header's text names these");
  std::printf("limit ok\n");
  return 0;
}
