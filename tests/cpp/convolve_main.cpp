// convolve_main.cpp — wbx_convolve.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_convolve_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   f <rate> <kind> <f1 bits> <f2 bits> <n_taps> <beta bits> <cap>   -> "f <status> <cap floats as hex bits>"
//   n <n_frames> <ir_frames>                                         -> "n <wbx_convolve_frames>"
// doubles travel as the 16 hex digits of their bits, floats as 8.  The output buffer holds exactly <cap> floats (a design
// that wrote past n_taps, or past a capacity it should have refused, is the sanitizer's to see) and starts as 7.0f.
// Ends with "convolve ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_convolve.h"

static double from_bits(const std::string& w) {
  const uint64_t u = std::stoull(w, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}
static uint32_t to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
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
    if (tag == "f") {
      uint32_t rate, n_taps;
      int kind;
      size_t cap;
      std::string f1, f2, beta;
      ss >> rate >> kind >> f1 >> f2 >> n_taps >> beta >> cap;
      std::vector<float> out(cap, 7.0f);
      const wbx_status st = wbx::fir_design(rate, kind, from_bits(f1), from_bits(f2), n_taps, from_bits(beta), out.data(), cap);
      std::printf("f %d", (int)st);
      for (float v : out) std::printf(" %08" PRIx32, to_bits(v));
      std::printf("\n");
    } else if (tag == "n") {
      uint64_t n, l;
      ss >> n >> l;
      std::printf("n %" PRIu64 "\n", wbx::convolve_frames(n, l));
    }
  }
  float one[3];
  if (wbx::fir_design(48000, WBX_FIR_LOWPASS, 100.0, 0.0, 3, 5.0, nullptr, 3) != WBX_ERR_INVALID) return 4;
  if (wbx::fir_design(48000, WBX_FIR_LOWPASS, 100.0, 0.0, 3, 5.0, one, 3) != WBX_OK) return 5;
  static_assert(wbx::kConvolveTile == 2048 && wbx::kConvolveSegment == 2048, "the header's text names these");
  std::printf("convolve ok\n");
  return 0;
}
