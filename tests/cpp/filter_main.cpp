// filter_main.cpp — wbx_filter.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_filter_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   d <rate> <kind> <freq bits> <q bits> <gain bits>      -> "d <status> <5 coefficients as hex bits>"
//   c <n_stages> <5 * n_stages coefficient bits>          -> "c <status of filter_check>"
//   t <n_stages> <5 * n_stages coefficient bits>          -> "t <D> <D * D matrix entries as hex bits>"   (a checked cascade)
// doubles travel as the 16 hex digits of their bits, so nothing is lost in print or scan.  Ends with "filter ok".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_filter.h"

static double from_bits(const std::string& w) {
  const uint64_t u = std::stoull(w, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
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
    if (tag == "d") {
      uint32_t rate;
      int kind;
      std::string f, q, g;
      ss >> rate >> kind >> f >> q >> g;
      double out[5] = {7.0, 7.0, 7.0, 7.0, 7.0};
      const wbx_status st = wbx::filter_design(rate, kind, from_bits(f), from_bits(q), from_bits(g), out);
      std::printf("d %d", (int)st);
      for (double v : out) std::printf(" %016" PRIx64, to_bits(v));
      std::printf("\n");
    } else if (tag == "c" || tag == "t") {
      uint32_t n;
      ss >> n;
      std::vector<double> coef;                                // exactly the doubles given: the sanitizer sees a read past them
      std::string w;
      while (ss >> w) coef.push_back(from_bits(w));
      if (tag == "c") {
        std::printf("c %d\n", (int)wbx::filter_check(coef.empty() ? nullptr : coef.data(), n));
      } else {
        if (wbx::filter_check(coef.data(), n) != WBX_OK) return 3;
        const uint32_t D = 2 * n + 2;
        std::vector<double> M((size_t)D * D);
        wbx::filter_transition(coef.data(), n, M.data());
        std::printf("t %u", D);
        for (double v : M) std::printf(" %016" PRIx64, to_bits(v));
        std::printf("\n");
      }
    }
  }
  if (wbx::filter_design(48000, 0, 100.0, 1.0, 1.0, nullptr) != WBX_ERR_INVALID) return 4;
  if (wbx::filter_check(nullptr, 1) != WBX_ERR_INVALID) return 5;
  std::printf("filter ok\n");
  return 0;
}
