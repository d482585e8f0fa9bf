// loudness_main.cpp — wbx_loudness.h by itself (no HIP, no library): the K filter's coefficients at the rates named on the
// first line of the input and the gate over every case that follows.  tests/test_loudness_host.py compiles this with
// -fsanitize=address,undefined, writes the cases (random ones and the degenerate ones: 0 to 3 hops, all zero, everything
// below the absolute gate), runs it directly and compares the output with the numpy twin.
//   input   "R rate ..." then per case "C H hop" and C * H hop energies as the 16 hex digits of their bits
//   output  "rate" and 10 x 16 hex digits per rate; per case: gated_power's bits, hops, blocks, blocks_gated, hop_frames and
//           the four logarithmic figures as %.17g
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_loudness.h"

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  unsigned n_rates = 0;
  if (std::fscanf(f, "%u", &n_rates) != 1) return 2;
  for (unsigned i = 0; i < n_rates; i++) {
    unsigned rate = 0;
    if (std::fscanf(f, "%u", &rate) != 1 || !wbx::loudness_rate_ok(rate)) return 2;
    double k[10];
    wbx::loudness_coefficients(rate, k);
    std::printf("%u", rate);
    for (double v : k) std::printf(" %016" PRIx64, bits(v));
    std::printf("\n");
  }
  unsigned channels = 0, hop = 0;
  unsigned long long hops = 0;
  while (std::fscanf(f, "%u %llu %u", &channels, &hops, &hop) == 3) {
    if (channels < 1 || channels > 2 || hop == 0) return 2;
    std::vector<double> E((size_t)(channels * hops));   // exactly the energies: one double more read and the sanitizer says so
    for (double& v : E) {
      uint64_t b = 0;
      if (std::fscanf(f, "%" SCNx64, &b) != 1) return 2;
      std::memcpy(&v, &b, 8);
    }
    wbx_loudness r;
    wbx::loudness_gate(channels, hops, hop, E.data(), &r);
    std::printf("%016" PRIx64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %.17g %.17g %.17g %.17g\n", bits(r.gated_power), r.hops,
                r.blocks, r.blocks_gated, r.hop_frames, r.integrated, r.momentary_max, r.short_term_max, r.range_lu);
  }
  std::fclose(f);
  bool ok = wbx::loudness_hop_frames(11025) == 1103 && wbx::loudness_hop_frames(22050) == 2205 && wbx::loudness_hop_frames(8000) == 800;
  ok = ok && wbx::loudness_oversampling(95999) == 4 && wbx::loudness_oversampling(96000) == 2 && wbx::loudness_oversampling(192000) == 1;
  ok = ok && !wbx::loudness_rate_ok(7999) && !wbx::loudness_rate_ok(384001) && wbx::loudness_rate_ok(384000);
  std::printf("hops %s\n", ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}
