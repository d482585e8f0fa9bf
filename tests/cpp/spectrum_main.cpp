// spectrum_main.cpp — wbx_spectrum.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_spectrum_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   h <n> <W> <H>                                        -> "h <spectrum_hops>"
//   c <n> <channel> <W> <B> <H> <has_out> <cap>          -> "c <status of spectrum_check>"
//   l <W> <B>                                            -> "l <spectrum_launch_hops>"
//   n <hops> <W> <B>                                     -> "n <spectrum_launches>"
//   f <W> <B>                                            -> "f <spectrum_basis_frames>"
//   s <W> <B> <H>                                        -> "s <K> <G> <F> <chunk> <stride> <span>"
//   b <W> <B> <kind> <beta> <has_lengths> <B freqs> [<B lengths>] -> "b <status>", the words appended to the file argv[2]
//   g <f_min> <bins_per_octave> <n_bins>                 -> "g <status> <clamped> <the frequencies as %a>"
// Doubles are read with strtod, so hexadecimal floats, "nan" and "inf" are cases.  Ends with "spectrum ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_spectrum.h"

static double num(std::istringstream& ss) {
  std::string s;
  ss >> s;
  return std::strtod(s.c_str(), nullptr);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1]);
  FILE* words_out = std::fopen(argv[2], "wb");
  if (!words_out) return 3;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "h") {
      uint64_t n;
      uint32_t W, H;
      ss >> n >> W >> H;
      std::printf("h %" PRIu64 "\n", wbx::spectrum_hops(n, W, H));
    } else if (tag == "c") {
      wbx::SpecCall k{};
      int has_out;
      uint64_t cap;
      ss >> k.n_frames >> k.channel >> k.window >> k.bins >> k.hop >> has_out >> cap;
      k.has_out = has_out != 0;
      k.cells_cap = (size_t)cap;
      const char* why = "";
      const wbx_status st = wbx::spectrum_check(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;             // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "l") {
      uint32_t W, B;
      ss >> W >> B;
      std::printf("l %u\n", (unsigned)wbx::spectrum_launch_hops(W, B));
    } else if (tag == "n") {
      uint64_t hops;
      uint32_t W, B;
      ss >> hops >> W >> B;
      std::printf("n %" PRIu64 "\n", wbx::spectrum_launches(hops, W, B));
    } else if (tag == "f") {
      uint32_t W, B;
      ss >> W >> B;
      std::printf("f %" PRIu64 "\n", wbx::spectrum_basis_frames(W, B));
    } else if (tag == "s") {
      uint32_t W, B, H;
      ss >> W >> B >> H;
      const wbx::SpecShape s = wbx::spectrum_shape(W, B, H);
      // what the kernel relies on: the span fits its array, the waves fill the workgroup, aligned chunks
      if (s.span > wbx::kSpecSpanWords || s.F * s.stride > wbx::kSpecSpanWords || (s.K != 1u && s.K != 2u) ||
          s.G * (s.F / (wbx::kSpecLaneCells / s.K)) != wbx::kSpecWaves || 64u * s.K * s.G < (B < 512u ? B : 512u) || s.chunk % 4u != 0u ||
          s.chunk > W || (s.stride != H && s.stride != s.chunk))
        return 5;
      std::printf("s %u %u %u %u %u %u\n", (unsigned)s.K, (unsigned)s.G, (unsigned)s.F, (unsigned)s.chunk, (unsigned)s.stride, (unsigned)s.span);
    } else if (tag == "b") {
      uint32_t W, B;
      int kind, has_lengths;
      ss >> W >> B >> kind;
      const double beta = num(ss);
      ss >> has_lengths;
      const uint32_t rows = B <= wbx::kSpecMaxBins ? B : 0u;      // (a refused bin count comes without its lists)
      std::vector<double> freqs(rows);
      std::vector<uint32_t> lengths(rows);
      for (uint32_t b = 0; b < rows; b++) freqs[b] = num(ss);
      if (has_lengths)
        for (uint32_t b = 0; b < rows; b++) ss >> lengths[b];
      const uint64_t frames = wbx::spectrum_basis_frames(W, B);
      std::vector<float> out((size_t)frames, 7.0f);               // exactly as long as the header says: ASan sees a word too many
      const char* why = "";
      const wbx_status st = wbx::spectrum_basis(W, B, freqs.data(), has_lengths ? lengths.data() : nullptr, kind, beta, out.data(), &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 6;
      if (st != WBX_OK)
        for (float v : out)
          if (v != 7.0f) return 7;                                // a refusal leaves out untouched
      if (st == WBX_OK) std::fwrite(out.data(), sizeof(float), out.size(), words_out);
      std::printf("b %d\n", (int)st);
    } else if (tag == "g") {
      const double f_min = num(ss), bpo = num(ss);
      uint32_t n_bins;
      ss >> n_bins;
      std::vector<double> out(n_bins <= wbx::kSpecMaxBins ? n_bins : 0u);
      uint32_t clamped = 0;
      const char* why = "";
      const wbx_status st = wbx::spectrum_log_freqs(f_min, bpo, n_bins, out.data(), &clamped, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 8;
      std::printf("g %d %u", (int)st, (unsigned)clamped);
      if (st == WBX_OK)
        for (double v : out) std::printf(" %a", v);
      std::printf("\n");
    }
  }
  std::fclose(words_out);
  static_assert(wbx::kSpecMaxHops == 1ull << 20 && wbx::kSpecMaxWindow == 8192 && wbx::kSpecMaxCells == 1ull << 25, "the header's text names these");
  static_assert(sizeof(wbx_spectrum_info) == 16, "the header's text names this");
  std::printf("spectrum ok\n");
  return 0;
}
