// align_main.cpp — wbx_align.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_align_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   k <n>                                                     -> "k <align_chunks>"
//   c <n> <m> <lag_min> <lag_max> <flags> <has_info> <has_curve> <cap> -> "c <status of align_check>"
//   b <lags>                                                  -> "b <align_band_chunks>"
//   n <n> <lags>                                              -> "n <align_launches>"
//   s <lags>                                                  -> "s <waves> <blocks> <align_lds_bytes>"
// Ends with "align ok".
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../whitebox_amd/csrc/wbx_align.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "k") {
      uint64_t n;
      ss >> n;
      std::printf("k %u\n", (unsigned)wbx::align_chunks(n));
    } else if (tag == "c") {
      wbx::AlignCall k{};
      int has_info, has_curve;
      uint64_t cap;
      ss >> k.n >> k.m >> k.lag_min >> k.lag_max >> k.flags >> has_info >> has_curve >> cap;
      k.has_info = has_info != 0, k.has_curve = has_curve != 0;
      k.curve_cap = (size_t)cap;
      const char* why = "";
      const wbx_status st = wbx::align_check(k, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;             // a refusal says why, an acceptance nothing
      std::printf("c %d\n", (int)st);
    } else if (tag == "b") {
      uint64_t lags;
      ss >> lags;
      const uint32_t per = wbx::align_band_chunks(lags);
      // what the run relies on: a band's partials fit the stage, its terms the launch's bound
      if (per && per > 1u && ((uint64_t)per * lags > wbx::kAlignStageRecords || (uint64_t)per * lags * wbx::kAlignChunk > wbx::kAlignLaunchTerms)) return 5;
      std::printf("b %u\n", (unsigned)per);
    } else if (tag == "n") {
      uint64_t n, lags;
      ss >> n >> lags;
      std::printf("n %u\n", (unsigned)wbx::align_launches(n, lags));
    } else if (tag == "s") {
      uint64_t lags;
      ss >> lags;
      const wbx::AlignShape s = wbx::align_shape(lags);
      // what the kernel relies on: the waves cover the block's lags, the staged words fit the LDS asked for
      if (s.waves < 1u || s.waves > 8u || (uint64_t)s.waves * wbx::kAlignWaveLags < (lags < wbx::kAlignBlockLags ? lags : wbx::kAlignBlockLags)) return 6;
      if ((uint64_t)s.blocks * wbx::kAlignBlockLags < lags || wbx::align_lds_bytes(s.waves) > 65536u) return 7;
      std::printf("s %u %u %u\n", (unsigned)s.waves, (unsigned)s.blocks, (unsigned)wbx::align_lds_bytes(s.waves));
    }
  }
  static_assert(wbx::kAlignMaxLags == 1ull << 17 && wbx::kAlignMaxN == 1ull << 24 && wbx::kAlignChunk == 2048, "the header's text names these");
  static_assert(sizeof(wbx_align_info) == 80 && sizeof(wbx_align_point) == 16, "the header's text names these");
  std::printf("align ok\n");
  return 0;
}
