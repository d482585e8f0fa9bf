// pitch_main.cpp — wbx_pitch.h alone, stand-alone (its own main, g++ only, no device, no library): what
// tests/test_pitch_host.py runs under AddressSanitizer and UBSan.  Reads a text file of cases, one per line:
//   m <out_frames> <num> <den>                          -> "m <pitch_mid_frames>"
//   r <num> <den>                                       -> "r <ok> <L> <M>"   (L and M as 0 where refused)
//   c <n> <m> <num> <den> <quality> <N> <D> <wants> <cap> -> "c <status of pitch_check_args> <m'> <K'> <L> <M> <H> <T>"
//                                                          (everything behind the status as 0 where refused)
//   t <L> <M> <T>                                       -> "t <pitch_tile> <pitch_span>"
// Ends with "pitch ok".
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../whitebox_amd/csrc/wbx_pitch.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "m") {
      uint64_t m;
      uint32_t num, den;
      ss >> m >> num >> den;
      std::printf("m %" PRIu64 "\n", wbx::pitch_mid_frames(m, num, den));
    } else if (tag == "r") {
      uint32_t num, den, L = 0, M = 0;
      ss >> num >> den;
      const bool ok = wbx::pitch_ratio_ok(num, den, &L, &M);
      std::printf("r %d %u %u\n", (int)ok, ok ? (unsigned)L : 0u, ok ? (unsigned)M : 0u);
    } else if (tag == "c") {
      wbx::PitchCall k{};
      int wants;
      ss >> k.n_frames >> k.out_frames >> k.num >> k.den >> k.quality >> k.window >> k.tolerance >> wants >> k.positions_cap;
      k.wants_positions = wants != 0;
      wbx::ResamplePlan plan;
      wbx::StretchCall sk{};
      const char* why = "";
      const wbx_status st = wbx::pitch_check_args(k, &plan, &sk, &why);
      if ((st == WBX_OK) != (why[0] == 0)) return 4;           // a refusal says why, an acceptance nothing
      if (st == WBX_OK) {
        if (sk.n_frames != k.n_frames || sk.first_frame != k.first_frame || sk.window != k.window || sk.tolerance != k.tolerance) return 5;
        std::printf("c 0 %" PRIu64 " %" PRIu64 " %u %u %u %u\n", sk.out_frames, wbx::stretch_steps(sk.out_frames, sk.window), (unsigned)plan.L,
                    (unsigned)plan.M, (unsigned)plan.H, (unsigned)plan.T);
      } else {
        std::printf("c %d 0 0 0 0 0 0\n", (int)st);
      }
    } else if (tag == "t") {
      uint32_t L, M, T;
      ss >> L >> M >> T;
      const uint32_t tile = wbx::pitch_tile(L, M, T);
      std::printf("t %u %u\n", (unsigned)tile, (unsigned)wbx::pitch_span(L, M, T, tile));
    }
  }
  static_assert(wbx::kPitchMaxSteps == 1u << 22 && wbx::kPitchMaxOctaves == 4, "the header's text names these");
  std::printf("pitch ok\n");
  return 0;
}
