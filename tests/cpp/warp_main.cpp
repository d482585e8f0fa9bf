// wbx_warp.h stand-alone: the markers' check, the steps, the segments and the launch plan of wbx_clip_warp, with no HIP and
// no library.  tests/test_warp_host.py builds this file alone with -fsanitize=address,undefined and compares every line
// with tests/warp_model.py.  Reads cases from the file named by argv[1], one per record:
//   c n m N D M s t s t ...   -> "c status"
//   s n m N M s t ...         -> "s K"
//   g n m N M s t ...         -> "g status S checksum"   (checksum: the sum over segments j of (j + 1) * (s_j + 3 t_j + 5 base_j + 7 K_j), mod 2^64)
//   l n m N D M s t ...       -> "l launches"
//   p n m N D M s t ...       -> "p S_r longest round:count round:count ..." and every id list checked against its round
#include <cstdio>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_warp.h"

static bool read_markers(FILE* f, unsigned long long M, std::vector<wbx_warp_marker>& mk) {
  mk.clear();
  for (unsigned long long i = 0; i < M; i++) {
    unsigned long long s, t;
    if (std::fscanf(f, "%llu %llu", &s, &t) != 2) return false;
    mk.push_back(wbx_warp_marker{s, t});
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 3;
  char op;
  std::vector<wbx_warp_marker> mk;
  while (std::fscanf(f, " %c", &op) == 1) {
    unsigned long long n, m, N, D = 0, M;
    if (std::fscanf(f, "%llu %llu %llu", &n, &m, &N) != 3) return 4;
    if ((op == 'c' || op == 'l' || op == 'p') && std::fscanf(f, "%llu", &D) != 1) return 4;
    if (std::fscanf(f, "%llu", &M) != 1 || !read_markers(f, M, mk)) return 4;
    const wbx_warp_marker* p = mk.empty() ? nullptr : mk.data();
    if (op == 'c') {
      std::printf("c %d\n", (int)wbx::warp_check_sizes(n, m, p, (uint32_t)M, (uint32_t)N, (uint32_t)D));
    } else if (op == 's') {
      std::printf("s %llu\n", (unsigned long long)wbx::warp_steps(n, m, p, (uint32_t)M, (uint32_t)N));
    } else if (op == 'g') {
      std::vector<wbx_warp_segment> seg(M + 1u);                // exactly S records: a write past them is caught
      const wbx_status st = wbx::warp_segments(n, m, p, (uint32_t)M, (uint32_t)N, seg.data(), seg.size());
      uint64_t sum = 0;
      if (st == WBX_OK)
        for (size_t j = 0; j < seg.size(); j++)
          sum += (uint64_t)(j + 1u) * (seg[j].src_frame + 3u * seg[j].out_frame + 5u * seg[j].first_step + 7u * seg[j].steps);
      std::printf("g %d %llu %llu\n", (int)st, M + 1u, (unsigned long long)sum);
    } else if (op == 'l') {
      std::printf("l %llu\n", (unsigned long long)wbx::warp_launches(n, m, p, (uint32_t)M, (uint32_t)N, (uint32_t)D));
    } else if (op == 'p') {
      std::vector<wbx_warp_segment> seg(M + 1u);
      if (wbx::warp_segments(n, m, p, (uint32_t)M, (uint32_t)N, seg.data(), seg.size()) != WBX_OK) return 5;
      const wbx::WarpPlan pl = wbx::warp_plan(seg.data(), (uint32_t)seg.size(), wbx::stretch_launch_steps(n, (uint32_t)N, (uint32_t)D));
      std::printf("p %u %llu", pl.round_steps, (unsigned long long)pl.longest);
      size_t at = 0;
      for (const wbx::WarpLaunch& l : pl.launches) {
        if (l.first != at || l.count == 0 || l.count > wbx::kWarpLaunchSegments) return 6;
        for (uint32_t i = 0; i < l.count; i++) {                // live in this round, ascending within a launch
          const uint32_t j = pl.ids[l.first + i];
          if (j >= seg.size() || seg[j].steps <= (uint64_t)l.round * pl.round_steps) return 7;
          if (i > 0 && pl.ids[l.first + i - 1u] >= j) return 8;
        }
        at += l.count;
        std::printf(" %u:%u", l.round, l.count);
      }
      if (at != pl.ids.size()) return 9;
      std::printf("\n");
    } else {
      return 10;
    }
  }
  std::fclose(f);
  if (wbx::kWarpMaxMarkers != 65535u || wbx::kWarpMaxSteps != (1ull << 22)) return 11;
  std::printf("warp ok\n");
  return 0;
}
