// resample_table_main.cpp — wbx_resample.h by itself (no HIP, no library): every coefficient table of the test list built and
// reduced to a checksum, the refusals walked.  tests/test_resample_host.py compiles this with -fsanitize=address,undefined
// and runs it directly; the checksums are compared with the numpy twin's tables.
#include <cstdio>
#include <vector>

#include "../../whitebox_amd/csrc/wbx_resample.h"

int main() {
  const uint32_t pairs[][2] = {{44100, 48000}, {48000, 44100}, {96000, 48000}, {48000, 96000},
                               {48000, 32000}, {192000, 44100}, {44100, 96000}, {8000, 44100}};
  for (const auto& pr : pairs) {
    for (int q = WBX_SRC_FAST; q <= WBX_SRC_BEST; q++) {
      wbx::ResamplePlan p;
      const char* why = "";
      if (wbx::resample_plan(pr[0], pr[1], q, &p, &why) != WBX_OK) {
        std::printf("%u %u %d refused: %s\n", pr[0], pr[1], q, why);
        return 1;
      }
      std::vector<float> tab((size_t)p.L * p.T);   // exactly the table: one float more written and the sanitizer says so
      wbx::resample_table(p, tab.data());
      uint32_t sum = 0;
      for (size_t i = 0; i < tab.size(); i++) {
        uint32_t b;
        __builtin_memcpy(&b, &tab[i], 4);
        sum ^= b * 2654435761u + (uint32_t)i;
      }
      std::printf("%u %u %d %08x\n", pr[0], pr[1], q, sum);
    }
  }
  wbx::ResamplePlan p;
  const char* why = "";
  bool ok = wbx::resample_plan(48000, 48000, WBX_SRC_GOOD, &p, &why) == WBX_ERR_INVALID;
  ok = ok && wbx::resample_plan(0, 48000, WBX_SRC_GOOD, &p, &why) == WBX_ERR_INVALID;
  ok = ok && wbx::resample_plan(44100, 48000, 3, &p, &why) == WBX_ERR_INVALID;
  ok = ok && wbx::resample_plan(11025, 192000, WBX_SRC_GOOD, &p, &why) == WBX_ERR_UNSUPPORTED;
  ok = ok && wbx::resample_plan(192000, 32000, WBX_SRC_BEST, &p, &why) == WBX_ERR_UNSUPPORTED;
  ok = ok && wbx::resample_plan(1, 4000000000u, WBX_SRC_FAST, &p, &why) == WBX_ERR_UNSUPPORTED;
  ok = ok && wbx::resample_plan(4000000000u, 1, WBX_SRC_FAST, &p, &why) == WBX_ERR_UNSUPPORTED;
  ok = ok && wbx::resample_out_frames(160, 147, ~0ull) == 0 && wbx::resample_out_frames(1, 2, 3) == 2;
  std::printf("refusals %s\n", ok ? "ok" : "WRONG");
  return ok ? 0 : 1;
}
