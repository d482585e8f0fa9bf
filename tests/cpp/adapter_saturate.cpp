// C++ host saturating a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), Engine::saturate_sample with a biased cubic table (wbx_saturate_table), a drive of 3 and a
// makeup of 0.5 at 4x oversampling, the result downloaded.  Writes the result to the file named by argv[1];
// tests/test_gpu_saturate.py compares it with tests/saturate_model.py.  tests/test_saturate_host.py only compiles and links it.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 5;
  wbx::Engine g_engine;
  g_engine.max_tracks = 8;
  g_engine.set_audio_channel_config(1, C, F, SR);
  g_engine.set_bpm(120.0);
  g_engine.add_track("take");
  g_engine.set_track_input(0, wbx::TrackInputType::ExternalMono, 0, true);
  g_engine.record();
  if (!g_engine.is_recording()) return 3;
  wbx::AudioBuffer<float> input(F, 1), output(F, C);
  for (uint32_t b = 0; b < NB; b++) {
    for (uint32_t i = 0; i < F; i++)   // 16 bits of a multiplicative hash around a DC offset: exact in fp32
      input.get_write_pointer(0)[i] = (float)(((b * F + i) * 2654435761u) & 0xFFFFu) / 65536.0f - 0.25f;
    g_engine.process(input, output, (double)SR);
    if (g_engine.process_status.load() != WBX_OK) {
      std::printf("process failed: %s\n", g_engine.process_error.c_str());
      return 4;
    }
  }
  g_engine.stop_record();
  wbx_clip_info ci{};
  if (wbx_engine_get_clip(g_engine.h, 0, 0, &ci) != WBX_OK) return 5;

  const uint64_t n = (uint64_t)NB * F;
  std::vector<double> table(WBX_SAT_TABLE);
  if (wbx_saturate_table(WBX_SAT_CUBIC, 0.25, table.data(), table.size()) != WBX_OK || wbx_saturate_check(table.data()) != WBX_OK) return 6;
  double mid = 1.0;
  if (wbx_saturate_lookup(table.data(), 0.0, &mid) != WBX_OK || mid != 0.0) return 7;
  uint32_t tile = 0, mid_span = 0, src_span = 0, lds = 0, tiles = 0;
  if (wbx_saturate_launch_shape(4, WBX_SRC_GOOD, 1, n, &tile, &mid_span, &src_span, &lds, &tiles) != WBX_OK || tile != 1024 || tiles != 3) return 8;
  wbx_saturate_stats ss{};
  wbx_clip_stats st{};
  const uint32_t id = g_engine.saturate_sample(ci.sample, 0, n, table.data(), 3.0, 0.5, 4, WBX_SRC_GOOD, &ss, &st);
  if (id == ci.sample) return 9;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter saturate ok %u peak %.9g peak_drive %.17g at %llu beyond %llu\n", (unsigned)out.size(), (double)st.peak[0],
              ss.peak_drive, (unsigned long long)ss.peak_index, (unsigned long long)ss.beyond);
  return 0;
}
