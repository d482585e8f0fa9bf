// C++ host tracking a take's pitch through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded
// through process(input, output, sr), Engine::f0_sample with a window of 256 frames, a hop of 64, lags 8 .. 255 and a
// threshold of 0.2.  Writes the records to the file named by argv[1]; tests/test_gpu_f0.py compares them with
// tests/f0_model.py.  tests/test_f0_host.py only compiles and links it.
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
    for (uint32_t i = 0; i < F; i++) {   // a triangle wave of period 50 plus 8 bits of a multiplicative hash: exact in fp32
      const uint32_t g = b * F + i, ph = g % 50u;
      input.get_write_pointer(0)[i] = (float)(ph < 25u ? ph : 50u - ph) / 32.0f - 0.375f + (float)((g * 2654435761u) >> 24) / 4096.0f;
    }
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
  const uint64_t hops = wbx_f0_hops(n, 256, 64, 255);
  if (hops != (n - 256 - 255) / 64 + 1 || wbx_f0_hops(n, 260, 64, 255) != 0 || wbx_f0_max_hops() != 1u << 20) return 6;
  if (wbx_f0_check(n, 256, 64, 8, 255, 0.2, 1, hops) != WBX_OK || wbx_f0_check(n, 256, 64, 8, 255, 0.2, 1, hops - 1) != WBX_ERR_INVALID) return 7;
  wbx_f0_info fi{};
  const std::vector<wbx_f0_frame> rec = g_engine.f0_sample(ci.sample, 0, n, 256, 64, 8, 255, 0.2, &fi);
  if (rec.size() != hops || fi.hops != hops || fi.terms != hops * 256u * 256u || fi.launches != 1) return 8;
  if (!g_engine.f0_sample(ci.sample, 0, 510, 256, 64, 8, 255).empty()) return 9;   // a range without a complete frame: no hops
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(rec.data(), sizeof(wbx_f0_frame), rec.size(), f);
  std::fclose(f);
  std::printf("adapter f0 ok %llu hops %llu voiced\n", (unsigned long long)fi.hops, (unsigned long long)fi.voiced_hops);
  return 0;
}
