// C++ host limiting a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), Engine::limit_sample with a drive of 3 under a ceiling of 0.891251f (-1 dBFS), the result
// downloaded.  Writes the result to the file named by argv[1]; tests/test_gpu_limit.py compares it with
// tests/limit_model.py.
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
  double ramp[72 + 10 + 480];
  if (wbx_limit_ramp(72, 10, 480, ramp, sizeof ramp / sizeof ramp[0]) != WBX_OK || ramp[82] != 0.0 || !(ramp[83] > 0.0)) return 6;
  wbx_limit_stats ls{};
  wbx_clip_stats st{};
  const uint32_t id = g_engine.limit_sample(ci.sample, 0, n, 0.891251f, 3.0, 72, 10, 480, &ls, &st);
  if (id == ci.sample) return 9;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter limit ok %u peak %.9g limited %llu min_gain %.17g at %llu peak_in %.17g\n", (unsigned)out.size(), (double)st.peak[0],
              (unsigned long long)ls.limited_frames, ls.min_gain, (unsigned long long)ls.min_gain_frame, ls.peak_in);
  return 0;
}
