// C++ host reducing a take's noise through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded
// through process(input, output, sr), Engine::denoise_profile_sample over its first 1024 frames, wbx_denoise_threshold at
// strength 1, Engine::denoise_sample at W = 256 with a floor of 0.1, the result downloaded.  Writes the result to the file
// named by argv[1]; tests/test_gpu_denoise.py compares it with tests/denoise_model.py.  tests/test_denoise_host.py only
// compiles and links it.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 5, W = 256, B = W / 2 + 1;
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
  if (wbx_denoise_hops(n, W) != n / (W / 4) + 3 || wbx_denoise_launches(n, W, 1) != 1 || wbx_denoise_band_hops(W, 1) != (1u << 22) / W - 11) return 6;
  std::vector<double> sums(B), thr(B);
  const uint64_t hops = g_engine.denoise_profile_sample(ci.sample, 0, 1024, W, sums.data());
  if (hops != wbx_denoise_profile_hops(1024, W) || hops != 13) return 7;
  if (wbx_denoise_threshold(sums.data(), hops, B, 1.0, thr.data()) != WBX_OK) return 8;
  if (wbx_denoise_check(n, W, 2, 1, thr.data(), 1, 0.1) != WBX_OK) return 9;
  wbx_denoise_stats st{};
  const uint32_t id = g_engine.denoise_sample(ci.sample, 0, n, W, thr.data(), 0.1, 2, 1, &st);
  if (id == ci.sample) return 10;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 11;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 12;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter denoise ok %u hops %llu cells %llu open %llu bands %u\n", (unsigned)out.size(), (unsigned long long)st.hops,
              (unsigned long long)st.cells, (unsigned long long)st.open_cells, (unsigned)st.bands);
  return 0;
}
