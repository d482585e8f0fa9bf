// C++ host finding a take's onsets and tempo through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take
// recorded through process(input, output, sr) — a noise burst of 256 frames every 2048 over a floor 36 dB below — then
// Engine::onsets_sample with hops of 64 frames and Engine::tempo_sample with windows of 64 hops every 8, lags 8 .. 63.
// Writes the onset records to the file named by argv[1] and the tempo records to argv[2]; tests/test_gpu_onsets.py compares
// them with tests/onset_model.py.  tests/test_onsets_host.py only compiles and links it.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 40;
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
    for (uint32_t i = 0; i < F; i++) {   // 8 bits of a multiplicative hash around zero, loud for 256 frames of 2048: exact in fp32
      const uint32_t g = b * F + i;
      input.get_write_pointer(0)[i] = ((float)((g * 2654435761u) >> 24) / 256.0f - 0.5f) * (g % 2048u < 256u ? 1.0f : 0.015625f);
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
  const uint64_t hops = wbx_onset_hops(n, 64);
  if (hops != n / 64 || wbx_onset_hops(n, 100) != 0 || wbx_onset_max_hops() != 1u << 20) return 6;
  if (wbx_onset_check(n, 64, 1e-9, 0.3, 0.1, 3, 8, 1, hops) != WBX_OK || wbx_onset_check(n, 64, 1e-9, 0.3, 0.1, 3, 8, 1, hops - 1) != WBX_ERR_INVALID)
    return 7;
  wbx_onset_info oi{};
  const std::vector<wbx_onset_frame> rec = g_engine.onsets_sample(ci.sample, 0, n, 64, 1e-9, 0.3, 0.1, 3, 8, &oi);
  if (rec.size() != hops || oi.hops != hops || oi.launches != 2) return 8;
  if (!g_engine.onsets_sample(ci.sample, 0, 63, 64).empty()) return 9;   // a range without a complete hop: no records
  uint64_t counted = 0;
  std::vector<wbx_onset_frame> again = rec;                        // the host-only pick gives the same flags
  if (wbx_onset_pick(again.data(), again.size(), 0.3, 0.1, 3, 8, &counted) != WBX_OK || counted != oi.onsets) return 10;
  for (size_t i = 0; i < rec.size(); i++)
    if (again[i].onset != rec[i].onset) return 10;
  wbx_f0_info fi{};
  const std::vector<wbx_f0_frame> tempo = g_engine.tempo_sample(ci.sample, 0, n, 64, 64, 8, 8, 63, 0.5, 1e-9, &fi);
  if (tempo.size() != (hops - 64 - 63) / 8 + 1 || fi.hops != tempo.size()) return 11;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 12;
  std::fwrite(rec.data(), sizeof(wbx_onset_frame), rec.size(), f);
  std::fclose(f);
  f = std::fopen(argv[2], "wb");
  if (!f) return 12;
  std::fwrite(tempo.data(), sizeof(wbx_f0_frame), tempo.size(), f);
  std::fclose(f);
  std::printf("adapter onsets ok %llu hops %llu onsets %llu windows %llu voiced\n", (unsigned long long)oi.hops,
              (unsigned long long)oi.onsets, (unsigned long long)fi.hops, (unsigned long long)fi.voiced_hops);
  return 0;
}
