// C++ host convolving a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), a linear-phase band-stop designed by wbx_fir_design and uploaded as a mono sample,
// Engine::convolve_sample with the filter's delay dropped, the result downloaded.  Writes the result to the file named by
// argv[1]; tests/test_gpu_convolve.py compares it with tests/convolve_model.py.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 5, TAPS = 255;
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

  std::vector<float> taps(TAPS);
  if (wbx_fir_design(SR, WBX_FIR_BANDSTOP, 3000.0, 9000.0, TAPS, 8.6, taps.data(), taps.size()) != WBX_OK) return 6;
  const void* planes[1] = {taps.data()};
  uint32_t fir = 0;
  if (wbx_engine_add_sample(g_engine.h, WBX_FMT_F32, 1, SR, TAPS, planes, &fir) != WBX_OK) return 7;
  const uint64_t n = (uint64_t)NB * F;
  if (wbx_convolve_frames(n, TAPS) != n + TAPS - 1) return 8;
  wbx_clip_stats st{};
  const uint32_t id = g_engine.convolve_sample(ci.sample, fir, 0, n, 0, TAPS, (TAPS - 1) / 2, n, 0.5, &st);
  if (id == ci.sample || id == fir) return 9;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter convolve ok %u peak %.9g\n", (unsigned)out.size(), (double)st.peak[0]);
  return 0;
}
