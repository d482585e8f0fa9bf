// C++ host transposing a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), Engine::pitch_sample up a fifth (3/2) at its own length, WBX_SRC_GOOD, with a window of 256
// frames and a tolerance of 96, the result downloaded.  Writes the result to the file named by argv[1];
// tests/test_gpu_pitch.py compares it with tests/pitch_model.py.  tests/test_pitch_host.py only compiles and links it.
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
  if (wbx_pitch_mid_frames(n, 3, 2) != n * 3 / 2 || wbx_pitch_mid_frames(n, 5, 1) != 0 || wbx_pitch_max_steps() != 1u << 22) return 6;
  wbx_pitch_info pi{};
  const uint32_t id = g_engine.pitch_sample(ci.sample, 0, n, n, 3, 2, WBX_SRC_GOOD, 256, 96, &pi);
  if (id == ci.sample) return 9;
  if (pi.mid_frames != n * 3 / 2 || pi.L != 2 || pi.M != 3) return 12;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter pitch ok %u steps %llu searched %llu candidates %llu max_shift %u\n", (unsigned)out.size(),
              (unsigned long long)pi.steps, (unsigned long long)pi.searched_steps, (unsigned long long)pi.candidates, (unsigned)pi.max_shift);
  return 0;
}
