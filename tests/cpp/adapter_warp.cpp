// C++ host warping a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), Engine::warp_sample along three markers to a result of 3001 frames with a window of 256
// frames and a tolerance of 96, the result downloaded.  Writes the result to the file named by argv[1];
// tests/test_gpu_warp.py compares it with tests/warp_model.py.  tests/test_warp_host.py only compiles and links it.
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

  const uint64_t n = (uint64_t)NB * F, m = 3001;
  const std::vector<wbx_warp_marker> markers = {{500, 700}, {1300, 1301}, {2100, 2750}};
  if (wbx_warp_check(n, m, markers.data(), 3, 256, 96) != WBX_OK) return 6;
  if (wbx_warp_steps(n, m, markers.data(), 3, 256) != 6 + 5 + 12 + 2) return 7;
  wbx_warp_info wi{};
  const uint32_t id = g_engine.warp_sample(ci.sample, 0, n, m, markers, 256, 96, &wi);
  if (id == ci.sample) return 9;
  std::vector<float> out(m);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter warp ok %u steps %llu searched %llu candidates %llu max_shift %u segments %u\n", (unsigned)out.size(),
              (unsigned long long)wi.steps, (unsigned long long)wi.searched_steps, (unsigned long long)wi.candidates,
              (unsigned)wi.max_shift, (unsigned)wi.segments);
  return 0;
}
