// C++ host compressing a take through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded through
// process(input, output, sr), a 4:1 compressor table from wbx_dynamics_table (threshold -12 dB, knee 6 dB),
// Engine::dynamics_sample keyed by the take itself with a drive of 2 and a makeup of 1.5, the result downloaded.  Writes
// the result to the file named by argv[1]; tests/test_gpu_dynamics.py compares it with tests/dynamics_model.py.
// tests/test_dynamics_host.py only compiles and links it.
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
  std::vector<double> table(WBX_DYN_TABLE);
  double lo = 0.0, at_one = 0.0;
  if (wbx_dynamics_table(WBX_DYN_COMPRESS, -12.0, 4.0, 6.0, -40.0, table.data(), table.size()) != WBX_OK) return 6;
  if (wbx_dynamics_check(table.data(), WBX_DYN_COMPRESS, &lo) != WBX_OK || !(lo > 0.0 && lo < 1.0)) return 7;
  if (wbx_dynamics_lookup(table.data(), 1.0, &at_one) != WBX_OK || !(at_one < 1.0) || table[0] != 1.0) return 8;
  wbx_dynamics_stats ds{};
  wbx_clip_stats st{};
  const uint32_t id = g_engine.dynamics_sample(ci.sample, WBX_DYN_NO_KEY, 0, n, 0, WBX_DYN_COMPRESS, table.data(), 2.0, 1.0, 1.5, 48,
                                               10, 480, &ds, &st);
  if (id == ci.sample) return 9;
  std::vector<float> out(n);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter dynamics ok %u peak %.9g reduced %llu min_gain %.17g at %llu\n", (unsigned)out.size(), (double)st.peak[0],
              (unsigned long long)ds.reduced_frames, ds.min_gain, (unsigned long long)ds.min_gain_frame);
  return 0;
}
