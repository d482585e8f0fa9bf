// C++ host reading a take along a position curve through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take
// recorded through process(input, output, sr), Engine::varispeed_sample along an integer-built curve (speed 3/4 for half of
// the result, then a glide up to 5/4, knot_shift 5, GOOD, guard 5/4), the result downloaded.  Writes the knots (int64) and
// then the result (float) to the file named by argv[1]; tests/test_gpu_varispeed.py compares it with
// tests/varispeed_model.py.  tests/test_varispeed_host.py only compiles and links it.
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

  const uint64_t n = (uint64_t)NB * F, out_frames = 2000;
  const uint32_t g = 5, G = 1u << g;
  const uint64_t K = (out_frames + G - 1) / G + 1;
  if (K > wbx_varispeed_max_knots()) return 6;
  std::vector<int64_t> knots(K);
  int64_t pos = 0;
  for (uint64_t i = 0; i < K; i++) {   // speed in 2^-32 frames per frame: 3/4, then up by 2^-6 per interval to at most 5/4
    knots[i] = pos;
    const int64_t up = i < K / 2 ? 0 : (int64_t)(i - K / 2) << 26;
    const int64_t speed = (3ll << 30) + (up < (2ll << 30) ? up : (2ll << 30));
    pos += speed * G;
  }
  if (wbx_varispeed_check(knots.data(), K, g, n, out_frames, WBX_SRC_GOOD, 5, 4) != WBX_OK) return 7;
  int64_t at = 0;
  if (wbx_varispeed_position(knots.data(), K, g, 33, &at) != WBX_OK || at != knots[1] + ((knots[2] - knots[1]) >> g)) return 8;
  uint64_t tiles = 0;
  if (wbx_varispeed_tiles(knots.data(), K, g, n, out_frames, WBX_SRC_GOOD, 5, 4, nullptr, 0, &tiles) != WBX_OK || tiles != 2) return 9;
  wbx_clip_stats st{};
  const uint32_t id = g_engine.varispeed_sample(ci.sample, 0, n, out_frames, knots.data(), K, g, WBX_SRC_GOOD, 5, 4, &st);
  if (id == ci.sample) return 10;
  std::vector<float> out(out_frames);
  if (wbx_clip_download(wbx_engine_ctx(g_engine.h), id, 0, out.data()) != WBX_OK) return 11;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 12;
  std::fwrite(knots.data(), sizeof(int64_t), knots.size(), f);
  std::fwrite(out.data(), sizeof(float), out.size(), f);
  std::fclose(f);
  std::printf("adapter varispeed ok %u knots %u peak %.9g\n", (unsigned)out.size(), (unsigned)K, (double)st.peak[0]);
  return 0;
}
