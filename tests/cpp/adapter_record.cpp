// C++ host recording through the reference-shaped adapter (include/wbx_adapter.hpp): set_track_input / record /
// process(input_buffer, output_buffer, sample_rate) / stop_record, written the way a reference host would (engine.h names).
// Writes every take (track order, channel after channel) to the file named by argv[1] and prints each clip's track and
// placement; tests/test_gpu_record.py compares them with tests/record_model.py.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 9, IN = 4;
  wbx::Engine g_engine;
  g_engine.max_tracks = 8;
  g_engine.set_audio_channel_config(IN, C, F, SR);
  g_engine.set_bpm(120.0);
  for (int i = 0; i < 3; i++) g_engine.add_track("t");
  g_engine.set_track_input(0, wbx::TrackInputType::ExternalStereo, 1, true);   // input channels 2 and 3
  g_engine.set_track_input(2, wbx::TrackInputType::ExternalMono, 0, false);
  g_engine.arm_track_recording(2, true);
  g_engine.record();
  if (!g_engine.is_recording()) return 3;

  wbx::AudioBuffer<float> input(F, IN), output(F, C);
  for (uint32_t b = 0; b < NB; b++) {
    for (uint32_t c = 0; c < IN; c++)
      for (uint32_t i = 0; i < F; i++) input.get_write_pointer(c)[i] = (float)((b * 4 + c) * 1000 + i);
    g_engine.process(input, output, (double)SR);
    if (g_engine.process_status.load() != WBX_OK) {
      std::printf("process failed: %s\n", g_engine.process_error.c_str());
      return 4;
    }
  }
  g_engine.stop_record();
  if (g_engine.is_recording()) return 5;

  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 6;
  for (uint32_t t : {0u, 2u}) {
    uint32_t n = 0;
    if (wbx_engine_clip_count(g_engine.h, t, &n) != WBX_OK || n != 1) return 7;
    wbx_clip_info ci{};
    if (wbx_engine_get_clip(g_engine.h, t, 0, &ci) != WBX_OK) return 8;
    wbx_record_info ri{};
    if (wbx_engine_record_info(g_engine.h, t, &ri) != WBX_OK || ri.frames != (uint64_t)NB * F || ri.status != 0) return 9;
    const uint32_t channels = t == 0 ? 2 : 1;
    std::vector<float> take(ri.frames);
    for (uint32_t ch = 0; ch < channels; ch++) {
      if (wbx_clip_download(wbx_engine_ctx(g_engine.h), ci.sample, ch, take.data()) != WBX_OK) return 10;
      std::fwrite(take.data(), sizeof(float), take.size(), f);
    }
    std::printf("clip %u %a %a\n", t, ci.min_time, ci.max_time);
  }
  std::fclose(f);
  std::printf("adapter record ok\n");
  return 0;
}
