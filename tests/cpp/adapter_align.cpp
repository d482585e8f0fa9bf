// C++ host aligning a take with itself through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded
// through process(input, output, sr), Engine::align_samples with the take's frames [256, 1280) as the template against the
// whole take over the lags -300 .. 300 — the template is found 256 frames in.  Writes info and the curve to the file named by
// argv[1]; tests/test_gpu_align.py compares them with tests/align_model.py.  tests/test_align_host.py only compiles and links it.
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
    for (uint32_t i = 0; i < F; i++) {   // 8 bits of a multiplicative hash around zero: exact in fp32, and no period
      const uint32_t g = b * F + i;
      input.get_write_pointer(0)[i] = (float)((g * 2654435761u) >> 24) / 256.0f - 0.5f;
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

  const uint64_t m = (uint64_t)NB * F;
  if (wbx_align_chunks(1024) != 1 || wbx_align_chunks(1028) != 0 || wbx_align_max_lags() != 1u << 17 || wbx_align_chunk_frames() != 2048) return 6;
  if (wbx_align_check(1024, m, -300, 300, 0, 1, 1, 601) != WBX_OK || wbx_align_check(1024, m, -300, 300, 0, 1, 1, 600) != WBX_ERR_INVALID) return 7;
  std::vector<wbx_align_point> curve;
  const wbx_align_info ai = g_engine.align_samples(ci.sample, 256, 1024, ci.sample, 0, m, -300, 300, 0, &curve);
  if (curve.size() != 601 || ai.lags != 601 || ai.chunks != 1 || ai.terms != 601u * 1024u || ai.launches != wbx_align_launches(1024, 601)) return 8;
  if (ai.lag != 256 || ai.inverted != 0) return 9;
  const wbx_align_info again = g_engine.align_samples(ci.sample, 256, 1024, ci.sample, 0, m, -300, 300);   // without a curve
  if (again.lag != ai.lag || again.score != ai.score || again.offset != ai.offset) return 10;
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 11;
  std::fwrite(&ai, sizeof(ai), 1, f);
  std::fwrite(curve.data(), sizeof(wbx_align_point), curve.size(), f);
  std::fclose(f);
  std::printf("adapter align ok lag %d confidence %.6f\n", (int)ai.lag, ai.confidence);
  return 0;
}
