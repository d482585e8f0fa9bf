// C++ host looking at a take's spectrum through the reference-shaped adapter (include/wbx_adapter.hpp): a mono take recorded
// through process(input, output, sr), a Hann basis of 24 bins a semitone apart from 0.01 cycles per frame designed with
// wbx_spectrum_log_freqs / wbx_spectrum_basis and uploaded with add_sample, Engine::spectrum_sample with a window of 256
// frames and a hop of 64.  Writes the basis words and then the cells to the file named by argv[1]; tests/test_gpu_spectrum.py
// compares both with tests/spectrum_model.py.  tests/test_spectrum_host.py only compiles and links it.
#include <cstdio>
#include <vector>

#include "wbx_adapter.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t F = 512, C = 2, SR = 48000, NB = 5, W = 256, B = 24, H = 64;
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
  const uint64_t hops = wbx_spectrum_hops(n, W, H);
  if (hops != (n - W) / H + 1 || wbx_spectrum_hops(n, W + 2, H) != 0 || wbx_spectrum_max_cells() != 1u << 25) return 6;
  if (wbx_spectrum_basis_frames(W, B) != 2ull * W * B || wbx_spectrum_launch_hops(W, B) == 0) return 6;
  if (wbx_spectrum_check(n, WBX_SPECTRUM_MID, W, B, H, 1, hops * B) != WBX_OK ||
      wbx_spectrum_check(n, WBX_SPECTRUM_MID, W, B, H, 1, hops * B - 1) != WBX_ERR_INVALID)
    return 7;
  std::vector<double> freqs(B);
  uint32_t clamped = 9;
  if (wbx_spectrum_log_freqs(0.01, 12.0, B, freqs.data(), &clamped) != WBX_OK || clamped != 0) return 8;
  std::vector<float> words(2u * W * B);
  if (wbx_spectrum_basis(W, B, freqs.data(), nullptr, WBX_WINDOW_HANN, 0.0, words.data()) != WBX_OK) return 9;
  const void* rows[1] = {words.data()};
  const uint32_t basis = g_engine.add_sample(WBX_FMT_F32, 1, SR, words.size(), rows);
  wbx_spectrum_info si{};
  const std::vector<float> cells = g_engine.spectrum_sample(ci.sample, 0, n, WBX_SPECTRUM_MID, basis, W, B, H, &si);
  if (cells.size() != hops * B || si.hops != hops || si.bins != B || si.launches != 1) return 10;
  if (!g_engine.spectrum_sample(ci.sample, 0, W - 1, 0, basis, W, B, H).empty()) return 11;   // a range without a complete frame: no hops
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) return 12;
  std::fwrite(words.data(), sizeof(float), words.size(), f);
  std::fwrite(cells.data(), sizeof(float), cells.size(), f);
  std::fclose(f);
  std::printf("adapter spectrum ok %llu hops %u bins\n", (unsigned long long)si.hops, (unsigned)si.bins);
  return 0;
}
