// wbx_loudness.h — the host half of wbx_clip_loudness (wbx.h "Measuring a clip's loudness"): hop arithmetic, the K-weighting
// coefficients and the gate over hop energies.  Plain C++ (no HIP, no wbx_ctx): the library calls it once per measurement,
// tests/cpp/loudness_main.cpp compiles it with g++ alone, and tests/loudness_model.py restates it in numpy operation for
// operation — the coefficients, every power and every count must come out BIT FOR BIT the same there.  Hence tan(x) is
// built here from + - * / in a fixed number of steps (libm's last place differs between platforms), the only libm calls are
// the log10s that turn a final power into LUFS or LU, and the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <algorithm>   // std::sort (of doubles: the result does not depend on the algorithm)
#include <cmath>       // std::log10, INFINITY
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint32_t kLoudMinRate = 8000, kLoudMaxRate = 384000;
constexpr int kLoudTrigTerms = 13;             // series terms behind the leading one; the argument stays below 0.67
constexpr double kLoudAbsGate = 1.1724653045822981e-07;   // 10^((-70 + 0.691) / 10)
constexpr uint32_t kLoudShortHops = 30, kLoudRangeStep = 10;

inline bool loudness_rate_ok(uint32_t rate) { return rate >= kLoudMinRate && rate <= kLoudMaxRate; }
inline uint32_t loudness_hop_frames(uint32_t rate) { return (rate + 5u) / 10u; }
inline uint32_t loudness_oversampling(uint32_t rate) { return rate < 96000u ? 4u : rate < 192000u ? 2u : 1u; }

// true_peak_kernel's launch: tiles of kPeakTile oversampled outputs (a multiple of every factor: a tile starts at phase 0),
// a capped grid that the kernel strides over the tiles by
constexpr uint32_t kPeakTile = 1024, kPeakGridMax = 1u << 16;
inline void true_peak_launch_shape(uint32_t factor, uint32_t n_in, uint32_t* n_tiles, uint32_t* grid) {
  *n_tiles = (n_in * factor + kPeakTile - 1u) / kPeakTile;     // (n_in * factor < 2^31 - 16)
  *grid = *n_tiles < kPeakGridMax ? *n_tiles : kPeakGridMax;
}

// K = tan(pi * f0 / rate): y = (pi * f0) / rate; sin and cos as alternating series in Horner form over y*y; one division
inline double loudness_tan(double f0, uint32_t rate) {
  const double y = (3.141592653589793 * f0) / (double)rate;
  const double y2 = y * y;
  double s = 1.0, c = 1.0;
  for (int n = kLoudTrigTerms; n >= 1; n--) {
    s = 1.0 - (s * y2) / (double)((2 * n) * (2 * n + 1));
    c = 1.0 - (c * y2) / (double)((2 * n - 1) * (2 * n));
  }
  return (y * s) / c;
}

// out[0..4]: stage 1's b0 b1 b2 a1 a2 (the shelf); out[5..9]: stage 2's (the high-pass)
inline void loudness_coefficients(uint32_t rate, double out[10]) {
  {
    const double Q = 0.7071752369554196, Vh = 1.5848647011308556, Vb = 1.2587209302325617;
    const double K = loudness_tan(1681.974450955533, rate);
    const double KQ = K / Q, KK = K * K;
    const double a0 = (1.0 + KQ) + KK;
    out[0] = ((Vh + Vb * KQ) + KK) / a0;
    out[1] = (2.0 * (KK - Vh)) / a0;
    out[2] = ((Vh - Vb * KQ) + KK) / a0;
    out[3] = (2.0 * (KK - 1.0)) / a0;
    out[4] = ((1.0 - KQ) + KK) / a0;
  }
  {
    const double Q = 0.5003270373238773;
    const double K = loudness_tan(38.13547087602444, rate);
    const double KQ = K / Q, KK = K * K;
    const double a0 = (1.0 + KQ) + KK;
    out[5] = 1.0;
    out[6] = -2.0;
    out[7] = 1.0;
    out[8] = (2.0 * (KK - 1.0)) / a0;
    out[9] = ((1.0 - KQ) + KK) / a0;
  }
}

inline double loudness_lufs(double power) { return power > 0.0 ? -0.691 + 10.0 * std::log10(power) : -INFINITY; }

// E: [channels][hops] hop energies.  Fills every field of *out but true_peak and oversampling (left 0).
inline void loudness_gate(uint32_t channels, uint64_t hops, uint32_t hop, const double* E, wbx_loudness* out) {
  *out = wbx_loudness{};
  out->hops = hops;
  out->hop_frames = hop;
  const uint64_t blocks = hops >= 4 ? hops - 3 : 0;
  out->blocks = blocks;
  const double* E0 = E;
  const double* E1 = channels > 1 ? E + hops : nullptr;

  // momentary blocks of 4 hops at every hop
  std::vector<double> z((size_t)blocks);
  const double block_frames = (double)(4ull * hop);
  double zmax = 0.0;
  for (uint64_t j = 0; j < blocks; j++) {
    double s = ((E0[j] + E0[j + 1]) + E0[j + 2]) + E0[j + 3];
    if (E1) s = s + (((E1[j] + E1[j + 1]) + E1[j + 2]) + E1[j + 3]);
    z[j] = s / block_frames;
    if (z[j] > zmax) zmax = z[j];
  }
  double sum = 0.0;
  uint64_t count = 0;
  for (uint64_t j = 0; j < blocks; j++)
    if (z[j] > kLoudAbsGate) sum = sum + z[j], count++;
  double gated = 0.0;
  uint64_t passed = 0;
  if (count) {
    const double rel = (sum / (double)count) * 0.1;
    sum = 0.0;
    for (uint64_t j = 0; j < blocks; j++)
      if (z[j] > kLoudAbsGate && z[j] > rel) sum = sum + z[j], passed++;
    if (passed) gated = sum / (double)passed;
  }
  out->gated_power = gated;
  out->blocks_gated = passed;
  out->integrated = loudness_lufs(gated);
  out->momentary_max = loudness_lufs(zmax);

  // short-term windows of 30 hops at every hop; those at every tenth hop feed the loudness range
  const uint64_t windows = hops >= kLoudShortHops ? hops - kLoudShortHops + 1 : 0;
  const double window_frames = (double)((uint64_t)kLoudShortHops * hop);
  double wmax = 0.0;
  std::vector<double> kept;
  for (uint64_t j = 0; j < windows; j++) {
    double s = 0.0;
    for (uint32_t k = 0; k < kLoudShortHops; k++) s = s + E0[j + k];
    double w = s / window_frames;
    if (E1) {
      s = 0.0;
      for (uint32_t k = 0; k < kLoudShortHops; k++) s = s + E1[j + k];
      w = w + s / window_frames;
    }
    if (w > wmax) wmax = w;
    if (j % kLoudRangeStep == 0 && w > kLoudAbsGate) kept.push_back(w);
  }
  out->short_term_max = loudness_lufs(wmax);
  double range = 0.0;
  if (!kept.empty()) {
    sum = 0.0;
    for (double w : kept) sum = sum + w;
    const double rel = (sum / (double)kept.size()) * 0.01;
    std::vector<double> s;
    for (double w : kept)
      if (w > rel) s.push_back(w);
    if (s.size() >= 2) {
      std::sort(s.begin(), s.end());
      const double top = (double)(s.size() - 1);
      const double lo = s[(size_t)(top * 0.10 + 0.5)], hi = s[(size_t)(top * 0.95 + 0.5)];
      range = 10.0 * std::log10(hi / lo);
    }
  }
  out->range_lu = range;
}

}  // namespace wbx
