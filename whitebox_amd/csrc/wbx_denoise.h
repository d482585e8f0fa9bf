// wbx_denoise.h — the host half of wbx_clip_denoise and wbx_clip_denoise_profile (wbx.h "Reducing a clip's noise"): the
// limits, the hop counts, the four transform tables (root-Hann window times cosine / sine, built on wbx_resample.h's sinpi,
// which is exact at integers), the threshold, the checks in their stated order, the bands and the launch shape of the two
// transform launches, and the tables as the device reads them.  Plain C++ (no HIP, no wbx_ctx, no libm beyond std::floor):
// tests/cpp/denoise_main.cpp compiles it with g++ alone, and tests/denoise_model.py restates it in numpy — the tables and the
// threshold must come out BIT FOR BIT the same there, so the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::isfinite, std::floor (correctly rounded, the same everywhere)
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/wbx.h"
#include "wbx_resample.h"   // resample_sinpi

namespace wbx {

constexpr uint32_t kDenMinWindow = 64, kDenMaxWindow = 2048;   // W: a power of two; H = W / 4, B = W / 2 + 1
constexpr uint32_t kDenMaxSmoothHops = 4, kDenMaxSmoothBins = 8;   // S, F
constexpr uint64_t kDenMaxFrames = (1ull << 31) - 16;          // n stays below it
constexpr uint32_t kDenLead = 3;                               // hop t starts at range frame (t - 3) H
constexpr uint32_t kDenStageWords = 1u << 22;                  // words of one stage buffer (cells; masked cells; chain values)
constexpr uint32_t kDenBandSlack = 2u * kDenMaxSmoothHops + kDenLead;   // hops a band computes beside its own blocks, at most
constexpr uint32_t kDenSpanWords = 4096;                       // LDS words of a transform workgroup's staged operand
constexpr uint32_t kDenChunk = 512;                            // terms staged at a time, at most
constexpr uint32_t kDenGateBins = 256;                         // bins of one gate workgroup

inline bool den_window_ok(uint32_t W) { return W >= kDenMinWindow && W <= kDenMaxWindow && (W & (W - 1u)) == 0u; }
inline bool den_frames_ok(uint64_t n) { return n >= 1u && n < kDenMaxFrames; }

// wbx_denoise_hops: T = ceil(n / H) + 3; 0 for a length or a window the call refuses
inline uint64_t denoise_hops(uint64_t n, uint32_t W) {
  if (!den_frames_ok(n) || !den_window_ok(W)) return 0;
  const uint32_t H = W / 4u;
  return (n + H - 1u) / H + kDenLead;
}
// the profile's: only complete windows, hop h at frame h H; 0 where the profile is refused
inline uint64_t denoise_profile_hops(uint64_t n, uint32_t W) {
  if (!den_frames_ok(n) || !den_window_ok(W) || n < W) return 0;
  return (n - W) / (W / 4u) + 1u;
}

// ---- the tables -----------------------------------------------------------------------------------------------------------------
// s[j] = sinpi((j + 0.5) / W), and over m = (k j) mod W, t = m / W: c[m] = sinpi(2 t + 0.5), z[m] = sinpi(2 t)
struct DenTrig {
  std::vector<double> s, c, z;
  explicit DenTrig(uint32_t W) : s(W), c(W), z(W) {
    for (uint32_t j = 0; j < W; j++) {
      s[j] = resample_sinpi(((double)j + 0.5) / (double)W);
      const double t = (double)j / (double)W;
      c[j] = resample_sinpi(2.0 * t + 0.5);
      z[j] = resample_sinpi(2.0 * t);
    }
  }
};
inline uint32_t den_m(uint32_t k, uint32_t j, uint32_t W) { return (k * j) & (W - 1u); }   // k j < 2^21
inline float den_ac(const DenTrig& g, uint32_t W, uint32_t k, uint32_t j) { return (float)((g.s[j] * g.c[den_m(k, j, W)]) / (double)W); }
inline float den_as(const DenTrig& g, uint32_t W, uint32_t k, uint32_t j) { return (float)(0.0 - ((g.s[j] * g.z[den_m(k, j, W)]) / (double)W)); }
inline double den_e(uint32_t W, uint32_t k) { return k == 0u || k == W / 2u ? 0.5 : 1.0; }
inline float den_yc(const DenTrig& g, uint32_t W, uint32_t k, uint32_t j) { return (float)(den_e(W, k) * (g.s[j] * g.c[den_m(k, j, W)])); }
inline float den_ys(const DenTrig& g, uint32_t W, uint32_t k, uint32_t j) { return (float)(0.0 - (den_e(W, k) * (g.s[j] * g.z[den_m(k, j, W)]))); }

// wbx_denoise_tables: analysis_out = AC[B][W] then AS[B][W], synthesis_out = YC[B][W] then YS[B][W] (2 B W floats each;
// either may be NULL and is left out then, not both)
inline wbx_status denoise_tables(uint32_t W, float* analysis_out, float* synthesis_out) {
  if (!den_window_ok(W) || (!analysis_out && !synthesis_out)) return WBX_ERR_INVALID;
  const DenTrig g(W);
  const uint32_t B = W / 2u + 1u;
  const size_t half = (size_t)B * W;
  for (uint32_t k = 0; k < B; k++)
    for (uint32_t j = 0; j < W; j++) {
      const size_t at = (size_t)k * W + j;
      if (analysis_out) analysis_out[at] = den_ac(g, W, k, j), analysis_out[half + at] = den_as(g, W, k, j);
      if (synthesis_out) synthesis_out[at] = den_yc(g, W, k, j), synthesis_out[half + at] = den_ys(g, W, k, j);
    }
  return WBX_OK;
}

// The tables as the device reads them, W x W floats each.  Rows 0 and B - 1 of AS and YS are all +0.0 (z is +-0 there and
// 0.0 - +-0 = +0.0), so the imaginary chain of those two bins stays +0.0 and their terms of a synthesis chain — which
// starts at +0.0 and therefore never holds -0.0 — add +-0 and change nothing.  What is left are W real chains of W terms
// either way, which the two layouts pack without a gap:
//   a cell row (W words)   word 0 = re[0], word 1 = re[B - 1], words 2 k, 2 k + 1 = re[k], im[k] for 0 < k < B - 1
//   analysis A[j][o]       o = 0: AC[0][j];  o = 1: AC[B - 1][j];  o = 2 k: AC[k][j];  o = 2 k + 1: AS[k][j]
//   a masked row (W words) word 0 = mr[0], words 2 k - 1, 2 k = mr[k], mi[k], word W - 1 = mr[B - 1]: the chain's own order
//   synthesis Y[i][j]      i = 0: YC[0][j];  i = 2 k - 1: YC[k][j];  i = 2 k: YS[k][j];  i = W - 1: YC[B - 1][j]
inline uint32_t den_cell_word(uint32_t W, uint32_t k) { return k == 0u ? 0u : k == W / 2u ? 1u : 2u * k; }     // of re[k]
inline uint32_t den_masked_word(uint32_t W, uint32_t k) { return k == 0u ? 0u : 2u * k - 1u; }                 // of mr[k]
inline void denoise_device_tables(uint32_t W, float* A, float* Y) {
  const DenTrig g(W);
  const uint32_t half = W / 2u;
  for (uint32_t j = 0; j < W; j++) {
    float* a = A + (size_t)j * W;
    a[0] = den_ac(g, W, 0, j), a[1] = den_ac(g, W, half, j);
    for (uint32_t k = 1; k < half; k++) a[2u * k] = den_ac(g, W, k, j), a[2u * k + 1u] = den_as(g, W, k, j);
    Y[j] = den_yc(g, W, 0, j);
    Y[(size_t)(W - 1u) * W + j] = den_yc(g, W, half, j);
    for (uint32_t k = 1; k < half; k++) {
      Y[(size_t)(2u * k - 1u) * W + j] = den_yc(g, W, k, j);
      Y[(size_t)(2u * k) * W + j] = den_ys(g, W, k, j);
    }
  }
}

// wbx_denoise_threshold: out = strength * (sum / (double)hops)
inline wbx_status denoise_threshold(const double* sums, uint64_t hops, size_t count, double strength, double* out) {
  if (!sums || !out || hops == 0 || !(strength >= 0.0) || !std::isfinite(strength)) return WBX_ERR_INVALID;
  for (size_t i = 0; i < count; i++) out[i] = strength * (sums[i] / (double)hops);
  return WBX_OK;
}

// ---- a call ---------------------------------------------------------------------------------------------------------------------
struct DenCall {
  uint64_t first_frame, n_frames;   // range of the source
  uint32_t window, smooth_hops, smooth_bins;   // W, S, F
  const double* thr;                // [channels][B]
  double floor;
};

// the arithmetic of a call, judged without a clip, in this order (all INVALID): n_frames, the window, S, F, a NULL thr, a
// thr entry, the floor.  `channels`: how many rows of thr are looked at — the clip's where it is known (1 or 2), else 1
inline wbx_status denoise_check_args(const DenCall& k, uint32_t channels, const char** why) {
  if (k.n_frames == 0) return *why = "clip denoise: no frames", WBX_ERR_INVALID;
  if (k.n_frames >= kDenMaxFrames) return *why = "clip denoise: n_frames reaches 2^31 - 16", WBX_ERR_INVALID;
  if (!den_window_ok(k.window)) return *why = "clip denoise: window_frames is not a power of two in 64 .. 2048", WBX_ERR_INVALID;
  if (k.smooth_hops > kDenMaxSmoothHops) return *why = "clip denoise: smooth_hops exceeds 4", WBX_ERR_INVALID;
  if (k.smooth_bins > kDenMaxSmoothBins) return *why = "clip denoise: smooth_bins exceeds 8", WBX_ERR_INVALID;
  if (!k.thr) return *why = "clip denoise: the threshold is NULL", WBX_ERR_INVALID;
  const size_t count = (size_t)channels * (k.window / 2u + 1u);
  for (size_t i = 0; i < count; i++)
    if (!(k.thr[i] >= 0.0) || !std::isfinite(k.thr[i])) return *why = "clip denoise: a threshold entry is negative or not finite", WBX_ERR_INVALID;
  if (!(k.floor >= 0.0 && k.floor <= 1.0)) return *why = "clip denoise: the floor is outside 0 .. 1", WBX_ERR_INVALID;   // (a NaN fails)
  return WBX_OK;
}
// the profile's: n_frames, the window, n_frames below the window, a NULL output
inline wbx_status denoise_profile_check_args(uint64_t n, uint32_t W, bool has_sums, bool has_hops, const char** why) {
  if (n == 0) return *why = "clip denoise profile: no frames", WBX_ERR_INVALID;
  if (n >= kDenMaxFrames) return *why = "clip denoise profile: n_frames reaches 2^31 - 16", WBX_ERR_INVALID;
  if (!den_window_ok(W)) return *why = "clip denoise profile: window_frames is not a power of two in 64 .. 2048", WBX_ERR_INVALID;
  if (n < W) return *why = "clip denoise profile: fewer frames than one window", WBX_ERR_INVALID;
  if (!has_sums || !has_hops) return *why = "clip denoise profile: an output is NULL", WBX_ERR_INVALID;
  return WBX_OK;
}

// ---- bands and launches -------------------------------------------------------------------------------------------------------
// A band owns consecutive BLOCKS of H output frames; block b lies under hops b .. b + 3.  The stage holds
// kDenStageWords / (W channels) hops; a band of blocks [b0, b1) synthesises hops [b0, b1 + 3) and analyses S more on either
// side (those that exist), so wbx_denoise_band_hops = the stage's hops less 2 * 4 + 3, whatever S is.  0 where refused
inline uint32_t denoise_band_hops(uint32_t W, uint32_t channels) {
  if (!den_window_ok(W) || channels < 1u || channels > 2u) return 0;
  return kDenStageWords / (W * channels) - kDenBandSlack;
}
// wbx_denoise_launches: the bands of a call, ceil(ceil(n / H) / band_hops); 0 where refused
inline uint64_t denoise_launches(uint64_t n, uint32_t W, uint32_t channels) {
  const uint32_t per = denoise_band_hops(W, channels);
  if (!per || !den_frames_ok(n)) return 0;
  const uint64_t blocks = (n + W / 4u - 1u) / (W / 4u);
  return (blocks + per - 1u) / per;
}
// the profile stages cells alone: its launches take the stage's whole hops
inline uint32_t denoise_profile_band_hops(uint32_t W, uint32_t channels) { return denoise_band_hops(W, channels) + kDenBandSlack; }

// denoise_transform_kernel's launch (both directions: W chains of W terms per hop and channel).  A lane owns K pairs of
// neighbouring chains (its own and, K = 2, the one 64 pairs on) x 8 / K consecutive hops; G of a workgroup's 4 waves stand
// side by side over the pairs, the 4 / G rows of waves own 8 / K hops each: hops_wg hops per workgroup.  The operand is
// staged in chunks of `chunk` terms; where the hops share their words (the analysis: a hop lies H frames behind the last)
// the rows lie H words apart, else chunk words
struct DenShape {
  uint32_t K, G, hops_wg, chunk, stride_shared, stride_own, pair_tiles;
};
inline DenShape denoise_shape(uint32_t W) {
  DenShape s{};
  const uint32_t pairs = W / 2u;
  s.K = pairs >= 128u ? 2u : 1u;
  const uint32_t wave_pairs = 64u * s.K;
  s.G = pairs >= 4u * wave_pairs ? 4u : pairs >= 2u * wave_pairs ? 2u : 1u;
  s.hops_wg = (8u / s.K) * (4u / s.G);
  s.chunk = W < kDenChunk ? W : kDenChunk;
  s.stride_shared = W / 4u;
  s.stride_own = s.chunk;
  s.pair_tiles = (pairs + wave_pairs * s.G - 1u) / (wave_pairs * s.G);
  return s;
}

}  // namespace wbx
