// wbx_spectrum.h — the host half of wbx_clip_spectrum (wbx.h "Seeing a clip's spectrum"): the limits of a call and their
// check, the number of hops, how a call is cut into launches bounded by their terms and by the stage for their cells, how
// spectrum_kernel's workgroup is shaped — and the basis builder and the logarithmic frequency grid.  Plain C++ (no HIP, no
// wbx_ctx, no libm beyond std::floor and std::sqrt): tests/cpp/spectrum_main.cpp compiles it with g++ alone, and
// tests/spectrum_model.py restates it in numpy — the basis words and the frequencies must come out BIT FOR BIT the same
// there, so the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::floor, std::sqrt, std::isfinite
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/wbx.h"
#include "wbx_dynamics.h"   // dyn_exp2
#include "wbx_resample.h"   // resample_sinpi, resample_i0

namespace wbx {

constexpr uint32_t kSpecMinWindow = 32, kSpecMaxWindow = 8192;  // W, a multiple of 4
constexpr uint32_t kSpecMaxHop = 65536;                         // H
constexpr uint32_t kSpecMaxBins = 1024;                         // B
constexpr uint64_t kSpecMaxBasis = 1ull << 21;                  // B W: the basis has 2 B W words, 16 MB at most
constexpr uint32_t kSpecMinLength = 4;                          // a bin's own window length L_b, up to W
constexpr double kSpecMaxBeta = 20.0;                           // Kaiser: resample_i0's 40 terms hold well past it
constexpr uint64_t kSpecMaxFrames = (1ull << 31) - 16;          // n stays below it, like every pool clip's length
constexpr uint64_t kSpecMaxHops = 1ull << 20;
constexpr uint64_t kSpecMaxCells = 1ull << 25;                  // hops B: 128 MB at the host
// terms hops W 2 B one launch may take: 2^37, about 10 ms at 1.3e13 multiply-adds per second (MEASUREMENTS.md "Seeing a
// clip's spectrum") ...
constexpr uint64_t kSpecLaunchTerms = 1ull << 37;
// ... and the cells it may leave in the device-side stage: 2^22 (16 MB), copied out before the next launch writes there.
// With W <= 8192 that is 2^36 terms at most: at the shapes the limits allow today the stage is the bound that binds
constexpr uint64_t kSpecStageCells = 1ull << 22;
// spectrum_kernel's workgroup: 4 waves; a lane owns 8 cells' chains — 4 consecutive hops x 2 bins (its own and the one 64
// further), or 8 hops x 1 bin where there are at most 64 bins, so that no lane's second bin lies idle — and a wave owns
// 4 hops x 128 bins or 8 x 64; G = 1, 2 or 4 waves stand side by side over the bins, 4 / G over the hops.  The window is
// walked in chunks of at most kSpecChunk terms; a chunk's span of the workgroup's hops is staged in LDS
constexpr uint32_t kSpecLanes = 256, kSpecWaves = 4, kSpecLaneCells = 8;
constexpr uint32_t kSpecChunk = 512;
constexpr uint32_t kSpecSpanWords = 8192;                                // 32 KB: F hops x the chunk
constexpr uint32_t kSpecMaxTileHops = kSpecWaves * kSpecLaneCells;       // 32

struct SpecCall {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint32_t channel;                 // 0, 1 or WBX_SPECTRUM_MID
  uint32_t window, bins, hop;       // W, B, H
  bool has_out;                     // power_out is not NULL ...
  size_t cells_cap;                 // ... and holds this many floats
};

inline bool spectrum_shape_ok(uint32_t W, uint32_t B, uint32_t H) {
  return W >= kSpecMinWindow && W <= kSpecMaxWindow && W % 4u == 0u && B >= 1u && B <= kSpecMaxBins &&
         (uint64_t)B * W <= kSpecMaxBasis && H >= 1u && H <= kSpecMaxHop;
}

// hops = n >= W ? (n - W) / H + 1 : 0 — only complete frames count; 0 for a window or hop length the call refuses
inline uint64_t spectrum_hops(uint64_t n, uint32_t W, uint32_t H) {
  if (!spectrum_shape_ok(W, 1u, H)) return 0;
  return n >= W ? (n - W) / H + 1u : 0u;
}

// frames of the basis clip: 2 B W; 0 for a shape the call refuses
inline uint64_t spectrum_basis_frames(uint32_t W, uint32_t B) { return spectrum_shape_ok(W, B, 1u) ? 2ull * B * W : 0u; }

// the arithmetic of a call, judged without a clip: what wbx_clip_spectrum refuses before it looks at source and basis
inline wbx_status spectrum_check(const SpecCall& k, const char** why) {
  if (k.n_frames == 0) return *why = "clip spectrum: no frames", WBX_ERR_INVALID;
  if (k.n_frames >= kSpecMaxFrames) return *why = "clip spectrum: the range has 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (k.channel != 0u && k.channel != 1u && k.channel != WBX_SPECTRUM_MID)
    return *why = "clip spectrum: channel is not 0, 1 or WBX_SPECTRUM_MID", WBX_ERR_INVALID;
  if (k.window < kSpecMinWindow || k.window > kSpecMaxWindow || k.window % 4u != 0u)
    return *why = "clip spectrum: window_frames is not a multiple of 4 in 32 .. 8192", WBX_ERR_INVALID;
  if (k.bins < 1u || k.bins > kSpecMaxBins) return *why = "clip spectrum: n_bins outside 1 .. 1024", WBX_ERR_INVALID;
  if ((uint64_t)k.bins * k.window > kSpecMaxBasis) return *why = "clip spectrum: n_bins x window_frames above 2^21", WBX_ERR_INVALID;
  if (k.hop < 1u || k.hop > kSpecMaxHop) return *why = "clip spectrum: hop_frames outside 1 .. 65536", WBX_ERR_INVALID;
  const uint64_t hops = spectrum_hops(k.n_frames, k.window, k.hop);
  const uint64_t cells = hops * k.bins;                          // < 2^41
  if (hops > 0 && !k.has_out) return *why = "clip spectrum: power_out is NULL", WBX_ERR_INVALID;
  if (k.cells_cap < cells) return *why = "clip spectrum: cells_cap is below hops x n_bins", WBX_ERR_INVALID;
  if (hops > kSpecMaxHops) return *why = "clip spectrum: more than 2^20 hops", WBX_ERR_UNSUPPORTED;
  if (cells > kSpecMaxCells) return *why = "clip spectrum: more than 2^25 cells", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// hops one launch takes: as many as stay within kSpecLaunchTerms and leave at most kSpecStageCells cells, in whole
// thirty-twos (a workgroup holds up to 32 hops; both bounds allow 4096 hops or more whatever the shape); 0 for a shape the
// call refuses
inline uint32_t spectrum_launch_hops(uint32_t W, uint32_t B) {
  if (!spectrum_shape_ok(W, B, 1u)) return 0;
  uint64_t h = kSpecLaunchTerms / (2ull * W * B);
  const uint64_t s = kSpecStageCells / B;
  if (s < h) h = s;
  if (h > kSpecMaxHops) h = kSpecMaxHops;
  return (uint32_t)(h & ~31ull);
}
static_assert(kSpecLaunchTerms / (2ull * kSpecMaxBasis) >= 4096 && kSpecStageCells / kSpecMaxBins >= 4096, "a launch takes whole thirty-twos");
inline uint64_t spectrum_launches(uint64_t hops, uint32_t W, uint32_t B) {
  const uint32_t per = spectrum_launch_hops(W, B);
  return per ? (hops + per - 1u) / per : 0u;
}

// spectrum_kernel's shape: K = 1 or 2 bins per lane (1 where B <= 64) and 8 / K hops; G waves side by side over the bins —
// ceil(B / (64 K)) rounded up to 1, 2 or 4, at most 4 — and F = (4 / G) (8 / K) consecutive hops per workgroup; the grid's
// y walks the bins in tiles of 64 K G.  The chunk is W, at most 512 and at most what F hops leave of the span each (256
// where F = 32).  The hops of a workgroup lie `stride` words apart in LDS: H where that is below the chunk (they share
// their words), else the chunk (they share none)
struct SpecShape {
  uint32_t K, G, F, chunk, stride, span;
};
inline SpecShape spectrum_shape(uint32_t W, uint32_t B, uint32_t H) {
  SpecShape s{B <= 64u ? 1u : 2u, 1u, 0u, 0u, 0u, 0u};
  const uint32_t wave_bins = 64u * s.K, waves = (B + wave_bins - 1u) / wave_bins;
  while (s.G < waves && s.G < kSpecWaves) s.G *= 2u;
  s.F = (kSpecWaves / s.G) * (kSpecLaneCells / s.K);
  s.chunk = kSpecSpanWords / s.F < kSpecChunk ? kSpecSpanWords / s.F : kSpecChunk;
  if (W < s.chunk) s.chunk = W;
  s.stride = H < s.chunk ? H : s.chunk;
  s.span = (s.F - 1u) * s.stride + s.chunk;                      // <= F chunk <= kSpecSpanWords
  return s;
}

// ---- the basis ----------------------------------------------------------------------------------------------------------------

// out[(i B + b) 2] = C_b[i], out[(i B + b) 2 + 1] = S_b[i] (wbx.h): bin b's window of L_b frames (NULL lengths: all W) centred
// in W at offset (W - L_b) / 2, zero outside; the window divided by its ascending fp64 sum; the phase t = f_b j (j counts
// from the window's first frame) less its integer part.  Every operator is one IEEE fp64 operation in the order written
inline wbx_status spectrum_basis(uint32_t W, uint32_t B, const double* freqs, const uint32_t* lengths, int kind, double beta, float* out,
                                 const char** why) {
  if (!spectrum_shape_ok(W, B, 1u)) return *why = "spectrum basis: window_frames, n_bins or their product out of range", WBX_ERR_INVALID;
  if (!freqs || !out) return *why = "spectrum basis: freqs or out is NULL", WBX_ERR_INVALID;
  if (kind != WBX_WINDOW_RECT && kind != WBX_WINDOW_HANN && kind != WBX_WINDOW_KAISER)
    return *why = "spectrum basis: unknown window kind", WBX_ERR_INVALID;
  if (kind == WBX_WINDOW_KAISER && !(beta >= 0.0 && beta <= kSpecMaxBeta)) return *why = "spectrum basis: kaiser_beta outside 0 .. 20, or a NaN", WBX_ERR_INVALID;
  for (uint32_t b = 0; b < B; b++) {
    if (!(freqs[b] >= 0.0 && freqs[b] <= 0.5)) return *why = "spectrum basis: a frequency outside 0 .. 0.5 cycles per frame, or a NaN", WBX_ERR_INVALID;
    if (lengths && (lengths[b] < kSpecMinLength || lengths[b] > W)) return *why = "spectrum basis: a window length outside 4 .. window_frames", WBX_ERR_INVALID;
  }
  const size_t words = (size_t)2u * B * W;
  for (size_t i = 0; i < words; i++) out[i] = 0.0f;
  const double i0b = kind == WBX_WINDOW_KAISER ? resample_i0(beta) : 1.0;
  std::vector<double> w(W);
  for (uint32_t b = 0; b < B; b++) {
    const uint32_t L = lengths ? lengths[b] : W;
    const uint32_t off = (W - L) / 2u;
    const double Ld = (double)L;
    double sum = 0.0;
    for (uint32_t j = 0; j < L; j++) {
      double v = 1.0;
      if (kind == WBX_WINDOW_HANN) {
        const double s = resample_sinpi(((double)j + 0.5) / Ld);
        v = s * s;
      } else if (kind == WBX_WINDOW_KAISER) {
        const double u = (((double)(2u * j + 1u)) - Ld) / Ld;
        double q = 1.0 - u * u;
        if (q < 0.0) q = 0.0;
        v = resample_i0(beta * std::sqrt(q)) / i0b;
      }
      w[j] = v;
      sum = sum + v;
    }
    const double f = freqs[b];
    for (uint32_t j = 0; j < L; j++) {
      const double wn = w[j] / sum;
      double t = f * (double)j;
      t = t - std::floor(t);
      const double t2 = 2.0 * t;
      const size_t at = ((size_t)(off + j) * B + b) * 2u;
      out[at] = (float)(wn * resample_sinpi(t2 + 0.5));
      out[at + 1u] = (float)(0.0 - (wn * resample_sinpi(t2)));
    }
  }
  return WBX_OK;
}

// out[b] = f_min / exp2(-(b / bins_per_octave)), f_min 2^(b / bins_per_octave) without libm; what exceeds 0.5 becomes 0.5
// and is counted into *clamped
inline wbx_status spectrum_log_freqs(double f_min, double bins_per_octave, uint32_t n_bins, double* out, uint32_t* clamped, const char** why) {
  if (!(f_min > 0.0 && f_min <= 0.5)) return *why = "spectrum log freqs: f_min outside (0, 0.5], or a NaN", WBX_ERR_INVALID;
  if (!(bins_per_octave > 0.0 && std::isfinite(bins_per_octave))) return *why = "spectrum log freqs: bins_per_octave not positive and finite", WBX_ERR_INVALID;
  if (n_bins < 1u || n_bins > kSpecMaxBins) return *why = "spectrum log freqs: n_bins outside 1 .. 1024", WBX_ERR_INVALID;
  if (!out) return *why = "spectrum log freqs: out is NULL", WBX_ERR_INVALID;
  uint32_t over = 0;
  for (uint32_t b = 0; b < n_bins; b++) {
    const double y = (double)b / bins_per_octave;
    double f = f_min / dyn_exp2(0.0 - y);
    if (!(f <= 0.5)) f = 0.5, over++;
    out[b] = f;
  }
  if (clamped) *clamped = over;
  return WBX_OK;
}

}  // namespace wbx
