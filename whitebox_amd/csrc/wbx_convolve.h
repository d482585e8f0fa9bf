// wbx_convolve.h — the host half of wbx_clip_convolve (wbx.h "Convolving a clip"): the kernel's shape constants, the limits
// of a call, the length of a full result and wbx_fir_design's Kaiser-windowed sinc.  Plain C++ (no HIP, no wbx_ctx, no libm
// but sqrt and floor): tests/cpp/convolve_main.cpp compiles it with g++ alone, and tests/convolve_model.py restates the
// design in numpy operation for operation — the taps must come out BIT FOR BIT the same there.  Hence sinc and I0 are
// wbx_resample.h's, and the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::sqrt, std::isfinite
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_resample.h"   // resample_sinc, resample_i0

namespace wbx {

constexpr uint32_t kConvolveTile = 2048;       // output frames a workgroup owns: 256 lanes x 8 frames
constexpr uint32_t kConvolveSegment = 2048;    // taps walked per staging of the source span: P
constexpr uint64_t kConvolveMaxTaps = 1ull << 20;
constexpr uint64_t kConvolveMaxWork = 1ull << 46;              // out_frames * ir_frames * channels, multiply-adds
constexpr uint64_t kConvolveMaxFrames = (1ull << 31) - 16;     // out_frames stays below it, like every pool clip's length
constexpr uint32_t kFirMinTaps = 3, kFirMaxTaps = 65535;

// n_frames + ir_frames - 1, or 0 where a call is refused whatever its window: no frames, no taps, more than 2^20 taps, a
// sum that does not fit 64 bits
inline uint64_t convolve_frames(uint64_t n_frames, uint64_t ir_frames) {
  if (n_frames == 0 || ir_frames == 0 || ir_frames > kConvolveMaxTaps) return 0;
  if (n_frames > UINT64_MAX - (ir_frames - 1)) return 0;
  return n_frames + (ir_frames - 1);
}

// the unnormalised low-pass tap k of n_taps at edge t = (2 f) / rate: (t * sinc(t * d)) * w[k].  i0b = I0(beta)
inline double fir_lp_tap(double t, uint32_t k, uint32_t c, double beta, double i0b) {
  const double d = (double)((int64_t)k - (int64_t)c);
  const double u = d / (double)c;
  double a = 1.0 - u * u;
  if (a < 0.0) a = 0.0;
  const double w = resample_i0(beta * std::sqrt(a)) / i0b;
  return (t * resample_sinc(t * d)) * w;
}

inline wbx_status fir_design(uint32_t rate, int kind, double f1, double f2, uint32_t n_taps, double beta, float* out, size_t cap_floats) {
  if (!out || rate == 0) return WBX_ERR_INVALID;
  if (kind < WBX_FIR_LOWPASS || kind > WBX_FIR_BANDSTOP) return WBX_ERR_INVALID;
  if (n_taps < kFirMinTaps || n_taps > kFirMaxTaps || (n_taps & 1u) == 0) return WBX_ERR_INVALID;
  if (cap_floats < n_taps) return WBX_ERR_INVALID;
  const double r = (double)rate;
  const bool band = kind == WBX_FIR_BANDPASS || kind == WBX_FIR_BANDSTOP;
  if (!(f1 > 0.0) || !(f1 < r / 2.0)) return WBX_ERR_INVALID;
  if (band && (!(f2 > 0.0) || !(f2 < r / 2.0) || !(f2 > f1))) return WBX_ERR_INVALID;
  if (!std::isfinite(beta) || !(beta >= 0.0) || !(beta <= 14.0)) return WBX_ERR_INVALID;
  const uint32_t c = (n_taps - 1u) / 2u;
  const double i0b = resample_i0(beta);
  const double t1 = (2.0 * f1) / r, t2 = band ? (2.0 * f2) / r : 0.0;
  double sum1 = 0.0, sum2 = 0.0;
  for (uint32_t k = 0; k < n_taps; k++) {
    sum1 = sum1 + fir_lp_tap(t1, k, c, beta, i0b);
    if (band) sum2 = sum2 + fir_lp_tap(t2, k, c, beta, i0b);
  }
  for (uint32_t k = 0; k < n_taps; k++) {
    const double delta = k == c ? 1.0 : 0.0;
    const double lp1 = fir_lp_tap(t1, k, c, beta, i0b) / sum1;
    double v;
    switch (kind) {
      case WBX_FIR_LOWPASS: v = lp1; break;
      case WBX_FIR_HIGHPASS: v = delta - lp1; break;
      case WBX_FIR_BANDPASS: v = fir_lp_tap(t2, k, c, beta, i0b) / sum2 - lp1; break;
      default: v = delta - (fir_lp_tap(t2, k, c, beta, i0b) / sum2 - lp1); break;   // WBX_FIR_BANDSTOP
    }
    out[k] = (float)v;
  }
  return WBX_OK;
}

}  // namespace wbx
