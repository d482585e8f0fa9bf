// wbx_filter.h — the host half of wbx_clip_filter (wbx.h "Filtering a clip"): the Audio-EQ-Cookbook designs, the test of a
// cascade's coefficients, one step of the cascade and the carry matrix of a chunk.  Plain C++ (no HIP, no wbx_ctx, no libm
// but sqrt and floor): the library calls it once per filter, tests/cpp/filter_main.cpp compiles it with g++ alone, and
// tests/filter_model.py restates it in numpy operation for operation — coefficients and matrix must come out BIT FOR BIT
// the same there.  Hence the trigonometry is wbx_resample.h's sinpi, and the file must be compiled without contraction
// (-ffp-contract=off).
#pragma once
#include <cmath>     // std::sqrt, std::isfinite
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_resample.h"   // resample_sinpi

namespace wbx {

constexpr uint32_t kFilterChunk = 512;         // frames per chunk: C
constexpr uint32_t kFilterMaxStages = 8;
constexpr uint32_t kFilterMaxDim = 2 * kFilterMaxStages + 2;   // D = 2 S + 2
constexpr uint64_t kFilterMaxFrames = (1ull << 31) - 16;       // n + tail stays below it, like every pool clip's length

// out[0..4] = b0 b1 b2 a1 a2 (a0 = 1).  Every line is one rounding per operator, in the order written
inline wbx_status filter_design(uint32_t rate, int kind, double f, double q, double gain, double out[5]) {
  if (!out || rate == 0) return WBX_ERR_INVALID;
  if (kind < WBX_FILT_LOWPASS || kind > WBX_FILT_HIGHSHELF) return WBX_ERR_INVALID;
  const double r = (double)rate;
  if (!(f > 0.0) || !(f < r / 2.0)) return WBX_ERR_INVALID;
  if (!std::isfinite(q) || !(q > 0.0)) return WBX_ERR_INVALID;
  if (!std::isfinite(gain) || !(gain > 0.0)) return WBX_ERR_INVALID;
  const double t = (2.0 * f) / r, h = f / r;
  const double sn = resample_sinpi(t), cs = resample_sinpi(t + 0.5);
  const double sh = resample_sinpi(h), ch = resample_sinpi(h + 0.5);
  const double hm = sh * sh, hp = ch * ch;     // (1 - cs) / 2, (1 + cs) / 2
  const double omc = 2.0 * hm, opc = 2.0 * hp; // 1 - cs, 1 + cs
  const double alpha = sn / (2.0 * q);
  const double m2cs = 0.0 - 2.0 * cs;
  double b0, b1, b2, a0, a1, a2;
  switch (kind) {
    case WBX_FILT_LOWPASS:
      a0 = 1.0 + alpha;
      b0 = hm, b1 = omc, b2 = hm;
      a1 = m2cs, a2 = 1.0 - alpha;
      break;
    case WBX_FILT_HIGHPASS:
      a0 = 1.0 + alpha;
      b0 = hp, b1 = 0.0 - opc, b2 = hp;
      a1 = m2cs, a2 = 1.0 - alpha;
      break;
    case WBX_FILT_BANDPASS:
      a0 = 1.0 + alpha;
      b0 = alpha, b1 = 0.0, b2 = 0.0 - alpha;
      a1 = m2cs, a2 = 1.0 - alpha;
      break;
    case WBX_FILT_NOTCH:
      a0 = 1.0 + alpha;
      b0 = 1.0, b1 = m2cs, b2 = 1.0;
      a1 = m2cs, a2 = 1.0 - alpha;
      break;
    case WBX_FILT_ALLPASS:
      a0 = 1.0 + alpha;
      b0 = 1.0 - alpha, b1 = m2cs, b2 = 1.0 + alpha;
      a1 = m2cs, a2 = 1.0 - alpha;
      break;
    case WBX_FILT_PEAK: {
      const double A = std::sqrt(gain);
      const double aA = alpha * A, aoA = alpha / A;
      a0 = 1.0 + aoA;
      b0 = 1.0 + aA, b1 = m2cs, b2 = 1.0 - aA;
      a1 = m2cs, a2 = 1.0 - aoA;
      break;
    }
    case WBX_FILT_LOWSHELF: {
      const double A = std::sqrt(gain);
      const double beta = (2.0 * std::sqrt(A)) * alpha;
      const double P = A * omc + opc, Q = A * opc + omc;   // (A+1) - (A-1) cs, (A+1) + (A-1) cs
      a0 = Q + beta;
      b0 = A * (P + beta), b1 = (2.0 * A) * (A * omc - opc), b2 = A * (P - beta);
      a1 = 0.0 - 2.0 * (A * opc - omc), a2 = Q - beta;
      break;
    }
    default: {   // WBX_FILT_HIGHSHELF
      const double A = std::sqrt(gain);
      const double beta = (2.0 * std::sqrt(A)) * alpha;
      const double P = A * omc + opc, Q = A * opc + omc;
      a0 = P + beta;
      b0 = A * (Q + beta), b1 = 0.0 - (2.0 * A) * (A * opc - omc), b2 = A * (Q - beta);
      a1 = 2.0 * (A * omc - opc), a2 = P - beta;
      break;
    }
  }
  out[0] = b0 / a0, out[1] = b1 / a0, out[2] = b2 / a0, out[3] = a1 / a0, out[4] = a2 / a0;
  return WBX_OK;
}

// finite values, 1 .. 8 stages, every stage strictly inside the stability triangle
inline wbx_status filter_check(const double* coef, uint32_t n_stages) {
  if (!coef || n_stages < 1 || n_stages > kFilterMaxStages) return WBX_ERR_INVALID;
  for (uint32_t s = 0; s < n_stages; s++) {
    const double* k = coef + 5 * s;
    for (int i = 0; i < 5; i++)
      if (!std::isfinite(k[i])) return WBX_ERR_INVALID;
    if (!(std::fabs(k[4]) < 1.0) || !(std::fabs(k[3]) < 1.0 + k[4])) return WBX_ERR_INVALID;
  }
  return WBX_OK;
}

// one frame through the cascade.  v = [x1, x2, y1_1, y2_1, ..., y1_S, y2_S]: stage s reads v[2s], v[2s+1] as its x1, x2
// (the stage before's y1, y2) and v[2s+2], v[2s+3] as its y1, y2.  Returns the last stage's y
inline double filter_step(const double* coef, uint32_t n_stages, double* v, double x) {
  double in = x;
  for (uint32_t s = 0; s < n_stages; s++) {
    const double* k = coef + 5 * s;
    const double x1 = v[2 * s], x2 = v[2 * s + 1], y1 = v[2 * s + 2], y2 = v[2 * s + 3];
    double y = k[0] * in + k[1] * x1;
    y = y + k[2] * x2;
    y = y - k[3] * y1;
    y = y - k[4] * y2;
    v[2 * s] = in, v[2 * s + 1] = x1;
    in = y;
  }
  v[2 * n_stages + 1] = v[2 * n_stages];
  v[2 * n_stages] = in;
  return in;
}

// M[i][k], D x D row-major: column k is the state after kFilterChunk frames of zero input from the unit state e_k
inline void filter_transition(const double* coef, uint32_t n_stages, double* M) {
  const uint32_t D = 2 * n_stages + 2;
  double v[kFilterMaxDim];
  for (uint32_t k = 0; k < D; k++) {
    for (uint32_t i = 0; i < D; i++) v[i] = i == k ? 1.0 : 0.0;
    for (uint32_t n = 0; n < kFilterChunk; n++) (void)filter_step(coef, n_stages, v, 0.0);
    for (uint32_t i = 0; i < D; i++) M[(size_t)i * D + k] = v[i];
  }
}

}  // namespace wbx
