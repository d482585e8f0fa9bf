// wbx_resample.h — the host half of wbx_clip_resample (wbx.h "Converting a clip's sample rate"): the plan of a conversion
// (ratio, filter length, output length, refusals) and the coefficient table.  Plain C++ (no HIP, no wbx_ctx, no libm): the
// library calls it once per conversion, tests/cpp/resample_table_main.cpp compiles it with g++ alone, and
// tests/resample_model.py restates it in numpy operation for operation — the table must come out BIT FOR BIT the same
// there.  Hence sin(pi x) and I0 are built here from + - * / floor sqrt in a fixed number of steps (glibc's sin and
// numpy's differ in the last place), and the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::floor, std::sqrt: correctly rounded, the same everywhere
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint32_t kResampleMaxL = 1280;       // phases (22050 -> 192000)
constexpr uint32_t kResampleMaxTaps = 512;
constexpr uint64_t kResampleMaxFrames = (1ull << 31) - 16;   // n_out stays below it, like every pool clip's length
constexpr int kResampleSinTerms = 13;          // series terms behind the leading one; the last is < 2e-23 at pi/2
constexpr int kResampleI0Terms = 40;           // (7^39 / 39!)^2 < 1e-25 at beta = 14

struct ResampleQuality {
  uint32_t zero_crossings;   // Z: the sinc's zero crossings on each side at the narrower of the two rates
  double beta;               // the Kaiser window's parameter
  double frac;               // cutoff as a fraction of the narrower Nyquist frequency
};
inline bool resample_quality(int quality, ResampleQuality* q) {
  switch (quality) {
    case WBX_SRC_FAST: *q = ResampleQuality{12, 7.0, 0.85}; return true;
    case WBX_SRC_GOOD: *q = ResampleQuality{24, 10.0, 0.92}; return true;
    case WBX_SRC_BEST: *q = ResampleQuality{48, 14.0, 0.96}; return true;
    default: return false;
  }
}

struct ResamplePlan {
  uint32_t L = 0, M = 0;     // dst_rate / g, src_rate / g: output frame j lies at source time j * M / L
  uint32_t H = 0, T = 0;     // half width in source frames, taps = 2 H
  double cutoff = 0.0, beta = 0.0;
};

inline uint32_t resample_gcd(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the ratio alone (no quality): WBX_ERR_INVALID for a rate of 0 or equal rates, WBX_ERR_UNSUPPORTED for L > 1280
inline wbx_status resample_ratio(uint32_t src_rate, uint32_t dst_rate, uint32_t* L, uint32_t* M, const char** why) {
  if (src_rate == 0 || dst_rate == 0) return *why = "resample: a sample rate of 0", WBX_ERR_INVALID;
  if (src_rate == dst_rate) return *why = "resample: the rates are equal (nothing to convert; the filter is not an identity)", WBX_ERR_INVALID;
  const uint32_t g = resample_gcd(src_rate, dst_rate);
  *L = dst_rate / g;
  *M = src_rate / g;
  if (*L > kResampleMaxL) return *why = "resample: the ratio needs more than 1280 phases", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// the filter of a reduced ratio M / L at a known quality (wbx_varispeed.h plans its guard ratio through it too): H, T, cutoff
// and beta; WBX_ERR_UNSUPPORTED for more than 512 taps, with the caller's reason
inline wbx_status resample_filter(uint64_t L, uint64_t M, const ResampleQuality& q, ResamplePlan* p, const char** why, const char* too_long) {
  // H = ceil(Z / rho) with rho = min(1, L / M), in integers: ceil(Z * M / L) when converting downwards
  const uint64_t H = L < M ? ((uint64_t)q.zero_crossings * M + L - 1) / L : q.zero_crossings;
  if (2 * H > kResampleMaxTaps) return *why = too_long, WBX_ERR_UNSUPPORTED;
  const double rho = L < M ? (double)L / (double)M : 1.0;
  p->H = (uint32_t)H;
  p->T = (uint32_t)(2 * H);
  p->cutoff = q.frac * rho;
  p->beta = q.beta;
  return WBX_OK;
}

inline wbx_status resample_plan(uint32_t src_rate, uint32_t dst_rate, int quality, ResamplePlan* p, const char** why) {
  ResampleQuality q;
  if (!resample_quality(quality, &q)) return *why = "resample: unknown quality", WBX_ERR_INVALID;
  uint32_t L = 0, M = 0;
  wbx_status st = resample_ratio(src_rate, dst_rate, &L, &M, why);
  if (st != WBX_OK) return st;
  st = resample_filter(L, M, q, p, why, "resample: the ratio needs more than 512 taps at this quality");
  if (st != WBX_OK) return st;
  p->L = L;
  p->M = M;
  return WBX_OK;
}

// ceil(n * L / M), or 0 where that reaches 2^31 - 16 (the product in 128 bits: any n_frames may be asked about)
inline uint64_t resample_out_frames(uint32_t L, uint32_t M, uint64_t n_frames) {
  const unsigned __int128 n_out = ((unsigned __int128)n_frames * L + (M - 1)) / M;
  return n_out < kResampleMaxFrames ? (uint64_t)n_out : 0;
}

// resample_kernel's launch (pitch_kernel's too): the tile is the most outputs (a multiple of 4, <= 1024) whose source span,
// ((L-1) + (tile-1) M) / L + T frames, fits 4096 floats — T <= 512 bounds M / L by 256 / 12, so tile >= 168 —; the grid is
// capped and the kernel strides over the tiles by it
constexpr uint32_t kResampleTileMax = 1024, kResampleSpanMax = 4096, kResampleGridMax = 1u << 16;
struct ResampleShape {
  uint32_t tile, span, n_tiles, grid;
};
inline uint32_t resample_span(uint32_t L, uint32_t M, uint32_t T, uint32_t tile) {
  return (uint32_t)(((uint64_t)(L - 1u) + (uint64_t)(tile - 1u) * M) / L) + T;
}
inline ResampleShape resample_launch_shape(uint32_t L, uint32_t M, uint32_t T, uint32_t n_out) {
  ResampleShape s;
  const uint64_t tm1 = (uint64_t)(kResampleSpanMax - T) * L / M;
  const uint64_t t = (tm1 + 1u) & ~3ull;
  s.tile = (uint32_t)(t < kResampleTileMax ? t : kResampleTileMax);
  s.span = resample_span(L, M, T, s.tile);
  s.n_tiles = (uint32_t)(((uint64_t)n_out + s.tile - 1u) / s.tile);
  s.grid = s.n_tiles < kResampleGridMax ? s.n_tiles : kResampleGridMax;
  return s;
}

// sin(pi x): x mod 2 reduced exactly to [0, 1/2], ONE multiplication by pi, the alternating series in Horner form
inline double resample_sinpi(double x) {
  double sign = 1.0;
  if (x < 0.0) x = 0.0 - x, sign = -1.0;
  double r = x - 2.0 * std::floor(x / 2.0);   // exact: x / 2 and the product are, and x mod 2 is representable
  if (r >= 1.0) r = r - 1.0, sign = 0.0 - sign;
  if (r > 0.5) r = 1.0 - r;
  const double y = 3.141592653589793 * r;
  const double y2 = y * y;
  double s = 1.0;
  for (int n = kResampleSinTerms; n >= 1; n--) s = 1.0 - (s * y2) / (double)((2 * n) * (2 * n + 1));
  return sign * (y * s);
}

inline double resample_sinc(double x) { return x == 0.0 ? 1.0 : resample_sinpi(x) / (3.141592653589793 * x); }

// I0(x) = sum over k of ((x/2)^k / k!)^2, kResampleI0Terms terms added in ascending k
inline double resample_i0(double x) {
  const double h = x / 2.0;
  double t = 1.0, s = 1.0;
  for (int k = 1; k < kResampleI0Terms; k++) {
    t = (t * h) / (double)k;
    s = s + t * t;
  }
  return s;
}

// one row of a table: the T coefficients at the fractional position `frac` (0 <= frac <= 1) of a filter (H, T, cutoff,
// beta; i0b = resample_i0(beta)), divided by their own ascending sum, rounded once to fp32
inline void resample_row(const ResamplePlan& p, double i0b, double frac, float* out) {
  const double Hd = (double)p.H;
  double row[kResampleMaxTaps];
  double sum = 0.0;
  for (uint32_t k = 0; k < p.T; k++) {
    const double d = (double)((int64_t)k - ((int64_t)p.H - 1)) - frac;
    const double u = d / Hd;
    double w = 1.0 - u * u;
    if (w < 0.0) w = 0.0;
    const double v = ((p.cutoff * resample_sinc(p.cutoff * d)) * resample_i0(p.beta * std::sqrt(w))) / i0b;
    row[k] = v;
    sum = sum + v;
  }
  for (uint32_t k = 0; k < p.T; k++) out[k] = (float)(row[k] / sum);
}

// out[p * T + k], p in [0, L), k in [0, T): phase p's coefficients, each phase divided by its own sum, rounded once to fp32
inline void resample_table(const ResamplePlan& p, float* out) {
  const double i0b = resample_i0(p.beta);
  for (uint32_t ph = 0; ph < p.L; ph++) resample_row(p, i0b, (double)ph / (double)p.L, out + (size_t)ph * p.T);
}

}  // namespace wbx
