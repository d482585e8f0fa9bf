// wbx_varispeed.h — the host half of wbx_clip_varispeed (wbx.h "Reading a clip along a position curve"): the filter plan of a
// guard ratio, the two phase-grid tables, the position of an output frame on the knot curve, the ordered check of a call
// and the tiles a call is launched over.  Plain C++ (no HIP, no wbx_ctx, no libm): the library and
// tests/cpp/varispeed_main.cpp compile it, tests/varispeed_model.py restates it in numpy operation for operation, and every
// table word, position and tile record must come out BIT FOR BIT the same there.  The filter's rows are wbx_resample.h's
// resample_row; compiled without contraction (-ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "wbx_resample.h"

namespace wbx {

constexpr uint32_t kVsMinShift = 4, kVsMaxShift = 10;
constexpr uint64_t kVsMaxKnots = 1ull << 22;
constexpr int64_t kVsMargin = 1ll << 16;          // frames a knot may lie before the range or behind it
constexpr uint32_t kVsTileMax = 1024, kVsSpanMax = 4096, kVsGridMax = 1u << 16;

struct VsPlan {
  uint32_t H = 0, T = 0;       // half width in source frames, taps = 2 H
  uint32_t P = 0, s = 0;       // phases (a power of two), s = 32 - log2 P: fr >> s is the phase, the low s bits are t
  double cutoff = 0.0, beta = 0.0;
  uint32_t row = 0;            // floats of one interleaved device row: 2 T rounded up to 16 (64 bytes)
};

inline uint32_t varispeed_phases(int quality) {
  switch (quality) {
    case WBX_SRC_FAST: return 256;
    case WBX_SRC_GOOD: return 512;
    case WBX_SRC_BEST: return 2048;
    default: return 0;
  }
}

inline uint64_t varispeed_gcd(uint64_t a, uint64_t b) {
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the quality (INVALID), the guard (INVALID), then resample_plan's filter for M / L = guard_num / guard_den (T > 512:
// UNSUPPORTED)
inline wbx_status varispeed_plan(int quality, uint32_t guard_num, uint32_t guard_den, VsPlan* p, const char** why) {
  ResampleQuality q;
  if (!resample_quality(quality, &q)) return *why = "varispeed: unknown quality", WBX_ERR_INVALID;
  if (guard_num == 0 || guard_den == 0) return *why = "varispeed: a guard of 0", WBX_ERR_INVALID;
  if (guard_num < guard_den) return *why = "varispeed: the guard is below 1", WBX_ERR_INVALID;
  const uint64_t g = varispeed_gcd(guard_num, guard_den);
  ResamplePlan r;
  const wbx_status st = resample_filter(guard_den / g, guard_num / g, q, &r, why, "varispeed: the guard needs more than 512 taps at this quality");
  if (st != WBX_OK) return st;
  p->H = r.H, p->T = r.T, p->cutoff = r.cutoff, p->beta = r.beta;
  p->P = varispeed_phases(quality);
  p->s = 32;
  for (uint32_t v = p->P; v > 1u; v >>= 1) p->s--;
  p->row = (2u * p->T + 15u) & ~15u;
  return WBX_OK;
}

// h[(P + 1) * T]: row p at frac = p / P (row P at exactly 1.0); d[P * T] = (float)((double)h[p + 1][k] - (double)h[p][k]).
// Either may be NULL
inline void varispeed_table(const VsPlan& p, float* h, float* d) {
  ResamplePlan r;
  r.H = p.H, r.T = p.T, r.cutoff = p.cutoff, r.beta = p.beta;
  const double i0b = resample_i0(p.beta);
  float prev[kResampleMaxTaps], cur[kResampleMaxTaps];
  for (uint32_t ph = 0; ph <= p.P; ph++) {
    resample_row(r, i0b, (double)ph / (double)p.P, cur);
    for (uint32_t k = 0; k < p.T; k++) {
      if (h) h[(size_t)ph * p.T + k] = cur[k];
      if (d && ph) d[(size_t)(ph - 1u) * p.T + k] = (float)((double)cur[k] - (double)prev[k]);
      prev[k] = cur[k];
    }
  }
}

// the device's copy: P rows of p.row floats, row p = h[p][0], D[p][0], h[p][1], D[p][1], ... and zeros behind 2 T
inline void varispeed_table_device(const VsPlan& p, float* out) {
  ResamplePlan r;
  r.H = p.H, r.T = p.T, r.cutoff = p.cutoff, r.beta = p.beta;
  const double i0b = resample_i0(p.beta);
  float prev[kResampleMaxTaps], cur[kResampleMaxTaps];
  resample_row(r, i0b, 0.0, prev);
  for (uint32_t ph = 0; ph < p.P; ph++) {
    resample_row(r, i0b, (double)(ph + 1u) / (double)p.P, cur);
    float* o = out + (size_t)ph * p.row;
    for (uint32_t k = 0; k < p.T; k++) {
      o[2u * k] = prev[k];
      o[2u * k + 1u] = (float)((double)cur[k] - (double)prev[k]);
      prev[k] = cur[k];
    }
    for (uint32_t k = 2u * p.T; k < p.row; k++) o[k] = 0.0f;
  }
}

// K = ceil(out_frames / G) + 1
inline uint64_t varispeed_knots(uint64_t out_frames, uint32_t g) { return ((out_frames + ((1ull << g) - 1u)) >> g) + 1u; }

// output frame j = i G + r lies at knots[i] + (((knots[i + 1] - knots[i]) * r) >> g): 64-bit product, arithmetic shift
// (it floors).  (i + 1 < n_knots, or r == 0)
inline int64_t varispeed_position(const int64_t* knots, uint32_t g, uint64_t j) {
  const uint64_t i = j >> g;
  const int64_t r = (int64_t)(j & ((1ull << g) - 1u));
  const int64_t k0 = knots[i];
  if (r == 0) return k0;
  return k0 + (((knots[i + 1u] - k0) * r) >> g);
}

struct VsCall {
  uint64_t first_frame, n_frames, out_frames;
  const int64_t* knots;
  uint64_t n_knots;
  uint32_t knot_shift;
  int quality;
  uint32_t guard_num, guard_den;
};

inline uint64_t varispeed_abs_diff(int64_t a, int64_t b) { return a < b ? (uint64_t)b - (uint64_t)a : (uint64_t)a - (uint64_t)b; }

// the call without its clip, in the header's order; *plan is filled once the guard has been accepted.  The reason of an
// interval past the span bound names it (kept per thread until the thread's next refusal of that kind)
inline wbx_status varispeed_check_args(const VsCall& c, VsPlan* plan, const char** why) {
  if (c.n_frames == 0 || c.out_frames == 0) return *why = "varispeed: no frames", WBX_ERR_INVALID;
  if (c.n_frames >= kResampleMaxFrames || c.out_frames >= kResampleMaxFrames)
    return *why = "varispeed: n_frames or out_frames reaches 2^31 - 16", WBX_ERR_INVALID;
  if (c.knot_shift < kVsMinShift || c.knot_shift > kVsMaxShift) return *why = "varispeed: knot_shift is not 4 .. 10", WBX_ERR_INVALID;
  if (!c.knots) return *why = "varispeed: the knots are NULL", WBX_ERR_INVALID;
  const uint64_t K = varispeed_knots(c.out_frames, c.knot_shift);
  if (c.n_knots != K) return *why = "varispeed: n_knots is not ceil(out_frames / 2^knot_shift) + 1", WBX_ERR_INVALID;
  ResampleQuality q;
  if (!resample_quality(c.quality, &q)) return *why = "varispeed: unknown quality", WBX_ERR_INVALID;
  if (c.guard_num == 0 || c.guard_den == 0) return *why = "varispeed: a guard of 0", WBX_ERR_INVALID;
  if (c.guard_num < c.guard_den) return *why = "varispeed: the guard is below 1", WBX_ERR_INVALID;
  if (K > kVsMaxKnots) return *why = "varispeed: more than 2^22 knots (use a greater knot_shift)", WBX_ERR_UNSUPPORTED;
  const wbx_status st = varispeed_plan(c.quality, c.guard_num, c.guard_den, plan, why);
  if (st != WBX_OK) return st;
  // (in frames: (n_frames + 2^16) * 2^32 may not fit 63 bits, and then every knot lies below it)
  const int64_t lo = -(kVsMargin << 32), hi_f = (int64_t)c.n_frames + kVsMargin;
  for (uint64_t i = 0; i < K; i++) {
    const int64_t f = c.knots[i] >> 32;
    if (c.knots[i] < lo || f > hi_f || (f == hi_f && (c.knots[i] & 0xFFFFFFFFll)))
      return *why = "varispeed: a knot lies more than 2^16 frames outside the range", WBX_ERR_INVALID;
  }
  for (uint64_t i = 0; i + 1u < K; i++)
    if ((varispeed_abs_diff(c.knots[i], c.knots[i + 1u]) >> 32) + 2u + plan->T > kVsSpanMax) {
      static thread_local char msg[160];
      std::snprintf(msg, sizeof msg, "varispeed: interval %llu moves too fast for one tile of 4096 frames: use a smaller knot_shift",
                    (unsigned long long)i);
      return *why = msg, WBX_ERR_UNSUPPORTED;
    }
  return WBX_OK;
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------
// A tile is a run of whole consecutive intervals chosen greedily from the front: at most 1024 output frames, and
// max_f - min_f + T <= 4096 over the run's count + 1 knots' frames (knot >> 32).  Every position of an interval lies between
// its two knots, so the staged span [min_f - (H - 1), max_f + H] holds every tap.  The check's interval bound lets every
// interval stand alone.  Returns the number of tiles; writes the first min(that, cap) records (out may be NULL with cap 0)
inline uint64_t varispeed_tiles(const int64_t* knots, uint64_t out_frames, uint32_t g, const VsPlan& p, wbx_varispeed_tile* out, uint64_t cap) {
  const uint64_t n_int = (out_frames + ((1ull << g) - 1u)) >> g;
  const uint64_t per = (uint64_t)kVsTileMax >> g;              // intervals of a tile at most
  uint64_t n = 0, i = 0;
  while (i < n_int) {
    int64_t mn = knots[i] >> 32, mx = mn;
    uint64_t cnt = 0;
    while (cnt < per && i + cnt < n_int) {
      const int64_t f = knots[i + cnt + 1u] >> 32;
      const int64_t a = f < mn ? f : mn, b = f > mx ? f : mx;
      if (cnt && (uint64_t)(b - a) + p.T > kVsSpanMax) break;
      mn = a, mx = b;
      cnt++;
    }
    if (n < cap) {
      const uint64_t first = i << g, end = (i + cnt) << g;
      wbx_varispeed_tile t;
      t.first_out = (uint32_t)first;
      t.n_out = (uint32_t)((end < out_frames ? end : out_frames) - first);
      t.lo_frame = mn - (int64_t)(p.H - 1u);
      t.span = (uint32_t)(mx - mn) + p.T;
      t.reserved = 0;
      out[n] = t;
    }
    n++;
    i += cnt;
  }
  return n;
}

}  // namespace wbx
