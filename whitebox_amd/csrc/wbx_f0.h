// wbx_f0.h — the host half of wbx_clip_f0 (wbx.h "Tracking a clip's pitch"): the limits of a call and their check, the
// number of hops, how a call is cut into launches bounded by their terms, and how f0_kernel's workgroup is shaped.  Plain
// C++ (no HIP, no wbx_ctx, no libm): tests/cpp/f0_main.cpp compiles it with g++ alone, and tests/f0_model.py restates it in
// Python integers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint32_t kF0MinWindow = 64, kF0MaxWindow = 8192;      // W, a multiple of 8
constexpr uint32_t kF0MinTauMax = 8, kF0MaxTauMax = 4095;       // tau_max; tau_min in [2, tau_max - 1]
constexpr uint32_t kF0MaxHop = 1u << 20;                        // H
constexpr uint64_t kF0MaxFrames = (1ull << 31) - 16;            // n stays below it, like every pool clip's length
constexpr uint64_t kF0MaxHops = 1ull << 20;                     // the record buffer: at most 32 MB
// products W x (tau_max + 1) one launch may score: 2^39, measured at 34 - 36 ms with W >= 1024 (1.5 - 1.6e13 terms/s)
// and 43 ms at W = 256, H = 1 (MEASUREMENTS.md "Tracking a clip's pitch") — as long as the convolution's longest launch
// (about 40 ms)
constexpr uint64_t kF0LaunchTerms = 1ull << 39;
// f0_kernel's workgroup: 512 lanes, 8 consecutive lags per lane, so a wave owns 512 lags; the staged span (floats)
constexpr uint32_t kF0Lanes = 512, kF0PerLane = 8, kF0WaveLags = 512;
constexpr uint32_t kF0SpanWords = 14336;                        // 56 KB at most (f0_lds_bytes: a workgroup asks for its shape's): two on a CU
constexpr uint32_t kF0SpanSlack = 16;                           // what a lane's unused lags and its last turn's look ahead read

struct F0Call {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint32_t window, hop;             // W, H
  uint32_t tau_min, tau_max;
  double threshold;
  bool has_out;                     // frames_out is not NULL ...
  size_t frames_cap;                // ... and holds this many records
};

inline bool f0_shape_ok(uint32_t W, uint32_t H, uint32_t tau_min, uint32_t tau_max) {
  return W >= kF0MinWindow && W <= kF0MaxWindow && W % 8u == 0u && tau_max >= kF0MinTauMax && tau_max <= kF0MaxTauMax &&
         tau_min >= 2u && tau_min < tau_max && H >= 1u && H <= kF0MaxHop;
}

// hops = n >= W + tau_max ? (n - W - tau_max) / H + 1 : 0 — only complete frames count; 0 for a shape the call refuses
inline uint64_t f0_hops(uint64_t n, uint32_t W, uint32_t H, uint32_t tau_max) {
  if (!f0_shape_ok(W, H, 2u, tau_max)) return 0;
  const uint64_t need = (uint64_t)W + tau_max;
  return n >= need ? (n - need) / H + 1u : 0u;
}

// the arithmetic of a call, judged without a clip: what wbx_clip_f0 refuses before it looks at the source
inline wbx_status f0_check(const F0Call& k, const char** why) {
  if (k.n_frames == 0) return *why = "clip f0: no frames", WBX_ERR_INVALID;
  if (k.n_frames >= kF0MaxFrames) return *why = "clip f0: the range has 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (k.window < kF0MinWindow || k.window > kF0MaxWindow || k.window % 8u != 0u)
    return *why = "clip f0: window_frames is not a multiple of 8 in 64 .. 8192", WBX_ERR_INVALID;
  if (k.tau_max < kF0MinTauMax || k.tau_max > kF0MaxTauMax) return *why = "clip f0: tau_max outside 8 .. 4095", WBX_ERR_INVALID;
  if (k.tau_min < 2u || k.tau_min >= k.tau_max) return *why = "clip f0: tau_min outside 2 .. tau_max - 1", WBX_ERR_INVALID;
  if (k.hop < 1u || k.hop > kF0MaxHop) return *why = "clip f0: hop_frames outside 1 .. 2^20", WBX_ERR_INVALID;
  if (!(k.threshold > 0.0 && k.threshold <= 1.0)) return *why = "clip f0: threshold outside (0, 1], or a NaN", WBX_ERR_INVALID;
  const uint64_t hops = f0_hops(k.n_frames, k.window, k.hop, k.tau_max);
  if (hops > 0 && !k.has_out) return *why = "clip f0: frames_out is NULL", WBX_ERR_INVALID;
  if (k.frames_cap < hops) return *why = "clip f0: frames_cap is below the number of hops", WBX_ERR_INVALID;
  if (hops > kF0MaxHops) return *why = "clip f0: more than 2^20 hops", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// hops one launch takes: as many as stay within kF0LaunchTerms, whole eights where there are that many (a workgroup holds
// up to 8 hops), at least 1 (the widest hop is 8192 x 4096 = 2^25 terms); 0 for a shape the call refuses
inline uint32_t f0_launch_hops(uint32_t W, uint32_t tau_max) {
  if (!f0_shape_ok(W, 1u, 2u, tau_max)) return 0;
  const uint64_t h = kF0LaunchTerms / ((uint64_t)W * (tau_max + 1u));
  return (uint32_t)(h < 8u ? (h < 1u ? 1u : h) : (h > kF0MaxHops ? kF0MaxHops : h & ~7ull));
}
inline uint64_t f0_launches(uint64_t hops, uint32_t W, uint32_t tau_max) {
  const uint32_t per = f0_launch_hops(W, tau_max);
  return per ? (hops + per - 1u) / per : 0u;
}

// f0_kernel's shape: G waves per hop — ceil((tau_max + 1) / 512) rounded up to 1, 2, 4 or 8 — and F consecutive hops per
// workgroup, 8 / G halved until their shared span (F - 1) H + W + 512 G (+ slack) fits kF0SpanWords.  F = 1 always fits
struct F0Shape {
  uint32_t G, F;
};
inline uint32_t f0_span_words(uint32_t W, uint32_t H, uint32_t G, uint32_t F) {
  const uint64_t w = (uint64_t)(F - 1u) * H + W + (uint64_t)kF0WaveLags * G + kF0SpanSlack;
  return w > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)w;
}
inline F0Shape f0_shape(uint32_t W, uint32_t H, uint32_t tau_max) {
  const uint32_t waves = (tau_max + kF0WaveLags) / kF0WaveLags;   // ceil((tau_max + 1) / 512)
  F0Shape s{1u, 1u};
  while (s.G < waves) s.G *= 2u;
  s.F = 8u / s.G;
  while (s.F > 1u && f0_span_words(W, H, s.G, s.F) > kF0SpanWords) s.F /= 2u;
  return s;
}
static_assert(kF0MaxWindow + kF0WaveLags * 8u + kF0SpanSlack <= kF0SpanWords, "F = 1 always fits");
// dynamic LDS of a workgroup of that shape: the span's words as floats — or, where that is more, what lies over them after the
// chains: c as doubles, 8 per lane of the 64 G F.  At most 4 kF0SpanWords = 56 KB
inline uint32_t f0_lds_bytes(uint32_t W, uint32_t H, uint32_t G, uint32_t F) {
  const uint32_t span = 4u * f0_span_words(W, H, G, F), c = 64u * G * F * kF0PerLane * 8u;
  return span > c ? span : c;
}
static_assert(kF0Lanes * kF0PerLane * 8u <= 4u * kF0SpanWords, "c lies over the span");

}  // namespace wbx
