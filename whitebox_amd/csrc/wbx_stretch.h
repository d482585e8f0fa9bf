// wbx_stretch.h — the host half of wbx_clip_stretch (wbx.h "Stretching a clip"): the limits of a call and their check, the
// steps, the anchors, the window table, and how a call is cut into bands of positions and bounded search launches.  Plain
// C++ (no HIP, no wbx_ctx, no libm beyond std::floor): tests/cpp/stretch_main.cpp compiles it with g++ alone, and
// tests/stretch_model.py restates anchors and window in numpy — they must come out BIT FOR BIT the same there, so the file
// must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_resample.h"   // resample_sinpi

namespace wbx {

constexpr uint32_t kStretchMinWindow = 32, kStretchMaxWindow = 8192;   // N, a multiple of 8
constexpr uint32_t kStretchMaxTolerance = 4096;                 // D
constexpr uint64_t kStretchMaxFrames = (1ull << 31) - 16;       // n and m stay below it, like every pool clip's length
constexpr uint32_t kStretchMaxRatio = 8;                        // m <= 8 n and n <= 8 m
constexpr uint32_t kStretchLanes = 512, kStretchPerLane = 8;    // the search workgroup: lanes, consecutive candidates of a lane
constexpr uint32_t kStretchBandSteps = 1u << 16;                // steps whose positions the stage holds (and one before them)
// scored terms (candidates x Hs) one search launch may take if every one of its steps searches its whole span: 2^30, 38 - 41
// ms at the 2.6 - 2.8e10 terms/s measured with N = 2048, D = 512 (MEASUREMENTS.md "Stretching a clip")
constexpr uint64_t kStretchLaunchTerms = 1ull << 30;
// what a searched step costs besides its terms — staging, three barriers, the arg-max — counted in terms: 2.5 - 3.1 us were
// measured per searched step at N = 32 with 3 and with 49 candidates, 2^16 terms at the rate above are 2.4 us
constexpr uint64_t kStretchStepTerms = 1ull << 16;

struct StretchCall {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint64_t out_frames;              // m
  uint32_t window, tolerance;       // N, D
  bool wants_positions;             // positions_out is not NULL ...
  size_t positions_cap;             // ... and holds this many
};

inline bool stretch_window_ok(uint32_t N) { return N >= kStretchMinWindow && N <= kStretchMaxWindow && N % 8u == 0u; }

// K = ceil(m / Hs); 0 for a window the call refuses
inline uint64_t stretch_steps(uint64_t m, uint32_t N) {
  if (!stretch_window_ok(N)) return 0;
  const uint64_t Hs = N / 2u;
  return m / Hs + (m % Hs ? 1u : 0u);
}

// a_k = floor(k Hs n / m); 0 for a window the call refuses or m == 0 (any k, n and m may be asked about: 128 bits)
inline uint64_t stretch_anchor(uint64_t k, uint64_t n, uint64_t m, uint32_t N) {
  if (!stretch_window_ok(N) || m == 0) return 0;
  return (uint64_t)(((unsigned __int128)k * (N / 2u) * n) / m);
}

// w_up[i] = sinpi(i / N)^2 into out[i], w_dn[i] = 1 - w_up[i] into out[Hs + i], i in [0, Hs): N doubles
inline wbx_status stretch_window(uint32_t N, double* out, size_t cap_doubles) {
  if (!out || !stretch_window_ok(N) || cap_doubles < N) return WBX_ERR_INVALID;
  const uint32_t Hs = N / 2u;
  for (uint32_t i = 0; i < Hs; i++) {
    const double t = resample_sinpi((double)i / (double)N);
    const double up = t * t;
    out[i] = up;
    out[Hs + i] = 1.0 - up;
  }
  return WBX_OK;
}

// the arithmetic of a call, judged without a clip: what wbx_clip_stretch refuses before it looks at the source
inline wbx_status stretch_check_args(const StretchCall& k, const char** why) {
  if (k.n_frames == 0 || k.out_frames == 0) return *why = "clip stretch: no frames", WBX_ERR_INVALID;
  if (k.n_frames >= kStretchMaxFrames || k.out_frames >= kStretchMaxFrames)
    return *why = "clip stretch: the range or the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (!stretch_window_ok(k.window)) return *why = "clip stretch: window_frames is not a multiple of 8 in 32 .. 8192", WBX_ERR_INVALID;
  if (k.tolerance > kStretchMaxTolerance) return *why = "clip stretch: tolerance_frames above 4096", WBX_ERR_INVALID;
  if (k.wants_positions && k.positions_cap < stretch_steps(k.out_frames, k.window))
    return *why = "clip stretch: positions_cap is below the number of steps", WBX_ERR_INVALID;
  if (k.out_frames > kStretchMaxRatio * k.n_frames || k.n_frames > kStretchMaxRatio * k.out_frames)
    return *why = "clip stretch: a ratio beyond 8 either way", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// candidates a step of this call can score at most: min(2 D + 1, n)
inline uint64_t stretch_max_candidates(uint64_t n, uint32_t D) {
  const uint64_t c = 2ull * D + 1u;
  return c < n ? c : n;
}
// steps one search launch walks: as many as stay within kStretchLaunchTerms if every one searched its whole span, a step
// counted as its scored terms + kStretchStepTerms; at least 1 (the widest step is 8193 x 4096 = 2^25 terms), at most a band
inline uint32_t stretch_launch_steps(uint64_t n, uint32_t N, uint32_t D) {
  if (!stretch_window_ok(N) || n == 0) return 0;
  const uint64_t per_step = stretch_max_candidates(n, D) * (N / 2u) + kStretchStepTerms;
  const uint64_t s = kStretchLaunchTerms / per_step;
  return (uint32_t)(s < 1u ? 1u : s > kStretchBandSteps ? kStretchBandSteps : s);
}

// A call is issued band by band: steps [first, first + steps), whose positions the stage holds behind p_{first - 1}; per
// band ceil(steps / launch_steps) search launches, then one overlap-add launch
struct StretchBand {
  uint64_t first;              // the band's first step
  uint32_t steps;              // its steps (<= kStretchBandSteps)
  uint32_t searches;           // search launches
};
inline uint64_t stretch_bands(uint64_t K) { return (K + kStretchBandSteps - 1u) / kStretchBandSteps; }
inline StretchBand stretch_band(uint64_t K, uint32_t launch_steps, uint64_t i) {
  StretchBand b{};
  b.first = i * kStretchBandSteps;
  if (b.first >= K || launch_steps == 0) return b;
  const uint64_t left = K - b.first;
  b.steps = (uint32_t)(left < kStretchBandSteps ? left : kStretchBandSteps);
  b.searches = (b.steps + launch_steps - 1u) / launch_steps;
  return b;
}
// kernel launches of a whole call
inline uint64_t stretch_launches(uint64_t K, uint32_t launch_steps) {
  uint64_t total = 0;
  for (uint64_t i = 0, nb = stretch_bands(K); i < nb; i++) total += stretch_band(K, launch_steps, i).searches + 1u;
  return total;
}

}  // namespace wbx
