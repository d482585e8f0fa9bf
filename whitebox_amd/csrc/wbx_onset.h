// wbx_onset.h — the host half of wbx_clip_onsets and wbx_clip_tempo (wbx.h "Finding a clip's onsets and tempo"): the limits
// of a call and their check, the number of hops, the pick over the novelty, and how onset_energy_kernel is launched.  Plain
// C++ (no HIP, no wbx_ctx, no libm): tests/cpp/onset_main.cpp compiles it with g++ alone, and tests/onset_model.py restates
// it in Python.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_f0.h"

namespace wbx {

constexpr uint32_t kOnsetMinHop = 64, kOnsetMaxHop = 16384;     // H, a multiple of 64
constexpr uint64_t kOnsetMaxFrames = (1ull << 31) - 16;         // n stays below it, like every pool clip's length
constexpr uint64_t kOnsetMaxHops = 1ull << 20;                  // the record buffer: at most 32 MB
constexpr double kOnsetMinFloor = 1e-30, kOnsetMaxFloor = 1.0;  // floor_power
constexpr double kOnsetMaxThreshold = 2.0, kOnsetMaxDelta = 2.0;   // threshold in (0, 2], delta in [0, 2]
constexpr uint32_t kOnsetMaxW = 64, kOnsetMaxA = 256;           // the pick's neighbourhoods, in hops
// onset_energy_kernel: 4 waves per workgroup, a wave per hop, the grid striding over the hops; a lane whose run has 1, 2 or
// 4 frames reads it directly, every other run length goes through a wave-private LDS chunk of at most 32 columns per lane
constexpr uint32_t kOnsetLanes = 256, kOnsetWaves = kOnsetLanes / 64u, kOnsetGridMax = 2048, kOnsetChunk = 32;

struct OnsetCall {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint32_t hop;                     // H
  double floor_power;
  double threshold, delta;          // the pick (wbx_clip_tempo has none: onset_check_sizes alone judges its call)
  uint32_t w, a;
  bool has_out;                     // frames_out is not NULL ...
  size_t frames_cap;                // ... and holds this many records
};

inline bool onset_hop_ok(uint32_t H) { return H >= kOnsetMinHop && H <= kOnsetMaxHop && H % 64u == 0u; }

// hops = n / H — only complete hops count; 0 for a hop length the call refuses
inline uint64_t onset_hops(uint64_t n, uint32_t H) { return onset_hop_ok(H) ? n / H : 0u; }

// the range, the hop and the floor: what both calls judge first
inline wbx_status onset_check_sizes(uint64_t n, uint32_t H, double floor_power, const char** why) {
  if (n == 0) return *why = "clip onsets: no frames", WBX_ERR_INVALID;
  if (n >= kOnsetMaxFrames) return *why = "clip onsets: the range has 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (!onset_hop_ok(H)) return *why = "clip onsets: hop_frames is not a multiple of 64 in 64 .. 16384", WBX_ERR_INVALID;
  if (!(floor_power >= kOnsetMinFloor && floor_power <= kOnsetMaxFloor))
    return *why = "clip onsets: floor_power outside [1e-30, 1], or a NaN", WBX_ERR_INVALID;
  return WBX_OK;
}
inline wbx_status onset_check_pick(double threshold, double delta, uint32_t w, uint32_t a, const char** why) {
  if (!(threshold > 0.0 && threshold <= kOnsetMaxThreshold)) return *why = "clip onsets: threshold outside (0, 2], or a NaN", WBX_ERR_INVALID;
  if (!(delta >= 0.0 && delta <= kOnsetMaxDelta)) return *why = "clip onsets: delta outside [0, 2], or a NaN", WBX_ERR_INVALID;
  if (w > kOnsetMaxW) return *why = "clip onsets: w above 64", WBX_ERR_INVALID;
  if (a > kOnsetMaxA) return *why = "clip onsets: a above 256", WBX_ERR_INVALID;
  return WBX_OK;
}

// the arithmetic of an onsets call, judged without a clip: what wbx_clip_onsets refuses before it looks at the source
inline wbx_status onset_check(const OnsetCall& k, const char** why) {
  wbx_status st = onset_check_sizes(k.n_frames, k.hop, k.floor_power, why);
  if (st == WBX_OK) st = onset_check_pick(k.threshold, k.delta, k.w, k.a, why);
  if (st != WBX_OK) return st;
  const uint64_t hops = onset_hops(k.n_frames, k.hop);
  if (hops > 0 && !k.has_out) return *why = "clip onsets: frames_out is NULL", WBX_ERR_INVALID;
  if (k.frames_cap < hops) return *why = "clip onsets: frames_cap is below the number of hops", WBX_ERR_INVALID;
  if (hops > kOnsetMaxHops) return *why = "clip onsets: more than 2^20 hops", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// ... and of a tempo call: the sizes, the number of hops, then the track's own rules with n = hops (`track` holds window,
// hop, lags, threshold and the output; its n_frames is set here).  A range without a complete hop has its track's shape
// judged alone: wbx_f0_check refuses no frames, this call does not
inline wbx_status tempo_check(const OnsetCall& k, F0Call* track, const char** why) {
  const wbx_status st = onset_check_sizes(k.n_frames, k.hop, k.floor_power, why);
  if (st != WBX_OK) return st;
  const uint64_t hops = onset_hops(k.n_frames, k.hop);
  if (hops > kOnsetMaxHops) return *why = "clip tempo: more than 2^20 hops", WBX_ERR_UNSUPPORTED;
  track->first_frame = 0;
  track->n_frames = hops ? hops : 1u;
  const wbx_status ft = f0_check(*track, why);
  track->n_frames = hops;
  return ft;
}

// The pick: frames[h].onset from frames[h].novelty (a float's value), the number of onsets returned.  o >= 0, no NaN
inline uint64_t onset_pick(wbx_onset_frame* frames, uint64_t hops, double threshold, double delta, uint32_t w, uint32_t a) {
  uint64_t count = 0;
  for (uint64_t h = 0; h < hops; h++) {
    const double o = frames[h].novelty;
    bool on = o >= threshold;
    const uint64_t lo = h >= w ? h - w : 0u, hi = h + w < hops ? h + w : hops - 1u;
    for (uint64_t g = lo; g < h && on; g++) on = !(frames[g].novelty >= o);
    for (uint64_t g = h + 1u; g <= hi && on; g++) on = !(frames[g].novelty > o);
    if (on) {
      const uint64_t m0 = h >= a ? h - a : 0u, m1 = h + a < hops ? h + a : hops - 1u;
      double m = 0.0;
      for (uint64_t g = m0; g <= m1; g++) m = m + frames[g].novelty;
      on = o >= m / (double)(m1 - m0 + 1u) + delta;
    }
    frames[h].onset = on ? 1u : 0u;
    frames[h]._pad = 0;
    count += on ? 1u : 0u;
  }
  return count;
}

// onset_energy_kernel's launch: q = H / 64 frames per lane; q of 1, 2 or 4 is read directly (row = 0), any other q through
// a wave's LDS chunk of min(q, 32) columns per lane whose rows lie `row` words apart — odd, so that the walks of the 32
// lanes a 4-byte LDS read serves meet 32 different banks.  A wave per hop up to kOnsetGridMax workgroups; the grid strides over the rest
struct OnsetShape {
  uint32_t q, row, grid, lds_bytes;
};
inline OnsetShape onset_shape(uint32_t H, uint64_t hops) {
  OnsetShape s{H / 64u, 0u, 0u, 0u};
  if (s.q != 1u && s.q != 2u && s.q != 4u) s.row = (s.q < kOnsetChunk ? s.q : kOnsetChunk) | 1u;
  const uint64_t groups = (hops + kOnsetWaves - 1u) / kOnsetWaves;
  s.grid = (uint32_t)(groups < kOnsetGridMax ? groups : kOnsetGridMax);
  s.lds_bytes = kOnsetWaves * 64u * s.row * 4u;
  return s;
}
static_assert(kOnsetWaves * 64u * (kOnsetChunk | 1u) * 4u <= 65536u, "a workgroup's chunks fit the LDS a launch may ask for");

}  // namespace wbx
