// wbx_pitch.h — the host half of wbx_clip_pitch (wbx.h "Pitch-shifting a clip"): the ratio's reduction, the length of the
// stretched intermediate, the step cap and the argument check.  A pitch shift is a stretch to mid_frames frames fed straight
// into a conversion by M / L, so everything here stands on wbx_stretch.h and wbx_resample.h.  Plain C++ (no HIP, no wbx_ctx,
// no libm): tests/cpp/pitch_main.cpp compiles it with g++ alone, and tests/pitch_model.py restates it in Python integers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_resample.h"
#include "wbx_stretch.h"

namespace wbx {

constexpr uint32_t kPitchMaxOctaves = 4;                        // num <= 4 den and den <= 4 num: two octaves either way
constexpr uint32_t kPitchMaxSteps = 1u << 22;                   // K' of a call: the positions buffer holds K' + 1 words (16 MB + 4 B)
constexpr uint64_t kPitchMaxFrames = kStretchMaxFrames;         // m stays below it, like every pool clip's length

struct PitchCall {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint64_t out_frames;              // m
  uint32_t num, den;                // the pitch ratio, above 1 meaning up
  int quality;                      // WBX_SRC_*
  uint32_t window, tolerance;       // N, D
  bool wants_positions;             // positions_out is not NULL ...
  size_t positions_cap;             // ... and holds this many
};

// L = den / g, M = num / g; false for a ratio the call refuses: num or den of 0, a ratio of 1, beyond two octaves, L > 1280
inline bool pitch_ratio_ok(uint32_t num, uint32_t den, uint32_t* L, uint32_t* M) {
  if (num == 0 || den == 0) return false;
  const uint32_t g = resample_gcd(num, den);
  *L = den / g;
  *M = num / g;
  if (*L == *M) return false;
  if ((uint64_t)num > (uint64_t)kPitchMaxOctaves * den || (uint64_t)den > (uint64_t)kPitchMaxOctaves * num) return false;
  return *L <= kResampleMaxL;
}

// m' = ceil(m M / L), the product in 128 bits (any out_frames may be asked about; what does not fit 64 bits is 2^64 - 1);
// 0 where the call would refuse the ratio
inline uint64_t pitch_mid_frames(uint64_t m, uint32_t num, uint32_t den) {
  uint32_t L = 0, M = 0;
  if (!pitch_ratio_ok(num, den, &L, &M)) return 0;
  const unsigned __int128 mid = ((unsigned __int128)m * M + (L - 1u)) / L;
  return mid > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)mid;
}

// The arithmetic of a call, judged without a clip, in this order: what is WBX_ERR_INVALID about the call's own arguments; the
// ratio (WBX_ERR_UNSUPPORTED); then everything stretch_check_args says about (n, m', N, D); then the step cap.  Fills the
// conversion's plan and the stretch the call performs (its out_frames is m')
inline wbx_status pitch_check_args(const PitchCall& k, ResamplePlan* plan, StretchCall* stretch, const char** why) {
  if (k.n_frames == 0 || k.out_frames == 0) return *why = "clip pitch: no frames", WBX_ERR_INVALID;
  if (k.num == 0 || k.den == 0) return *why = "clip pitch: a ratio with a term of 0", WBX_ERR_INVALID;
  const uint32_t g = resample_gcd(k.num, k.den);
  if (k.num / g == k.den / g) return *why = "clip pitch: a ratio of 1 (wbx_clip_stretch changes the length alone; the filter is not an identity)", WBX_ERR_INVALID;
  ResampleQuality q;
  if (!resample_quality(k.quality, &q)) return *why = "clip pitch: unknown quality", WBX_ERR_INVALID;
  if (k.out_frames >= kPitchMaxFrames) return *why = "clip pitch: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if ((uint64_t)k.num > (uint64_t)kPitchMaxOctaves * k.den || (uint64_t)k.den > (uint64_t)kPitchMaxOctaves * k.num)
    return *why = "clip pitch: a ratio beyond two octaves either way", WBX_ERR_UNSUPPORTED;
  const char* msg = "";
  wbx_status st = resample_plan(k.num, k.den, k.quality, plan, &msg);   // (source rate num, destination rate den: L = den / g, M = num / g)
  if (st != WBX_OK) return *why = "clip pitch: the ratio needs more than 1280 phases or 512 taps", WBX_ERR_UNSUPPORTED;
  const uint64_t mid = pitch_mid_frames(k.out_frames, k.num, k.den);
  *stretch = StretchCall{k.first_frame, k.n_frames, mid, k.window, k.tolerance, k.wants_positions, k.positions_cap};
  st = stretch_check_args(*stretch, &msg);
  if (st != WBX_OK) return *why = msg, st;
  if (stretch_steps(mid, k.window) > kPitchMaxSteps) return *why = "clip pitch: more than 2^22 steps", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// pitch_kernel's tile and its span of the intermediate are the conversion's: one formula, resample_launch_shape
// (wbx_resample.h), which launch_pitch calls for the grid as well.  The tile depends on (L, M, T) alone
inline uint32_t pitch_tile(uint32_t L, uint32_t M, uint32_t T) { return resample_launch_shape(L, M, T, 1u).tile; }
inline uint32_t pitch_span(uint32_t L, uint32_t M, uint32_t T, uint32_t tile) { return resample_span(L, M, T, tile); }

}  // namespace wbx
