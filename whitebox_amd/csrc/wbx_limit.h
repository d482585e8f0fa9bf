// wbx_limit.h — the host half of wbx_clip_limit (wbx.h "Limiting a clip"): the kernels' shape constants, the limits of a
// call and their check, the ramp table, and how a call is cut into bands.  Plain C++ (no HIP, no wbx_ctx, no libm):
// tests/cpp/limit_main.cpp compiles it with g++ alone, and tests/limit_model.py restates the table in numpy — it must
// come out BIT FOR BIT the same there, so the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cfloat>    // FLT_MIN
#include <cmath>     // std::isfinite, std::fabs
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint32_t kLimitTile = 2048;          // frames a workgroup owns: 256 lanes x 8 frames (curve and apply)
constexpr uint32_t kLimitSegment = 2048;       // terms of the ramp walked per staging of the need span: P
constexpr uint32_t kLimitBand = 1u << 20;      // output frames per band: the fp64 stage holds kLimitBand + A curve frames
constexpr uint32_t kLimitMaxLookahead = 4096, kLimitMaxHold = 65536, kLimitMaxRelease = 1u << 20;
constexpr uint64_t kLimitMaxWork = 1ull << 44;                 // n_frames * (A + H + R), terms
constexpr uint64_t kLimitMaxFrames = (1ull << 31) - 16;        // n_frames stays below it, like every pool clip's length
constexpr double kLimitMaxDrive = 4294967296.0;                // 2^32
constexpr double kLimitRampPad = 2.0;                          // a term that can never lower a curve that starts at 1.0

struct LimitCall {
  uint64_t first_frame, n_frames;   // range of the source
  float ceiling;                    // linear
  double drive;                     // linear
  uint32_t lookahead, hold, release;   // A, H, R in frames
};

// terms of the ramp: k = -A .. H + R - 1
inline uint64_t limit_terms(uint32_t A, uint32_t H, uint32_t R) { return (uint64_t)A + H + R; }

inline bool limit_shape_ok(uint32_t A, uint32_t H, uint32_t R) {
  return A <= kLimitMaxLookahead && H <= kLimitMaxHold && R >= 1u && R <= kLimitMaxRelease;
}

// the arithmetic of a call, judged without a clip: what wbx_clip_limit refuses before it looks at the source
inline wbx_status limit_check_args(const LimitCall& k, const char** why) {
  if (k.n_frames == 0) return *why = "clip limit: no frames", WBX_ERR_INVALID;
  if (!std::isfinite(k.ceiling) || !(k.ceiling >= FLT_MIN)) return *why = "clip limit: the ceiling is not a finite value of at least FLT_MIN", WBX_ERR_INVALID;
  if (!std::isfinite(k.drive) || !(std::fabs(k.drive) > 0.0) || !(std::fabs(k.drive) <= kLimitMaxDrive))
    return *why = "clip limit: the drive is not finite, is 0 or exceeds 2^32", WBX_ERR_INVALID;
  if (k.lookahead > kLimitMaxLookahead) return *why = "clip limit: lookahead_frames above 4096", WBX_ERR_INVALID;
  if (k.hold > kLimitMaxHold) return *why = "clip limit: hold_frames above 65536", WBX_ERR_INVALID;
  if (k.release < 1u || k.release > kLimitMaxRelease) return *why = "clip limit: release_frames outside 1 .. 2^20", WBX_ERR_INVALID;
  if (k.n_frames >= kLimitMaxFrames) return *why = "clip limit: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (k.n_frames * limit_terms(k.lookahead, k.hold, k.release) > kLimitMaxWork)   // (< 2^31 * 2^21: the product fits)
    return *why = "clip limit: more than 2^44 terms (n_frames * (lookahead + hold + release))", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// table[k + A] = ramp[k], k = -A .. H + R - 1: 0.0 up to k = H, then (k - H) * (1 / R) — one multiplication each
inline wbx_status limit_ramp(uint32_t A, uint32_t H, uint32_t R, double* out, size_t cap_doubles) {
  if (!out || !limit_shape_ok(A, H, R)) return WBX_ERR_INVALID;
  const uint64_t terms = limit_terms(A, H, R);
  if (cap_doubles < terms) return WBX_ERR_INVALID;
  const double s = 1.0 / (double)R;
  const uint64_t flat = (uint64_t)A + H;                       // table[0 .. flat] is 0.0 (k <= H)
  for (uint64_t t = 0; t < terms; t++) out[t] = t <= flat ? 0.0 : (double)(t - flat) * s;
  return WBX_OK;
}

// A call is issued band by band: output frames [first, first + frames), whose gain reads curve frames first - A ..
// first + frames - 1 — frames + A of them, recomputed per band into the stage, which therefore never grows with the clip
struct LimitBand {
  uint64_t first;              // the band's first output frame
  uint32_t frames;             // its output frames (<= kLimitBand)
  uint32_t curve_frames;       // frames + A
  uint32_t curve_tiles;        // workgroups of the curve kernel
  uint32_t apply_tiles;        // workgroups of the apply kernel
};
inline uint64_t limit_bands(uint64_t n_frames) { return (n_frames + kLimitBand - 1u) / kLimitBand; }
inline LimitBand limit_band(uint64_t n_frames, uint32_t A, uint64_t i) {
  LimitBand b{};
  b.first = i * kLimitBand;
  if (b.first >= n_frames) return b;
  const uint64_t left = n_frames - b.first;
  b.frames = (uint32_t)(left < kLimitBand ? left : kLimitBand);
  b.curve_frames = b.frames + A;
  b.curve_tiles = (b.curve_frames + kLimitTile - 1u) / kLimitTile;
  b.apply_tiles = (b.frames + kLimitTile - 1u) / kLimitTile;
  return b;
}
// doubles the stage needs for any call with this look-ahead (whole tiles: a tile's last lanes store no further)
inline size_t limit_stage_doubles(uint32_t A) { return (size_t)kLimitBand + A; }

}  // namespace wbx
