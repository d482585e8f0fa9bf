// wbx_saturate.h — the host half of wbx_clip_saturate (wbx.h "Saturating a clip"): the shape table's grid, its design
// (wbx_saturate_table: hard, cubic and tanh curves in plain fp64 operations), its check and its lookup, the limits of a
// call and their check in the stated order, and how saturate_kernel is launched (the tile, what it stages, its LDS).  The
// oversampling filters are wbx_resample.h's plans (1, os) and (os, 1), used as they are; the tanh is built from
// wbx_dynamics.h's exp2.  Plain C++ (no HIP, no wbx_ctx, no libm beyond std::floor): tests/cpp/saturate_main.cpp compiles it
// with g++ alone, and tests/saturate_model.py restates the table and the lookup in numpy — they must come out BIT FOR BIT
// the same there, so the file must be compiled without contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::isfinite, std::fabs, std::floor (correctly rounded, the same everywhere)
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"
#include "wbx_dynamics.h"
#include "wbx_resample.h"

namespace wbx {

constexpr uint32_t kSatTable = 16385;                          // entries: the levels -8 .. +8, 1024 cells per unit
static_assert(kSatTable == WBX_SAT_TABLE, "wbx.h names the table's length");
constexpr double kSatCells = 1024.0, kSatEdge = 8192.0;        // a = d * 1024; beyond |a| >= 8192 the end entries
constexpr double kSatMaxGain = 4294967296.0;                   // 2^32: drive, makeup, an entry's magnitude
constexpr double kSatMaxBias = 4.0;
constexpr double kSatLog2e = 1.4426950408889634;
constexpr double kSatCubic = 4.0 / 27.0;
constexpr uint64_t kSatMaxMid = (1ull << 31) - 16;             // n * os stays below it
constexpr uint32_t kSatTileMax = 1024, kSatTileStep = 256, kSatLdsMax = 65536;

inline bool sat_os_ok(uint32_t os) { return os == 1u || os == 2u || os == 4u || os == 8u; }

// ---- the table ----------------------------------------------------------------------------------------------------------------
// f(z) of the three designs
inline double sat_curve(int kind, double z) {
  if (kind == WBX_SAT_HARD) return z < -1.0 ? -1.0 : z > 1.0 ? 1.0 : z;
  if (kind == WBX_SAT_CUBIC) {
    if (z >= 1.5) return 1.0;
    if (z <= -1.5) return -1.0;
    return z - (kSatCubic * z) * (z * z);
  }
  const double a = std::fabs(z);                               // WBX_SAT_TANH: (1 - e) / (1 + e), e = exp(-2 |z|)
  const double e = dyn_exp2((-2.0 * a) * kSatLog2e);
  const double t = (1.0 - e) / (1.0 + e);
  return z < 0.0 ? 0.0 - t : t;
}

// wbx_saturate_table: entry k = f(v + bias) - f(bias), v = (k - 8192) / 1024.  With bias == 0 f(bias) is +0.0 and every f
// is odd by construction (a clamp, products of z, the sign put back last), so the table is bitwise odd
inline wbx_status saturate_table(int kind, double bias, double* out, size_t cap_doubles) {
  if (!out || cap_doubles < kSatTable) return WBX_ERR_INVALID;
  if (kind != WBX_SAT_HARD && kind != WBX_SAT_CUBIC && kind != WBX_SAT_TANH) return WBX_ERR_INVALID;
  if (!(std::fabs(bias) <= kSatMaxBias)) return WBX_ERR_INVALID;   // (a NaN fails the comparison)
  const double f0 = sat_curve(kind, bias);
  for (uint32_t k = 0; k < kSatTable; k++) {
    const double v = ((double)k - kSatEdge) / kSatCells;
    out[k] = sat_curve(kind, v + bias) - f0;
  }
  return WBX_OK;
}

// wbx_saturate_check: every entry finite with a magnitude of at most 2^32
inline wbx_status saturate_table_check(const double* table) {
  if (!table) return WBX_ERR_INVALID;
  for (uint32_t k = 0; k < kSatTable; k++)
    if (!(std::fabs(table[k]) <= kSatMaxGain)) return WBX_ERR_INVALID;   // (a NaN fails the comparison)
  return WBX_OK;
}

// wbx_saturate_lookup: w = tab(d) for a driven sample d (not a NaN)
inline double saturate_lookup(const double* table, double d) {
  const double a = d * kSatCells;
  if (a <= 0.0 - kSatEdge) return table[0];
  if (a >= kSatEdge) return table[kSatTable - 1u];
  const double fl = std::floor(a);
  const uint32_t idx = (uint32_t)((int)fl + 8192);             // 0 .. 16383
  const double f = a - fl;                                     // (may round to 1.0 for a tiny negative a)
  return table[idx] + f * (table[idx + 1u] - table[idx]);
}

// ---- a call ---------------------------------------------------------------------------------------------------------------------
struct SatCall {
  uint64_t first_frame, n_frames;   // range of the source
  uint32_t os;                      // 1, 2, 4 or 8
  int quality;                      // WBX_SRC_*
  const double* table;              // [kSatTable]
  double drive, makeup;             // linear
};

// the two conversions of a call with os > 1: up = (1 -> os), down = (os -> 1), what wbx_resample_plan refuses refused with
// its status and reason
inline wbx_status saturate_plans(uint32_t os, int quality, ResamplePlan* up, ResamplePlan* down, const char** why) {
  wbx_status st = resample_plan(1u, os, quality, up, why);
  if (st == WBX_OK) st = resample_plan(os, 1u, quality, down, why);
  return st;
}

// the arithmetic of a call, judged without a clip, in this order: n_frames, os, quality, the table, drive, makeup, the
// length (all INVALID), then the two plans (BEST at os 8: UNSUPPORTED)
inline wbx_status saturate_check_args(const SatCall& k, const char** why) {
  if (k.n_frames == 0) return *why = "clip saturate: no frames", WBX_ERR_INVALID;
  if (!sat_os_ok(k.os)) return *why = "clip saturate: os is not 1, 2, 4 or 8", WBX_ERR_INVALID;
  ResampleQuality q;
  if (!resample_quality(k.quality, &q)) return *why = "clip saturate: unknown quality", WBX_ERR_INVALID;
  if (!k.table) return *why = "clip saturate: the table is NULL", WBX_ERR_INVALID;
  if (saturate_table_check(k.table) != WBX_OK) return *why = "clip saturate: a table entry is not finite or exceeds 2^32", WBX_ERR_INVALID;
  if (!dyn_gain_ok(k.drive)) return *why = "clip saturate: the drive is not finite, is 0 or exceeds 2^32", WBX_ERR_INVALID;
  if (!(std::fabs(k.makeup) <= kSatMaxGain)) return *why = "clip saturate: the makeup is not finite or exceeds 2^32", WBX_ERR_INVALID;
  if (k.n_frames >= kSatMaxMid / k.os + (kSatMaxMid % k.os ? 1u : 0u))   // n * os >= 2^31 - 16, without the product
    return *why = "clip saturate: n_frames * os reaches 2^31 - 16", WBX_ERR_INVALID;
  if (k.os > 1u) {
    ResamplePlan up, down;
    return saturate_plans(k.os, k.quality, &up, &down, why);
  }
  return WBX_OK;
}

// saturate_kernel's launch.  A workgroup of 256 lanes owns a tile of output frames, a multiple of 256 and at most 1024: the
// greatest whose LDS — per channel the tile + 4 Z source frames (one word never used) and os planes of tile + 2 Z mid
// samples, 4 bytes each — stays within 64 KB.  os == 1 stages nothing: 1024 frames per workgroup, 4 per lane
struct SatShape {
  uint32_t tile, mid_span, src_span, lds_bytes, n_tiles;
  uint32_t Z, plane, row;          // zero crossings; words of one plane / of one staged source row
};
inline uint32_t sat_lds_bytes(uint32_t os, uint32_t Z, uint32_t channels, uint32_t tile) {
  return channels * 4u * ((tile + 2u * Z) * os + tile + 4u * Z);
}
// (os, quality and channels are ones saturate_check_args and the clip's check accept; n >= 1, n * os < 2^31 - 16)
inline SatShape saturate_shape(uint32_t os, int quality, uint32_t channels, uint64_t n) {
  SatShape s{};
  s.tile = kSatTileMax;
  if (os > 1u) {
    ResampleQuality q{};
    (void)resample_quality(quality, &q);
    s.Z = q.zero_crossings;
    while (s.tile > kSatTileStep && sat_lds_bytes(os, s.Z, channels, s.tile) > kSatLdsMax) s.tile -= kSatTileStep;
    s.plane = s.tile + 2u * s.Z;
    s.row = s.tile + 4u * s.Z;
    s.mid_span = s.plane * os;
    s.src_span = s.row - 1u;
    s.lds_bytes = sat_lds_bytes(os, s.Z, channels, s.tile);
  } else {
    s.mid_span = s.src_span = s.tile;
  }
  s.n_tiles = (uint32_t)((n + s.tile - 1u) / s.tile);
  return s;
}

}  // namespace wbx
