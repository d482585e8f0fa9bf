// wbx_dynamics.h — the host half of wbx_clip_dynamics (wbx.h "Dynamics of a clip"): the transfer table's grid, its design
// (wbx_dynamics_table: a log2 and an exp2 in plain fp64 operations), its check and its lookup, and the limits of a call and
// their check.  The ramp, the bands and the stage are wbx_limit.h's, used as they are.  Plain C++ (no HIP, no wbx_ctx, no
// libm beyond std::floor): tests/cpp/dynamics_main.cpp compiles it with g++ alone, and tests/dynamics_model.py restates the
// table and the lookup in numpy — they must come out BIT FOR BIT the same there, so the file must be compiled without
// contraction (-ffp-contract=off).
#pragma once
#include <cmath>     // std::isfinite, std::fabs, std::floor (correctly rounded, the same everywhere)
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/wbx.h"
#include "wbx_limit.h"

namespace wbx {

constexpr int kDynMinExp = -40, kDynMaxExp = 8;                // the table covers the levels 2^-40 .. 2^8
constexpr uint32_t kDynCells = 64;                             // cells per octave, linear in the mantissa
constexpr uint32_t kDynTable = (uint32_t)(kDynMaxExp - kDynMinExp) * kDynCells + 1u;
static_assert(kDynTable == WBX_DYN_TABLE, "wbx.h names the table's length");
constexpr double kDynMaxGain = 4294967296.0;                   // 2^32: drive and key_gain
constexpr double kDynDbPerOctave = 6.020599913279624;          // 20 log10(2), rounded once
constexpr double kDynTwoOverLn2 = 2.8853900817779268;          // 2 / ln 2
constexpr double kDynLn2 = 0.6931471805599453;
constexpr double kDynSqrt2 = 1.4142135623730951;
constexpr int kDynLogTerms = 12, kDynExpTerms = 16;
constexpr double kDynMaxDb = 1000.0;                           // |threshold_db| and knee_db of a design stay under it

inline uint64_t dyn_bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}
inline double dyn_from_bits(uint64_t u) {
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

// log2(m), m in [1, 2): halved where it exceeds sqrt(2) (exact), then 2 atanh(s) / ln 2 with s = (m - 1) / (m + 1),
// |s| < 0.172, as a series of kDynLogTerms odd powers in Horner form.  log2(1) is exactly 0.0
inline double dyn_log2_mantissa(double m) {
  double whole = 0.0;
  if (m > kDynSqrt2) m = m / 2.0, whole = 1.0;
  const double s = (m - 1.0) / (m + 1.0);
  const double s2 = s * s;
  double p = 1.0 / (double)(2 * kDynLogTerms + 1);
  for (int n = kDynLogTerms - 1; n >= 0; n--) p = p * s2 + 1.0 / (double)(2 * n + 1);
  return whole + (s * p) * kDynTwoOverLn2;
}

// 2^y for y <= 0: 0.0 below y = -1021; else i = floor(y + 0.5), f = y - i (exact, |f| <= 0.5 and a little), e^(f ln 2) as
// kDynExpTerms terms of the exponential series in Horner form, times 2^i built from its bits (an exact scaling: the
// product is a normal number).  exp2(+-0.0) is exactly 1.0, and no y <= 0 gives more than 1.0: with i = 0 the last step
// adds a product that is not positive to 1.0, with i < 0 the result is below 0.5 * 1.42
inline double dyn_exp2(double y) {
  if (y < -1021.0) return 0.0;
  const double i = std::floor(y + 0.5);
  const double t = (y - i) * kDynLn2;
  double p = 1.0;
  for (int n = kDynExpTerms; n >= 1; n--) p = 1.0 + (p * t) / (double)n;
  return p * dyn_from_bits((uint64_t)((int64_t)i + 1023) << 52);
}

// the level of entry (e - kDynMinExp) * 64 + k is 2^e * (1 + k / 64): its level in octaves, e + log2(1 + k / 64)
inline double dyn_entry_octaves(uint32_t entry) {
  const double e = (double)((int)(entry / kDynCells) + kDynMinExp);
  return e + dyn_log2_mantissa(1.0 + (double)(entry % kDynCells) / (double)kDynCells);
}

// wbx_dynamics_table: the static curve at the kDynTable grid levels, all in octaves (a dB figure / kDynDbPerOctave)
inline wbx_status dynamics_table(int kind, double threshold_db, double ratio, double knee_db, double range_db, double* out,
                                 size_t cap_doubles) {
  if (!out || cap_doubles < kDynTable) return WBX_ERR_INVALID;
  if (kind != WBX_DYN_COMPRESS && kind != WBX_DYN_GATE) return WBX_ERR_INVALID;
  if (!std::isfinite(threshold_db) || std::fabs(threshold_db) > kDynMaxDb) return WBX_ERR_INVALID;
  if (!(ratio >= 1.0) || (kind == WBX_DYN_GATE && !std::isfinite(ratio))) return WBX_ERR_INVALID;
  if (!(knee_db >= 0.0) || !(knee_db <= kDynMaxDb)) return WBX_ERR_INVALID;
  if (!(range_db <= 0.0)) return WBX_ERR_INVALID;
  const double T = threshold_db / kDynDbPerOctave, W = knee_db / kDynDbPerOctave, floor_oct = range_db / kDynDbPerOctave;
  const double half = W / 2.0;
  const double slope = kind == WBX_DYN_COMPRESS ? 1.0 / ratio - 1.0 : ratio - 1.0;   // octaves of gain per octave of level
  for (uint32_t t = 0; t < kDynTable; t++) {
    const double over = dyn_entry_octaves(t) - T;
    const double two = 2.0 * over;
    double y;
    if (kind == WBX_DYN_COMPRESS) {
      if (two <= 0.0 - W) {
        out[t] = 1.0;                                          // under the knee: exactly 1.0, by this branch
        continue;
      }
      if (two < W) {
        const double u = over + half;
        y = slope * ((u * u) / (2.0 * W));
      } else {
        y = slope * over;
      }
    } else {
      if (two >= W) {
        out[t] = 1.0;                                          // above the knee
        continue;
      }
      if (two > 0.0 - W) {
        const double u = over - half;
        y = 0.0 - slope * ((u * u) / (2.0 * W));
      } else {
        y = slope * over;
      }
    }
    if (y < floor_oct) y = floor_oct;
    out[t] = dyn_exp2(y);
  }
  return WBX_OK;
}

// wbx_dynamics_check: every entry finite, its sign bit clear, at most 1.0.  *lo (may be NULL): the smallest entry
inline wbx_status dynamics_table_check(const double* table, int sense, double* lo) {
  if (!table || (sense != WBX_DYN_COMPRESS && sense != WBX_DYN_GATE)) return WBX_ERR_INVALID;
  double least = 1.0;
  for (uint32_t t = 0; t < kDynTable; t++) {
    const double v = table[t];
    if ((dyn_bits(v) >> 63) != 0u || !(v <= 1.0)) return WBX_ERR_INVALID;   // (a NaN fails the comparison)
    if (v < least) least = v;
  }
  if (lo) *lo = least;
  return WBX_OK;
}

// wbx_dynamics_lookup: want = tab(p) for a level p >= 0 (not a NaN), from the bits of p
inline double dynamics_lookup(const double* table, double p) {
  if (p < 0x1p-40) return table[0];
  if (p >= 256.0) return table[kDynTable - 1u];
  const uint64_t u = dyn_bits(p), m = u & ((1ull << 52) - 1u);
  const uint32_t idx = ((uint32_t)(u >> 52) - (uint32_t)(1023 + kDynMinExp)) * kDynCells + (uint32_t)(m >> 46);
  const double f = (double)(int64_t)(m & ((1ull << 46) - 1u)) * 0x1p-46;
  return table[idx] + f * (table[idx + 1u] - table[idx]);
}

struct DynCall {
  uint64_t first_frame, n_frames;   // range of the source
  uint64_t key_first;               // the key's first frame (keyed calls)
  bool keyed;
  int sense;
  const double* table;              // [kDynTable]
  double drive, key_gain, makeup;   // linear
  uint32_t lookahead, hold, release;   // A, H, R in frames
};

inline bool dyn_gain_ok(double g) { return std::isfinite(g) && std::fabs(g) > 0.0 && std::fabs(g) <= kDynMaxGain; }

// the arithmetic of a call, judged without a clip: what wbx_clip_dynamics refuses before it looks at the source or the key.
// *lo: the table's smallest entry
inline wbx_status dynamics_check_args(const DynCall& k, double* lo, const char** why) {
  if (k.n_frames == 0) return *why = "clip dynamics: no frames", WBX_ERR_INVALID;
  if (k.sense != WBX_DYN_COMPRESS && k.sense != WBX_DYN_GATE) return *why = "clip dynamics: unknown sense", WBX_ERR_INVALID;
  if (!k.table) return *why = "clip dynamics: the table is NULL", WBX_ERR_INVALID;
  if (dynamics_table_check(k.table, k.sense, lo) != WBX_OK)
    return *why = "clip dynamics: a table entry is not finite, carries a sign or exceeds 1.0", WBX_ERR_INVALID;
  if (!dyn_gain_ok(k.drive)) return *why = "clip dynamics: the drive is not finite, is 0 or exceeds 2^32", WBX_ERR_INVALID;
  if (k.keyed && !dyn_gain_ok(k.key_gain)) return *why = "clip dynamics: the key_gain is not finite, is 0 or exceeds 2^32", WBX_ERR_INVALID;
  if (!std::isfinite(k.makeup) || !(k.makeup >= 0.0)) return *why = "clip dynamics: the makeup is not finite or is negative", WBX_ERR_INVALID;
  if (k.lookahead > kLimitMaxLookahead) return *why = "clip dynamics: lookahead_frames above 4096", WBX_ERR_INVALID;
  if (k.hold > kLimitMaxHold) return *why = "clip dynamics: hold_frames above 65536", WBX_ERR_INVALID;
  if (k.release < 1u || k.release > kLimitMaxRelease) return *why = "clip dynamics: release_frames outside 1 .. 2^20", WBX_ERR_INVALID;
  if (k.n_frames >= kLimitMaxFrames) return *why = "clip dynamics: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (k.n_frames * limit_terms(k.lookahead, k.hold, k.release) > kLimitMaxWork)   // (< 2^31 * 2^21: the product fits)
    return *why = "clip dynamics: more than 2^44 terms (n_frames * (lookahead + hold + release))", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

}  // namespace wbx
