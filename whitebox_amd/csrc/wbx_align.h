// wbx_align.h — the host half of wbx_clip_align (wbx.h "Aligning two clips"): the limits of a call and their check, the
// number of chunks, how a call is cut into bands of chunks bounded by the device stage and by their terms, and how
// align_partial_kernel's workgroup is shaped.  Plain C++ (no HIP, no wbx_ctx, no libm): tests/cpp/align_main.cpp compiles
// it with g++ alone, and tests/align_model.py restates it in Python integers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint64_t kAlignMinN = 64, kAlignMaxN = 1ull << 24;    // n, a multiple of 8: the template
constexpr uint64_t kAlignMaxM = (1ull << 31) - 16;              // m stays below it, like every pool clip's length
constexpr int64_t kAlignMaxLag = 1ll << 24;                     // lag_min, lag_max in [-2^24, 2^24]
constexpr uint64_t kAlignMaxLags = 1ull << 17;                  // the curve: at most 2 MB
constexpr uint32_t kAlignChunk = 2048;                          // C: terms per chunk, part of the arithmetic
// the device stage: records {pr, pE} per (chunk of the band, lag), 64 MB at most
constexpr uint64_t kAlignStageRecords = 1ull << 22;
constexpr uint64_t kAlignLaunchTerms = 1ull << 39;              // terms of one band's partial launch: f0's bound (wbx_f0.h)
// align_partial_kernel's workgroup: up to 512 lanes, 8 consecutive lags per lane, so a wave owns 512 lags and a workgroup
// a block of 4096; what it stages (floats)
constexpr uint32_t kAlignLanes = 512, kAlignPerLane = 8, kAlignWaveLags = 512, kAlignBlockLags = 4096;
constexpr uint32_t kAlignSpanSlack = 16;                        // what a lane's last turn's look ahead reads
constexpr uint32_t kAlignTmplWords = kAlignChunk + 16;          // the template, and the 4 words the last turn asks for
constexpr uint32_t kAlignKnownFlags = WBX_ALIGN_EITHER_POLARITY;

struct AlignCall {
  uint64_t a_first, n;              // range of the reference clip: the template
  uint64_t b_first, m;              // range of the clip to be aligned
  int64_t lag_min, lag_max;
  uint32_t flags;
  bool has_info, has_curve;         // info / curve_out is not NULL ...
  size_t curve_cap;                 // ... and curve_out holds this many records
};

inline bool align_n_ok(uint64_t n) { return n >= kAlignMinN && n <= kAlignMaxN && n % 8u == 0u; }

// chunks = ceil(n / C); 0 for an n the call refuses
inline uint32_t align_chunks(uint64_t n) { return align_n_ok(n) ? (uint32_t)((n + kAlignChunk - 1u) / kAlignChunk) : 0u; }

// the arithmetic of a call, judged without a clip: what wbx_clip_align refuses before it looks at the clips
inline wbx_status align_check(const AlignCall& k, const char** why) {
  if (!align_n_ok(k.n)) return *why = "clip align: n_frames is not a multiple of 8 in 64 .. 2^24", WBX_ERR_INVALID;
  if (k.m < 1u || k.m >= kAlignMaxM) return *why = "clip align: m_frames outside 1 .. 2^31 - 17", WBX_ERR_INVALID;
  if (k.lag_min < -kAlignMaxLag || k.lag_min > kAlignMaxLag) return *why = "clip align: lag_min outside -2^24 .. 2^24", WBX_ERR_INVALID;
  if (k.lag_max < -kAlignMaxLag || k.lag_max > kAlignMaxLag) return *why = "clip align: lag_max outside -2^24 .. 2^24", WBX_ERR_INVALID;
  if (k.lag_min > k.lag_max) return *why = "clip align: lag_min is above lag_max", WBX_ERR_INVALID;
  if (k.flags & ~kAlignKnownFlags) return *why = "clip align: unknown flag bits", WBX_ERR_INVALID;
  if (!k.has_info && !k.has_curve) return *why = "clip align: info and curve_out are both NULL", WBX_ERR_INVALID;
  const uint64_t lags = (uint64_t)(k.lag_max - k.lag_min) + 1u;
  if (k.has_curve && k.curve_cap < lags) return *why = "clip align: curve_cap is below the number of lags", WBX_ERR_INVALID;
  if (lags > kAlignMaxLags) return *why = "clip align: more than 2^17 lags", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// chunks one band takes: as many as the stage holds records for, and as stay within kAlignLaunchTerms, at least 1; 0 for a
// number of lags the call refuses.  (With C = 2048 the stage is the tighter bound for every lags; both are stated.)
inline uint32_t align_band_chunks(uint64_t lags) {
  if (lags < 1u || lags > kAlignMaxLags) return 0;
  const uint64_t by_stage = kAlignStageRecords / lags, by_terms = kAlignLaunchTerms / (lags * kAlignChunk);
  const uint64_t c = by_stage < by_terms ? by_stage : by_terms;
  return (uint32_t)(c < 1u ? 1u : c);
}
inline uint32_t align_bands(uint64_t n, uint64_t lags) {
  const uint32_t chunks = align_chunks(n), per = align_band_chunks(lags);
  return chunks && per ? (chunks + per - 1u) / per : 0u;
}
// launches of a call: the reference's energy, a partial and a fold launch per band, the pick; 0 for a refused shape
inline uint32_t align_launches(uint64_t n, uint64_t lags) {
  const uint32_t bands = align_bands(n, lags);
  return bands ? 2u * bands + 2u : 0u;
}

// align_partial_kernel's shape: the waves of a workgroup — ceil(min(lags, 4096) / 512) — and the lag blocks of the grid
struct AlignShape {
  uint32_t waves, blocks;
};
inline AlignShape align_shape(uint64_t lags) {
  const uint64_t in_block = lags < kAlignBlockLags ? lags : kAlignBlockLags;
  return AlignShape{(uint32_t)((in_block + kAlignWaveLags - 1u) / kAlignWaveLags), (uint32_t)((lags + kAlignBlockLags - 1u) / kAlignBlockLags)};
}
// words of B a workgroup of `waves` waves stages for a chunk of `terms` terms: lag j of lane l at term i reads word
// 8 l + j + i, and the last turn asks for words up to terms + 11 past a lane's first
constexpr uint32_t align_span_words(uint32_t terms, uint32_t waves) { return terms + kAlignWaveLags * waves + kAlignSpanSlack; }
// dynamic LDS of a workgroup: the template, then the span — 8256 + 4 (2048 + 4096 + 16) = 32896 bytes at most
inline uint32_t align_lds_bytes(uint32_t waves) { return 4u * (kAlignTmplWords + align_span_words(kAlignChunk, waves)); }
static_assert(kAlignTmplWords % 4u == 0u, "the span starts on 16 bytes");
static_assert(kAlignLanes * kAlignPerLane == kAlignBlockLags && kAlignWaveLags == 64u * kAlignPerLane);
static_assert(kAlignStageRecords / kAlignMaxLags >= 1u, "a band holds a chunk");

}  // namespace wbx
