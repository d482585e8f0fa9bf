// wbx_warp.h — the host half of wbx_clip_warp (wbx.h "Warping a clip"): the markers' check, the segments they bound, the
// steps, and how a call's searches are planned into rounds and launches.  Everything about a single chain — window, limits,
// the steps one workgroup walks per launch — is wbx_stretch.h's.  Plain C++ (no HIP, no wbx_ctx):
// tests/cpp/warp_main.cpp compiles it with g++ alone, and tests/warp_model.py restates it in numpy.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/wbx.h"
#include "wbx_stretch.h"

namespace wbx {

constexpr uint32_t kWarpMaxMarkers = 65535;                     // M
constexpr uint64_t kWarpMaxSteps = 1ull << 22;                  // K: all positions of a call stay resident (16 MB)
// workgroups one search launch takes at most.  The densest launch — every workgroup searching the whole span of every step
// of its round, kStretchLaunchTerms each — must stay within twice the longest search launch of a stretch (38 - 41 ms).  The
// device saturates at 5.2 - 6.8e12 scored terms/s, what 256 workgroups reach (one per CU; a second one on a CU adds
// nothing): 256 x 2^30 terms are 40 - 53 ms, 512 would be 81 - 106 ms (MEASUREMENTS.md "Warping a clip")
constexpr uint32_t kWarpLaunchSegments = 256;

struct WarpCall {
  uint64_t first_frame, n_frames;   // range of the source: n
  uint64_t out_frames;              // m
  const wbx_warp_marker* markers;   // M pairs, both columns strictly ascending inside (0, n) and (0, m)
  uint32_t n_markers;
  uint32_t window, tolerance;       // N, D
  bool wants_positions;             // positions_out is not NULL ...
  size_t positions_cap;             // ... and holds this many
};

// the markers alone: NULL with M > 0, M > 65535, a column not strictly ascending, a frame that is 0 or not below n / m
inline bool warp_markers_ok(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M) {
  if (M > kWarpMaxMarkers || (M > 0 && !mk)) return false;
  uint64_t s = 0, t = 0;
  for (uint32_t j = 0; j < M; j++) {
    if (mk[j].src_frame <= s || mk[j].out_frame <= t || mk[j].src_frame >= n || mk[j].out_frame >= m) return false;
    s = mk[j].src_frame, t = mk[j].out_frame;
  }
  return true;
}

// segment j of S = M + 1: from (s_j, t_j) to (s_{j+1}, t_{j+1}), with (s_0, t_0) = (0, 0) and (s_S, t_S) = (n, m)
struct WarpSpan {
  uint64_t s0, t0, n_j, m_j;
};
inline WarpSpan warp_span(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M, uint32_t j) {
  const uint64_t s0 = j ? mk[j - 1].src_frame : 0, t0 = j ? mk[j - 1].out_frame : 0;
  const uint64_t s1 = j < M ? mk[j].src_frame : n, t1 = j < M ? mk[j].out_frame : m;
  return WarpSpan{s0, t0, s1 - s0, t1 - t0};
}

// K = sum of ceil(m_j / Hs); 0 for a window the call refuses or markers the call refuses
inline uint64_t warp_steps(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M, uint32_t N) {
  if (!stretch_window_ok(N) || n == 0 || m == 0 || !warp_markers_ok(n, m, mk, M)) return 0;
  const uint64_t Hs = N / 2u;
  uint64_t K = 0;
  for (uint32_t j = 0; j <= M; j++) K += (warp_span(n, m, mk, M, j).m_j + Hs - 1u) / Hs;
  return K;
}

// The arithmetic of a call, judged without a clip.  First what wbx_clip_stretch refuses for (n, m, N, D); next the markers,
// and a positions_cap below K (K needs the markers); next a segment's ratio beyond 8 either way and K > 2^22
inline wbx_status warp_check_args(const WarpCall& k, const char** why) {
  const uint64_t n = k.n_frames, m = k.out_frames;
  if (n == 0 || m == 0) return *why = "clip warp: no frames", WBX_ERR_INVALID;
  if (n >= kStretchMaxFrames || m >= kStretchMaxFrames)
    return *why = "clip warp: the range or the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (!stretch_window_ok(k.window)) return *why = "clip warp: window_frames is not a multiple of 8 in 32 .. 8192", WBX_ERR_INVALID;
  if (k.tolerance > kStretchMaxTolerance) return *why = "clip warp: tolerance_frames above 4096", WBX_ERR_INVALID;
  if (k.n_markers > 0 && !k.markers) return *why = "clip warp: markers is NULL", WBX_ERR_INVALID;
  if (k.n_markers > kWarpMaxMarkers) return *why = "clip warp: more than 65535 markers", WBX_ERR_INVALID;
  if (!warp_markers_ok(n, m, k.markers, k.n_markers))
    return *why = "clip warp: a marker column is not strictly ascending inside (0, n_frames) / (0, out_frames)", WBX_ERR_INVALID;
  const uint64_t K = warp_steps(n, m, k.markers, k.n_markers, k.window);
  if (k.wants_positions && k.positions_cap < K) return *why = "clip warp: positions_cap is below the number of steps", WBX_ERR_INVALID;
  for (uint32_t j = 0; j <= k.n_markers; j++) {
    const WarpSpan g = warp_span(n, m, k.markers, k.n_markers, j);
    if (g.m_j > kStretchMaxRatio * g.n_j || g.n_j > kStretchMaxRatio * g.m_j)
      return *why = "clip warp: a segment's ratio beyond 8 either way", WBX_ERR_UNSUPPORTED;
  }
  if (K > kWarpMaxSteps) return *why = "clip warp: more than 2^22 steps", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}
inline wbx_status warp_check_sizes(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M, uint32_t N, uint32_t D) {
  const char* why = "";
  return warp_check_args(WarpCall{0, n, m, mk, M, N, D, false, 0}, &why);
}

// fills out[0 .. S) for a call warp_check_sizes accepts (apart from its tolerance); WBX_ERR_INVALID otherwise, or for cap < S
inline wbx_status warp_segments(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M, uint32_t N, wbx_warp_segment* out,
                                size_t cap) {
  if (!out || !stretch_window_ok(N) || n == 0 || m == 0 || !warp_markers_ok(n, m, mk, M) || cap < (size_t)M + 1u) return WBX_ERR_INVALID;
  const uint64_t Hs = N / 2u;
  uint64_t base = 0;
  for (uint32_t j = 0; j <= M; j++) {
    const WarpSpan g = warp_span(n, m, mk, M, j);
    const uint64_t Kj = (g.m_j + Hs - 1u) / Hs;
    out[j] = wbx_warp_segment{g.s0, g.t0, base, Kj};
    base += Kj;
  }
  return WBX_OK;
}

// The searches of a call.  Round r walks steps [r S_r, (r + 1) S_r) of every segment that has them — S_r =
// stretch_launch_steps(n, N, D), the bound of one workgroup's launch — one workgroup per such segment, and is issued in
// slices of at most kWarpLaunchSegments workgroups.  ids holds the segment ids of all launches back to back, ascending
// within a round; a round's list is a subset of the round's before it, so the plan costs what it holds
struct WarpLaunch {
  uint32_t round, first, count;   // ids[first .. first + count)
};
struct WarpPlan {
  std::vector<uint32_t> ids;
  std::vector<WarpLaunch> launches;   // the search launches, in issue order
  uint32_t round_steps = 0;           // S_r
  uint64_t longest = 0;               // the most steps of a segment
};
inline WarpPlan warp_plan(const wbx_warp_segment* seg, uint32_t S, uint32_t round_steps) {
  WarpPlan pl;
  pl.round_steps = round_steps;
  if (round_steps == 0) return pl;
  size_t from = 0, to = 0;
  for (uint32_t j = 0; j < S; j++) {
    if (seg[j].steps > pl.longest) pl.longest = seg[j].steps;
    if (seg[j].steps > 0) pl.ids.push_back(j);
  }
  to = pl.ids.size();
  for (uint32_t r = 0; to > from; r++) {
    for (size_t at = from; at < to; at += kWarpLaunchSegments)
      pl.launches.push_back(WarpLaunch{r, (uint32_t)at, (uint32_t)(to - at < kWarpLaunchSegments ? to - at : kWarpLaunchSegments)});
    const uint64_t done = ((uint64_t)r + 1u) * round_steps;
    for (size_t at = from; at < to; at++) {
      const uint32_t j = pl.ids[at];
      if (seg[j].steps > done) pl.ids.push_back(j);
    }
    from = to, to = pl.ids.size();
  }
  return pl;
}
// kernel launches of a whole call: its search launches and the one overlap-add; 0 for a call warp_check_sizes refuses
inline uint64_t warp_launches(uint64_t n, uint64_t m, const wbx_warp_marker* mk, uint32_t M, uint32_t N, uint32_t D) {
  if (warp_check_sizes(n, m, mk, M, N, D) != WBX_OK) return 0;
  std::vector<wbx_warp_segment> seg((size_t)M + 1u);
  (void)warp_segments(n, m, mk, M, N, seg.data(), seg.size());
  return (uint64_t)warp_plan(seg.data(), M + 1u, stretch_launch_steps(n, N, D)).launches.size() + 1u;
}

}  // namespace wbx
