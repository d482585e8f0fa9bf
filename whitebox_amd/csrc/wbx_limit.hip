// wbx_limit.hip — curve_kernel<LimitCurve>, limit_apply_kernel and limit_reduce_kernel: a frame range of a resident planar F32
// clip through a look-ahead peak limiter into a new planar F32 clip (wbx.h "Limiting a clip"), and layer 1's calls on top
// of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/limit_model.py.  The curve is
// wbx_gaincurve.h's in its min sense over need, need being 1.0 outside [0, n):
//     y[m] = min(1.0, min over t in [0, A + H + R) of need[m - t] + table[t]),   m in [0, n + A).
// The tiles, the segments, the sliding register window, the padded LDS rows, the vote, the window sum, the fold and the
// host's band loop are that header's, shared with wbx_dynamics.hip.  What is the limiter's own:
//   staging   need from coalesced 4-B loads of the source's channels: drive, |.|, the maximum over the channels, one
//             division where the ceiling is exceeded
//   the vote  raised by a need below 1.0
//   apply     the window sum divided by A + 1, the minimum with need[i] recomputed from the source, one multiplication per
//             channel, one rounding; the tile's wbx_limit_stats go to part[tile]
// LDS: curve 40 KB (four workgroups per CU); apply 7690 doubles + 8 KB for the statistics (68 KB, two per CU).
#include "wbx_gaincurve.h"

namespace wbx {

namespace {

// d of every channel at range frame g (inside [0, n)), and the detector's p
template <int CH>
__device__ __forceinline__ double drive_in(const LimitArgs& a, uint32_t g, double (&d)[CH]) {
  double p = 0.0;
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const float v = a.src[c][g];
    d[c] = __dmul_rn(a.drive, finite_bits(v) ? (double)v : 0.0);
    p = fmax(p, fabs(d[c]));
  }
  return p;
}
__device__ __forceinline__ double need_of(double p, double ceiling) { return p > ceiling ? __ddiv_rn(ceiling, p) : 1.0; }

template <int CH>
struct LimitCurve {            // curve_kernel's policy
  typedef LimitArgs Args;
  static constexpr bool kMax = false;
  static __device__ __forceinline__ double rest(const Args&) { return 1.0; }
  static __device__ __forceinline__ double staged(const Args& a, uint32_t g) {
    double d[CH];
    return need_of(drive_in<CH>(a, g, d), a.ceiling);
  }
  static __device__ __forceinline__ bool moved(double need, double) { return need < 1.0; }
};

struct LimitFold {
  typedef LimitPartial Partial;
  static __device__ __forceinline__ void merge(LimitPartial& a, const LimitPartial& b) {
    a.peak_in = fmax(a.peak_in, b.peak_in);
    if (b.min_gain < a.min_gain || (b.min_gain == a.min_gain && b.min_gain_frame < a.min_gain_frame)) {
      a.min_gain = b.min_gain;
      a.min_gain_frame = b.min_gain_frame;
    }
    a.limited_frames += b.limited_frames;
  }
  static __device__ __forceinline__ LimitPartial nothing() { return LimitPartial{0.0, 2.0, ~0ull, 0ull}; }
};

template <int CH>
struct LimitApply {            // apply_kernel's policy
  typedef LimitArgs Args;
  typedef LimitFold Fold;
  static constexpr int kCh = CH;
  static __device__ __forceinline__ void frame(const Args& a, uint32_t i, double avg, int f, float (&y)[CH][8], LimitPartial& mine) {
    double d[CH];
    const double p = drive_in<CH>(a, i, d);
    const double g = fmin(avg, need_of(p, a.ceiling));
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const float v = __double2float_rn(__dmul_rn(d[c], g));
      y[c][f] = v != v ? __uint_as_float(kCanonNaN) : v;
    }
    mine.peak_in = fmax(mine.peak_in, p);
    if (g < mine.min_gain) mine.min_gain = g, mine.min_gain_frame = i;   // (ascending frames: the first stays)
    mine.limited_frames += g < 1.0 ? 1u : 0u;
  }
};

}  // namespace

void launch_limit_curve(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(curve_kernel<LimitCurve<2>>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(curve_kernel<LimitCurve<1>>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_limit_apply(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(apply_kernel<LimitApply<2>>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(apply_kernel<LimitApply<1>>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_limit_reduce(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL((reduce_kernel<LimitFold, LimitArgs>), dim3(1), dim3(256), 0, s, a, n_tiles);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status limit_check(const ClipSrc& src, const LimitCall& k, const char** why) {
  const wbx_status st = limit_check_args(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip limit: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip limit: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip limit: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status limit_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const LimitCall& k, ClipSlot& slot, wbx_limit_stats* out,
                     wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.n_frames, why);
  if (st != WBX_OK) return st;
  LimitArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.ceiling = (double)k.ceiling;
  a.drive = k.drive;
  a.channels = src.channels;
  return gain_run(
      c, c->lim, "clip limit", hipSuccess, a, k.lookahead, k.hold, k.release, k.n_frames, slot, stats, why,
      [&](const LimitBand& b) { return launch_band(a, b, on, launch_limit_curve, launch_limit_apply, launch_limit_reduce); },
      [&](const LimitPartial& t) {
        if (!out) return;
        out->peak_in = t.peak_in;
        out->min_gain = t.min_gain;
        out->min_gain_frame = t.min_gain_frame;
        out->limited_frames = t.limited_frames;
      });
}

}  // namespace wbx

extern "C" wbx_status wbx_limit_ramp(uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames, double* out,
                                     size_t cap_doubles) {
  return limit_ramp(lookahead_frames, hold_frames, release_frames, out, cap_doubles);
}
extern "C" uint32_t wbx_limit_tile_frames(void) { return kLimitTile; }
extern "C" uint32_t wbx_limit_segment_terms(void) { return kLimitSegment; }
extern "C" uint32_t wbx_limit_band_frames(void) { return kLimitBand; }

extern "C" wbx_status wbx_limit_ms(wbx_ctx* c, double* out) {
  return stage_ms(c, &wbx_ctx::lim, "limit time: no limit has completed on this context", out);
}

extern "C" wbx_status wbx_clip_limit(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                     float ceiling, double drive, uint32_t lookahead_frames, uint32_t hold_frames,
                                     uint32_t release_frames, wbx_limit_stats* limit_stats, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip limit: unknown source clip", "clip limit: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const LimitCall k{first_frame, n_frames, ceiling, drive, lookahead_frames, hold_frames, release_frames};
  const char* msg = "";
  st = limit_check(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return limit_run(c, src, rate, k, slot, limit_stats, stats_of_result, why);
  });
}
