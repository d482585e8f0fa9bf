// wbx_dynamics.hip — curve_kernel<DynCurve>, dynamics_apply_kernel and dynamics_reduce_kernel: a frame range of a resident
// planar F32 clip through a table-driven compressor / expander / gate / ducker into a new planar F32 clip (wbx.h "Dynamics
// of a clip"), and layer 1's calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/dynamics_model.py.  The curve is
// wbx_gaincurve.h's (read that file's head for the tiles, the segments, the sliding register window, the padded LDS rows
// and the vote, all shared with wbx_limit.hip): with curve frame m = j + A and term t = k + A
//     compress   y[m] = min(1.0, min over t of want[m - t] + table[t])
//     gate       y[m] = max(lo,  max over t of want[m - t] - table[t]),          m in [0, n + A), t in [0, A + H + R)
// want being `rest` (1.0 / lo) outside [0, n).  What is this file's own:
//   staging   a staged value is want = tab(p): the level p from coalesced 4-B loads of the DETECTOR's channels (the key's,
//             or the source's own), then two dependent 8-B gathers from the 24.6 KB table in global memory (it stays in
//             L2 / the vector cache; LDS is full of the row) and three fp64 operations.  4095 lookups per 2048 x 2048 terms
//   the vote  raised by a staged value that differs from rest; a segment without one changes nothing in either sense
//   apply     the window sum, one division, two multiplications (gain, makeup), one rounding
// The stage of (2^20 + A) doubles, the cached ramp, the bands and their tiles are the limiter's own (LimitStage,
// wbx_limit.h): one edit runs at a time.
#include "wbx_gaincurve.h"

namespace wbx {

namespace {

// the detector's p at range frame g (inside [0, n))
template <int DCH>
__device__ __forceinline__ double level_in(const DynArgs& a, uint32_t g) {
  double p = 0.0;
#pragma unroll
  for (int c = 0; c < DCH; c++) {
    const float v = a.det[c][g];
    p = fmax(p, fabs(__dmul_rn(a.det_gain, finite_bits(v) ? (double)v : 0.0)));
  }
  return p;
}

// want = tab(p), p >= 0 and finite: wbx_dynamics.h's dynamics_lookup.  idx <= 47 * 64 + 63, so idx + 1 <= kDynTable - 1
__device__ __forceinline__ double lookup(const double* __restrict__ tab, double p) {
  if (p < 0x1p-40) return tab[0];
  if (p >= 256.0) return tab[kDynTable - 1u];
  const uint64_t u = (uint64_t)__double_as_longlong(p), m = u & ((1ull << 52) - 1u);
  const uint32_t idx = ((uint32_t)(u >> 52) - (uint32_t)(1023 + kDynMinExp)) * kDynCells + (uint32_t)(m >> 46);
  const double f = __dmul_rn((double)(long long)(m & ((1ull << 46) - 1u)), 0x1p-46);
  const double lo = tab[idx], hi = tab[idx + 1u];
  return __dadd_rn(lo, __dmul_rn(f, __dsub_rn(hi, lo)));
}

template <int DCH, int SENSE>
struct DynCurve {              // curve_kernel's policy
  typedef DynArgs Args;
  static constexpr bool kMax = SENSE == WBX_DYN_GATE;
  static __device__ __forceinline__ double rest(const Args& a) { return a.rest; }
  static __device__ __forceinline__ double staged(const Args& a, uint32_t g) { return lookup(a.tab, level_in<DCH>(a, g)); }
  static __device__ __forceinline__ bool moved(double want, double rest) { return want != rest; }
};

struct DynFold {
  typedef DynPartial Partial;
  static __device__ __forceinline__ void merge(DynPartial& a, const DynPartial& b) {
    if (b.min_gain < a.min_gain || (b.min_gain == a.min_gain && b.min_gain_frame < a.min_gain_frame)) {
      a.min_gain = b.min_gain;
      a.min_gain_frame = b.min_gain_frame;
    }
    a.reduced_frames += b.reduced_frames;
  }
  static __device__ __forceinline__ DynPartial nothing() { return DynPartial{2.0, ~0ull, 0ull}; }
};

template <int CH>
struct DynApply {              // apply_kernel's policy
  typedef DynArgs Args;
  typedef DynFold Fold;
  static constexpr int kCh = CH;
  static __device__ __forceinline__ void frame(const Args& a, uint32_t i, double g, int f, float (&y)[CH][8], DynPartial& mine) {
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const float x = a.src[c][i];
      const double d = __dmul_rn(a.drive, finite_bits(x) ? (double)x : 0.0);
      const float v = __double2float_rn(__dmul_rn(__dmul_rn(d, g), a.makeup));
      y[c][f] = v != v ? __uint_as_float(kCanonNaN) : v;
    }
    if (g < mine.min_gain) mine.min_gain = g, mine.min_gain_frame = i;   // (ascending frames: the first stays)
    mine.reduced_frames += g < 1.0 ? 1u : 0u;
  }
};

template <int DCH>
void launch_curve_of(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.sense == WBX_DYN_GATE) hipLaunchKernelGGL((curve_kernel<DynCurve<DCH, WBX_DYN_GATE>>), dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((curve_kernel<DynCurve<DCH, WBX_DYN_COMPRESS>>), dim3(n_tiles), dim3(256), 0, s, a);
}

}  // namespace

void launch_dynamics_curve(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.det_channels == 2u) launch_curve_of<2>(a, n_tiles, s);
  else launch_curve_of<1>(a, n_tiles, s);
}
void launch_dynamics_apply(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(apply_kernel<DynApply<2>>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(apply_kernel<DynApply<1>>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_dynamics_reduce(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL((reduce_kernel<DynFold, DynArgs>), dim3(1), dim3(256), 0, s, a, n_tiles);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clips
wbx_status dynamics_check(const ClipSrc& src, uint32_t src_rate, const ClipSrc* key, uint32_t key_rate, const DynCall& k, double* lo,
                          const char** why) {
  const wbx_status st = dynamics_check_args(k, lo, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32 || (key && key->format != (uint32_t)WBX_FMT_F32))
    return *why = "clip dynamics: a clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2 || (key && (key->channels < 1 || key->channels > 2)))
    return *why = "clip dynamics: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip dynamics: the range ends past the clip", WBX_ERR_INVALID;
  if (key && (k.key_first > key->frames || k.n_frames > key->frames - k.key_first))
    return *why = "clip dynamics: the key's range ends past the clip", WBX_ERR_INVALID;
  if (key && key_rate != src_rate) return *why = "clip dynamics: the key's sample rate differs from the source's", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status dynamics_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc* key, uint32_t rate, const DynCall& k, double lo, ClipSlot& slot,
                        wbx_dynamics_stats* out, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.n_frames, why);
  if (st != WBX_OK) return st;
  DynStage& z = c->dyn;
  DynArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.det[i] = key ? clip_row(*key, i) + k.key_first : a.src[i];
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.drive = k.drive;
  a.det_gain = key ? k.key_gain : k.drive;
  a.makeup = k.makeup;
  a.rest = k.sense == WBX_DYN_GATE ? lo : 1.0;
  a.channels = src.channels;
  a.det_channels = key ? key->channels : src.channels;
  a.sense = k.sense;
  hipError_t e = z.h_tab.ensure(kDynTable);
  if (e == hipSuccess) e = z.d_tab.ensure(kDynTable);
  if (e == hipSuccess) std::memcpy(z.h_tab.p, k.table, kDynTable * sizeof(double));
  a.tab = z.d_tab.p;
  return gain_run(
      c, z, "clip dynamics", e, a, k.lookahead, k.hold, k.release, k.n_frames, slot, stats, why,
      [&](const LimitBand& b) {
        hipError_t up = hipSuccess;                            // the transfer table goes up in front of the first band
        if (b.first == 0) up = hipMemcpyAsync(z.d_tab.p, z.h_tab.p, kDynTable * sizeof(double), hipMemcpyHostToDevice, on);
        return up != hipSuccess ? up : launch_band(a, b, on, launch_dynamics_curve, launch_dynamics_apply, launch_dynamics_reduce);
      },
      [&](const DynPartial& t) {
        if (!out) return;
        out->min_gain = t.min_gain;
        out->min_gain_frame = t.min_gain_frame;
        out->reduced_frames = t.reduced_frames;
      });
}

}  // namespace wbx

extern "C" wbx_status wbx_dynamics_table(int kind, double threshold_db, double ratio, double knee_db, double range_db, double* out,
                                         size_t cap_doubles) {
  return dynamics_table(kind, threshold_db, ratio, knee_db, range_db, out, cap_doubles);
}
extern "C" wbx_status wbx_dynamics_check(const double* table, int sense, double* lo) { return dynamics_table_check(table, sense, lo); }
extern "C" wbx_status wbx_dynamics_lookup(const double* table, double level, double* out) {
  if (!table || !out || !(level >= 0.0)) return WBX_ERR_INVALID;
  *out = dynamics_lookup(table, level);
  return WBX_OK;
}

extern "C" wbx_status wbx_dynamics_ms(wbx_ctx* c, double* out) {
  return stage_ms(c, &wbx_ctx::dyn, "dynamics time: no dynamics call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_dynamics(wbx_ctx* c, uint32_t src_clip, uint32_t key_clip, uint32_t dst_clip, uint64_t first_frame,
                                        uint64_t n_frames, uint64_t key_first, int sense, const double* table, double drive,
                                        double key_gain, double makeup, uint32_t lookahead_frames, uint32_t hold_frames,
                                        uint32_t release_frames, wbx_dynamics_stats* dynamics_stats, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  const bool keyed = key_clip != WBX_DYN_NO_KEY;
  wbx_status st = keyed ? clipfx_check_ids(c, src_clip, key_clip, dst_clip, "clip dynamics: unknown source clip", "clip dynamics: unknown key clip",
                                           "clip dynamics: the result may not replace its source or its key")
                        : clipfx_check_ids(c, src_clip, dst_clip, "clip dynamics: unknown source clip",
                                           "clip dynamics: the result may not replace its source or its key");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  ClipSrc key{};
  uint32_t key_rate = rate;
  if (keyed) key = clip_src(c->clips[key_clip]), key_rate = c->clips[key_clip].d.sample_rate;
  const DynCall k{first_frame, n_frames, key_first, keyed, sense, table, drive, key_gain, makeup, lookahead_frames, hold_frames, release_frames};
  const char* msg = "";
  double lo = 1.0;
  st = dynamics_check(src, rate, keyed ? &key : nullptr, key_rate, k, &lo, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return dynamics_run(c, src, keyed ? &key : nullptr, rate, k, lo, slot, dynamics_stats, stats_of_result, why);
  });
}
