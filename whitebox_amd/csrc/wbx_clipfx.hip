// wbx_clipfx.hip — clipfx_kernel: measure a frame range of a resident planar F32 clip, or derive a new F32 clip from it
// (trim, reverse, channel mode, gain, fade-in, fade-out; wbx.h "Editing clips"), and layer 1's two calls on top of it.
//
// No reference counterpart as a whole: dsp::find_abs_maximum and dsp::gain (dsp/dsp_ops.h:10-25) are the pieces, and
// AudioClip::fade_start / fade_end (engine/clip.h:41-42) are stored but read by nothing in Sampler::stream.  The arithmetic
// is written out in wbx.h and mirrored by tests/clipfx_model.py: fp32 with explicit round-to-nearest operations, one fp64
// division per faded frame, no libm.  A NaN result is stored as the quiet NaN 0x7FC00000 whatever produced it, so the
// stored bits do not depend on a processor's NaN conventions (inf * 0 is a negative NaN on x86 and a positive one here).
//
// Lane ownership is export_kernel's: a lane owns 8 consecutive OUTPUT frames of every output channel and stores them as two
// whole 16-B words per channel (a pool clip's channel rows are 256-B aligned: 64-KiB extents, 256-B row stride).  A wave owns
// 512 consecutive frames and strides over the range by the grid, so one launch covers any length.
//   forward   two nontemporal 16-B loads per source channel through a type that promises 4-byte alignment only; a lane
//             whose frames reach past the range reads on into at most 7 frames behind it (the pool's padding covers a
//             clip's end) and stores, sample by sample, only the frames inside the range
//   reversed  the lane loads the MIRRORED 16-B words — source frames first + n - 8 - j0 .. first + n - 1 - j0 — and reverses
//             them in registers: the wave still reads one contiguous 2-KiB span, descending.  Only the range's last lane
//             can start before the range (by at most 7 frames); where that is before the clip's first frame it loads its
//             frames one by one, each guarded
//   fades     the weights (one fp64 division per frame) are computed only in waves whose 512 frames intersect a fade; the
//             branch is wave-uniform.  A body wave pays one multiply per sample
// Statistics are of the values stored (derive) or read (measure): reduced in registers over the lane's whole stride loop,
// across the wave by lane shuffles, across waves by one atomic per wave and value — a 64-bit integer max of
// (bits of |x|) << 32 | ~frame for the peak and its FIRST frame in one word, integer min / max of an order-preserving key
// for the signed extremes, integer adds, and fp64 adds for sum and sum of squares (the only order-dependent fields).
// No LDS, no scratch.
#include "wbx_ctx.h"

namespace wbx {

namespace {

// bits of a non-NaN float -> an unsigned key with the floats' order (-inf < ... < -0.0 < +0.0 < ... < +inf)
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m));
  return v;
}
struct OpMax { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpMin { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct OpAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };

// CS source channels read, CO output channels: (1,1) and (2,2) copy channel for channel (KEEP; SWAP, LEFT and RIGHT through
// the row pointers), (2,1) is MONO_MIX, (1,2) DUAL_MONO.  STORE false: measure — nothing multiplied, nothing written.
template <int CS, int CO, bool REV, bool STORE>
__global__ void __launch_bounds__(256) clipfx_kernel(ClipFxArgs a) {
  constexpr int CC = (CS == 2 && CO == 2) ? 2 : 1;           // channels computed (DUAL_MONO stores one twice)
  const uint32_t n = a.n_frames;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t stride = gridDim.x * 2048u;                 // (n < 2^31, stride <= 2^23: base + stride does not wrap)
  const uint32_t out_from = n - a.fade_out;                  // frames from here on are in the fade-out

  float pk[CC];
  uint32_t pkf[CC], mn[CC], mx[CC], over[CC], nans[CC];
  double sum[CC], sq[CC];
#pragma unroll
  for (int c = 0; c < CC; c++) {
    pk[c] = 0.0f;
    pkf[c] = over[c] = nans[c] = mx[c] = 0u;
    mn[c] = 0xFFFFFFFFu;
    sum[c] = sq[c] = 0.0;
  }

  for (uint32_t base = (blockIdx.x * 4u + wave) * 512u; base < n; base += stride) {
    const uint32_t j0 = base + lane * 8u;                    // the lane's first output frame
    if (j0 >= n) continue;
    const uint32_t left = n - j0;
    const bool faded = STORE && (base < a.fade_in || (a.fade_out && base + 512u > out_from));   // wave-uniform
    float win[8], wout[8];
    if (faded) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const uint32_t j = j0 + (uint32_t)i;
        win[i] = j < a.fade_in ? fade_weight(j, a.fade_in, a.shape_in) : 1.0f;
        wout[i] = (j >= out_from && j < n) ? fade_weight(n - 1u - j, a.fade_out, a.shape_out) : 1.0f;
      }
    }

    float x[CS][8];                                          // the source frames of output frames j0 .. j0 + 7, in output order
#pragma unroll
    for (int c = 0; c < CS; c++) {
      if constexpr (!REV) {
        const float* p = a.src[c] + a.first_frame + j0;
        const f4u lo = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p));
        const f4u hi = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + 4));
        x[c][0] = lo.x, x[c][1] = lo.y, x[c][2] = lo.z, x[c][3] = lo.w;
        x[c][4] = hi.x, x[c][5] = hi.y, x[c][6] = hi.z, x[c][7] = hi.w;
      } else {
        const uint32_t top = a.first_frame + left - 1u;      // source frame of output frame j0 (first + n - 1 - j0)
        if (top >= 7u) {
          const float* p = a.src[c] + (top - 7u);
          const f4u lo = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p));
          const f4u hi = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + 4));
          x[c][7] = lo.x, x[c][6] = lo.y, x[c][5] = lo.z, x[c][4] = lo.w;
          x[c][3] = hi.x, x[c][2] = hi.y, x[c][1] = hi.z, x[c][0] = hi.w;
        } else {                                             // the span would start before the clip's first frame
#pragma unroll
          for (int i = 0; i < 8; i++) x[c][i] = (uint32_t)i <= top ? a.src[c][top - (uint32_t)i] : 0.0f;
        }
      }
    }

#pragma unroll
    for (int c = 0; c < CC; c++) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        float y;
        if constexpr (CS == 2 && CO == 1) y = __fmul_rn(__fadd_rn(x[0][i], x[1][i]), 0.5f);
        else y = x[c][i];
        if constexpr (STORE) y = __fmul_rn(y, a.gain);
        v[i] = y;
      }
      if (faded) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const uint32_t j = j0 + (uint32_t)i;
          if (j < a.fade_in) v[i] = __fmul_rn(v[i], win[i]);
          if (j >= out_from) v[i] = __fmul_rn(v[i], wout[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        if constexpr (STORE) v[i] = v[i] != v[i] ? __uint_as_float(kCanonNaN) : v[i];
        const bool in = (uint32_t)i < left;                  // frames past the range count for nothing
        const float y = v[i], ay = fabsf(y);
        const bool num = in && y == y;
        if (in && ay > pk[c]) pk[c] = ay, pkf[c] = j0 + (uint32_t)i;
        over[c] += (in && (y > 1.0f || y < -1.0f)) ? 1u : 0u;
        nans[c] += (in && y != y) ? 1u : 0u;
        const uint32_t key = order_key(y);
        if (num && key < mn[c]) mn[c] = key;
        if (num && key > mx[c]) mx[c] = key;
        const double d = num ? (double)y : 0.0;
        sum[c] += d;
        sq[c] += d * d;
      }
      if constexpr (STORE) {
#pragma unroll
        for (int o = (CO == CC ? c : 0); o < (CO == CC ? c + 1 : CO); o++) {
          float* out = a.dst[o] + j0;
          if (left >= 8u) {
            __builtin_nontemporal_store(f4v{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4v*>(out));
            __builtin_nontemporal_store(f4v{v[4], v[5], v[6], v[7]}, reinterpret_cast<f4v*>(out) + 1);
          } else {                                           // the range's last lane: only the frames inside it
#pragma unroll
            for (int i = 0; i < 8; i++)
              if ((uint32_t)i < left) out[i] = v[i];
          }
        }
      }
    }
  }

  // statistics: registers -> wave -> one atomic per wave and value that differs from the block's initial image
  const bool first = lane == 0u;
#pragma unroll
  for (int c = 0; c < CC; c++) {
    const uint32_t pb = __float_as_uint(pk[c]);
    const unsigned long long pkey = pb ? ((unsigned long long)pb << 32) | (unsigned long long)(0xFFFFFFFFu - pkf[c]) : 0ull;
    const unsigned long long p = wave_reduce(pkey, OpMax{});
    const uint32_t lo = wave_reduce(mn[c], OpMin{}), hi = wave_reduce(mx[c], OpMax{});
    const uint32_t o = wave_reduce(over[c], OpAdd{}), nn = wave_reduce(nans[c], OpAdd{});
    const double s = wave_reduce(sum[c], OpAdd{}), q = wave_reduce(sq[c], OpAdd{});
    if (first) {
#pragma unroll
      for (int t = c; t < (CO == CC ? c + 1 : CO); t++) {   // DUAL_MONO: both channels hold the same values
        if (p) atomicMax(&a.stats->peak[t], p);
        if (lo != 0xFFFFFFFFu) atomicMin(&a.stats->mn[t], lo);
        if (hi) atomicMax(&a.stats->mx[t], hi);
        if (o) atomicAdd(&a.stats->over[t], o);
        if (nn) atomicAdd(&a.stats->nans[t], nn);
        if (s != 0.0) atomicAdd(&a.stats->sum[t], s);
        if (q != 0.0) atomicAdd(&a.stats->sum_sq[t], q);
      }
    }
  }
}

template <int CS, int CO, bool STORE>
void launch_rev(const ClipFxArgs& a, dim3 grid, hipStream_t s) {
  if constexpr (STORE) {
    if (a.reversed) {
      hipLaunchKernelGGL((clipfx_kernel<CS, CO, true, true>), grid, dim3(256), 0, s, a);
      return;
    }
  }
  hipLaunchKernelGGL((clipfx_kernel<CS, CO, false, STORE>), grid, dim3(256), 0, s, a);
}

}  // namespace

constexpr uint32_t kClipFxGroupFrames = 2048, kClipFxGridMax = 4096;   // 4 waves of 512 frames per workgroup and stride

// 10 instances: (1,1) (2,2) (2,1) (1,2) x forward / reversed with the store, (1,1) (2,2) forward without (measure)
void launch_clipfx(const ClipFxArgs& a, hipStream_t s) {
  const dim3 grid(std::min<uint32_t>((a.n_frames + kClipFxGroupFrames - 1u) / kClipFxGroupFrames, kClipFxGridMax));
  if (!a.dst[0]) {
    if (a.src_channels == 2u) launch_rev<2, 2, false>(a, grid, s);
    else launch_rev<1, 1, false>(a, grid, s);
  } else if (a.src_channels == 2u) {
    if (a.out_channels == 2u) launch_rev<2, 2, true>(a, grid, s);
    else launch_rev<2, 1, true>(a, grid, s);
  } else {
    if (a.out_channels == 2u) launch_rev<1, 2, true>(a, grid, s);
    else launch_rev<1, 1, true>(a, grid, s);
  }
}

// ---- layer 1: checks (no device call), the stream and its ordering, the two runs ------------------------------------------

wbx_status clipfx_check_range(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, const char** why) {
  if (n_frames == 0) return *why = "clip edit: no frames", WBX_ERR_INVALID;
  if (first_frame > src.frames || n_frames > src.frames - first_frame) return *why = "clip edit: the range ends past the clip", WBX_ERR_INVALID;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip edit: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip edit: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

wbx_status clipfx_check_derive(const ClipSrc& src, const wbx_clip_edit_desc* d, uint32_t* out_channels, const char** why) {
  if (!d) return *why = "clip edit: the descriptor is NULL", WBX_ERR_INVALID;
  if (d->n_frames == 0) return *why = "clip edit: no frames", WBX_ERR_INVALID;
  if (d->first_frame > src.frames || d->n_frames > src.frames - d->first_frame) return *why = "clip edit: the range ends past the clip", WBX_ERR_INVALID;
  if (d->flags & ~(uint32_t)WBX_EDIT_REVERSE) return *why = "clip edit: unknown flags", WBX_ERR_INVALID;
  if (d->fade_in_shape < WBX_FADE_LINEAR || d->fade_in_shape > WBX_FADE_SMOOTH || d->fade_out_shape < WBX_FADE_LINEAR ||
      d->fade_out_shape > WBX_FADE_SMOOTH)
    return *why = "clip edit: unknown fade shape", WBX_ERR_INVALID;
  if (d->fade_in > d->n_frames || d->fade_out > d->n_frames) return *why = "clip edit: a fade longer than the range", WBX_ERR_INVALID;
  uint32_t need = 0, out = 0;   // source channels the mode asks for (0: any), channels of the result
  switch (d->channel_mode) {
    case WBX_CH_KEEP: out = src.channels; break;
    case WBX_CH_SWAP: need = 2, out = 2; break;
    case WBX_CH_LEFT:
    case WBX_CH_RIGHT:
    case WBX_CH_MONO_MIX: need = 2, out = 1; break;
    case WBX_CH_DUAL_MONO: need = 1, out = 2; break;
    default: return *why = "clip edit: unknown channel mode", WBX_ERR_INVALID;
  }
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip edit: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip edit: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (need && need != src.channels) return *why = "clip edit: the channel mode does not fit the clip's channel count", WBX_ERR_INVALID;
  *out_channels = out;
  return WBX_OK;
}

void clipfx_release(wbx_ctx* c) {
  side_release(c->fx.side);
  c->fx = ClipFxStage{};
}

wbx_status clipfx_prepare(wbx_ctx* c, std::string* why) {
  ClipFxStage& x = c->fx;
  if (x.side.stream) return WBX_OK;
  (void)hipSetDevice(c->cfg.device);
  hipError_t e = side_prepare(c, x.side);
  if (e == hipSuccess) e = x.d_stats.ensure(1);
  if (e == hipSuccess) e = x.h_stats.ensure(2);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    clipfx_release(c);
    return stage_fail(why, WBX_ERR_DEVICE, "clip edit: stream, events and statistics block", e);
  }
  ClipFxStats& init = x.h_stats.p[0];                         // what a launch starts from
  std::memset(&init, 0, sizeof(init));
  init.mn[0] = init.mn[1] = 0xFFFFFFFFu;
  return WBX_OK;
}

wbx_status clipfx_order(wbx_ctx* c, std::string* why) {
  const hipError_t e = side_order(c, c->fx.side);
  return e == hipSuccess ? WBX_OK : stage_fail(why, WBX_ERR_DEVICE, "clip edit: ordering after the pool's writers", e);
}

wbx_status clipfx_check_ids(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, const char* unknown_src, const char* same) {
  if (!find_clip(c, src_clip)) return fail(c, WBX_ERR_INVALID, unknown_src);
  if (dst_clip == src_clip) return fail(c, WBX_ERR_INVALID, same);
  if (dst_clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  return WBX_OK;
}

wbx_status clipfx_check_ids(wbx_ctx* c, uint32_t src_clip, uint32_t src2_clip, uint32_t dst_clip, const char* unknown_src,
                            const char* unknown_src2, const char* same) {
  if (!find_clip(c, src_clip)) return fail(c, WBX_ERR_INVALID, unknown_src);
  if (!find_clip(c, src2_clip)) return fail(c, WBX_ERR_INVALID, unknown_src2);
  if (dst_clip == src2_clip) return fail(c, WBX_ERR_INVALID, same);
  return clipfx_check_ids(c, src_clip, dst_clip, unknown_src, same);
}

static float key_to_float(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}

// launch, bring the statistics block back where somebody asked for it, wait.  (Every instance reduces and adds its
// statistics, asked for or not — instances without them would double the eight that store.)
static hipError_t fx_launch(wbx_ctx* c, const ClipFxArgs& a, uint32_t channels, uint64_t n_frames, wbx_clip_stats* out) {
  ClipFxStage& x = c->fx;
  const hipStream_t on = x.side.stream;
  hipError_t e = hipMemcpyAsync(x.d_stats.p, &x.h_stats.p[0], sizeof(ClipFxStats), hipMemcpyHostToDevice, on);
  if (e != hipSuccess) return e;
  launch_clipfx(a, on);
  e = hipGetLastError();
  if (e == hipSuccess && out) e = hipMemcpyAsync(&x.h_stats.p[1], x.d_stats.p, sizeof(ClipFxStats), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);             // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess || !out) return e;
  const ClipFxStats& r = x.h_stats.p[1];
  wbx_clip_stats st{};
  for (uint32_t ch = 0; ch < channels; ch++) {
    const uint32_t bits = (uint32_t)(r.peak[ch] >> 32);
    std::memcpy(&st.peak[ch], &bits, sizeof(float));
    st.peak_frame[ch] = bits ? (uint64_t)(0xFFFFFFFFu - (uint32_t)r.peak[ch]) : 0u;
    st.over[ch] = r.over[ch];
    st.nans[ch] = r.nans[ch];
    const bool any = (uint64_t)r.nans[ch] < n_frames;        // a sample that is no NaN was counted
    st.min[ch] = any ? key_to_float(r.mn[ch]) : 0.0f;
    st.max[ch] = any ? key_to_float(r.mx[ch]) : 0.0f;
    st.sum[ch] = r.sum[ch];
    st.sum_sq[ch] = r.sum_sq[ch];
  }
  *out = st;
  return hipSuccess;
}

wbx_status clipfx_measure_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, wbx_clip_stats* out,
                              std::string* why) {
  ClipFxArgs a{};
  for (uint32_t ch = 0; ch < 2; ch++) a.src[ch] = clip_row(src, ch);
  a.stats = c->fx.d_stats.p;
  a.first_frame = (uint32_t)first_frame;
  a.n_frames = (uint32_t)n_frames;
  a.src_channels = a.out_channels = src.channels;
  const hipError_t e = fx_launch(c, a, src.channels, n_frames, out);
  return e == hipSuccess ? WBX_OK : stage_fail(why, WBX_ERR_DEVICE, "clip measure", e);
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status clipfx_derive_run(wbx_ctx* c, const ClipSrc& src, uint32_t sample_rate, const wbx_clip_edit_desc& d,
                             uint32_t out_channels, ClipSlot& slot, wbx_clip_stats* stats, std::string* why) {
  const wbx_status st = clipfx_blank_clip(c, slot, out_channels, sample_rate, d.n_frames, why);
  if (st != WBX_OK) return st;
  ClipFxArgs a{};
  const float* row[2] = {clip_row(src, 0), clip_row(src, 1)};
  switch (d.channel_mode) {
    case WBX_CH_SWAP: a.src[0] = row[1], a.src[1] = row[0]; break;
    case WBX_CH_RIGHT: a.src[0] = a.src[1] = row[1]; break;
    case WBX_CH_LEFT: a.src[0] = a.src[1] = row[0]; break;
    default: a.src[0] = row[0], a.src[1] = row[1]; break;
  }
  a.src_channels = (d.channel_mode == WBX_CH_LEFT || d.channel_mode == WBX_CH_RIGHT) ? 1u : src.channels;
  a.out_channels = out_channels;
  a.dst[0] = (float*)slot.d.ch[0];
  a.dst[1] = (float*)slot.d.ch[1];
  a.stats = c->fx.d_stats.p;
  a.first_frame = (uint32_t)d.first_frame;
  a.n_frames = (uint32_t)d.n_frames;
  a.fade_in = (uint32_t)d.fade_in;
  a.fade_out = (uint32_t)d.fade_out;
  a.shape_in = (uint32_t)d.fade_in_shape;
  a.shape_out = (uint32_t)d.fade_out_shape;
  a.gain = d.gain;
  a.reversed = (d.flags & WBX_EDIT_REVERSE) ? 1u : 0u;
  const hipError_t e = fx_launch(c, a, out_channels, d.n_frames, stats);
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip derive", e);
  }
  return WBX_OK;
}

}  // namespace wbx

extern "C" uint64_t wbx_clipfx_pass_frames(void) { return (uint64_t)wbx::kClipFxGridMax * wbx::kClipFxGroupFrames; }

extern "C" wbx_status wbx_clip_measure(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, wbx_clip_stats* out) {
  if (!c) return WBX_ERR_INVALID;
  if (!out) return fail(c, WBX_ERR_INVALID, "clip measure: out is NULL");
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip measure: unknown clip");
  const ClipSrc src = clip_src(*s);
  const char* msg = "";
  const wbx_status st = clipfx_check_range(src, first_frame, n_frames, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return clipfx_measure_run(c, src, first_frame, n_frames, out, why); });
}

extern "C" wbx_status wbx_clip_derive(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, const wbx_clip_edit_desc* d,
                                      wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip derive: unknown source clip", "clip derive: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const char* msg = "";
  uint32_t out_channels = 0;
  st = clipfx_check_derive(src, d, &out_channels, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return clipfx_derive_run(c, src, rate, *d, out_channels, slot, stats_of_result, why);
  });
}
