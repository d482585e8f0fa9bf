// wbx_stretch.hip — stretch_search_kernel and stretch_ola_kernel: a frame range of a resident planar F32 clip time-stretched
// by WSOLA (waveform-similarity overlap-add) into a new planar F32 clip of another length and the same pitch (wbx.h
// "Stretching a clip"), and layer 1's calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/stretch_model.py.
//   the search   step k needs p_{k-1}, so the steps are a chain and ONE workgroup of 512 lanes walks the steps of a launch in
//             order.  A step whose natural continuation c_k lies within the tolerance of its anchor costs a few scalar
//             operations.  A step that searches is wbx_wsola.h's wsola_search — staging, the lanes' score chains, the
//             arg-max — the same code warp_search_kernel (wbx_warp.hip) runs (moving the window and reading at the point
//             of use instead of a turn ahead: 24 % slower)
//   the carry    p and the call's record travel from launch to launch through StretchCarry in device memory, the positions
//             of a band through the stage: pos[0] = p_{band0 - 1}, pos[1 + k - band0] = p_k
//   overlap-add  a lane per 16-B word of the result (4 frames of one step: Hs is a multiple of 4), over the band's frames:
//             the copy branch (p_k == c_k) or the blend, one rounding to fp32, the result's ragged last word frame by frame
// Nothing waits on another workgroup anywhere.
#include "wbx_ctx.h"
#include "wbx_wsola.h"

#include <cstring>

namespace wbx {

namespace {

using namespace wsola;   // wbx_wsola.h: the searched step, shared with warp_search_kernel

template <int CH>
__global__ void __launch_bounds__(kLanes) stretch_search_kernel(StretchArgs a) {
  __shared__ Lds lds;
  const uint32_t tid = threadIdx.x;
  const int64_t n = (int64_t)a.n, Hs = (int64_t)a.Hs, D = (int64_t)a.D;
  // (everything below up to the staging is the same in every lane)
  int64_t p = a.k0 == 0u ? -Hs : (int64_t)a.carry->p;
  uint32_t max_shift = a.k0 == 0u ? 0u : a.carry->max_shift;
  uint64_t searched = a.k0 == 0u ? 0ull : a.carry->searched, scored = a.k0 == 0u ? 0ull : a.carry->candidates;
  if (a.k0 == a.band0 && tid == 0u) a.pos[0] = (int32_t)p;
  int64_t anchor = (int64_t)a.a0;
  uint64_t rem = a.r0;
  for (uint32_t k = a.k0; k < a.k1; k++) {
    const int64_t c = p + Hs;
    const int64_t lo = anchor - D > 0 ? anchor - D : 0, hi = anchor + D < n - 1 ? anchor + D : n - 1;
    if (lo <= c && c <= hi) {
      p = c;
    } else if (lo == hi) {                                     // one candidate: its score is the greatest
      p = lo;
      searched++, scored++;
    } else {
      const uint32_t ncand = (uint32_t)(hi - lo) + 1u;
      p = wsola_search<CH>(lds, a.src[0], a.src[1], n, a.Hs, c, lo, ncand, tid);
      searched++, scored += ncand;
    }
    const int64_t shift = p > anchor ? p - anchor : anchor - p;
    max_shift = (uint32_t)shift > max_shift ? (uint32_t)shift : max_shift;
    if (tid == 0u) a.pos[1u + (k - a.band0)] = (int32_t)p;
    anchor += (int64_t)a.qn;
    rem += a.rn;
    if (rem >= (uint64_t)a.m) rem -= a.m, anchor++;
  }
  __syncthreads();                                             // every lane has read the carry (a launch may hold no search, hence no barrier)
  if (tid == 0u) *a.carry = StretchCarry{(int32_t)p, max_shift, searched, scored};
}

// x[c][g] of the text: zero outside [0, n), what is not finite as 0.0
__device__ __forceinline__ double x_at(const float* __restrict__ row, int64_t g, int64_t n) { return g < n ? sample_in(row[g]) : 0.0; }

template <int CH>
__global__ void __launch_bounds__(256) stretch_ola_kernel(StretchArgs a) {
  const uint64_t word = (uint64_t)blockIdx.x * 256u + threadIdx.x;   // the lane's 16-B word of the band
  const uint64_t j0 = (uint64_t)a.band0 * a.Hs + 4u * word;     // its first frame of the result
  const uint64_t band_end = ((uint64_t)a.band0 + a.band_steps) * a.Hs;
  if (j0 >= (uint64_t)a.m || j0 >= band_end) return;
  const uint32_t k = (uint32_t)(j0 / a.Hs), i0 = (uint32_t)(j0 - (uint64_t)k * a.Hs);
  const int64_t n = (int64_t)a.n;
  const int64_t p = (int64_t)a.pos[1u + (k - a.band0)], c = (int64_t)a.pos[k - a.band0] + (int64_t)a.Hs;
  const double* __restrict__ up = a.win;
  const double* __restrict__ dn = a.win + a.Hs;
  const uint32_t left = a.m - (uint32_t)j0;
#pragma unroll
  for (int ch = 0; ch < CH; ch++) {
    const float* __restrict__ row = a.src[ch];
    float y[4];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const uint32_t i = i0 + (uint32_t)f;
      const double xp = x_at(row, p + (int64_t)i, n);
      y[f] = p == c ? __double2float_rn(xp)
                    : __double2float_rn(__dadd_rn(__dmul_rn(up[i], xp), __dmul_rn(dn[i], x_at(row, c + (int64_t)i, n))));
    }
    float* out = a.dst[ch] + j0;
    if (left >= 4u) {
      __builtin_nontemporal_store(f4{y[0], y[1], y[2], y[3]}, reinterpret_cast<f4*>(out));
    } else {                                                   // the result's last word: only the frames inside it
#pragma unroll
      for (int f = 0; f < 4; f++)
        if ((uint32_t)f < left) out[f] = y[f];
    }
  }
}

}  // namespace

void launch_stretch_search(const StretchArgs& a, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(stretch_search_kernel<2>, dim3(1), dim3(kLanes), 0, s, a);
  else hipLaunchKernelGGL(stretch_search_kernel<1>, dim3(1), dim3(kLanes), 0, s, a);
}
void launch_stretch_ola(const StretchArgs& a, hipStream_t s) {
  const uint64_t frames = (uint64_t)a.band_steps * a.Hs;       // (the kernel stops at the result's end)
  const uint32_t blocks = (uint32_t)((frames / 4u + 255u) / 256u);
  if (a.channels == 2u) hipLaunchKernelGGL(stretch_ola_kernel<2>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(stretch_ola_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status stretch_check(const ClipSrc& src, const StretchCall& k, const char** why) {
  const wbx_status st = stretch_check_args(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip stretch: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip stretch: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip stretch: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status stretch_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const StretchCall& k, ClipSlot& slot, int32_t* positions_out,
                       wbx_stretch_info* info, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.out_frames, why);
  if (st != WBX_OK) return st;
  StretchStage& z = c->str;
  const uint32_t N = k.window, Hs = N / 2u;
  const uint64_t n = k.n_frames, m = k.out_frames, K = stretch_steps(m, N);
  const uint32_t per_launch = stretch_launch_steps(n, N, k.tolerance);
  StretchArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.n = (uint32_t)n, a.m = (uint32_t)m;
  a.Hs = Hs, a.D = k.tolerance;
  a.qn = (uint32_t)(((uint64_t)Hs * n) / m), a.rn = (uint32_t)(((uint64_t)Hs * n) % m);
  a.channels = src.channels;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  const bool fresh = z.win_of != N;
  if (e == hipSuccess && fresh) {
    z.win_of = 0;                                              // (no table until this one's upload has completed)
    e = z.h_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) e = z.d_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) (void)stretch_window(N, z.h_win.p, N);
  }
  if (e == hipSuccess) e = z.d_pos.ensure((size_t)kStretchBandSteps + 1u);
  if (e == hipSuccess && positions_out) e = z.h_pos.ensure((size_t)kStretchBandSteps + 1u);
  if (e == hipSuccess) e = z.d_carry.ensure(1);
  if (e == hipSuccess) e = z.h_carry.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(z.d_win.p, z.h_win.p, (size_t)N * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.pos = z.d_pos.p;
    a.carry = z.d_carry.p;
    a.win = z.d_win.p;
  }
  uint64_t launches = 0;
  const uint64_t bands = stretch_bands(K);
  for (uint64_t i = 0; i < bands && e == hipSuccess; i++) {
    const StretchBand b = stretch_band(K, per_launch, i);
    a.band0 = (uint32_t)b.first;
    a.band_steps = b.steps;
    for (uint32_t k0 = a.band0; k0 < a.band0 + b.steps && e == hipSuccess; k0 += per_launch) {
      a.k0 = k0;
      a.k1 = k0 + per_launch < a.band0 + b.steps ? k0 + per_launch : a.band0 + b.steps;
      const unsigned __int128 at = (unsigned __int128)k0 * Hs * n;   // (< 2^27 * 2^12 * 2^31)
      a.a0 = (uint64_t)(at / m), a.r0 = (uint64_t)(at % m);
      launch_stretch_search(a, on);
      e = hipGetLastError();
      launches++;
    }
    if (e == hipSuccess) {
      launch_stretch_ola(a, on);
      e = hipGetLastError();
      launches++;
    }
    if (e == hipSuccess && positions_out) {                    // a caller who asks for positions waits band by band
      e = hipMemcpyAsync(z.h_pos.p, z.d_pos.p + 1, (size_t)b.steps * sizeof(int32_t), hipMemcpyDeviceToHost, on);
      if (e == hipSuccess) e = hipStreamSynchronize(on);
      if (e == hipSuccess) std::memcpy(positions_out + b.first, z.h_pos.p, (size_t)b.steps * sizeof(int32_t));
    }
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_carry.p, z.d_carry.p, sizeof(StretchCarry), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip stretch", e);
  }
  z.win_of = N;
  z.timed = true;
  if (info) {
    const StretchCarry& t = z.h_carry.p[0];
    info->steps = K;
    info->searched_steps = t.searched;
    info->candidates = t.candidates;
    info->max_shift = t.max_shift;
    info->launches = (uint32_t)launches;
  }
  return clipfx_measure_result(c, slot, m, stats, why);
}

}  // namespace wbx

extern "C" uint64_t wbx_stretch_steps(uint64_t out_frames, uint32_t window_frames) { return wbx::stretch_steps(out_frames, window_frames); }
extern "C" uint64_t wbx_stretch_anchor(uint64_t k, uint64_t n_frames, uint64_t out_frames, uint32_t window_frames) {
  return wbx::stretch_anchor(k, n_frames, out_frames, window_frames);
}
extern "C" wbx_status wbx_stretch_window(uint32_t window_frames, double* out, size_t cap_doubles) {
  return wbx::stretch_window(window_frames, out, cap_doubles);
}
extern "C" uint32_t wbx_stretch_band_steps(void) { return wbx::kStretchBandSteps; }
extern "C" uint64_t wbx_stretch_launch_terms(void) { return wbx::kStretchLaunchTerms; }
extern "C" uint64_t wbx_stretch_step_terms(void) { return wbx::kStretchStepTerms; }
extern "C" uint32_t wbx_stretch_launch_steps(uint64_t n_frames, uint32_t window_frames, uint32_t tolerance_frames) {
  return wbx::stretch_launch_steps(n_frames, window_frames, tolerance_frames);
}

extern "C" wbx_status wbx_stretch_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::str, "stretch time: no stretch call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_stretch(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                       uint64_t out_frames, uint32_t window_frames, uint32_t tolerance_frames, int32_t* positions_out,
                                       size_t positions_cap, wbx_stretch_info* info, wbx_clip_stats* stats_of_result) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip stretch: unknown source clip", "clip stretch: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const StretchCall k{first_frame, n_frames, out_frames, window_frames, tolerance_frames, positions_out != nullptr, positions_cap};
  const char* msg = "";
  st = stretch_check(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return stretch_run(c, src, rate, k, slot, positions_out, info, stats_of_result, why);
  });
}
