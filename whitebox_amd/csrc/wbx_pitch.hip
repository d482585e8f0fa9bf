// wbx_pitch.hip — pitch_kernel: a frame range of a resident planar F32 clip transposed — another PITCH at a length of the
// caller's choice — into a new planar F32 clip that keeps the source's rate (wbx.h "Pitch-shifting a clip"), and layer 1's
// calls on top of it.
//
// No reference counterpart.  The result is by definition the composition of two texts of wbx.h: "Stretching a clip" to
// m' = ceil(m M / L) frames, then "Converting a clip's sample rate" of that intermediate by M / L, of which the first m frames
// are kept; tests/pitch_model.py is those two models one after the other.  The intermediate exists only in LDS:
//   the search   wbx_stretch.hip's stretch_search_kernel as it is, launch by launch as stretch_run plans them, but into ONE
//             buffer of all K' + 1 positions (pos[0] = p_{-1} = -Hs, pos[1 + k] = p_k): a band's launches get buffer + band0,
//             so the kernel's own write of pos[0] at a band's start rewrites the word with the value it already holds
//   pitch_kernel resample_kernel's tile — 256 lanes per tile of <= 1024 outputs, a span of <= 4096 floats per channel in
//             dynamic LDS, grid-stride over the tiles, 4 consecutive outputs x CH fp64 accumulators per lane, the table in
//             phase-visit order, whole 16-B stores — whose staging step is stretch_ola_kernel's arithmetic: span word s is
//             frame g = lo + s of the intermediate, step k = g / Hs, the copy branch or the blend with the same explicit fp64
//             operators, rounded once to fp32.  A frame outside [0, m') is staged as 0.0f and nothing is read for it
// A lane stages at most 16 words per channel and tile against its 4 * T >= 96 multiply-adds per channel, so the staging's
// division and its two dependent loads are in the noise.
// LDS: CH * span * 4 bytes, dynamic (at most 32 KB).  No scratch.  Nothing waits on another workgroup.
#include "wbx_ctx.h"

#include <cstring>

namespace wbx {

namespace {

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
// x[c][g] of the stretch's text: zero outside [0, n), what is not finite as 0.0
__device__ __forceinline__ double x_at(const float* __restrict__ row, int64_t g, int64_t n) {
  if (g >= n) return 0.0;
  const float v = row[g];
  return finite_bits(v) ? (double)v : 0.0;
}

template <int CH>
__global__ void __launch_bounds__(256) pitch_kernel(PitchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [CH][span]: the intermediate's frames lo .. lo + span - 1
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = tid * 4u;                                // the lane's first output frame inside the tile
  const int64_t n = (int64_t)a.n;
  const double* __restrict__ up = a.win;
  const double* __restrict__ dn = a.win + a.Hs;
  for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const uint32_t j0 = tile * a.tile;                         // < n_out < 2^31
    const uint64_t t0 = (uint64_t)j0 * a.M;
    const uint64_t i0 = t0 / a.L;                              // < mid
    const uint32_t p0 = (uint32_t)(t0 - i0 * a.L);
    const int64_t lo = (int64_t)i0 - (int64_t)(a.H - 1u);      // the frame of the intermediate that xs[0] holds (may be < 0)
    for (uint32_t s = tid; s < a.span; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      if (g < 0 || g >= (int64_t)a.mid) {
#pragma unroll
        for (int c = 0; c < CH; c++) xs[c * a.span + s] = 0.0f;
        continue;
      }
      const uint32_t k = (uint32_t)g / a.Hs, i = (uint32_t)g - k * a.Hs;   // (g < 2^31; k < K': pos[k], pos[1 + k] exist)
      const int64_t p = (int64_t)a.pos[1u + k], cc = (int64_t)a.pos[k] + (int64_t)a.Hs;
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float* __restrict__ row = a.src[c];
        const double xp = x_at(row, p + (int64_t)i, n);
        xs[c * a.span + s] = p == cc ? __double2float_rn(xp)
                                     : __double2float_rn(__dadd_rn(__dmul_rn(up[i], xp), __dmul_rn(dn[i], x_at(row, cc + (int64_t)i, n))));
      }
    }
    __syncthreads();
    if (q0 < a.tile && j0 + q0 < a.n_out) {
      const uint32_t r0 = j0 % a.L;
      uint32_t off[4], row[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {                            // (q0 + q <= tile - 1: off + k stays below span)
        off[q] = (p0 + (q0 + (uint32_t)q) * a.M) / a.L;
        row[q] = (r0 + q0 + (uint32_t)q) % a.L;
      }
      double acc[CH][4];
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[c][q] = 0.0;
      const float* tab = a.table;
      for (uint32_t k = 0; k < a.T; k++, tab += a.L) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const double h = (double)tab[row[q]];
#pragma unroll
          for (int c = 0; c < CH; c++) acc[c][q] = __fma_rn(h, (double)xs[c * a.span + off[q] + k], acc[c][q]);
        }
      }
      const uint32_t left = a.n_out - (j0 + q0);
#pragma unroll
      for (int c = 0; c < CH; c++) {
        float y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float v = __double2float_rn(acc[c][q]);
          y[q] = v != v ? __uint_as_float(kCanonNaN) : v;
        }
        float* out = a.dst[c] + j0 + q0;
        if (left >= 4u) {
          __builtin_nontemporal_store(f4v{y[0], y[1], y[2], y[3]}, reinterpret_cast<f4v*>(out));
        } else {                                               // the result's last lane: only the frames inside it
#pragma unroll
          for (int q = 0; q < 4; q++)
            if ((uint32_t)q < left) out[q] = y[q];
        }
      }
    }
    __syncthreads();                                           // the next tile's staging overwrites xs
  }
}

}  // namespace

void launch_pitch(PitchArgs a, hipStream_t s) {
  const ResampleShape sh = resample_launch_shape(a.L, a.M, a.T, a.n_out);   // the conversion's own tile, span and grid
  a.tile = sh.tile, a.span = sh.span, a.n_tiles = sh.n_tiles;
  const dim3 grid(sh.grid);
  const size_t lds = (size_t)a.channels * a.span * sizeof(float);
  if (a.channels == 2u) hipLaunchKernelGGL((pitch_kernel<2>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((pitch_kernel<1>), grid, dim3(256), lds, s, a);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status pitch_check(const ClipSrc& src, const PitchCall& k, ResamplePlan* plan, StretchCall* stretch, const char** why) {
  const wbx_status st = pitch_check_args(k, plan, stretch, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip pitch: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip pitch: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip pitch: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise).  `sk` is
// the stretch the call performs: its out_frames is m'
wbx_status pitch_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const PitchCall& k, const ResamplePlan& plan, const StretchCall& sk,
                     ClipSlot& slot, int32_t* positions_out, wbx_pitch_info* info, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.out_frames, why);
  if (st != WBX_OK) return st;
  StretchStage& z = c->str;
  PitchStage& y = c->pit;
  const uint32_t N = sk.window, Hs = N / 2u;
  const uint64_t n = sk.n_frames, mid = sk.out_frames, K = stretch_steps(mid, N);
  const uint32_t per_launch = stretch_launch_steps(n, N, sk.tolerance);
  StretchArgs a{};                                             // the searches': their result is the intermediate, which nobody stores
  PitchArgs f{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = f.src[i] = clip_row(src, i) + k.first_frame;
    f.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.n = (uint32_t)n, a.m = (uint32_t)mid;
  a.Hs = Hs, a.D = sk.tolerance;
  a.qn = (uint32_t)(((uint64_t)Hs * n) / mid), a.rn = (uint32_t)(((uint64_t)Hs * n) % mid);
  a.channels = src.channels;
  y.timed = false;
  hipError_t e = hipSuccess;
  for (Event& ev : y.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  const bool fresh_win = z.win_of != N;
  if (e == hipSuccess && fresh_win) {
    z.win_of = 0;                                              // (no table until this one's upload has completed)
    e = z.h_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) e = z.d_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) (void)stretch_window(N, z.h_win.p, N);
  }
  if (e == hipSuccess) e = y.d_pos.ensure((size_t)K + 1u);
  if (e == hipSuccess && positions_out) e = y.h_pos.ensure((size_t)K);
  if (e == hipSuccess) e = z.d_carry.ensure(1);
  if (e == hipSuccess) e = z.h_carry.ensure(1);
  bool fresh_tab = false;
  if (e == hipSuccess) e = resample_table_device(c, plan, k.quality, &f.table, &fresh_tab);
  if (e == hipSuccess) e = hipEventRecord(y.mark[0], on);
  if (e == hipSuccess && fresh_win) e = hipMemcpyAsync(z.d_win.p, z.h_win.p, (size_t)N * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.carry = z.d_carry.p;
    a.win = f.win = z.d_win.p;
    f.pos = y.d_pos.p;
  }
  uint64_t launches = 0;
  const uint64_t bands = stretch_bands(K);
  for (uint64_t i = 0; i < bands && e == hipSuccess; i++) {
    const StretchBand b = stretch_band(K, per_launch, i);
    a.band0 = (uint32_t)b.first;
    a.band_steps = b.steps;
    a.pos = y.d_pos.p + a.band0;                               // the kernel's pos[1 + k - band0] is the buffer's [1 + k]
    for (uint32_t k0 = a.band0; k0 < a.band0 + b.steps && e == hipSuccess; k0 += per_launch) {
      a.k0 = k0;
      a.k1 = k0 + per_launch < a.band0 + b.steps ? k0 + per_launch : a.band0 + b.steps;
      const unsigned __int128 at = (unsigned __int128)k0 * Hs * n;   // (< 2^22 * 2^12 * 2^31)
      a.a0 = (uint64_t)(at / mid), a.r0 = (uint64_t)(at % mid);
      launch_stretch_search(a, on);
      e = hipGetLastError();
      launches++;
    }
  }
  if (e == hipSuccess) {
    f.n = (uint32_t)n, f.mid = (uint32_t)mid, f.n_out = (uint32_t)k.out_frames;
    f.Hs = Hs;
    f.L = plan.L, f.M = plan.M, f.H = plan.H, f.T = plan.T;
    f.channels = src.channels;
    launch_pitch(f, on);
    e = hipGetLastError();
    launches++;
  }
  if (e == hipSuccess) e = hipEventRecord(y.mark[1], on);
  if (e == hipSuccess && positions_out) e = hipMemcpyAsync(y.h_pos.p, y.d_pos.p + 1, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_carry.p, z.d_carry.p, sizeof(StretchCarry), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (fresh_tab) std::vector<float>().swap(c->rs_tables.back().host);   // uploaded (or never will be)
  if (e != hipSuccess) {
    if (fresh_tab) c->rs_tables.pop_back();                    // its upload may not have happened
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip pitch", e);
  }
  z.win_of = N;
  y.timed = true;
  if (positions_out) std::memcpy(positions_out, y.h_pos.p, (size_t)K * sizeof(int32_t));
  if (info) {
    const StretchCarry& t = z.h_carry.p[0];
    info->steps = K;
    info->searched_steps = t.searched;
    info->candidates = t.candidates;
    info->mid_frames = mid;
    info->max_shift = t.max_shift;
    info->launches = (uint32_t)launches;
    info->L = plan.L;
    info->M = plan.M;
  }
  return clipfx_measure_result(c, slot, k.out_frames, stats, why);
}

}  // namespace wbx

extern "C" uint64_t wbx_pitch_mid_frames(uint64_t out_frames, uint32_t num, uint32_t den) { return wbx::pitch_mid_frames(out_frames, num, den); }
extern "C" uint32_t wbx_pitch_max_steps(void) { return wbx::kPitchMaxSteps; }

extern "C" wbx_status wbx_pitch_launch_shape(uint32_t num, uint32_t den, int quality, uint64_t out_frames, uint32_t* tile, uint32_t* span,
                                             uint32_t* n_tiles, uint32_t* grid) {
  using namespace wbx;
  uint32_t L = 0, M = 0;
  ResamplePlan p;
  const char* msg = "";
  if (out_frames == 0 || out_frames >= kPitchMaxFrames || !tile || !span || !n_tiles || !grid) return WBX_ERR_INVALID;
  if (num == 0 || den == 0) return WBX_ERR_INVALID;
  if (!pitch_ratio_ok(num, den, &L, &M)) return L == M ? WBX_ERR_INVALID : WBX_ERR_UNSUPPORTED;   // (a ratio of 1 is the call's INVALID)
  const wbx_status st = resample_plan(num, den, quality, &p, &msg);
  if (st != WBX_OK) return st;
  const ResampleShape sh = resample_launch_shape(p.L, p.M, p.T, (uint32_t)out_frames);
  *tile = sh.tile, *span = sh.span, *n_tiles = sh.n_tiles, *grid = sh.grid;
  return WBX_OK;
}

extern "C" wbx_status wbx_pitch_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::pit, "pitch time: no pitch call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_pitch(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                     uint64_t out_frames, uint32_t num, uint32_t den, int quality, uint32_t window_frames,
                                     uint32_t tolerance_frames, int32_t* positions_out, size_t positions_cap, wbx_pitch_info* info,
                                     wbx_clip_stats* stats_of_result) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip pitch: unknown source clip", "clip pitch: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const PitchCall k{first_frame, n_frames, out_frames, num, den, quality, window_frames, tolerance_frames, positions_out != nullptr, positions_cap};
  ResamplePlan plan;
  StretchCall sk{};
  const char* msg = "";
  st = pitch_check(src, k, &plan, &sk, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return pitch_run(c, src, rate, k, plan, sk, slot, positions_out, info, stats_of_result, why);
  });
}
