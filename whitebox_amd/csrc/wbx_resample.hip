// wbx_resample.hip — resample_kernel: a frame range of a resident planar F32 clip converted to another sample rate into a
// new planar F32 clip (wbx.h "Converting a clip's sample rate"), and layer 1's calls on top of it.
//
// No reference counterpart: Sampler::stream's two-tap sample_linear is its only resampler.  The arithmetic is written out in
// wbx.h, planned and tabulated by wbx_resample.h (host-only) and mirrored by tests/resample_model.py: per output frame T fp64
// multiply-adds in ascending tap order, one rounding to fp32, a NaN stored as 0x7FC00000.  The product of two fp32 values is
// exact in fp64, so the explicit fp64 fma below is bit-equal to the model's multiply-then-add.
//
// A workgroup owns a TILE of consecutive output frames (a multiple of 4, at most 1024, chosen on the host so that the source
// span the tile needs — ceil(tile * M / L) + T frames per channel — is at most 4096 floats) and strides over the tiles by the
// grid, so one launch covers any length.  Per tile:
//   stage    the span goes into LDS once, 4 B per lane and load, coalesced.  A frame outside the selected range is staged as
//            0.0f and NOT read: H exceeds the pool's 16 padding frames, a range may start at frame 0 of a slab's first clip,
//            and whatever the clip holds beside the range must not count.  (Adding h * 0 never changes an accumulator that
//            started at +0.0 — it can never become -0.0 — so a staged zero is the masked tap.)
//   compute  a lane owns 4 consecutive output frames of every channel: 4 * CH fp64 accumulators, per tap 4 coefficient loads
//            and 4 * CH LDS reads.  The device copy of the table is in phase-VISIT order, laid out [k][r] with row r holding
//            phase (r * M) mod L: output j uses row j mod L, so consecutive outputs read consecutive words of one tap's row
//            (the lanes of a wave 256 consecutive words, wrapping at L).  Tables run from 192 B to 2.6 MB and stay in global
//            memory, where the caches hold the common ones (44.1k <-> 48k at GOOD: 30 KB) whole
//   store    one whole 16-B word per channel (a pool clip's rows are 256-B aligned, a tile starts at a multiple of 4); the
//            result's last lane stores its frames one by one
// Positions: j * M in 64 bits once per tile (j < 2^31, M < 2^15); inside a tile p0 + q * M < 2^25 in 32 bits.
// LDS: CH * span * 4 bytes, dynamic (8 KB for a stereo 44.1k -> 48k tile, at most 32 KB).  No scratch.
#include "wbx_ctx.h"

namespace wbx {

namespace {

template <int CH>
__global__ void __launch_bounds__(256) resample_kernel(ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [CH][span]
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = tid * 4u;                                // the lane's first output frame inside the tile
  for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const uint32_t j0 = tile * a.tile;                         // < n_out < 2^31
    const uint64_t t0 = (uint64_t)j0 * a.M;
    const uint64_t i0 = t0 / a.L;                              // < n_in
    const uint32_t p0 = (uint32_t)(t0 - i0 * a.L);
    const int64_t lo = (int64_t)i0 - (int64_t)(a.H - 1u);      // the frame of the range that xs[0] holds (may be < 0)
    for (uint32_t s = tid; s < a.span; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      const bool in = g >= 0 && g < (int64_t)a.n_in;
#pragma unroll
      for (int c = 0; c < CH; c++) xs[c * a.span + s] = in ? a.src[c][g] : 0.0f;
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

// the tile, its span and the capped grid: resample_launch_shape (wbx_resample.h)
void launch_resample(ResampleArgs a, hipStream_t s) {
  const ResampleShape sh = resample_launch_shape(a.L, a.M, a.T, a.n_out);
  a.tile = sh.tile, a.span = sh.span, a.n_tiles = sh.n_tiles;
  const dim3 grid(sh.grid);
  const size_t lds = (size_t)a.channels * a.span * sizeof(float);
  if (a.channels == 2u) hipLaunchKernelGGL((resample_kernel<2>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((resample_kernel<1>), grid, dim3(256), lds, s, a);
}

// ---- layer 1: checks (no device call), the table, the run ------------------------------------------------------------------

wbx_status resample_check(const ClipSrc& src, uint32_t src_rate, uint64_t first_frame, uint64_t n_frames, uint32_t dst_rate,
                          int quality, ResamplePlan* plan, uint64_t* n_out, const char** why) {
  if (n_frames == 0) return *why = "resample: no frames", WBX_ERR_INVALID;
  if (first_frame > src.frames || n_frames > src.frames - first_frame) return *why = "resample: the range ends past the clip", WBX_ERR_INVALID;
  ResampleQuality q;
  if (!resample_quality(quality, &q)) return *why = "resample: unknown quality", WBX_ERR_INVALID;
  if (dst_rate == 0) return *why = "resample: a destination rate of 0", WBX_ERR_INVALID;
  if (dst_rate == src_rate) return *why = "resample: the clip has that rate already (nothing to convert; the filter is not an identity)", WBX_ERR_INVALID;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "resample: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "resample: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  const wbx_status st = resample_plan(src_rate, dst_rate, quality, plan, why);
  if (st != WBX_OK) return st;
  *n_out = resample_out_frames(plan->L, plan->M, n_frames);
  if (*n_out == 0) return *why = "resample: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  return WBX_OK;
}

// the device copy of the plan's table, phase-visit order [k][r]; made at first use (uploaded on the edit stream, which every
// run waits for before it returns) and kept for the context: a session converts between a handful of rates
hipError_t resample_table_device(wbx_ctx* c, const ResamplePlan& p, int quality, const float** out, bool* fresh) {
  for (const ResampleTable& t : c->rs_tables)
    if (t.L == p.L && t.M == p.M && t.quality == quality) return *out = t.d.p, hipSuccess;
  const size_t n = (size_t)p.L * p.T;
  ResampleTable t;
  t.L = p.L, t.M = p.M, t.quality = quality;
  std::vector<float> phase(n);
  resample_table(p, phase.data());
  t.host.resize(n);
  for (uint32_t r = 0; r < p.L; r++) {
    const float* h = &phase[(size_t)(((uint64_t)r * p.M) % p.L) * p.T];
    for (uint32_t k = 0; k < p.T; k++) t.host[(size_t)k * p.L + r] = h[k];
  }
  hipError_t e = t.d.ensure(n);
  if (e == hipSuccess) e = hipMemcpyAsync(t.d.p, t.host.data(), n * sizeof(float), hipMemcpyHostToDevice, c->fx.side.stream);
  if (e != hipSuccess) return e;
  *out = t.d.p;
  *fresh = true;
  c->rs_tables.push_back(std::move(t));                        // (the vector's buffer moves with it: the copy's source stays put)
  return hipSuccess;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status resample_run(wbx_ctx* c, const ClipSrc& src, const ResamplePlan& p, int quality, uint64_t first_frame, uint64_t n_frames,
                        uint64_t n_out, uint32_t dst_rate, ClipSlot& slot, wbx_clip_stats* stats, std::string* why) {
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, dst_rate, n_out, why);
  if (st != WBX_OK) return st;
  ResampleArgs a{};
  bool fresh = false;
  hipError_t e = resample_table_device(c, p, quality, &a.table, &fresh);
  if (e == hipSuccess) {
    for (uint32_t ch = 0; ch < 2; ch++) {
      a.src[ch] = clip_row(src, ch) + first_frame;
      a.dst[ch] = (float*)slot.d.ch[ch % src.channels];
    }
    a.n_in = (uint32_t)n_frames;
    a.n_out = (uint32_t)n_out;
    a.L = p.L, a.M = p.M, a.H = p.H, a.T = p.T;
    a.channels = src.channels;
    launch_resample(a, c->fx.side.stream);
    e = hipGetLastError();
  }
  const hipError_t w = hipStreamSynchronize(c->fx.side.stream);     // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (fresh) std::vector<float>().swap(c->rs_tables.back().host);   // uploaded (or never will be)
  if (e != hipSuccess) {
    if (fresh) c->rs_tables.pop_back();                        // its upload may not have happened
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip resample", e);
  }
  return clipfx_measure_result(c, slot, n_out, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_resample_plan(uint32_t src_rate, uint32_t dst_rate, int quality, wbx_resample_info* out) {
  if (!out) return WBX_ERR_INVALID;
  ResamplePlan p;
  const char* msg = "";
  const wbx_status st = resample_plan(src_rate, dst_rate, quality, &p, &msg);
  if (st != WBX_OK) return st;
  *out = wbx_resample_info{p.L, p.M, p.H, p.T, (uint64_t)p.L * p.T};
  return WBX_OK;
}

extern "C" wbx_status wbx_resample_launch_shape(uint32_t src_rate, uint32_t dst_rate, int quality, uint64_t n_out, uint32_t* tile,
                                                uint32_t* span, uint32_t* n_tiles, uint32_t* grid) {
  ResamplePlan p;
  const char* msg = "";
  const wbx_status st = resample_plan(src_rate, dst_rate, quality, &p, &msg);
  if (st != WBX_OK) return st;
  if (n_out == 0 || n_out >= kResampleMaxFrames || !tile || !span || !n_tiles || !grid) return WBX_ERR_INVALID;
  const ResampleShape sh = resample_launch_shape(p.L, p.M, p.T, (uint32_t)n_out);
  *tile = sh.tile, *span = sh.span, *n_tiles = sh.n_tiles, *grid = sh.grid;
  return WBX_OK;
}

extern "C" uint64_t wbx_resample_frames(uint32_t src_rate, uint32_t dst_rate, uint64_t n_frames) {
  uint32_t L = 0, M = 0;
  const char* msg = "";
  if (resample_ratio(src_rate, dst_rate, &L, &M, &msg) != WBX_OK) return 0;
  return resample_out_frames(L, M, n_frames);
}

extern "C" wbx_status wbx_resample_table(uint32_t src_rate, uint32_t dst_rate, int quality, float* out, size_t cap_floats) {
  ResamplePlan p;
  const char* msg = "";
  const wbx_status st = resample_plan(src_rate, dst_rate, quality, &p, &msg);
  if (st != WBX_OK) return st;
  if (!out || cap_floats < (size_t)p.L * p.T) return WBX_ERR_INVALID;
  resample_table(p, out);
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_resample(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                        uint32_t dst_rate, int quality, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip resample: unknown source clip", "clip resample: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const char* msg = "";
  ResamplePlan plan;
  uint64_t n_out = 0;
  st = resample_check(src, c->clips[src_clip].d.sample_rate, first_frame, n_frames, dst_rate, quality, &plan, &n_out, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return resample_run(c, src, plan, quality, first_frame, n_frames, n_out, dst_rate, slot, stats_of_result, why);
  });
}
