// wbx_varispeed.hip — varispeed_kernel: a frame range of a resident planar F32 clip read along a caller-given position
// curve through a band-limited interpolator into a new planar F32 clip (wbx.h "Reading a clip along a position curve"),
// and layer 1's calls on top of it.
//
// No reference counterpart.  The arithmetic is written out in wbx.h, planned, tabulated and tiled by wbx_varispeed.h
// (host-only) and mirrored by tests/varispeed_model.py: per output frame and channel two fp64 chains of T multiply-adds in
// ascending tap order — A over the phase's row h[p], B over the difference row D[p] —, then y = (float)(A + t * B), one
// multiplication, one addition, one rounding; a NaN stored as 0x7FC00000.  The product of two fp32 values is exact in fp64,
// so the explicit fp64 fma below is bit-equal to the model's multiply-then-add; t * B is NOT exact and is never fused.
//
// resample_kernel's shape with a per-output position.  A workgroup of 256 lanes takes one TILE (wbx_varispeed.h: a run of
// whole knot intervals, at most 1024 outputs, its source span at most 4096 frames) and strides over the tiles by the grid:
//   stage    the tile's span goes into LDS once, 4 B per lane and load, coalesced.  A frame outside [0, n_in) is staged as
//            0.0f and NOT read (the accumulators start at +0.0 and h * 0 never changes them: a staged zero is the masked tap)
//   compute  a lane owns 4 consecutive output frames of every channel: 8 * CH fp64 accumulators.  The 4 frames lie in one
//            interval (tiles start at a multiple of G >= 16), so a lane reads its two knots once and forms the positions
//            in 64-bit integers.  Each frame has its own table row; the device table interleaves h and D per row, so one
//            16-byte load brings two taps with both coefficients.  The lanes of a wave sit on unrelated rows (rows are
//            padded to 64 bytes, so a lane's loads stay inside its own cache lines); per tap pair and frame: one 16-byte
//            global load, 2 * CH LDS words, 4 * CH fma
//   store    one whole 16-B word per channel (a pool clip's rows are 256-B aligned, a tile starts at a multiple of 16, a
//            lane at a multiple of 4); the tile's last lane stores its frames one by one, so the clip's padding stays zero
// LDS: CH * (the call's greatest span) * 4 bytes, dynamic, at most 32 KB.  No scratch.  Nothing waits on another workgroup.
#include <cstring>

#include "wbx_ctx.h"

namespace wbx {

namespace {

template <int CH>
__global__ void __launch_bounds__(256) varispeed_kernel(VsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [CH][span]
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = tid * 4u;                                // the lane's first output frame inside the tile
  const uint32_t gmask = (1u << a.g) - 1u;
  const uint32_t tmask = (1u << a.s) - 1u;
  const double tscale = __longlong_as_double((long long)(1023u - a.s) << 52);   // 2^-s
  for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const wbx_varispeed_tile tl = a.tiles[tile];
    const uint32_t span = tl.span;
    const long long lo = tl.lo_frame;
    for (uint32_t s = tid; s < span; s += 256u) {
      const long long g = lo + (long long)s;
      const bool in = g >= 0 && g < (long long)a.n_in;
#pragma unroll
      for (int c = 0; c < CH; c++) xs[c * span + s] = in ? a.src[c][g] : 0.0f;
    }
    __syncthreads();
    if (q0 < tl.n_out) {
      const uint32_t j0 = tl.first_out + q0;                   // < n_out < 2^31; all 4 frames lie in interval j0 >> g
      const uint32_t left = tl.n_out - q0;
      const long long k0 = a.knots[j0 >> a.g];
      const long long dk = a.knots[(j0 >> a.g) + 1u] - k0;     // (|dk| < 2^45, r < 2^10: the product fits 64 bits)
      const uint32_t r0 = j0 & gmask;
      const long long base = lo + (long long)(a.H - 1u);       // the tile's least knot frame
      uint32_t off[4];
      const float* row[4];
      double t[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bool on = (uint32_t)q < left;
        const long long pos = k0 + ((dk * (long long)(r0 + (uint32_t)q)) >> a.g);
        const uint32_t fr = (uint32_t)((unsigned long long)pos & 0xFFFFFFFFull);
        off[q] = on ? (uint32_t)((pos >> 32) - base) : 0u;     // off + T <= span
        row[q] = a.table + (size_t)(on ? fr >> a.s : 0u) * a.row;
        t[q] = __dmul_rn((double)(fr & tmask), tscale);        // exact: at most 24 bits times a power of two
      }
      double A[CH][4], B[CH][4];
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) A[c][q] = 0.0, B[c][q] = 0.0;
#pragma unroll 2
      for (uint32_t k = 0; k < a.T; k += 2u) {
        f4v w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = *reinterpret_cast<const f4v*>(row[q] + 2u * k);
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
          for (int c = 0; c < CH; c++) {
            const double x0 = (double)xs[c * span + off[q] + k];
            const double x1 = (double)xs[c * span + off[q] + k + 1u];
            A[c][q] = __fma_rn((double)w[q].x, x0, A[c][q]);
            B[c][q] = __fma_rn((double)w[q].y, x0, B[c][q]);
            A[c][q] = __fma_rn((double)w[q].z, x1, A[c][q]);
            B[c][q] = __fma_rn((double)w[q].w, x1, B[c][q]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CH; c++) {
        float y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const float v = __double2float_rn(__dadd_rn(A[c][q], __dmul_rn(t[q], B[c][q])));
          y[q] = v != v ? __uint_as_float(kCanonNaN) : v;
        }
        float* out = a.dst[c] + j0;
        if (left >= 4u) {
          __builtin_nontemporal_store(f4v{y[0], y[1], y[2], y[3]}, reinterpret_cast<f4v*>(out));
        } else {                                               // the tile's last lane: only the frames inside it
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

// lds_bytes: a.channels * (the greatest span of the call's tiles) * 4
void launch_varispeed(const VsArgs& a, uint32_t lds_bytes, hipStream_t s) {
  const size_t lds = lds_bytes;
  const dim3 grid(a.n_tiles < kVsGridMax ? a.n_tiles : kVsGridMax);
  if (a.channels == 2u) hipLaunchKernelGGL((varispeed_kernel<2>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((varispeed_kernel<1>), grid, dim3(256), lds, s, a);
}

// ---- layer 1: the check (no device call), the tables, the run --------------------------------------------------------------

wbx_status varispeed_check(const ClipSrc* src, bool replaces, const VsCall& k, VsPlan* plan, const char** why) {
  const wbx_status st = varispeed_check_args(k, plan, why);
  if (st != WBX_OK) return st;
  if (!src) return *why = "clip varispeed: unknown source clip", WBX_ERR_INVALID;
  if (k.first_frame > src->frames || k.n_frames > src->frames - k.first_frame)
    return *why = "clip varispeed: the range ends past the clip", WBX_ERR_INVALID;
  if (replaces) return *why = "clip varispeed: the result may not replace its source", WBX_ERR_INVALID;
  if (src->format != (uint32_t)WBX_FMT_F32) return *why = "clip varispeed: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src->channels < 1 || src->channels > 2) return *why = "clip varispeed: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

namespace {

// the device copy of a plan's interleaved table, made at first use (uploaded on the edit stream, which every run waits for
// before it returns) and kept for the context by (quality, reduced guard)
hipError_t varispeed_table_on_device(wbx_ctx* c, const VsPlan& p, int quality, uint32_t gn, uint32_t gd, const float** out, bool* fresh) {
  VsStage& z = c->vs;
  for (const VsTable& t : z.tables)
    if (t.quality == quality && t.gn == gn && t.gd == gd) return *out = t.d.p, hipSuccess;
  const size_t n = (size_t)p.P * p.row;
  VsTable t;
  t.quality = quality, t.gn = gn, t.gd = gd;
  t.host.resize(n);
  varispeed_table_device(p, t.host.data());
  hipError_t e = t.d.ensure(n);
  if (e == hipSuccess) e = hipMemcpyAsync(t.d.p, t.host.data(), n * sizeof(float), hipMemcpyHostToDevice, c->fx.side.stream);
  if (e != hipSuccess) return e;
  *out = t.d.p;
  *fresh = true;
  z.tables.push_back(std::move(t));                            // (the vector's buffer moves with it: the copy's source stays put)
  return hipSuccess;
}

}  // namespace

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status varispeed_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const VsCall& k, const VsPlan& plan, ClipSlot& slot,
                         wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.out_frames, why);
  if (st != WBX_OK) return st;
  VsStage& z = c->vs;
  z.timed = false;
  const uint64_t n_tiles = varispeed_tiles(k.knots, k.out_frames, k.knot_shift, plan, nullptr, 0);
  const uint64_t g = varispeed_gcd(k.guard_num, k.guard_den);
  VsArgs a{};
  bool fresh = false;
  hipError_t e = hipSuccess;
  for (Event& m : z.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess) e = z.h_knots.ensure(k.n_knots);
  if (e == hipSuccess) e = z.d_knots.ensure(k.n_knots);
  if (e == hipSuccess) e = z.h_tiles.ensure(n_tiles);
  if (e == hipSuccess) e = z.d_tiles.ensure(n_tiles);
  uint32_t span_max = 0;
  if (e == hipSuccess) {
    std::memcpy(z.h_knots.p, k.knots, k.n_knots * sizeof(int64_t));
    (void)varispeed_tiles(k.knots, k.out_frames, k.knot_shift, plan, z.h_tiles.p, n_tiles);
    for (uint64_t i = 0; i < n_tiles; i++)
      if (z.h_tiles.p[i].span > span_max) span_max = z.h_tiles.p[i].span;
    e = hipEventRecord(z.mark[0], on);
  }
  if (e == hipSuccess) e = varispeed_table_on_device(c, plan, k.quality, (uint32_t)(k.guard_num / g), (uint32_t)(k.guard_den / g), &a.table, &fresh);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_knots.p, z.h_knots.p, k.n_knots * sizeof(int64_t), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_tiles.p, z.h_tiles.p, n_tiles * sizeof(wbx_varispeed_tile), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    for (uint32_t ch = 0; ch < 2; ch++) {
      a.src[ch] = clip_row(src, ch) + k.first_frame;
      a.dst[ch] = (float*)slot.d.ch[ch % src.channels];
    }
    a.knots = z.d_knots.p;
    a.tiles = z.d_tiles.p;
    a.n_in = (uint32_t)k.n_frames;
    a.n_out = (uint32_t)k.out_frames;
    a.n_tiles = (uint32_t)n_tiles;
    a.H = plan.H, a.T = plan.T, a.row = plan.row;
    a.g = k.knot_shift, a.s = plan.s;
    a.channels = src.channels;
    launch_varispeed(a, a.channels * span_max * (uint32_t)sizeof(float), on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (fresh) std::vector<float>().swap(z.tables.back().host);  // uploaded (or never will be)
  if (e != hipSuccess) {
    if (fresh) z.tables.pop_back();                            // its upload may not have happened
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip varispeed", e);
  }
  z.timed = true;
  return clipfx_measure_result(c, slot, k.out_frames, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_varispeed_plan(int quality, uint32_t guard_num, uint32_t guard_den, wbx_varispeed_info* out) {
  if (!out) return WBX_ERR_INVALID;
  VsPlan p;
  const char* msg = "";
  const wbx_status st = varispeed_plan(quality, guard_num, guard_den, &p, &msg);
  if (st != WBX_OK) return st;
  *out = wbx_varispeed_info{p.H, p.T, p.P, 0, p.cutoff, p.beta};
  return WBX_OK;
}

extern "C" wbx_status wbx_varispeed_table(int quality, uint32_t guard_num, uint32_t guard_den, float* h, float* d, size_t cap_floats) {
  VsPlan p;
  const char* msg = "";
  const wbx_status st = varispeed_plan(quality, guard_num, guard_den, &p, &msg);
  if (st != WBX_OK) return st;
  if (cap_floats < ((size_t)p.P + 1u) * p.T) return WBX_ERR_INVALID;
  varispeed_table(p, h, d);
  return WBX_OK;
}

extern "C" wbx_status wbx_varispeed_position(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t j, int64_t* pos) {
  if (!knots || !pos || knot_shift < kVsMinShift || knot_shift > kVsMaxShift) return WBX_ERR_INVALID;
  const uint64_t i = j >> knot_shift;
  const bool at_knot = (j & ((1ull << knot_shift) - 1u)) == 0;
  if (i >= n_knots || (i + 1u >= n_knots && !at_knot)) return WBX_ERR_INVALID;
  *pos = varispeed_position(knots, knot_shift, j);
  return WBX_OK;
}

extern "C" wbx_status wbx_varispeed_check(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t n_frames,
                                          uint64_t out_frames, int quality, uint32_t guard_num, uint32_t guard_den) {
  const VsCall k{0, n_frames, out_frames, knots, n_knots, knot_shift, quality, guard_num, guard_den};
  VsPlan p;
  const char* msg = "";
  return varispeed_check_args(k, &p, &msg);
}

extern "C" wbx_status wbx_varispeed_tiles(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t n_frames,
                                          uint64_t out_frames, int quality, uint32_t guard_num, uint32_t guard_den,
                                          wbx_varispeed_tile* tiles, uint64_t cap, uint64_t* n_tiles) {
  const VsCall k{0, n_frames, out_frames, knots, n_knots, knot_shift, quality, guard_num, guard_den};
  VsPlan p;
  const char* msg = "";
  const wbx_status st = varispeed_check_args(k, &p, &msg);
  if (st != WBX_OK) return st;
  if (!n_tiles || (!tiles && cap)) return WBX_ERR_INVALID;
  *n_tiles = varispeed_tiles(knots, out_frames, knot_shift, p, tiles, cap);
  return WBX_OK;
}

extern "C" uint64_t wbx_varispeed_max_knots(void) { return kVsMaxKnots; }

extern "C" wbx_status wbx_varispeed_ms(wbx_ctx* c, double* out) {
  return stage_ms(c, &wbx_ctx::vs, "varispeed time: no varispeed call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_varispeed(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                         uint64_t out_frames, const int64_t* knots, uint64_t n_knots, uint32_t knot_shift,
                                         int quality, uint32_t guard_num, uint32_t guard_den, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, src_clip);
  ClipSrc src{};
  uint32_t rate = 0;
  if (s) src = clip_src(*s), rate = s->d.sample_rate;
  const VsCall k{first_frame, n_frames, out_frames, knots, n_knots, knot_shift, quality, guard_num, guard_den};
  VsPlan plan;
  const char* msg = "";
  const wbx_status st = varispeed_check(s ? &src : nullptr, dst_clip == src_clip, k, &plan, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  if (dst_clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return varispeed_run(c, src, rate, k, plan, slot, stats_of_result, why);
  });
}
