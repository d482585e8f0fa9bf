// wbx_saturate.hip — saturate_kernel, saturate_direct_kernel and saturate_reduce_kernel: a frame range of a resident planar
// F32 clip through an oversampled table waveshaper into a new planar F32 clip (wbx.h "Saturating a clip"), and layer 1's
// calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h, planned by wbx_saturate.h (host-only) and mirrored by
// tests/saturate_model.py: the up conversion (L = os, M = 1) and the down conversion (L = 1, M = os) are wbx_resample.hip's
// sums — T fp64 multiply-adds in ascending tap order, one rounding to fp32 — with the lookup between them, and the call is
// bit-equal to those three calls in a row.  resample_kernel is not used: the intermediate of os times the clip's length
// never leaves the workgroup.
//
// saturate_kernel<OS, CH>: ONE launch, a workgroup of 256 lanes per tile of output frames (wbx_saturate.h picks the tile: a
// multiple of 256, at most 1024, LDS within 64 KB so that two workgroups share a CU), grid.x = the tiles (at most 2^21: no
// cap, no second pass).  With Z the quality's zero crossings, per tile:
//   stage    the tile + 4 Z - 1 source frames per channel the tile's mid samples reach go into LDS once, 4 B per lane and
//            load, coalesced.  A frame outside the range is staged as 0.0f and NOT read (wbx_resample.hip's rule and reason)
//   up +     a lane takes a source index i of the tile + 2 Z the down filter reaches and computes all OS mid samples
//   shape    i OS + p of every channel: OS * CH fp64 accumulators, per tap one LDS word per channel (consecutive lanes,
//            consecutive words) feeding OS fmas.  The OS coefficients of a tap are wave-uniform and lie side by side in the
//            device table ([2 Z][OS], as doubles: fp32 values widened on the host, so the products stay exact): a uniform
//            index, one scalar load.  Then the lookup: floor, two gathered doubles of the 128 KB table in global memory (it
//            stays in L2; audio is locally smooth, so neighbouring lanes hit the same lines), one rounding to fp32.  The
//            result goes into LDS DE-INTERLEAVED BY PHASE: plane p holds s[i OS + p] at word i.  An index outside [0, n)
//            is stored as 0.0f without a lookup — the intermediate counts as a whole file.  Only the tile's own indices,
//            not its halo, feed the statistics, so every mid sample counts once
//   down     a lane owns 4 consecutive output frames of every channel: 4 * CH fp64 accumulators.  Tap k of output i is
//            word i + m of plane p' with OS m + p' = k - (H - 1), floor-divided, H = Z OS: walking m outside and p' inside
//            is ascending k.  Consecutive lanes read consecutive 16-B words of a plane — no bank conflict at any OS; the
//            interleaved layout would put a lane's 4 frames 4 OS words apart and be 2- to 8-way conflicted.  Per plane the
//            lane keeps a sliding window of 8 words in registers: a block of 4 m costs one 16-B read per plane and channel
//            for 16 fmas.  The device table is [2 Z + 1][OS] doubles with ONE 0.0 in front (k = -1 does not exist: s is
//            always finite, and fma(0.0, s, +0.0) is +0.0, so the first row needs no branch); the last tap, m = 2 Z of
//            plane 0, is the loop's tail.  Whole 16-B stores; the result's last lane stores frame by frame
// and the lanes' statistics are folded through the LDS the planes leave behind into part[tile].  saturate_direct_kernel<CH>
// is os == 1: no stage, no LDS but the fold's, 4 frames per lane.  saturate_reduce_kernel (one workgroup) merges the tiles'
// records — maximum, lowest index among equals, a sum of counts: any order gives the same record, no float atomics.
// LDS: CH * 4 * ((tile + 2 Z) OS + tile + 4 Z) bytes, dynamic, at most 59136.  No scratch.
#include "wbx_ctx.h"

namespace wbx {

namespace {

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ SatPartial sat_nothing() { return SatPartial{-1.0, ~0ull, 0ull}; }
__device__ __forceinline__ void sat_merge(SatPartial& a, const SatPartial& b) {
  if (b.peak_drive > a.peak_drive || (b.peak_drive == a.peak_drive && b.peak_index < a.peak_index)) {
    a.peak_drive = b.peak_drive;
    a.peak_index = b.peak_index;
  }
  a.beyond += b.beyond;
}
// red[0 .. 255] folded into red[0] (every lane of the workgroup calls it)
__device__ __forceinline__ void sat_fold(SatPartial* red, uint32_t tid) {
  for (uint32_t step = 128u; step > 0u; step >>= 1) {
    __syncthreads();
    if (tid < step) {
      SatPartial m = red[tid];
      sat_merge(m, red[tid + step]);
      red[tid] = m;
    }
  }
  __syncthreads();
}

// s of one mid sample u at mid index j: wbx_saturate.h's saturate_lookup on the driven sample, times the makeup, rounded
// once.  `own`: the sample enters the lane's statistics.  idx <= 16383, so idx + 1 <= kSatTable - 1
__device__ __forceinline__ float shape_one(const double* __restrict__ tab, double drive, double makeup, float u, unsigned long long j,
                                           bool own, SatPartial& mine) {
  const double d = finite_bits(u) ? __dmul_rn(drive, (double)u) : 0.0;
  const double a = __dmul_rn(d, kSatCells);
  const bool past = a <= -kSatEdge || a >= kSatEdge;
  double w;
  if (past) {
    w = a < 0.0 ? tab[0] : tab[kSatTable - 1u];
  } else {
    const double fl = floor(a);
    const uint32_t idx = (uint32_t)((int)fl + 8192);
    const double f = __dsub_rn(a, fl);
    const double lo = tab[idx], hi = tab[idx + 1u];
    w = __dadd_rn(lo, __dmul_rn(f, __dsub_rn(hi, lo)));
  }
  if (own) {
    const double mag = fabs(d);
    if (mag > mine.peak_drive || (mag == mine.peak_drive && j < mine.peak_index)) mine.peak_drive = mag, mine.peak_index = j;
    mine.beyond += past ? 1u : 0u;
  }
  return __double2float_rn(__dmul_rn(w, makeup));
}

__device__ __forceinline__ float canon(float v) { return v != v ? __uint_as_float(kCanonNaN) : v; }

// 4 frames of one channel at out (16-B aligned), `left` of them inside the result
__device__ __forceinline__ void store4(float* out, const float (&y)[4], uint32_t left) {
  if (left >= 4u) {
    __builtin_nontemporal_store(f4v{y[0], y[1], y[2], y[3]}, reinterpret_cast<f4v*>(out));
  } else {                                                     // the result's last lane: only the frames inside it
#pragma unroll
    for (int q = 0; q < 4; q++)
      if ((uint32_t)q < left) out[q] = y[q];
  }
}

template <int OS, int CH>
__global__ void __launch_bounds__(256) saturate_kernel(SatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // xs[CH][row], then mid[CH][OS][plane]
  float* xs = lds;
  float* mid = lds + CH * a.row;
  const uint32_t tid = threadIdx.x;
  const uint32_t t0 = blockIdx.x * a.tile;                     // the tile's first output frame, < n < 2^31
  const uint32_t Z = a.Z, taps = 2u * Z, row = a.row, plane = a.plane;
  const double* __restrict__ tab = a.tab;

  // stage: word s of a row holds range frame t0 - (2 Z - 1) + s (the row's last word is never used)
  const int64_t lo = (int64_t)t0 - (int64_t)(taps - 1u);
  for (uint32_t s = tid; s + 1u < row; s += 256u) {
    const int64_t g = lo + (int64_t)s;
    const bool in = g >= 0 && g < (int64_t)a.n;
#pragma unroll
    for (int c = 0; c < CH; c++) xs[c * row + s] = in ? a.src[c][g] : 0.0f;
  }
  __syncthreads();

  // up + shape: word m of a plane holds source index t0 - Z + m, whose taps are words m .. m + 2 Z - 1 of the row
  SatPartial mine = sat_nothing();
  for (uint32_t m = tid; m < plane; m += 256u) {
    const int64_t i = (int64_t)t0 - (int64_t)Z + (int64_t)m;
    float sv[CH][OS];
    if (i >= 0 && i < (int64_t)a.n) {
      double acc[CH][OS];
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int p = 0; p < OS; p++) acc[c][p] = 0.0;
      const double* __restrict__ up = a.up;
      for (uint32_t k = 0; k < taps; k++, up += OS) {
        double h[OS];
#pragma unroll
        for (int p = 0; p < OS; p++) h[p] = up[p];
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const double x = (double)xs[c * row + m + k];
#pragma unroll
          for (int p = 0; p < OS; p++) acc[c][p] = __fma_rn(h[p], x, acc[c][p]);
        }
      }
      const bool own = m >= Z && m < Z + a.tile;               // the tile's own index, not its halo
      const unsigned long long j0 = (unsigned long long)i * OS;
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int p = 0; p < OS; p++)
          sv[c][p] = shape_one(tab, a.drive, a.makeup, __double2float_rn(acc[c][p]), j0 + (unsigned)p, own, mine);
    } else {
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int p = 0; p < OS; p++) sv[c][p] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int p = 0; p < OS; p++) mid[(c * OS + p) * plane + m] = sv[c][p];
  }
  __syncthreads();

  // down: output t0 + q reads words q .. q + 2 Z of the planes; lo / hi = words q0 + w0 .. + 3 / + 4 .. + 7
  const uint32_t q0 = 4u * tid;
  if (q0 < a.tile && t0 + q0 < a.n) {
    double acc[CH][4];
    f4v wl[CH][OS], wh[CH][OS];
#pragma unroll
    for (int c = 0; c < CH; c++) {
#pragma unroll
      for (int q = 0; q < 4; q++) acc[c][q] = 0.0;
#pragma unroll
      for (int p = 0; p < OS; p++) wl[c][p] = *reinterpret_cast<const f4v*>(mid + (c * OS + p) * plane + q0);
    }
    const double* __restrict__ dn = a.down;
    for (uint32_t w0 = 0; w0 < taps; w0 += 4u, dn += 4 * OS) {
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int p = 0; p < OS; p++) wh[c][p] = *reinterpret_cast<const f4v*>(mid + (c * OS + p) * plane + q0 + w0 + 4u);
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int p = 0; p < OS; p++) {
          const double h = dn[r * OS + p];
#pragma unroll
          for (int c = 0; c < CH; c++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const int at = r + q;
              const float v = at < 4 ? wl[c][p][at] : wh[c][p][at - 4];
              acc[c][q] = __fma_rn(h, (double)v, acc[c][q]);
            }
        }
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int p = 0; p < OS; p++) wl[c][p] = wh[c][p];
    }
    const double last = dn[0];                                 // k = 2 H - 1: m = 2 Z of plane 0
    const uint32_t left = a.n - (t0 + q0);
#pragma unroll
    for (int c = 0; c < CH; c++) {
      float y[4];
#pragma unroll
      for (int q = 0; q < 4; q++) y[q] = canon(__double2float_rn(__fma_rn(last, (double)wl[c][0][q], acc[c][q])));
      store4(a.dst[c] + t0 + q0, y, left);
    }
  }
  __syncthreads();                                             // the fold's records overwrite the planes
  SatPartial* red = reinterpret_cast<SatPartial*>(lds);
  red[tid] = mine;
  sat_fold(red, tid);
  if (tid == 0) a.part[blockIdx.x] = red[0];
}

// os == 1: y = s, 1024 frames per workgroup, 4 per lane
template <int CH>
__global__ void __launch_bounds__(256) saturate_direct_kernel(SatArgs a) {
  __shared__ SatPartial red[256];
  const uint32_t tid = threadIdx.x;
  const uint32_t i0 = blockIdx.x * a.tile + 4u * tid;
  SatPartial mine = sat_nothing();
  if (i0 < a.n) {
    const uint32_t left = a.n - i0;
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const float* in = a.src[c] + i0;
      float x[4], y[4];
      if (left >= 4u) {
        const f4u v = *reinterpret_cast<const f4u*>(in);
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = v[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = (uint32_t)q < left ? in[q] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 4; q++) y[q] = shape_one(a.tab, a.drive, a.makeup, x[q], (unsigned long long)i0 + (unsigned)q, (uint32_t)q < left, mine);
      store4(a.dst[c] + i0, y, left);
    }
  }
  red[tid] = mine;
  sat_fold(red, tid);
  if (tid == 0) a.part[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) saturate_reduce_kernel(SatArgs a) {
  __shared__ SatPartial red[256];
  const uint32_t tid = threadIdx.x;
  SatPartial mine = sat_nothing();
  for (uint32_t t = tid; t < a.n_tiles; t += 256u) sat_merge(mine, a.part[t]);
  red[tid] = mine;
  sat_fold(red, tid);
  if (tid == 0) a.part[a.n_tiles] = red[0];
}

template <int OS>
void launch_saturate_of(const SatArgs& a, uint32_t lds, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL((saturate_kernel<OS, 2>), dim3(a.n_tiles), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((saturate_kernel<OS, 1>), dim3(a.n_tiles), dim3(256), lds, s, a);
}

}  // namespace

void launch_saturate(const SatArgs& a, uint32_t lds_bytes, hipStream_t s) {
  switch (a.os) {
    case 8u: launch_saturate_of<8>(a, lds_bytes, s); break;
    case 4u: launch_saturate_of<4>(a, lds_bytes, s); break;
    case 2u: launch_saturate_of<2>(a, lds_bytes, s); break;
    default:
      if (a.channels == 2u) hipLaunchKernelGGL(saturate_direct_kernel<2>, dim3(a.n_tiles), dim3(256), 0, s, a);
      else hipLaunchKernelGGL(saturate_direct_kernel<1>, dim3(a.n_tiles), dim3(256), 0, s, a);
  }
}
void launch_saturate_reduce(const SatArgs& a, hipStream_t s) { hipLaunchKernelGGL(saturate_reduce_kernel, dim3(1), dim3(256), 0, s, a); }

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip to be refused — then the clip: unknown, the range, the result in the
// source's place, the storage
wbx_status saturate_check(const ClipSrc* src, bool replaces, const SatCall& k, const char** why) {
  const wbx_status st = saturate_check_args(k, why);
  if (st != WBX_OK) return st;
  if (!src) return *why = "clip saturate: unknown source clip", WBX_ERR_INVALID;
  if (k.first_frame > src->frames || k.n_frames > src->frames - k.first_frame)
    return *why = "clip saturate: the range ends past the clip", WBX_ERR_INVALID;
  if (replaces) return *why = "clip saturate: the result may not replace its source", WBX_ERR_INVALID;
  if (src->format != (uint32_t)WBX_FMT_F32) return *why = "clip saturate: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src->channels < 1 || src->channels > 2) return *why = "clip saturate: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

namespace {

// the two filters as saturate_kernel reads them, into h (2 Z os doubles, then (2 Z + 1) os): the up table tap-major, the
// down table behind one 0.0 and padded with 0.0
void saturate_filters(uint32_t os, int quality, double* h) {
  ResamplePlan up, down;
  const char* msg = "";
  (void)saturate_plans(os, quality, &up, &down, &msg);         // (the check has accepted them)
  std::vector<float> t((size_t)down.T);                        // down.T = up.L * up.T = 2 Z os
  resample_table(up, t.data());
  for (uint32_t p = 0; p < os; p++)
    for (uint32_t k = 0; k < up.T; k++) h[(size_t)k * os + p] = (double)t[(size_t)p * up.T + k];
  double* d = h + (size_t)up.T * os;
  resample_table(down, t.data());
  d[0] = 0.0;
  for (uint32_t k = 0; k < down.T; k++) d[1u + k] = (double)t[k];
  for (uint32_t k = down.T + 1u; k < (up.T + 1u) * os; k++) d[k] = 0.0;
}

}  // namespace

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status saturate_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const SatCall& k, ClipSlot& slot, wbx_saturate_stats* out,
                        wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.n_frames, why);
  if (st != WBX_OK) return st;
  SatStage& z = c->sat;
  const SatShape sh = saturate_shape(k.os, k.quality, src.channels, k.n_frames);
  SatArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.drive = k.drive, a.makeup = k.makeup;
  a.n = (uint32_t)k.n_frames;
  a.os = k.os, a.channels = src.channels;
  a.tile = sh.tile, a.Z = sh.Z, a.plane = sh.plane, a.row = sh.row, a.n_tiles = sh.n_tiles;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : z.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess) e = z.h_tab.ensure(kSatTable);
  if (e == hipSuccess) e = z.d_tab.ensure(kSatTable);
  if (e == hipSuccess) std::memcpy(z.h_tab.p, k.table, kSatTable * sizeof(double));
  const size_t up_n = (size_t)2u * sh.Z * k.os, coefs = up_n + ((size_t)2u * sh.Z + 1u) * k.os;
  const bool fresh = k.os > 1u && (z.coef_of[0] != k.os || z.coef_of[1] != (uint32_t)k.quality + 1u);
  if (e == hipSuccess && fresh) {
    z.coef_of[0] = 0;                                          // (no filters until these have been uploaded)
    e = z.h_coef.ensure(coefs);
    if (e == hipSuccess) e = z.d_coef.ensure(coefs);
    if (e == hipSuccess) saturate_filters(k.os, k.quality, z.h_coef.p);
  }
  if (e == hipSuccess) e = z.d_part.ensure((size_t)sh.n_tiles + 1u);
  if (e == hipSuccess) e = z.h_total.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_tab.p, z.h_tab.p, kSatTable * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(z.d_coef.p, z.h_coef.p, coefs * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.tab = z.d_tab.p;
    a.up = z.d_coef.p;
    a.down = z.d_coef.p + up_n;
    a.part = z.d_part.p;
    launch_saturate(a, sh.lds_bytes, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_saturate_reduce(a, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_total.p, a.part + sh.n_tiles, sizeof(SatPartial), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip saturate", e);
  }
  if (fresh) z.coef_of[0] = k.os, z.coef_of[1] = (uint32_t)k.quality + 1u;
  z.timed = true;
  if (out) {
    const SatPartial& t = z.h_total.p[0];
    out->peak_drive = t.peak_drive;
    out->peak_index = t.peak_index;
    out->beyond = t.beyond;
  }
  return clipfx_measure_result(c, slot, k.n_frames, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_saturate_table(int kind, double bias, double* out, size_t cap_doubles) {
  return saturate_table(kind, bias, out, cap_doubles);
}
extern "C" wbx_status wbx_saturate_check(const double* table) { return saturate_table_check(table); }
extern "C" wbx_status wbx_saturate_lookup(const double* table, double d, double* out) {
  if (!table || !out || d != d) return WBX_ERR_INVALID;
  *out = saturate_lookup(table, d);
  return WBX_OK;
}

extern "C" wbx_status wbx_saturate_launch_shape(uint32_t os, int quality, uint32_t channels, uint64_t n_frames, uint32_t* tile,
                                                uint32_t* mid_span, uint32_t* src_span, uint32_t* lds_bytes, uint32_t* n_tiles) {
  ResampleQuality q;
  if (n_frames == 0 || !sat_os_ok(os) || !resample_quality(quality, &q)) return WBX_ERR_INVALID;
  if (n_frames >= kSatMaxMid / os + (kSatMaxMid % os ? 1u : 0u)) return WBX_ERR_INVALID;
  if (os > 1u) {
    ResamplePlan up, down;
    const char* msg = "";
    const wbx_status st = saturate_plans(os, quality, &up, &down, &msg);
    if (st != WBX_OK) return st;
  }
  if (channels < 1u || channels > 2u || !tile || !mid_span || !src_span || !lds_bytes || !n_tiles) return WBX_ERR_INVALID;
  const SatShape sh = saturate_shape(os, quality, channels, n_frames);
  *tile = sh.tile, *mid_span = sh.mid_span, *src_span = sh.src_span, *lds_bytes = sh.lds_bytes, *n_tiles = sh.n_tiles;
  return WBX_OK;
}

extern "C" wbx_status wbx_saturate_ms(wbx_ctx* c, double* out) {
  return stage_ms(c, &wbx_ctx::sat, "saturate time: no saturate call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_saturate(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                        uint32_t os, int quality, const double* table, double drive, double makeup,
                                        wbx_saturate_stats* saturate_stats, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, src_clip);
  ClipSrc src{};
  uint32_t rate = 0;
  if (s) src = clip_src(*s), rate = s->d.sample_rate;
  const SatCall k{first_frame, n_frames, os, quality, table, drive, makeup};
  const char* msg = "";
  const wbx_status st = saturate_check(s ? &src : nullptr, dst_clip == src_clip, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  if (dst_clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return saturate_run(c, src, rate, k, slot, saturate_stats, stats_of_result, why);
  });
}
