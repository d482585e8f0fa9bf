// wbx_loudness.hip — loudness_kernel and true_peak_kernel: ITU-R BS.1770-4 / EBU R 128 figures of a frame range of a resident
// planar F32 clip (wbx.h "Measuring a clip's loudness"), and layer 1's call on top of them.
//
// No reference counterpart: dsp/dsp_ops.h stops at find_abs_maximum.  The arithmetic is written out in wbx.h, its host half
// (hops, coefficients, gate) is wbx_loudness.h and all of it is mirrored by tests/loudness_model.py: the K filter is two fp64
// biquads whose every * + - is one IEEE operation (the explicit _rn intrinsics below: nothing may be fused), run per hop from
// rest two hops earlier, so hops are independent of each other and the device's energies equal the model's bit for bit.
//
// loudness_kernel: a lane owns ONE hop and every channel of it (CH independent fp64 recurrences that hide each other's
// latency), a wave — one workgroup — owns 64 consecutive hops.  A lane's run is the 3 * hop frames from (h - 2) * hop on;
// the lanes' frames lie `hop` apart, so the wave stages the runs chunk by chunk through LDS:
//   stage    for each of its 64 rows the 64 lanes load 64 consecutive frames of that row's run, one coalesced 256-B read
//            per row and channel, into xs[c][row][0..63].  A frame below 0 of the range (the first two hops' run-in), a row
//            past the last hop and a column past the run are staged as 0.0f and NOT read.  No run reaches past its own hop,
//            so nothing behind the range is read either
//   consume  each lane walks its own row in frame order.  Rows are 65 floats long: lane l reads word 65 l + k, bank
//            (l + k) mod 32 — the 32 lanes a 4-byte LDS read serves per cycle hit 32 banks.  Every lane runs the same
//            3 * hop steps (starting from rest over zeros leaves the state zero: no per-lane start masks); the squares are
//            added on the run's last `hop` frames only, a wave-uniform test
// E[c][h] is stored as fp64, one value per lane and channel: no atomics.  LDS: CH * 64 * 65 * 4 bytes (33 KB stereo).
// The pass is bound by the latency of its recurrence (some 24 dependent fp64 operations per frame), not by bandwidth.
//
// true_peak_kernel: resample_kernel's tile at L = factor, M = 1 — the source span staged in LDS, frames outside the range
// staged as 0.0f and never read, a lane owning 4 consecutive outputs of every channel, the same fp64 fma chain in ascending
// tap order and one rounding to fp32 — with a running maximum per lane and channel in place of the store; phase-0 outputs
// also take the source sample they sit on.  Reduced across the wave by lane shuffles and across waves by one integer
// atomic max per wave and channel on the bits of the non-negative float (clipfx_kernel's way with its peak).
#include "wbx_ctx.h"

namespace wbx {

namespace {

constexpr uint32_t kRowWords = 65;                             // a staged row: 64 frames and one word of padding
constexpr uint32_t kPeakSpanMax = 560;                         // 1024 / 2 + 48 at factor 2 (kPeakTile: wbx_loudness.h)

struct Biquad {
  double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
  // y = ((((b0*x + b1*x1) + b2*x2) - a1*y1) - a2*y2), single operations
  __device__ __forceinline__ double step(const double* k, double x) {
    double y = __dadd_rn(__dmul_rn(k[0], x), __dmul_rn(k[1], x1));
    y = __dadd_rn(y, __dmul_rn(k[2], x2));
    y = __dsub_rn(y, __dmul_rn(k[3], y1));
    y = __dsub_rn(y, __dmul_rn(k[4], y2));
    x2 = x1, x1 = x, y2 = y1, y1 = y;
    return y;
  }
};

template <int CH>
__global__ void __launch_bounds__(64) loudness_kernel(LoudnessArgs a) {
  __shared__ float xs[CH][64][kRowWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t h0 = blockIdx.x * 64u;                        // the wave's first hop (< hops <= 2^31 / 800)
  const uint32_t steps = 3u * a.hop, own_from = 2u * a.hop;    // a run's frames / the first that belongs to the hop itself
  double k1[5], k2[5];
#pragma unroll
  for (int i = 0; i < 5; i++) k1[i] = a.coef[i], k2[i] = a.coef[5 + i];
  Biquad s1[CH], s2[CH];
  double e[CH];
#pragma unroll
  for (int c = 0; c < CH; c++) e[c] = 0.0;

  for (uint32_t t0 = 0; t0 < steps; t0 += 64u) {
    const uint32_t t = t0 + lane;                              // the column this lane stages, in every row
#pragma unroll 8
    for (uint32_t r = 0; r < 64u; r++) {
      const int64_t g = ((int64_t)(h0 + r) - 2) * (int64_t)a.hop + (int64_t)t;   // frame of the range; < (h0 + r + 1) * hop
      const bool in = t < steps && h0 + r < a.hops && g >= 0;
#pragma unroll
      for (int c = 0; c < CH; c++) xs[c][r][lane] = in ? a.src[c][g] : 0.0f;
    }
    __syncthreads();
    const uint32_t m = steps - t0 < 64u ? steps - t0 : 64u;
    for (uint32_t k = 0; k < m; k++) {
      const bool own = t0 + k >= own_from;                     // wave-uniform
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float xf = xs[c][lane][k];
        const double v = s2[c].step(k2, s1[c].step(k1, xf != xf ? 0.0 : (double)xf));
        if (own) e[c] = __dadd_rn(e[c], __dmul_rn(v, v));
      }
    }
    __syncthreads();                                           // the next chunk's staging overwrites xs
  }
  if (h0 + lane < a.hops) {
#pragma unroll
    for (int c = 0; c < CH; c++) a.energy[(size_t)c * a.hops + h0 + lane] = e[c];
  }
}

template <int CH>
__global__ void __launch_bounds__(256) true_peak_kernel(TruePeakArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[CH * kPeakSpanMax];
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = tid * 4u;                                // the lane's first output frame inside the tile
  const uint32_t span = (a.L - 1u + (kPeakTile - 1u)) / a.L + a.T;   // 304 at L = 4, 560 at L = 2
  const uint32_t n_out = a.n_in * a.L;                         // < 2^31 - 16
  const uint32_t n_tiles = (n_out + kPeakTile - 1u) / kPeakTile;
  float pk[CH];
#pragma unroll
  for (int c = 0; c < CH; c++) pk[c] = 0.0f;
  uint32_t off[4], row[4];                                     // kPeakTile is a multiple of L: a tile starts at phase 0
#pragma unroll
  for (int q = 0; q < 4; q++) {                                // (off + k <= 1023 / L + T - 1 < span)
    off[q] = (q0 + (uint32_t)q) / a.L;
    row[q] = (q0 + (uint32_t)q) % a.L;
  }
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t j0 = tile * kPeakTile;
    const int64_t lo = (int64_t)(j0 / a.L) - (int64_t)(a.H - 1u);   // the frame of the range that xs[0] holds (may be < 0)
    for (uint32_t s = tid; s < span; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      const bool in = g >= 0 && g < (int64_t)a.n_in;
#pragma unroll
      for (int c = 0; c < CH; c++) xs[c * span + s] = in ? a.src[c][g] : 0.0f;
    }
    __syncthreads();
    if (j0 + q0 < n_out) {
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
          for (int c = 0; c < CH; c++) acc[c][q] = __fma_rn(h, (double)xs[c * span + off[q] + k], acc[c][q]);
        }
      }
      const uint32_t left = n_out - (j0 + q0);
#pragma unroll
      for (int c = 0; c < CH; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if ((uint32_t)q >= left) continue;                   // outputs past the result count for nothing
          const float v = fabsf(__double2float_rn(acc[c][q]));
          if (v > pk[c]) pk[c] = v;                            // (a NaN never raises it)
          if (row[q] == 0u) {                                  // the source frame this output sits on: xs[off + H - 1]
            const float x = fabsf(xs[c * span + off[q] + a.H - 1u]);
            if (x > pk[c]) pk[c] = x;
          }
        }
    }
    __syncthreads();                                           // the next tile's staging overwrites xs
  }
#pragma unroll
  for (int c = 0; c < CH; c++) {
    uint32_t b = __float_as_uint(pk[c]);                       // non-negative, no NaN: the bits order as the values do
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)b, m);
      b = o > b ? o : b;
    }
    if ((tid & 63u) == 0u && b) atomicMax(&a.peak[c], b);
  }
}

}  // namespace

void launch_loudness(const LoudnessArgs& a, hipStream_t s) {
  const dim3 grid((a.hops + 63u) / 64u);
  if (a.channels == 2u) hipLaunchKernelGGL((loudness_kernel<2>), grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL((loudness_kernel<1>), grid, dim3(64), 0, s, a);
}

void launch_true_peak(const TruePeakArgs& a, hipStream_t s) {
  uint32_t n_tiles = 0, blocks = 0;
  true_peak_launch_shape(a.L, a.n_in, &n_tiles, &blocks);
  const dim3 grid(blocks);
  if (a.channels == 2u) hipLaunchKernelGGL((true_peak_kernel<2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((true_peak_kernel<1>), grid, dim3(256), 0, s, a);
}

// ---- layer 1: checks (no device call), the run ------------------------------------------------------------------------------

wbx_status loudness_check(const ClipSrc& src, uint32_t rate, uint64_t first_frame, uint64_t n_frames, uint32_t flags,
                          const wbx_loudness* out, const double* hop_energy, size_t cap_doubles, LoudnessPlan* plan, const char** why) {
  if (!out) return *why = "clip loudness: out is NULL", WBX_ERR_INVALID;
  if (n_frames == 0) return *why = "clip loudness: no frames", WBX_ERR_INVALID;
  if (first_frame > src.frames || n_frames > src.frames - first_frame) return *why = "clip loudness: the range ends past the clip", WBX_ERR_INVALID;
  if (flags & ~(uint32_t)WBX_LOUD_TRUE_PEAK) return *why = "clip loudness: unknown flags", WBX_ERR_INVALID;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip loudness: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip loudness: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (!loudness_rate_ok(rate)) return *why = "clip loudness: the clip's sample rate is outside 8000 .. 384000", WBX_ERR_UNSUPPORTED;
  plan->rate = rate;
  plan->hop = loudness_hop_frames(rate);
  plan->hops = n_frames / plan->hop;
  plan->factor = (flags & WBX_LOUD_TRUE_PEAK) ? loudness_oversampling(rate) : 0u;
  if (hop_energy && cap_doubles < (size_t)(src.channels * plan->hops)) return *why = "clip loudness: hop_energy holds fewer than channels * hops doubles", WBX_ERR_INVALID;
  if (plan->factor && n_frames * plan->factor >= kResampleMaxFrames)
    return *why = "clip loudness: the oversampled range would have 2^31 - 16 frames or more", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

wbx_status loudness_run(wbx_ctx* c, const ClipSrc& src, const LoudnessPlan& p, uint64_t first_frame, uint64_t n_frames,
                        wbx_loudness* out, double* hop_energy, std::string* why) {
  LoudnessStage& x = c->loud;
  const hipStream_t on = c->fx.side.stream;
  const size_t n_energy = (size_t)src.channels * p.hops;
  const float* row[2] = {clip_row(src, 0) + first_frame, clip_row(src, 1) + first_frame};
  ResamplePlan rp;                                             // the oversampling as a conversion: L = factor, M = 1
  const char* msg = "";
  if (p.factor > 1u && resample_plan(p.rate, p.rate * p.factor, WBX_SRC_GOOD, &rp, &msg) != WBX_OK)
    return stage_fail(why, WBX_ERR_UNSUPPORTED, msg);
  hipError_t e = hipSuccess;
  if (n_energy) {
    e = x.d_energy.ensure(n_energy);
    if (e == hipSuccess) e = x.h_energy.ensure(n_energy);
    if (e == hipSuccess) {
      LoudnessArgs a{};
      a.src[0] = row[0], a.src[1] = row[1];
      a.energy = x.d_energy.p;
      loudness_coefficients(p.rate, a.coef);
      a.hop = p.hop;
      a.hops = (uint32_t)p.hops;
      a.channels = src.channels;
      launch_loudness(a, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(x.h_energy.p, x.d_energy.p, n_energy * sizeof(double), hipMemcpyDeviceToHost, on);
  }
  bool fresh = false;
  if (e == hipSuccess && p.factor > 1u) {
    TruePeakArgs a{};
    e = x.d_peak.ensure(2);
    if (e == hipSuccess) e = x.h_peak.ensure(2);
    if (e == hipSuccess) e = resample_table_device(c, rp, WBX_SRC_GOOD, &a.table, &fresh);
    if (e == hipSuccess) e = hipMemsetAsync(x.d_peak.p, 0, 2 * sizeof(uint32_t), on);
    if (e == hipSuccess) {
      a.src[0] = row[0], a.src[1] = row[1];
      a.peak = x.d_peak.p;
      a.n_in = (uint32_t)n_frames;
      a.L = rp.L, a.H = rp.H, a.T = rp.T;
      a.channels = src.channels;
      launch_true_peak(a, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(x.h_peak.p, x.d_peak.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, on);
  }
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: the table's upload reads host memory)
  if (e == hipSuccess) e = w;
  if (fresh) std::vector<float>().swap(c->rs_tables.back().host);   // uploaded (or never will be)
  if (e != hipSuccess) {
    if (fresh) c->rs_tables.pop_back();                        // its upload may not have happened
    return stage_fail(why, WBX_ERR_DEVICE, "clip loudness", e);
  }
  wbx_loudness r;
  loudness_gate(src.channels, p.hops, p.hop, x.h_energy.p, &r);
  r.oversampling = p.factor;
  if (p.factor > 1u) {
    for (uint32_t ch = 0; ch < src.channels; ch++) std::memcpy(&r.true_peak[ch], &x.h_peak.p[ch], sizeof(float));
  } else if (p.factor == 1u) {                                 // the sample peak: the measure pass, on the same stream
    wbx_clip_stats st{};
    const wbx_status ms = clipfx_measure_run(c, src, first_frame, n_frames, &st, why);
    if (ms != WBX_OK) return ms;
    for (uint32_t ch = 0; ch < src.channels; ch++) r.true_peak[ch] = st.peak[ch];
  }
  if (hop_energy && n_energy) std::memcpy(hop_energy, x.h_energy.p, n_energy * sizeof(double));
  *out = r;
  return WBX_OK;
}

}  // namespace wbx

extern "C" uint32_t wbx_loudness_hop_frames(uint32_t rate) { return loudness_rate_ok(rate) ? loudness_hop_frames(rate) : 0u; }

extern "C" uint64_t wbx_loudness_hops(uint32_t rate, uint64_t n_frames) {
  return loudness_rate_ok(rate) ? n_frames / loudness_hop_frames(rate) : 0u;
}

extern "C" wbx_status wbx_true_peak_launch_shape(uint32_t rate, uint64_t n_frames, uint32_t* factor, uint32_t* n_tiles, uint32_t* grid) {
  if (!factor || !n_tiles || !grid || n_frames == 0) return WBX_ERR_INVALID;
  if (!loudness_rate_ok(rate)) return WBX_ERR_UNSUPPORTED;
  const uint32_t f = loudness_oversampling(rate);
  if (n_frames * f >= kResampleMaxFrames) return WBX_ERR_UNSUPPORTED;
  *factor = f;
  *n_tiles = *grid = 0;                                        // factor 1: the sample peak is the measure pass, no tiles
  if (f > 1u) true_peak_launch_shape(f, (uint32_t)n_frames, n_tiles, grid);
  return WBX_OK;
}

extern "C" wbx_status wbx_loudness_coefficients(uint32_t rate, double out[10]) {
  if (!out) return WBX_ERR_INVALID;
  if (!loudness_rate_ok(rate)) return WBX_ERR_UNSUPPORTED;
  loudness_coefficients(rate, out);
  return WBX_OK;
}

extern "C" wbx_status wbx_loudness_gate(uint32_t channels, uint64_t hops, uint32_t hop_frames, const double* hop_energy, wbx_loudness* out) {
  if (!out || channels < 1 || channels > 2 || hop_frames == 0 || (hops && !hop_energy)) return WBX_ERR_INVALID;
  loudness_gate(channels, hops, hop_frames, hop_energy, out);
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_loudness(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t flags,
                                        wbx_loudness* out, double* hop_energy, size_t cap_doubles) {
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip loudness: unknown clip");
  const ClipSrc src = clip_src(*s);
  const char* msg = "";
  LoudnessPlan plan;
  const wbx_status st = loudness_check(src, s->d.sample_rate, first_frame, n_frames, flags, out, hop_energy, cap_doubles, &plan, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return loudness_run(c, src, plan, first_frame, n_frames, out, hop_energy, why); });
}
