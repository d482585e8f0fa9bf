// wbx_f0.hip — f0_kernel: the period track of a frame range of a resident planar F32 clip, one YIN record per hop (wbx.h
// "Tracking a clip's pitch"), and layer 1's call on top of it.  A measurement: nothing is allocated in the pool.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/f0_model.py.
//   the mapping  hops are independent, so the device is filled with them: a wave owns 512 consecutive lags of one hop, a hop
//             takes G = 1, 2, 4 or 8 waves, and a workgroup of 64 G F lanes holds F <= 8 / G CONSECUTIVE hops that share
//             one staged span d[t0 .. t0 + (F - 1) H + W + 512 G) in LDS as FLOATS — the detector is an fp32 value by
//             definition; what lies outside [0, n) is staged as 0 and never read — with the detector (and the non-finite
//             rule) computed while staging.  A hop's template is that same span at the hop's offset, read as a wave-uniform
//             broadcast: there is no second array
//   the chains   stretch_search_kernel's turn, COPIED (wbx_stretch.hip's instances are untouched): a lane owns 8 consecutive
//             lags and their 16 fp64 accumulators (r and E), a sliding window of 12 span words in registers feeds 4 terms x
//             8 lags = 64 fma per 16 bytes read, both reads asked for one turn ahead.  Both factors of every product are
//             fp32 values, so the product is exact in fp64 and fma(t, w, r) IS the model's r + t * w.  A hop's offset in the
//             span is a multiple of H, so only a hop length that is a multiple of 4 keeps the 16-byte reads aligned: the
//             other instance (AL = false) reads word by word
//   the epilogue per hop, between workgroup barriers: dd and the run sums P in registers, T(g) to LDS, one lane per hop
//             walks B, c to LDS as doubles (over the span, which nobody reads any more) for the neighbours, the pick as two
//             minima — (predicate ? tau : none) and (c, tau) — that are exact and free of order, one lane writes the record
// Nothing waits on another workgroup, and there is no scratch.
#include "wbx_ctx.h"

#include <cstring>

namespace wbx {

namespace {

constexpr uint32_t kLanes = kF0Lanes, kPer = kF0PerLane, kWaves = kLanes / 64u;
static_assert(kPer == 8 && kWaves == 8 && kF0WaveLags == 64u * kPer);
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double sample_in(float v) { return finite_bits(v) ? (double)v : 0.0; }

// the detector d[g] for a frame g of the range, g < n ("Stretching a clip"'s)
template <int CH>
__device__ __forceinline__ float detector(const F0Args& a, uint32_t g) {
  if (CH == 1) return finite_bits(a.src[0][g]) ? a.src[0][g] : 0.0f;
  return __double2float_rn(__dmul_rn(0.5, __dadd_rn(sample_in(a.src[0][g]), sample_in(a.src[1][g]))));
}

template <bool AL>
__device__ __forceinline__ f4 ld4(const float* p) {
  if (AL) return *reinterpret_cast<const f4*>(p);
  return f4{p[0], p[1], p[2], p[3]};
}

struct Chains {
  double r[kPer], E[kPer];     // the two chains of the lane's 8 lags
};
// Turn b: terms 4 b .. 4 b + 3 on the lane's 8 lags.  lo, mid = span words 4 b .. 4 b + 7 of the lane (as doubles); hi
// receives words 4 b + 8 .. 4 b + 11 from nv, tv the template's 4 values from nt, and nv / nt are asked for again, for turn
// b + 1 (the last turn asks for 4 words nobody uses: the span holds them).  Lag j at term t reads word j + t
template <bool AL>
__device__ __forceinline__ void turn4(Chains& sc, const double (&lo)[4], const double (&mid)[4], double (&hi)[4], f4& nv, f4& nt,
                                      const float* sp, const float* tp, uint32_t b) {
  const f4 tv = nt;
#pragma unroll
  for (int j = 0; j < 4; j++) hi[j] = (double)nv[j];
  nv = ld4<AL>(sp + 4u * (b + 3u));
  nt = ld4<AL>(tp + 4u * (b + 1u));
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const double td = (double)tv[t];
#pragma unroll
    for (int j = 0; j < (int)kPer; j++) {
      const int q = j + t;
      const double w = q < 4 ? lo[q] : q < 8 ? mid[q - 4] : hi[q - 8];
      sc.r[j] = fma(td, w, sc.r[j]);
      sc.E[j] = fma(w, w, sc.E[j]);
    }
  }
}

__device__ __forceinline__ bool less_c(double c, uint32_t t, double oc, uint32_t ot) { return c < oc || (c == oc && t < ot); }

template <int CH, bool AL>
__global__ void __launch_bounds__(kLanes) f0_kernel(F0Args a) {
  extern __shared__ __attribute__((aligned(16))) float span[];   // f0_lds_bytes: the detector; after the chains: c as doubles
  __shared__ double run[kLanes];                               // T(g), then B(g), of the lane's run
  __shared__ double e0[kWaves];                                // per hop of the workgroup
  __shared__ uint32_t red_first[kWaves], red_tau[kWaves];      // per wave
  __shared__ double red_c[kWaves];
  const uint32_t tid = threadIdx.x;
  const uint32_t hop_lanes = 64u * a.G;                        // lanes of a hop
  const uint32_t fh = tid / hop_lanes, l = tid - fh * hop_lanes;   // the lane's hop of the workgroup, its run of 8 lags
  const uint32_t hop_first = a.hop0 + blockIdx.x * a.F;        // (the grid holds no workgroup without a hop)
  const uint32_t hop = hop_first + fh;
  const bool live = hop < a.hop1;                              // (the same in every lane of a wave)
  const uint32_t n_live = a.hop1 - hop_first < a.F ? a.hop1 - hop_first : a.F;
  const uint64_t t0 = (uint64_t)hop_first * a.H;               // < n: the hop is complete
  const uint32_t words = (n_live - 1u) * a.H + a.W + kF0WaveLags * a.G + kF0SpanSlack;   // <= kF0SpanWords (wbx_f0.h)
  for (uint32_t s = tid; s < words; s += blockDim.x) {
    const uint64_t g = t0 + s;
    span[s] = g < (uint64_t)a.n ? detector<CH>(a, (uint32_t)g) : 0.0f;
  }
  __syncthreads();
  const uint32_t tau0 = l * kPer;                              // the lane's first lag
  const bool works = live && (tau0 & ~(kF0WaveLags - 1u)) <= a.tau_max;   // (per wave) some lag of the wave counts
  Chains sc;
#pragma unroll
  for (int j = 0; j < (int)kPer; j++) sc.r[j] = 0.0, sc.E[j] = 0.0;
  if (works) {
    const float* tp = span + fh * a.H;
    const float* sp = tp + tau0;
    // three groups of 4 span words take turns as the window's low, middle and high part, so that nothing is moved; the
    // operands of the next turn (a 16-B span read, a broadcast template read) are asked for ahead of the fma run
    double w0[4], w1[4], w2[4];
    {
      const f4 v0 = ld4<AL>(sp), v1 = ld4<AL>(sp + 4);
#pragma unroll
      for (int j = 0; j < 4; j++) w0[j] = (double)v0[j], w1[j] = (double)v1[j];
    }
    f4 nv = ld4<AL>(sp + 8), nt = ld4<AL>(tp);
    const uint32_t turns = a.W >> 2;                           // a turn: terms 4 b .. 4 b + 3
    uint32_t b = 0;
    for (; b + 3u <= turns; b += 3u) {
      turn4<AL>(sc, w0, w1, w2, nv, nt, sp, tp, b);
      turn4<AL>(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
      turn4<AL>(sc, w2, w0, w1, nv, nt, sp, tp, b + 2u);
    }
    if (b < turns) turn4<AL>(sc, w0, w1, w2, nv, nt, sp, tp, b);
    if (b + 1u < turns) turn4<AL>(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
  }
  if (l == 0u) e0[fh] = sc.E[0];
  __syncthreads();                                             // (also: every lane is done with the span)
  // dd and the run sums P(g, i) of the lane's run g = l
  const double E0 = e0[fh];
  double dd[kPer], P[kPer];
#pragma unroll
  for (int i = 0; i < (int)kPer; i++) {
    const uint32_t tau = tau0 + (uint32_t)i;
    double v = __dsub_rn(__dadd_rn(E0, sc.E[i]), __dmul_rn(2.0, sc.r[i]));
    if (v < 0.0 || tau == 0u || tau > a.tau_max) v = 0.0;
    dd[i] = v;
    P[i] = i == 0 ? v : __dadd_rn(P[i > 0 ? i - 1 : 0], v);
  }
  run[tid] = P[kPer - 1];
  __syncthreads();
  if (l == 0u) {                                               // B(0) = 0, B(g) = B(g - 1) + T(g - 1), in place
    double* T = run + fh * hop_lanes;
    const uint32_t runs = a.tau_max / kPer + 1u;               // the runs that hold a lag that counts (<= hop_lanes)
    double B = 0.0;
    for (uint32_t g = 0; g < runs; g++) {
      const double t = T[g];
      T[g] = B;
      B = __dadd_rn(B, t);
    }
  }
  __syncthreads();
  double* cs = reinterpret_cast<double*>(span);                // c(8 tid + i) of the workgroup's hops
  double c[kPer];
  {
    const double B = run[tid];
#pragma unroll
    for (int i = 0; i < (int)kPer; i++) {
      const uint32_t tau = tau0 + (uint32_t)i;
      const double S = __dadd_rn(B, P[i]);
      c[i] = (tau == 0u || S == 0.0) ? 1.0 : __ddiv_rn(__dmul_rn(dd[i], (double)tau), S);
      cs[tid * kPer + (uint32_t)i] = c[i];
    }
  }
  __syncthreads();
  // the pick: the lowest tau of [tau_min, tau_max - 1] with c(tau) < threshold and c(tau + 1) >= c(tau); else the least c
  uint32_t first = kNone, best_tau = kNone;
  double best_c = __builtin_huge_val();
  if (live) {
    const double next = tau0 + kPer <= a.tau_max ? cs[(tid + 1u) * kPer] : 1.0;   // c of the next run's first lag
#pragma unroll
    for (int i = 0; i < (int)kPer; i++) {
      const uint32_t tau = tau0 + (uint32_t)i;
      if (tau < a.tau_min || tau >= a.tau_max) continue;
      const double cn = i < (int)kPer - 1 ? c[i < (int)kPer - 1 ? i + 1 : 0] : next;
      if (first == kNone && c[i] < a.threshold && cn >= c[i]) first = tau;
      if (c[i] < best_c) best_c = c[i], best_tau = tau;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t of = (uint32_t)__shfl_xor((int)first, off);
    const double oc = __shfl_xor(best_c, off);
    const uint32_t ot = (uint32_t)__shfl_xor((int)best_tau, off);
    first = of < first ? of : first;
    if (less_c(oc, ot, best_c, best_tau)) best_c = oc, best_tau = ot;
  }
  if ((tid & 63u) == 0u) red_first[tid >> 6] = first, red_c[tid >> 6] = best_c, red_tau[tid >> 6] = best_tau;
  __syncthreads();
  if (l == 0u && live) {
    const uint32_t w0 = fh * a.G;
    for (uint32_t v = 1; v < a.G; v++) {
      first = red_first[w0 + v] < first ? red_first[w0 + v] : first;
      if (less_c(red_c[w0 + v], red_tau[w0 + v], best_c, best_tau)) best_c = red_c[w0 + v], best_tau = red_tau[w0 + v];
    }
    const uint32_t lag = first != kNone ? first : best_tau;    // in [tau_min, tau_max - 1]: lag - 1 >= 1, lag + 1 <= tau_max
    const double* ch = cs + (size_t)tid * kPer;                // the hop's c(0)
    const double ca = ch[lag - 1u], cb = ch[lag], cg = ch[lag + 1u];
    const double den = __dsub_rn(__dadd_rn(ca, cg), __dmul_rn(2.0, cb));
    const double off = (den > 0.0 && ca >= cb && cg >= cb) ? __ddiv_rn(__dmul_rn(0.5, __dsub_rn(ca, cg)), den) : 0.0;
    wbx_f0_frame rec;
    rec.period = __dadd_rn((double)lag, off);
    rec.dip = cb;
    rec.energy = E0;
    rec.lag = lag;
    rec.voiced = first != kNone ? 1u : 0u;
    a.out[hop] = rec;
  }
}

}  // namespace

void launch_f0(const F0Args& a, hipStream_t s) {
  const dim3 grid((a.hop1 - a.hop0 + a.F - 1u) / a.F), block(64u * a.G * a.F);
  const uint32_t lds = f0_lds_bytes(a.W, a.H, a.G, a.F);       // the span, or the block's c where that is more
  const bool al = a.H % 4u == 0u;
  if (a.channels == 2u) {
    if (al) hipLaunchKernelGGL((f0_kernel<2, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((f0_kernel<2, false>), grid, block, lds, s, a);
  } else {
    if (al) hipLaunchKernelGGL((f0_kernel<1, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((f0_kernel<1, false>), grid, block, lds, s, a);
  }
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status f0_check_call(const ClipSrc& src, const F0Call& k, const char** why) {
  const wbx_status st = f0_check(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip f0: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip f0: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip f0: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

wbx_status f0_run(wbx_ctx* c, const ClipSrc& src, const F0Call& k, wbx_f0_frame* frames_out, wbx_f0_info* info, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  F0Stage& z = c->f0;
  const uint64_t hops = f0_hops(k.n_frames, k.window, k.hop, k.tau_max);
  const uint32_t per_launch = f0_launch_hops(k.window, k.tau_max);
  const F0Shape shape = f0_shape(k.window, k.hop, k.tau_max);
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  if (e == hipSuccess && hops) e = z.d_rec.ensure((size_t)hops);
  if (e == hipSuccess && hops) e = z.h_rec.ensure((size_t)hops);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  F0Args a{};
  a.src[0] = clip_row(src, 0) + k.first_frame, a.src[1] = clip_row(src, 1) + k.first_frame;
  a.out = z.d_rec.p;
  a.threshold = k.threshold;
  a.n = (uint32_t)k.n_frames;
  a.W = k.window, a.H = k.hop;
  a.tau_min = k.tau_min, a.tau_max = k.tau_max;
  a.G = shape.G, a.F = shape.F;
  a.channels = src.channels;
  uint64_t launches = 0;
  for (uint64_t h = 0; h < hops && e == hipSuccess; h += per_launch) {
    a.hop0 = (uint32_t)h;
    a.hop1 = (uint32_t)(h + per_launch < hops ? h + per_launch : hops);
    launch_f0(a, on);
    e = hipGetLastError();
    launches++;
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess && hops) e = hipMemcpyAsync(z.h_rec.p, z.d_rec.p, (size_t)hops * sizeof(wbx_f0_frame), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still read the clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) return stage_fail(why, WBX_ERR_DEVICE, "clip f0", e);
  z.timed = true;
  uint64_t voiced = 0;
  for (uint64_t h = 0; h < hops; h++) voiced += z.h_rec.p[h].voiced;
  if (hops) std::memcpy(frames_out, z.h_rec.p, (size_t)hops * sizeof(wbx_f0_frame));
  if (info) {
    info->hops = hops;
    info->voiced_hops = voiced;
    info->terms = hops * k.window * ((uint64_t)k.tau_max + 1u);
    info->launches = (uint32_t)launches;
    info->_pad = 0;
  }
  return WBX_OK;
}

}  // namespace wbx

extern "C" uint64_t wbx_f0_hops(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames, uint32_t tau_max) {
  return wbx::f0_hops(n_frames, window_frames, hop_frames, tau_max);
}
extern "C" wbx_status wbx_f0_check(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max,
                                   double threshold, int has_frames_out, size_t frames_cap) {
  const wbx::F0Call k{0, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold, has_frames_out != 0, frames_cap};
  const char* msg = "";
  return wbx::f0_check(k, &msg);
}
extern "C" uint64_t wbx_f0_max_hops(void) { return wbx::kF0MaxHops; }
extern "C" uint64_t wbx_f0_launch_terms(void) { return wbx::kF0LaunchTerms; }
extern "C" uint32_t wbx_f0_launch_hops(uint32_t window_frames, uint32_t tau_max) { return wbx::f0_launch_hops(window_frames, tau_max); }

extern "C" wbx_status wbx_f0_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::f0, "f0 time: no f0 call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_f0(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                                  uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max, double threshold, wbx_f0_frame* frames_out,
                                  size_t frames_cap, wbx_f0_info* info) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip f0: unknown clip");
  const ClipSrc src = clip_src(*s);
  const F0Call k{first_frame, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold, frames_out != nullptr, frames_cap};
  const char* msg = "";
  const wbx_status st = f0_check_call(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return f0_run(c, src, k, frames_out, info, why); });
}
