// wbx_align.hip — aligning two resident planar F32 clips (wbx.h "Aligning two clips"): the cross-correlation of a template of
// clip A with a range of clip B over signed lags, cut into chunks of 2048 terms along the template, and layer 1's call on top
// of it.  A measurement: nothing is allocated in the pool.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/align_model.py.
//   the mapping  a long template over few lags would leave the device empty, so the sum over the template is cut along time —
//             the cut is part of the definition — and a workgroup of align_partial_kernel owns ONE chunk and a block of up to
//             4096 consecutive lags: 64 w lanes x 8 lags, w = align_shape's waves.  It stages the chunk's template (2048
//             floats) and B's span [k C + L0, k C + L0 + terms + 512 w + slack) in LDS as FLOATS — both detectors are fp32
//             values by definition, and they (and the non-finite rule) are computed while staging; a span index is a signed
//             64-bit frame of B's range, and what lies outside [0, m) is staged as 0 and never read
//   the chains   f0_kernel's turn, COPIED (wbx_f0.hip's instances are untouched; a later change shares one core): a lane owns
//             8 consecutive lags and their 16 fp64 accumulators (pr and pE), a sliding window of 12 span words in registers
//             feeds 4 terms x 8 lags = 64 fma per 16 bytes read, the template's 4 values a wave-uniform broadcast, both reads
//             asked for one turn ahead.  Both factors of every product are fp32 values, so the product is exact in fp64 and
//             fma(t, w, r) IS the model's r + t * w.  A lane's span offset is 8 l words: every read is an aligned 16 bytes
//   the stage    {pr, pE} per (chunk of the band, lag) as one 16-byte store; a lane's lags past lag_max are computed on
//             staged data and never stored
//   the fold     align_fold_kernel, a lane per lag: the band's partials ascending onto the running r, E of the curve buffer —
//             bands continue the same chain — and, after the last band, the score and the workgroup's (greatest score,
//             lowest lag) by comparisons that are exact and free of order
//   the pick     align_pick_kernel, ONE workgroup behind the last fold on the stream: the global pick over the workgroups'
//             best, the refine from the curve, Ea's fold.  align_ref_kernel computes Ea's partials, a workgroup per chunk
// Nothing waits on another workgroup, and there is no scratch.
#include "wbx_ctx.h"

#include <cstring>

namespace wbx {

namespace {

constexpr uint32_t kPer = kAlignPerLane;
static_assert(kPer == 8 && kAlignLanes == 512);
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kFoldLanes = 256;

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double sample_in(float v) { return finite_bits(v) ? (double)v : 0.0; }

// the detector d[g] for a frame g of a range ("Stretching a clip"'s)
template <int CH>
__device__ __forceinline__ float detector(const float* const* src, uint32_t g) {
  if (CH == 1) return finite_bits(src[0][g]) ? src[0][g] : 0.0f;
  return __double2float_rn(__dmul_rn(0.5, __dadd_rn(sample_in(src[0][g]), sample_in(src[1][g]))));
}

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }

struct Chains {
  double r[kPer], E[kPer];     // the two chains of the lane's 8 lags
};
// Turn b: terms 4 b .. 4 b + 3 on the lane's 8 lags.  lo, mid = span words 4 b .. 4 b + 7 of the lane (as doubles); hi
// receives words 4 b + 8 .. 4 b + 11 from nv, tv the template's 4 values from nt, and nv / nt are asked for again, for turn
// b + 1 (the last turn asks for 4 words nobody uses: span and template hold them).  Lag j at term t reads word j + t
__device__ __forceinline__ void turn4(Chains& sc, const double (&lo)[4], const double (&mid)[4], double (&hi)[4], f4& nv, f4& nt,
                                      const float* sp, const float* tp, uint32_t b) {
  const f4 tv = nt;
#pragma unroll
  for (int j = 0; j < 4; j++) hi[j] = (double)nv[j];
  nv = ld4(sp + 4u * (b + 3u));
  nt = ld4(tp + 4u * (b + 1u));
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

template <int CHA, int CHB>
__global__ void __launch_bounds__(kAlignLanes) align_partial_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // align_lds_bytes: the template, then the span
  float* tmpl = lds;
  float* span = lds + kAlignTmplWords;
  const uint32_t tid = threadIdx.x;
  const uint32_t i0 = (a.chunk0 + blockIdx.y) * kAlignChunk;   // the chunk's first term (< n: the grid holds no other)
  const uint32_t terms = a.n - i0 < kAlignChunk ? a.n - i0 : kAlignChunk;   // a multiple of 8
  const uint32_t q0 = blockIdx.x * kAlignBlockLags;            // the block's first lag, counted from lag_min (< lags)
  const uint32_t block_lags = a.lags - q0 < kAlignBlockLags ? a.lags - q0 : kAlignBlockLags;
  const uint32_t waves = (block_lags + kAlignWaveLags - 1u) / kAlignWaveLags;   // that work (<= blockDim.x / 64)
  for (uint32_t s = tid; s < terms + 4u; s += blockDim.x) tmpl[s] = s < terms ? detector<CHA>(a.a, i0 + s) : 0.0f;
  const int64_t g0 = (int64_t)i0 + (int64_t)a.lag_min + (int64_t)q0;   // B's frame of span word 0: may lie in front of B
  const uint32_t words = align_span_words(terms, waves);
  for (uint32_t s = tid; s < words; s += blockDim.x) {
    const int64_t g = g0 + (int64_t)s;
    span[s] = (g >= 0 && g < (int64_t)a.m) ? detector<CHB>(a.b, (uint32_t)g) : 0.0f;
  }
  __syncthreads();
  if ((tid >> 6) >= waves) return;                             // (per wave) no lag of the wave counts
  Chains sc;
#pragma unroll
  for (int j = 0; j < (int)kPer; j++) sc.r[j] = 0.0, sc.E[j] = 0.0;
  const float* tp = tmpl;
  const float* sp = span + tid * kPer;
  // three groups of 4 span words take turns as the window's low, middle and high part, so that nothing is moved; the
  // operands of the next turn (a 16-B span read, a broadcast template read) are asked for ahead of the fma run
  double w0[4], w1[4], w2[4];
  {
    const f4 v0 = ld4(sp), v1 = ld4(sp + 4);
#pragma unroll
    for (int j = 0; j < 4; j++) w0[j] = (double)v0[j], w1[j] = (double)v1[j];
  }
  f4 nv = ld4(sp + 8), nt = ld4(tp);
  const uint32_t turns = terms >> 2;                           // a turn: terms 4 b .. 4 b + 3; even
  uint32_t b = 0;
  for (; b + 3u <= turns; b += 3u) {
    turn4(sc, w0, w1, w2, nv, nt, sp, tp, b);
    turn4(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
    turn4(sc, w2, w0, w1, nv, nt, sp, tp, b + 2u);
  }
  if (b < turns) turn4(sc, w0, w1, w2, nv, nt, sp, tp, b);
  if (b + 1u < turns) turn4(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
  AlignPartial* out = a.stage + (size_t)blockIdx.y * a.lags + q0 + tid * kPer;
#pragma unroll
  for (int j = 0; j < (int)kPer; j++)
    if (tid * kPer + (uint32_t)j < block_lags) out[j] = AlignPartial{sc.r[j], sc.E[j]};   // (a lag past lag_max is never stored)
}

// Ea's partials: a workgroup (one wave) per chunk stages the chunk's template, one lane walks it ascending
template <int CHA>
__global__ void __launch_bounds__(64) align_ref_kernel(AlignArgs a) {
  __shared__ float tmpl[kAlignChunk];
  const uint32_t i0 = blockIdx.x * kAlignChunk;
  const uint32_t terms = a.n - i0 < kAlignChunk ? a.n - i0 : kAlignChunk;
  for (uint32_t s = threadIdx.x; s < terms; s += 64u) tmpl[s] = detector<CHA>(a.a, i0 + s);
  __syncthreads();
  if (threadIdx.x != 0u) return;
  double e = 0.0;
  for (uint32_t s = 0; s < terms; s++) {
    const double d = (double)tmpl[s];
    e = fma(d, d, e);
  }
  a.ea_part[blockIdx.x] = e;
}

__device__ __forceinline__ double score_of(double r, double E, bool either) {
  return E == 0.0 ? 0.0 : __ddiv_rn(__dmul_rn(r, either ? r : fabs(r)), E);
}
// (greatest score, lowest lag): exact, and free of the order it is applied in
__device__ __forceinline__ bool better(double s, uint32_t q, double os, uint32_t oq) { return s > os || (s == os && q < oq); }

template <uint32_t WAVES>
__device__ __forceinline__ void reduce_best(double& s, uint32_t& q, double* red_s, uint32_t* red_q) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(s, off);
    const uint32_t oq = (uint32_t)__shfl_xor((int)q, off);
    if (better(os, oq, s, q)) s = os, q = oq;
  }
  if ((threadIdx.x & 63u) == 0u) red_s[threadIdx.x >> 6] = s, red_q[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0u)
    for (uint32_t v = 1; v < WAVES; v++)
      if (better(red_s[v], red_q[v], s, q)) s = red_s[v], q = red_q[v];
}

__global__ void __launch_bounds__(kFoldLanes) align_fold_kernel(AlignArgs a) {
  __shared__ double red_s[kFoldLanes / 64u];
  __shared__ uint32_t red_q[kFoldLanes / 64u];
  const uint32_t q = blockIdx.x * kFoldLanes + threadIdx.x;
  const bool live = q < a.lags;
  double r = 0.0, E = 0.0;
  if (live) {
    if (a.chunk0 != 0u) r = a.curve[q].r, E = a.curve[q].energy;
    const AlignPartial* p = a.stage + q;
    for (uint32_t k = a.chunk0; k < a.chunk1; k++, p += a.lags) {
      const AlignPartial v = *p;
      r = __dadd_rn(r, v.pr);
      E = __dadd_rn(E, v.pE);
    }
    a.curve[q] = wbx_align_point{r, E};
  }
  if (a.chunk1 != a.chunks) return;                            // (the same in every lane) a later band goes on
  double s = live ? score_of(r, E, a.either != 0u) : -__builtin_huge_val();
  uint32_t bq = live ? q : kNone;
  reduce_best<kFoldLanes / 64u>(s, bq, red_s, red_q);
  if (threadIdx.x == 0u) a.best[blockIdx.x] = AlignBest{s, bq, 0u};   // (lane 0 is live: the grid holds no empty workgroup)
}

__global__ void __launch_bounds__(kFoldLanes) align_pick_kernel(AlignArgs a) {
  __shared__ double red_s[kFoldLanes / 64u];
  __shared__ uint32_t red_q[kFoldLanes / 64u];
  __shared__ double ea_sh;
  const uint32_t groups = (a.lags + kFoldLanes - 1u) / kFoldLanes;
  double s = -__builtin_huge_val();
  uint32_t q = kNone;
  for (uint32_t i = threadIdx.x; i < groups; i += kFoldLanes) {
    const AlignBest v = a.best[i];
    if (better(v.score, v.q, s, q)) s = v.score, q = v.q;
  }
  if (threadIdx.x == 64u) {                                    // Ea's fold, beside the first wave's work
    double e = 0.0;
    for (uint32_t k = 0; k < a.chunks; k++) e = __dadd_rn(e, a.ea_part[k]);
    ea_sh = e;
  }
  reduce_best<kFoldLanes / 64u>(s, q, red_s, red_q);           // (its barrier also publishes ea_sh)
  if (threadIdx.x != 0u) return;
  const bool either = a.either != 0u;
  const wbx_align_point at = a.curve[q];
  double off = 0.0;
  if (q >= 1u && q + 1u < a.lags) {
    const wbx_align_point lo = a.curve[q - 1u], hi = a.curve[q + 1u];
    const double ca = score_of(lo.r, lo.energy, either), cg = score_of(hi.r, hi.energy, either);
    const double den = __dsub_rn(__dmul_rn(2.0, s), __dadd_rn(ca, cg));
    off = (den > 0.0 && s >= ca && s >= cg) ? __ddiv_rn(__dmul_rn(0.5, __dsub_rn(cg, ca)), den) : 0.0;
  }
  const double Ea = ea_sh;
  AlignPick rec;
  rec.offset = off;
  rec.score = s;
  rec.r = at.r;
  rec.energy = at.energy;
  rec.ref_energy = Ea;
  rec.confidence = Ea == 0.0 ? 0.0 : __ddiv_rn(s, Ea);
  rec.q = q;
  rec.inverted = at.r < 0.0 ? 1u : 0u;
  *a.pick = rec;
}

}  // namespace

void launch_align_ref(const AlignArgs& a, hipStream_t s) {
  if (a.cha == 2u) hipLaunchKernelGGL((align_ref_kernel<2>), dim3(a.chunks), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((align_ref_kernel<1>), dim3(a.chunks), dim3(64), 0, s, a);
}
void launch_align_partial(const AlignArgs& a, hipStream_t s) {
  const dim3 grid((a.lags + kAlignBlockLags - 1u) / kAlignBlockLags, a.chunk1 - a.chunk0), block(64u * a.waves);
  const uint32_t lds = align_lds_bytes(a.waves);
  if (a.cha == 2u) {
    if (a.chb == 2u) hipLaunchKernelGGL((align_partial_kernel<2, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((align_partial_kernel<2, 1>), grid, block, lds, s, a);
  } else {
    if (a.chb == 2u) hipLaunchKernelGGL((align_partial_kernel<1, 2>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((align_partial_kernel<1, 1>), grid, block, lds, s, a);
  }
}
void launch_align_fold(const AlignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(align_fold_kernel, dim3((a.lags + kFoldLanes - 1u) / kFoldLanes), dim3(kFoldLanes), 0, s, a);
}
void launch_align_pick(const AlignArgs& a, hipStream_t s) { hipLaunchKernelGGL(align_pick_kernel, dim3(1), dim3(kFoldLanes), 0, s, a); }

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// Whether the clips exist, then the arithmetic of the call — it needs no clip of that size to be refused — then the clips
wbx_status align_check_call(const ClipSrc* ref, uint32_t ref_rate, const ClipSrc* src, uint32_t src_rate, const AlignCall& k, const char** why) {
  if (!ref) return *why = "clip align: unknown reference clip", WBX_ERR_INVALID;
  if (!src) return *why = "clip align: unknown clip", WBX_ERR_INVALID;
  const wbx_status st = align_check(k, why);
  if (st != WBX_OK) return st;
  if (ref->format != (uint32_t)WBX_FMT_F32) return *why = "clip align: the reference clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (ref->channels < 1 || ref->channels > 2) return *why = "clip align: reference clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (src->format != (uint32_t)WBX_FMT_F32) return *why = "clip align: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src->channels < 1 || src->channels > 2) return *why = "clip align: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (ref_rate != src_rate) return *why = "clip align: the clips' sample rates differ", WBX_ERR_UNSUPPORTED;
  if (k.a_first > ref->frames || k.n > ref->frames - k.a_first)
    return *why = "clip align: the reference's range ends past the clip", WBX_ERR_INVALID;
  if (k.b_first > src->frames || k.m > src->frames - k.b_first) return *why = "clip align: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

wbx_status align_run(wbx_ctx* c, const ClipSrc& ref, const ClipSrc& src, const AlignCall& k, wbx_align_info* info, wbx_align_point* curve_out,
                     std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  AlignStage& z = c->aln;
  const uint32_t lags = (uint32_t)(k.lag_max - k.lag_min + 1);
  const uint32_t chunks = align_chunks(k.n), per_band = align_band_chunks(lags);
  const AlignShape shape = align_shape(lags);
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  if (e == hipSuccess) e = z.d_part.ensure((size_t)(chunks < per_band ? chunks : per_band) * lags);
  if (e == hipSuccess) e = z.d_curve.ensure(lags);
  if (e == hipSuccess && curve_out) e = z.h_curve.ensure(lags);
  if (e == hipSuccess) e = z.d_best.ensure((lags + kFoldLanes - 1u) / kFoldLanes);
  if (e == hipSuccess) e = z.d_ea.ensure(chunks);
  if (e == hipSuccess) e = z.d_pick.ensure(1);
  if (e == hipSuccess) e = z.h_pick.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  AlignArgs a{};
  a.a[0] = clip_row(ref, 0) + k.a_first, a.a[1] = clip_row(ref, 1) + k.a_first;
  a.b[0] = clip_row(src, 0) + k.b_first, a.b[1] = clip_row(src, 1) + k.b_first;
  a.stage = z.d_part.p, a.curve = z.d_curve.p, a.best = z.d_best.p, a.ea_part = z.d_ea.p, a.pick = z.d_pick.p;
  a.n = (uint32_t)k.n, a.m = (uint32_t)k.m;
  a.lag_min = (int32_t)k.lag_min;
  a.lags = lags, a.chunks = chunks;
  a.waves = shape.waves;
  a.cha = ref.channels, a.chb = src.channels;
  a.either = (k.flags & WBX_ALIGN_EITHER_POLARITY) ? 1u : 0u;
  uint32_t launches = 0;
  if (e == hipSuccess) {
    launch_align_ref(a, on);
    e = hipGetLastError();
    launches++;
  }
  for (uint32_t k0 = 0; k0 < chunks && e == hipSuccess; k0 += per_band) {
    a.chunk0 = k0;
    a.chunk1 = k0 + per_band < chunks ? k0 + per_band : chunks;
    launch_align_partial(a, on);
    e = hipGetLastError();
    if (e == hipSuccess) {
      launch_align_fold(a, on);
      e = hipGetLastError();
    }
    launches += 2;
  }
  if (e == hipSuccess) {
    launch_align_pick(a, on);
    e = hipGetLastError();
    launches++;
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_pick.p, z.d_pick.p, sizeof(AlignPick), hipMemcpyDeviceToHost, on);
  if (e == hipSuccess && curve_out)
    e = hipMemcpyAsync(z.h_curve.p, z.d_curve.p, (size_t)lags * sizeof(wbx_align_point), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still read the clips)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) return stage_fail(why, WBX_ERR_DEVICE, "clip align", e);
  z.timed = true;
  if (curve_out) std::memcpy(curve_out, z.h_curve.p, (size_t)lags * sizeof(wbx_align_point));
  if (info) {
    const AlignPick& p = *z.h_pick.p;
    info->lag = (int32_t)(k.lag_min + (int64_t)p.q);
    info->inverted = p.inverted;
    info->offset = p.offset;
    info->score = p.score;
    info->r = p.r;
    info->energy = p.energy;
    info->ref_energy = p.ref_energy;
    info->confidence = p.confidence;
    info->lags = lags;
    info->chunks = chunks;
    info->terms = (uint64_t)lags * k.n;
    info->launches = launches;
    info->_pad = 0;
  }
  return WBX_OK;
}

}  // namespace wbx

extern "C" wbx_status wbx_align_check(uint64_t n_frames, uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags, int has_info,
                                      int has_curve_out, size_t curve_cap) {
  const wbx::AlignCall k{0, n_frames, 0, m_frames, lag_min, lag_max, flags, has_info != 0, has_curve_out != 0, curve_cap};
  const char* msg = "";
  return wbx::align_check(k, &msg);
}
extern "C" uint32_t wbx_align_chunks(uint64_t n_frames) { return wbx::align_chunks(n_frames); }
extern "C" uint64_t wbx_align_max_lags(void) { return wbx::kAlignMaxLags; }
extern "C" uint32_t wbx_align_chunk_frames(void) { return wbx::kAlignChunk; }
extern "C" uint32_t wbx_align_band_chunks(uint64_t lags) { return wbx::align_band_chunks(lags); }
extern "C" uint32_t wbx_align_launches(uint64_t n_frames, uint64_t lags) { return wbx::align_launches(n_frames, lags); }

extern "C" wbx_status wbx_align_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::aln, "align time: no align call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_align(wbx_ctx* c, uint32_t ref_clip, uint64_t a_first, uint64_t n_frames, uint32_t clip, uint64_t b_first,
                                     uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags, wbx_align_info* info,
                                     wbx_align_point* curve_out, size_t curve_cap) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* ra = find_clip(c, ref_clip);
  const ClipSlot* rb = find_clip(c, clip);
  ClipSrc ref{}, src{};
  if (ra) ref = clip_src(*ra);
  if (rb) src = clip_src(*rb);
  const AlignCall k{a_first, n_frames, b_first, m_frames, lag_min, lag_max, flags, info != nullptr, curve_out != nullptr, curve_cap};
  const char* msg = "";
  const wbx_status st = align_check_call(ra ? &ref : nullptr, ra ? ra->d.sample_rate : 0u, rb ? &src : nullptr, rb ? rb->d.sample_rate : 0u, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return align_run(c, ref, src, k, info, curve_out, why); });
}
