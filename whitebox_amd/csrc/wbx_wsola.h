// wbx_wsola.h — the searched step of a WSOLA chain (wbx.h "Stretching a clip"), shared by stretch_search_kernel
// (wbx_stretch.hip) and warp_search_kernel (wbx_warp.hip): the detector, the score chains of a lane's 8 candidates, the
// staging of template and span, the passes and the cross-lane arg-max.  Device code only; one 512-lane workgroup calls
// wsola_search with arguments that are the same in every lane.
//   staging      the template (Hs detector values from c on) and the candidates' span (Hs + hi - lo values from lo on) go
//             to LDS as FLOATS — the detector is an fp32 value by definition; what lies outside [0, n) is staged as 0 and
//             never read — with the detector (and the non-finite rule) computed while staging
//   the chains   each lane owns 8 CONSECUTIVE candidates and holds their 16 fp64 accumulators (s and E) in registers across
//             the Hs terms; a sliding window of 12 span words in registers (three groups of 4 taking turns as its low,
//             middle and high part, so nothing is moved) feeds 4 terms x 8 candidates = 64 fma per 16-B LDS read, the 4
//             template values of a turn come from one wave-uniform (broadcast) read, and both reads are asked for one turn
//             ahead of the fma run that uses them.  Both factors of every product are fp32 values, so the product is exact
//             in fp64 and fma(t, w, s) IS the model's s + t * w
//   the arg-max  no sum crosses lanes; only the arg-max does, compared as (score, -q): exact and free of order.  More than
//             4096 candidates take a second and a third pass over the same staged span
#pragma once
#include <hip/hip_runtime.h>

#include "wbx_stretch.h"

namespace wbx {
namespace wsola {

constexpr uint32_t kLanes = kStretchLanes, kPer = kStretchPerLane, kWaves = kLanes / 64u;
constexpr uint32_t kMaxHs = kStretchMaxWindow / 2u;
constexpr uint32_t kSpanWords = kMaxHs + 2u * kStretchMaxTolerance + 16u;   // Hs + hi - lo values, and what the last lanes ask for
static_assert(kPer == 8 && kLanes % 64u == 0u && kMaxHs % 4u == 0u);
typedef float f4 __attribute__((ext_vector_type(4)));

// what a search workgroup keeps in LDS: 65 712 bytes
struct Lds {
  __attribute__((aligned(16))) float tmpl[kMaxHs + 4u];
  __attribute__((aligned(16))) float span[kSpanWords];
  double red_score[kWaves];
  int32_t red_q[kWaves];
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double sample_in(float v) { return finite_bits(v) ? (double)v : 0.0; }

// the detector d[g] for a frame g of the range, g < n (mono: s1 unused)
template <int CH>
__device__ __forceinline__ float detector(const float* s0, const float* s1, uint32_t g) {
  if (CH == 1) return finite_bits(s0[g]) ? s0[g] : 0.0f;
  return __double2float_rn(__dmul_rn(0.5, __dadd_rn(sample_in(s0[g]), sample_in(s1[g]))));
}

struct Best {
  double score;
  int32_t q;
};
__device__ __forceinline__ bool better(double s, int32_t q, const Best& b) { return s > b.score || (s == b.score && q < b.q); }

struct Scores {
  double s[kPer], E[kPer];     // the two chains of the lane's 8 candidates
};
// Turn b: terms 4 b .. 4 b + 3 on the lane's 8 candidates.  lo, mid = span words 4 b .. 4 b + 7 of the lane (as doubles);
// hi receives words 4 b + 8 .. 4 b + 11 from nv, tv the template's 4 values from nt, and nv / nt are asked for again, for
// turn b + 1 (the call's last turn asks for 4 words nobody uses: both arrays hold them).  Candidate j at term t reads word j + t
__device__ __forceinline__ void turn4(Scores& sc, const double (&lo)[4], const double (&mid)[4], double (&hi)[4], f4& nv, f4& nt,
                                      const f4* sp, const f4* tp, uint32_t b) {
  const f4 tv = nt;
#pragma unroll
  for (int j = 0; j < 4; j++) hi[j] = (double)nv[j];
  nv = sp[b + 3u];
  nt = tp[b + 1u];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const double td = (double)tv[t];
#pragma unroll
    for (int j = 0; j < (int)kPer; j++) {
      const int q = j + t;
      const double w = q < 4 ? lo[q] : q < 8 ? mid[q - 4] : hi[q - 8];
      sc.s[j] = fma(td, w, sc.s[j]);
      sc.E[j] = fma(w, w, sc.E[j]);
    }
  }
}

// The position of a step that searches: the candidate of [lo, lo + ncand), ncand >= 2, with the greatest score against the
// template d[c + .], the lowest among equals.  Called by all 512 lanes of the workgroup with the same arguments; two
// barriers inside, and every lane is done with the LDS block when it returns
template <int CH>
__device__ __forceinline__ int64_t wsola_search(Lds& l, const float* s0, const float* s1, int64_t n,
                                                uint32_t Hs, int64_t c, int64_t lo, uint32_t ncand, uint32_t tid) {
  // staged: template words [0, Hs), span words [0, Hs + ncand - 1) and up to 23 more that only a lane's unused candidates
  // and its last turn's look ahead read (a lane reads up to word ncand - 1 + Hs + 11; at most kSpanWords are staged)
  for (uint32_t s = tid; s < Hs; s += kLanes) {
    const int64_t g = c + (int64_t)s;
    l.tmpl[s] = g < n ? detector<CH>(s0, s1, (uint32_t)g) : 0.0f;
  }
  const uint32_t words = ((Hs + ncand - 1u + 7u) & ~7u) + 16u;
  for (uint32_t s = tid; s < words; s += kLanes) {
    const int64_t g = lo + (int64_t)s;
    l.span[s] = g < n ? detector<CH>(s0, s1, (uint32_t)g) : 0.0f;
  }
  __syncthreads();
  Best mine{-__builtin_huge_val(), 0x7FFFFFFF};
  for (uint32_t base = 0; base < ncand; base += kLanes * kPer) {
    const uint32_t cb = base + tid * kPer;                 // the lane's first candidate of this pass
    if (cb >= ncand) continue;
    Scores sc;
#pragma unroll
    for (int j = 0; j < (int)kPer; j++) sc.s[j] = 0.0, sc.E[j] = 0.0;
    const f4* sp = reinterpret_cast<const f4*>(l.span + cb);
    const f4* tp = reinterpret_cast<const f4*>(l.tmpl);
    // three groups of 4 span words take turns as the window's low, middle and high part, so that nothing is moved;
    // the operands of the next turn (a 16-B span read, a broadcast template read) are asked for ahead of the fma run
    double w0[4], w1[4], w2[4];
    {
      const f4 v0 = sp[0], v1 = sp[1];
#pragma unroll
      for (int j = 0; j < 4; j++) w0[j] = (double)v0[j], w1[j] = (double)v1[j];
    }
    f4 nv = sp[2], nt = tp[0];
    const uint32_t turns = Hs >> 2;                        // a turn: terms 4 b .. 4 b + 3
    uint32_t b = 0;
    for (; b + 3u <= turns; b += 3u) {
      turn4(sc, w0, w1, w2, nv, nt, sp, tp, b);
      turn4(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
      turn4(sc, w2, w0, w1, nv, nt, sp, tp, b + 2u);
    }
    if (b < turns) turn4(sc, w0, w1, w2, nv, nt, sp, tp, b);
    if (b + 1u < turns) turn4(sc, w1, w2, w0, nv, nt, sp, tp, b + 1u);
    const double(&s)[kPer] = sc.s;
    const double(&E)[kPer] = sc.E;
#pragma unroll
    for (int j = 0; j < (int)kPer; j++) {
      if (cb + (uint32_t)j < ncand) {
        const double score = E[j] == 0.0 ? 0.0 : __ddiv_rn(__dmul_rn(s[j], fabs(s[j])), E[j]);
        const int32_t q = (int32_t)(lo + (int64_t)(cb + (uint32_t)j));
        if (better(score, q, mine)) mine.score = score, mine.q = q;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double os = __shfl_xor(mine.score, off);
    const int32_t oq = __shfl_xor(mine.q, off);
    if (better(os, oq, mine)) mine.score = os, mine.q = oq;
  }
  if ((tid & 63u) == 0u) l.red_score[tid >> 6] = mine.score, l.red_q[tid >> 6] = mine.q;
  __syncthreads();                                         // (also: every lane is done with tmpl and span)
  Best all{l.red_score[0], l.red_q[0]};
#pragma unroll
  for (int v = 1; v < (int)kWaves; v++)
    if (better(l.red_score[v], l.red_q[v], all)) all.score = l.red_score[v], all.q = l.red_q[v];
  return (int64_t)__builtin_amdgcn_readfirstlane(all.q);
}

}  // namespace wsola
}  // namespace wbx
