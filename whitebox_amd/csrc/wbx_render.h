// wbx_render.h — the exact general row renderer: one source sample of Sampler::stream (sample_at) and a lane's four frames
// of a track's mixing buffer over any number of stream calls (render_generic).  Shared by the pre-render pass (gen_kernel,
// wbx_kernels.hip) and the stem kernel (wbx_bounce.hip): both produce the values mix_body holds in registers, bit for bit.
// Parity-critical arithmetic uses the explicitly rounded intrinsics; every file that includes this is built with
// -ffp-contract=off.
#pragma once
#include "wbx_mix.h"
#include "wbx_seq.h"

namespace wbx {

// ------------------------------------------------------------------------------------------------
// per-sample rendering helpers
// ------------------------------------------------------------------------------------------------

// One source sample of Sampler::stream for destination frame jj of segment sg, channel c:
// unity path sampler.cpp:106-158, linear path sampler.cpp:34-59 (normalisers :7-18 and :95-97).
__device__ __forceinline__ float sample_at(const DSeg& sg, uint32_t c, uint32_t jj) {
  const void* base = c ? sg.src[1] : sg.src[0];   // (no dynamic index: keeps the descriptor in registers)
  const float WBX_GLOBAL* bf = as_global<float>(base);
  const int16_t WBX_GLOBAL* b16 = as_global<int16_t>(base);
  const int32_t WBX_GLOBAL* b32 = as_global<int32_t>(base);
  if (sg.speed == 1.0) {
    const uint32_t idx = u32_of_double_x86(sg.pos) + jj;                 // :107 (the low word, as x86-64 converts)
    switch (sg.format) {
      case FMT_F32: return bf[idx];
      case FMT_I16: {
        const float norm = 1.0f / 32767.0f;                              // :95
        return clampf(__fmul_rn((float)b16[idx], norm), -1.0f, 1.0f);
      }
      case FMT_I24: {
        const double norm = 1.0 / 8388607.0;                             // :96
        return (float)clampd(__dmul_rn((double)b32[idx], norm), -1.0, 1.0);
      }
      default: {
        const double norm = 1.0 / 2147483647.0;                          // :97
        return (float)clampd(__dmul_rn((double)b32[idx], norm), -1.0, 1.0);
      }
    }
  }
  const double x = __dadd_rn(sg.pos, __dmul_rn((double)(int32_t)jj, sg.speed));   // :50
  const long long ix = (long long)x;                                               // :51
  const float fx = (float)__dsub_rn(x, (double)ix);                                // :52 (negative for x < 0: ix truncates)
  // Q12: a NEGATIVE playback speed (calc_resize_clip's stretch, clip_edit.h:59-67,110-118) runs the position
  // below zero; the reference then reads the heap in front of the channel array (sampler.cpp:53-54, undefined).  A tap at
  // a negative index reads 0 — never memory in front of the clip.
  const bool ta = ix >= 0, tb = ix >= -1;
  float a, b;
  switch (sg.format) {
    case FMT_F32:
      a = ta ? bf[ix] : 0.0f;
      b = tb ? bf[ix + 1] : 0.0f;
      break;
    case FMT_I16: {
      const float norm = (float)(1.0 / 32767.0);                                   // :9-10
      a = __fmul_rn(norm, (float)(ta ? b16[ix] : (int16_t)0));
      b = __fmul_rn(norm, (float)(tb ? b16[ix + 1] : (int16_t)0));
      break;
    }
    case FMT_I24: {
      const double norm = 1.0 / 8388607.0;                                         // :11-12
      a = (float)__dmul_rn(norm, (double)(ta ? b32[ix] : 0));
      b = (float)__dmul_rn(norm, (double)(tb ? b32[ix + 1] : 0));
      break;
    }
    default: {
      const double norm = 1.0 / 2147483647.0;                                      // :13-14
      a = (float)__dmul_rn(norm, (double)(ta ? b32[ix] : 0));
      b = (float)__dmul_rn(norm, (double)(tb ? b32[ix + 1] : 0));
      break;
    }
  }
  return __fadd_rn(a, __fmul_rn(fx, __fsub_rn(b, a)));                             // :55
}

// Generic track-block: any number of segments, any coverage, any format.  Returns the track's
// mixing-buffer value for frame j of channel c BEFORE the track gain (the buffer the reference clears
// at engine.cpp:1602 and Sampler::stream accumulates into, sampler.cpp:56,152).
// One lane's 4 frames of a generic track-block: the mixing-buffer values BEFORE the track gain.
__device__ __forceinline__ f4 render_generic(const DTrackBlock& tb, const DSeg* pool, uint32_t c, uint32_t j0) {
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t nseg = tb.nseg;
  for (uint32_t s = 0; s < nseg; s++) {
    const DSeg sg = (s == 0) ? get_seg0(tb) : pool[(size_t)tb.extra * kChunk + (s - 1)];
    const uint32_t d0 = sg.dst_start, n = sg.len;
    if (j0 + 4u <= d0 || j0 >= d0 + n) continue;   // none of the lane's frames lies in this segment
    // fp32 segments whose source positions stay below 2^31 (all but multi-hour clips): 32-bit index math, and one
    // 16-B load for a lane whose four frames all lie inside a unity-speed segment
    // (and a speed above zero: a negative one runs the position below zero, where `fract` is not x - trunc(x) and the
    //  taps in front of the clip read 0 — sample_at, Q12)
    const bool small = sg.pos >= 0.0 && sg.speed > 0.0 && sg.pos + (double)n * (sg.speed > 1.0 ? sg.speed : 1.0) < 2147483000.0;
    if (sg.format == FMT_F32 && small) {
      const float WBX_GLOBAL* bf = as_global<float>(c ? sg.src[1] : sg.src[0]);
      if (sg.speed == 1.0) {
        const uint32_t base = (uint32_t)sg.pos;                                            // sampler.cpp:107
        if (j0 >= d0 && j0 + 4u <= d0 + n) {
          const f4u v = *reinterpret_cast<const f4u WBX_GLOBAL*>(bf + base + (j0 - d0));
          acc[0] = __fadd_rn(acc[0], __fmul_rn(v.x, sg.gain));                             // :151-152
          acc[1] = __fadd_rn(acc[1], __fmul_rn(v.y, sg.gain));
          acc[2] = __fadd_rn(acc[2], __fmul_rn(v.z, sg.gain));
          acc[3] = __fadd_rn(acc[3], __fmul_rn(v.w, sg.gain));
        } else {
#pragma unroll
          for (uint32_t e = 0; e < 4; e++) {
            const uint32_t j = j0 + e;
            if (j >= d0 && j < d0 + n) acc[e] = __fadd_rn(acc[e], __fmul_rn(bf[base + (j - d0)], sg.gain));
          }
        }
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; e++) {
          const uint32_t j = j0 + e;
          if (j >= d0 && j < d0 + n) {
            const double x = __dadd_rn(sg.pos, __dmul_rn((double)(int32_t)(j - d0), sg.speed));   // :50
            const int ix = (int)x;                                                                // :51
            const float fx = (float)__builtin_amdgcn_fract(x);                                    // :52 (x >= 0: exact)
            const float a = bf[ix], b = bf[ix + 1];
            acc[e] = __fadd_rn(acc[e], __fmul_rn(__fadd_rn(a, __fmul_rn(fx, __fsub_rn(b, a))), sg.gain));   // :55-56
          }
        }
      }
      continue;
    }
#pragma unroll
    for (uint32_t e = 0; e < 4; e++) {
      const uint32_t j = j0 + e;
      if (j >= d0 && j < d0 + n) acc[e] = __fadd_rn(acc[e], __fmul_rn(sample_at(sg, c, j - d0), sg.gain));
    }
  }
  return f4{acc[0], acc[1], acc[2], acc[3]};
}

}  // namespace wbx
