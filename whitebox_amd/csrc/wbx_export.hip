// wbx_export.hip — export_kernel: a frame range of a resident planar F32 clip -> interleaved samples of a device format.
//
// The way out for takes (wbx_engine_stop_record) and bounces (wbx_engine_bounce): both end as planar fp32 pool clips, and
// a file wants [frames][channels] samples of its own sample format.  The conversion is the master's
// (core/audio_format_conv.cpp:5-91 through to_i16 / to_i24 / to_i32 of wbx_sum.h: __fmul_rn, asymmetric scales, the x86
// truncation with its 0x80000000 results), optionally behind the compare-clamp of engine.cpp:1627-1636
// (x > 1 ? 1 : (x < -1 ? -1 : x): NaN passes), and the same pass takes per channel, of the SOURCE values, the peak
// (max |x| by `a > peak`: a NaN never raises it), the number of samples beyond +-1 and the number of NaNs — all three
// independent of the order they are reduced in, hence exact.
//
// Layout: sample i, channel c at index i*C + c in every format — WBX_OUT_I24 included, byte k of to_i24(x) at
// (i*C + c)*3 + k.  (wbx_fetch_interleaved's WBX_OUT_I24 mirrors the reference writer, whose index ignores the channel:
// right for parity of the callback, no use for a file, which needs every channel.)
//
// One lane owns 8 consecutive frames of every channel: 16 B (mono 16-bit) to 64 B (stereo 32-bit) of output, stored as
// whole 16-B words — stereo packed 24-bit is 48 B per lane, three words; only mono packed 24-bit (24 B per lane, 8-B
// aligned) goes out as three 8-B words.  The source is read once, with nontemporal 16-B loads whose type promises 4-byte
// alignment only (the range starts at any frame).  A lane whose 8 frames reach past the range reads on into what follows
// it in the row (at most 7 frames: the clip's 16 zero frames of padding cover the end of the clip) and stores, sample by
// sample, only the frames inside the range.  No LDS, no scratch: statistics are reduced in registers, across the wave by
// lane shuffles, and across workgroups by one atomic per wave and non-zero value (integer max on the bit pattern of the
// non-negative peak, integer adds).
#include "wbx_ctx.h"
#include "wbx_sum.h"

namespace wbx {

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at a 4-byte aligned address
typedef uint32_t u4v __attribute__((ext_vector_type(4)));            // a 16-B / an 8-B word of output
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float export_clamp(float x) { return x > 1.0f ? 1.0f : (x < -1.0f ? -1.0f : x); }   // engine.cpp:1627-1636

template <int FMT>
__device__ __forceinline__ uint32_t export_word(float v) {   // one sample as the low bytes of a word
  if constexpr (FMT == WBX_OUT_I16) return (uint32_t)(uint16_t)(int16_t)to_i16(v);
  else if constexpr (FMT == WBX_OUT_I24 || FMT == WBX_OUT_I24_X8) return (uint32_t)(to_i24(v) & 0xFFFFFF);
  else if constexpr (FMT == WBX_OUT_I32) return (uint32_t)to_i32(v);
  else return __float_as_uint(v);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}

template <int C, int FMT>
__global__ void __launch_bounds__(256) export_kernel(ExportArgs a) {
  constexpr int S = 8 * C;                                   // samples of a lane
  constexpr int BPS = FMT == WBX_OUT_I16 ? 2 : FMT == WBX_OUT_I24 ? 3 : 4;
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  const uint32_t j0 = slot * 8u;                             // the lane's first frame (n_frames <= 2^24: no overflow)
  uint32_t peak[C], over[C], nans[C];
#pragma unroll
  for (int c = 0; c < C; c++) peak[c] = over[c] = nans[c] = 0u;

  if (j0 < a.n_frames) {
    const uint32_t left = a.n_frames - j0;
    const bool clamp = (a.flags & WBX_EXPORT_CLAMP) != 0u;
    uint32_t w[S];                                           // the lane's samples in output order, one per word
#pragma unroll
    for (int c = 0; c < C; c++) {
      const float* p = a.src[c] + j0;
      const f4u lo = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p));
      const f4u hi = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + 4));
      const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      float pk = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const bool in = (uint32_t)i < left;                  // frames past the range count for nothing
        const float v = x[i], av = fabsf(v);
        if (in && av > pk) pk = av;
        over[c] += (in && (v > 1.0f || v < -1.0f)) ? 1u : 0u;
        nans[c] += (in && v != v) ? 1u : 0u;
        w[i * C + c] = export_word<FMT>(clamp ? export_clamp(v) : v);
      }
      peak[c] = __float_as_uint(pk);
    }

    char* out = (char*)a.dst + (size_t)j0 * (C * BPS);
    if (left >= 8u) {
      if constexpr (FMT == WBX_OUT_I16) {
        uint32_t q[S / 2];
#pragma unroll
        for (int k = 0; k < S / 2; k++) q[k] = w[2 * k] | (w[2 * k + 1] << 16);
#pragma unroll
        for (int k = 0; k < S / 8; k++)
          __builtin_nontemporal_store(u4v{q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]}, reinterpret_cast<u4v*>(out) + k);
      } else if constexpr (FMT == WBX_OUT_I24) {
        uint32_t q[3 * S / 4];                               // S samples of 24 bits, back to back, little-endian
#pragma unroll
        for (int k = 0; k < 3 * S / 4; k++) q[k] = 0u;
#pragma unroll
        for (int s = 0; s < S; s++) {
          const int bit = 24 * s, k = bit / 32, sh = bit % 32;
          q[k] |= w[s] << sh;
          if (sh > 8) q[k + 1] |= w[s] >> (32 - sh);
        }
        if constexpr (C == 2) {
#pragma unroll
          for (int k = 0; k < 3; k++)
            __builtin_nontemporal_store(u4v{q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]}, reinterpret_cast<u4v*>(out) + k);
        } else {                                             // 24 B per lane: 8-byte aligned
#pragma unroll
          for (int k = 0; k < 3; k++) __builtin_nontemporal_store(u2v{q[2 * k], q[2 * k + 1]}, reinterpret_cast<u2v*>(out) + k);
        }
      } else {
#pragma unroll
        for (int k = 0; k < S / 4; k++)
          __builtin_nontemporal_store(u4v{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]}, reinterpret_cast<u4v*>(out) + k);
      }
    } else {                                                 // the range's last lane: only the frames inside it
#pragma unroll
      for (int s = 0; s < S; s++) {
        if ((uint32_t)(s / C) >= left) continue;
        if constexpr (FMT == WBX_OUT_I16) {
          reinterpret_cast<uint16_t*>(out)[s] = (uint16_t)w[s];
        } else if constexpr (FMT == WBX_OUT_I24) {
          out[3 * s + 0] = (char)(w[s] & 0xFFu);
          out[3 * s + 1] = (char)((w[s] >> 8) & 0xFFu);
          out[3 * s + 2] = (char)((w[s] >> 16) & 0xFFu);
        } else {
          reinterpret_cast<uint32_t*>(out)[s] = w[s];
        }
      }
    }
  }

  // statistics: registers -> wave -> one atomic per wave and value that is not zero
  const bool first = (threadIdx.x & 63u) == 0u;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const uint32_t p = wave_max_u32(peak[c]), o = wave_add_u32(over[c]), n = wave_add_u32(nans[c]);
    if (first) {
      if (p) atomicMax(a.stats + c, p);
      if (o) atomicAdd(a.stats + 2 + c, o);
      if (n) atomicAdd(a.stats + 4 + c, n);
    }
  }
}

template <int C>
void launch_export_c(const ExportArgs& a, dim3 grid, hipStream_t s) {
  switch (a.format) {
    case WBX_OUT_I16: hipLaunchKernelGGL((export_kernel<C, WBX_OUT_I16>), grid, dim3(256), 0, s, a); break;
    case WBX_OUT_I24: hipLaunchKernelGGL((export_kernel<C, WBX_OUT_I24>), grid, dim3(256), 0, s, a); break;
    case WBX_OUT_I24_X8: hipLaunchKernelGGL((export_kernel<C, WBX_OUT_I24_X8>), grid, dim3(256), 0, s, a); break;
    case WBX_OUT_I32: hipLaunchKernelGGL((export_kernel<C, WBX_OUT_I32>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((export_kernel<C, WBX_OUT_F32>), grid, dim3(256), 0, s, a); break;
  }
}

}  // namespace

void launch_export(const ExportArgs& a, hipStream_t s) {
  const dim3 grid((a.n_frames + 2047u) / 2048u);             // 256 lanes of 8 frames
  if (a.channels == 2u) launch_export_c<2>(a, grid, s);
  else launch_export_c<1>(a, grid, s);
}

}  // namespace wbx
