// wbx_convolve.hip — convolve_taps_kernel and convolve_kernel: a frame range of a resident planar F32 clip convolved with a
// frame range of another (the impulse response) into a new planar F32 clip (wbx.h "Convolving a clip"), and layer 1's calls
// on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/convolve_model.py: per output frame
// L fp64 multiply-adds in ascending tap order from +0.0, one multiplication by the gain, one rounding to fp32, a NaN stored
// as 0x7FC00000.  The product of two fp32 values is exact in fp64, so the explicit fp64 fma below is bit-equal to the
// model's multiply-then-add; only the order of the additions counts, and it is one chain per output frame here.
//
// convolve_taps_kernel: the response's range becomes doubles once per call, [ir_channels][l_pad], what is not finite as
// 0.0, zero from L up to l_pad (L rounded up to 16).  A padded tap adds 0 * x = +-0 to an accumulator that started at +0.0
// and can never be -0.0: it changes nothing, so the tap loop needs no tail.
//
// convolve_kernel<CS, CI>: a workgroup of 256 lanes owns a TILE of 2048 consecutive output frames, a lane 8 consecutive
// frames of every output channel (max(CS, CI) of them): 8 or 16 fp64 accumulators that live in registers for the whole tap
// loop.  The response is walked in SEGMENTS of P = 2048 taps.  Per segment:
//   stage    the tile's frames m0 .. m0 + 2047 and the taps k0 .. k0 + P - 1 read source frames m0 - k0 - P + 1 ..
//            m0 - k0 + 2047: 4095 floats per source channel go into LDS, 4 B per lane and load, coalesced.  A frame outside
//            [0, n_in) is staged as 0.0f and NOT read, one that is not finite as 0.0f (for the reason above a staged zero
//            is the masked tap).  A segment whose whole span lies outside the range is skipped: nothing to add.
//   compute  per 8 taps the lane reads the 8 words below its window as two 16-B words, converts them once and runs
//            8 taps x 8 frames x channels fma: xs word (8 lane + i - kk + P - 1) for frame i, tap kk.  The window of 15
//            doubles per source channel slides by renaming registers: a turn of the loop is two blocks of 8 taps that swap
//            two register sets.  The 8 taps are wave-uniform: read from the tap buffer with a uniform index, they arrive in
//            scalar registers.  The next block's words and taps are asked for before this block's fma run.
// and after the last segment y = (float)(gain * acc), whole 16-B stores; the result's last lane stores frame by frame.
// Nothing is written at or past n_out: the pool's 16 padding frames stay as clip_build zeroed them.
//
// Lanes stand 8 words apart, so the 16-B reads of a 16-lane group fall two by two on the same banks: a 2-way conflict on 2
// reads per 64 (mono) or 128 (stereo result) fp64 fma, which take 4 cycles each.  Rows are therefore neither padded nor
// swizzled.
//
// One call issues the tiles in BANDS, one launch per band, back to back on the edits' stream: a band is as many tiles as
// make 2^36 multiply-adds, but at least 512 (two workgroups per CU).  Output frames are independent, so the banding changes
// no result; it keeps a call at the work cap from being one dispatch of seconds.
// LDS: CS * 4096 * 4 bytes (16 KB / 32 KB).  No scratch.
#include "wbx_ctx.h"

namespace wbx {

namespace {

constexpr uint32_t kT = kConvolveTile, kP = kConvolveSegment;
constexpr uint32_t kRow = kT + kP;                             // staged words per channel: kT + kP - 1 and one never used
constexpr uint64_t kBandWork = 1ull << 36;                     // multiply-adds per launch ...
constexpr uint32_t kBandMinTiles = 512;                        // ... but no fewer tiles than this
static_assert(kT == 256 * 8 && kP % 8 == 0);

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ void __launch_bounds__(256) convolve_taps_kernel(ConvolveArgs a) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= a.l_pad) return;
  for (uint32_t c = 0; c < a.ir_channels; c++) {
    double h = 0.0;
    if (k < a.n_ir) {
      const float v = a.ir[c][k];
      h = finite_bits(v) ? (double)v : 0.0;
    }
    a.taps[(size_t)c * a.l_pad + k] = h;
  }
}

// words w .. w + 7 of every staged channel, as two 16-B reads each (w is a multiple of 4)
template <int CS>
__device__ __forceinline__ void load_words(const float (&xs)[CS][kRow], uint32_t w, f4v (&raw)[CS][2]) {
#pragma unroll
  for (int c = 0; c < CS; c++) {
    raw[c][0] = *reinterpret_cast<const f4v*>(&xs[c][w]);
    raw[c][1] = *reinterpret_cast<const f4v*>(&xs[c][w + 4u]);
  }
}
template <int CS>
__device__ __forceinline__ void widen(const f4v (&raw)[CS][2], double (&out)[CS][8]) {
#pragma unroll
  for (int c = 0; c < CS; c++)
#pragma unroll
    for (int i = 0; i < 8; i++) out[c][i] = (double)raw[c][i >> 2][i & 3];
}
// 8 consecutive taps of every response channel: a wave-uniform address, so they arrive in scalar registers
template <int CI>
__device__ __forceinline__ void load_taps(const double* hp, uint32_t l_pad, double (&h)[CI][8]) {
#pragma unroll
  for (int c = 0; c < CI; c++)
#pragma unroll
    for (int t = 0; t < 8; t++) h[c][t] = hp[(size_t)c * l_pad + t];
}
// taps kk0 .. kk0 + 7 on the lane's 8 frames: lo = words b - 8 .. b - 1, hi = words b .. b + 7; frame i at tap kk0 + t
// reads word b - 1 + i - t.  Per accumulator the taps come in ascending order
template <int CS, int CI, int CO>
__device__ __forceinline__ void taps8(double (&acc)[CO][8], const double (&h)[CI][8], const double (&lo)[CS][8], const double (&hi)[CS][8]) {
#pragma unroll
  for (int t = 0; t < 8; t++)
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
      for (int c = 0; c < CO; c++) {
        const int q = 7 + i - t, cs = CS == 1 ? 0 : c;
        acc[c][i] = __fma_rn(h[CI == 1 ? 0 : c][t], q < 8 ? lo[cs][q] : hi[cs][q - 8], acc[c][i]);
      }
}

template <int CS, int CI>
__global__ void __launch_bounds__(256) convolve_kernel(ConvolveArgs a) {
  constexpr int CO = CS > CI ? CS : CI;
  __shared__ __attribute__((aligned(16))) float xs[CS][kRow];
  const uint32_t tid = threadIdx.x;
  const uint32_t j0 = (a.tile0 + blockIdx.x) * kT;             // the tile's first stored frame, < n_out < 2^31
  const int64_t m0 = (int64_t)a.out_first + (int64_t)j0;       // ... as a frame of the full result
  double acc[CO][8];
#pragma unroll
  for (int c = 0; c < CO; c++)
#pragma unroll
    for (int i = 0; i < 8; i++) acc[c][i] = 0.0;
  for (uint32_t k0 = 0; k0 < a.l_pad; k0 += kP) {
    const int64_t lo = m0 - (int64_t)k0 - (int64_t)(kP - 1u);  // the frame of the range that xs[0] holds (may be < 0)
    if (lo + (int64_t)(kRow - 2u) < 0 || lo >= (int64_t)a.n_in) continue;   // (workgroup-uniform) no frame of the range in reach
    for (uint32_t s = tid; s < kRow; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      const bool in = g >= 0 && g < (int64_t)a.n_in;
#pragma unroll
      for (int c = 0; c < CS; c++) {
        const float v = in ? a.src[c][g] : 0.0f;
        xs[c][s] = finite_bits(v) ? v : 0.0f;
      }
    }
    __syncthreads();
    const uint32_t seg = min(kP, a.l_pad - k0);                // a multiple of 16
    uint32_t b = 8u * tid + kP;                                // the word of frame 0 at tap kk0 - 1: 8 tid - kk0 + P
    double wa[CS][8], wb[CS][8];                               // wa: words b .. b + 7 (the last is never used)
    f4v raw[CS][2];
    double h[CI][8];
    load_words<CS>(xs, b, raw);
    widen<CS>(raw, wa);
    load_words<CS>(xs, b - 8u, raw);
    const double* hp = a.taps + k0;
    load_taps<CI>(hp, a.l_pad, h);
    // 16 taps per turn, as two blocks of 8 that swap the roles of wa and wb: no register is copied.  The words and taps of
    // the NEXT block are asked for once this block's have arrived and before its fma run, which hides their latency
    for (uint32_t kk0 = 0; kk0 < seg; kk0 += 16u, hp += 16, b -= 16u) {
      f4v raw_n[CS][2];
      double h_n[CI][8];
      widen<CS>(raw, wb);                                      // words b - 8 .. b - 1
      load_words<CS>(xs, b - 16u, raw_n);
      load_taps<CI>(hp + 8, a.l_pad, h_n);
      taps8<CS, CI, CO>(acc, h, wb, wa);
      widen<CS>(raw_n, wa);                                    // words b - 16 .. b - 9
      load_words<CS>(xs, (b < 24u ? 24u : b) - 24u, raw);      // (the segment's last turn asks for words nobody uses)
      load_taps<CI>(hp + 16, a.l_pad, h);                      // (... and the call's last for the 8 doubles behind the taps)
      taps8<CS, CI, CO>(acc, h_n, wa, wb);
    }
    __syncthreads();                                           // the next segment's staging overwrites xs
  }
  const uint32_t j = j0 + 8u * tid;
  if (j >= a.n_out) return;
  const uint32_t left = a.n_out - j;
#pragma unroll
  for (int c = 0; c < CO; c++) {
    float y[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const float v = __double2float_rn(__dmul_rn(a.gain, acc[c][i]));
      y[i] = v != v ? __uint_as_float(kCanonNaN) : v;
    }
    float* out = a.dst[c] + j;
    if (left >= 8u) {
      __builtin_nontemporal_store(f4v{y[0], y[1], y[2], y[3]}, reinterpret_cast<f4v*>(out));
      __builtin_nontemporal_store(f4v{y[4], y[5], y[6], y[7]}, reinterpret_cast<f4v*>(out + 4));
    } else {                                                   // the result's last lane: only the frames inside it
#pragma unroll
      for (int i = 0; i < 8; i++)
        if ((uint32_t)i < left) out[i] = y[i];
    }
  }
}

}  // namespace

void launch_convolve_taps(const ConvolveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(convolve_taps_kernel, dim3((a.l_pad + 255u) / 256u), dim3(256), 0, s, a);
}

void launch_convolve(const ConvolveArgs& a, uint32_t n_tiles, hipStream_t s) {
  const dim3 grid(n_tiles), block(256);
  if (a.src_channels == 2u) {
    if (a.ir_channels == 2u) hipLaunchKernelGGL((convolve_kernel<2, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((convolve_kernel<2, 1>), grid, block, 0, s, a);
  } else {
    if (a.ir_channels == 2u) hipLaunchKernelGGL((convolve_kernel<1, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((convolve_kernel<1, 1>), grid, block, 0, s, a);
  }
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clips
wbx_status convolve_check(const ClipSrc& src, uint32_t src_rate, const ClipSrc& ir, uint32_t ir_rate, const ConvolveCall& k,
                          uint32_t* out_channels, const char** why) {
  if (k.n_frames == 0 || k.ir_frames == 0 || k.out_frames == 0) return *why = "clip convolve: no frames", WBX_ERR_INVALID;
  if (!std::isfinite(k.gain)) return *why = "clip convolve: the gain is not finite", WBX_ERR_INVALID;
  if (k.ir_frames > kConvolveMaxTaps) return *why = "clip convolve: a response of more than 2^20 frames", WBX_ERR_UNSUPPORTED;
  const uint64_t full = convolve_frames(k.n_frames, k.ir_frames);
  if (full == 0 || k.out_first > full || k.out_frames > full - k.out_first)
    return *why = "clip convolve: the window ends past the full result (n_frames + ir_frames - 1 frames)", WBX_ERR_INVALID;
  if (k.out_frames >= kConvolveMaxFrames) return *why = "clip convolve: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (src.format != (uint32_t)WBX_FMT_F32 || ir.format != (uint32_t)WBX_FMT_F32)
    return *why = "clip convolve: a clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2 || ir.channels < 1 || ir.channels > 2)
    return *why = "clip convolve: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  const uint32_t ch = std::max(src.channels, ir.channels);
  if (k.out_frames * k.ir_frames > kConvolveMaxWork / ch)      // (< 2^31 * 2^20: the product fits)
    return *why = "clip convolve: more than 2^46 multiply-adds (convolve ranges and overlap-add them with wbx_clip_splice)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip convolve: the source's range ends past the clip", WBX_ERR_INVALID;
  if (k.ir_first > ir.frames || k.ir_frames > ir.frames - k.ir_first)
    return *why = "clip convolve: the response's range ends past the clip", WBX_ERR_INVALID;
  if (src_rate != ir_rate) return *why = "clip convolve: the clips' sample rates differ (convert first: wbx_clip_resample)", WBX_ERR_INVALID;
  *out_channels = ch;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status convolve_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc& ir, uint32_t rate, const ConvolveCall& k, ClipSlot& slot,
                        wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const uint32_t ch = std::max(src.channels, ir.channels);
  const wbx_status st = clipfx_blank_clip(c, slot, ch, rate, k.out_frames, why);
  if (st != WBX_OK) return st;
  ConvolveStage& x = c->conv;
  ConvolveArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.ir[i] = clip_row(ir, i) + k.ir_first;
    a.dst[i] = (float*)slot.d.ch[i % ch];
  }
  a.gain = k.gain;
  a.out_first = k.out_first;
  a.n_in = (uint32_t)k.n_frames;
  a.n_ir = (uint32_t)k.ir_frames;
  a.n_out = (uint32_t)k.out_frames;
  a.l_pad = (a.n_ir + 15u) & ~15u;
  a.src_channels = src.channels;
  a.ir_channels = ir.channels;
  const uint32_t n_tiles = (a.n_out + kT - 1u) / kT;
  const uint64_t tile_work = (uint64_t)kT * a.l_pad * ch;
  const uint32_t band = (uint32_t)std::min<uint64_t>(n_tiles, std::max<uint64_t>(kBandMinTiles, kBandWork / tile_work));
  x.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : x.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess) e = x.d_taps.ensure((size_t)ir.channels * a.l_pad + 8u);   // (8 more: the kernel asks one block ahead)
  if (e == hipSuccess) e = hipEventRecord(x.mark[0], on);
  if (e == hipSuccess) {
    a.taps = x.d_taps.p;
    launch_convolve_taps(a, on);
    e = hipGetLastError();
  }
  for (uint32_t t = 0; t < n_tiles && e == hipSuccess; t += band) {
    a.tile0 = t;
    launch_convolve(a, std::min(band, n_tiles - t), on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(x.mark[1], on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip convolve", e);
  }
  x.timed = true;
  return clipfx_measure_result(c, slot, k.out_frames, stats, why);
}

}  // namespace wbx

extern "C" uint64_t wbx_convolve_frames(uint64_t n_frames, uint64_t ir_frames) { return convolve_frames(n_frames, ir_frames); }
extern "C" uint32_t wbx_convolve_tile_frames(void) { return kConvolveTile; }
extern "C" uint32_t wbx_convolve_segment_taps(void) { return kConvolveSegment; }

extern "C" wbx_status wbx_fir_design(uint32_t rate, int kind, double f1_hz, double f2_hz, uint32_t n_taps, double beta, float* out,
                                     size_t cap_floats) {
  return fir_design(rate, kind, f1_hz, f2_hz, n_taps, beta, out, cap_floats);
}

extern "C" wbx_status wbx_convolve_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::conv, "convolve time: no convolution has completed on this context", out);
}

extern "C" wbx_status wbx_clip_convolve(wbx_ctx* c, uint32_t src_clip, uint32_t ir_clip, uint32_t dst_clip, uint64_t first_frame,
                                        uint64_t n_frames, uint64_t ir_first, uint64_t ir_frames, uint64_t out_first,
                                        uint64_t out_frames, double gain, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, ir_clip, dst_clip, "clip convolve: unknown source clip",
                                   "clip convolve: unknown response clip", "clip convolve: the result may not replace its source or its response");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]), ir = clip_src(c->clips[ir_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const ConvolveCall k{first_frame, n_frames, ir_first, ir_frames, out_first, out_frames, gain};
  const char* msg = "";
  uint32_t ch = 0;
  st = convolve_check(src, rate, ir, c->clips[ir_clip].d.sample_rate, k, &ch, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return convolve_run(c, src, ir, rate, k, slot, stats_of_result, why);
  });
}
