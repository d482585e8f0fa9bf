// wbx_filter.hip — filter_state_kernel, filter_carry_kernel and filter_apply_kernel: a frame range of a resident planar F32
// clip through a cascade of biquads into a new planar F32 clip (wbx.h "Filtering a clip"), and layer 1's calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h, its host half (designs, the test of a cascade, the
// carry matrix) is wbx_filter.h and all of it is mirrored by tests/filter_model.py: a stage is loudness_kernel's biquad —
// every * + - one IEEE fp64 operation, the explicit _rn intrinsics below: nothing may be fused — and the output depends on
// every frame before it, so the frames are cut into chunks of 512 and the state crosses a chunk boundary as the
// specification says it does: three launches back to back on the edits' stream, no host round trip between them.
//
// filter_state_kernel<CH, S>: a lane owns ONE chunk and every channel of it (CH independent cascades that hide each
// other's latency), a wave — one workgroup — owns 64 consecutive chunks and runs them from rest: z_j.  The lanes' frames
// lie 512 apart, so the wave stages them as loudness_kernel does, 64 rows x 64 columns per step: for each row the 64 lanes
// load 64 consecutive frames of that row's chunk, one coalesced 256-B read per row and channel, into xs[c][row][0..63]; a
// frame at or past the range's end (the tail, a row past the last chunk) is staged as 0.0f and NOT read.  Each lane then
// walks its own row: rows are 65 floats long, lane l reads word 65 l + k, bank (l + k) mod 32.  z goes out as fp64,
// [chunk][channel][D].  The last chunk's z is needed by nobody and is not computed.
//
// filter_carry_kernel<S>: one wave walks the chunks in order.  Lane (c, i) keeps row i of the carry matrix in registers
// and owns element i of channel c's state: t_{j+1}[i] = z_j[i] + (sum over k ascending of M[i][k] * t_j[k]), t_j read from
// LDS (every lane of a channel reads the same word: a broadcast), t_{j+1} written to the other of two LDS copies — one
// barrier per chunk — and over z_j in global memory.  The z of the NEXT group of 8 chunks is loaded before the walk over the
// current group, so one memory round trip is paid per 8 chunks, not per chunk.
//
// filter_apply_kernel<CH, S>: the same staging, each lane's cascade started from t_j (chunk 0: from rest), every output
// rounded once to fp32 and written back into the word of xs it was read from (a lane reads and writes its own row only);
// the wave then stores the 64 rows transposed back, one coalesced 256-B row per chunk and channel.  Nothing is stored at
// or past frame n_out: the pool's 16 padding frames stay as clip_build zeroed them.
//
// Stage count and channel count are template parameters: coefficients (wave-uniform) and states stay in registers, no
// scratch.  LDS: CH * 64 * 65 * 4 bytes (33 KB stereo) for the two outer kernels, 2 * 2 * D doubles for the carry.
#include "wbx_ctx.h"

namespace wbx {

namespace {

constexpr uint32_t kRowWords = 65;                             // a staged row: 64 frames and one word of padding
constexpr uint32_t kCarryGroup = 8;                            // chunks whose z the carry loads ahead of its serial walk
static_assert(kFilterChunk == 512 && kFilterChunk % 64 == 0);

// wbx_filter.h's filter_step: v = [x1, x2, y1_1, y2_1, ..., y1_S, y2_S]
template <int S>
__device__ __forceinline__ double cascade_step(const double (&k)[5 * S], double (&v)[2 * S + 2], double x) {
  double in = x;
#pragma unroll
  for (int s = 0; s < S; s++) {
    const double x1 = v[2 * s], x2 = v[2 * s + 1], y1 = v[2 * s + 2], y2 = v[2 * s + 3];
    double y = __dadd_rn(__dmul_rn(k[5 * s], in), __dmul_rn(k[5 * s + 1], x1));
    y = __dadd_rn(y, __dmul_rn(k[5 * s + 2], x2));
    y = __dsub_rn(y, __dmul_rn(k[5 * s + 3], y1));
    y = __dsub_rn(y, __dmul_rn(k[5 * s + 4], y2));
    v[2 * s] = in, v[2 * s + 1] = x1;
    in = y;
  }
  v[2 * S + 1] = v[2 * S];
  v[2 * S] = in;
  return in;
}

// 64 columns from t0 on of the wave's 64 chunks: frame (j0 + r) * 512 + t0 + lane (< 2^31 + 2^15) of row r
template <int CH>
__device__ __forceinline__ void stage_rows(float (&xs)[CH][64][kRowWords], const FilterArgs& a, uint32_t j0, uint32_t t0, uint32_t lane) {
#pragma unroll 8
  for (uint32_t r = 0; r < 64u; r++) {
    const uint32_t g = (j0 + r) * kFilterChunk + t0 + lane;
    const bool in = g < a.n_in;
#pragma unroll
    for (int c = 0; c < CH; c++) xs[c][r][lane] = in ? a.src[c][g] : 0.0f;
  }
}

__device__ __forceinline__ double sample_in(float xf) {        // a sample that is not finite enters as 0.0
  return (__float_as_uint(xf) & 0x7F800000u) == 0x7F800000u ? 0.0 : (double)xf;
}

template <int CH, int S>
__global__ void __launch_bounds__(64) filter_state_kernel(FilterArgs a) {
  constexpr int D = 2 * S + 2;
  __shared__ float xs[CH][64][kRowWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t j0 = blockIdx.x * 64u;                        // the wave's first chunk
  double k[5 * S];
#pragma unroll
  for (int i = 0; i < 5 * S; i++) k[i] = a.coef[i];
  double v[CH][D];
#pragma unroll
  for (int c = 0; c < CH; c++)
#pragma unroll
    for (int i = 0; i < D; i++) v[c][i] = 0.0;
  for (uint32_t t0 = 0; t0 < kFilterChunk; t0 += 64u) {
    stage_rows<CH>(xs, a, j0, t0, lane);
    __syncthreads();
    for (uint32_t q = 0; q < 64u; q++) {
#pragma unroll
      for (int c = 0; c < CH; c++) (void)cascade_step<S>(k, v[c], sample_in(xs[c][lane][q]));
    }
    __syncthreads();                                           // the next step's staging overwrites xs
  }
  const uint32_t j = j0 + lane;
  if (j + 1u < a.n_chunks) {
    double* z = a.state + (size_t)j * (CH * D);
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int i = 0; i < D; i++) z[c * D + i] = v[c][i];
  }
}

template <int S>
__global__ void __launch_bounds__(64) filter_carry_kernel(FilterArgs a) {
  constexpr int D = 2 * S + 2;
  __shared__ double t[2][2 * D];
  const uint32_t lane = threadIdx.x;
  const uint32_t rows = a.channels * (uint32_t)D;              // <= 36
  const bool active = lane < rows;
  const uint32_t c = active ? lane / (uint32_t)D : 0u, i = active ? lane % (uint32_t)D : 0u;
  double m[D];
#pragma unroll
  for (int q = 0; q < D; q++) m[q] = a.M[i * (uint32_t)D + (uint32_t)q];
  if (lane < 2u * (uint32_t)D) t[0][lane] = 0.0;               // t_0
  __syncthreads();
  const uint32_t n = a.n_chunks - 1u;                          // states to carry: slot j holds z_j and receives t_{j+1}
  double z[kCarryGroup], z_next[kCarryGroup];                  // this group's z_j; the next group's, in flight behind it
#pragma unroll
  for (uint32_t g = 0; g < kCarryGroup; g++) z[g] = active && g < n ? a.state[(size_t)g * rows + lane] : 0.0;
  for (uint32_t j0 = 0; j0 < n; j0 += kCarryGroup) {
#pragma unroll
    for (uint32_t g = 0; g < kCarryGroup; g++) {               // (slots the group below does not write)
      const uint32_t j = j0 + kCarryGroup + g;
      z_next[g] = active && j < n ? a.state[(size_t)j * rows + lane] : 0.0;
    }
#pragma unroll
    for (uint32_t g = 0; g < kCarryGroup; g++) {
      const uint32_t j = j0 + g;
      if (j >= n) break;                                       // wave-uniform
      const double* tj = &t[j & 1u][c * (uint32_t)D];
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < D; q++) acc = __dadd_rn(acc, __dmul_rn(m[q], tj[q]));
      const double tn = __dadd_rn(z[g], acc);
      if (active) {
        t[(j + 1u) & 1u][lane] = tn;
        a.state[(size_t)j * rows + lane] = tn;
      }
      __syncthreads();
    }
#pragma unroll
    for (uint32_t g = 0; g < kCarryGroup; g++) z[g] = z_next[g];
  }
}

template <int CH, int S>
__global__ void __launch_bounds__(64) filter_apply_kernel(FilterArgs a) {
  constexpr int D = 2 * S + 2;
  __shared__ float xs[CH][64][kRowWords];
  const uint32_t lane = threadIdx.x;
  const uint32_t j0 = blockIdx.x * 64u;
  const uint32_t j = j0 + lane;
  double k[5 * S];
#pragma unroll
  for (int i = 0; i < 5 * S; i++) k[i] = a.coef[i];
  double v[CH][D];
  const bool carried = j >= 1u && j < a.n_chunks;              // chunk 0 starts from rest; a lane past the result computes nothing kept
  const double* tj = a.state + (size_t)(carried ? j - 1u : 0u) * (CH * D);
#pragma unroll
  for (int c = 0; c < CH; c++)
#pragma unroll
    for (int i = 0; i < D; i++) v[c][i] = carried ? tj[c * D + i] : 0.0;
  for (uint32_t t0 = 0; t0 < kFilterChunk; t0 += 64u) {
    stage_rows<CH>(xs, a, j0, t0, lane);
    __syncthreads();
    for (uint32_t q = 0; q < 64u; q++) {
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float y = __double2float_rn(cascade_step<S>(k, v[c], sample_in(xs[c][lane][q])));
        xs[c][lane][q] = y != y ? __uint_as_float(kCanonNaN) : y;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (uint32_t r = 0; r < 64u; r++) {
      const uint32_t g = (j0 + r) * kFilterChunk + t0 + lane;
      if (g < a.n_out) {
#pragma unroll
        for (int c = 0; c < CH; c++) a.dst[c][g] = xs[c][r][lane];
      }
    }
    __syncthreads();                                           // the next step's staging overwrites xs
  }
}

template <template <int, int> class Launch>
void dispatch(const FilterArgs& a, dim3 grid, hipStream_t s) {
#define WBX_FILTER_CASE(S_)                                  \
  case S_:                                                   \
    if (a.channels == 2u) Launch<2, S_>::go(a, grid, s);     \
    else Launch<1, S_>::go(a, grid, s);                      \
    break;
  switch (a.stages) {
    WBX_FILTER_CASE(1) WBX_FILTER_CASE(2) WBX_FILTER_CASE(3) WBX_FILTER_CASE(4)
    WBX_FILTER_CASE(5) WBX_FILTER_CASE(6) WBX_FILTER_CASE(7) WBX_FILTER_CASE(8)
  }
#undef WBX_FILTER_CASE
}
template <int CH, int S>
struct LaunchState {
  static void go(const FilterArgs& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((filter_state_kernel<CH, S>), grid, dim3(64), 0, s, a); }
};
template <int CH, int S>
struct LaunchApply {
  static void go(const FilterArgs& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((filter_apply_kernel<CH, S>), grid, dim3(64), 0, s, a); }
};
template <int CH, int S>
struct LaunchCarry {                                           // (one instance per stage count: the channel count is an argument)
  static void go(const FilterArgs& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((filter_carry_kernel<S>), grid, dim3(64), 0, s, a); }
};

}  // namespace

void launch_filter_state(const FilterArgs& a, hipStream_t s) { dispatch<LaunchState>(a, dim3((a.n_chunks - 1u + 63u) / 64u), s); }
void launch_filter_carry(const FilterArgs& a, hipStream_t s) { dispatch<LaunchCarry>(a, dim3(1), s); }
void launch_filter_apply(const FilterArgs& a, hipStream_t s) { dispatch<LaunchApply>(a, dim3((a.n_chunks + 63u) / 64u), s); }

// ---- layer 1: checks (no device call), the run ------------------------------------------------------------------------------

wbx_status filter_check_call(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, uint64_t tail_frames, const double* coef,
                             uint32_t n_stages, const char** why) {
  if (n_frames == 0) return *why = "clip filter: no frames", WBX_ERR_INVALID;
  if (first_frame > src.frames || n_frames > src.frames - first_frame) return *why = "clip filter: the range ends past the clip", WBX_ERR_INVALID;
  if (!coef) return *why = "clip filter: coef is NULL", WBX_ERR_INVALID;
  if (filter_check(coef, n_stages) != WBX_OK)
    return *why = "clip filter: 1 to 8 stages of finite coefficients strictly inside the stability triangle", WBX_ERR_INVALID;
  if (tail_frames >= kFilterMaxFrames || n_frames + tail_frames >= kFilterMaxFrames)
    return *why = "clip filter: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip filter: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip filter: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status filter_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, uint64_t first_frame, uint64_t n_frames, uint64_t tail_frames,
                      const double* coef, uint32_t n_stages, ClipSlot& slot, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const uint64_t n_out = n_frames + tail_frames;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, n_out, why);
  if (st != WBX_OK) return st;
  FilterStage& x = c->filt;
  const uint32_t D = 2u * n_stages + 2u;
  FilterArgs a{};
  for (uint32_t ch = 0; ch < 2; ch++) {
    a.src[ch] = clip_row(src, ch) + first_frame;
    a.dst[ch] = (float*)slot.d.ch[ch % src.channels];
  }
  for (uint32_t i = 0; i < 5u * n_stages; i++) a.coef[i] = coef[i];
  a.n_in = (uint32_t)n_frames;
  a.n_out = (uint32_t)n_out;
  a.n_chunks = (uint32_t)((n_out + kFilterChunk - 1u) / kFilterChunk);
  a.channels = src.channels;
  a.stages = n_stages;
  hipError_t e = hipSuccess;
  x.timed = false;
  for (Event& m : x.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess && a.n_chunks > 1u) {                    // (one chunk IS the sequential pass: nothing to carry)
    e = x.d_state.ensure((size_t)(a.n_chunks - 1u) * src.channels * D);
    if (e == hipSuccess) e = x.d_M.ensure((size_t)kFilterMaxDim * kFilterMaxDim);
    if (e == hipSuccess) e = x.h_M.ensure((size_t)kFilterMaxDim * kFilterMaxDim);
    if (e == hipSuccess) {
      filter_transition(coef, n_stages, x.h_M.p);              // (the stream was waited for when the last run returned)
      e = hipMemcpyAsync(x.d_M.p, x.h_M.p, (size_t)D * D * sizeof(double), hipMemcpyHostToDevice, on);
    }
    if (e == hipSuccess) e = hipEventRecord(x.mark[0], on);
    if (e == hipSuccess) {
      a.state = x.d_state.p;
      a.M = x.d_M.p;
      launch_filter_state(a, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(x.mark[1], on);
    if (e == hipSuccess) {
      launch_filter_carry(a, on);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipEventRecord(x.mark[2], on);
  if (e == hipSuccess) {
    launch_filter_apply(a, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(x.mark[3], on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip filter", e);
  }
  x.timed = true;
  x.carried = a.n_chunks > 1u;
  return clipfx_measure_result(c, slot, n_out, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_filter_phase_ms(wbx_ctx* c, double out[3]) {
  if (!c || !out) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->fx_mu);
  FilterStage& x = c->filt;
  if (!x.timed) return fail(c, WBX_ERR_INVALID, "filter phase times: no filter has completed on this context");
  float ms[3] = {0.0f, 0.0f, 0.0f};
  for (int i = x.carried ? 0 : 2; i < 3; i++) WBX_HIP(c, hipEventElapsedTime(&ms[i], x.mark[i], x.mark[i + 1]));
  for (int i = 0; i < 3; i++) out[i] = (double)ms[i];
  return WBX_OK;
}

extern "C" wbx_status wbx_filter_design(uint32_t rate, int kind, double freq_hz, double q, double gain, double out[5]) {
  return filter_design(rate, kind, freq_hz, q, gain, out);
}

extern "C" wbx_status wbx_filter_check(const double* coef, uint32_t n_stages) { return filter_check(coef, n_stages); }

extern "C" wbx_status wbx_filter_transition(const double* coef, uint32_t n_stages, double* M, size_t cap_doubles) {
  if (!M || filter_check(coef, n_stages) != WBX_OK) return WBX_ERR_INVALID;
  const size_t D = 2 * (size_t)n_stages + 2;
  if (cap_doubles < D * D) return WBX_ERR_INVALID;
  filter_transition(coef, n_stages, M);
  return WBX_OK;
}

extern "C" uint32_t wbx_filter_chunk_frames(void) { return kFilterChunk; }

extern "C" wbx_status wbx_clip_filter(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                      uint64_t tail_frames, const double* coef, uint32_t n_stages, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip filter: unknown source clip", "clip filter: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const char* msg = "";
  st = filter_check_call(src, first_frame, n_frames, tail_frames, coef, n_stages, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return filter_run(c, src, rate, first_frame, n_frames, tail_frames, coef, n_stages, slot, stats_of_result, why);
  });
}
