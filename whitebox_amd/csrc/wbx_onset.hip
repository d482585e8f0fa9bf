// wbx_onset.hip — onset_energy_kernel and onset_novelty_kernel: the onset-strength curve of a frame range of a resident planar
// F32 clip, one value per hop (wbx.h "Finding a clip's onsets and tempo"), and layer 1's two calls on top of them.
// Measurements: nothing is allocated in the pool.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/onset_model.py.
//   the energy pass  reads the range once.  A wave owns one hop at a time and strides over the hops by the grid; lane i owns
//             the hop's run i of q = H / 64 consecutive frames, its two fp64 sums a (squares) and b (squared first
//             differences), and the wave adds the 64 runs by an xor butterfly — the balanced tree of adjacent pairs, as
//             u + v == v + u — and stores (A, B) as one 16-byte word.  The detector and the non-finite rule are computed on
//             load.  d[t-1] of a run's first frame is the frame before it in the range, 0.0 at the range's first frame:
//             the frame before the range is never read, and no run reaches past its own hop
//   q = 1, 2, 4   a lane reads its run directly, as one 4-, 8- or 16-byte load where the rows lie on that many bytes (word
//             by word otherwise), coalesced across the wave; d[t-1] comes from the lane below by a shuffle, lane 0 loads
//             it.  Four hops of the wave are loaded, summed and reduced side by side, free of branches, to keep more bytes in flight
//             and to let the four butterflies hide each other's latency
//   other q   the wave stages the run in chunks of C = min(q, 32) columns per lane through a wave-private LDS block of 64
//             rows: the 64 C words are loaded in flat order — word s is row s / C, column s % C, both kept incrementally —
//             so a chunk is read as 64 / C rows' whole segments per load (for q <= 32: the hop, contiguously), whatever H
//             is.  Rows lie an odd number of words apart (wbx_onset.h onset_shape), so the lanes' walks, each along its own
//             row, meet different banks.  d[t-1] of a lane's first frame is one load per lane and hop (a line the wave
//             reads anyway); between chunks it stays in a register.  A wave's block is its own: no workgroup barrier
//   the novelty pass  a lane per hop: the two rises against the maximum of the three hops before, the record, and o as a
//             float into a buffer of its own, which a tempo call hands to f0_run as a mono F32 clip whose frames are hops
// Nothing waits on another workgroup, and there is no scratch.
#include "wbx_ctx.h"

#include <cstring>

namespace wbx {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int kAhead = 4;                                      // hops a wave of the direct instances asks for at once

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double sample_in(float v) { return finite_bits(v) ? (double)v : 0.0; }

// the detector d of one frame from its channels' samples ("Stretching a clip"'s)
template <int CH>
__device__ __forceinline__ float detector(float x0, float x1) {
  if (CH == 1) return finite_bits(x0) ? x0 : 0.0f;
  return __double2float_rn(__dmul_rn(0.5, __dadd_rn(sample_in(x0), sample_in(x1))));
}

// one frame of a run: a = a + d d (exact product: the fma is the model's), e = d - prev, b = b + (e e) (two roundings)
__device__ __forceinline__ void term(float df, double& prev, double& A, double& B) {
  const double d = (double)df;
  A = fma(d, d, A);
  const double e = __dsub_rn(d, prev);
  B = __dadd_rn(B, __dmul_rn(e, e));
  prev = d;
}

// the 64 run sums as a balanced tree of adjacent pairs; lane 0 stores the hop's pair
__device__ __forceinline__ void finish(const OnsetArgs& a, uint32_t h, uint32_t lane, double A, double B) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    A = __dadd_rn(A, __shfl_xor(A, off));
    B = __dadd_rn(B, __shfl_xor(B, off));
  }
  if (lane == 0u) a.energy[h] = OnsetEnergy{A, B};
}

template <int CH, int Q>
struct Run {
  float v[CH][Q];              // the lane's run, per channel
  float halo[CH];              // lane 0: the frame before the hop (0.0f at the range's first frame, not read)
};

template <int CH, int Q>
__device__ __forceinline__ void run_load(const OnsetArgs& a, uint32_t h, uint32_t lane, Run<CH, Q>& r) {
  const uint32_t t = h * a.H + lane * (uint32_t)Q;             // < (h + 1) H <= n < 2^31
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const float* p = a.src[c] + t;
    if (Q == 2 && a.aligned) {
      const f2 v = *reinterpret_cast<const f2*>(p);
      r.v[c][0] = v[0], r.v[c][Q > 1 ? 1 : 0] = v[1];
    } else if (Q == 4 && a.aligned) {
      const f4 v = *reinterpret_cast<const f4*>(p);
#pragma unroll
      for (int j = 0; j < Q; j++) r.v[c][j] = v[j & 3];
    } else {
#pragma unroll
      for (int j = 0; j < Q; j++) r.v[c][j] = p[j];
    }
    r.halo[c] = (lane == 0u && t > 0u) ? p[-1] : 0.0f;
  }
}

// the two run sums of the lane from what run_load asked for
template <int CH, int Q>
__device__ __forceinline__ void run_sum(uint32_t lane, const Run<CH, Q>& r, double& A, double& B) {
  float d[Q];
#pragma unroll
  for (int j = 0; j < Q; j++) d[j] = detector<CH>(r.v[0][j], r.v[CH - 1][j]);
  const float below = __shfl_up(d[Q - 1], 1);                  // the last frame of the run before this one
  double prev = (double)(lane == 0u ? detector<CH>(r.halo[0], r.halo[CH - 1]) : below);
  A = 0.0, B = 0.0;
#pragma unroll
  for (int j = 0; j < Q; j++) term(d[j], prev, A, B);
}

// where a lane's words of a staged chunk of C columns lie: word s = lane + 64 i is row s / C, column s % C
struct Walk {
  uint32_t r, c, dr, dc;
};
__device__ __forceinline__ Walk walk_of(uint32_t lane, uint32_t C) {
  Walk w;
  w.r = lane / C, w.c = lane - w.r * C;
  w.dr = 64u / C, w.dc = 64u - w.dr * C;
  return w;
}

__device__ __forceinline__ void wave_sync() {                  // the wave's LDS writes before its reads, and the reverse
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// columns [k0, k0 + C) of every lane's run of the hop at frame t0: staged, then walked
template <int CH>
__device__ __forceinline__ void chunk(const OnsetArgs& a, float* rows, uint32_t t0, uint32_t k0, uint32_t C, const Walk& w,
                                      uint32_t lane, double& prev, double& A, double& B) {
  uint32_t r = w.r, c = w.c;
#pragma unroll 4
  for (uint32_t i = 0; i < C; i++) {                           // r <= 63: the last word is 64 C - 1
    const uint32_t t = t0 + r * a.q + k0 + c;                  // < t0 + H
    rows[r * a.row + c] = detector<CH>(a.src[0][t], a.src[CH - 1][t]);
    r += w.dr, c += w.dc;
    if (c >= C) c -= C, r++;
  }
  wave_sync();
  const float* mine = rows + lane * a.row;
  for (uint32_t k = 0; k < C; k++) term(mine[k], prev, A, B);
  wave_sync();
}

template <int CH, int Q>
__global__ void __launch_bounds__(kOnsetLanes) onset_energy_kernel(OnsetArgs a) {
  extern __shared__ float lds[];                               // onset_shape's lds_bytes: a block of 64 rows per wave (Q = 0)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t first = blockIdx.x * kOnsetWaves + wave, stride = gridDim.x * kOnsetWaves;
  if constexpr (Q > 0) {
    constexpr int QQ = Q > 0 ? Q : 1;
    // kAhead hops of the wave at a time, without a branch between them so that their loads and their butterflies interleave:
    // a turn past the wave's last hop reads the call's last hop again (a hop that exists) and stores nothing
    for (uint32_t h0 = first; h0 < a.hops; h0 += (uint32_t)kAhead * stride) {
      Run<CH, QQ> r[kAhead];
      uint32_t h[kAhead];
      double A[kAhead], B[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; u++) {
        h[u] = h0 + (uint32_t)u * stride;
        run_load<CH, QQ>(a, h[u] < a.hops ? h[u] : a.hops - 1u, lane, r[u]);
      }
#pragma unroll
      for (int u = 0; u < kAhead; u++) run_sum<CH, QQ>(lane, r[u], A[u], B[u]);
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {                 // finish()'s tree, the hops side by side
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
          A[u] = __dadd_rn(A[u], __shfl_xor(A[u], off));
          B[u] = __dadd_rn(B[u], __shfl_xor(B[u], off));
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; u++)
        if (lane == 0u && h[u] < a.hops) a.energy[h[u]] = OnsetEnergy{A[u], B[u]};
    }
    return;
  }
  float* rows = lds + wave * 64u * a.row;
  const uint32_t C = a.q < kOnsetChunk ? a.q : kOnsetChunk, tail = a.q > kOnsetChunk ? a.q % kOnsetChunk : 0u;
  const Walk full = walk_of(lane, C), last = walk_of(lane, tail ? tail : 1u);
  for (uint32_t h = first; h < a.hops; h += stride) {
    const uint32_t t0 = h * a.H, mine = t0 + lane * a.q;       // the hop's and the run's first frame
    double prev = mine > 0u ? (double)detector<CH>(a.src[0][mine - 1u], a.src[CH - 1][mine - 1u]) : 0.0;
    double A = 0.0, B = 0.0;
    uint32_t k0 = 0;
    for (; k0 + C <= a.q; k0 += C) chunk<CH>(a, rows, t0, k0, C, full, lane, prev, A, B);
    if (tail) chunk<CH>(a, rows, t0, k0, tail, last, lane, prev, A, B);
    finish(a, h, lane, A, B);
  }
}

// ref = max(X(h-1), X(h-2), X(h-3)); up = X - ref, not > 0 -> 0; rise = up / ((X + ref) + floor)
__device__ __forceinline__ double rise(double x, double x1, double x2, double x3, double floor) {
  double ref = x1 > x2 ? x1 : x2;
  ref = ref > x3 ? ref : x3;
  double up = __dsub_rn(x, ref);
  if (!(up > 0.0)) up = 0.0;
  return __ddiv_rn(up, __dadd_rn(__dadd_rn(x, ref), floor));
}

__global__ void __launch_bounds__(256) onset_novelty_kernel(OnsetArgs a) {
  const uint32_t h = blockIdx.x * 256u + threadIdx.x;
  if (h >= a.hops) return;
  const OnsetEnergy zero{0.0, 0.0};
  const OnsetEnergy x = a.energy[h], x1 = h >= 1u ? a.energy[h - 1u] : zero, x2 = h >= 2u ? a.energy[h - 2u] : zero,
                    x3 = h >= 3u ? a.energy[h - 3u] : zero;
  const float o = __double2float_rn(__dadd_rn(rise(x.a, x1.a, x2.a, x3.a, a.floor), rise(x.b, x1.b, x2.b, x3.b, a.floor)));
  wbx_onset_frame rec;
  rec.energy = x.a;
  rec.edge_energy = x.b;
  rec.novelty = (double)o;
  rec.onset = 0u;
  rec._pad = 0u;
  a.rec[h] = rec;
  a.novelty[h] = o;
}

template <int CH>
void launch_energy_of(const OnsetArgs& a, const OnsetShape& sh, hipStream_t s) {
  const dim3 grid(sh.grid), block(kOnsetLanes);
  if (a.q == 1u) hipLaunchKernelGGL((onset_energy_kernel<CH, 1>), grid, block, 0, s, a);
  else if (a.q == 2u) hipLaunchKernelGGL((onset_energy_kernel<CH, 2>), grid, block, 0, s, a);
  else if (a.q == 4u) hipLaunchKernelGGL((onset_energy_kernel<CH, 4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((onset_energy_kernel<CH, 0>), grid, block, sh.lds_bytes, s, a);
}

}  // namespace

void launch_onset_energy(const OnsetArgs& a, hipStream_t s) {
  const OnsetShape sh = onset_shape(a.H, a.hops);
  if (a.channels == 2u) launch_energy_of<2>(a, sh, s);
  else launch_energy_of<1>(a, sh, s);
}
void launch_onset_novelty(const OnsetArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(onset_novelty_kernel, dim3((a.hops + 255u) / 256u), dim3(256), 0, s, a);
}

// ---- layer 1: the checks (no device call), the runs -------------------------------------------------------------------------

namespace {

wbx_status onset_check_clip(const ClipSrc& src, const OnsetCall& k, const char* what[3], const char** why) {
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = what[0], WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = what[1], WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame) return *why = what[2], WBX_ERR_INVALID;
  return WBX_OK;
}

// Both passes on the edits' stream, nothing waited for: energies, novelty and records are on the device when the stream
// gets there.  Zero hops launch nothing
hipError_t onset_measure(wbx_ctx* c, const ClipSrc& src, const OnsetCall& k, uint64_t hops) {
  const hipStream_t on = c->fx.side.stream;
  OnsetStage& z = c->ons;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  if (e == hipSuccess && hops) e = z.d_energy.ensure((size_t)hops);
  if (e == hipSuccess && hops) e = z.d_nov.ensure((size_t)hops);
  if (e == hipSuccess && hops) e = z.d_rec.ensure((size_t)hops);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess && hops) {
    const OnsetShape sh = onset_shape(k.hop, hops);
    OnsetArgs a{};
    a.src[0] = clip_row(src, 0) + k.first_frame, a.src[1] = clip_row(src, 1) + k.first_frame;
    a.energy = z.d_energy.p, a.novelty = z.d_nov.p, a.rec = z.d_rec.p;
    a.floor = (double)k.hop * k.floor_power;
    a.hops = (uint32_t)hops;
    a.H = k.hop, a.q = sh.q, a.row = sh.row;
    a.channels = src.channels;
    a.aligned = (((uintptr_t)a.src[0] | (uintptr_t)a.src[1]) % (4u * sh.q)) == 0u ? 1u : 0u;
    launch_onset_energy(a, on);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
    if (e == hipSuccess) {
      launch_onset_novelty(a, on);
      e = hipGetLastError();
    }
  } else if (e == hipSuccess) {
    e = hipEventRecord(z.mark[1], on);
  }
  return e;
}

}  // namespace

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status onset_check_call(const ClipSrc& src, const OnsetCall& k, const char** why) {
  const wbx_status st = onset_check(k, why);
  if (st != WBX_OK) return st;
  const char* what[3] = {"clip onsets: the clip's storage format is not F32", "clip onsets: clip channel count (1 or 2)",
                         "clip onsets: the range ends past the clip"};
  return onset_check_clip(src, k, what, why);
}
wbx_status tempo_check_call(const ClipSrc& src, const OnsetCall& k, F0Call* track, const char** why) {
  const wbx_status st = tempo_check(k, track, why);
  if (st != WBX_OK) return st;
  const char* what[3] = {"clip tempo: the clip's storage format is not F32", "clip tempo: clip channel count (1 or 2)",
                         "clip tempo: the range ends past the clip"};
  return onset_check_clip(src, k, what, why);
}

wbx_status onset_run(wbx_ctx* c, const ClipSrc& src, const OnsetCall& k, wbx_onset_frame* frames_out, wbx_onset_info* info, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  OnsetStage& z = c->ons;
  const uint64_t hops = onset_hops(k.n_frames, k.hop);
  z.timed = false;
  hipError_t e = hops ? z.h_rec.ensure((size_t)hops) : hipSuccess;
  if (e == hipSuccess) e = onset_measure(c, src, k, hops);
  if (e == hipSuccess && hops) e = hipMemcpyAsync(z.h_rec.p, z.d_rec.p, (size_t)hops * sizeof(wbx_onset_frame), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still read the clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) return stage_fail(why, WBX_ERR_DEVICE, "clip onsets", e);
  z.timed = true;
  const uint64_t onsets = onset_pick(z.h_rec.p, hops, k.threshold, k.delta, k.w, k.a);
  if (hops) std::memcpy(frames_out, z.h_rec.p, (size_t)hops * sizeof(wbx_onset_frame));
  if (info) {
    info->hops = hops;
    info->onsets = onsets;
    info->launches = hops ? 2u : 0u;
    info->_pad = 0;
  }
  return WBX_OK;
}

// The novelty stays on the device: f0_run — unchanged — reads it as a mono F32 range of `hops` frames on the same stream,
// behind the two passes, and waits for the device
wbx_status tempo_run(wbx_ctx* c, const ClipSrc& src, const OnsetCall& k, const F0Call& track, wbx_f0_frame* frames_out, wbx_f0_info* info,
                     std::string* why) {
  OnsetStage& z = c->ons;
  const uint64_t hops = onset_hops(k.n_frames, k.hop);
  z.timed = false;
  const hipError_t e = onset_measure(c, src, k, hops);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->fx.side.stream);             // nothing may still read the clip
    return stage_fail(why, WBX_ERR_DEVICE, "clip tempo", e);
  }
  const ClipSrc novelty{z.d_nov.p, 0, 1u, (uint32_t)WBX_FMT_F32, hops};
  const wbx_status st = f0_run(c, novelty, track, frames_out, info, why);
  z.timed = st == WBX_OK;
  return st;
}

}  // namespace wbx

extern "C" uint64_t wbx_onset_hops(uint64_t n_frames, uint32_t hop_frames) { return wbx::onset_hops(n_frames, hop_frames); }
extern "C" wbx_status wbx_onset_check(uint64_t n_frames, uint32_t hop_frames, double floor_power, double threshold, double delta,
                                      uint32_t w, uint32_t a, int has_frames_out, size_t frames_cap) {
  const wbx::OnsetCall k{0, n_frames, hop_frames, floor_power, threshold, delta, w, a, has_frames_out != 0, frames_cap};
  const char* msg = "";
  return wbx::onset_check(k, &msg);
}
extern "C" uint64_t wbx_onset_max_hops(void) { return wbx::kOnsetMaxHops; }
extern "C" wbx_status wbx_onset_pick(wbx_onset_frame* frames, uint64_t hops, double threshold, double delta, uint32_t w, uint32_t a,
                                     uint64_t* onsets) {
  const char* msg = "";
  if (wbx::onset_check_pick(threshold, delta, w, a, &msg) != WBX_OK || (hops > 0 && !frames)) return WBX_ERR_INVALID;
  const uint64_t count = wbx::onset_pick(frames, hops, threshold, delta, w, a);
  if (onsets) *onsets = count;
  return WBX_OK;
}

extern "C" wbx_status wbx_onset_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::ons, "onset time: no onsets or tempo call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_onsets(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                                      double floor_power, double threshold, double delta, uint32_t w, uint32_t a,
                                      wbx_onset_frame* frames_out, size_t frames_cap, wbx_onset_info* info) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip onsets: unknown clip");
  const ClipSrc src = clip_src(*s);
  const OnsetCall k{first_frame, n_frames, hop_frames, floor_power, threshold, delta, w, a, frames_out != nullptr, frames_cap};
  const char* msg = "";
  const wbx_status st = onset_check_call(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return onset_run(c, src, k, frames_out, info, why); });
}

extern "C" wbx_status wbx_clip_tempo(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                                     double floor_power, uint32_t window_hops, uint32_t step_hops, uint32_t lag_min, uint32_t lag_max,
                                     double threshold, wbx_f0_frame* frames_out, size_t frames_cap, wbx_f0_info* info) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip tempo: unknown clip");
  const ClipSrc src = clip_src(*s);
  const OnsetCall k{first_frame, n_frames, hop_frames, floor_power, 0.0, 0.0, 0u, 0u, false, 0};
  F0Call track{0, 0, window_hops, step_hops, lag_min, lag_max, threshold, frames_out != nullptr, frames_cap};
  const char* msg = "";
  const wbx_status st = tempo_check_call(src, k, &track, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return tempo_run(c, src, k, track, frames_out, info, why); });
}
