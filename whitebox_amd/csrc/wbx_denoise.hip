// wbx_denoise.hip — reducing a resident clip's noise (wbx.h "Reducing a clip's noise"): a spectral gate between a direct
// forward and a direct inverse transform, overlap-added into a new clip, and the noise profile that feeds its threshold;
// layer 1's two calls on top.  No FFT, no sin and no log on the device: both transforms are host-built tables.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/denoise_model.py.
//   the product  rows 0 and B - 1 of the sine tables are all +0.0, so per hop and channel BOTH transforms are W real chains of
//             W terms (wbx_denoise.h packs cells, masked cells and the two tables accordingly): one kernel,
//             denoise_transform_kernel, serves both.  It is spectrum_kernel's turn: a lane owns K pairs of neighbouring
//             chains x 8 / K consecutive hops in 16 fp64 accumulators, the operand of the workgroup's hops is staged in LDS
//             as floats in chunks of at most 512 terms and read as broadcasts, 16 bytes per hop and turn of four terms; the
//             table row [i][pair] is read coalesced, 8 bytes per lane, one turn ahead.  Both factors are fp32 values, so
//             fma(d, c, acc) IS acc + d * c.  The ragged bin grid (B = 64 m + 1) is gone with the packing: the Nyquist bin's
//             real chain sits where bin 0's imaginary chain would idle, and no lane diverges.  Only W = 64 (32 pairs) leaves
//             half a wave without a chain of its own: it computes pair 31 again and stores nothing
//   analysis  the operand is the clip: hop t of the workgroup lies H words behind hop t - 1, so the hops share one run of
//             (F - 1) H + chunk frames.  A frame before the range's first or at or past its last is staged as 0.0 and NOT
//             read; what is not finite is staged as 0.0.  The epilogue rounds to the fp32 cell pair
//   synthesis the operand is a hop's masked row, chunk words per hop.  The epilogue stores the chain values as DOUBLES
//   LDS banks a turn's staged reads are one 16-byte word per hop at the same address in every lane of a wave: a broadcast,
//             one bank group per read, no conflict by the guide's rule (same address, any bank).  The gate's box reads
//             p[row][lane + f]: consecutive 8-byte words over the lanes, two per bank pair, conflict-free.  Derived, not
//             counted
//   the gate  denoise_gate_kernel: a workgroup owns (hop, channel, 256 bins); the powers of the box's rows — at most 9 x
//             (256 + 16) doubles, what lies outside the grid as +0.0, which adds nothing to a sum that is never negative —
//             are staged once, every lane walks its (2 S + 1) x (2 F + 1) box in order.  The masked cells go to their own
//             rows (neighbours need the unmasked).  Open cells: an integer per workgroup, folded by one workgroup
//             (denoise_fold_kernel), no float atomics
//   the add   denoise_ola_kernel: a lane owns 4 consecutive output frames, reads the four hops' chain values (32 bytes
//             each), adds them in hop order in fp64, rounds once and stores 16 bytes (the range's tail frame by frame)
//   the profile  denoise_profile_kernel: a lane per (channel, bin) walks the launch's hops in order over the cells
// No scratch, no inline assembly, nothing waits on another workgroup.
#include "wbx_ctx.h"

#include <cstring>
#include <vector>

namespace wbx {

namespace {

constexpr uint32_t kLanes = 256;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

template <int KB>
struct TableTurn {
  f2 v[4][KB];                 // the table words of terms i .. i + 3 at the lane's pairs
};
// (rows past the last read that one again: asked for ahead, never used)
template <int KB>
__device__ __forceinline__ void ask(TableTurn<KB>& t, const float* tab, uint32_t i, uint32_t W, const uint32_t (&pc)[KB]) {
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const uint32_t row = i + k < W ? i + k : W - 1u;
    const f2* p = reinterpret_cast<const f2*>(tab + (size_t)row * W);
#pragma unroll
    for (int b = 0; b < KB; b++) t.v[k][b] = p[pc[b]];
  }
}

// SYN false: cells[hop][channel][2 pair ..] = the chains over the clip's frames; true: chain[...] = the chains over masked rows
template <bool SYN, int KB>
__global__ void __launch_bounds__(kLanes) denoise_transform_kernel(DenArgs a) {
  constexpr int KH = 8 / KB;
  constexpr uint32_t kWavePairs = 64u * KB;
  __shared__ __attribute__((aligned(16))) float span[kDenSpanWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t wb = wave % a.G, wh = wave / a.G;             // the wave's column of pairs, its row of hops
  const uint32_t ch = blockIdx.z;
  const uint32_t hop_first = a.hop0 + blockIdx.x * a.hops_wg;  // (the grid holds no workgroup without a hop)
  const uint32_t n_live = a.hop1 - hop_first < a.hops_wg ? a.hop1 - hop_first : a.hops_wg;
  const uint32_t j0 = wh * (uint32_t)KH;                       // the lane's first hop of the workgroup's
  const bool works = j0 < n_live;                              // (the same in every lane of a wave)
  const uint32_t pairs = a.W >> 1;
  const uint32_t pair = blockIdx.y * (kWavePairs * a.G) + wb * kWavePairs + lane;
  uint32_t pc[KB];                                             // (a pair past the last reads the last one's words)
#pragma unroll
  for (int b = 0; b < KB; b++) pc[b] = pair + 64u * (uint32_t)b < pairs ? pair + 64u * (uint32_t)b : pairs - 1u;
  double acc[KH][KB][2];
#pragma unroll
  for (int q = 0; q < KH; q++)
#pragma unroll
    for (int b = 0; b < KB; b++) acc[q][b][0] = 0.0, acc[q][b][1] = 0.0;
  TableTurn<KB> next;
  if (works) ask<KB>(next, a.tab, 0u, a.W, pc);
  const float* row_src = SYN ? a.masked : a.src[ch];
  for (uint32_t i0 = 0; i0 < a.W; i0 += a.chunk) {
    const uint32_t kc = a.chunk;                               // (W is a multiple of the chunk)
    if (!SYN) {
      // hop j of the workgroup at words [j H, j H + kc): range frames (hop_first + j - lead) H + i0 + k
      const uint32_t words = (a.hops_wg - 1u) * a.stride + kc;
      const long long g0 = ((long long)hop_first - (long long)a.lead) * (long long)a.H + (long long)i0;
      for (uint32_t s = tid; s < words; s += kLanes) {
        const long long g = g0 + (long long)s;
        float v = 0.0f;
        if (g >= 0 && g < (long long)a.n) {
          v = row_src[g];
          if (!finite_bits(v)) v = 0.0f;
        }
        span[s] = v;
      }
    } else {
      const uint32_t words = a.hops_wg * a.stride;             // stride == chunk
      for (uint32_t s = tid; s < words; s += kLanes) {
        const uint32_t j = s / a.stride, k = s - j * a.stride;
        float v = 0.0f;
        if (j < n_live) v = row_src[((size_t)(hop_first + j - a.row0) * a.channels + ch) * a.W + i0 + k];
        span[s] = v;
      }
    }
    __syncthreads();
    if (works) {
      const float* hp = span + j0 * a.stride;
      for (uint32_t k = 0; k < kc; k += 4u) {
        const TableTurn<KB> cur = next;
        f4 hv[KH];
#pragma unroll
        for (int q = 0; q < KH; q++) hv[q] = *reinterpret_cast<const f4*>(hp + (uint32_t)q * a.stride + k);
        ask<KB>(next, a.tab, i0 + k + 4u, a.W, pc);
#pragma unroll
        for (int t = 0; t < 4; t++) {
          double c[KB][2];
#pragma unroll
          for (int b = 0; b < KB; b++) c[b][0] = (double)cur.v[t][b][0], c[b][1] = (double)cur.v[t][b][1];
#pragma unroll
          for (int q = 0; q < KH; q++) {
            const double d = (double)hv[q][t];
#pragma unroll
            for (int b = 0; b < KB; b++) {
              acc[q][b][0] = fma(d, c[b][0], acc[q][b][0]);
              acc[q][b][1] = fma(d, c[b][1], acc[q][b][1]);
            }
          }
        }
      }
    }
    __syncthreads();                                           // every lane is done with the span before the next chunk lands
  }
  if (!works) return;
#pragma unroll
  for (int q = 0; q < KH; q++) {
    const uint32_t hop = hop_first + j0 + (uint32_t)q;
    if (hop >= a.hop1) continue;
    const size_t row = ((size_t)(hop - a.row0) * a.channels + ch) * a.W;
#pragma unroll
    for (int b = 0; b < KB; b++) {
      const uint32_t at = pair + 64u * (uint32_t)b;
      if (at >= pairs) continue;
      if (SYN) *reinterpret_cast<d2*>(a.chain + row + 2u * at) = d2{acc[q][b][0], acc[q][b][1]};
      else *reinterpret_cast<f2*>(a.cells + row + 2u * at) = f2{__double2float_rn(acc[q][b][0]), __double2float_rn(acc[q][b][1])};
    }
  }
}

// the cell of bin k out of a cell row: im of bins 0 and B - 1 is +0.0 and not stored
__device__ __forceinline__ void cell_of(const float* row, uint32_t k, uint32_t B, float* r, float* i) {
  const bool edge = k == 0u || k == B - 1u;
  const uint32_t w = k == 0u ? 0u : k == B - 1u ? 1u : 2u * k;
  *r = row[w];
  *i = edge ? 0.0f : row[w + 1u];
}
__device__ __forceinline__ double power_of(float r, float i) {
  return __dadd_rn(__dmul_rn((double)r, (double)r), __dmul_rn((double)i, (double)i));
}

__global__ void __launch_bounds__(kLanes) denoise_gate_kernel(DenArgs a) {
  constexpr uint32_t kWide = kDenGateBins + 2u * kDenMaxSmoothBins;
  __shared__ double p[(2u * kDenMaxSmoothHops + 1u) * kWide];
  __shared__ uint32_t open[kLanes];
  const uint32_t tid = threadIdx.x;
  const uint32_t t = a.hop0 + blockIdx.x, ch = blockIdx.z, k0 = blockIdx.y * kDenGateBins;
  const uint32_t rows = 2u * a.S + 1u, wide = kDenGateBins + 2u * a.F;
  for (uint32_t s = tid; s < rows * wide; s += kLanes) {
    const uint32_t r = s / wide, col = s - r * wide;
    const int tp = (int)t - (int)a.S + (int)r, kp = (int)k0 - (int)a.F + (int)col;
    double v = 0.0;
    if (tp >= 0 && tp < (int)a.T && kp >= 0 && kp < (int)a.B) {
      float re, im;
      cell_of(a.cells + ((size_t)((uint32_t)tp - a.row0) * a.channels + ch) * a.W, (uint32_t)kp, a.B, &re, &im);
      v = power_of(re, im);
    }
    p[r * kWide + col] = v;
  }
  __syncthreads();
  const uint32_t k = k0 + tid;
  uint32_t mine = 0;
  if (k < a.B) {
    double q = 0.0;
    for (uint32_t r = 0; r < rows; r++)
      for (uint32_t f = 0; f <= 2u * a.F; f++) q = __dadd_rn(q, p[r * kWide + tid + f]);
    const uint32_t t_lo = t > a.S ? t - a.S : 0u, t_hi = t + a.S < a.T ? t + a.S : a.T - 1u;
    const uint32_t k_lo = k > a.F ? k - a.F : 0u, k_hi = k + a.F < a.B ? k + a.F : a.B - 1u;
    q = __ddiv_rn(q, (double)((t_hi - t_lo + 1u) * (k_hi - k_lo + 1u)));
    const double th = a.thr[ch * a.B + k];
    double g = a.floor;
    if (q > th) {
      const double v = __dsub_rn(1.0, __ddiv_rn(th, q));
      if (v > a.floor) g = v;
      mine = t >= a.own0 && t < a.own1 ? 1u : 0u;
    }
    const size_t row = ((size_t)(t - a.row0) * a.channels + ch) * a.W;
    float re, im;
    cell_of(a.cells + row, k, a.B, &re, &im);
    const float mr = __double2float_rn(__dmul_rn(g, (double)re)), mi = __double2float_rn(__dmul_rn(g, (double)im));
    float* m = a.masked + row;
    if (k == 0u) m[0] = mr;
    else if (k == a.B - 1u) m[a.W - 1u] = mr;
    else m[2u * k - 1u] = mr, m[2u * k] = mi;
  }
  open[tid] = mine;
  __syncthreads();
  for (uint32_t s = kLanes / 2u; s > 0u; s >>= 1) {
    if (tid < s) open[tid] += open[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = open[0];
}

__global__ void __launch_bounds__(kLanes) denoise_fold_kernel(DenArgs a) {
  __shared__ unsigned long long red[kLanes];
  const uint32_t tid = threadIdx.x;
  unsigned long long mine = 0;
  for (uint32_t i = tid; i < a.n_part; i += kLanes) mine += a.part[i];
  red[tid] = mine;
  __syncthreads();
  for (uint32_t s = kLanes / 2u; s > 0u; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) *a.total += red[0];
}

__global__ void __launch_bounds__(kLanes) denoise_ola_kernel(DenArgs a) {
  const uint32_t ch = blockIdx.y;
  const unsigned long long x = (unsigned long long)a.blk0 * a.H + 4ull * ((unsigned long long)blockIdx.x * kLanes + threadIdx.x);
  const unsigned long long end = (unsigned long long)a.blk1 * a.H < a.n ? (unsigned long long)a.blk1 * a.H : a.n;
  if (x >= end) return;
  const uint32_t t0 = (uint32_t)(x / a.H), r = (uint32_t)(x - (unsigned long long)t0 * a.H);
  d4 sum;
#pragma unroll
  for (uint32_t u = 0; u < 4u; u++) {
    const double* row = a.chain + ((size_t)(t0 + u - a.row0) * a.channels + ch) * a.W + r + (3u - u) * a.H;
    const d4 v = *reinterpret_cast<const d4*>(row);
    if (u == 0u) sum = v;
    else
#pragma unroll
      for (int e = 0; e < 4; e++) sum[e] = __dadd_rn(sum[e], v[e]);
  }
  float* out = a.dst[ch] + x;
  if (x + 4u <= end) {
    *reinterpret_cast<f4*>(out) = f4{__double2float_rn(sum[0]), __double2float_rn(sum[1]), __double2float_rn(sum[2]), __double2float_rn(sum[3])};
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (x + (unsigned)e < end) out[e] = __double2float_rn(sum[e]);
  }
}

__global__ void __launch_bounds__(kLanes) denoise_profile_kernel(DenArgs a) {
  const uint32_t at = blockIdx.x * kLanes + threadIdx.x;
  if (at >= a.channels * a.B) return;
  const uint32_t ch = at / a.B, k = at - ch * a.B;
  double sum = a.sums[at];
  for (uint32_t h = a.hop0; h < a.hop1; h++) {
    float re, im;
    cell_of(a.cells + ((size_t)(h - a.row0) * a.channels + ch) * a.W, k, a.B, &re, &im);
    sum = __dadd_rn(sum, power_of(re, im));
  }
  a.sums[at] = sum;
}

}  // namespace

void launch_denoise_transform(const DenArgs& a, bool synthesis, hipStream_t s) {
  const uint32_t tile = 64u * a.K * a.G;
  const dim3 grid((a.hop1 - a.hop0 + a.hops_wg - 1u) / a.hops_wg, (a.W / 2u + tile - 1u) / tile, a.channels), block(kLanes);
  if (a.K == 1u) {
    if (synthesis) hipLaunchKernelGGL((denoise_transform_kernel<true, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((denoise_transform_kernel<false, 1>), grid, block, 0, s, a);
  } else {
    if (synthesis) hipLaunchKernelGGL((denoise_transform_kernel<true, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((denoise_transform_kernel<false, 2>), grid, block, 0, s, a);
  }
}
void launch_denoise_gate(const DenArgs& a, hipStream_t s) {
  const dim3 grid(a.hop1 - a.hop0, (a.B + kDenGateBins - 1u) / kDenGateBins, a.channels);
  hipLaunchKernelGGL(denoise_gate_kernel, grid, dim3(kLanes), 0, s, a);
}
void launch_denoise_fold(const DenArgs& a, hipStream_t s) { hipLaunchKernelGGL(denoise_fold_kernel, dim3(1), dim3(kLanes), 0, s, a); }
void launch_denoise_ola(const DenArgs& a, hipStream_t s) {
  const uint64_t quads = ((uint64_t)(a.blk1 - a.blk0) * a.H + 3u) / 4u;
  hipLaunchKernelGGL(denoise_ola_kernel, dim3((uint32_t)((quads + kLanes - 1u) / kLanes), a.channels), dim3(kLanes), 0, s, a);
}
void launch_denoise_profile(const DenArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(denoise_profile_kernel, dim3((a.channels * a.B + kLanes - 1u) / kLanes), dim3(kLanes), 0, s, a);
}

// ---- layer 1: the checks (no device call), the runs -----------------------------------------------------------------------------

namespace {
wbx_status denoise_check_clip(const ClipSrc* src, uint64_t first, uint64_t n, bool replaces, const char** why) {
  if (!src) return *why = "clip denoise: unknown source clip", WBX_ERR_INVALID;
  if (first > src->frames || n > src->frames - first) return *why = "clip denoise: the range ends past the clip", WBX_ERR_INVALID;
  if (replaces) return *why = "clip denoise: the result may not replace its source", WBX_ERR_INVALID;
  if (src->format != (uint32_t)WBX_FMT_F32) return *why = "clip denoise: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src->channels < 1 || src->channels > 2) return *why = "clip denoise: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}
// how many rows of thr the check reads: the clip's channels where it is known and served, else 1
uint32_t thr_rows(const ClipSrc* src) { return src && src->channels == 2 ? 2u : 1u; }

// the two tables of W on the device (kept while W stays the same)
hipError_t denoise_tables_device(DenStage& z, uint32_t W, hipStream_t on) {
  if (z.tab_w == W) return hipSuccess;
  z.tab_w = 0;                                                 // (no tables until these have been uploaded)
  const size_t words = (size_t)W * W;
  hipError_t e = z.d_tab.ensure(2u * words);
  if (e != hipSuccess) return e;
  std::vector<float> h(2u * words);
  denoise_device_tables(W, h.data(), h.data() + words);
  e = hipMemcpyAsync(z.d_tab.p, h.data(), 2u * words * sizeof(float), hipMemcpyHostToDevice, on);
  const hipError_t w = hipStreamSynchronize(on);               // (h leaves with this scope)
  if (e == hipSuccess) e = w;
  if (e == hipSuccess) z.tab_w = W;
  return e;
}

void denoise_shape_into(DenArgs& a, uint32_t W, uint32_t channels) {
  const DenShape sh = denoise_shape(W);
  a.W = W, a.H = W / 4u, a.B = W / 2u + 1u, a.channels = channels;
  a.K = sh.K, a.G = sh.G, a.hops_wg = sh.hops_wg, a.chunk = sh.chunk;
}
}  // namespace

wbx_status denoise_check(const ClipSrc* src, bool replaces, const DenCall& k, const char** why) {
  const wbx_status st = denoise_check_args(k, thr_rows(src), why);
  if (st != WBX_OK) return st;
  return denoise_check_clip(src, k.first_frame, k.n_frames, replaces, why);
}
wbx_status denoise_profile_check(const ClipSrc* src, uint64_t first_frame, uint64_t n_frames, uint32_t window, bool has_sums, bool has_hops,
                                 const char** why) {
  const wbx_status st = denoise_profile_check_args(n_frames, window, has_sums, has_hops, why);
  if (st != WBX_OK) return st;
  return denoise_check_clip(src, first_frame, n_frames, false, why);
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status denoise_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const DenCall& k, ClipSlot& slot, wbx_denoise_stats* out,
                       std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.n_frames, why);
  if (st != WBX_OK) return st;
  DenStage& z = c->den;
  const uint32_t W = k.window, H = W / 4u, B = W / 2u + 1u, C = src.channels;
  const uint32_t T = (uint32_t)denoise_hops(k.n_frames, W), blocks = T - kDenLead;
  const uint32_t per = denoise_band_hops(W, C), cap = per + kDenBandSlack;
  const size_t stage = (size_t)(blocks < per ? blocks + kDenBandSlack : cap) * C * W;
  const uint32_t gate_tiles = (B + kDenGateBins - 1u) / kDenGateBins;
  const size_t parts = (size_t)(blocks < per ? blocks + kDenLead : per + kDenLead) * gate_tiles * C;
  DenArgs a{};
  denoise_shape_into(a, W, C);
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % C];
  }
  a.n = (uint32_t)k.n_frames;
  a.S = k.smooth_hops, a.F = k.smooth_bins, a.T = T, a.lead = kDenLead;
  a.floor = k.floor;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : z.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess) e = denoise_tables_device(z, W, on);
  if (e == hipSuccess) e = z.d_cells.ensure(stage);
  if (e == hipSuccess) e = z.d_masked.ensure(stage);
  if (e == hipSuccess) e = z.d_chain.ensure(stage);
  if (e == hipSuccess) e = z.d_thr.ensure((size_t)C * B);
  if (e == hipSuccess) e = z.h_thr.ensure((size_t)C * B);
  if (e == hipSuccess) e = z.d_part.ensure(parts + 1u);
  if (e == hipSuccess) e = z.h_total.ensure(1);
  uint32_t bands = 0;
  if (e == hipSuccess) {
    std::memcpy(z.h_thr.p, k.thr, (size_t)C * B * sizeof(double));
    a.cells = z.d_cells.p, a.masked = z.d_masked.p, a.chain = z.d_chain.p, a.thr = z.d_thr.p, a.part = z.d_part.p;
    e = hipEventRecord(z.mark[0], on);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_thr.p, z.h_thr.p, (size_t)C * B * sizeof(double), hipMemcpyHostToDevice, on);
  a.total = z.d_part.p + parts;                                // (behind the greatest count of partials a band has)
  if (e == hipSuccess) e = hipMemsetAsync(a.total, 0, sizeof(unsigned long long), on);
  // a band: blocks [b0, b1) lie under hops [b0, b1 + 3), whose boxes reach S hops further on either side
  for (uint32_t b0 = 0; b0 < blocks && e == hipSuccess; b0 += per, bands++) {
    const uint32_t b1 = blocks - b0 < per ? blocks : b0 + per;
    const uint32_t s0 = b0, s1 = b1 + kDenLead;                // <= T
    const uint32_t a0 = s0 > a.S ? s0 - a.S : 0u, a1 = s1 + a.S < T ? s1 + a.S : T;
    a.row0 = a0;
    a.tab = z.d_tab.p, a.hop0 = a0, a.hop1 = a1, a.stride = H;
    launch_denoise_transform(a, false, on);
    a.hop0 = s0, a.hop1 = s1;
    a.own0 = s0, a.own1 = b1 == blocks ? T : b1;               // the next band counts hops b1 .. b1 + 2
    a.n_part = (s1 - s0) * gate_tiles * C;
    launch_denoise_gate(a, on);
    launch_denoise_fold(a, on);
    a.tab = z.d_tab.p + (size_t)W * W, a.stride = a.chunk;
    launch_denoise_transform(a, true, on);
    a.blk0 = b0, a.blk1 = b1;
    launch_denoise_ola(a, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_total.p, z.d_part.p + parts, sizeof(unsigned long long), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip denoise", e);
  }
  z.timed = true;
  if (out) {
    out->hops = T;
    out->cells = (uint64_t)T * B * C;
    out->open_cells = z.h_total.p[0];
    out->bands = bands;
    out->reserved = 0;
  }
  return WBX_OK;
}

// a measurement: launches of whole stages of hops, each followed by the walk that adds its powers to the running sums
wbx_status denoise_profile_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, uint32_t window, double* sums_out,
                               uint64_t* hops_out, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  DenStage& z = c->den;
  const uint32_t W = window, B = W / 2u + 1u, C = src.channels;
  const uint32_t hops = (uint32_t)denoise_profile_hops(n_frames, W), per = denoise_profile_band_hops(W, C);
  const size_t stage = (size_t)(hops < per ? hops : per) * C * W, count = (size_t)C * B;
  DenArgs a{};
  denoise_shape_into(a, W, C);
  for (uint32_t i = 0; i < 2; i++) a.src[i] = clip_row(src, i) + first_frame;
  a.n = (uint32_t)n_frames;
  a.T = hops, a.lead = 0;
  a.stride = a.H;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : z.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  if (e == hipSuccess) e = denoise_tables_device(z, W, on);
  if (e == hipSuccess) e = z.d_cells.ensure(stage);
  if (e == hipSuccess) e = z.d_sums.ensure(count);
  if (e == hipSuccess) e = z.h_sums.ensure(count);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess) e = hipMemsetAsync(z.d_sums.p, 0, count * sizeof(double), on);   // (all bits zero: +0.0)
  a.tab = z.d_tab.p, a.cells = z.d_cells.p, a.sums = z.d_sums.p;
  for (uint32_t h0 = 0; h0 < hops && e == hipSuccess; h0 += per) {
    a.row0 = a.hop0 = h0;
    a.hop1 = hops - h0 < per ? hops : h0 + per;
    launch_denoise_transform(a, false, on);
    launch_denoise_profile(a, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_sums.p, z.d_sums.p, count * sizeof(double), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still read the clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) return stage_fail(why, WBX_ERR_DEVICE, "clip denoise profile", e);
  z.timed = true;
  std::memcpy(sums_out, z.h_sums.p, count * sizeof(double));
  *hops_out = hops;
  return WBX_OK;
}

}  // namespace wbx

extern "C" uint64_t wbx_denoise_hops(uint64_t n_frames, uint32_t window_frames) { return wbx::denoise_hops(n_frames, window_frames); }
extern "C" uint64_t wbx_denoise_profile_hops(uint64_t n_frames, uint32_t window_frames) {
  return wbx::denoise_profile_hops(n_frames, window_frames);
}
extern "C" uint32_t wbx_denoise_band_hops(uint32_t window_frames, uint32_t channels) { return wbx::denoise_band_hops(window_frames, channels); }
extern "C" uint64_t wbx_denoise_launches(uint64_t n_frames, uint32_t window_frames, uint32_t channels) {
  return wbx::denoise_launches(n_frames, window_frames, channels);
}
extern "C" wbx_status wbx_denoise_tables(uint32_t window_frames, float* analysis_out, float* synthesis_out) {
  return wbx::denoise_tables(window_frames, analysis_out, synthesis_out);
}
extern "C" wbx_status wbx_denoise_threshold(const double* sums, uint64_t hops, size_t count, double strength, double* out) {
  return wbx::denoise_threshold(sums, hops, count, strength, out);
}
extern "C" wbx_status wbx_denoise_check(uint64_t n_frames, uint32_t window_frames, uint32_t smooth_hops, uint32_t smooth_bins, const double* thr,
                                        uint32_t channels, double floor) {
  const wbx::DenCall k{0, n_frames, window_frames, smooth_hops, smooth_bins, thr, floor};
  const char* msg = "";
  return wbx::denoise_check_args(k, channels == 2u ? 2u : 1u, &msg);
}

extern "C" wbx_status wbx_denoise_ms(wbx_ctx* c, double* out) {
  return stage_ms(c, &wbx_ctx::den, "denoise time: no denoise call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_denoise_profile(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                                               double* sums_out, uint64_t* hops_out) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  const ClipSrc src = s ? clip_src(*s) : ClipSrc{};
  const char* msg = "";
  const wbx_status st = denoise_profile_check(s ? &src : nullptr, first_frame, n_frames, window_frames, sums_out != nullptr, hops_out != nullptr, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return denoise_profile_run(c, src, first_frame, n_frames, window_frames, sums_out, hops_out, why); });
}

extern "C" wbx_status wbx_clip_denoise(wbx_ctx* c, uint32_t src_clip, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                                       uint32_t smooth_hops, uint32_t smooth_bins, const double* thr, double floor, uint32_t dst_clip,
                                       wbx_denoise_stats* stats) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, src_clip);
  ClipSrc src{};
  uint32_t rate = 0;
  if (s) src = clip_src(*s), rate = s->d.sample_rate;
  const DenCall k{first_frame, n_frames, window_frames, smooth_hops, smooth_bins, thr, floor};
  const char* msg = "";
  const wbx_status st = denoise_check(s ? &src : nullptr, dst_clip == src_clip, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  if (dst_clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) { return denoise_run(c, src, rate, k, slot, stats, why); });
}
