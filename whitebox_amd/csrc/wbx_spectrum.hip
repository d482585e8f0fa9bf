// wbx_spectrum.hip — spectrum_kernel: the power of a frame range of a resident planar F32 clip at B frequencies per hop, as a
// direct transform against a basis that is itself a resident mono F32 clip (wbx.h "Seeing a clip's spectrum"), and layer 1's
// call on top of it.  A measurement: nothing is allocated in the pool.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/spectrum_model.py.
//   the mapping  a tall matrix product whose left factor is the clip read through overlapping windows.  Hops and bins are
//             independent, so the grid tiles both: x walks the launch's hops in tiles of F, y the bins in tiles of 128 G.  A
//             workgroup has 4 waves; G = 1, 2 or 4 of them stand side by side over the bins (a wave owns 128: lane l the bins
//             l and l + 64 of them, so that consecutive lanes read consecutive {C, S} pairs of the i-major basis), the 4 / G
//             rows of waves own 4 consecutive hops each: F = 16 / G hops per workgroup.  With at most 64 bins a lane's second
//             bin would lie idle: there (KB = 1) a lane owns ONE bin and 8 hops, a wave 64 bins, a workgroup 32 hops
//   the span     the window is walked in chunks of 512 terms (the whole window where it is shorter).  A chunk's detector
//             values of the workgroup's F hops are staged in LDS as FLOATS, what is not finite zeroed while staging, frames
//             at or past n as 0 (only hops past the launch's last read them): hops lie H words apart and share their words
//             where H is below the chunk, else chunk words apart, each with its own (H > W leaves gaps that are never read).
//             At most 16 x 512 (KB = 1: 32 x 256) words = 32 KB, whatever W and H: a large hop length costs no hops per
//             workgroup
//   the chains   a lane owns 4 hops x 2 bins (or 8 x 1): 16 fp64 accumulators (re and im of each).  It walks a chunk in turns of
//             four terms: four 16-byte LDS reads (one per hop, the same address in every lane of the wave: a broadcast) and eight
//             8-byte global reads of the basis (512 contiguous bytes per wave and read; the table is at most 16 MB and every
//             workgroup reads it, so it stays in L2 / the Infinity Cache), the basis words asked for one turn ahead of their
//             fma run.  Both factors of every product are fp32 values, so the product is exact in fp64 and fma(d, c, re) IS
//             the model's re + d * c.  A hop's offset in the span is a multiple of H, so only a hop length that is a
//             multiple of 4 (or one of at least a chunk) keeps the 16-byte reads aligned: the other instance (AL = false)
//             reads word by word
//   the count    per turn and lane: 4 terms x 4 hops x 2 bins x {re, im} = 64 fma for 64 LDS bytes (broadcast), 64 global
//             bytes and 32 float-to-double conversions (16 of the span, 16 of the basis).  f0_kernel's turn has 64 fma per 16
//             LDS bytes and 8 conversions: its operands slide along one array, here every fma row meets a fresh basis word.
//             The conversions share the fp64 pipe with the fma: 96 issue slots per 64 fma, two thirds of the rate at best.
//             KB = 1: 64 fma for 128 LDS bytes, 32 global bytes and 40 conversions
//   the epilogue p = re * re + im * im (rounded products, a rounded sum) in the lane that holds both chains, one float per
//             cell.  No cross-lane sums, no atomics, no scratch; nothing waits on another workgroup.
#include "wbx_ctx.h"

#include <cstring>

namespace wbx {

namespace {

constexpr uint32_t kLanes = kSpecLanes;
static_assert(kLanes == 64u * kSpecWaves && kSpecLaneCells == 8);
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double sample_in(float v) { return finite_bits(v) ? (double)v : 0.0; }

// the detector d[g] for a frame g of the range, g < n ("Tracking a clip's pitch"'s)
template <bool MID>
__device__ __forceinline__ float detector(const SpecArgs& a, uint32_t g) {
  if (!MID) return finite_bits(a.src[0][g]) ? a.src[0][g] : 0.0f;
  return __double2float_rn(__dmul_rn(0.5, __dadd_rn(sample_in(a.src[0][g]), sample_in(a.src[1][g]))));
}

template <bool AL>
__device__ __forceinline__ f4 ld4(const float* p) {
  if (AL) return *reinterpret_cast<const f4*>(p);
  return f4{p[0], p[1], p[2], p[3]};
}

template <int KB>
struct BasisTurn {
  f2 v[4][KB];                 // {C, S} of terms i .. i + 3 at the lane's bins
};
// the basis words of terms i .. i + 3 (rows past the window's last read that one again: asked for ahead, never used)
template <int KB>
__device__ __forceinline__ void ask(BasisTurn<KB>& t, const float* basis, uint32_t i, uint32_t W, uint32_t B, const uint32_t (&bc)[KB]) {
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const uint32_t row = i + k < W ? i + k : W - 1u;
    const f2* p = reinterpret_cast<const f2*>(basis) + (size_t)row * B;   // (row B + b) 2 words: 8-byte pairs
#pragma unroll
    for (int b = 0; b < KB; b++) t.v[k][b] = p[bc[b]];
  }
}

// KB bins per lane (the lane's own and, KB = 2, the one 64 further) x KH = 8 / KB consecutive hops
template <bool MID, bool AL, int KB>
__global__ void __launch_bounds__(kLanes) spectrum_kernel(SpecArgs a) {
  constexpr int KH = (int)kSpecLaneCells / KB;
  constexpr uint32_t kWaveBins = 64u * KB;
  __shared__ __attribute__((aligned(16))) float span[kSpecSpanWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t wb = wave % a.G, wh = wave / a.G;             // the wave's column of bins, its row of hops
  const uint32_t hop_first = a.hop0 + blockIdx.x * a.F;        // (the grid holds no workgroup without a hop)
  const uint32_t n_live = a.hop1 - hop_first < a.F ? a.hop1 - hop_first : a.F;
  const uint32_t j0 = wh * (uint32_t)KH;                       // the lane's first hop of the workgroup's
  const bool works = j0 < n_live;                              // (the same in every lane of a wave)
  const uint32_t bin = blockIdx.y * (kWaveBins * a.G) + wb * kWaveBins + lane;   // the lane's bins: bin (and bin + 64)
  uint32_t bc[KB];                                             // (a bin past B reads the last one's words)
#pragma unroll
  for (int b = 0; b < KB; b++) bc[b] = bin + 64u * (uint32_t)b < a.B ? bin + 64u * (uint32_t)b : a.B - 1u;
  const uint64_t t0 = (uint64_t)hop_first * a.H;               // < n: the hop is complete
  const bool share = a.stride == a.H;                          // the hops' words are one run of frames
  double re[KH][KB], im[KH][KB];
#pragma unroll
  for (int q = 0; q < KH; q++)
#pragma unroll
    for (int b = 0; b < KB; b++) re[q][b] = 0.0, im[q][b] = 0.0;
  BasisTurn<KB> next;
  if (works) ask<KB>(next, a.basis, 0u, a.W, a.B, bc);
  for (uint32_t i0 = 0; i0 < a.W; i0 += a.chunk) {
    const uint32_t kc = a.W - i0 < a.chunk ? a.W - i0 : a.chunk;   // terms of this chunk, a multiple of 4
    // hop j of the workgroup at words [j stride, j stride + kc): frames t0 + j H + i0 + k.  (F - 1) stride + chunk words at most
    if (share) {
      const uint32_t words = (a.F - 1u) * a.stride + kc;
      for (uint32_t s = tid; s < words; s += kLanes) {
        const uint64_t g = t0 + i0 + s;
        span[s] = g < (uint64_t)a.n ? detector<MID>(a, (uint32_t)g) : 0.0f;
      }
    } else {
      const uint32_t words = a.F * a.stride;                   // stride == chunk >= kc
      for (uint32_t s = tid; s < words; s += kLanes) {
        const uint32_t j = s / a.stride, k = s - j * a.stride;
        const uint64_t g = t0 + (uint64_t)j * a.H + i0 + k;
        span[s] = (k < kc && g < (uint64_t)a.n) ? detector<MID>(a, (uint32_t)g) : 0.0f;
      }
    }
    __syncthreads();
    if (works) {
      const float* hp = span + j0 * a.stride;
      for (uint32_t k = 0; k < kc; k += 4u) {
        const BasisTurn<KB> cur = next;
        f4 hv[KH];
#pragma unroll
        for (int q = 0; q < KH; q++) hv[q] = ld4<AL>(hp + (uint32_t)q * a.stride + k);
        ask<KB>(next, a.basis, i0 + k + 4u, a.W, a.B, bc);
#pragma unroll
        for (int t = 0; t < 4; t++) {
          double c[KB], s[KB];
#pragma unroll
          for (int b = 0; b < KB; b++) c[b] = (double)cur.v[t][b][0], s[b] = (double)cur.v[t][b][1];
#pragma unroll
          for (int q = 0; q < KH; q++) {
            const double d = (double)hv[q][t];
#pragma unroll
            for (int b = 0; b < KB; b++) {
              re[q][b] = fma(d, c[b], re[q][b]);
              im[q][b] = fma(d, s[b], im[q][b]);
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
    float* row = a.out + (size_t)(hop - a.hop0) * a.B;
#pragma unroll
    for (int b = 0; b < KB; b++) {
      const uint32_t at = bin + 64u * (uint32_t)b;
      if (at >= a.B) continue;
      const double p = __dadd_rn(__dmul_rn(re[q][b], re[q][b]), __dmul_rn(im[q][b], im[q][b]));
      row[at] = __double2float_rn(p);
    }
  }
}

template <int KB>
void launch_bins(const SpecArgs& a, const dim3& grid, hipStream_t s) {
  const dim3 block(kLanes);
  const bool al = a.stride % 4u == 0u;
  if (a.mid) {
    if (al) hipLaunchKernelGGL((spectrum_kernel<true, true, KB>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((spectrum_kernel<true, false, KB>), grid, block, 0, s, a);
  } else {
    if (al) hipLaunchKernelGGL((spectrum_kernel<false, true, KB>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((spectrum_kernel<false, false, KB>), grid, block, 0, s, a);
  }
}

}  // namespace

void launch_spectrum(const SpecArgs& a, hipStream_t s) {
  const uint32_t tile_bins = 64u * a.K * a.G;
  const dim3 grid((a.hop1 - a.hop0 + a.F - 1u) / a.F, (a.B + tile_bins - 1u) / tile_bins);
  if (a.K == 1u) launch_bins<1>(a, grid, s);
  else launch_bins<2>(a, grid, s);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the source, then the basis (null: unknown)
wbx_status spectrum_check_call(const ClipSrc& src, const ClipSrc* basis, const SpecCall& k, const char** why) {
  const wbx_status st = spectrum_check(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip spectrum: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip spectrum: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.channel == 1u && src.channels < 2) return *why = "clip spectrum: channel 1 of a mono clip", WBX_ERR_INVALID;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip spectrum: the range ends past the clip", WBX_ERR_INVALID;
  if (!basis) return *why = "clip spectrum: unknown basis clip", WBX_ERR_INVALID;
  if (basis->format != (uint32_t)WBX_FMT_F32) return *why = "clip spectrum: the basis clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (basis->channels != 1) return *why = "clip spectrum: the basis clip is not mono", WBX_ERR_UNSUPPORTED;
  if (basis->frames != spectrum_basis_frames(k.window, k.bins))
    return *why = "clip spectrum: the basis clip does not have 2 x n_bins x window_frames frames", WBX_ERR_INVALID;
  return WBX_OK;
}

wbx_status spectrum_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc& basis, const SpecCall& k, float* power_out, wbx_spectrum_info* info,
                        std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  SpecStage& z = c->spec;
  const uint64_t hops = spectrum_hops(k.n_frames, k.window, k.hop);
  const uint32_t per_launch = spectrum_launch_hops(k.window, k.bins);
  const SpecShape shape = spectrum_shape(k.window, k.bins, k.hop);
  const size_t stage = (size_t)(hops < per_launch ? hops : per_launch) * k.bins;   // <= kSpecStageCells
  z.timed = false;
  z.ms = 0.0;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  if (e == hipSuccess && hops) e = z.d_cells.ensure(stage);
  if (e == hipSuccess && hops) e = z.h_cells.ensure(stage);
  SpecArgs a{};
  const bool mid = k.channel == WBX_SPECTRUM_MID && src.channels == 2;
  a.src[0] = clip_row(src, mid ? 0u : (k.channel == 1u ? 1u : 0u)) + k.first_frame;
  a.src[1] = clip_row(src, 1) + k.first_frame;
  a.basis = clip_row(basis, 0);
  a.out = z.d_cells.p;
  a.n = (uint32_t)k.n_frames;
  a.W = k.window, a.B = k.bins, a.H = k.hop;
  a.K = shape.K, a.G = shape.G, a.F = shape.F;
  a.chunk = shape.chunk, a.stride = shape.stride;
  a.mid = mid ? 1u : 0u;
  uint64_t launches = 0;
  // a launch, its cells to pinned memory, the wait, the cells to the caller: the stage holds one launch's cells
  for (uint64_t h = 0; h < hops && e == hipSuccess; h += per_launch) {
    a.hop0 = (uint32_t)h;
    a.hop1 = (uint32_t)(h + per_launch < hops ? h + per_launch : hops);
    const size_t cells = (size_t)(a.hop1 - a.hop0) * k.bins;
    e = hipEventRecord(z.mark[0], on);
    if (e == hipSuccess) {
      launch_spectrum(a, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
    if (e == hipSuccess) e = hipMemcpyAsync(z.h_cells.p, z.d_cells.p, cells * sizeof(float), hipMemcpyDeviceToHost, on);
    const hipError_t w = hipStreamSynchronize(on);             // (also after a failure: nothing may still read the clips)
    if (e == hipSuccess) e = w;
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, z.mark[0], z.mark[1]);
    if (e != hipSuccess) break;
    z.ms += (double)ms;
    std::memcpy(power_out + (size_t)h * k.bins, z.h_cells.p, cells * sizeof(float));
    launches++;
  }
  if (e != hipSuccess) return stage_fail(why, WBX_ERR_DEVICE, "clip spectrum", e);
  z.timed = true;
  if (info) {
    info->hops = hops;
    info->bins = k.bins;
    info->launches = (uint32_t)launches;
  }
  return WBX_OK;
}

}  // namespace wbx

extern "C" uint64_t wbx_spectrum_hops(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames) {
  return wbx::spectrum_hops(n_frames, window_frames, hop_frames);
}
extern "C" wbx_status wbx_spectrum_check(uint64_t n_frames, uint32_t channel, uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames,
                                         int has_power_out, size_t cells_cap) {
  const wbx::SpecCall k{0, n_frames, channel, window_frames, n_bins, hop_frames, has_power_out != 0, cells_cap};
  const char* msg = "";
  return wbx::spectrum_check(k, &msg);
}
extern "C" uint64_t wbx_spectrum_max_cells(void) { return wbx::kSpecMaxCells; }
extern "C" uint64_t wbx_spectrum_launch_terms(void) { return wbx::kSpecLaunchTerms; }
extern "C" uint32_t wbx_spectrum_launch_hops(uint32_t window_frames, uint32_t n_bins) { return wbx::spectrum_launch_hops(window_frames, n_bins); }
extern "C" uint64_t wbx_spectrum_basis_frames(uint32_t window_frames, uint32_t n_bins) { return wbx::spectrum_basis_frames(window_frames, n_bins); }
extern "C" wbx_status wbx_spectrum_basis(uint32_t window_frames, uint32_t n_bins, const double* freqs, const uint32_t* lengths,
                                         int window_kind, double kaiser_beta, float* out) {
  const char* msg = "";
  return wbx::spectrum_basis(window_frames, n_bins, freqs, lengths, window_kind, kaiser_beta, out, &msg);
}
extern "C" wbx_status wbx_spectrum_log_freqs(double f_min, double bins_per_octave, uint32_t n_bins, double* out, uint32_t* clamped) {
  const char* msg = "";
  return wbx::spectrum_log_freqs(f_min, bins_per_octave, n_bins, out, clamped, &msg);
}

extern "C" wbx_status wbx_spectrum_ms(wbx_ctx* c, double* out) {
  using namespace wbx;
  if (!c || !out) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->fx_mu);
  const SpecStage& z = c->spec;
  if (!z.timed) return fail(c, WBX_ERR_INVALID, "spectrum time: no spectrum call has completed on this context");
  *out = z.ms;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_spectrum(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t channel,
                                        uint32_t basis_clip, uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames,
                                        float* power_out, size_t cells_cap, wbx_spectrum_info* info) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "clip spectrum: unknown clip");
  const ClipSrc src = clip_src(*s);
  const ClipSlot* bs = find_clip(c, basis_clip);
  const ClipSrc basis = bs ? clip_src(*bs) : ClipSrc{};
  const SpecCall k{first_frame, n_frames, channel, window_frames, n_bins, hop_frames, power_out != nullptr, cells_cap};
  const char* msg = "";
  const wbx_status st = spectrum_check_call(src, bs ? &basis : nullptr, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_reading(c, [&](std::string* why) { return spectrum_run(c, src, basis, k, power_out, info, why); });
}
