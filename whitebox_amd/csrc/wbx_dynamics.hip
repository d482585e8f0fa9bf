// wbx_dynamics.hip — dynamics_curve_kernel, dynamics_apply_kernel and dynamics_reduce_kernel: a frame range of a resident
// planar F32 clip through a table-driven compressor / expander / gate / ducker into a new planar F32 clip (wbx.h "Dynamics
// of a clip"), and layer 1's calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/dynamics_model.py.  The kernels
// take the shape of wbx_limit.hip's (read that file's head for the tiles, the segments, the sliding register window, the
// padded LDS rows and the vote): with curve frame m = j + A and term t = k + A
//     compress   y[m] = min(1.0, min over t of want[m - t] + table[t])
//     gate       y[m] = max(lo,  max over t of want[m - t] - table[t]),          m in [0, n + A), t in [0, A + H + R)
// want being `rest` (1.0 / lo) outside [0, n).  Minimum and maximum are exact and independent of order, every term is one
// fp64 addition (the gate's subtraction is an addition with a negated operand), so any walk of the terms gives the model's
// bits.  What differs from the limiter:
//   staging   a staged value is want = tab(p): the level p from coalesced 4-B loads of the DETECTOR's channels (the key's,
//             or the source's own), then two dependent 8-B gathers from the 24.6 KB table in global memory (it stays in
//             L2 / the vector cache; LDS is full of the row) and three fp64 operations.  4095 lookups per 2048 x 2048 terms
//   the vote  raised by a staged value that differs from rest; a segment without one changes nothing in either sense
//   padding   the ramp's padding of 2.0 neither lowers a minimum (want + 2.0 > 1.0) nor raises a maximum (want - 2.0 < 0 <= lo)
//   apply     no need[i]: the ascending window sum, one division, two multiplications (gain, makeup), one rounding
// The stage of (2^20 + A) doubles, the cached ramp, the bands and their tiles are the limiter's own (LimitStage,
// wbx_limit.h): one edit runs at a time.  Nothing here is shared with wbx_limit.hip in code.
#include "wbx_ctx.h"

namespace wbx {

namespace {

constexpr uint32_t kT = kLimitTile, kP = kLimitSegment;
constexpr uint32_t kRow = kT + kP;                             // staged words of the curve kernel: kT + kP - 1 and one never used
constexpr uint32_t kApplyRow = kT + kLimitMaxLookahead + 8u;   // ... of the apply kernel: the tile, A + 1 rounded up to 8
constexpr uint32_t kReduceMax = 512;                           // apply tiles of a band
static_assert(kT == 256 * 8 && kP % 32 == 0 && kLimitBand % kT == 0 && kLimitBand / kT == kReduceMax);
typedef double d2v __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr uint32_t phys(uint32_t w) { return w + ((w >> 3) << 1); }   // where logical word w lives

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// the detector's p at range frame g (inside [0, n))
template <int DCH>
__device__ __forceinline__ double level_in(const DynArgs& a, uint32_t g) {
  double p = 0.0;
#pragma unroll
  for (int c = 0; c < DCH; c++) {
    const float v = a.det[c][g];
    p = fmax(p, fabs(__dmul_rn(a.det_gain, finite_bits(v) ? (double)v : 0.0)));
  }
  return p;
}

// want = tab(p), p >= 0 and finite: wbx_dynamics.h's dynamics_lookup.  idx <= 47 * 64 + 63, so idx + 1 <= kDynTable - 1
__device__ __forceinline__ double lookup(const double* __restrict__ tab, double p) {
  if (p < 0x1p-40) return tab[0];
  if (p >= 256.0) return tab[kDynTable - 1u];
  const uint64_t u = (uint64_t)__double_as_longlong(p), m = u & ((1ull << 52) - 1u);
  const uint32_t idx = ((uint32_t)(u >> 52) - (uint32_t)(1023 + kDynMinExp)) * kDynCells + (uint32_t)(m >> 46);
  const double f = __dmul_rn((double)(long long)(m & ((1ull << 46) - 1u)), 0x1p-46);
  const double lo = tab[idx], hi = tab[idx + 1u];
  return __dadd_rn(lo, __dmul_rn(f, __dsub_rn(hi, lo)));
}

// logical words w .. w + 7 (w a multiple of 8), as four 16-B reads
__device__ __forceinline__ void load_words(const double* xs, uint32_t w, double (&out)[8]) {
  const d2v* p = reinterpret_cast<const d2v*>(xs + phys(w));
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const d2v v = p[i];
    out[2 * i] = v[0];
    out[2 * i + 1] = v[1];
  }
}
// 8 consecutive ramp entries: a wave-uniform address, so they arrive in scalar registers.  Read as 64-bit integers, so that
// these loads alias none of the kernel's accesses to doubles
typedef long long ramp_word;
__device__ __forceinline__ void load_ramp(const ramp_word* hp, double (&h)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) h[t] = __longlong_as_double(hp[t]);
}
// terms kk0 .. kk0 + 7 on the lane's 8 frames: lo = words b - 8 .. b - 1, hi = words b .. b + 7; frame i at term kk0 + t
// reads word b - 1 + i - t.  A term's 8 sums, then their 8 extrema (wbx_limit.hip's order)
template <int SENSE>
__device__ __forceinline__ void terms8(double (&acc)[8], const double (&h)[8], const double (&lo)[8], const double (&hi)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) {
    double s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int q = 7 + i - t;
      const double w = q < 8 ? lo[q] : hi[q - 8];
      s[i] = SENSE == WBX_DYN_GATE ? __dsub_rn(w, h[t]) : __dadd_rn(w, h[t]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = SENSE == WBX_DYN_GATE ? fmax(acc[i], s[i]) : fmin(acc[i], s[i]);
  }
}

template <int DCH, int SENSE>
__global__ void __launch_bounds__(256) dynamics_curve_kernel(DynArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[phys(kRow)];
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = blockIdx.x * kT;                         // the tile's first curve frame within the band's stage
  const int64_t m0 = (int64_t)a.band0 + (int64_t)q0;           // ... as a curve frame of the call (m = j + A)
  // the vote: three flags taken in turn, in the padding behind the last group of 8 words (wbx_limit.hip)
  int* vote = reinterpret_cast<int*>(&xs[phys(kRow) - 2u]);
  if (tid < 3u) vote[tid] = 0;
  __syncthreads();
  uint32_t turn = 0;
  const ramp_word* __restrict__ ramp = reinterpret_cast<const ramp_word*>(a.ramp);
  const double* __restrict__ tab = a.tab;
  const double rest = a.rest;
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = rest;
  for (uint32_t k0 = 0; k0 < a.l_pad; k0 += kP) {
    const int64_t lo = m0 - (int64_t)k0 - (int64_t)(kP - 1u);  // the frame of the range that word 0 holds (may be < 0)
    if (lo + (int64_t)(kRow - 2u) < 0 || lo >= (int64_t)a.n) continue;   // (workgroup-uniform) no frame of the range in reach
    int moved = 0;
    for (uint32_t s = tid; s < kRow; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      double want = rest;
      if (g >= 0 && g < (int64_t)a.n) want = lookup(tab, level_in<DCH>(a, (uint32_t)g));
      moved |= want != rest;
      xs[phys(s)] = want;
    }
    if (moved) vote[turn] = 1;
    __syncthreads();
    const bool any = __builtin_amdgcn_readfirstlane(vote[turn]) != 0;   // (workgroup-uniform, and known to be)
    if (tid == 0) vote[turn == 0u ? 2u : turn - 1u] = 0;
    turn = turn == 2u ? 0u : turn + 1u;
    // a multiple of 32, or no turn at all where nothing in reach can move the curve (skipped by the trip count)
    const uint32_t seg = any ? min(kP, a.l_pad - k0) : 0u;
    uint32_t b = 8u * tid + kP;                                // the word of frame 0 at term kk0 - 1: 8 tid - kk0 + P
    double s0[8], s1[8], s2[8], s3[8], h0[8], h1[8];
    load_words(xs, b, s3);                                     // words b .. b + 7 (the last is never used)
    load_words(xs, b - 8u, s0);
    const ramp_word* __restrict__ hp = ramp + k0;
    load_ramp(hp, h0);
    for (uint32_t kk0 = 0; kk0 < seg; kk0 += 32u, hp += 32, b -= 32u) {
      load_words(xs, b - 16u, s1);
      load_ramp(hp + 8, h1);
      terms8<SENSE>(acc, h0, s0, s3);
      load_words(xs, b - 24u, s2);
      load_ramp(hp + 16, h0);
      terms8<SENSE>(acc, h1, s1, s0);
      load_words(xs, b - 32u, s3);
      load_ramp(hp + 24, h1);
      terms8<SENSE>(acc, h0, s2, s1);
      load_words(xs, (b < 40u ? 40u : b) - 40u, s0);           // (the segment's last turn asks for words nobody uses)
      load_ramp(hp + 32, h0);                                  // (... and the call's last for the 8 doubles behind the table)
      terms8<SENSE>(acc, h1, s3, s2);
    }
    __syncthreads();                                           // the next segment's staging overwrites xs
  }
  const uint32_t q = q0 + 8u * tid;
  const uint32_t count = a.band_n + a.A;                       // curve frames of this band
  if (q >= count) return;
  double* out = a.y + q;
  if (count - q >= 8u) {
#pragma unroll
    for (int i = 0; i < 4; i++) reinterpret_cast<d2v*>(out)[i] = d2v{acc[2 * i], acc[2 * i + 1]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++)
      if ((uint32_t)i < count - q) out[i] = acc[i];
  }
}

__device__ __forceinline__ void merge(DynPartial& a, const DynPartial& b) {
  if (b.min_gain < a.min_gain || (b.min_gain == a.min_gain && b.min_gain_frame < a.min_gain_frame)) {
    a.min_gain = b.min_gain;
    a.min_gain_frame = b.min_gain_frame;
  }
  a.reduced_frames += b.reduced_frames;
}
__device__ __forceinline__ DynPartial nothing() { return DynPartial{2.0, ~0ull, 0ull}; }

// red[0 .. 255] folded into red[0] (every lane of the workgroup calls it)
__device__ __forceinline__ void fold(DynPartial* red, uint32_t tid) {
  for (uint32_t step = 128u; step > 0u; step >>= 1) {
    __syncthreads();
    if (tid < step) {
      DynPartial m = red[tid];
      merge(m, red[tid + step]);
      red[tid] = m;
    }
  }
  __syncthreads();
}

// lo = words w .. w + 7, hi = words w + 8 .. w + 15: frame f adds word w + f + t for t = 0 .. 7 ascending; terms t >= keep
// are +0.0 (MASK: the window's last block), which changes no sum that is not negative
template <bool MASK>
__device__ __forceinline__ void sums8(double (&acc)[8], const double (&lo)[8], const double (&hi)[8], uint32_t keep) {
#pragma unroll
  for (int t = 0; t < 8; t++)
#pragma unroll
    for (int f = 0; f < 8; f++) {
      const int q = f + t;
      const double v = q < 8 ? lo[q] : hi[q - 8];
      acc[f] = __dadd_rn(acc[f], MASK ? ((uint32_t)t < keep ? v : 0.0) : v);
    }
}

template <int CH>
__global__ void __launch_bounds__(256) dynamics_apply_kernel(DynArgs a) {
  __shared__ __attribute__((aligned(16))) double ys[phys(kApplyRow)];
  __shared__ DynPartial red[256];
  const uint32_t tid = threadIdx.x;
  const uint32_t t0 = blockIdx.x * kT;                         // the tile's first output frame within the band
  const uint32_t window = a.A + 1u, count = a.band_n + a.A;    // curve frames per gain / in the stage
  const uint32_t span = kT + ((window + 7u) & ~7u);            // words staged: output frame t0 + f reads words f .. f + A
  for (uint32_t s = tid; s < span; s += 256u) ys[phys(s)] = t0 + s < count ? a.y[t0 + s] : 0.0;
  __syncthreads();
  double acc[8], lo[8], hi[8];
#pragma unroll
  for (int f = 0; f < 8; f++) acc[f] = 0.0;
  uint32_t w = 8u * tid;
  load_words(ys, w, lo);
  const uint32_t whole = window & ~7u;
  uint32_t u0 = 0;
  for (; u0 + 16u <= whole; u0 += 16u, w += 16u) {             // two blocks per turn, the two sets swapping roles
    load_words(ys, w + 8u, hi);
    sums8<false>(acc, lo, hi, 8u);
    load_words(ys, w + 16u, lo);
    sums8<false>(acc, hi, lo, 8u);
  }
  if (u0 < whole) {
    load_words(ys, w + 8u, hi);
    sums8<false>(acc, lo, hi, 8u);
    w += 8u;
#pragma unroll
    for (int i = 0; i < 8; i++) lo[i] = hi[i];
  }
  if (window & 7u) {
    load_words(ys, w + 8u, hi);
    sums8<true>(acc, lo, hi, window & 7u);
  }
  const uint32_t i0 = a.band0 + t0 + 8u * tid;                 // the lane's first frame of the range
  DynPartial mine = nothing();
  float y[CH][8];
  const double width = (double)window;
#pragma unroll
  for (int f = 0; f < 8; f++) {
    const uint32_t i = i0 + (uint32_t)f;
    if (i < a.n) {
      const double g = __ddiv_rn(acc[f], width);
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float x = a.src[c][i];
        const double d = __dmul_rn(a.drive, finite_bits(x) ? (double)x : 0.0);
        const float v = __double2float_rn(__dmul_rn(__dmul_rn(d, g), a.makeup));
        y[c][f] = v != v ? __uint_as_float(kCanonNaN) : v;
      }
      if (g < mine.min_gain) mine.min_gain = g, mine.min_gain_frame = i;   // (ascending frames: the first stays)
      mine.reduced_frames += g < 1.0 ? 1u : 0u;
    } else {
#pragma unroll
      for (int c = 0; c < CH; c++) y[c][f] = 0.0f;
    }
  }
  if (i0 < a.n) {
    const uint32_t left = a.n - i0;
#pragma unroll
    for (int c = 0; c < CH; c++) {
      float* out = a.dst[c] + i0;
      if (left >= 8u) {
        __builtin_nontemporal_store(f4v{y[c][0], y[c][1], y[c][2], y[c][3]}, reinterpret_cast<f4v*>(out));
        __builtin_nontemporal_store(f4v{y[c][4], y[c][5], y[c][6], y[c][7]}, reinterpret_cast<f4v*>(out + 4));
      } else {                                                 // the result's last lane: only the frames inside it
#pragma unroll
        for (int f = 0; f < 8; f++)
          if ((uint32_t)f < left) out[f] = y[c][f];
      }
    }
  }
  red[tid] = mine;
  fold(red, tid);
  if (tid == 0) a.part[blockIdx.x] = red[0];
}

// a band's tiles into the call's record (band 0 starts it)
__global__ void __launch_bounds__(256) dynamics_reduce_kernel(DynArgs a, uint32_t n_tiles) {
  __shared__ DynPartial red[256];
  const uint32_t tid = threadIdx.x;
  DynPartial mine = nothing();
  for (uint32_t t = tid; t < n_tiles; t += 256u) merge(mine, a.part[t]);
  red[tid] = mine;
  fold(red, tid);
  if (tid == 0) {
    DynPartial m = red[0];
    if (a.band0 != 0u) merge(m, *a.total);
    *a.total = m;
  }
}

template <int DCH>
void launch_curve_of(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.sense == WBX_DYN_GATE) hipLaunchKernelGGL((dynamics_curve_kernel<DCH, WBX_DYN_GATE>), dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dynamics_curve_kernel<DCH, WBX_DYN_COMPRESS>), dim3(n_tiles), dim3(256), 0, s, a);
}

}  // namespace

void launch_dynamics_curve(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.det_channels == 2u) launch_curve_of<2>(a, n_tiles, s);
  else launch_curve_of<1>(a, n_tiles, s);
}
void launch_dynamics_apply(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(dynamics_apply_kernel<2>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(dynamics_apply_kernel<1>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_dynamics_reduce(const DynArgs& a, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(dynamics_reduce_kernel, dim3(1), dim3(256), 0, s, a, n_tiles);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clips
wbx_status dynamics_check(const ClipSrc& src, uint32_t src_rate, const ClipSrc* key, uint32_t key_rate, const DynCall& k, double* lo,
                          const char** why) {
  const wbx_status st = dynamics_check_args(k, lo, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32 || (key && key->format != (uint32_t)WBX_FMT_F32))
    return *why = "clip dynamics: a clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2 || (key && (key->channels < 1 || key->channels > 2)))
    return *why = "clip dynamics: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip dynamics: the range ends past the clip", WBX_ERR_INVALID;
  if (key && (k.key_first > key->frames || k.n_frames > key->frames - k.key_first))
    return *why = "clip dynamics: the key's range ends past the clip", WBX_ERR_INVALID;
  if (key && key_rate != src_rate) return *why = "clip dynamics: the key's sample rate differs from the source's", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status dynamics_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc* key, uint32_t rate, const DynCall& k, double lo, ClipSlot& slot,
                        wbx_dynamics_stats* out, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  ClipFill fill{};
  fill.kind = CLIP_SRC_NONE;   // the kernel writes every frame; clip_build clears the 16 padding frames (and the row's slack)
  wbx_status st = clip_build(c, slot, WBX_FMT_F32, src.channels, rate, k.n_frames, fill, on);
  if (st != WBX_OK) return *why = c->err, st;
  LimitStage& x = c->lim;      // the ramp and the curve's stage: the limiter's
  DynStage& z = c->dyn;
  const uint32_t A = k.lookahead, H = k.hold, R = k.release;
  const size_t terms = (size_t)limit_terms(A, H, R);
  DynArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.det[i] = key ? clip_row(*key, i) + k.key_first : a.src[i];
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.drive = k.drive;
  a.det_gain = key ? k.key_gain : k.drive;
  a.makeup = k.makeup;
  a.rest = k.sense == WBX_DYN_GATE ? lo : 1.0;
  a.n = (uint32_t)k.n_frames;
  a.A = A;
  a.l_pad = (uint32_t)((terms + 31u) & ~(size_t)31u);
  a.channels = src.channels;
  a.det_channels = key ? key->channels : src.channels;
  a.sense = k.sense;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : z.mark)
    if (e == hipSuccess) e = m.ensure(hipEventDefault);
  const size_t table = (size_t)a.l_pad + 8u;                   // (8 more: the kernel asks one block ahead)
  const bool fresh = x.ramp_of[0] != A || x.ramp_of[1] != H || x.ramp_of[2] != R;
  if (e == hipSuccess && fresh) {
    x.ramp_of[2] = 0;                                          // (no table until this one's upload has completed)
    e = x.h_ramp.ensure(table);
    if (e == hipSuccess) e = x.d_ramp.ensure(table);
    if (e == hipSuccess) {
      (void)limit_ramp(A, H, R, x.h_ramp.p, terms);
      for (size_t t = terms; t < table; t++) x.h_ramp.p[t] = kLimitRampPad;
    }
  }
  if (e == hipSuccess) e = z.h_tab.ensure(kDynTable);
  if (e == hipSuccess) e = z.d_tab.ensure(kDynTable);
  if (e == hipSuccess) std::memcpy(z.h_tab.p, k.table, kDynTable * sizeof(double));
  if (e == hipSuccess) e = x.d_y.ensure(limit_stage_doubles(A));
  if (e == hipSuccess) e = z.d_part.ensure(kReduceMax + 1u);
  if (e == hipSuccess) e = z.h_total.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(x.d_ramp.p, x.h_ramp.p, table * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_tab.p, z.h_tab.p, kDynTable * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.ramp = x.d_ramp.p;
    a.tab = z.d_tab.p;
    a.y = x.d_y.p;
    a.part = z.d_part.p;
    a.total = z.d_part.p + kReduceMax;
  }
  const uint64_t bands = limit_bands(k.n_frames);
  for (uint64_t i = 0; i < bands && e == hipSuccess; i++) {
    const LimitBand b = limit_band(k.n_frames, A, i);
    a.band0 = (uint32_t)b.first;
    a.band_n = b.frames;
    launch_dynamics_curve(a, b.curve_tiles, on);
    e = hipGetLastError();
    if (e == hipSuccess) {
      launch_dynamics_apply(a, b.apply_tiles, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      launch_dynamics_reduce(a, b.apply_tiles, on);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_total.p, a.total, sizeof(DynPartial), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip dynamics", e);
  }
  x.ramp_of[0] = A, x.ramp_of[1] = H, x.ramp_of[2] = R;
  z.timed = true;
  if (out) {
    const DynPartial& t = z.h_total.p[0];
    out->min_gain = t.min_gain;
    out->min_gain_frame = t.min_gain_frame;
    out->reduced_frames = t.reduced_frames;
  }
  if (stats) {                                                 // the measure pass over the result, on the same stream
    st = clipfx_measure_run(c, clip_src(slot), 0, k.n_frames, stats, why);
    if (st != WBX_OK) clip_release(c, slot);
  }
  return st;
}

}  // namespace wbx

extern "C" wbx_status wbx_dynamics_table(int kind, double threshold_db, double ratio, double knee_db, double range_db, double* out,
                                         size_t cap_doubles) {
  return dynamics_table(kind, threshold_db, ratio, knee_db, range_db, out, cap_doubles);
}
extern "C" wbx_status wbx_dynamics_check(const double* table, int sense, double* lo) { return dynamics_table_check(table, sense, lo); }
extern "C" wbx_status wbx_dynamics_lookup(const double* table, double level, double* out) {
  if (!table || !out || !(level >= 0.0)) return WBX_ERR_INVALID;
  *out = dynamics_lookup(table, level);
  return WBX_OK;
}

extern "C" wbx_status wbx_dynamics_ms(wbx_ctx* c, double* out) {
  if (!c || !out) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->fx_mu);
  DynStage& z = c->dyn;
  if (!z.timed) return fail(c, WBX_ERR_INVALID, "dynamics time: no dynamics call has completed on this context");
  float ms = 0.0f;
  WBX_HIP(c, hipEventElapsedTime(&ms, z.mark[0], z.mark[1]));
  *out = (double)ms;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_dynamics(wbx_ctx* c, uint32_t src_clip, uint32_t key_clip, uint32_t dst_clip, uint64_t first_frame,
                                        uint64_t n_frames, uint64_t key_first, int sense, const double* table, double drive,
                                        double key_gain, double makeup, uint32_t lookahead_frames, uint32_t hold_frames,
                                        uint32_t release_frames, wbx_dynamics_stats* dynamics_stats, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  const bool keyed = key_clip != WBX_DYN_NO_KEY;
  wbx_status st = keyed ? clipfx_check_ids(c, src_clip, key_clip, dst_clip, "clip dynamics: unknown source clip", "clip dynamics: unknown key clip",
                                           "clip dynamics: the result may not replace its source or its key")
                        : clipfx_check_ids(c, src_clip, dst_clip, "clip dynamics: unknown source clip",
                                           "clip dynamics: the result may not replace its source or its key");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  ClipSrc key{};
  uint32_t key_rate = rate;
  if (keyed) key = clip_src(c->clips[key_clip]), key_rate = c->clips[key_clip].d.sample_rate;
  const DynCall k{first_frame, n_frames, key_first, keyed, sense, table, drive, key_gain, makeup, lookahead_frames, hold_frames, release_frames};
  const char* msg = "";
  double lo = 1.0;
  st = dynamics_check(src, rate, keyed ? &key : nullptr, key_rate, k, &lo, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return dynamics_run(c, src, keyed ? &key : nullptr, rate, k, lo, slot, dynamics_stats, stats_of_result, why);
  });
}
