// wbx_limit.hip — limit_curve_kernel, limit_apply_kernel and limit_reduce_kernel: a frame range of a resident planar F32
// clip through a look-ahead peak limiter into a new planar F32 clip (wbx.h "Limiting a clip"), and layer 1's calls on top
// of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/limit_model.py.  With curve frame
// m = j + A and term t = k + A the curve is a (min, +) convolution of the same shape as wbx_convolve.hip's sum,
//     y[m] = min(1.0, min over t in [0, A + H + R) of need[m - t] + table[t]),   m in [0, n + A),
// need being 1.0 outside [0, n).  Minimum is exact and independent of order, every term is one fp64 addition, so any walk of
// the terms gives the model's bits; the gain's moving average is one ascending chain of additions per frame.
//
// limit_curve_kernel<CH>: a workgroup of 256 lanes owns a TILE of 2048 consecutive curve frames, a lane 8 of them: 8 fp64
// minima that live in registers for the whole walk.  The table is walked in SEGMENTS of P = 2048 terms.  Per segment:
//   stage    the tile's frames m0 .. m0 + 2047 and the terms k0 .. k0 + P - 1 read need[m0 - k0 - P + 1 .. m0 - k0 + 2047]:
//            4095 doubles go into LDS, computed while staging from coalesced 4-B loads of the source's channels
//            (drive, |.|, the maximum over the channels, one division where the ceiling is exceeded).  A frame outside
//            [0, n) is staged as 1.0 and NOT read.  The workgroup votes (a flag in LDS) whether the span holds any
//            value below 1.0; where it holds none — most of a real clip lies under the ceiling — the segment is skipped,
//            as is one whose whole span lies outside the range.
//   compute  per 8 terms the lane reads the 8 doubles below its window as four 16-B words and runs 8 terms x 8 frames of
//            v_add_f64 + v_min_f64: word (8 lane + i - kk + P - 1) for frame i, term kk.  The window of 15 doubles slides by
//            renaming registers: a turn of the loop is four blocks of 8 terms that take four register sets in turn.  The 8 table
//            entries are wave-uniform: read with a uniform index, they arrive in scalar registers.  The next block's words
//            and entries are asked for before this block's add / min run.
// and after the last segment the 8 minima go to the stage as four 16-B stores (the band's last lane frame by frame).
// The table is padded to a multiple of 32 (and 8 more) with 2.0: need + 2.0 can lower nothing, so the walk needs no tail.
//
// limit_apply_kernel<CH>: the same tiles over the band's OUTPUT frames.  The curve span of tile + A (at most 6144 doubles)
// goes from the stage into LDS; a lane runs the ascending sum of A + 1 curve frames for each of its 8 frames — the same
// sliding window, 8 additions per frame and block, the last block's surplus terms replaced by +0.0, which changes no
// positive sum — divides, takes the minimum with need[i] recomputed from the source, multiplies each channel and rounds
// once.  Whole 16-B stores, the result's last lane frame by frame; nothing is written at or past n.  The tile's
// wbx_limit_stats go to part[tile]; limit_reduce_kernel (one workgroup) folds a band's tiles into the call's record.
//
// LDS rows of doubles: lanes stand 8 doubles = 16 dwords apart, so plain rows would put the 16-B reads of a 16-lane group on
// 16 of the 64 banks, a 4-way conflict (an 8-B read: 8-way over a 32-lane half).  Both kernels therefore keep logical word w
// at double w + 2 * (w / 8): 10 doubles = 20 dwords per group of 8, still 16-B aligned, and the 16 lanes of a group start
// on 20 l mod 64 = sixteen different multiples of 4 — no conflict.  Curve: 5120 doubles, the vote inside them (40 KB, four
// workgroups per CU); apply: 7690 doubles + 8 KB for the statistics (68 KB, two per CU).  No scratch.
//
// One call is issued in BANDS of 2^20 output frames (wbx_limit.h): curve, apply, reduce per band, back to back on the
// edits' stream, each band recomputing its A frames of halo, so the stage is (2^20 + A) doubles whatever the clip's length.
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

// d of every channel at range frame g (inside [0, n)), and the detector's p
template <int CH>
__device__ __forceinline__ double drive_in(const LimitArgs& a, uint32_t g, double (&d)[CH]) {
  double p = 0.0;
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const float v = a.src[c][g];
    d[c] = __dmul_rn(a.drive, finite_bits(v) ? (double)v : 0.0);
    p = fmax(p, fabs(d[c]));
  }
  return p;
}
__device__ __forceinline__ double need_of(double p, double ceiling) { return p > ceiling ? __ddiv_rn(ceiling, p) : 1.0; }

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
// 8 consecutive table entries: a wave-uniform address, so they arrive in scalar registers (s_load_dwordx16).  The device
// reads the table as 64-bit integers and nothing else, so that these loads alias none of the kernel's accesses to doubles;
// what decided between scalar and vector loads, though, was the shape of the segment skip (see the kernel)
typedef long long ramp_word;
__device__ __forceinline__ void load_ramp(const ramp_word* hp, double (&h)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) h[t] = __longlong_as_double(hp[t]);
}
// terms kk0 .. kk0 + 7 on the lane's 8 frames: lo = words b - 8 .. b - 1, hi = words b .. b + 7; frame i at term kk0 + t
// reads word b - 1 + i - t
__device__ __forceinline__ void terms8(double (&acc)[8], const double (&h)[8], const double (&lo)[8], const double (&hi)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) {
    // a term's 8 sums, then their 8 minima: written add, min, add, min every minimum waits for the addition in front of
    // it (5 - 15 % slower at two waves per SIMD: EXPERIMENTS.md)
    double s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int q = 7 + i - t;
      s[i] = __dadd_rn(q < 8 ? lo[q] : hi[q - 8], h[t]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = fmin(acc[i], s[i]);
  }
}

template <int CH>
__global__ void __launch_bounds__(256) limit_curve_kernel(LimitArgs a) {
  __shared__ __attribute__((aligned(16))) double xs[phys(kRow)];
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = blockIdx.x * kT;                         // the tile's first curve frame within the band's stage
  const int64_t m0 = (int64_t)a.band0 + (int64_t)q0;           // ... as a curve frame of the call (m = j + A)
  // the vote: three flags taken in turn, in the padding behind the last group of 8 words.  A segment's staging raises its
  // flag, everybody reads it behind the barrier, and lane 0 then lowers the flag of the segment after the next — which
  // nobody reads any more and nobody raises before the next barrier
  int* vote = reinterpret_cast<int*>(&xs[phys(kRow) - 2u]);
  if (tid < 3u) vote[tid] = 0;
  __syncthreads();
  uint32_t turn = 0;
  const ramp_word* __restrict__ ramp = reinterpret_cast<const ramp_word*>(a.ramp);
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = 1.0;
  for (uint32_t k0 = 0; k0 < a.l_pad; k0 += kP) {
    const int64_t lo = m0 - (int64_t)k0 - (int64_t)(kP - 1u);  // the frame of the range that word 0 holds (may be < 0)
    if (lo + (int64_t)(kRow - 2u) < 0 || lo >= (int64_t)a.n) continue;   // (workgroup-uniform) no frame of the range in reach
    int below = 0;
    for (uint32_t s = tid; s < kRow; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      double need = 1.0;
      if (g >= 0 && g < (int64_t)a.n) {
        double d[CH];
        need = need_of(drive_in<CH>(a, (uint32_t)g, d), a.ceiling);
      }
      below |= need < 1.0;
      xs[phys(s)] = need;
    }
    if (below) vote[turn] = 1;
    __syncthreads();
    const bool any = __builtin_amdgcn_readfirstlane(vote[turn]) != 0;   // (workgroup-uniform, and known to be)
    if (tid == 0) vote[turn == 0u ? 2u : turn - 1u] = 0;
    turn = turn == 2u ? 0u : turn + 1u;
    // a multiple of 32, or no turn at all where nothing in reach can lower the curve.  (Skipped by the trip count, not
    // by a branch around the loop: behind such a branch the compiler fetches the table through vector loads)
    const uint32_t seg = any ? min(kP, a.l_pad - k0) : 0u;
    uint32_t b = 8u * tid + kP;                                // the word of frame 0 at term kk0 - 1: 8 tid - kk0 + P
    double s0[8], s1[8], s2[8], s3[8], h0[8], h1[8];
    load_words(xs, b, s3);                                     // words b .. b + 7 (the last is never used)
    load_words(xs, b - 8u, s0);
    const ramp_word* __restrict__ hp = ramp + k0;
    load_ramp(hp, h0);
    // 32 terms per turn, as four blocks of 8.  A block reads two sets of 8 words and the NEXT block's words are asked for
    // before its add / min run, which hides their latency: three sets live, four sets taken in turn, so that after four
    // blocks every set has its first role again and no register is ever copied.  The entries alternate between two sets
    for (uint32_t kk0 = 0; kk0 < seg; kk0 += 32u, hp += 32, b -= 32u) {
      load_words(xs, b - 16u, s1);
      load_ramp(hp + 8, h1);
      terms8(acc, h0, s0, s3);
      load_words(xs, b - 24u, s2);
      load_ramp(hp + 16, h0);
      terms8(acc, h1, s1, s0);
      load_words(xs, b - 32u, s3);
      load_ramp(hp + 24, h1);
      terms8(acc, h0, s2, s1);
      load_words(xs, (b < 40u ? 40u : b) - 40u, s0);           // (the segment's last turn asks for words nobody uses)
      load_ramp(hp + 32, h0);                                  // (... and the call's last for the 8 doubles behind the table)
      terms8(acc, h1, s3, s2);
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

__device__ __forceinline__ void merge(LimitPartial& a, const LimitPartial& b) {
  a.peak_in = fmax(a.peak_in, b.peak_in);
  if (b.min_gain < a.min_gain || (b.min_gain == a.min_gain && b.min_gain_frame < a.min_gain_frame)) {
    a.min_gain = b.min_gain;
    a.min_gain_frame = b.min_gain_frame;
  }
  a.limited_frames += b.limited_frames;
}
__device__ __forceinline__ LimitPartial nothing() { return LimitPartial{0.0, 2.0, ~0ull, 0ull}; }

// red[0 .. 255] folded into red[0] (every lane of the workgroup calls it)
__device__ __forceinline__ void fold(LimitPartial* red, uint32_t tid) {
  for (uint32_t step = 128u; step > 0u; step >>= 1) {
    __syncthreads();
    if (tid < step) {
      LimitPartial m = red[tid];
      merge(m, red[tid + step]);
      red[tid] = m;
    }
  }
  __syncthreads();
}

// lo = words w .. w + 7, hi = words w + 8 .. w + 15: frame f adds word w + f + t for t = 0 .. 7 ascending; terms t >= keep
// are +0.0 (MASK: the window's last block)
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
__global__ void __launch_bounds__(256) limit_apply_kernel(LimitArgs a) {
  __shared__ __attribute__((aligned(16))) double ys[phys(kApplyRow)];
  __shared__ LimitPartial red[256];
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
  LimitPartial mine = nothing();
  float y[CH][8];
  const double width = (double)window;
#pragma unroll
  for (int f = 0; f < 8; f++) {
    const uint32_t i = i0 + (uint32_t)f;
    if (i < a.n) {
      double d[CH];
      const double p = drive_in<CH>(a, i, d);
      const double g = fmin(__ddiv_rn(acc[f], width), need_of(p, a.ceiling));
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float v = __double2float_rn(__dmul_rn(d[c], g));
        y[c][f] = v != v ? __uint_as_float(kCanonNaN) : v;
      }
      mine.peak_in = fmax(mine.peak_in, p);
      if (g < mine.min_gain) mine.min_gain = g, mine.min_gain_frame = i;   // (ascending frames: the first stays)
      mine.limited_frames += g < 1.0 ? 1u : 0u;
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
__global__ void __launch_bounds__(256) limit_reduce_kernel(LimitArgs a, uint32_t n_tiles) {
  __shared__ LimitPartial red[256];
  const uint32_t tid = threadIdx.x;
  LimitPartial mine = nothing();
  for (uint32_t t = tid; t < n_tiles; t += 256u) merge(mine, a.part[t]);
  red[tid] = mine;
  fold(red, tid);
  if (tid == 0) {
    LimitPartial m = red[0];
    if (a.band0 != 0u) merge(m, *a.total);
    *a.total = m;
  }
}

}  // namespace

void launch_limit_curve(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(limit_curve_kernel<2>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(limit_curve_kernel<1>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_limit_apply(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(limit_apply_kernel<2>, dim3(n_tiles), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(limit_apply_kernel<1>, dim3(n_tiles), dim3(256), 0, s, a);
}
void launch_limit_reduce(const LimitArgs& a, uint32_t n_tiles, hipStream_t s) {
  hipLaunchKernelGGL(limit_reduce_kernel, dim3(1), dim3(256), 0, s, a, n_tiles);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status limit_check(const ClipSrc& src, const LimitCall& k, const char** why) {
  const wbx_status st = limit_check_args(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip limit: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip limit: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip limit: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status limit_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const LimitCall& k, ClipSlot& slot, wbx_limit_stats* out,
                     wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  ClipFill fill{};
  fill.kind = CLIP_SRC_NONE;   // the kernel writes every frame; clip_build clears the 16 padding frames (and the row's slack)
  wbx_status st = clip_build(c, slot, WBX_FMT_F32, src.channels, rate, k.n_frames, fill, on);
  if (st != WBX_OK) return *why = c->err, st;
  LimitStage& x = c->lim;
  const uint32_t A = k.lookahead, H = k.hold, R = k.release;
  const size_t terms = (size_t)limit_terms(A, H, R);
  LimitArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.ceiling = (double)k.ceiling;
  a.drive = k.drive;
  a.n = (uint32_t)k.n_frames;
  a.A = A;
  a.l_pad = (uint32_t)((terms + 31u) & ~(size_t)31u);
  a.channels = src.channels;
  x.timed = false;
  hipError_t e = hipSuccess;
  for (Event& m : x.mark)
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
  if (e == hipSuccess) e = x.d_y.ensure(limit_stage_doubles(A));
  if (e == hipSuccess) e = x.d_part.ensure(kReduceMax + 1u);
  if (e == hipSuccess) e = x.h_total.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(x.mark[0], on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(x.d_ramp.p, x.h_ramp.p, table * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.ramp = x.d_ramp.p;
    a.y = x.d_y.p;
    a.part = x.d_part.p;
    a.total = x.d_part.p + kReduceMax;
  }
  const uint64_t bands = limit_bands(k.n_frames);
  for (uint64_t i = 0; i < bands && e == hipSuccess; i++) {
    const LimitBand b = limit_band(k.n_frames, A, i);
    a.band0 = (uint32_t)b.first;
    a.band_n = b.frames;
    launch_limit_curve(a, b.curve_tiles, on);
    e = hipGetLastError();
    if (e == hipSuccess) {
      launch_limit_apply(a, b.apply_tiles, on);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      launch_limit_reduce(a, b.apply_tiles, on);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipEventRecord(x.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(x.h_total.p, a.total, sizeof(LimitPartial), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip limit", e);
  }
  x.ramp_of[0] = A, x.ramp_of[1] = H, x.ramp_of[2] = R;
  x.timed = true;
  if (out) {
    const LimitPartial& t = x.h_total.p[0];
    out->peak_in = t.peak_in;
    out->min_gain = t.min_gain;
    out->min_gain_frame = t.min_gain_frame;
    out->limited_frames = t.limited_frames;
  }
  if (stats) {                                                 // the measure pass over the result, on the same stream
    st = clipfx_measure_run(c, clip_src(slot), 0, k.n_frames, stats, why);
    if (st != WBX_OK) clip_release(c, slot);
  }
  return st;
}

}  // namespace wbx

extern "C" wbx_status wbx_limit_ramp(uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames, double* out,
                                     size_t cap_doubles) {
  return limit_ramp(lookahead_frames, hold_frames, release_frames, out, cap_doubles);
}
extern "C" uint32_t wbx_limit_tile_frames(void) { return kLimitTile; }
extern "C" uint32_t wbx_limit_segment_terms(void) { return kLimitSegment; }
extern "C" uint32_t wbx_limit_band_frames(void) { return kLimitBand; }

extern "C" wbx_status wbx_limit_ms(wbx_ctx* c, double* out) {
  if (!c || !out) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->fx_mu);
  LimitStage& x = c->lim;
  if (!x.timed) return fail(c, WBX_ERR_INVALID, "limit time: no limit has completed on this context");
  float ms = 0.0f;
  WBX_HIP(c, hipEventElapsedTime(&ms, x.mark[0], x.mark[1]));
  *out = (double)ms;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_limit(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                     float ceiling, double drive, uint32_t lookahead_frames, uint32_t hold_frames,
                                     uint32_t release_frames, wbx_limit_stats* limit_stats, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip limit: unknown source clip", "clip limit: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const LimitCall k{first_frame, n_frames, ceiling, drive, lookahead_frames, hold_frames, release_frames};
  const char* msg = "";
  st = limit_check(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return limit_run(c, src, rate, k, slot, limit_stats, stats_of_result, why);
  });
}
