// wbx_gaincurve.h — what wbx_limit.hip and wbx_dynamics.hip have in common (nothing else includes it): a gain curve that is
// an extremum over a ramp table, walked into the fp64 stage; the gain as the moving average of that curve; the tiles'
// statistics folded into one record; and the host's half of such a call.  The three kernels are templates defined here.  With curve frame m = j + A and term t = k + A
//     min sense   y[m] = min(rest, min over t in [0, A + H + R) of v[m - t] + table[t])      (limiter, compress)
//     max sense   y[m] = max(rest, max over t of v[m - t] - table[t]),                        m in [0, n + A)      (gate)
// v being `rest` outside [0, n).  Minimum and maximum are exact and independent of order, every term is one fp64 addition
// (the subtraction is an addition with a negated operand), so any walk of the terms gives the models' bits; the gain's
// moving average is one ascending chain of additions per frame.  What a processor supplies are POLICIES: small structs of static functions (see each kernel).
//
// curve_kernel<P>: a workgroup of 256 lanes owns a TILE of 2048 consecutive curve frames, a lane 8 of them: 8 fp64 extrema that
// live in registers for the whole walk.  The table is walked in SEGMENTS of P = 2048 terms.  Per segment:
//   stage    the tile's frames m0 .. m0 + 2047 and the terms k0 .. k0 + P - 1 read v[m0 - k0 - P + 1 .. m0 - k0 + 2047]:
//            4095 doubles go into LDS, computed while staging by the policy.  A frame outside [0, n) is staged as `rest`
//            and NOT read.  The workgroup votes (a flag in LDS) whether the span holds any value that can move the curve;
//            where it holds none — most of a real clip lies under a limiter's ceiling — the segment is skipped, as is one
//            whose whole span lies outside the range.
//   compute  per 8 terms the lane reads the 8 doubles below its window as four 16-B words and runs 8 terms x 8 frames of
//            v_add_f64 + v_min_f64 (v_max_f64): word (8 lane + i - kk + P - 1) for frame i, term kk.  The window of 15
//            doubles slides by renaming registers: a turn of the loop is four blocks of 8 terms that take four register
//            sets in turn.  The 8 table entries are wave-uniform: read with a uniform index, they arrive in scalar
//            registers.  The next block's words and entries are asked for before this block's add / min run.
// and after the last segment the 8 extrema go to the stage as four 16-B stores (the band's last lane frame by frame).
// The table is padded to a multiple of 32 (and 8 more) with 2.0: v + 2.0 lowers no minimum that starts at 1.0 and v - 2.0
// < 0 raises no maximum, so the walk needs no tail.
//
// apply_kernel<P>: the same tiles over the band's OUTPUT frames.  The curve span of tile + A (at most 6144 doubles) goes from
// the stage into LDS; a lane runs the ascending sum of A + 1 curve frames for each of its 8 frames — the same sliding
// window, 8 additions per frame and block, the last block's surplus terms replaced by +0.0, which changes no sum that is
// not negative — and divides; the policy makes a frame's samples and statistics of that.  Whole 16-B stores, the result's
// last lane frame by frame; nothing is written at or past n.  The tile's statistics go to part[tile]; reduce_kernel (one
// workgroup) folds a band's tiles into the call's record.
//
// LDS rows of doubles: lanes stand 8 doubles = 16 dwords apart, so plain rows would put the 16-B reads of a 16-lane group on
// 16 of the 64 banks, a 4-way conflict (an 8-B read: 8-way over a 32-lane half).  Both rows therefore keep logical word w
// at double w + 2 * (w / 8): 10 doubles = 20 dwords per group of 8, still 16-B aligned, and the 16 lanes of a group start
// on 20 l mod 64 = sixteen different multiples of 4 — no conflict.  Curve: 5120 doubles, the vote inside them (40 KB, four
// workgroups per CU); apply: 7690 doubles + the statistics (two workgroups per CU).  No scratch.
//
// One call is issued in BANDS of 2^20 output frames (wbx_limit.h): curve, apply, reduce per band, back to back on the
// edits' stream, each band recomputing its A frames of halo, so the stage is (2^20 + A) doubles whatever the clip's length.
#pragma once
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
// what decided between scalar and vector loads, though, was the shape of the segment skip (see curve_kernel)
typedef long long ramp_word;
__device__ __forceinline__ void load_ramp(const ramp_word* hp, double (&h)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) h[t] = __longlong_as_double(hp[t]);
}
// terms kk0 .. kk0 + 7 on the lane's 8 frames: lo = words b - 8 .. b - 1, hi = words b .. b + 7; frame i at term kk0 + t
// reads word b - 1 + i - t.  MAX: the maximum of the differences, not the minimum of the sums
template <bool MAX>
__device__ __forceinline__ void terms8(double (&acc)[8], const double (&h)[8], const double (&lo)[8], const double (&hi)[8]) {
#pragma unroll
  for (int t = 0; t < 8; t++) {
    // a term's 8 sums, then their 8 minima: written add, min, add, min every minimum waits for the addition in front of
    // it (5 - 15 % slower at two waves per SIMD: EXPERIMENTS.md)
    double s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int q = 7 + i - t;
      const double w = q < 8 ? lo[q] : hi[q - 8];
      s[i] = MAX ? __dsub_rn(w, h[t]) : __dadd_rn(w, h[t]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = MAX ? fmax(acc[i], s[i]) : fmin(acc[i], s[i]);
  }
}

// The curve kernel.  It is the kernel itself that is shared, not a function for two kernels to call: inlined into a kernel
// of each file the same text compiled to another loop — the turn's first table entries fetched at its top and waited for
// at once, not one block ahead.  P, the policy, supplies
//   Args                      the kernel's argument block: its ramp, y, n, band0, band_n, A and l_pad are read here
//   kMax                      the sense: false = minimum of sums, true = maximum of differences
//   rest(a)                   the value of a frame outside the range, and where every extremum starts
//   staged(a, g)              the value of range frame g, g in [0, n): the policy reads its detector here
//   moved(v, rest)            whether a staged value can move the curve at all
template <class P>
__global__ void __launch_bounds__(256) curve_kernel(typename P::Args a) {
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
  const double rest = P::rest(a);
  double acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = rest;
  for (uint32_t k0 = 0; k0 < a.l_pad; k0 += kP) {
    const int64_t lo = m0 - (int64_t)k0 - (int64_t)(kP - 1u);  // the frame of the range that word 0 holds (may be < 0)
    if (lo + (int64_t)(kRow - 2u) < 0 || lo >= (int64_t)a.n) continue;   // (workgroup-uniform) no frame of the range in reach
    int moved = 0;
    for (uint32_t s = tid; s < kRow; s += 256u) {
      const int64_t g = lo + (int64_t)s;
      double v = rest;
      if (g >= 0 && g < (int64_t)a.n) v = P::staged(a, (uint32_t)g);
      moved |= P::moved(v, rest);
      xs[phys(s)] = v;
    }
    if (moved) vote[turn] = 1;
    __syncthreads();
    const bool any = __builtin_amdgcn_readfirstlane(vote[turn]) != 0;   // (workgroup-uniform, and known to be)
    if (tid == 0) vote[turn == 0u ? 2u : turn - 1u] = 0;
    turn = turn == 2u ? 0u : turn + 1u;
    // a multiple of 32, or no turn at all where nothing in reach can move the curve.  (Skipped by the trip count, not
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
      terms8<P::kMax>(acc, h0, s0, s3);
      load_words(xs, b - 24u, s2);
      load_ramp(hp + 16, h0);
      terms8<P::kMax>(acc, h1, s1, s0);
      load_words(xs, b - 32u, s3);
      load_ramp(hp + 24, h1);
      terms8<P::kMax>(acc, h0, s2, s1);
      load_words(xs, (b < 40u ? 40u : b) - 40u, s0);           // (the segment's last turn asks for words nobody uses)
      load_ramp(hp + 32, h0);                                  // (... and the call's last for the 8 doubles behind the table)
      terms8<P::kMax>(acc, h1, s3, s2);
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

// F, the fold of a partial record, supplies Partial, merge(Partial&, const Partial&) — every field merges in any order —
// and nothing(), the record of no frame.  red[0 .. 255] folded into red[0] (every lane of the workgroup calls it)
template <class F>
__device__ __forceinline__ void fold(typename F::Partial* red, uint32_t tid) {
  for (uint32_t step = 128u; step > 0u; step >>= 1) {
    __syncthreads();
    if (tid < step) {
      typename F::Partial m = red[tid];
      F::merge(m, red[tid + step]);
      red[tid] = m;
    }
  }
  __syncthreads();
}

// The apply kernel: the same tiles over the band's OUTPUT frames.  P supplies Args, Fold (see fold), kCh — the channels — and
//   frame(a, i, g, f, y, mine)    range frame i, the lane's frame f, whose curve average is g: the samples into y[c][f],
//                                 the statistics into mine
// Like the curve kernel it is the kernel itself that is shared
template <class P>
__global__ void __launch_bounds__(256) apply_kernel(typename P::Args a) {
  typedef typename P::Fold F;
  constexpr int CH = P::kCh;
  __shared__ __attribute__((aligned(16))) double ys[phys(kApplyRow)];
  __shared__ typename F::Partial red[256];
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
  typename F::Partial mine = F::nothing();
  float y[CH][8];
  const double width = (double)window;
#pragma unroll
  for (int f = 0; f < 8; f++) {
    const uint32_t i = i0 + (uint32_t)f;
    if (i < a.n) {
      P::frame(a, i, __ddiv_rn(acc[f], width), f, y, mine);
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
  fold<F>(red, tid);
  if (tid == 0) a.part[blockIdx.x] = red[0];
}

// The reduce kernel (one workgroup): a band's tiles into the call's record (band 0 starts it)
template <class F, class Args>
__global__ void __launch_bounds__(256) reduce_kernel(Args a, uint32_t n_tiles) {
  __shared__ typename F::Partial red[256];
  const uint32_t tid = threadIdx.x;
  typename F::Partial mine = F::nothing();
  for (uint32_t t = tid; t < n_tiles; t += 256u) F::merge(mine, a.part[t]);
  red[tid] = mine;
  fold<F>(red, tid);
  if (tid == 0) {
    typename F::Partial m = red[0];
    if (a.band0 != 0u) F::merge(m, *a.total);
    *a.total = m;
  }
}

}  // namespace

// ---- the host's half -------------------------------------------------------------------------------------------------------

// one band's three launches, stopping at the first that fails
template <class Args>
hipError_t launch_band(const Args& a, const LimitBand& b, hipStream_t on, void (*curve)(const Args&, uint32_t, hipStream_t),
                       void (*apply)(const Args&, uint32_t, hipStream_t), void (*reduce)(const Args&, uint32_t, hipStream_t)) {
  curve(a, b.curve_tiles, on);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    apply(a, b.apply_tiles, on);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    reduce(a, b.apply_tiles, on);
    e = hipGetLastError();
  }
  return e;
}

// What limit_run and dynamics_run do once `slot` is built and `a` holds what is the processor's own: the ramp of A, H, R
// made fresh on LimitStage where the cached one is another, the stage and z's record ensured (`e`: what became of the
// caller's own buffers), a's common fields filled in, band(b) — the three launches — for every band between z's two
// events, and the record brought back.  report(record) runs once all of it has completed, then the measure pass over the
// result on the same stream where `stats` asks for it.  The slot is released on every failure.  Z is LimitStage itself or
// DynStage: mark, timed, d_part and h_total are read here
template <class Z, class Args, class Band, class Report>
wbx_status gain_run(wbx_ctx* c, Z& z, const char* what, hipError_t e, Args& a, uint32_t A, uint32_t H, uint32_t R, uint64_t n_frames,
                    ClipSlot& slot, wbx_clip_stats* stats, std::string* why, Band&& band, Report&& report) {
  const hipStream_t on = c->fx.side.stream;
  LimitStage& x = c->lim;      // the ramp and the curve's stage: the limiter's
  const size_t terms = (size_t)limit_terms(A, H, R);
  a.n = (uint32_t)n_frames;
  a.A = A;
  a.l_pad = (uint32_t)((terms + 31u) & ~(size_t)31u);
  z.timed = false;
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
  if (e == hipSuccess) e = x.d_y.ensure(limit_stage_doubles(A));
  if (e == hipSuccess) e = z.d_part.ensure(kReduceMax + 1u);
  if (e == hipSuccess) e = z.h_total.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(x.d_ramp.p, x.h_ramp.p, table * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    a.ramp = x.d_ramp.p;
    a.y = x.d_y.p;
    a.part = z.d_part.p;
    a.total = z.d_part.p + kReduceMax;
  }
  const uint64_t bands = limit_bands(n_frames);
  for (uint64_t i = 0; i < bands && e == hipSuccess; i++) {
    const LimitBand b = limit_band(n_frames, A, i);
    a.band0 = (uint32_t)b.first;
    a.band_n = b.frames;
    e = band(b);
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_total.p, a.total, sizeof(*a.total), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, what, e);
  }
  x.ramp_of[0] = A, x.ramp_of[1] = H, x.ramp_of[2] = R;
  z.timed = true;
  report(z.h_total.p[0]);
  return clipfx_measure_result(c, slot, n_frames, stats, why);
}

}  // namespace wbx
