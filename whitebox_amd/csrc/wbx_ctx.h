// wbx_ctx.h — internals shared by the translation units of libwbx.so's host side (wbx_runtime.hip: layer 1,
// wbx_engine.hip: layer 2, wbx_dist.hip: multi-GPU).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <mutex>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/wbx.h"
#include "wbx_dev.h"
#include "wbx_shape.h"
#include "wbx_convolve.h"
#include "wbx_filter.h"
#include "wbx_dynamics.h"
#include "wbx_limit.h"
#include "wbx_loudness.h"
#include "wbx_resample.h"
#include "wbx_saturate.h"
#include "wbx_varispeed.h"
#include "wbx_splice.h"
#include "wbx_stretch.h"
#include "wbx_warp.h"
#include "wbx_pitch.h"
#include "wbx_f0.h"
#include "wbx_align.h"
#include "wbx_spectrum.h"
#include "wbx_denoise.h"
#include "wbx_onset.h"
#include "wbx_pool.h"
#include "wbx_res.h"

namespace wbx {
void launch_plan(const PlanArgs& a, hipStream_t s);
void launch_times_copy(const DBlockTime* host_pinned, DBlockTime* dev, uint32_t n_blocks, uint32_t* zero_counters, hipStream_t s);
void launch_gen(const GenArgs& a, uint32_t max_grid, hipStream_t s);
void launch_plan_segments(const PlanArgs& a, const SegArgs& g, bool beside, hipStream_t s);
const char* launch_mix(const MixInstance& inst, const MixArgs& a, uint32_t grid_z, hipStream_t s, hipEvent_t t0 = nullptr,
                       hipEvent_t t1 = nullptr);   // -> the instance's name, null: not compiled in
void launch_sum(const SumArgs& a, uint32_t n_blocks, hipStream_t s);
// the one-block callback as one launch (wbx_callback.h): sequencer + mix + sum + completion flag -> the instance's name
const char* launch_callback(const MixInstance& inst, const MixArgs& m, const PlanArgs& p, const SumArgs& s, uint32_t* done, uint32_t done_base, uint32_t done_base2,
                            bool spread, uint32_t* gave_up, uint32_t spin_bound, uint32_t* flag, uint32_t seq, unsigned long long* dbg, hipStream_t st);
void launch_clamp(float* buf, size_t n, hipStream_t s);
void launch_clamp_into(const float* src, float* dst, size_t n, int clamp, hipStream_t s);
void launch_convert(const float* master, void* dst, uint32_t n_blocks, uint32_t F, uint32_t C, int fmt, hipStream_t s);
void launch_synth(void* dst, uint64_t frames, uint64_t key, float amp, int fmt, hipStream_t s);
void launch_levels_take(uint32_t* levels, uint32_t* dst, uint32_t n, hipStream_t s);
bool probe_xcd_layout(hipStream_t s, uint32_t* n_xcds);   // workgroup ids round-robin over 8 / 4 / 2 / 1 XCDs? (wbx_kernels.hip)
void launch_deinterleave(const void* src, void* dst0, void* dst1, uint64_t frames, uint32_t channels, uint32_t elem,
                         hipStream_t s);
// recording (wbx_record.hip): one staged input block -> the chunks of every take that records it
struct RecChunk {
  uint32_t* ch[2];             // the chunk's channel rows (F32 samples moved as words)
};
struct RecCaptureArgs {
  const uint32_t* stage;       // pinned: [in_channels][frames] samples of the block
  const uint32_t* desc;        // pinned, beside them: [n_takes] ch0 << 2 | channels, 0 = skip the take this block
  const RecChunk* table;       // device: [n_takes][table_cap] chunk rows
  uint64_t start;              // the takes' frame of the block's first frame
  uint32_t frames, in_channels, n_takes, table_cap, chunk_frames;
};
void launch_record_capture(const RecCaptureArgs& a, hipStream_t s);
// bouncing (wbx_bounce.hip): the blocks of one render pass -> the destination clips of the signals asked for
struct StemSrc {               // one signal of a bounce (32 B, read as eight broadcast dwords)
  float* dst[2];               // the destination clip's channel rows (planar, frame 0); mono: dst[1] unused
  uint32_t kind, index, tap;   // WBX_BOUNCE_* / track or bus index / WBX_TAP_*
  uint32_t _pad;
};
static_assert(sizeof(StemSrc) == 32, "StemSrc must be 32 bytes");
struct StemArgs {
  const StemSrc* src;          // device: [n_src]
  const DRow* rows;            // the pass's plan: [n_blocks][n_tracks] rows, their templates, the overflow pool
  const DTrackBlock* tmpl;
  const DSeg* pool;
  const float* gains;          // device: [n_tracks][2] fl(volume * pan_coeffs[c]), the pass's gain row
  const float* master;         // the pass's results: [n_blocks][C][F] (clamped), [n_blocks][n_buses][C][F]; null: silence
  const float* buses;
  uint64_t first_frame;        // destination frame of the pass's first block
  uint64_t n_frames;           // frames of every destination clip: what lies past them is dropped
  uint32_t n_src, n_blocks, n_tracks, n_buses, block_frames, channels;
  uint32_t tmpl_cap, pool_chunks;
};
void launch_stem(const StemArgs& a, hipStream_t s);
// exporting (wbx_export.hip): one staging chunk of a planar F32 clip -> interleaved samples of a device format
struct ExportArgs {
  const float* src[2];         // the channel rows at the chunk's first frame (4-byte aligned; mono: src[1] unused)
  void* dst;                   // the chunk's samples, 16-byte aligned: [n_frames][channels]
  uint32_t* stats;             // device: peak bits [2], samples beyond +-1 [2], NaNs [2] — zero before the launch
  uint32_t n_frames;           // <= kExportChunkMax
  uint32_t channels, format, flags;   // 1 or 2 / WBX_OUT_* / WBX_EXPORT_*
};
void launch_export(const ExportArgs& a, hipStream_t s);
// editing clips (wbx_clipfx.hip): a frame range of a planar F32 clip measured, or derived into a new planar F32 clip
struct ClipFxStats {           // the device's statistics block (80 B), per output channel
  unsigned long long peak[2];  // (bits of max |x|) << 32 | ~(its first frame): one 64-bit integer max; 0: the peak is 0
  double sum[2], sum_sq[2];    // over the samples that are no NaN
  uint32_t mn[2], mx[2];       // order-preserving keys of the signed extremes; initially 0xFFFFFFFF / 0
  uint32_t over[2], nans[2];
};
struct ClipFxArgs {
  const float* src[2];         // the source's channel rows at the CLIP's frame 0, as the channel mode orders them
  float* dst[2];               // the new clip's rows (256-B aligned); dst[0] null: measure only
  ClipFxStats* stats;          // device, holding the initial image
  uint32_t first_frame, n_frames;   // the range; n_frames < 2^31 - 16
  uint32_t fade_in, fade_out, shape_in, shape_out;   // frames (<= n_frames) / WBX_FADE_*
  float gain;
  uint32_t reversed, src_channels, out_channels;   // src_channels: rows read (LEFT / RIGHT read one)
};
void launch_clipfx(const ClipFxArgs& a, hipStream_t s);
// what clipfx_kernel and splice_kernel share: the vector words, the stored NaN and the fade weight of wbx.h "Editing clips"
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at a 4-byte aligned address
typedef float f4v __attribute__((ext_vector_type(4)));               // a 16-B word of output
constexpr uint32_t kCanonNaN = 0x7FC00000u;
__device__ __forceinline__ float fade_weight(uint32_t k, uint32_t len, uint32_t shape) {
  const float t = __double2float_rn(__ddiv_rn((double)k, (double)len));
  if (shape == (uint32_t)WBX_FADE_LINEAR) return t;
  const float tt = __fmul_rn(t, t);
  if (shape == (uint32_t)WBX_FADE_SQUARE) return tt;
  return __fmul_rn(tt, __fsub_rn(3.0f, __fmul_rn(2.0f, t)));   // WBX_FADE_SMOOTH
}
// converting a clip's sample rate (wbx_resample.hip): a frame range of a planar F32 clip -> a new planar F32 clip
struct ResampleArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const float* table;          // device: the coefficients in phase-visit order, [T][L]: row r holds phase (r * M) mod L
  uint32_t n_in, n_out;        // frames of the range / of the result, both < 2^31 - 16
  uint32_t L, M, H, T;         // the plan (wbx_resample.h)
  uint32_t channels;           // 1 or 2
  uint32_t tile, span, n_tiles;   // filled by launch_resample: outputs per tile, floats staged per channel and tile, tiles
};
void launch_resample(ResampleArgs a, hipStream_t s);
// reading a clip along a position curve (wbx_varispeed.hip): a frame range of a planar F32 clip -> a new planar F32 clip
struct VsArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const float* table;          // device: [P][row] — row p holds h[p][k], D[p][k] pairs, k ascending (16-B aligned rows)
  const long long* knots;      // device: [K]
  const wbx_varispeed_tile* tiles;   // device: [n_tiles]
  uint32_t n_in, n_out;        // frames of the range / of the result, both < 2^31 - 16
  uint32_t n_tiles;
  uint32_t H, T, row;          // the plan (wbx_varispeed.h); row: floats of one table row
  uint32_t g, s;               // knot_shift; 32 - log2 P
  uint32_t channels;           // 1 or 2
};
void launch_varispeed(const VsArgs& a, uint32_t lds_bytes, hipStream_t s);
// measuring a clip's loudness (wbx_loudness.hip): hop energies behind the K filter, and the oversampled peak
struct LoudnessArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  double* energy;              // device: [channels][hops]
  double coef[10];             // wbx_loudness.h: stage 1's b0 b1 b2 a1 a2, stage 2's
  uint32_t hop, hops;          // frames per hop (800 .. 38400) / complete hops of the range (>= 1; hops * hop < 2^31)
  uint32_t channels;           // 1 or 2
};
void launch_loudness(const LoudnessArgs& a, hipStream_t s);
struct TruePeakArgs {
  const float* src[2];         // as above
  const float* table;          // device: resample_kernel's table for rate -> factor * rate, [T][L]
  uint32_t* peak;              // device: bits of the largest |value| per channel — zero before the launch
  uint32_t n_in;               // frames of the range; n_in * L < 2^31 - 16
  uint32_t L, H, T;            // the plan: factor (4 or 2), 24, 48
  uint32_t channels;
};
void launch_true_peak(const TruePeakArgs& a, hipStream_t s);
// filtering a clip (wbx_filter.hip): zero-state runs per chunk, the serial carry over them, the runs from the carried states
struct FilterArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  double* state;               // device: [n_chunks - 1][channels][D] — z_j, which the carry overwrites with t_{j+1}
  const double* M;             // device: the carry matrix, [D][D] (wbx_filter.h)
  double coef[5 * kFilterMaxStages];   // [stages][b0 b1 b2 a1 a2]
  uint32_t n_in, n_out;        // frames of the range / of the result (n_in + tail), n_out < 2^31 - 16
  uint32_t n_chunks;           // ceil(n_out / 512)
  uint32_t channels, stages;   // 1 or 2 / 1 .. 8
};
void launch_filter_state(const FilterArgs& a, hipStream_t s);   // (n_chunks > 1)
void launch_filter_carry(const FilterArgs& a, hipStream_t s);   // (n_chunks > 1)
void launch_filter_apply(const FilterArgs& a, hipStream_t s);
// convolving a clip (wbx_convolve.hip): the response sanitised into doubles once, then bands of tiles of the result
struct ConvolveArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  const float* ir[2];          // the response's channel rows at ITS range's first frame (mono: ir[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  double* taps;                // device: [ir_channels][l_pad] — the response as doubles, what is not finite as 0.0, zero-padded (and 8 more behind)
  double gain;
  uint64_t out_first;          // full-result frame of stored frame 0 (< 2^32 + 2^20)
  uint32_t n_in, n_ir, n_out;  // frames of the source range / of the response range / of the result (< 2^31 - 16)
  uint32_t l_pad;              // n_ir rounded up to a multiple of 16
  uint32_t tile0;              // this launch's first tile (the grid is its band of tiles)
  uint32_t src_channels, ir_channels;   // 1 or 2 each
};
void launch_convolve_taps(const ConvolveArgs& a, hipStream_t s);
void launch_convolve(const ConvolveArgs& a, uint32_t n_tiles, hipStream_t s);   // tiles [tile0, tile0 + n_tiles)
// limiting a clip (wbx_limit.hip): per band the gain curve into the fp64 stage, then gain, product and partial statistics
struct LimitPartial {          // what one tile (or the whole call so far) knows of wbx_limit_stats; every field merges in any order
  double peak_in;              // the largest p
  double min_gain;             // the smallest g ...
  uint64_t min_gain_frame;     // ... and the first frame that has it
  uint64_t limited_frames;     // frames with g < 1.0
};
struct LimitArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const double* ramp;          // device: [l_pad + 8] — the ramp table, kLimitRampPad from its last term on
  double* y;                   // device: the stage, curve frame band0 - A + q at [q], q < band_n + A
  LimitPartial* part;          // device: [apply tiles of a band]
  LimitPartial* total;         // device: the call's record, merged band by band
  double ceiling, drive;
  uint32_t n;                  // frames of the range (< 2^31 - 16)
  uint32_t band0, band_n;      // this band's first output frame and its output frames
  uint32_t A;                  // look-ahead
  uint32_t l_pad;              // A + H + R rounded up to a multiple of 32
  uint32_t channels;           // 1 or 2
};
void launch_limit_curve(const LimitArgs& a, uint32_t n_tiles, hipStream_t s);
void launch_limit_apply(const LimitArgs& a, uint32_t n_tiles, hipStream_t s);
void launch_limit_reduce(const LimitArgs& a, uint32_t n_tiles, hipStream_t s);   // part[0 .. n_tiles) into *total
// dynamics of a clip (wbx_dynamics.hip): the limiter's shape — per band the gain curve into the limiter's fp64 stage, then
// gain, product and partial statistics — with a table lookup where the limiter divides
struct DynPartial {            // what one tile (or the whole call so far) knows of wbx_dynamics_stats; every field merges in any order
  double min_gain;             // the smallest g ...
  uint64_t min_gain_frame;     // ... and the first frame that has it
  uint64_t reduced_frames;     // frames with g < 1.0
};
struct DynArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  const float* det[2];         // the detector's rows at its first frame: the key's, or the source's again
  float* dst[2];               // the new clip's rows (256-B aligned)
  const double* ramp;          // device: [l_pad + 8] — the limiter's ramp table, kLimitRampPad from its last term on
  const double* tab;           // device: [kDynTable] — the transfer table
  double* y;                   // device: the stage, curve frame band0 - A + q at [q], q < band_n + A
  DynPartial* part;            // device: [apply tiles of a band]
  DynPartial* total;           // device: the call's record, merged band by band
  double drive, det_gain, makeup;   // det_gain: key_gain, or the drive again
  double rest;                 // 1.0 (compress) or the table's smallest entry (gate)
  uint32_t n;                  // frames of the range (< 2^31 - 16)
  uint32_t band0, band_n;      // this band's first output frame and its output frames
  uint32_t A;                  // look-ahead
  uint32_t l_pad;              // A + H + R rounded up to a multiple of 32
  uint32_t channels;           // the source's: 1 or 2
  uint32_t det_channels;       // the detector's: 1 or 2
  int sense;                   // WBX_DYN_COMPRESS or WBX_DYN_GATE
};
void launch_dynamics_curve(const DynArgs& a, uint32_t n_tiles, hipStream_t s);
void launch_dynamics_apply(const DynArgs& a, uint32_t n_tiles, hipStream_t s);
void launch_dynamics_reduce(const DynArgs& a, uint32_t n_tiles, hipStream_t s);   // part[0 .. n_tiles) into *total
// saturating a clip (wbx_saturate.hip): oversample, shape through a table, band-limit back — one launch over tiles of output
// frames, the tiles' statistics folded by a second, one-workgroup launch
struct SatPartial {            // what one tile (or the whole call) knows of wbx_saturate_stats; every field merges in any order
  double peak_drive;           // the greatest |d|; -1.0: no mid sample yet
  unsigned long long peak_index, beyond;
};
struct SatArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const double* tab;           // device: [kSatTable] — the shape table
  const double* up;            // device: [2 Z][os] — the up filter, tap-major, as doubles (os > 1)
  const double* down;          // device: [2 Z + 1][os] — the down filter behind one 0.0, padded with 0.0 (os > 1)
  SatPartial* part;            // device: [n_tiles], and behind them the call's record
  double drive, makeup;
  uint32_t n;                  // frames of the range and of the result; n * os < 2^31 - 16
  uint32_t os, channels;
  uint32_t tile, Z, plane, row, n_tiles;   // wbx_saturate.h's SatShape
};
void launch_saturate(const SatArgs& a, uint32_t lds_bytes, hipStream_t s);
void launch_saturate_reduce(const SatArgs& a, hipStream_t s);      // part[0 .. n_tiles) into part[n_tiles]
// stretching a clip (wbx_stretch.hip): per band of steps the positions — stretch_search_kernel, ONE workgroup walking the
// steps of a launch in order — then the overlap-add over the band's frames
struct StretchCarry {          // what one search launch hands the next, and the call's record so far (a device word block)
  int32_t p;                   // the last position found: p_{k0 - 1} of the next launch
  uint32_t max_shift;          // the largest |p_k - a_k|
  uint64_t searched;           // steps that searched
  uint64_t candidates;         // candidates scored
};
struct StretchArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  int32_t* pos;                // device: the stage — pos[0] = p_{band0 - 1}, pos[1 + k - band0] = p_k
  StretchCarry* carry;         // device
  const double* win;           // device: [N] — w_up[Hs], then w_dn[Hs]
  uint64_t a0, r0;             // anchor and remainder of step k0: k0 Hs n = a0 m + r0
  uint32_t qn, rn;             // an anchor's advance per step: Hs n = qn m + rn
  uint32_t n, m;               // frames of the range and of the result (< 2^31 - 16)
  uint32_t Hs, D;              // N / 2, the tolerance
  uint32_t band0, band_steps;  // the band's first step and its steps
  uint32_t k0, k1;             // the steps of this search launch: [k0, k1)
  uint32_t channels;           // 1 or 2
};
void launch_stretch_search(const StretchArgs& a, hipStream_t s);
void launch_stretch_ola(const StretchArgs& a, hipStream_t s);
// warping a clip (wbx_warp.hip): the segments between markers are independent chains — warp_search_kernel, one workgroup
// per live segment of a launch walking its steps of the round in order — then one overlap-add over the whole result
struct WarpRecord {            // the call's record, added to by every search workgroup (integer atomics: free of order)
  unsigned long long searched;    // steps that searched
  unsigned long long candidates;  // candidates scored
  uint32_t max_shift;          // the largest |p_k - a_k|
  uint32_t pad;
};
struct WarpArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  int32_t* pos;                // device: [K] — all positions of the call
  const wbx_warp_segment* seg; // device: [S + 1] — the segments, then (n, m, K, 0)
  const uint32_t* ids;         // device: the segment ids of this search launch, one per workgroup
  WarpRecord* rec;             // device
  const double* win;           // device: [N] — w_up[Hs], then w_dn[Hs]
  uint32_t n, m;               // frames of the range and of the result (< 2^31 - 16)
  uint32_t Hs, D;              // N / 2, the tolerance
  uint32_t S;                  // segments
  uint32_t round, round_steps; // this search launch walks steps [round * round_steps, (round + 1) * round_steps) of its segments
  uint32_t count;              // workgroups of this search launch
  uint32_t channels;           // 1 or 2
};
void launch_warp_search(const WarpArgs& a, hipStream_t s);
void launch_warp_ola(const WarpArgs& a, hipStream_t s);
// pitch-shifting a clip (wbx_pitch.hip): the stretch's searches fill ALL positions of the call, then one pitch_kernel launch —
// resample_kernel's tile, staged from the overlap-add of the range instead of from a clip
struct PitchArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const float* table;          // device: the conversion's coefficients in phase-visit order, [T][L] (resample_table_device)
  const int32_t* pos;          // device: [K' + 1] — pos[0] = p_{-1} = -Hs, pos[1 + k] = p_k
  const double* win;           // device: [N] — w_up[Hs], then w_dn[Hs]
  uint32_t n, mid, n_out;      // frames of the range, of the intermediate (m') and of the result (m), all < 2^31 - 16
  uint32_t Hs;                 // N / 2
  uint32_t L, M, H, T;         // the plan (wbx_resample.h)
  uint32_t channels;           // 1 or 2
  uint32_t tile, span, n_tiles;   // filled by launch_pitch: outputs per tile, floats staged per channel and tile, tiles
};
void launch_pitch(PitchArgs a, hipStream_t s);
// tracking a clip's pitch (wbx_f0.hip): one launch scores hops [hop0, hop1) of the call, F consecutive hops per workgroup
struct F0Args {
  const float* src[2];         // the clip's channel rows at the RANGE's first frame (mono: src[1] unused)
  wbx_f0_frame* out;           // device: the call's records, [hops]
  double threshold;
  uint32_t n;                  // frames of the range (< 2^31 - 16)
  uint32_t W, H;               // window and hop
  uint32_t tau_min, tau_max;
  uint32_t hop0, hop1;         // the hops of this launch
  uint32_t G, F;               // waves per hop (1, 2, 4 or 8), hops per workgroup (wbx_f0.h f0_shape)
  uint32_t channels;           // 1 or 2
};
void launch_f0(const F0Args& a, hipStream_t s);
// seeing a clip's spectrum (wbx_spectrum.hip): one launch computes the cells of hops [hop0, hop1) of the call, F consecutive
// hops x 64 K G bins per workgroup
struct SpecArgs {
  const float* src[2];         // the row(s) the detector reads, at the RANGE's first frame (src[1] only where mid is set)
  const float* basis;          // the basis clip's row: [W][B][2]
  float* out;                  // device: the cells of THIS launch, [hop1 - hop0][B]
  uint32_t n;                  // frames of the range (< 2^31 - 16)
  uint32_t W, B, H;            // window, bins, hop
  uint32_t hop0, hop1;         // the hops of this launch
  uint32_t K, G, F;            // bins per lane (1 or 2), waves over the bins (1, 2 or 4), hops per workgroup (wbx_spectrum.h spectrum_shape)
  uint32_t chunk, stride;      // terms staged at a time, words between the workgroup's hops in LDS
  uint32_t mid;                // 1: d = (float)(0.5 * (src[0] + src[1])); 0: d = src[0]
};
void launch_spectrum(const SpecArgs& a, hipStream_t s);
// reducing a clip's noise (wbx_denoise.hip): per band of hops the analysis (the transform launch, cells out), the gate (masked
// cells out, the open cells counted per workgroup and folded), the synthesis (the same launch turned round, chain values
// out as doubles) and the overlap-add into the new clip; the profile walks the analysis' cells.  Stage rows are
// [hop - row0][channel][W]
struct DenArgs {
  const float* src[2];         // the source's channel rows at the RANGE's first frame (mono: src[1] unused)
  float* dst[2];               // the new clip's rows (256-B aligned)
  const float* tab;            // device: [W][W] — the transform launch's table (wbx_denoise.h's A or Y)
  float* cells;                // device: the band's cell rows
  float* masked;               // device: the band's masked rows
  double* chain;               // device: the band's chain values
  const double* thr;           // device: [channels][B]
  double* sums;                // device: [channels][B] — the profile's running sums
  unsigned long long* part;    // device: the gate workgroups' open cells, [n_part]
  unsigned long long* total;   // device: the call's open cells so far
  double floor;
  uint32_t n;                  // frames of the range
  uint32_t W, H, B, channels;
  uint32_t S, F;               // the box
  uint32_t T;                  // hops of the call
  uint32_t lead;               // hop t starts at range frame (t - lead) H: 3, the profile 0
  uint32_t row0;               // the hop of the stage's first row
  uint32_t hop0, hop1;         // the hops of THIS launch (transform, gate, profile)
  uint32_t own0, own1;         // the hops whose open cells this band counts
  uint32_t blk0, blk1;         // the blocks of H frames the overlap-add writes
  uint32_t n_part;
  uint32_t K, G, hops_wg, chunk, stride;   // wbx_denoise.h's DenShape; stride: words between two hops' staged rows
};
void launch_denoise_transform(const DenArgs& a, bool synthesis, hipStream_t s);
void launch_denoise_gate(const DenArgs& a, hipStream_t s);           // part[0 .. n_part) written
void launch_denoise_fold(const DenArgs& a, hipStream_t s);           // *total += part[0 .. n_part)
void launch_denoise_ola(const DenArgs& a, hipStream_t s);
void launch_denoise_profile(const DenArgs& a, hipStream_t s);        // sums += the power of rows [hop0, hop1), ascending
// aligning two clips (wbx_align.hip): the partials of one band — a workgroup per (block of 4096 lags, chunk) —, the fold of a
// band onto the running curve with the scores and the workgroups' best after the last, Ea's partials, and the pick
struct alignas(16) AlignPartial {  // what a chunk leaves per lag: one 16-byte store
  double pr, pE;
};
struct alignas(8) AlignBest {      // a fold workgroup's greatest score and the lowest lag index that has it
  double score;
  uint32_t q, _pad;
};
struct AlignPick {                 // what the pick leaves for the host
  double offset, score, r, energy, ref_energy, confidence;
  uint32_t q, inverted;            // the lag's index from lag_min
};
struct AlignArgs {
  const float* a[2];           // the reference's channel rows at a_first (mono: a[1] unused)
  const float* b[2];           // the clip's channel rows at b_first (mono: b[1] unused)
  AlignPartial* stage;         // device: [chunks of the band][lags]
  wbx_align_point* curve;      // device: [lags], the running r and E
  AlignBest* best;             // device: [ceil(lags / 256)]
  double* ea_part;             // device: [chunks]
  AlignPick* pick;             // device: the record
  uint32_t n, m;               // frames of the template (<= 2^24) and of B's range (< 2^31 - 16)
  int32_t lag_min;
  uint32_t lags;
  uint32_t chunks;             // of the call
  uint32_t chunk0, chunk1;     // the chunks of this band
  uint32_t waves;              // of a partial workgroup (wbx_align.h align_shape)
  uint32_t cha, chb;           // channels, 1 or 2
  uint32_t either;             // WBX_ALIGN_EITHER_POLARITY
};
void launch_align_ref(const AlignArgs& a, hipStream_t s);
void launch_align_partial(const AlignArgs& a, hipStream_t s);
void launch_align_fold(const AlignArgs& a, hipStream_t s);
void launch_align_pick(const AlignArgs& a, hipStream_t s);
// finding a clip's onsets (wbx_onset.hip): the energy pass — a wave per hop, striding over the hops by the grid — and the
// novelty pass, a lane per hop
struct alignas(16) OnsetEnergy {   // what the energy pass leaves per hop: one 16-byte store
  double a, b;                 // A(h), B(h)
};
struct OnsetArgs {
  const float* src[2];         // the clip's channel rows at the RANGE's first frame (mono: src[1] unused)
  OnsetEnergy* energy;         // device: [hops]
  float* novelty;              // device: o(h) as floats, [hops] — the "clip" a tempo call tracks
  wbx_onset_frame* rec;        // device: the call's records, [hops] (onset = 0: the pick runs on the host)
  double floor;                // (double)H * floor_power
  uint32_t hops;               // complete hops of the range (<= 2^20)
  uint32_t H, q;               // hop length, a lane's run H / 64
  uint32_t row;                // words between the lanes' rows of a wave's staged chunk (wbx_onset.h; 0: no LDS)
  uint32_t channels;           // 1 or 2
  uint32_t aligned;            // both rows lie on 4 q bytes: a lane's run is one load (q = 1, 2 or 4)
};
void launch_onset_energy(const OnsetArgs& a, hipStream_t s);
void launch_onset_novelty(const OnsetArgs& a, hipStream_t s);
// splicing clips (wbx_splice.hip): parts of planar F32 clips placed, faded and added into a new planar F32 clip
struct SplicePartDev {         // 48 bytes, read with wave-uniform loads
  const float* src[2];         // the rows output channel 0 / 1 reads (MONO_MIX: L and R), at the PART's first source frame
  uint32_t n, at;              // frames of the part / output frame of its first one
  uint32_t fade_in, fade_out;  // frames (<= n)
  float gain;
  uint32_t bits;               // kSpliceShapeIn/Out: WBX_FADE_* in two bits each; kSpliceReversed; kSpliceMonoMix
  uint32_t _pad[2];
};
constexpr uint32_t kSpliceShapeOutShift = 2, kSpliceReversed = 1u << 4, kSpliceMonoMix = 1u << 5;
struct SpliceArgs {
  const SplicePartDev* parts;  // device
  const uint32_t* tile_off;    // device: [n_tiles + 1] (wbx_splice.h)
  const uint32_t* tile_parts;  // device: [tile_off[n_tiles]]
  float* dst[2];               // the new clip's rows (256-B aligned)
  uint32_t n_frames, n_tiles;  // n_frames < 2^31 - 16
  uint32_t channels;           // of the result: 1 or 2
};
void launch_splice(const SpliceArgs& a, hipStream_t s);
void launch_mip(const MipArgs& a, int format, int bits, hipStream_t s);
}  // namespace wbx

namespace wbx {

constexpr int kEventRing = 64;
// Plan buffers, partial-sum buffers and their events form a ring of three: the plan of render i may start as soon as
// the mix of render i-3 and the sum of render i-3 are over, i.e. a full render before its own mix — the one-wave-per-
// track plan kernel is starved for CU slots while a mix runs, so it needs that much slack to stay off the critical path.
constexpr int kRing = 3;
constexpr uint32_t kPaceRing = 64;
// Events whose only waiters are other streams of this device (or a host that waits for "done" and reads nothing the device
// wrote) are released to the DEVICE — a marker's default release is to the system.  (No measurable effect by itself; the A/Bs
// that seemed to show one were reading the copy engine's two speeds: EXPERIMENTS.md.)  Results leave through sum_done and the
// callback's own system-scope stores, which keep the system scope.
constexpr unsigned kDevEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;
constexpr uint32_t kCbDoneWords = 2 * 16 * 64;   // wbx_ctx::d_cb_done: two counters of kCbLanes words, kCbStride apart (wbx_callback.h)

// (ClipSlab, the clip pool's slabs and the policy that carves them up: wbx_pool.h)

struct ClipSlot {
  void* alloc = nullptr;    // an allocation of its own (hipFree), or
  ClipSlab* slab = nullptr; // the slab it lives in
  size_t slab_off = 0, slab_len = 0;   // ... and its extent there (the gap in front of the clip included)
  void* base = nullptr;     // first channel row; all channels in one piece
  size_t stride = 0;        // bytes between channel rows
  DSample d{};
  bool used = false;
  // waveform mip-maps (built on request): one allocation, level l at mip_off[l], [channels][mip_count[l]] elements
  void* mip = nullptr;
  int mip_bits = 0;
  std::vector<size_t> mip_off;
  std::vector<uint64_t> mip_count;
};

// (DevBuf, PinnedBuf, Event, Stream, PinnedSlot — the holders every resource below lives in: wbx_res.h)

struct DistState;   // wbx_dist.hip

// A side stream: what an editing-thread call that reads or creates pool clips beside the renders works on.  A stream of the
// call's own (no mix or sum stream) and the two events that order it behind what last wrote the pool: the main and the
// upload stream.  Export and the clip edits each own one; side_prepare / side_order / side_release (wbx_runtime.hip).
struct SideStream {
  Stream stream;
  Event after_main, after_upload;
};

// wbx_clip_export's staging: a side stream and kExportSlots chunks, each a device buffer the kernel writes, a pinned
// host buffer the copy engine moves it into and a block of statistics — made at first use, the same size for a clip of a
// thousand frames and one of 2^31 (a chunk is at most 8 bytes per frame: two channels of 32 bits), freed with the context.
constexpr int kExportSlots = 3;
constexpr uint32_t kExportChunkDefault = 1u << 20, kExportChunkMax = 1u << 24;
struct ExportStage {
  SideStream side;
  uint32_t chunk = 0;                     // frames the slots were made for
  DevBuf<uint8_t> d_slot[kExportSlots];
  PinnedSlot<uint8_t> h_slot[kExportSlots];   // pinned; done: the chunk's copies out of the slot are over
  DevBuf<uint32_t> d_stats[kExportSlots];     // 8 words each (6 used)
  PinnedBuf<uint32_t> h_stats;                // pinned: [kExportSlots][8]
};
// a clip's storage as a side call needs it (layer 2 copies it out of the pool under the editor lock)
struct ClipSrc {
  const void* base = nullptr;
  size_t stride = 0;
  uint32_t channels = 0, format = 0;
  uint64_t frames = 0;
};

// wbx_clip_measure / wbx_clip_derive: a side stream and the statistics block (device, and pinned: [0] the image a launch
// starts from, [1] what it left) — made at first use, freed with the context
struct ClipFxStage {
  SideStream side;
  DevBuf<ClipFxStats> d_stats;
  PinnedBuf<ClipFxStats> h_stats;
};

// wbx_clip_resample's coefficient tables on the device, one per (L, M, quality) a context has converted with — made at
// first use, freed with the context (192 B .. 2.6 MB each)
struct ResampleTable {
  uint32_t L = 0, M = 0;
  int quality = 0;
  DevBuf<float> d;
  std::vector<float> host;     // the upload's source, until the stream has been waited for
};

// wbx_clip_varispeed's interleaved tables on the device, one per (quality, reduced guard) a context has read with — made at
// first use, freed with the context (48 KB .. 8 MB each) —, the call's knots and tiles, and the timing events
struct VsTable {
  int quality = 0;
  uint32_t gn = 0, gd = 0;
  DevBuf<float> d;
  std::vector<float> host;     // the upload's source, until the stream has been waited for
};
struct VsStage {
  std::vector<VsTable> tables;
  PinnedBuf<long long> h_knots;
  DevBuf<long long> d_knots;
  PinnedBuf<wbx_varispeed_tile> h_tiles;
  DevBuf<wbx_varispeed_tile> d_tiles;
  Event mark[2];               // (timing events) around the uploads and the launch of the last run: wbx_varispeed_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_loudness's results on the device and in pinned memory — grown on demand, freed with the context
struct LoudnessStage {
  DevBuf<double> d_energy;
  PinnedBuf<double> h_energy;
  DevBuf<uint32_t> d_peak;     // 2 words
  PinnedBuf<uint32_t> h_peak;
};

// wbx_clip_filter's chunk states and carry matrix on the device, the matrix's upload source in pinned memory — grown on
// demand, freed with the context
struct FilterStage {
  DevBuf<double> d_state, d_M;
  PinnedBuf<double> h_M;
  Event mark[4];               // (timing events) around the three launches of the last run: wbx_filter_phase_ms
  bool timed = false, carried = false;   // the last run completed / had more than one chunk
};

// wbx_clip_convolve's response as doubles on the device (at most 2 x 2^20 x 8 bytes) — grown on demand, freed with the context
struct ConvolveStage {
  DevBuf<double> d_taps;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_convolve_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_dynamics' own buffers: the transfer table (3073 doubles, uploaded per call), the statistics and the timing
// events.  The curve's stage and the cached ramp are LimitStage's — one edit runs at a time
struct DynStage {
  PinnedBuf<double> h_tab;
  DevBuf<double> d_tab;
  DevBuf<DynPartial> d_part;     // a band's tiles, and behind them the call's record
  PinnedBuf<DynPartial> h_total;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_dynamics_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_stretch's own buffers: the positions of one band (2^16 + 1 words, whatever the clip's length) with their pinned
// twin (filled only for a caller who asks for positions), the carry, the window table (kept while N stays the same) and
// the timing events
struct StretchStage {
  DevBuf<int32_t> d_pos;
  PinnedBuf<int32_t> h_pos;
  DevBuf<StretchCarry> d_carry;
  PinnedBuf<StretchCarry> h_carry;
  PinnedBuf<double> h_win;
  DevBuf<double> d_win;
  uint32_t win_of = 0;         // the N the device table was built for (0: none)
  Event mark[2];               // (timing events) around the launches of the last run: wbx_stretch_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_warp's own buffers: ALL positions of a call (K <= 2^22: at most 16 MB) with their pinned twin (filled only for a
// caller who asks for positions), the segment table (S + 1 records), the segment ids of all search launches, the record and
// the timing events.  The window table is StretchStage's — one edit runs at a time
struct WarpStage {
  DevBuf<int32_t> d_pos;
  PinnedBuf<int32_t> h_pos;
  DevBuf<wbx_warp_segment> d_seg;
  PinnedBuf<wbx_warp_segment> h_seg;
  DevBuf<uint32_t> d_ids;
  PinnedBuf<uint32_t> h_ids;
  DevBuf<WarpRecord> d_rec;
  PinnedBuf<WarpRecord> h_rec;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_warp_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_pitch's own buffers: ALL positions of a call behind p_{-1} (K' + 1 words, K' <= 2^22: at most 16 MB + 4 B) with
// their pinned twin (filled only for a caller who asks for positions) and the timing events.  The window table and the
// carry are StretchStage's — one edit runs at a time
struct PitchStage {
  DevBuf<int32_t> d_pos;
  PinnedBuf<int32_t> h_pos;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_pitch_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_f0's records on the device and in pinned memory (at most 2^20 x 32 bytes) — grown on demand, freed with the
// context — and the timing events
struct F0Stage {
  DevBuf<wbx_f0_frame> d_rec;
  PinnedBuf<wbx_f0_frame> h_rec;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_f0_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_align's buffers: the stage of one band's partials (at most 2^22 x 16 bytes = 64 MB, made at first use), the
// running curve (at most 2^17 x 16 bytes) with its pinned twin (filled only for a caller who asks for the curve), the fold
// workgroups' best, Ea's partials (at most 8192), the record with its pinned twin — grown on demand, freed with the context
// — and the timing events
struct AlignStage {
  DevBuf<AlignPartial> d_part;
  DevBuf<wbx_align_point> d_curve;
  PinnedBuf<wbx_align_point> h_curve;
  DevBuf<AlignBest> d_best;
  DevBuf<double> d_ea;
  DevBuf<AlignPick> d_pick;
  PinnedBuf<AlignPick> h_pick;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_align_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_spectrum's cells of one launch on the device and in pinned memory (at most 2^22 x 4 bytes each) — grown on
// demand, freed with the context — and the timing events of a launch, whose times are summed
struct SpecStage {
  DevBuf<float> d_cells;
  PinnedBuf<float> h_cells;
  Event mark[2];               // (timing events) around each launch of the last run: wbx_spectrum_ms adds them up
  double ms = 0.0;
  bool timed = false;          // the last run completed
};

// wbx_clip_onsets' and wbx_clip_tempo's energies (16 bytes per hop), novelty (4) and records (32) on the device, the records'
// pinned twin (at most 2^20 hops each) — grown on demand, freed with the context — and the timing events
struct OnsetStage {
  DevBuf<OnsetEnergy> d_energy;
  DevBuf<float> d_nov;
  DevBuf<wbx_onset_frame> d_rec;
  PinnedBuf<wbx_onset_frame> h_rec;
  Event mark[2];               // (timing events) around the energy pass of the last run: wbx_onset_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_limit's ramp table (at most (4096 + 65536 + 2^20 + 40) x 8 bytes, kept while A, H and R stay the same), the fp64
// curve of one band ((2^20 + 4096) x 8 bytes = 8.4 MB, whatever the clip's length) and the statistics — grown on demand,
// freed with the context
struct LimitStage {
  PinnedBuf<double> h_ramp;
  DevBuf<double> d_ramp, d_y;
  DevBuf<LimitPartial> d_part;   // a band's tiles, and behind them the call's record
  PinnedBuf<LimitPartial> h_total;
  uint32_t ramp_of[3] = {0, 0, 0};   // A, H, R of the table d_ramp holds (R == 0: none)
  Event mark[2];               // (timing events) around the launches of the last run: wbx_limit_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_saturate's own buffers: the shape table (16385 doubles, uploaded per call), the two filters as doubles (kept
// while os and the quality stay the same), the tiles' statistics with the call's record behind them — grown on demand, freed
// with the context — and the timing events
struct SatStage {
  PinnedBuf<double> h_tab, h_coef;
  DevBuf<double> d_tab, d_coef;
  uint32_t coef_of[2] = {0, 0};  // os and quality + 1 of the filters d_coef holds (os == 0: none)
  DevBuf<SatPartial> d_part;
  PinnedBuf<SatPartial> h_total;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_saturate_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_denoise's and wbx_clip_denoise_profile's own buffers: the two tables as the device reads them (W x W floats
// each, kept while W stays the same; not in the pool), a band's cells, masked cells and chain values, the threshold, the
// profile's sums, the gate's partial counts with the call's total behind them — grown on demand, freed with the context —
// and the timing events
struct DenStage {
  DevBuf<float> d_tab;         // A, then Y
  uint32_t tab_w = 0;          // the W of the tables d_tab holds (0: none)
  DevBuf<float> d_cells, d_masked;
  DevBuf<double> d_chain, d_thr, d_sums;
  DevBuf<unsigned long long> d_part;
  PinnedBuf<double> h_thr, h_sums;
  PinnedBuf<unsigned long long> h_total;
  Event mark[2];               // (timing events) around the launches of the last run: wbx_denoise_ms
  bool timed = false;          // the last run completed
};

// wbx_clip_splice's part descriptors and tile table on the device — grown on demand, freed with the context
struct SpliceStage {
  DevBuf<SplicePartDev> parts;
  DevBuf<uint32_t> tile_off, tile_parts;
};

}  // namespace wbx

using namespace wbx;   // (internal header: only the host-side translation units of the library include it)

struct wbx_ctx {
  wbx_config cfg{};
  Stream stream;                      // the main stream: made here, or wbx_config.stream adopted (never destroyed)
  std::string err;

  std::vector<ClipSlot> clips;
  ClipSlabs slabs;   // clip storage (slab_mu: clips are built outside the editor lock)
  std::mutex slab_mu;
  std::atomic<uint32_t> slab_seq{0};  // clips placed so far (seeds the gap in front of the next one)
  std::atomic<uint64_t> pool_limit{0};   // wbx_clip_pool_limit: bytes the pool may reserve from the driver, 0 = no bound
  std::atomic<uint64_t> own_alloc_bytes{0};   // ... of which: clips with an allocation of their own
  DevBuf<DSample> d_samples;
  bool samples_dirty = true;

  // routing
  uint32_t routing_tracks = 0, n_buses = 0;
  std::vector<int32_t> track_bus;
  std::vector<uint32_t> order;
  std::vector<DGroup> groups;         // member lists cut into pieces of group_size tracks (one workgroup per piece and block)
  std::vector<DGroup> groups_exact;   // the member lists whole: the reference's summation order (build_routing)
  bool buses_alias_exact = false;     // buses_alias_partials of groups_exact
  uint32_t longest_list = 0;          // tracks in the longest member list
  mutable bool chain_broken = false;  // a chained render reported a failed hand-over (plan_status_to_error)
  uint32_t chain_epoch = 0;
  DevBuf<uint32_t> d_chain;           // chained renders: the "running sum is out" words
  DevBuf<uint32_t> d_sticky_status;      // failure bits (32 | 64) of every chained render since the last report (render_status)
  DevBuf<uint32_t> d_order;
  DevBuf<DGroup> d_groups;
  bool routing_dirty = true;

  // The plan of a render (track-block records, overflow pool, pre-render queue + rows) is double-buffered:
  // the sequencer of step i+1 runs on `plan_stream` while the mix of step i runs on `stream`.
  struct PlanBuf {
    DevBuf<DRow> prows;               // [K][N] 16-B plan rows
    DevBuf<DTrackBlock> tmpl;         // templates the rows point at (one per steady run / per block with events)
    uint32_t tmpl_cap = 0;
    bool static_tmpl = false;         // the last plan into this buffer gave track t the templates 2t, 2t + 1 (no allocation count)
    DevBuf<DSeg> pool;
    uint32_t pool_chunks = 0;
    DevBuf<DBlockTime> times;         // [K] per-block transport records of a batch render (PlanArgs::times)
    DevBuf<uint32_t> counters;        // [0] pool chunks allocated, [1] status bits, [2] generic records queued,
                                      // [3] templates allocated
    bool counters_zero = true;        // cleared already (at creation, or by the sum kernel of a callback block)
    DevBuf<uint32_t> gen_list;        // pre-render queue of KIND_GENERIC records
    DevBuf<float> rows;               // [gen_cap][C][F+8] pre-rendered mixing buffers
    DevBuf<DTrackBlock> saved;        // original records of the queue (plan read-back)
    uint32_t gen_cap = 0;
    Event planned;                    // recorded on plan_stream when plan + pre-render are done
    hipEvent_t consumed = nullptr;    // (not owned) ctx->mix_done[] of the render whose mix read this buffer
    bool consumed_valid = false;
  } pb[kRing];
  int cur = 0;
  Stream plan_stream;
  DevBuf<float> d_zero;               // zero page (F+8 floats)
  uint32_t* levels_target = nullptr;  // [N][C] running per-track maxima (VUMeter::level), or null
  DevBuf<float> d_partial2[kRing];    // group partials, one per render in flight (a sum may still read an older one)
  DevBuf<float> d_master, d_buses, d_gains;
  DevBuf<float> d_peaks[2];           // per-track-block peaks: one buffer per mix stream (two mixes may be in flight)
  float* last_peaks = nullptr;        // where the last render / submit put its peaks
  // WBX_MIX_ALT=1 (CtxKnobs::mix_alternate; experiment, off by default): consecutive batch renders of layer 2 alternate between the main stream
  // and `alt_stream`, so that nothing orders mix i+1 after mix i and the head of one can fill the CUs the tail of the
  // other leaves idle.  Everything else stays on the main stream, which joins the alternate one (join_alt) wherever it
  // joins the sum stream.  Measured: no gain in step time, each kernel's own interval grows by ~45 %.
  Stream alt_stream;
  hipStream_t cur_mix_stream = nullptr;   // the stream of the last mix (launch_mix_sum): what wbx_pace marks and the alternation reads
  int alt_pending = -1;                   // partial-buffer index of a mix on alt_stream the main stream has not joined
  // The sum of render i runs on its own stream beside the mix of render i+1 (it is PCIe-bound when the master goes to
  // host memory and needs few CUs).  sum_pending: a sum has been issued that the main stream has not waited for yet.
  Stream sum_stream;
  Event mix_done[kRing], sum_done[kRing];
  // recorded right behind the sum KERNEL, in front of the copy that takes a staged master to host memory: from here on the
  // partial buffer may be written again.  What the next user of the buffer waits for (round 6) — sum_done lies behind the
  // copy, 8 MB over PCIe per 2048-block render: a 256-track session's plans waited 0.3 ms for it and its mixes 0.07 ms for them
  Event partial_free[kRing];
  bool sum_valid[kRing] = {};
  int sum_pending = -1;
  uint32_t render_seq = 0;
  DevBuf<uint8_t> d_conv;
  DevBuf<unsigned long long> d_dbg;   // diagnostic (WBX_DBG_CLOCK=1): per-workgroup start / end times of the last mix
  size_t dbg_wgs = 0;
  std::vector<DTrackBlock> h_tb;      // layer-1 staging
  std::vector<DRow> h_rows;
  std::vector<DSeg> h_pool;

  uint32_t last_K = 0, last_N = 0;
  // the one-launch callback (wbx_callback.h; what one launch needs from its caller: RenderCall)
  DevBuf<uint32_t> d_cb_done;         // device: "workgroups done" ticket counter, never reset: launches count from cb_base
  uint32_t cb_base = 0;               // ... the first counter (every multi-group launch arrives there)
  uint32_t cb_base2 = 0;              // ... the second one (only launches whose workgroups each add a share of the master)
  uint64_t cb_launches = 0, cb_spread_launches = 0;   // one-launch callbacks issued / ... with the spread sum
  bool seg_broken = false;            // plan_seg_kernel found its XCD layout broken (status bit 7): one lane per track from then on
  // Which mix instance a render takes and what follows from it (wbx_shape.h).  `shape` is assigned ONCE per render — by
  // render_locked / wbx_submit, from the knobs, the session's facts and the context's state (render_shape) — and read by
  // everything that launches for that render, the repeats of a callback block included.
  ShapeKnobs knobs;                   // the switches, read once at wbx_create (wbx_knobs.h): those that enter the shape ...
  CtxKnobs ck;                        // ... and the others the context consults
  SessionFacts session;               // of the last render (a bare context: layer 1's "unknown, assume so")
  RenderShape shape;
  uint32_t n_xcds = 0;                // the XCD layout probe of wbx_create: 8 / 4 / 2 / 1, or 0 — not round-robin: no chained pieces
                                      // (chain_broken), no segmented sequencer (seg_broken) from the start
  uint32_t n_cus = 0;                 // the device's CU count (wbx_create), what callback_spread_limit (wbx_shape.h) starts from
  bool cb_no_spread = false;          // a spread launch gave up waiting for the whole grid (not resident at once: a CU mask, a
                                      // device shared with another process): the context keeps to "the last workgroup adds"
  bool buses_alias_partials = false;  // see build_routing
  const float* last_buses = nullptr;  // where the last render's bus sums are: d_buses or the partial buffer
  bool buses_clean = false;           // d_buses zeroed since the last routing change / reallocation
  float* last_master = nullptr;       // where the last render / submit put its master (d_master, the caller's target, or
  bool last_master_on_host = false;   // the engine's pinned staging block, which is host memory)
  bool clamp = true;
  float* master_target = nullptr;     // caller-owned device buffer, or null: d_master
  bool master_target_on_host = false; // ... it is pinned host memory: batch renders stage the master in d_stage and copy it out
  DevBuf<float> d_stage[kRing];       // (see choose_issue, wbx_shape.h: a sum that stores 8 MB over PCIe itself holds up the next mix)
  int master_format = 0;              // wbx_set_master_format: 0 planar fp32, else WBX_OUT_* interleaved (sum kernel epilogue)
  int last_master_format = 0;         // ... of the last render
  const float* master_init = nullptr; // wbx_set_master_init: the running sum the first group starts from, or null: zero

  // kernel timing (mix kernel)
  Event ev[kEventRing][3];              // before the mix, after the mix, after the sum
  int ev_pending = 0;
  double mix_ms_total = 0.0;
  double gap_ms_total = 0.0;           // end of one mix -> start of the next, consecutive launches of one drain (wbx_gap_time)
  uint64_t gap_count = 0;
  double tail_ms_total = 0.0;          // mix end -> sum end (launch gap + sum kernel incl. its PCIe stores)
  uint64_t mix_launches = 0;
  const char* mix_kernel_name = "";   // the instance launch_mix chose last (wbx_kernel_name)
  double last_uniform_speed = 0.0;    // MixArgs::uniform_speed of the last launch (wbx_render_uniform_speed)
  bool has_integer_clips = false;
  bool has_non16_clips = false;       // a clip asset that is not 16-bit PCM
  bool auto_group = false;            // wbx_config.group_size was 0: the library picks the track-group size

  // wbx_clip_export / wbx_engine_export_sample: one export at a time (export_mu), on a stream that is no mix or sum stream
  ExportStage exp;
  std::mutex export_mu;
  std::atomic<uint32_t> export_chunk{0};   // wbx_set_export_chunk: frames per staging chunk, 0 = kExportChunkDefault

  // wbx_clip_measure / wbx_clip_derive and layer 2's forms: one at a time (fx_mu), on a stream that is no mix or sum stream
  ClipFxStage fx;
  std::mutex fx_mu;
  std::vector<ResampleTable> rs_tables;   // wbx_clip_resample (under fx_mu, on fx.side.stream)
  SpliceStage splice;                     // wbx_clip_splice (under fx_mu, on fx.side.stream)
  LoudnessStage loud;                     // wbx_clip_loudness (under fx_mu, on fx.side.stream)
  FilterStage filt;                       // wbx_clip_filter (under fx_mu, on fx.side.stream)
  ConvolveStage conv;                     // wbx_clip_convolve (under fx_mu, on fx.side.stream)
  LimitStage lim;                         // wbx_clip_limit (under fx_mu, on fx.side.stream)
  DynStage dyn;                           // wbx_clip_dynamics (under fx_mu, on fx.side.stream; shares lim's stage and ramp)
  StretchStage str;                       // wbx_clip_stretch (under fx_mu, on fx.side.stream)
  WarpStage wrp;                          // wbx_clip_warp (under fx_mu, on fx.side.stream)
  F0Stage f0;                             // wbx_clip_f0 and wbx_clip_tempo's track (under fx_mu, on fx.side.stream)
  OnsetStage ons;                         // wbx_clip_onsets, wbx_clip_tempo (under fx_mu, on fx.side.stream)
  SpecStage spec;                         // wbx_clip_spectrum (under fx_mu, on fx.side.stream)
  AlignStage aln;                         // wbx_clip_align (under fx_mu, on fx.side.stream)
  SatStage sat;                           // wbx_clip_saturate (under fx_mu, on fx.side.stream)
  VsStage vs;                             // wbx_clip_varispeed (under fx_mu, on fx.side.stream)
  DenStage den;                           // wbx_clip_denoise, wbx_clip_denoise_profile (under fx_mu, on fx.side.stream)
  PitchStage pit;                         // wbx_clip_pitch (under fx_mu, on fx.side.stream; shares str's window table and carry)

  Stream upload_stream;                // clip uploads of layer 2 run here, outside the engine's editor lock
  Event ready_ev;                      // wbx_master_ready: results of an in-stream sum, for a foreign stream
  Event pace_ev[kPaceRing];            // wbx_pace
  uint64_t pace_seq = 0;
  // layer 2 back pointer: asks whether a clip list still names a sample (wbx_clip_free), null for a bare ctx
  bool (*sample_in_use)(void* owner, uint32_t sample) = nullptr;
  void* owner = nullptr;
  wbx::DistState* dist = nullptr;      // multi-GPU exchange (wbx_dist.hip), null on a single GPU
};

namespace wbx {

inline wbx_ctx::PlanBuf& PB(wbx_ctx* c) { return c->pb[c->cur]; }

// What ONE call of launch_mix_sum needs from its caller.  wbx_ctx holds state — what outlives a render —; the inputs of a
// single render are arguments: built by value where the call is made (wbx_submit, render_locked, each repeat path of
// wbx_engine_process), read only by the callee, gone when it returns.
struct RenderCall {
  hipStream_t mix_stream = nullptr;   // where the mix runs: the main stream or the alternate one (pick_mix_stream)
  bool plan_waits_partial = false;    // the plan stream — which the mix follows — already waits for partial_free[] of this
                                      // render's partial buffer: no second wait on the mix stream
  uint32_t* status = nullptr;         // pinned: where the sum (or the one launch) drops the plan's four counters, or null
  bool clear_counters = false;        // ... and the kernel then clears the device's copy for the buffer's next plan
  // the one-launch callback (wbx_callback.h): the sequencer's arguments — the block may then run plan + mix + sum as one
  // kernel —, the pinned word that kernel writes `seq` into when master and status are out, and the pinned word it writes
  // `seq` into when one of its workgroups gave up at the spread barrier
  const PlanArgs* plan = nullptr;
  uint32_t* done_word = nullptr;
  uint32_t* gave_up_word = nullptr;
  uint32_t seq = 0;
  // wbx_engine_process: the block's master goes here (pinned host memory) in this format, whatever the setters say;
  // null: the context's own master_target / master_format
  float* master = nullptr;
  int format = 0;
};

// a failure's text, `what[: the HIP error]`, into *why (the side calls' messages) ...
inline wbx_status stage_fail(std::string* why, wbx_status st, const char* what, hipError_t e = hipSuccess) {
  if (why) {
    *why = what;
    if (e != hipSuccess) {
      *why += ": ";
      *why += hipGetErrorString(e);
    }
  }
  return st;
}
// ... or into the context's error string
inline wbx_status fail(wbx_ctx* c, wbx_status s, const char* what, hipError_t e = hipSuccess) {
  return stage_fail(c ? &c->err : nullptr, s, what, e);
}

#define WBX_HIP(ctx, call)                                                       \
  do {                                                                           \
    hipError_t _e = (call);                                                      \
    if (_e != hipSuccess) return ::wbx::fail((ctx), WBX_ERR_DEVICE, #call, _e);  \
  } while (0)

inline size_t fmt_bytes(int fmt) {
  switch (fmt) {
    case WBX_FMT_I16: return 2;
    case WBX_FMT_I24:
    case WBX_FMT_I32:
    case WBX_FMT_F32: return 4;
    default: return 0;
  }
}

size_t out_format_bytes(int fmt);   // bytes of a sample in a WBX_OUT_* device format, 0: no such format (wbx_runtime.hip)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

enum : int { CLIP_SRC_PLANAR = 0, CLIP_SRC_INTERLEAVED_HOST = 1, CLIP_SRC_INTERLEAVED_DEVICE = 2, CLIP_SRC_SYNTH = 3,
             CLIP_SRC_ZERO = 4 /* every frame zero, asynchronous on `on` (take chunks, recorded clips before their gather) */,
             CLIP_SRC_NONE = 5 /* only the padding is zeroed, asynchronous on `on`: a kernel writes every frame (bounced clips) */ };
struct ClipFill {           // where a new clip's audio comes from
  int kind;
  const void* const* planar;   // CLIP_SRC_PLANAR: host channel arrays
  const void* interleaved;     // CLIP_SRC_INTERLEAVED_*: [frames][channels]
  uint64_t seed;               // CLIP_SRC_SYNTH
  uint32_t key_track;
  float amp;
};

// wbx_runtime.hip
wbx_status clip_build(wbx_ctx* c, ClipSlot& s, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames,
                      const ClipFill& f, hipStream_t on);
wbx_status clip_publish(wbx_ctx* c, uint32_t clip, ClipSlot& s);
void clip_release(wbx_ctx* c, ClipSlot& s);
// side streams: side_prepare makes the stream and its events (at once if they exist; after a failure the struct is empty
// again), side_order puts the stream behind everything enqueued so far on the streams that write the pool's clips (enqueues
// only; layer 2 calls it under the editor lock), side_release waits for the stream and empties the struct
hipError_t side_prepare(wbx_ctx* c, SideStream& s);
hipError_t side_order(wbx_ctx* c, SideStream& s);
void side_release(SideStream& s);
// a pool clip as the side calls see it: the slot of a clip that exists (or null), its storage, a channel's row (ch % channels)
inline const ClipSlot* find_clip(const wbx_ctx* c, uint32_t id) {
  return id < c->clips.size() && c->clips[id].used && c->clips[id].base ? &c->clips[id] : nullptr;
}
inline ClipSrc clip_src(const ClipSlot& s) { return ClipSrc{s.base, s.stride, s.d.channels, s.d.format, s.d.count}; }
inline const float* clip_row(const ClipSrc& src, uint32_t ch) {
  return reinterpret_cast<const float*>((const char*)src.base + src.stride * (ch % src.channels));
}
// exporting: argument checks (no device call), the side stream with its slots, its ordering and the chunk loop (no lock
// held; `why` gets the message of a failure)
wbx_status export_check(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, int out_format, uint32_t flags,
                        const void* dst, const char** why);
wbx_status export_prepare(wbx_ctx* c, std::string* why);   // side stream, events and slots for the chunk size in force
wbx_status export_order(wbx_ctx* c, std::string* why);     // side_order of exp.side
wbx_status export_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, int out_format, uint32_t flags,
                      void* dst, wbx_export_stats* stats, std::string* why);
void export_release(wbx_ctx* c);
// editing clips (wbx_clipfx.hip), cut like the export: argument checks (no device call), the side stream with its statistics
// block, its ordering and the runs (no lock held; they wait for the device)
wbx_status clipfx_check_range(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, const char** why);
wbx_status clipfx_check_derive(const ClipSrc& src, const wbx_clip_edit_desc* d, uint32_t* out_channels, const char** why);
wbx_status clipfx_prepare(wbx_ctx* c, std::string* why);
wbx_status clipfx_order(wbx_ctx* c, std::string* why);     // side_order of fx.side
wbx_status clipfx_measure_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, wbx_clip_stats* out,
                              std::string* why);
wbx_status clipfx_derive_run(wbx_ctx* c, const ClipSrc& src, uint32_t sample_rate, const wbx_clip_edit_desc& d,
                             uint32_t out_channels, ClipSlot& slot, wbx_clip_stats* stats, std::string* why);
void clipfx_release(wbx_ctx* c);
// layer 1's calls that make clip dst_clip out of clip src_clip on the edit stream (wbx_clip_derive, wbx_clip_resample): the
// test of the two ids with the caller's messages, and "prepare, order, run(slot, why), publish" under fx_mu
wbx_status clipfx_check_ids(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, const char* unknown_src, const char* same);
// ... out of TWO clips (wbx_clip_convolve: the second may be the first, the result may be neither)
wbx_status clipfx_check_ids(wbx_ctx* c, uint32_t src_clip, uint32_t src2_clip, uint32_t dst_clip, const char* unknown_src,
                            const char* unknown_src2, const char* same);
template <class Run>
wbx_status clipfx_into_clip(wbx_ctx* c, uint32_t dst_clip, Run run) {
  std::lock_guard<std::mutex> g(c->fx_mu);
  std::string why;
  ClipSlot slot;
  wbx_status st = clipfx_prepare(c, &why);
  if (st == WBX_OK) st = clipfx_order(c, &why);
  if (st == WBX_OK) st = run(slot, &why);
  if (st != WBX_OK) return c->err = why, st;
  return clip_publish(c, dst_clip, slot);   // (may reallocate the pool's table: references into it are dead from here)
}
// ... and its twin for layer 1's calls that make no clip (wbx_clip_measure, _loudness, _f0, _onsets, _tempo, _spectrum,
// _align): "prepare, order, run(why)" under fx_mu
template <class Run>
wbx_status clipfx_reading(wbx_ctx* c, Run run) {
  std::lock_guard<std::mutex> g(c->fx_mu);
  std::string why;
  wbx_status st = clipfx_prepare(c, &why);
  if (st == WBX_OK) st = clipfx_order(c, &why);
  if (st == WBX_OK) st = run(&why);
  if (st != WBX_OK) c->err = why;
  return st;
}
// how the runs that make a clip open: `slot` becomes a blank planar F32 clip on the edit stream — the kernel writes every
// frame; clip_build clears the 16 padding frames (and the row's slack)
inline wbx_status clipfx_blank_clip(wbx_ctx* c, ClipSlot& slot, uint32_t channels, uint32_t sample_rate, uint64_t frames, std::string* why) {
  ClipFill fill{};
  fill.kind = CLIP_SRC_NONE;
  const wbx_status st = clip_build(c, slot, WBX_FMT_F32, channels, sample_rate, frames, fill, c->fx.side.stream);
  if (st != WBX_OK) *why = c->err;
  return st;
}
// ... and close: the measure pass over the finished result, on the same stream, where `stats` asks for it; a failure
// releases the slot
inline wbx_status clipfx_measure_result(wbx_ctx* c, ClipSlot& slot, uint64_t frames, wbx_clip_stats* stats, std::string* why) {
  if (!stats) return WBX_OK;
  const wbx_status st = clipfx_measure_run(c, clip_src(slot), 0, frames, stats, why);
  if (st != WBX_OK) clip_release(c, slot);
  return st;
}
// the device time of a stage's last run, between its two events (the wbx_*_ms accessors; Z has mark[2] and timed); `none`:
// what is said where no run has completed
template <class Z>
wbx_status stage_ms(wbx_ctx* c, Z wbx_ctx::*stage, const char* none, double* out) {
  if (!c || !out) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->fx_mu);
  Z& z = c->*stage;
  if (!z.timed) return fail(c, WBX_ERR_INVALID, none);
  float ms = 0.0f;
  WBX_HIP(c, hipEventElapsedTime(&ms, z.mark[0], z.mark[1]));
  *out = (double)ms;
  return WBX_OK;
}
// converting a clip's sample rate (wbx_resample.hip), cut the same way; it runs under fx_mu on the edit stream, behind
// clipfx_prepare / clipfx_order, and measures its result through clipfx_measure_run
wbx_status resample_check(const ClipSrc& src, uint32_t src_rate, uint64_t first_frame, uint64_t n_frames, uint32_t dst_rate,
                          int quality, ResamplePlan* plan, uint64_t* n_out, const char** why);
wbx_status resample_run(wbx_ctx* c, const ClipSrc& src, const ResamplePlan& p, int quality, uint64_t first_frame, uint64_t n_frames,
                        uint64_t n_out, uint32_t dst_rate, ClipSlot& slot, wbx_clip_stats* stats, std::string* why);
// the device copy of a plan's table in resample_kernel's order, made on the edit stream at first use and kept (*fresh: this
// call uploaded it, from rs_tables.back().host, which must outlive the stream's next wait)
hipError_t resample_table_device(wbx_ctx* c, const ResamplePlan& p, int quality, const float** out, bool* fresh);
// measuring a clip's loudness (wbx_loudness.hip), cut the same way: the checks make no device call; the run works under
// fx_mu on the edit stream behind clipfx_prepare / clipfx_order and waits for the device
struct LoudnessPlan {
  uint32_t rate = 0, hop = 0, factor = 0;   // factor: 0 without true peak
  uint64_t hops = 0;
};
wbx_status loudness_check(const ClipSrc& src, uint32_t rate, uint64_t first_frame, uint64_t n_frames, uint32_t flags,
                          const wbx_loudness* out, const double* hop_energy, size_t cap_doubles, LoudnessPlan* plan, const char** why);
wbx_status loudness_run(wbx_ctx* c, const ClipSrc& src, const LoudnessPlan& p, uint64_t first_frame, uint64_t n_frames,
                        wbx_loudness* out, double* hop_energy, std::string* why);
// filtering a clip (wbx_filter.hip), cut the same way: the checks make no device call; the run works under fx_mu on the edit
// stream behind clipfx_prepare / clipfx_order and measures its result through clipfx_measure_run
wbx_status filter_check_call(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, uint64_t tail_frames, const double* coef,
                             uint32_t n_stages, const char** why);
wbx_status filter_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, uint64_t first_frame, uint64_t n_frames, uint64_t tail_frames,
                      const double* coef, uint32_t n_stages, ClipSlot& slot, wbx_clip_stats* stats, std::string* why);
// convolving a clip (wbx_convolve.hip), cut the same way: the check makes no device call (and looks at the arithmetic of the
// call before it looks at the clips); the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order and
// measures its result through clipfx_measure_run
struct ConvolveCall {
  uint64_t first_frame, n_frames;   // range of the source
  uint64_t ir_first, ir_frames;     // range of the response
  uint64_t out_first, out_frames;   // window of the full result
  double gain;
};
wbx_status convolve_check(const ClipSrc& src, uint32_t src_rate, const ClipSrc& ir, uint32_t ir_rate, const ConvolveCall& k,
                          uint32_t* out_channels, const char** why);
wbx_status convolve_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc& ir, uint32_t rate, const ConvolveCall& k, ClipSlot& slot,
                        wbx_clip_stats* stats, std::string* why);
// limiting a clip (wbx_limit.hip), cut the same way: the check makes no device call (wbx_limit.h's limit_check_args first,
// then the clip); the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status limit_check(const ClipSrc& src, const LimitCall& k, const char** why);
wbx_status limit_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const LimitCall& k, ClipSlot& slot, wbx_limit_stats* out,
                     wbx_clip_stats* stats, std::string* why);
// dynamics of a clip (wbx_dynamics.hip), beside their limiter twins: the check makes no device call (wbx_dynamics.h's
// dynamics_check_args first, then the clips; `key` is NULL for a call that keys itself) and yields the table's smallest
// entry; the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status dynamics_check(const ClipSrc& src, uint32_t src_rate, const ClipSrc* key, uint32_t key_rate, const DynCall& k, double* lo,
                          const char** why);
wbx_status dynamics_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc* key, uint32_t rate, const DynCall& k, double lo, ClipSlot& slot,
                        wbx_dynamics_stats* out, wbx_clip_stats* stats, std::string* why);
// saturating a clip (wbx_saturate.hip), cut the same way: the check makes no device call (wbx_saturate.h's
// saturate_check_args first, then the clip: NULL for an unknown one, `replaces` where dst_clip is the source); the run works
// under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status saturate_check(const ClipSrc* src, bool replaces, const SatCall& k, const char** why);
wbx_status saturate_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const SatCall& k, ClipSlot& slot, wbx_saturate_stats* out,
                        wbx_clip_stats* stats, std::string* why);
// reading a clip along a position curve (wbx_varispeed.hip), cut the same way: the check makes no device call
// (wbx_varispeed.h's varispeed_check_args first — sizes and curve are judged before the clip —, then the clip: NULL for an
// unknown one, `replaces` where dst_clip is the source); the run works under fx_mu on the edit stream behind clipfx_prepare /
// clipfx_order
wbx_status varispeed_check(const ClipSrc* src, bool replaces, const VsCall& k, VsPlan* plan, const char** why);
wbx_status varispeed_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const VsCall& k, const VsPlan& plan, ClipSlot& slot,
                         wbx_clip_stats* stats, std::string* why);
// reducing a clip's noise (wbx_denoise.hip), cut the same way: the checks make no device call (wbx_denoise.h's argument
// checks first, then the clip: NULL for an unknown one, `replaces` where dst_clip is the source); the runs work under fx_mu
// on the edit stream behind clipfx_prepare / clipfx_order
wbx_status denoise_check(const ClipSrc* src, bool replaces, const DenCall& k, const char** why);
wbx_status denoise_profile_check(const ClipSrc* src, uint64_t first_frame, uint64_t n_frames, uint32_t window, bool has_sums, bool has_hops,
                                 const char** why);
wbx_status denoise_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const DenCall& k, ClipSlot& slot, wbx_denoise_stats* out,
                       std::string* why);
wbx_status denoise_profile_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, uint32_t window, double* sums_out,
                               uint64_t* hops_out, std::string* why);
// stretching a clip (wbx_stretch.hip), cut the same way: the check makes no device call (wbx_stretch.h's
// stretch_check_args first, then the clip); the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status stretch_check(const ClipSrc& src, const StretchCall& k, const char** why);
wbx_status stretch_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const StretchCall& k, ClipSlot& slot, int32_t* positions_out,
                       wbx_stretch_info* info, wbx_clip_stats* stats, std::string* why);
// warping a clip (wbx_warp.hip), beside its stretch twin: the check makes no device call (wbx_warp.h's warp_check_args
// first, then the clip); the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status warp_check(const ClipSrc& src, const WarpCall& k, const char** why);
wbx_status warp_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const WarpCall& k, ClipSlot& slot, int32_t* positions_out,
                    wbx_warp_info* info, wbx_clip_stats* stats, std::string* why);
// pitch-shifting a clip (wbx_pitch.hip), beside its stretch twin: the check makes no device call (wbx_pitch.h's
// pitch_check_args first, then the clip) and yields the conversion's plan and the stretch the call performs; the run works
// under fx_mu on the edit stream behind clipfx_prepare / clipfx_order
wbx_status pitch_check(const ClipSrc& src, const PitchCall& k, ResamplePlan* plan, StretchCall* stretch, const char** why);
wbx_status pitch_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const PitchCall& k, const ResamplePlan& plan, const StretchCall& stretch,
                     ClipSlot& slot, int32_t* positions_out, wbx_pitch_info* info, wbx_clip_stats* stats, std::string* why);
// tracking a clip's pitch (wbx_f0.hip), cut as the loudness measurement is: the check makes no device call (wbx_f0.h's
// f0_check first, then the clip); the run works under fx_mu on the edit stream behind clipfx_prepare / clipfx_order and
// waits for the device
wbx_status f0_check_call(const ClipSrc& src, const F0Call& k, const char** why);
wbx_status f0_run(wbx_ctx* c, const ClipSrc& src, const F0Call& k, wbx_f0_frame* frames_out, wbx_f0_info* info, std::string* why);
// finding a clip's onsets and tempo (wbx_onset.hip), cut the same way: the checks make no device call (wbx_onset.h's
// onset_check / tempo_check first, then the clip); the runs work under fx_mu on the edit stream behind clipfx_prepare /
// clipfx_order and wait for the device.  tempo_run leaves the novelty on the device and hands it to f0_run as a mono F32
// range of `hops` frames: the stream orders the two
wbx_status onset_check_call(const ClipSrc& src, const OnsetCall& k, const char** why);
wbx_status tempo_check_call(const ClipSrc& src, const OnsetCall& k, F0Call* track, const char** why);   // (sets track's range: the hops)
wbx_status onset_run(wbx_ctx* c, const ClipSrc& src, const OnsetCall& k, wbx_onset_frame* frames_out, wbx_onset_info* info, std::string* why);
wbx_status tempo_run(wbx_ctx* c, const ClipSrc& src, const OnsetCall& k, const F0Call& track, wbx_f0_frame* frames_out, wbx_f0_info* info,
                     std::string* why);
// seeing a clip's spectrum (wbx_spectrum.hip), cut the same way: the check makes no device call (wbx_spectrum.h's
// spectrum_check first, then the source, then the basis); the run works under fx_mu on the edit stream behind
// clipfx_prepare / clipfx_order and waits for the device after every launch, whose cells it copies out
wbx_status spectrum_check_call(const ClipSrc& src, const ClipSrc* basis, const SpecCall& k, const char** why);
wbx_status spectrum_run(wbx_ctx* c, const ClipSrc& src, const ClipSrc& basis, const SpecCall& k, float* power_out, wbx_spectrum_info* info,
                        std::string* why);
// aligning two clips (wbx_align.hip), cut the same way: the check makes no device call (wbx_align.h's align_check first,
// then the reference, then the clip; NULL for an unknown one); the run works under fx_mu on the edit stream behind
// clipfx_prepare / clipfx_order and waits for the device once, at the end
wbx_status align_check_call(const ClipSrc* ref, uint32_t ref_rate, const ClipSrc* src, uint32_t src_rate, const AlignCall& k, const char** why);
wbx_status align_run(wbx_ctx* c, const ClipSrc& ref, const ClipSrc& src, const AlignCall& k, wbx_align_info* info, wbx_align_point* curve_out,
                     std::string* why);
// splicing clips (wbx_splice.hip), cut the same way: the plan is wbx_splice.h's (no device call); the run works under fx_mu
// on the edit stream behind clipfx_prepare / clipfx_order and measures its result through clipfx_measure_run.  srcs[i] is
// the storage of parts[i]'s source (layer 2 copies it out of the pool under the editor lock)
wbx_status splice_run(wbx_ctx* c, const ClipSrc* srcs, const wbx_splice_part* parts, uint32_t n_parts, const SplicePlan& plan,
                      uint32_t channels, uint64_t n_frames, ClipSlot& slot, wbx_clip_stats* stats, std::string* why);
hipError_t join_sum(wbx_ctx* c);
hipError_t join_alt(wbx_ctx* c);
hipError_t sync_main(wbx_ctx* c);          // the host waits for the main stream and every mix / sum beside it
hipStream_t pick_mix_stream(const wbx_ctx* c, uint32_t K, bool alternate);   // (a choice, stored nowhere: RenderCall::mix_stream)
void drain_events(wbx_ctx* c, int upto = 0);
wbx_status upload_tables(wbx_ctx* c, uint32_t n_tracks);
wbx_status ensure_result_buffers(wbx_ctx* c, uint32_t K, uint32_t N);
wbx_status ensure_template_capacity(wbx_ctx* c, size_t n);
wbx_status ensure_gen_capacity(wbx_ctx* c, size_t rows);
wbx_status ensure_pool_slack(wbx_ctx* c);   // twice the default overflow pool (renders planned by segments; not when the host fixed max_segments)
wbx_status launch_pre_render(wbx_ctx* c, hipStream_t on);
// mix + sum over the current plan buffer as `call` says; *one_launch (if asked for): the block ran as the one-launch callback
wbx_status launch_mix_sum(wbx_ctx* c, uint32_t K, uint32_t N, const RenderCall& call, bool* one_launch = nullptr);
wbx_status plan_status_to_error(wbx_ctx* c, uint32_t bits);
wbx_status render_status(wbx_ctx* c);      // the latched hand-over failures of chained renders (the streams must be idle)
float* begin_master(wbx_ctx* c, float* target, hipStream_t writer, hipError_t* err);   // target: the caller's buffer, or null
RenderShape render_shape(const wbx_ctx* c, uint32_t K, uint32_t N, bool callback);   // choose_shape over the context's facts

// wbx_dist.hip
float* dist_begin_render(wbx_ctx* c, hipStream_t sum_stream, hipError_t* err);
const float* dist_mix_init(wbx_ctx* c, uint32_t K, hipStream_t mix_stream, wbx_status* st);
bool dist_receives_running_sum(const wbx_ctx* c);   // chain mode, rank > 0: every render continues the previous rank's sum
hipError_t dist_mix_issued(wbx_ctx* c, hipStream_t mix_stream);
void dist_destroy(wbx_ctx* c);

}  // namespace wbx
