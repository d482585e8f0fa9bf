/*
 * wbx.h — C ABI of the MI355X-native whitebox mix path (libwbx.so).
 *
 * Drop-in boundary for the reference's per-block multitrack mix
 *   Engine::process -> Track::process -> dsp::Sampler::stream / dsp::apply_gain /
 *   VUMeter::push_samples -> AudioBuffer::mix -> master clamp
 * (reference: src/engine/engine.cpp:1576-1654, src/engine/track.cpp:587-736,
 *  src/dsp/sampler.cpp:34-59,88-210, src/dsp/dsp_ops.h:27-31, src/engine/vu_meter.h:20-30,
 *  src/core/audio_buffer.h:73-82).
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 *   Layer 1  wbx_ctx      the device mix runtime.  The HOST keeps the reference's own clip
 *                         sequencer (Track::process_event) and hands the device, per block and
 *                         track, the Sampler::stream calls it would have made ("segments") plus
 *                         the block-rate gains; the device does every per-sample operation.
 *   Layer 2  wbx_engine   the whole path, sequencer included, resident on the device behind the
 *                         reference's Engine/Track surface (set_bpm, add_track, add_audio_clip,
 *                         Track::set_volume/pan/mute, play/stop, process).
 *
 * Conventions: every call returns wbx_status (0 = ok; negatives mirror the reference's
 * PluginResult, src/plughost/plugin_interface.h:24-29, plus device errors); host pointers are
 * caller-owned, device memory is ctx-owned; no callbacks into the host; nothing here falls back to the CPU
 * — without a gfx950 device wbx_create/wbx_engine_create return WBX_ERR_NO_DEVICE.
 * Threads: layer 1 (wbx_ctx) has one submitting thread per ctx.  Layer 2 (wbx_engine) has the reference's
 * contract: ONE audio thread in wbx_engine_process / wbx_engine_render, which hold the engine's editor lock for
 * the host side of the block (Engine::process, engine.cpp:1587-1651), and ONE UI thread for everything else —
 * its edits take the same lock, wbx_track_set_volume / _pan / _mute and wbx_engine_solo_track go through a
 * per-track single-producer ring of 64 messages without it (track.cpp:47-79, core/queue.h:142-196),
 * wbx_engine_set_bpm is an atomic store (engine.cpp:24-30).
 */
#ifndef WBX_H
#define WBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int wbx_status;
enum {
  WBX_OK = 0,
  WBX_ERR_FAILED = -1,        /* PluginResult::Failed        */
  WBX_ERR_UNIMPLEMENTED = -2, /* PluginResult::Unimplemented */
  WBX_ERR_UNSUPPORTED = -3,   /* PluginResult::Unsupported   */
  WBX_ERR_INVALID = -4,       /* bad argument                */
  WBX_ERR_NO_DEVICE = -5,     /* no HIP device / not gfx950  */
  WBX_ERR_DEVICE = -6,        /* HIP runtime error (see wbx_last_error) */
  WBX_ERR_OOM = -7,
  WBX_ERR_OVERFLOW = -8       /* more segments in one block than the plan can hold */
};

/* AudioFormat of clip storage — values of the reference enum, src/core/audio_format.h:7-20.
 * I24 clips are stored in 32-bit containers, as the reference does (src/dsp/sample.cpp:20). */
enum { WBX_FMT_I16 = 3, WBX_FMT_I24 = 5, WBX_FMT_I32 = 7, WBX_FMT_F32 = 9 };

/* Interleaved device-output formats for wbx_*_fetch_interleaved — reference converters
 * src/core/audio_format_conv.cpp:5-91 (values of the reference's AudioFormat enum).
 * WBX_OUT_I24 (packed 3-byte samples, audio_format_conv.cpp:22-43) mirrors the reference's bytes, quirk included:
 * its writer's destination index ignores the channel and the channel count, so every channel overwrites bytes
 * [0, 3*F) of a block's output and the LAST channel is what remains; the other 3*F*(C-1) bytes of the block's
 * 3*F*C-byte region are never written (wbx leaves them as the caller passed them).
 * Float -> integer conversions give the x86 results the reference build produces, also out of range (master
 * left un-clamped, NaN): cvttss2si / cvttsd2si return 0x80000000, the i16 / i24 paths then truncate. */
enum { WBX_OUT_I16 = 3, WBX_OUT_I24 = 5, WBX_OUT_I24_X8 = 6, WBX_OUT_I32 = 7, WBX_OUT_F32 = 9 };

typedef struct wbx_config {
  int32_t device;          /* HIP device ordinal */
  uint32_t max_tracks;     /* N upper bound */
  uint32_t max_blocks;     /* K upper bound per submit/render (1..4096) */
  uint32_t block_frames;   /* F, Engine::audio_buffer_size (reference default 512, src/config.cpp:146); multiple of 4 */
  uint32_t channels;       /* C, output channels: 1 or 2 (reference: 2, src/config.cpp:224) */
  uint32_t sample_rate;    /* destination rate, Engine::audio_sample_rate */
  uint32_t group_size;     /* tracks summed in index order by one workgroup; the master is the in-order sum of the group
                              sums, so group_size >= N reproduces the reference's strictly sequential order (engine.cpp:
                              1600-1617) bit for bit.  0 = the library picks: renders of >= 1024 blocks add ALL tracks of a
                              block (of a bus) in track order — the reference's order, bit-exact master, at the full rate:
                              128-track workgroups that continue each other's running sum, the blocks of the render supply
                              the parallelism (blocks shorter than 256 lanes count by the workgroup: 2048 blocks of 256
                              frames, 4096 of 128 — wbx_render_order tells); shorter renders take groups of 128 (when
                              max_blocks == 1, the audio-callback configuration: one group up to 16 tracks and one TRACK per group up to
                              64 — both the reference's order bit for bit — then 4 / 8 / 16 tracks above 64 / 256 / 512
                              tracks), within 1e-6 RMS of the reference's order at mix-bus levels (DESIGN.md "Summation
                              order" states the levels). */
  uint32_t max_segments;   /* extra (beyond one per track-block) segment slots per launch; 0 = default */
  void* stream;            /* hipStream_t to launch on, or NULL: the ctx creates its own */
} wbx_config;

typedef struct wbx_ctx wbx_ctx;
typedef struct wbx_engine wbx_engine;

/* One Sampler::stream call of one track in one block (dsp/sampler.h:29-35, sampler.cpp:88-210),
 * with the sampler state the host's sequencer holds at that point. */
typedef struct wbx_segment {
  double sample_offset;    /* Sampler::sample_offset_ before the call */
  double playback_speed;   /* Sampler::playback_speed_ ((src_rate/dst_rate)*clip speed, sampler.h:24) */
  uint32_t clip;           /* clip id given to wbx_clip_upload */
  uint32_t buffer_offset;  /* first destination frame in the block */
  uint32_t num_samples;    /* frames requested (the device applies the clip-tail limit of sampler.cpp:102-104) */
  float gain;              /* AudioClip::gain */
} wbx_segment;

/* ---- library ------------------------------------------------------------------------------- */
const char* wbx_version(void);
int wbx_device_count(void);                 /* gfx950 devices visible; 0 without a GPU (never an error) */
const char* wbx_status_string(wbx_status);

/* ---- layer 1: device mix runtime ------------------------------------------------------------
 * replaces the body of the per-track loop of Engine::process (engine.cpp:1600-1617) and the master
 * clamp (engine.cpp:1627-1636). */
wbx_status wbx_create(const wbx_config* cfg, wbx_ctx** out);
void wbx_destroy(wbx_ctx* ctx);
const char* wbx_last_error(const wbx_ctx* ctx);

/* Clip audio -> HBM (planar, +16 zero frames of tail padding like Sample::sample_padding,
 * src/dsp/sample.h:19, sample.cpp:127,140).  Replaces the storage half of `struct Sample`
 * (sample.h:18-28).  frames < 2^31-16. */
wbx_status wbx_clip_upload(wbx_ctx* ctx, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                           uint64_t frames, const void* const* planar);
/* Device-side synthetic clip (bench/test helper; integer-hash generator, DESIGN.md "Synthetic input"). */
wbx_status wbx_clip_synth(wbx_ctx* ctx, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                          uint64_t frames, uint64_t seed, uint32_t key_track, float amp);
wbx_status wbx_clip_free(wbx_ctx* ctx, uint32_t clip);
/* Clip storage in numbers.  Clip audio lives in slabs (64 MiB, 256 MiB, then 1 GiB each) carved up in order; the extent of
 * a freed or replaced clip is reused by the next clip that fits (first fit), a slab whose last clip went is empty again;
 * slabs go back to the driver with the context.  bytes_reserved: what the pool holds from the driver; bytes_live: what
 * its clips occupy.  Any pointer may be NULL. */
wbx_status wbx_clip_pool_stats(wbx_ctx* ctx, uint32_t* n_slabs, uint64_t* bytes_reserved, uint64_t* bytes_live);

/* Clip ingest: interleaved frames as a decoder delivers them (sf_readf_short/int/float, drmp3_read_pcm_frames_f32)
 * -> the same planar storage.  Replaces deinterleave_samples<T> + the allocation/padding of Sample::load_file
 * (src/dsp/sample.cpp:29-43, :127-142, :154-183); the transposition runs on the GPU.
 *   wbx_clip_upload_interleaved  `interleaved` is host memory ([frames][channels]); staged through pinned chunks
 *   wbx_clip_ingest_device       `interleaved` is device memory, 16-byte aligned (a GPU decoder / own staging) */
wbx_status wbx_clip_upload_interleaved(wbx_ctx* ctx, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                                       uint64_t frames, const void* interleaved);
wbx_status wbx_clip_ingest_device(wbx_ctx* ctx, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                                  uint64_t frames, const void* device_interleaved);
/* planar clip audio back to the host (tests; also Sample::get_read_pointer's role for host-side tools) */
wbx_status wbx_clip_download(wbx_ctx* ctx, uint32_t clip, uint32_t channel, void* dst);

/* Export: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels (a take, a bounce, any
 * uploaded F32 clip) as interleaved samples of a device format — the way into an audio file.  The counterpart of
 * wbx_clip_upload_interleaved; the conversion is wbx_fetch_interleaved's (core/audio_format_conv.cpp:5-91: asymmetric
 * scales, truncation, the x86 results out of range), run on the device in the pass that interleaves.
 *   layout   sample i, channel c at index i*C + c in EVERY format.  WBX_OUT_I24 here is TRUE packed interleave: byte k of
 *            the 24-bit sample at dst[(i*C + c)*3 + k].  This is deliberately NOT wbx_fetch_interleaved's WBX_OUT_I24,
 *            which mirrors the reference writer's quirk (every channel overwrites bytes [0, 3F)): that is right for parity
 *            of the audio callback and useless for a file, which needs every channel
 *   flags    WBX_EXPORT_CLAMP: every sample first goes through the master's clamp, x > 1 ? 1 : (x < -1 ? -1 : x)
 *            (engine.cpp:1627-1636; NaN passes).  Without it a post-fader stem beyond +-1.0 wraps as the reference's
 *            conversion does (1.5 as 16-bit: -16386)
 *   stats    (may be NULL) per channel, over the SOURCE values of this call's range, before any clamp: peak = max |x|
 *            (a NaN never raises it; 0 for an all-NaN range), over = samples with x > 1 or x < -1, nans = NaN samples
 *   dst      caller-owned host memory of wbx_export_bytes(out_format, channels, n_frames) bytes, pageable or from
 *            wbx_host_alloc (then the copy engine writes it directly)
 *   staging  the range goes in chunks through three pinned slots made at first use and freed with the context: device
 *            and pinned memory used do not depend on the clip's length; the kernel and transfer of the next chunks run
 *            while the host copies one out.  A long clip may be exported in several calls with advancing first_frame
 *            (streaming into a file): the bytes are those of one call, the stats are per call
 *   order    runs on a stream of its own (no mix or sum stream), ordered after everything enqueued so far on the
 *            context's main and upload streams; returns when dst is complete
 * WBX_ERR_INVALID: unknown clip, n_frames == 0, first_frame + n_frames > the clip's frames, dst NULL, flags other than
 * WBX_EXPORT_CLAMP.  WBX_ERR_UNSUPPORTED: an unknown out_format, a clip whose storage format is not F32 (the reference
 * has no integer-to-device-format path).  dst is untouched after a refusal. */
enum { WBX_EXPORT_CLAMP = 1 };
typedef struct wbx_export_stats {
  float peak[2];
  uint64_t over[2];
  uint64_t nans[2];
} wbx_export_stats;
uint64_t wbx_export_bytes(int out_format, uint32_t channels, uint64_t n_frames);   /* 0 for an unknown format */
wbx_status wbx_clip_export(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, int out_format,
                           uint32_t flags, void* dst, wbx_export_stats* stats);
/* Frames per staging chunk of later exports: a multiple of 8, 8 .. 2^24; 0 = the default (2^20).  For tests, which reach
 * chunk seams with 1000-frame clips this way (cf. wbx_engine_set_record_chunk); results do not depend on it. */
wbx_status wbx_set_export_chunk(wbx_ctx* ctx, uint32_t frames);

/* Editing clips: measure a frame range of a resident F32 clip of 1 or 2 channels (the class of clip wbx_clip_export takes),
 * or derive a NEW F32 clip from it — trim, reverse, channel mode, gain, fade-in, fade-out — without the samples leaving
 * HBM.  No reference counterpart as a whole: dsp::find_abs_maximum and dsp::gain (dsp/dsp_ops.h:10-25) and Sample::resize
 * (sample.cpp:69-110) are the pieces; AudioClip::fade_start / fade_end (engine/clip.h:41-42) are stored and read by nothing.
 * Both calls run on a stream of their own (no mix or sum stream), ordered after everything enqueued so far on the
 * context's main and upload streams, and return when the result is complete.
 *
 * wbx_clip_measure: per channel over [first_frame, first_frame + n_frames)
 *   peak        max |x| taken by `a > peak` from 0: a NaN never raises it (the export's rule)
 *   peak_frame  the smallest frame, relative to first_frame, whose |x| equals peak; 0 when peak is 0
 *   min, max    signed, NaNs skipped, -0.0 below +0.0; +0.0 for both when no sample was counted
 *   over, nans  samples with x > 1 or x < -1 / NaN samples
 *   sum, sum_sq fp64 over the samples that are no NaN, every square formed in fp64
 * Every field but sum and sum_sq is independent of the order of reduction, hence exact; those two are summed in an order
 * that is not fixed: |error| <= (n - 1) * 2^-53 * sum |term|.
 *
 * wbx_clip_derive: dst_clip becomes a new F32 pool clip of n_frames frames (plus the pool's 16 zero frames of padding) at
 * the source's sample rate; an existing dst_clip is replaced as wbx_clip_upload would replace it; dst_clip != src_clip.
 * Output frame j in [0, n) of output channel c, with every operation a single IEEE fp32 round-to-nearest one:
 *   source frame  s = first_frame + j, or first_frame + n - 1 - j with WBX_EDIT_REVERSE
 *   channel       WBX_CH_KEEP      src[c][s]                     (mono or stereo)
 *                 WBX_CH_SWAP      src[1 - c][s]                 (stereo)
 *                 WBX_CH_LEFT / WBX_CH_RIGHT   that channel, mono result   (stereo)
 *                 WBX_CH_MONO_MIX  fl(fl(L + R) * 0.5f), mono result       (stereo)
 *                 WBX_CH_DUAL_MONO src[0][s] on both channels of a stereo result (mono)
 *   gain          y = fl(x * gain), always multiplied (invert: gain = -1)
 *   fade-in       j < fade_in:       t = (float)((double)j / (double)fade_in),               y = fl(y * w(t))
 *   fade-out      j >= n - fade_out: t = (float)((double)(n - 1 - j) / (double)fade_out),    y = fl(y * w(t))   (after the fade-in)
 *   w(t)          WBX_FADE_LINEAR t;  WBX_FADE_SQUARE fl(t*t);  WBX_FADE_SMOOTH fl(fl(t*t) * fl(3 - fl(2*t)))
 *   NaN           a result that is a NaN is stored as 0x7FC00000, whatever its source's payload
 * Frames outside both fades get no fade multiplication; the first frame of a fade-in and the last of a fade-out have
 * weight 0, so a reversed edit with a fade-in is bit-equal to the reverse of the forward edit with that fade-out.
 * stats_of_result (may be NULL): wbx_clip_measure of the whole result, taken in the same pass from the values stored.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: unknown source clip, NULL
 * descriptor, n_frames == 0, a range past the clip, dst_clip == src_clip, an unknown flag, mode or shape, a fade longer
 * than n_frames, a channel mode that does not fit the source's channel count; WBX_ERR_UNSUPPORTED: a source whose storage
 * format is not F32.  WBX_ERR_OOM when wbx_clip_pool_limit does not allow the new clip (nothing is left allocated).
 * wbx_clipfx_pass_frames (host-only, no device): the frames ONE pass of the measure / derive kernel's capped grid covers; a
 * longer range is finished by further passes of the same launch.  For tests that must reach such a pass; nothing else
 * reads it. */
enum { WBX_EDIT_REVERSE = 1 };
enum { WBX_CH_KEEP = 0, WBX_CH_SWAP = 1, WBX_CH_LEFT = 2, WBX_CH_RIGHT = 3, WBX_CH_MONO_MIX = 4, WBX_CH_DUAL_MONO = 5 };
enum { WBX_FADE_LINEAR = 0, WBX_FADE_SQUARE = 1, WBX_FADE_SMOOTH = 2 };
typedef struct wbx_clip_stats {   /* 104 bytes */
  float peak[2];
  float min[2];
  float max[2];
  uint64_t peak_frame[2];
  uint64_t over[2];
  uint64_t nans[2];
  double sum[2];
  double sum_sq[2];
} wbx_clip_stats;
typedef struct wbx_clip_edit_desc {   /* 56 bytes */
  uint64_t first_frame, n_frames;
  uint32_t flags;          /* WBX_EDIT_* */
  int32_t channel_mode;    /* WBX_CH_* */
  float gain;
  uint32_t _pad;
  uint64_t fade_in, fade_out;   /* frames, each <= n_frames */
  int32_t fade_in_shape, fade_out_shape;   /* WBX_FADE_* */
} wbx_clip_edit_desc;
uint64_t wbx_clipfx_pass_frames(void);
wbx_status wbx_clip_measure(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, wbx_clip_stats* out);
wbx_status wbx_clip_derive(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, const wbx_clip_edit_desc* d,
                           wbx_clip_stats* stats_of_result);

/* Converting a clip's sample rate: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels
 * become a NEW F32 clip at dst_rate through a band-limited (windowed-sinc, polyphase) filter, without the samples leaving
 * HBM — a file conformed once to the session rate then plays at speed 1.0 through the mix's unity row mode instead of its
 * per-block two-tap interpolation (Sampler::stream's sample_linear rows), and a bounce can leave at another rate than the
 * session's.  No reference counterpart: Sampler::stream is its only resampler.  This text is the specification;
 * tests/resample_model.py restates it in numpy and the device equals that BIT FOR BIT.
 *   ratio     g = gcd(src_rate, dst_rate), L = dst_rate / g, M = src_rate / g.  Output frame j lies at source time j*M/L:
 *             in 64-bit integers t = j*M, i = t div L, p = t mod L (the phase).  n source frames give
 *             n_out = ceil(n*L / M) output frames
 *   quality   WBX_SRC_FAST / GOOD / BEST: (Z, beta, frac) = (12, 7.0, 0.85) / (24, 10.0, 0.92) / (48, 14.0, 0.96).
 *             rho = L < M ? (double)L / (double)M : 1.0; cutoff c = frac * rho; half width H = ceil(Z / rho) source frames
 *             (in integers: ceil(Z*M / L) when L < M, else Z); T = 2H taps
 *   table     fp64 on the host, for p in [0, L), k in [0, T):  d = (double)(k - (H-1)) - (double)p / (double)L,
 *               h64[p][k] = ((c * sinc(c*d)) * I0(beta * sqrt(max(0, 1 - (d/H)*(d/H))))) / I0(beta)
 *             each phase divided by the sum of its T values (added in ascending k), then rounded ONCE to fp32: h[p][k].
 *             sinc(x) = x == 0 ? 1 : sinpi(x) / (pi*x) and I0 are built from + - * / floor sqrt alone in a fixed number of
 *             steps (libm's sin differs between platforms in the last place):
 *               sinpi(x)  a = |x|; r = a - 2*floor(a/2) (exact); r >= 1: r = r - 1, the sign flips; r > 1/2: r = 1 - r;
 *                         y = pi*r (pi = 3.141592653589793); s = 1; for n = 13 .. 1: s = 1 - (s*(y*y)) / ((2n)(2n+1));
 *                         result sign * (y*s)
 *               I0(x)     h = x/2; t = s = 1; for k = 1 .. 39: t = (t*h)/k, s = s + t*t
 *   output    channel c, frame j:  acc = 0.0 (fp64); for k = 0 .. T-1 ascending: acc = acc + (double)h[p][k] *
 *             (double)x[c][i - (H-1) + k]  (the product of two fp32 values is exact in fp64);  y = (float)acc.
 *             x is ZERO outside [first_frame, first_frame + n_frames), whatever the clip holds there — the range is
 *             converted as if it were a whole file.  A NaN result is stored as 0x7FC00000 (wbx_clip_derive's rule).
 *             Only the order of the T additions is fixed; output frames are independent of each other
 * The filter is no identity at any ratio, so equal rates are refused rather than copied (wbx_clip_derive copies).
 * wbx_resample_plan / _frames / _table are host-only and need no device: the plan's numbers, n_out (0 when refused: a rate
 * of 0, equal rates, L > 1280, or n_out >= 2^31 - 16), and the table in phase order [p][k] (WBX_ERR_INVALID when cap_floats
 * is below L*T; `out` untouched after any refusal).
 * wbx_clip_resample: dst_clip becomes a new F32 pool clip of n_out frames (plus the pool's 16 zero frames of padding) at
 * dst_rate with the source's channel count, replaced or allocated as wbx_clip_derive does it, on the same stream and
 * behind the same ordering; one edit or conversion runs at a time.  stats_of_result (may be NULL): wbx_clip_measure of
 * the whole result, a second pass over the output only.  The coefficient table is kept on the device per context and
 * (L, M, quality) after its first use.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: unknown source clip,
 * n_frames == 0, a range past the clip, dst_clip == src_clip, unknown quality, dst_rate == 0, dst_rate == the source's
 * rate, n_out >= 2^31 - 16; WBX_ERR_UNSUPPORTED: a source whose storage format is not F32 (bounce a track pre-fader to get
 * one) or with more than 2 channels, L > 1280 (22050 -> 192000 has 1280), T > 512 (192000 -> 32000 at BEST has 576).
 * WBX_ERR_OOM when wbx_clip_pool_limit does not allow the new clip (nothing is left allocated).
 * wbx_resample_launch_shape (host-only, no device): how a conversion to n_out output frames is launched — a workgroup's
 * tile of output frames, the source span it stages, the tiles, and the workgroups that share them (fewer than the tiles
 * once the grid's cap is reached: then a workgroup takes further tiles, one pass of the grid after another).  What
 * wbx_resample_plan refuses is refused with its status; WBX_ERR_INVALID for n_out of 0 or >= 2^31 - 16 or a NULL pointer.
 * For tests that must reach a second pass; nothing else reads it. */
enum { WBX_SRC_FAST = 0, WBX_SRC_GOOD = 1, WBX_SRC_BEST = 2 };
typedef struct wbx_resample_info {   /* 24 bytes */
  uint32_t L, M;             /* dst_rate / g, src_rate / g */
  uint32_t half_width;       /* H */
  uint32_t taps;             /* T = 2H */
  uint64_t table_floats;     /* L * T */
} wbx_resample_info;
wbx_status wbx_resample_plan(uint32_t src_rate, uint32_t dst_rate, int quality, wbx_resample_info* out);
uint64_t wbx_resample_frames(uint32_t src_rate, uint32_t dst_rate, uint64_t n_frames);
wbx_status wbx_resample_table(uint32_t src_rate, uint32_t dst_rate, int quality, float* out, size_t cap_floats);
wbx_status wbx_resample_launch_shape(uint32_t src_rate, uint32_t dst_rate, int quality, uint64_t n_out, uint32_t* tile,
                                     uint32_t* span, uint32_t* n_tiles, uint32_t* grid);
wbx_status wbx_clip_resample(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                             uint32_t dst_rate, int quality, wbx_clip_stats* stats_of_result);

/* Splicing clips: a list of PARTS — each a wbx_clip_derive edit of some resident F32 clip, placed at an output frame —
 * becomes ONE new F32 clip, without the samples leaving HBM: takes comped, a crossfade between two clips, a bounce joined
 * to the take before it, a loop repeated, silence inserted, a region cut out.  wbx_clip_derive has one source; this is the
 * call with several.  No reference counterpart: AudioClip::fade_start / fade_end (engine/clip.h:41-42) are read by nothing
 * and Engine::reserve_track_region (engine.cpp:478-569) trims overlapping clips, it never blends them.  This text is the
 * specification; tests/splice_model.py restates it in numpy and the device equals that BIT FOR BIT.
 *   the result    dst_clip becomes a new F32 pool clip of `channels` (1 or 2) x n_frames frames (plus the pool's 16 zero
 *                 frames of padding) at the sources' common sample rate; an existing dst_clip is replaced as
 *                 wbx_clip_upload would replace it; dst_clip is no part's source
 *   a part        part p has the value v_p[c][k], k in [0, n_p): exactly what wbx_clip_derive would STORE for frame k of the
 *                 edit (first_frame, n_frames, flags, channel_mode, gain, fade_in, fade_out, shapes) of src_clip — the same
 *                 operations in the same order with the same single roundings ("Editing clips" above)
 *   a frame       output frame j of channel c walks, in LIST order, the parts that cover j (at_p <= j < at_p + n_p):
 *                 the first one ASSIGNS acc = v_p[c][j - at_p]; every later one does acc = fl(acc + v_p[c][j - at_p]), one
 *                 fp32 round-to-nearest addition.  A frame no part covers is +0.0f.  A NaN result is stored as 0x7FC00000
 * Hence: a one-part splice with at = 0 and n_frames = n_p is bit-equal to wbx_clip_derive (-0.0 survives: it is assigned,
 * not added to a zero); the order of the additions is the list's and nothing else's; a crossfade is two overlapping parts,
 * one with a fade-out and one with a fade-in; concatenation, inserted silence, a removed region and a loop (one source in
 * many parts) are part lists.
 * stats_of_result (may be NULL): wbx_clip_measure of the whole result, a second pass over the output only.
 * Stream and ordering are wbx_clip_derive's: the edits' stream, behind everything enqueued so far on the context's main
 * and upload streams; one edit, conversion or splice runs at a time; the call returns when the result is complete.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: parts NULL or n_parts == 0,
 * n_frames == 0 or >= 2^31 - 16, channels not 1 or 2, an unknown source clip, dst_clip equal to a part's source, a part
 * with no frames, with a range past its clip or with at + n_p > n_frames, an unknown flag, mode or shape, a fade longer
 * than its part, a mode that does not fit its source's channel count or does not yield `channels`, sources whose sample
 * rates differ (convert first: wbx_clip_resample); WBX_ERR_UNSUPPORTED: a source whose storage format is not F32,
 * n_parts > 65536, a tile table (below) of more than 2^24 entries.  WBX_ERR_OOM as for wbx_clip_derive.
 * wbx_splice_plan is host-only and needs no device: the refusals above (all but dst_clip's) against a table of sources
 * indexed by src_clip (an id >= n_sources, or an entry with channels == 0, is an unknown clip), and the table the kernel
 * walks — the output cut into tiles of 512 frames, tile_off[t] .. tile_off[t + 1] indexing tile_parts[], the indices of the
 * parts that touch tile t, ascending.  *n_tiles and *n_entries (each may be NULL) are always given on WBX_OK; the arrays are
 * filled when both are non-NULL and cap_off >= n_tiles + 1 and cap_parts >= n_entries (WBX_ERR_INVALID when a capacity
 * is too small; nothing written then). */
typedef struct wbx_splice_part {   /* 64 bytes */
  uint32_t src_clip;
  uint32_t flags;                  /* WBX_EDIT_REVERSE */
  uint64_t first_frame, n_frames;  /* the source range */
  uint64_t at;                     /* output frame of the part's first frame */
  int32_t channel_mode;            /* WBX_CH_* */
  float gain;
  uint64_t fade_in, fade_out;      /* frames, each <= n_frames */
  int32_t fade_in_shape, fade_out_shape;   /* WBX_FADE_LINEAR / SQUARE / SMOOTH */
} wbx_splice_part;
typedef struct wbx_splice_source {   /* 24 bytes */
  uint32_t channels;               /* 0: no such clip */
  uint32_t sample_rate;
  uint64_t frames;
  int32_t format;                  /* WBX_FMT_* */
  uint32_t _pad;
} wbx_splice_source;
wbx_status wbx_splice_plan(uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts,
                           const wbx_splice_source* sources, uint32_t n_sources, uint64_t* n_tiles, uint64_t* n_entries,
                           uint32_t* tile_off, size_t cap_off, uint32_t* tile_parts, size_t cap_parts);
wbx_status wbx_clip_splice(wbx_ctx* ctx, uint32_t dst_clip, uint32_t channels, uint64_t n_frames,
                           const wbx_splice_part* parts, uint32_t n_parts, wbx_clip_stats* stats_of_result);

/* Measuring a clip's loudness: ITU-R BS.1770-4 / EBU R 128 figures of frames [first_frame, first_frame + n) of a resident
 * F32 clip of 1 or 2 channels at `rate` — integrated loudness, momentary and short-term maxima, loudness range (EBU Tech
 * 3342) and true peak — without the samples leaving HBM: a bounce is delivered to a loudness target (-14, -16, -23 LUFS)
 * under a true-peak ceiling, and wbx_clip_measure knows only the sample peak and a sum of squares.  No reference
 * counterpart (dsp/dsp_ops.h stops at find_abs_maximum).  This text is the specification; tests/loudness_model.py restates
 * it in numpy, and the coefficients, the hop energies, the powers, the counts and the true peak equal that BIT FOR BIT.
 *   range     8000 <= rate <= 384000.  hop = (rate + 5) / 10 in integers (100 ms); hops = n / hop: only complete hops
 *             count, trailing frames are ignored.  x is ZERO outside the range, whatever the clip holds there, and a frame
 *             outside the range is never read.  A NaN sample enters the filter as 0.0
 *   K filter  two biquads, coefficients in fp64 on the host:
 *               stage 1 (shelf)      f0 = 1681.974450955533, Q = 0.7071752369554196, Vh = 1.5848647011308556,
 *                                    Vb = 1.2587209302325617 (decimal literals, no pow);  K = tan(pi*f0/rate), KQ = K/Q, KK = K*K,
 *                                    a0 = (1 + KQ) + KK;  b0 = ((Vh + Vb*KQ) + KK)/a0, b1 = (2*(KK - Vh))/a0,
 *                                    b2 = ((Vh - Vb*KQ) + KK)/a0;  a1 = (2*(KK - 1))/a0, a2 = ((1 - KQ) + KK)/a0
 *               stage 2 (high-pass)  f0 = 38.13547087602444, Q = 0.5003270373238773;  b = [1, -2, 1], a1 and a2 as above
 *             tan is built from + - * / alone in a fixed number of steps (libm's last place differs between platforms):
 *               y = (pi*f0) / (double)rate (pi = 3.141592653589793); y2 = y*y; s = c = 1;
 *               for n = 13 .. 1: s = 1 - (s*y2) / ((2n)(2n+1)), c = 1 - (c*y2) / ((2n-1)(2n));  K = (y*s) / c
 *             At 48000 Hz this is the standard's published table to its 14 decimals
 *   energies  per channel c and hop h both stages run in fp64 from rest (all state 0), starting at frame (h - 2)*hop of
 *             the range (frames below 0 are zero) through frame (h + 1)*hop - 1, direct form I, per stage
 *               y = ((((b0*x + b1*x1) + b2*x2) - a1*y1) - a2*y2)
 *             every * + - a single IEEE fp64 operation, nothing fused.  E[c][h] = the sum over the hop's own `hop` frames,
 *             ascending, of e = e + v*v, v being stage 2's output.  The first three hops ARE one sequential pass; later
 *             hops equal it to about 1e-14 relative (the filter's memory of what lies two hops back is below fp64's
 *             resolution).  The segmented definition is the specification, not an approximation of one: hops are
 *             independent of each other, which is what lets a lane own a hop
 *   gate      on the host in fp64, on powers; log10 is called only on the final figures.  blocks = hops >= 4 ? hops - 3 : 0;
 *             block j: s_c = ((E[c][j] + E[c][j+1]) + E[c][j+2]) + E[c][j+3], z_j = (s_0 [+ s_1]) / (double)(4*hop), both
 *             channels at weight 1.0.  Absolute gate: z_j > 1.1724653045822981e-07 (= 10^((-70 + 0.691)/10)); m = the
 *             ascending sum of the passing z_j divided by their count; relative gate: z_j > m * 0.1.  gated_power = the
 *             ascending sum of the z_j that pass both, divided by their count (blocks_gated);
 *             integrated = -0.691 + 10*log10(gated_power), -infinity when no block passes
 *   momentary_max   the same formula over the largest z_j, ungated; -infinity without a block
 *   short_term_max  windows of 30 hops starting at every hop: per channel s = 0, s = s + E[c][j+k] for k = 0 .. 29,
 *                   w_c = s / (double)(30*hop); w_j = w_0 [+ w_1]; the formula over the largest w_j
 *   range_lu        over the windows w_j at j = 0, 10, 20, ...: keep those above the absolute gate; then those above
 *                   0.01 x (their ascending sum / their count); sort the n survivors ascending;
 *                   lo = s[(size_t)((n-1)*0.10 + 0.5)], hi = s[(size_t)((n-1)*0.95 + 0.5)]; 10*log10(hi/lo); 0 when n < 2
 *   true_peak       with WBX_LOUD_TRUE_PEAK, per channel.  factor = 4 below 96000 Hz, 2 below 192000, else 1 (`oversampling`).
 *                   factor > 1: the largest |value| among the range's own samples and every output frame of
 *                   "Converting a clip's sample rate" from rate to factor*rate at WBX_SRC_GOOD (L = factor, M = 1, T = 48,
 *                   the same table, fp64 accumulation in ascending tap order, one rounding to fp32); nothing is stored.
 *                   factor 1: the sample peak.  The maximum is taken by `a > peak` from 0 (wbx_clip_measure's rule: a NaN
 *                   never raises it) and is independent of the order of reduction, hence exact.  A range cut hard out of a
 *                   louder signal overshoots at its ends, legitimately; 0 when not asked for
 * A range shorter than 4 hops is no error: blocks = 0 and integrated = -infinity.
 * wbx_loudness_hop_frames (0 outside the supported rates), wbx_loudness_hops, wbx_loudness_coefficients (out[0..4] stage
 * 1's b0 b1 b2 a1 a2, out[5..9] stage 2's; WBX_ERR_UNSUPPORTED outside the supported rates) and wbx_loudness_gate (E is
 * [channels][hops]; fills every field but true_peak and oversampling, which become 0; WBX_ERR_INVALID: channels not 1 or 2,
 * hop_frames == 0, NULL out, NULL E with hops > 0) are host-only and need no device.
 * wbx_clip_loudness runs on the edits' stream behind wbx_clip_derive's ordering, one edit or measurement at a time, and
 * returns when *out is complete.  hop_energy (may be NULL): E as the device wrote it, [channels][hops].
 * Refused before any device call — WBX_ERR_INVALID: unknown clip, NULL out, n_frames == 0, a range past the clip, an unknown
 * flag, cap_doubles below channels*hops when hop_energy is given; WBX_ERR_UNSUPPORTED: a source whose storage format is not
 * F32, more than 2 channels, a rate outside 8000 .. 384000, with true peak factor*n_frames >= 2^31 - 16.
 * wbx_true_peak_launch_shape (host-only, no device): the true peak's factor at `rate`, the tiles of oversampled frames a
 * range of n_frames has and the workgroups that share them (wbx_resample_launch_shape's meaning; both 0 at factor 1, where
 * the sample peak is wbx_clip_measure's pass).  WBX_ERR_INVALID: n_frames == 0 or a NULL pointer; WBX_ERR_UNSUPPORTED: the
 * rate, factor*n_frames >= 2^31 - 16.  For tests that must reach a second pass; nothing else reads it. */
enum { WBX_LOUD_TRUE_PEAK = 1 };
typedef struct wbx_loudness {   /* 80 bytes */
  double integrated;         /*  0: LUFS */
  double gated_power;        /*  8 */
  double momentary_max;      /* 16: LUFS */
  double short_term_max;     /* 24: LUFS */
  double range_lu;           /* 32: LU */
  float true_peak[2];        /* 40: linear */
  uint64_t hops;             /* 48 */
  uint64_t blocks;           /* 56 */
  uint64_t blocks_gated;     /* 64 */
  uint32_t hop_frames;       /* 72 */
  uint32_t oversampling;     /* 76: the true peak's factor; 0 when not asked for */
} wbx_loudness;
uint32_t wbx_loudness_hop_frames(uint32_t rate);
uint64_t wbx_loudness_hops(uint32_t rate, uint64_t n_frames);
wbx_status wbx_loudness_coefficients(uint32_t rate, double out[10]);
wbx_status wbx_true_peak_launch_shape(uint32_t rate, uint64_t n_frames, uint32_t* factor, uint32_t* n_tiles, uint32_t* grid);
wbx_status wbx_loudness_gate(uint32_t channels, uint64_t hops, uint32_t hop_frames, const double* hop_energy, wbx_loudness* out);
wbx_status wbx_clip_loudness(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t flags,
                             wbx_loudness* out, double* hop_energy, size_t cap_doubles);

/* Filtering a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels run through a
 * cascade of 1 .. 8 biquads into a NEW F32 clip of n_frames + tail_frames frames (the tail is the ring-out over zero
 * input), without the samples leaving HBM: rumble or DC removed from a take, a bounce low-passed or notched, a corrective
 * EQ baked into a frozen stem.  No reference counterpart (its filters live in plug-ins).  This text is the specification;
 * tests/filter_model.py restates it in numpy, and the coefficients, the carry matrix and every output frame equal that
 * BIT FOR BIT.
 *   design    wbx_filter_design: out = b0 b1 b2 a1 a2 (a0 divided out) of one Audio-EQ-Cookbook biquad in fp64, every
 *             operator below one IEEE operation in the order written.  gain is a LINEAR amplitude ratio (no pow) and is
 *             ignored (but checked) by the kinds without one.  sinpi is "Converting a clip's sample rate"'s:
 *               t = (2*f)/rate, h = f/rate;  sn = sinpi(t), cs = sinpi(t + 0.5);  hm = sinpi(h)*sinpi(h),
 *               hp = sinpi(h + 0.5)*sinpi(h + 0.5);  omc = 2*hm (1 - cos, without the cancellation), opc = 2*hp (1 + cos);
 *               alpha = sn/(2*q);  m2cs = 0 - 2*cs
 *               LOWPASS    a0 = 1 + alpha;  b = [hm, omc, hm];                  a1 = m2cs, a2 = 1 - alpha
 *               HIGHPASS   a0 = 1 + alpha;  b = [hp, 0 - opc, hp];              a1 = m2cs, a2 = 1 - alpha
 *               BANDPASS   a0 = 1 + alpha;  b = [alpha, 0, 0 - alpha];          a1 = m2cs, a2 = 1 - alpha   (0 dB peak)
 *               NOTCH      a0 = 1 + alpha;  b = [1, m2cs, 1];                   a1 = m2cs, a2 = 1 - alpha
 *               ALLPASS    a0 = 1 + alpha;  b = [1 - alpha, m2cs, 1 + alpha];   a1 = m2cs, a2 = 1 - alpha
 *               PEAK       A = sqrt(gain), aA = alpha*A, aoA = alpha/A;  a0 = 1 + aoA;  b = [1 + aA, m2cs, 1 - aA];
 *                          a1 = m2cs, a2 = 1 - aoA
 *               shelves    A = sqrt(gain), beta = (2*sqrt(A))*alpha, P = A*omc + opc, Q = A*opc + omc
 *               LOWSHELF   a0 = Q + beta;  b = [A*(P + beta), (2*A)*(A*omc - opc), A*(P - beta)];
 *                          a1 = 0 - 2*(A*opc - omc), a2 = Q - beta
 *               HIGHSHELF  a0 = P + beta;  b = [A*(Q + beta), 0 - (2*A)*(A*opc - omc), A*(Q - beta)];
 *                          a1 = 2*(A*omc - opc), a2 = P - beta
 *             and out = [b0/a0, b1/a0, b2/a0, a1/a0, a2/a0].  WBX_ERR_INVALID: NULL out, an unknown kind, rate == 0,
 *             freq_hz not inside (0, rate/2), q or gain not finite and > 0
 *   check     wbx_filter_check: WBX_OK when every value is finite, 1 <= n_stages <= 8 and every stage lies strictly inside
 *             the stability triangle (|a2| < 1 and |a1| < 1 + a2), else WBX_ERR_INVALID.  Any such cascade may be used, not
 *             only designed ones; coef is [n_stages][5]
 *   input     per channel x[i], i in [0, n_frames + tail_frames): (double) of the fp32 sample for i < n_frames, a sample that
 *             is not finite (NaN, +-inf) entering as 0.0; ZERO from n_frames on.  Whatever the clip holds beside the range
 *             does not count and is never read
 *   a stage   direct form I, y = ((((b0*x + b1*x1) + b2*x2) - a1*y1) - a2*y2), every * + - a single IEEE fp64 operation,
 *             nothing fused; then x2 = x1, x1 = x, y2 = y1, y1 = y
 *   cascade   stage s's input is stage s-1's output, so stage s's x1, x2 ARE stage s-1's y1, y2 and a channel's state is
 *             v = [x1, x2, y1_1, y2_1, ..., y1_S, y2_S], D = 2S + 2 doubles.  The output frame is (float) of the last
 *             stage's y, rounded once; a NaN is stored as 0x7FC00000 (wbx_clip_derive's rule)
 *   chunks    the frames are cut into chunks of C = 512 (wbx_filter_chunk_frames).  For every chunk j but the last, z_j is the
 *             state after running chunk j's frames from REST (v = 0).  The carry matrix M (wbx_filter_transition, D x D,
 *             row-major M[i][k]) has as column k the state after C frames of zero input from the unit state e_k, run by the
 *             same step in fp64 on the host.  t_0 = 0 and t_{j+1}[i] = z_j[i] + acc_i, where acc_i starts at 0.0 and does
 *             acc_i = acc_i + M[i][k]*t_j[k] for k = 0 .. D-1 ascending, single operations.  The STORED output of chunk j is
 *             the run of its frames from state t_j
 * Hence chunk 0 — and any result of at most 512 frames — IS the one sequential pass; later chunks equal it up to the
 * rounding of the carry: direct form I with poles near z = 1 is ill-conditioned, M*t cancels against z, and M's own rounding
 * acts as a small systematic coefficient error.  Measured against a wider sequential pass the deviation
 * stays below one fp32 ulp of the output's peak up to 384 kHz — it is no 1e-15.  The chunked definition is the
 * specification, not an approximation of one: chunks are independent but for D doubles, which is what lets a lane own one.
 * wbx_filter_design / _check / _transition / _chunk_frames are host-only and need no device (wbx_filter_transition:
 * WBX_ERR_INVALID for NULL M, cap_doubles below D*D, or a cascade wbx_filter_check refuses; M untouched then).
 * wbx_clip_filter: dst_clip becomes a new F32 pool clip of n_frames + tail_frames frames (plus the pool's 16 zero frames
 * of padding) at the source's rate and channel count, replaced or allocated as wbx_clip_derive does it, on the same stream
 * and behind the same ordering; one edit, conversion or filter runs at a time.  stats_of_result (may be NULL):
 * wbx_clip_measure of the whole result, a second pass over the output only.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: unknown source clip,
 * n_frames == 0, a range past the clip, dst_clip == src_clip, NULL coef, a cascade wbx_filter_check refuses,
 * n_frames + tail_frames >= 2^31 - 16; WBX_ERR_UNSUPPORTED: a source whose storage format is not F32 or with more than 2
 * channels.  WBX_ERR_OOM as for wbx_clip_derive.
 * wbx_filter_phase_ms: device milliseconds of the three launches of the context's last completed filter (layer 1's or layer
 * 2's), between events on the edits' stream — out[0] the zero-state runs, out[1] the carry, out[2] the runs from the carried
 * states; the first two are 0 for a result of one chunk.  WBX_ERR_INVALID for NULL arguments or when no filter has
 * completed.  For tools/bench_filter.py; nothing else reads it.
 * Not offered: zero-phase filtering (filter, derive reversed, filter, derive reversed does it), filters at render time,
 * FIR by FFT (direct convolution: "Convolving a clip" below), more than 8 stages or 2 channels, in-place edits. */
enum { WBX_FILT_LOWPASS = 0, WBX_FILT_HIGHPASS = 1, WBX_FILT_BANDPASS = 2, WBX_FILT_NOTCH = 3, WBX_FILT_ALLPASS = 4,
       WBX_FILT_PEAK = 5, WBX_FILT_LOWSHELF = 6, WBX_FILT_HIGHSHELF = 7 };
wbx_status wbx_filter_design(uint32_t rate, int kind, double freq_hz, double q, double gain, double out[5]);
wbx_status wbx_filter_check(const double* coef, uint32_t n_stages);
wbx_status wbx_filter_transition(const double* coef, uint32_t n_stages, double* M, size_t cap_doubles);
uint32_t wbx_filter_chunk_frames(void);
wbx_status wbx_filter_phase_ms(wbx_ctx* ctx, double out[3]);
wbx_status wbx_clip_filter(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                           uint64_t tail_frames, const double* coef /* [n_stages][5] */, uint32_t n_stages,
                           wbx_clip_stats* stats_of_result);

/* Convolving a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels convolved with
 * frames [ir_first, ir_first + ir_frames) of another resident F32 clip, the impulse response of L = ir_frames taps, into a
 * NEW F32 clip, without the samples leaving HBM: a recorded room, plate or cabinet put on a frozen stem, a linear-phase
 * low-pass or band-stop baked into a bounce, a measured response used as a match EQ.  Direct convolution in fp64; no
 * reference counterpart.  This text is the specification; tests/convolve_model.py restates it in numpy, and the designed
 * taps and every output frame equal that BIT FOR BIT.
 *   input     x[c][i], i in [0, n_frames): (double) of the source range's fp32 sample; h[c][k], k in [0, L): (double) of the
 *             response range's fp32 sample.  A value that is not finite (NaN, +-inf) enters as 0.0 — the filter's rule,
 *             applied to both.  x is ZERO outside [0, n_frames), whatever the clip holds beside the range.  Nothing beside
 *             either range counts or is ever read: the response may be longer than the pool's 16 padding frames, and a range
 *             may start at frame 0 of a slab
 *   output    the full result has n_frames + L - 1 frames (wbx_convolve_frames); stored frame j, j in [0, out_frames), is
 *             full-result frame m = out_first + j:
 *               acc = 0.0;  for k = 0 .. L-1 ascending: acc = acc + h[k] * x[m - k]     (fp64, one IEEE operation each)
 *               y = (float)(gain * acc)                       (one multiplication, one rounding)
 *             a NaN is stored as 0x7FC00000 (wbx_clip_derive's rule); it can arise only from gain = 0 times an overflow,
 *             which no input can cause (|acc| <= 2^20 * 2^128 * 2^128).  The product of two fp32 values is exact in fp64,
 *             so fma(h, x, acc) IS acc + h * x and only the order of the additions is fixed.  A tap whose x[m - k] lies
 *             outside the range may be skipped or computed with a zero: acc starts at +0.0 and can never become -0.0
 *             (a sum of +0.0 and +-0.0 is +0.0, an exact cancellation rounds to +0.0), and adding h * 0 = +-0 to it never
 *             changes it.  The same holds for a tap that entered as 0.0
 *   window    out_first lets a linear-phase FIR's delay (L - 1) / 2 be dropped; out_first = 0 with out_frames = n_frames
 *             gives a result as long as the range; out_frames = n_frames + L - 1 gives the whole ring-out
 *   channels  the result has max(source channels, response channels) channels and the source's rate.  A mono response goes
 *             to every source channel, a stereo response on a stereo source works channel by channel, a stereo response on a
 *             mono source gives a stereo result (source * left, source * right)
 * The response may be the source itself (an autocorrelation's cousin).  dst_clip becomes a new F32 pool clip of out_frames
 * frames (plus the pool's 16 zero frames of padding), replaced or allocated as wbx_clip_derive does it, on the same stream
 * and behind the same ordering; one edit, conversion, filter or convolution runs at a time.  The work is issued as several
 * bounded launches.  stats_of_result (may be NULL): wbx_clip_measure of the whole result, a second pass over
 * the output only.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: an unknown source or response
 * clip, n_frames, ir_frames or out_frames of 0, a range past its clip, out_first + out_frames > n_frames + ir_frames - 1,
 * dst_clip equal to the source or the response, a gain that is not finite, out_frames >= 2^31 - 16, sample rates that
 * differ (convert first: wbx_clip_resample); WBX_ERR_UNSUPPORTED: either clip not F32 or with more than 2 channels,
 * ir_frames > 2^20 (21.8 s at 48 kHz), out_frames * ir_frames * channels > 2^46 multiply-adds (channels: the result's).
 * The sizes are judged before the clips are looked at.  WBX_ERR_OOM as for wbx_clip_derive.
 * The work cap is a stated limit of the interface — one hour of stereo at 48 kHz with a 4 s response, 6.6e13, lies under it;
 * DESIGN.md 7i says how long a call at the cap takes.  The way past it: convolve ranges of the source (each with its
 * ring-out) and overlap-add them with wbx_clip_splice, whose parts are added in list order — a sum of rounded fp32 parts,
 * NOT bit-equal to one call.
 * Host-only, no device: wbx_convolve_frames — the full result's length n_frames + ir_frames - 1, or 0 for a pair no window
 * of which is accepted (either 0, ir_frames > 2^20, a sum past 64 bits); wbx_convolve_tile_frames (2048, the output frames
 * one workgroup owns) and wbx_convolve_segment_taps (2048, the taps walked per staging) — the kernel's two shape constants.
 * wbx_fir_design (host-only; wbx_convolve.h, which a C++ compiler takes alone): n_taps of a Kaiser-windowed sinc, linear
 * phase, in fp64 through "Converting a clip's sample rate"'s sinpi, sinc and I0 — no libm; every operator below is one
 * IEEE operation in the order written.  n_taps odd, 3 .. 65535;  c = (n_taps - 1) / 2;  for k = 0 .. n_taps - 1:
 *               d = (double)(k - c);  u = d / c;  a = max(0, 1 - u*u);  w[k] = I0(beta * sqrt(a)) / I0(beta)
 *               lp_f[k] = ((t * sinc(t * d)) * w[k]) / S_f   with t = (2*f) / rate and S_f = the sum over k ascending of
 *                         (t * sinc(t * d)) * w[k], started at 0.0
 *               LOWPASS = lp_f1;  HIGHPASS = delta - lp_f1;  BANDPASS = lp_f2 - lp_f1;  BANDSTOP = delta - (lp_f2 - lp_f1)
 *             delta is 1.0 at tap c and 0.0 elsewhere; out[k] is the value rounded once to fp32.  f2_hz is not looked at
 *             by LOWPASS and HIGHPASS.  The taps are symmetric, out[k] == out[n_taps - 1 - k]; played with
 *             out_first = c the result carries no delay.  WBX_ERR_INVALID: NULL out, cap_floats below n_taps, an unknown
 *             kind, rate == 0, n_taps even or out of range, an edge not inside (0, rate / 2), f2 <= f1 for the band kinds,
 *             a beta that is not finite or outside [0, 14].  The taps become a response through wbx_clip_upload (one
 *             channel, F32): there is no other upload path.
 * wbx_convolve_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed convolution (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_convolve.py; nothing else reads it.
 * Not offered: FFT or partitioned convolution (not reproducible bit for bit), convolution at render time, more than 2
 * channels, "true stereo" matrices of four responses, responses longer than 2^20 frames. */
enum { WBX_FIR_LOWPASS = 0, WBX_FIR_HIGHPASS = 1, WBX_FIR_BANDPASS = 2, WBX_FIR_BANDSTOP = 3 };
wbx_status wbx_fir_design(uint32_t rate, int kind, double f1_hz, double f2_hz, uint32_t n_taps, double beta, float* out,
                          size_t cap_floats);
uint64_t wbx_convolve_frames(uint64_t n_frames, uint64_t ir_frames);
uint32_t wbx_convolve_tile_frames(void);
uint32_t wbx_convolve_segment_taps(void);
wbx_status wbx_convolve_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_convolve(wbx_ctx* ctx, uint32_t src_clip, uint32_t ir_clip, uint32_t dst_clip, uint64_t first_frame,
                             uint64_t n_frames, uint64_t ir_first, uint64_t ir_frames, uint64_t out_first,
                             uint64_t out_frames, double gain, wbx_clip_stats* stats_of_result);

/* Limiting a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels through a
 * look-ahead peak limiter into a NEW F32 clip of n_frames frames, without the samples leaving HBM: the last step of a
 * mastering chain, which lets a clip reach a loudness target under a ceiling without being turned down as a whole for a few
 * tall peaks.  Purely feed-forward: the gain curve is a sliding minimum, a slope-limited release written in closed form as
 * a (min, +) convolution, and a moving average.  No reference counterpart.  This text is the specification;
 * tests/limit_model.py restates it in numpy, and the ramp table, the statistics and every output frame equal that BIT FOR
 * BIT.  n = n_frames, A = lookahead_frames (0 .. 4096), H = hold_frames (0 .. 65536), R = release_frames (1 .. 2^20);
 * ceiling is linear, a float, finite and >= FLT_MIN; drive is a linear pre-gain, finite with 0 < |drive| <= 2^32.  Every
 * operator below is one IEEE fp64 operation and nothing is fused.
 *   input     d[c][i] = drive * (double)x[c][i], i in [0, n).  A sample that is not finite enters as 0.0 (the filter's
 *             rule).  Nothing beside the range counts or is ever read
 *   detector  (channels linked) p[i] = the maximum over the channels of |d[c][i]|;  need[i] = p[i] > c ? c / p[i] : 1.0
 *             with c = (double)ceiling.  need is 1.0 for every i outside [0, n)
 *   ramp      s = 1.0 / (double)R;  for k = -A .. H + R - 1: ramp[k] = 0.0 when k <= H, else (double)(k - H) * s.  The
 *             host builds it as a table of A + H + R doubles, table[k + A] (wbx_limit_ramp): no fma(k, s, ..) can arise
 *   curve     for j = -A .. n - 1: y[j] = 1.0, then y[j] = min(y[j], need[j - k] + ramp[k]) for every k.  Every value is
 *             finite and positive, so the minimum is the same in any order and grouping; a run of terms whose need values
 *             are all 1.0 contributes nothing below 1.0 and may be skipped.  This is look-ahead A, then hold H, then a
 *             release that rises linearly in gain by 1 / R per frame — in exact arithmetic y[j] = min(m[j], y[j-1] + s)
 *             with m the sliding minimum — written so that no frame depends on another
 *   gain      acc = 0.0;  for j = i - A .. i ascending: acc = acc + y[j];  g[i] = min(acc / (double)(A + 1), need[i]).
 *             Every y[j] of that window has need[i] inside its own look-ahead, so the average reaches need[i] at a peak
 *             and ramps down to it over A frames; the final min makes the guarantee immune to the rounding of the sum
 *   output    out[c][i] = (float)(d[c][i] * g[i]), rounded once; a NaN is stored as 0x7FC00000 (none can arise).  The
 *             result has n frames, the source's channels and rate and NO delay.  GUARANTEE: |out[c][i]| <= ceiling for
 *             every sample.  Where g[i] == 1.0, out is (float)d: with drive == 1.0 a clip that never exceeds the ceiling
 *             comes back bit for bit
 *   wbx_limit_stats (may be NULL; every field independent of order): peak_in = the maximum of p; min_gain and
 *             min_gain_frame = the smallest g and the first frame that has it (1.0 and 0 where nothing was limited);
 *             limited_frames = the count of g[i] < 1.0
 * dst_clip becomes a new F32 pool clip of n frames (plus the pool's 16 zero frames of padding), replaced or allocated as
 * wbx_clip_derive does it, on the same stream and behind the same ordering; one edit, conversion, filter, convolution or
 * limit runs at a time.  The curve lives in a stage of (2^20 + A) doubles whatever the clip's length: the call is issued
 * in bands of 2^20 output frames, each recomputing its A frames of halo.  stats_of_result (may be NULL):
 * wbx_clip_measure of the whole result, a second pass over the output only.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: an unknown source clip,
 * n_frames of 0, a range past the clip, dst_clip equal to the source, a ceiling, drive, lookahead_frames, hold_frames or
 * release_frames outside the ranges above, n_frames >= 2^31 - 16; WBX_ERR_UNSUPPORTED: a source that is not F32 or has
 * more than 2 channels, n_frames * (A + H + R) > 2^44 terms (a stated cap of the interface, not a measurement; one hour
 * of 48 kHz with 100 ms of release lies under it).  The sizes are judged before the clip is looked at.  WBX_ERR_OOM as for
 * wbx_clip_derive.
 * Host-only, no device (wbx_limit.h, which a C++ compiler takes alone): wbx_limit_ramp writes the A + H + R doubles of the
 * table (WBX_ERR_INVALID: NULL out, A, H or R out of range, cap_doubles below A + H + R); wbx_limit_tile_frames (2048, the
 * frames one workgroup owns), wbx_limit_segment_terms (2048, the ramp terms walked per staging) and
 * wbx_limit_band_frames (2^20) — the kernels' shape constants.
 * wbx_limit_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed limit (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_limit.py; nothing else reads it.
 * Not offered: a detector on the oversampled signal (a true-peak limiter; wbx_clip_loudness reports the result's true
 * peak), unlinked stereo, the gain curve as a clip of its own, limiting at render time or on the master bus, more than 2
 * channels, in-place edits.  Compressors, expanders, gates and ducking are "Dynamics of a clip" below: their curve in dB is
 * a table the host builds, so the device needs no log and no pow. */
typedef struct wbx_limit_stats {
  double peak_in;
  double min_gain;
  uint64_t min_gain_frame;
  uint64_t limited_frames;
} wbx_limit_stats;
wbx_status wbx_limit_ramp(uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames, double* out,
                          size_t cap_doubles);
uint32_t wbx_limit_tile_frames(void);
uint32_t wbx_limit_segment_terms(void);
uint32_t wbx_limit_band_frames(void);
wbx_status wbx_limit_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_limit(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                          float ceiling, double drive, uint32_t lookahead_frames, uint32_t hold_frames,
                          uint32_t release_frames, wbx_limit_stats* limit_stats, wbx_clip_stats* stats_of_result);

/* Dynamics of a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels through a
 * table-driven dynamics processor into a NEW F32 clip of n_frames frames, the source's channels and rate and NO delay,
 * without the samples leaving HBM: a compressor of any ratio and knee, a downward expander or gate, ducking from a
 * sidechain, or any hand-drawn transfer curve, between the EQ and the limiter of a mastering chain.  The gain follows the
 * level of the clip itself, or of a second resident clip (the key), through a transfer table the HOST builds — a gain per
 * level, so the device needs no log and no pow: it looks the table up and interpolates — and through the limiter's purely
 * feed-forward look-ahead / hold / release curve, so no frame depends on another.  No reference counterpart.  This text is
 * the specification; tests/dynamics_model.py restates it in numpy, and the table, the statistics and every output frame
 * equal that BIT FOR BIT.  n = n_frames, A = lookahead_frames (0 .. 4096), H = hold_frames (0 .. 65536), R = release_frames
 * (1 .. 2^20): "Limiting a clip"'s ranges and its wbx_limit_ramp table, unchanged.  sense is WBX_DYN_COMPRESS or
 * WBX_DYN_GATE.  drive and key_gain are linear, finite with 0 < |.| <= 2^32 (key_gain is not looked at without a key);
 * makeup is linear, finite and >= 0.  Every operator below is one IEEE fp64 operation and nothing is fused.
 *   input     d[c][i] = drive * (double)x[c][i], i in [0, n).  A sample that is not finite enters as 0.0.  Nothing beside
 *             the range counts or is ever read
 *   level     without a key (key_clip == WBX_DYN_NO_KEY): p[i] = the maximum over the channels of |d[c][i]|.  With a key:
 *             p[i] = the maximum over the KEY's channels of |key_gain * (double)key[c][key_first + i]|, what is not finite
 *             entering as 0.0.  The key has 1 or 2 channels of its own, whatever the source has, and the source's rate
 *   table     WBX_DYN_TABLE = 48 * 64 + 1 = 3073 doubles over the levels 2^-40 .. 2^8, 64 cells per octave, linear in the
 *             mantissa: entry (e + 40) * 64 + k belongs to the level 2^e * (1 + k / 64).  Every entry is finite, its sign
 *             bit clear, and <= 1.0 (wbx_dynamics_check).  lo = the smallest entry
 *   lookup    want = tab(p):  p < 2^-40 (0 included): tab[0];  p >= 2^8: tab[3072];  otherwise, with e the unbiased
 *             exponent and m the 52 mantissa bits of p:  idx = (e + 40) * 64 + (m >> 46);
 *             f = (double)(m & (2^46 - 1)) * 2^-46 (exact);  want = tab[idx] + f * (tab[idx + 1] - tab[idx]).
 *             want lies between its two entries (f <= 1 - 2^-46, and two roundings cannot carry the sum past
 *             tab[idx + 1]), so want is in [lo, 1.0]
 *   rest      the gain of a level that asks for nothing: 1.0 in the compress sense, lo in the gate sense.  want is rest for
 *             every frame outside [0, n)
 *   curve     for j = -A .. n - 1, with ramp[k], k = -A .. H + R - 1, the limiter's (0.0 when k <= H, else (k - H) * (1 / R)):
 *             compress: y[j] = 1.0, then y[j] = min(y[j], want[j - k] + ramp[k]) for every k — the limiter's curve with want
 *             in place of need: the gain falls A frames ahead of a loud passage, is held H frames and recovers by 1 / R per
 *             frame.  gate: y[j] = lo, then y[j] = max(y[j], want[j - k] - ramp[k]) for every k — the mirror image: the gate
 *             opens A frames before the signal arrives, is held H frames and closes by 1 / R per frame.  No -0.0 can arise
 *             (the entries carry no sign, x - x is +0.0), so minimum and maximum are the same in any order and grouping; a
 *             run of terms whose want values all equal rest changes nothing and may be skipped
 *   gain      acc = 0.0;  for j = i - A .. i ascending: acc = acc + y[j];  g[i] = acc / (double)(A + 1).  No final minimum:
 *             there is no guarantee to keep here, that is the limiter's job.  g <= 1.0 (a sum of A + 1 values <= 1.0 cannot
 *             round above A + 1); g may round below lo by a few units in the last place
 *   output    out[c][i] = (float)((d[c][i] * g[i]) * makeup), rounded once to fp32; a NaN is stored as 0x7FC00000
 *   wbx_dynamics_stats (may be NULL; every field independent of order): min_gain and min_gain_frame = the smallest g and
 *             the first frame that has it; reduced_frames = the count of g[i] < 1.0
 * dst_clip becomes a new F32 pool clip of n frames (plus the pool's 16 zero frames of padding), replaced or allocated as
 * wbx_clip_derive does it, on the same stream and behind the same ordering; one edit, conversion, filter, convolution,
 * limit or dynamics call runs at a time.  The call is issued in the limiter's bands of 2^20 output frames over the
 * limiter's stage.  stats_of_result (may be NULL): wbx_clip_measure of the whole result, a second pass over
 * the output only.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: an unknown source or key clip,
 * n_frames of 0, a range past either clip, dst_clip equal to the source or the key, a NULL table or one wbx_dynamics_check
 * refuses, an unknown sense, a drive, key_gain, makeup, lookahead_frames, hold_frames or release_frames outside the ranges
 * above, n_frames >= 2^31 - 16, a key whose sample rate differs from the source's; WBX_ERR_UNSUPPORTED: a source or key
 * that is not F32 or has more than 2 channels, n_frames * (A + H + R) > 2^44 terms (the limiter's stated cap).  The sizes
 * are judged before the clips are looked at.  WBX_ERR_OOM as for wbx_clip_derive.
 * Host-only, no device (wbx_dynamics.h, which a C++ compiler takes alone):
 * wbx_dynamics_table writes the 3073 entries of the usual static curve.  kind WBX_DYN_COMPRESS: above the threshold the
 *             gain in dB is (1 / ratio - 1) * (L - T), L the level and T the threshold in dB; kind WBX_DYN_GATE (a downward
 *             expander; a gate is one of high ratio): below the threshold it is (ratio - 1) * (L - T).  ratio >= 1, +inf
 *             allowed for the compressor only.  knee_db (0 .. 1000) blends quadratically over [T - knee / 2, T + knee / 2]:
 *             (1 / ratio - 1) * (L - T + knee / 2)^2 / (2 knee), the expander -(ratio - 1) * (L - T - knee / 2)^2 / (2 knee).
 *             The gain is never below range_db (<= 0; -inf: no floor, and an entry below 2^-1021 is 0.0).  |T| <= 1000.
 *             On the side of the knee where the curve asks for nothing the entry is EXACTLY 1.0, by a branch.  Computed in
 *             octaves (a dB figure divided by 20 log10(2) = 6.020599913279624) with a log2 and an exp2 made of + - * /
 *             and floor in a fixed number of steps — no libm, so the table is the same on every host.  WBX_ERR_INVALID:
 *             NULL out, cap_doubles below WBX_DYN_TABLE, an unknown kind, a parameter outside the ranges above or a NaN;
 *             nothing is written then
 * wbx_dynamics_check judges any table, designed or hand-drawn (WBX_ERR_INVALID: NULL, an unknown sense, an entry that is
 *             not finite, carries a sign bit or exceeds 1.0); lo (may be NULL) receives the smallest entry
 * wbx_dynamics_lookup the lookup above for one level (WBX_ERR_INVALID: NULL table or out, a level that is negative or a NaN).
 * wbx_dynamics_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed dynamics call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_dynamics.py; nothing else reads it.
 * Not offered: an RMS or true-peak detector, unlinked stereo, upward compression (entries above 1.0), multiband, a release
 * that is exponential in dB, the gain curve as a clip of its own, dynamics at render time or on buses, more than 2
 * channels, in-place edits. */
enum { WBX_DYN_COMPRESS = 0, WBX_DYN_GATE = 1 };
#define WBX_DYN_TABLE 3073
#define WBX_DYN_NO_KEY 0xFFFFFFFFu
typedef struct wbx_dynamics_stats {
  double min_gain;
  uint64_t min_gain_frame;
  uint64_t reduced_frames;
} wbx_dynamics_stats;
wbx_status wbx_dynamics_table(int kind, double threshold_db, double ratio, double knee_db, double range_db, double* out,
                              size_t cap_doubles);
wbx_status wbx_dynamics_check(const double* table, int sense, double* lo);
wbx_status wbx_dynamics_lookup(const double* table, double level, double* out);
wbx_status wbx_dynamics_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_dynamics(wbx_ctx* ctx, uint32_t src_clip, uint32_t key_clip /* WBX_DYN_NO_KEY: the source keys itself */,
                             uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames, uint64_t key_first, int sense,
                             const double* table /* [WBX_DYN_TABLE] */, double drive, double key_gain, double makeup,
                             uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames,
                             wbx_dynamics_stats* dynamics_stats, wbx_clip_stats* stats_of_result);

/* Saturating a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels through an
 * OVERSAMPLED table waveshaper into a NEW F32 clip of n_frames frames, the source's channels and rate and NO delay, without
 * the samples leaving HBM: a soft clipper, tape or tube style saturation, or any hand-drawn transfer curve applied to the
 * samples themselves, between the compressor and the limiter of a mastering chain.  The limiter and the dynamics only
 * multiply by a gain curve; this is the memoryless non-linearity, which adds harmonics.  At the clip's own rate a
 * waveshaper aliases, so the call converts up by os, shapes, and band-limits back, as ONE call whose intermediate is never
 * stored.  The curve is a table the HOST builds, so the device needs no tanh and no exp.  No reference counterpart.  This
 * text is the specification; tests/saturate_model.py restates it in numpy (the two conversions are
 * tests/resample_model.py's), and the table, the statistics and every output sample equal that BIT FOR BIT.
 * n = n_frames; os is 1, 2, 4 or 8; quality is WBX_SRC_FAST / GOOD / BEST with its Z zero crossings (12 / 24 / 48); drive
 * is linear, finite with 0 < |drive| <= 2^32; makeup is linear, finite with |makeup| <= 2^32 (0 is allowed); the table has
 * WBX_SAT_TABLE = 16385 doubles, every entry finite with a magnitude <= 2^32 (wbx_saturate_check).  Every operator below is
 * one IEEE fp64 operation and nothing is fused, except that the product of two fp32 values added into an fp64 accumulator
 * may be an fma: that product is exact, as in "Converting a clip's sample rate".
 *   up        (only when os > 1) that section's conversion with L = os, M = 1 at `quality`, unchanged: its table
 *             wbx_resample_table(1, os, quality), H = Z, T = 2 Z.  Mid sample j in [0, n os): i = j div os, p = j mod os,
 *             u[c][j] = (float)(sum over k of h_up[p][k] * x[c][i - (Z - 1) + k]), k ascending from acc = 0.0.  x is ZERO
 *             outside the range whatever the clip holds there, and nothing beside the range is ever read.  A NaN is
 *             stored as 0x7FC00000.  With os == 1, u = x
 *   shape     d = finite(u) ? drive * (double)u : 0.0;  a = d * 1024.0;  a <= -8192: w = tab[0];  a >= 8192: w = tab[16384];
 *             otherwise fl = floor(a), idx = (int)fl + 8192 (0 .. 16383), f = a - fl (ONE subtraction: it may round to
 *             1.0 for a tiny negative a), w = tab[idx] + f * (tab[idx + 1] - tab[idx]).  Entry k belongs to the level
 *             (k - 8192) / 1024: +-8 full scales, 1024 cells per unit.  s[c][j] = (float)(w * makeup)
 *   down      (only when os > 1) that section's conversion with L = 1, M = os at `quality`, unchanged: one phase,
 *             H = Z os, T = 2 Z os.  y[c][i] = (float)(sum over k of h_dn[k] * s[c][i os - (H - 1) + k]), ascending.  s is
 *             ZERO outside [0, n os) — NOT shape(0): the intermediate counts as a whole file, as it does there.  With
 *             os == 1, y = s
 * BY DEFINITION the call with os > 1 is these three existing calls in a row: wbx_clip_resample to rate * os, this call with
 * os = 1, wbx_clip_resample back to rate; every output bit equals that composition.  No NaN and no infinity can appear in
 * the result: what is not finite enters the shape as 0.0; |f| <= 1 and the entries are at most 2^32, so |w| <= 3 * 2^32 and
 * |w * makeup| < 2^66, which an fp32 holds — s is always finite; the down filter has at most 768 coefficients, each below 2 in
 * magnitude, so its sum stays below 2^77, which an fp32 holds as well.
 * NO CEILING GUARANTEE: the band-limiting overshoots.  A hard table at drive 8 over a half-scale sine gives a peak of 1.156
 * at os = 4.  Where a ceiling must hold, follow the call with wbx_clip_limit.
 *   wbx_saturate_stats (may be NULL; every field independent of order): peak_drive = the greatest |d| over all channels and
 *             mid samples j in [0, n os); peak_index = the lowest such j; beyond = the count over channels and j of
 *             |a| >= 8192.  Every mid sample counts once.
 * dst_clip becomes a new F32 pool clip of n frames (plus the pool's 16 zero frames of padding), replaced or allocated as
 * wbx_clip_derive does it, on the same stream and behind the same ordering; one edit, conversion, filter, convolution,
 * limit, dynamics or saturate call runs at a time.  Nothing else is allocated in the pool: the oversampled intermediate
 * lives in the workgroups' LDS.  stats_of_result (may be NULL): wbx_clip_measure of the whole result, a
 * second pass over the output only.
 * Refused before any device call, nothing allocated, dst_clip and stats untouched, in this order.  First the sizes and
 * parameters, before the clips are looked at — WBX_ERR_INVALID: n_frames of 0; an os that is not 1, 2, 4 or 8; an unknown
 * quality; a NULL table or one wbx_saturate_check refuses; a drive, then a makeup outside the ranges above; n_frames * os
 * >= 2^31 - 16.  Then what wbx_resample_plan(1, os, quality) or (os, 1, quality) refuses, with its status and reason:
 * WBX_SRC_BEST at os = 8 has T = 768 > 512 and is WBX_ERR_UNSUPPORTED.  Then the clip — WBX_ERR_INVALID: an unknown source
 * clip; a range past the clip; dst_clip equal to the source; WBX_ERR_UNSUPPORTED: a source that is not F32 or has more than
 * 2 channels; last, wbx_clip_derive's rule: WBX_ERR_INVALID for a dst_clip of 2^24 or more.  WBX_ERR_OOM as for
 * wbx_clip_derive.
 * Host-only, no device (wbx_saturate.h, which a C++ compiler takes alone):
 * wbx_saturate_table writes the 16385 entries of a usual curve: entry k = f(v + bias) - f(bias) with v = ((double)k -
 *             8192.0) / 1024.0 and |bias| <= 4 (a bias gives even harmonics).  WBX_SAT_HARD: f(z) = z clamped to +-1.
 *             WBX_SAT_CUBIC: +-1 where |z| >= 1.5, else z - (c z) (z z) with c = 4.0 / 27.0.  WBX_SAT_TANH: a = |z|,
 *             e = exp2((-2.0 a) * 1.4426950408889634) — wbx_dynamics_table's exp2, whose argument is <= 0 —,
 *             t = (1.0 - e) / (1.0 + e), with the sign of z.  No libm, so the table is the same on every host.  With
 *             bias == 0 the table is exactly odd and entry 8192 is exactly 0.0.  WBX_ERR_INVALID: NULL out, cap_doubles
 *             below WBX_SAT_TABLE, an unknown kind, a bias outside the range or a NaN; nothing is written then
 * wbx_saturate_check judges any table, designed or hand-drawn (WBX_ERR_INVALID: NULL, an entry that is not finite or whose
 *             magnitude exceeds 2^32)
 * wbx_saturate_lookup the lookup above for one driven sample d (WBX_ERR_INVALID: NULL table or out, a NaN)
 * wbx_saturate_launch_shape how a call is launched: the tile (output frames of one workgroup: a multiple of 256, at most
 *             1024, the greatest whose LDS stays within 64 KB), the mid samples (tile + 2 Z) os and the source frames
 *             tile + 4 Z - 1 a tile computes and stages per channel, the LDS bytes channels * 4 * ((tile + 2 Z) os + tile +
 *             4 Z), and the tiles = the grid, ceil(n / tile) <= 2^21.  os == 1: tile 1024, both spans 1024, no LDS.
 *             Refused as the call refuses os, quality and n_frames; WBX_ERR_INVALID for channels other than 1 or 2 or a
 *             NULL pointer
 * wbx_saturate_ms: device milliseconds between two events on the edits' stream around the table's upload (and the filters',
 * where os or the quality changed) and the two launches of the context's last completed saturate call (layer 1's or layer
 * 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_saturate.py; nothing else reads it.
 * Not offered: waveshaping at render time or on buses, a true-peak-safe clipper (no ceiling guarantee, see above),
 * oversampling above 8, unlinked per-channel tables, more than 2 channels, in-place edits. */
enum { WBX_SAT_HARD = 0, WBX_SAT_CUBIC = 1, WBX_SAT_TANH = 2 };
#define WBX_SAT_TABLE 16385
typedef struct wbx_saturate_stats { /* 24 bytes */
  double peak_drive;
  uint64_t peak_index;
  uint64_t beyond;
} wbx_saturate_stats;
wbx_status wbx_saturate_table(int kind, double bias, double* out, size_t cap_doubles);
wbx_status wbx_saturate_check(const double* table);
wbx_status wbx_saturate_lookup(const double* table, double d, double* out);
wbx_status wbx_saturate_launch_shape(uint32_t os, int quality, uint32_t channels, uint64_t n_frames, uint32_t* tile,
                                     uint32_t* mid_span, uint32_t* src_span, uint32_t* lds_bytes, uint32_t* n_tiles);
wbx_status wbx_saturate_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_saturate(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                             uint32_t os, int quality, const double* table /* [WBX_SAT_TABLE] */, double drive,
                             double makeup, wbx_saturate_stats* saturate_stats, wbx_clip_stats* stats_of_result);

/* Reducing a clip's noise: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels through
 * a SPECTRAL GATE into a NEW F32 clip of n_frames frames, the source's channels and rate and NO delay, without the samples
 * leaving HBM: hiss, hum or room tone of a recorded take pushed down by `floor` wherever a cell's smoothed power does not
 * rise above a per-bin threshold, which wbx_clip_denoise_profile measures on a stretch of the noise alone.  The forward
 * and the inverse transform are DIRECT — ascending fp64 chains of exact fp32 products against host-built tables — so the
 * device needs no FFT, no sin and no log and every bit is reproducible.  No reference counterpart.  This text is the
 * specification; tests/denoise_model.py restates it in numpy, and the tables, the threshold, the profile's sums, the
 * statistics and every output sample equal that BIT FOR BIT.  Every operator below is ONE IEEE fp64 operation in the order
 * written and nothing is fused, except that the product of two fp32 values added into an fp64 chain may be an fma: that
 * product is exact.
 * W = window_frames, a power of two in 64 .. 2048; H = W / 4; B = W / 2 + 1; n = n_frames in [1, 2^31 - 16); S =
 * smooth_hops in 0 .. 4; F = smooth_bins in 0 .. 8.  Channels are processed independently.  x[c][f] is the range's frame f of
 * channel c as fp64, what is not finite as 0.0, and 0.0 for f < 0 or f >= n whatever the clip holds there: nothing beside
 * the range is ever read.  T = ceil(n / H) + 3 hops; hop t starts at range frame (t - 3) H, d_t[j] = x[(t - 3) H + j], so
 * every output frame lies under exactly four windows.
 *   tables    (wbx_denoise_tables, host-only, no libm: sinpi is wbx_resample_table's, exact at integers)  s[j] =
 *             sinpi(((double)j + 0.5) / (double)W) — the square root of a Hann window; its squares over the four
 *             overlapping windows add up to 2.  m = (k j) mod W in integers, t = (double)m / (double)W, c = sinpi(2.0 t +
 *             0.5), z = sinpi(2.0 t).  Analysis, [B][W]: AC[k][j] = (float)((s[j] c) / (double)W), AS[k][j] = (float)(0.0 -
 *             ((s[j] z) / (double)W)).  Synthesis, e_k = 0.5 for k = 0 and k = B - 1, else 1.0 (the Hermitian doubling and
 *             the overlap's 1/2 folded in): YC[k][j] = (float)(e_k (s[j] c)), YS[k][j] = (float)(0.0 - (e_k (s[j] z))).
 *             Rows 0 and B - 1 of AS and YS are all +0.0.  The 1 / W sits in the ANALYSIS table, so |re|, |im| <= 0.64
 *             max|x|: a cell always fits an fp32
 *   analysis  per hop, channel and bin from re = im = 0.0, j = 0 .. W - 1 ascending: re = re + d[j] AC[k][j], im = im +
 *             d[j] AS[k][j]; the cell r = (float)re, i = (float)im; its power p = ((double)r (double)r) + ((double)i
 *             (double)i) — two exact products, one rounded sum, from the STORED fp32 cell
 *   gate      q = the sum from 0.0 of p[t'][k'] over t' = t - S .. t + S (outer, ascending) and k' = k - F .. k + F (inner,
 *             ascending), cells with t' outside [0, T) or k' outside [0, B) left out, then divided by (double)count of the
 *             cells that were present.  With th = thr[c B + k]: if q > th, v = 1.0 - (th / q) and g = v > floor ? v : floor;
 *             otherwise g = floor.  The masked cell mr = (float)(g (double)r), mi = (float)(g (double)i)
 *   synthesis per hop, channel and window position j from a = 0.0, k = 0 .. B - 1 ascending: a = a + mr[k] YC[k][j], then
 *             a = a + mi[k] YS[k][j]
 *   add       output frame f (0 <= f < n) lies in hops t0 = f div H .. t0 + 3, in hop t0 + u at position f - (t0 + u - 3) H:
 *             out[c][f] = (float)(((a_0 + a_1) + a_2) + a_3), the chain values as fp64, not rounded on the way.  That last
 *             rounding may give +-inf only where the sum itself reaches 2^128; no NaN is ever produced
 *   wbx_denoise_stats (may be NULL; every field an integer independent of order): hops = T; cells = T B channels;
 *             open_cells = the count over hops, channels and bins of q > th; bands = how many bands the call ran in
 * thr has channels x B entries, finite and >= 0 (0: always open — with floor anything the call then returns the source
 * within 1e-7 of its peak; 1e30: all floor); floor is in [0, 1].
 * dst_clip becomes a new F32 pool clip of n frames (plus the pool's 16 zero frames of padding), replaced or allocated as
 * wbx_clip_derive does it, on the same stream and behind the same ordering; one edit, conversion, filter, convolution,
 * limit, dynamics, saturate or denoise call runs at a time.  Nothing else is allocated in the pool: the tables (2 W^2
 * floats, kept per context while W stays the same) and a band's cells, masked cells and chain values live in the context's
 * own buffers.  Long ranges run in BANDS of wbx_denoise_band_hops(W, channels) blocks of H output frames;
 * the band size changes no bit of the result.
 * Refused before any device call, nothing allocated, dst_clip and stats untouched, in this order.  First the sizes and
 * parameters, before the clips are looked at — WBX_ERR_INVALID: n_frames of 0 or >= 2^31 - 16; a window_frames that is not
 * a power of two in 64 .. 2048; smooth_hops above 4; smooth_bins above 8; a NULL thr; a thr entry that is negative or not
 * finite (the rows of the clip's channels where the clip is known and has 1 or 2, else the first row); a floor outside
 * [0, 1] or a NaN.  Then the clip — WBX_ERR_INVALID: an unknown source clip; a range past the clip; dst_clip equal to the
 * source; WBX_ERR_UNSUPPORTED: a source that is not F32 or has more than 2 channels; last, wbx_clip_derive's rule:
 * WBX_ERR_INVALID for a dst_clip of 2^24 or more.  WBX_ERR_OOM as for wbx_clip_derive.
 * wbx_clip_denoise_profile is a MEASUREMENT (nothing allocated in the pool): over the COMPLETE windows of the range only —
 * *hops_out = (n - W) / H + 1, hop h at range frame h H — the cells and p as in the analysis above; sums_out[c B + k] =
 * the fp64 sum of p over h ascending from 0.0.  Refused, in this order — WBX_ERR_INVALID: n_frames of 0 or >= 2^31 - 16;
 * the window as above; n_frames < W; a NULL sums_out or hops_out; then the clip as above (no dst_clip).
 * Host-only, no device (wbx_denoise.h, which a C++ compiler takes alone):
 * wbx_denoise_tables writes analysis_out = AC then AS and synthesis_out = YC then YS, 2 B W floats each, [k][j] (either
 *             may be NULL and is left out; WBX_ERR_INVALID for a window as above or both NULL)
 * wbx_denoise_threshold out[i] = strength * (sums[i] / (double)hops) for i < count (WBX_ERR_INVALID: NULL, hops of 0, a
 *             strength that is negative or not finite)
 * wbx_denoise_hops T (0 where n_frames or the window is refused); wbx_denoise_profile_hops the profile's (0 where refused)
 * wbx_denoise_band_hops the blocks of H output frames of one band: 2^22 / (W channels) - 11, the context's stage of 2^22
 *             words per buffer less the 3 hops a band's last block reaches on and 4 hops of box on either side (a band
 *             computes those again instead of keeping them); 0 for a window or channel count as above
 * wbx_denoise_launches the bands of a call: ceil(ceil(n / H) / band_hops); 0 where refused
 * wbx_denoise_check the status of the sizes and parameters alone, `channels` rows of thr read (1 or 2)
 * wbx_denoise_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed denoise or profile call (layer 1's or layer 2's); the tables' upload, where W changed, lies before the first.
 * WBX_ERR_INVALID for NULL arguments or when none has completed.  For tools/bench_denoise.py; nothing else reads it.
 * Not offered: linked-stereo gating, an adaptive or estimated profile, windows above 2048, other overlaps, attack /
 * release smoothing of the gains, de-hum by comb, click repair, denoising at render time or on live input. */
typedef struct wbx_denoise_stats { /* 32 bytes */
  uint64_t hops;
  uint64_t cells;
  uint64_t open_cells;
  uint32_t bands;
  uint32_t reserved; /* 0 */
} wbx_denoise_stats;
wbx_status wbx_denoise_tables(uint32_t window_frames, float* analysis_out, float* synthesis_out);
wbx_status wbx_denoise_threshold(const double* sums, uint64_t hops, size_t count, double strength, double* out);
uint64_t wbx_denoise_hops(uint64_t n_frames, uint32_t window_frames);
uint64_t wbx_denoise_profile_hops(uint64_t n_frames, uint32_t window_frames);
uint32_t wbx_denoise_band_hops(uint32_t window_frames, uint32_t channels);
uint64_t wbx_denoise_launches(uint64_t n_frames, uint32_t window_frames, uint32_t channels);
wbx_status wbx_denoise_check(uint64_t n_frames, uint32_t window_frames, uint32_t smooth_hops, uint32_t smooth_bins,
                             const double* thr, uint32_t channels, double floor);
wbx_status wbx_denoise_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_denoise_profile(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames,
                                    uint32_t window_frames, double* sums_out /* [channels][B] */, uint64_t* hops_out);
wbx_status wbx_clip_denoise(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                            uint32_t smooth_hops, uint32_t smooth_bins, const double* thr /* [channels][B] */, double floor,
                            uint32_t dst_clip, wbx_denoise_stats* stats);

/* Reading a clip along a position curve (varispeed): frames [first_frame, first_frame + n_frames) of a resident F32 clip of
 * 1 or 2 channels read at an arbitrary, caller-given position per output frame through a band-limited interpolator into a
 * NEW F32 clip of out_frames frames, the source's rate and channels, without the samples leaving HBM: tape stop and start,
 * a pitch bend or glide, vibrato, wow and flutter, scratching and reverse sweeps, conforming a recording whose clock
 * drifted; behind wbx_clip_warp, pitch that changes over time at unchanged timing.  wbx_clip_resample and wbx_clip_pitch
 * have one ratio per call; this call has a curve.  The result plays at speed 1.0 through the mix's unity row mode.  No
 * reference counterpart.  This text is the specification; tests/varispeed_model.py restates it in numpy and every table
 * word, position, tile and output sample equals that BIT FOR BIT.
 *   curve     integers only.  knot_shift = g in 4 .. 10, G = 2^g output frames per interval.  knots[i], i in [0, K),
 *             K = ceil(out_frames / G) + 1, is a signed 64-bit position in units of 2^-32 source frames relative to
 *             first_frame and belongs to output frame i*G.  Output frame j = i*G + r lies at
 *               pos = knots[i] + (((knots[i+1] - knots[i]) * r) >> g)
 *             the product in 64 bits, the shift arithmetic (it floors, also for a descending curve whose difference G does
 *             not divide).  Knots need not be monotone: a negative slope plays backwards, a zero slope freezes.  Every
 *             knot lies in [-2^16, n_frames + 2^16] frames; every interval satisfies
 *             (|knots[i+1] - knots[i]| >> 32) + 2 + T <= 4096 (about speed 15 at G = 256, far more at G = 16); K <= 2^22
 *   filter    "Converting a clip's sample rate"'s, with a phase grid instead of a ratio.  guard_num / guard_den >= 1 is
 *             the fastest speed the caller wants protected from aliasing; after dividing by their gcd, M = guard_num,
 *             L = guard_den, and H, T = 2H, cutoff and beta are exactly what that section's quality rule gives for M / L
 *             (guard_num == guard_den: H = Z, cutoff = frac).  T > 512 is refused as there.  One guard serves the call
 *   tables    P = 256 / 512 / 2048 phases for WBX_SRC_FAST / GOOD / BEST.  h has P + 1 rows of T floats: row p is that
 *             section's row formula at the fraction (double)p / (double)P — row P sits at exactly 1.0 —, divided by its own
 *             ascending sum and rounded once to fp32.  D[p][k] = (float)((double)h[p+1][k] - (double)h[p][k]) for p < P
 *   output    f = pos >> 32 (arithmetic), fr = pos & 0xFFFFFFFF, s = 32 - log2 P, p = fr >> s,
 *             t = (double)(fr & (2^s - 1)) * 2^-s (exact: at most 24 bits).  Per channel two fp64 chains from +0.0 in
 *             ascending k:  A = A + (double)h[p][k] * (double)x[f - (H-1) + k],  B = B + (double)D[p][k] * (double)x[...]
 *             (fp32 times fp32 is exact in fp64, so an fma is the same),  then  y = (float)(A + t * B): ONE fp64
 *             multiplication, ONE fp64 addition, one rounding, never an fma (t * B is not exact).  A NaN is stored as
 *             0x7FC00000.  x is ZERO outside [0, n_frames) of the range, whatever the clip holds there, and nothing
 *             outside the range is ever read: a curve may start before the range (a tape start out of silence) or run
 *             past it.  Interpolating the coefficients linearly lets one product serve both rows: the kernel has no
 *             per-tap coefficient arithmetic
 * The filter is NOT an identity: speed 1.0 at integer positions is phase 0's low-pass, as a conversion's is.  At a constant
 * speed whose phases fall on table rows (t = 0) the result equals wbx_clip_resample's at that ratio bit for bit.
 *   tiles     the call is launched over runs of whole consecutive intervals chosen greedily from the front: at most 1024
 *             output frames, and max_f - min_f + T <= 4096, min_f / max_f the least and greatest knots[] >> 32 over the
 *             run's count + 1 knots.  A tile stages source frames [min_f - (H-1), max_f + H]: lo_frame = min_f - (H-1),
 *             span = max_f - min_f + T.  The interval bound lets every interval stand alone
 * wbx_clip_varispeed: dst_clip becomes a new F32 pool clip of out_frames frames (plus the pool's 16 zero frames of padding),
 * replaced or allocated as wbx_clip_derive does it, on the same stream and behind the same ordering; one edit runs at a
 * time.  stats_of_result (may be NULL): wbx_clip_measure of the whole result, a second pass over the output only.  The
 * tables are kept on the device per context and (quality, guard) after their first use; knots and tiles are uploaded per
 * call.
 * Refused before any device call, nothing allocated, dst_clip and the statistics untouched, in this order:
 * WBX_ERR_INVALID for n_frames or out_frames of 0 or >= 2^31 - 16; a knot_shift outside 4 .. 10; NULL knots; n_knots != K; an
 * unknown quality; guard_num or guard_den of 0, or guard_num < guard_den.  WBX_ERR_UNSUPPORTED for K > 2^22 or T > 512.
 * WBX_ERR_INVALID for a knot outside its bounds.  WBX_ERR_UNSUPPORTED for an interval past the span bound (the message
 * names the interval and says to use a smaller knot_shift).  Then the clip — WBX_ERR_INVALID: an unknown source clip, a
 * range past the clip, dst_clip equal to the source; WBX_ERR_UNSUPPORTED: a source that is not F32 or has more than 2
 * channels; last, wbx_clip_derive's rule: WBX_ERR_INVALID for a dst_clip of 2^24 or more.  WBX_ERR_OOM as for
 * wbx_clip_derive.
 * Host-only, no device (wbx_varispeed.h, which a C++ compiler takes alone):
 * wbx_varispeed_plan the filter's numbers (WBX_ERR_INVALID: NULL out, unknown quality, a bad guard; UNSUPPORTED: T > 512)
 * wbx_varispeed_table h as [P+1][T] and d as [P][T] (either may be NULL; WBX_ERR_INVALID when cap_floats is below
 *             (P+1)*T; nothing written after a refusal)
 * wbx_varispeed_position pos of output frame j (WBX_ERR_INVALID: NULL, a knot_shift outside 4 .. 10, j past the curve:
 *             (j >> g) + 1 >= n_knots unless j is the last knot's own frame)
 * wbx_varispeed_check the refusals above that need no clip, in that order
 * wbx_varispeed_tiles the tiles of a call wbx_varispeed_check accepts (refused as there): *n_tiles the count, the first
 *             min(count, cap) records written (tiles may be NULL with cap 0)
 * wbx_varispeed_max_knots 2^22
 * wbx_varispeed_ms: device milliseconds between two events on the edits' stream around the uploads and the launch of the
 * context's last completed varispeed call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has
 * completed.  For tools/bench_varispeed.py; nothing else reads it.
 * Not offered: a cutoff that follows the speed within one call, more than 2^22 knots, intervals faster than the span bound,
 * varispeed at render time or on live input, more than 2 channels, in-place edits. */
typedef struct wbx_varispeed_info { /* 32 bytes */
  uint32_t half_width;       /* H */
  uint32_t taps;             /* T = 2H */
  uint32_t phases;           /* P */
  uint32_t reserved;
  double cutoff, beta;
} wbx_varispeed_info;
typedef struct wbx_varispeed_tile { /* 24 bytes */
  uint32_t first_out, n_out; /* output frames [first_out, first_out + n_out) */
  int64_t lo_frame;          /* the first staged frame of the range (may be negative) */
  uint32_t span;             /* staged frames per channel */
  uint32_t reserved;
} wbx_varispeed_tile;
wbx_status wbx_varispeed_plan(int quality, uint32_t guard_num, uint32_t guard_den, wbx_varispeed_info* out);
wbx_status wbx_varispeed_table(int quality, uint32_t guard_num, uint32_t guard_den, float* h, float* d, size_t cap_floats);
wbx_status wbx_varispeed_position(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t j, int64_t* pos);
wbx_status wbx_varispeed_check(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t n_frames,
                               uint64_t out_frames, int quality, uint32_t guard_num, uint32_t guard_den);
wbx_status wbx_varispeed_tiles(const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, uint64_t n_frames,
                               uint64_t out_frames, int quality, uint32_t guard_num, uint32_t guard_den,
                               wbx_varispeed_tile* tiles, uint64_t cap, uint64_t* n_tiles);
uint64_t wbx_varispeed_max_knots(void);
wbx_status wbx_varispeed_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_varispeed(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                              uint64_t out_frames, const int64_t* knots, uint64_t n_knots, uint32_t knot_shift, int quality,
                              uint32_t guard_num, uint32_t guard_den, wbx_clip_stats* stats_of_result);

/* Stretching a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels time-stretched
 * into a NEW F32 clip of out_frames frames — another LENGTH at the same PITCH — without the samples leaving HBM, by WSOLA
 * (waveform-similarity overlap-add): fitting a loop or a take to the session's tempo.  The result plays at speed 1.0 through
 * the unity row mode; the reference's own `stretch` resize only changes the playback speed (pitch moves with tempo).  No
 * reference counterpart.  Purely time-domain: no FFT, no log, no sqrt.  This text is the specification;
 * tests/stretch_model.py restates it in numpy, and the positions, the window table and every output sample equal that BIT
 * FOR BIT.  Every operator below is one IEEE fp64 operation in the order written and nothing is fused; where both factors
 * are fp32 values the product is exact in fp64, so an fma there is the same thing.
 *   input     x[c][i], i in [0, n), n = n_frames: the (double) of the range's fp32 sample; a value that is not finite enters
 *             as 0.0.  x is zero outside [0, n), whatever the clip holds beside the range; nothing beside it is ever read
 *   detector  linked channels, one set of positions for all: mono d[i] = x[0][i]; stereo d[i] = (float)(0.5 * (x[0][i] +
 *             x[1][i])), one rounding to fp32 (it cannot overflow).  d is an fp32 value, so every product below is exact
 *   shape     N = window_frames, a multiple of 8 in [32, 8192]; Hs = N / 2; D = tolerance_frames in [0, 4096];
 *             m = out_frames; K = ceil(m / Hs) steps (wbx_stretch_steps)
 *   anchors   a_k = floor(k * Hs * n / m) in 64-bit integers (wbx_stretch_anchor); a_k <= n - 1
 *   positions with p_{-1} = -Hs, for k = 0 .. K - 1: c_k = p_{k-1} + Hs, the natural continuation; lo = max(a_k - D, 0);
 *             hi = min(a_k + D, n - 1).  If lo <= c_k <= hi, p_k = c_k with no search (so p_0 = 0).  Otherwise every
 *             candidate q in [lo, hi] is scored:
 *                 s = 0.0; E = 0.0; for i = 0 .. Hs - 1 ascending: s = s + d[c_k + i] * d[q + i]; E = E + d[q + i] * d[q + i]
 *                 score = (E == 0.0) ? 0.0 : (s * |s|) / E
 *             — a signed, energy-normalised correlation without a square root; it stays below 2^540, so nothing overflows
 *             and no NaN can arise — and p_k is the candidate with the greatest score, the LOWEST q among equals.  A
 *             template past the end of the range is all zeros: every score is 0 and p_k = lo.  Positions are int32
 *   window    wbx_stretch_window (host-only, no libm): for i in [0, Hs): t = sinpi((double)i / (double)N) ("Converting a
 *             clip's sample rate"'s sinpi); w_up[i] = t * t; w_dn[i] = 1.0 - w_up[i].  out receives w_up[0 .. Hs), then
 *             w_dn[0 .. Hs): N doubles
 *   output    frame j = k * Hs + i, i in [0, Hs), j < m, each channel: if p_k == c_k, y = (float)x[c][p_k + i] — the
 *             source's sample unchanged, so a range stretched to its own length is a copy, bit for bit; otherwise
 *             y = (float)((w_up[i] * x[c][p_k + i]) + (w_dn[i] * x[c][c_k + i])).  A NaN cannot arise
 * dst_clip becomes a new F32 pool clip of m frames (plus the pool's 16 zero frames of padding) with the source's channels
 * and rate, replaced or allocated as wbx_clip_derive does it, on the same stream and behind the same ordering; one edit,
 * conversion, filter, convolution, limit, dynamics or stretch call runs at a time.  positions_out (may be NULL): the K
 * positions (a caller who asks for them makes the call wait band by band).  info (may be NULL): steps = K; searched_steps,
 * the steps that scored candidates; candidates, the total scored; max_shift, the maximum of |p_k - a_k|; launches, the
 * kernel launches of the call.  stats_of_result (may be NULL): wbx_clip_measure of the whole result.
 * The search is a chain (step k needs p_{k-1}): ONE workgroup walks the steps of a launch in order; a launch takes the steps
 * whose scored terms (candidates x Hs, and wbx_stretch_step_terms more per step for what a searched step costs besides)
 * stay within wbx_stretch_launch_terms if every one searched its whole span (wbx_stretch_launch_steps, at least 1), and the positions are staged in bands of wbx_stretch_band_steps steps.
 * Refused before any device call, nothing allocated, dst_clip untouched — WBX_ERR_INVALID: an unknown source, n_frames or
 * out_frames of 0, a range past the clip, dst_clip equal to the source, n_frames or out_frames >= 2^31 - 16, a
 * window_frames that is not a multiple of 8 or lies outside [32, 8192], tolerance_frames > 4096, a non-NULL positions_out
 * with positions_cap < K; WBX_ERR_UNSUPPORTED: a clip that is not F32 or has more than 2 channels, out_frames > 8 n_frames
 * or n_frames > 8 out_frames.  The sizes are judged before the clip is looked at.  WBX_ERR_OOM as for wbx_clip_derive.
 * Host-only, no device (wbx_stretch.h, which a C++ compiler takes alone): wbx_stretch_steps (0 for a window the call refuses),
 * wbx_stretch_anchor (any k, n and m; 0 for such a window or m == 0), wbx_stretch_window (WBX_ERR_INVALID: NULL out, such a
 * window, cap_doubles < N; nothing is written then), wbx_stretch_band_steps, wbx_stretch_launch_terms, wbx_stretch_step_terms,
 * wbx_stretch_launch_steps (0 for such a window or n_frames == 0).
 * wbx_stretch_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed stretch call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_stretch.py; nothing else reads it.
 * Not offered (pitch shifting is "Pitch-shifting a clip" below): transient or formant preservation,
 * unlinked stereo, a phase vocoder or anything with an FFT, stretching at render time, several clips in one call, more than
 * 2 channels, in-place edits; the reference's `stretch` resize is unchanged. */
typedef struct wbx_stretch_info {       /* 32 bytes */
  uint64_t steps;
  uint64_t searched_steps;
  uint64_t candidates;
  uint32_t max_shift;
  uint32_t launches;
} wbx_stretch_info;
uint64_t wbx_stretch_steps(uint64_t out_frames, uint32_t window_frames);
uint64_t wbx_stretch_anchor(uint64_t k, uint64_t n_frames, uint64_t out_frames, uint32_t window_frames);
wbx_status wbx_stretch_window(uint32_t window_frames, double* out /* [window_frames] */, size_t cap_doubles);
uint32_t wbx_stretch_band_steps(void);
uint64_t wbx_stretch_launch_terms(void);
uint64_t wbx_stretch_step_terms(void);
uint32_t wbx_stretch_launch_steps(uint64_t n_frames, uint32_t window_frames, uint32_t tolerance_frames);
wbx_status wbx_stretch_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_stretch(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                            uint64_t out_frames, uint32_t window_frames, uint32_t tolerance_frames, int32_t* positions_out,
                            size_t positions_cap, wbx_stretch_info* info, wbx_clip_stats* stats_of_result);

/* Warping a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels warped along time
 * markers into a NEW F32 clip of out_frames frames at the same PITCH — quantizing a take to the grid, conforming it to a
 * tempo map.  A marker is a promise that source frame src_frame sounds at output frame out_frame; between two markers the
 * clip is stretched by WSOLA exactly as "Stretching a clip" does it.  No reference counterpart.  This text is the
 * specification; tests/warp_model.py restates it in numpy, and the positions, the info and every output sample equal that BIT
 * FOR BIT.  Everything not said here is "Stretching a clip" word for word: x, the non-finite rule and zero outside [0, n) of
 * the RANGE, the linked detector d, N, Hs = N / 2, D, the score and the lowest candidate among equals, wbx_stretch_window,
 * one IEEE fp64 operation per operator and nothing fused.
 *   markers   M = n_markers pairs (src_frame, out_frame), 0 <= M <= 65535; both columns strictly ascending, 0 < src_frame <
 *             n, 0 < out_frame < m.  With (s_0, t_0) = (0, 0) and (s_{M+1}, t_{M+1}) = (n, m) they bound S = M + 1
 *             segments; segment j has n_j = s_{j+1} - s_j source frames and m_j = t_{j+1} - t_j output frames
 *   steps     segment j has K_j = ceil(m_j / Hs) steps; its step i starts at output frame o = t_j + i * Hs and is
 *             l = min(Hs, t_{j+1} - o) frames long (only a segment's last step may be short).  The global step index is
 *             k = base_j + i, base_j = the sum of K_j' over j' < j; K = the sum of all K_j (wbx_warp_steps)
 *   anchors   a_k = s_j + floor(i * Hs * n_j / m_j) in 64-bit integers
 *   continuation  c_k = p_{k-1} + l_{k-1}, with p_{-1} = -Hs and l_{-1} = Hs, so c_0 = 0
 *   positions i = 0 (pinned): p_k = s_j, never scored, counted in neither searched_steps nor candidates.  i >= 1: the
 *             stretch's rule as it is, with lo = max(a_k - D, 0) and hi = min(a_k + D, n - 1) — the clamp is the range's,
 *             not the segment's: candidates may lie beyond a marker, nothing outside the range is read.  p_k = c_k where
 *             lo <= c_k <= hi; otherwise every q in [lo, hi] is scored over Hs terms against the template d[c_k + .]
 *   output    frame o + i', i' < l, each channel: (float)x[p_k + i'] where p_k == c_k; otherwise
 *             (float)((w_up[i'] * x[p_k + i']) + (w_dn[i'] * x[c_k + i'])).  A pinned step is blended like any other step
 *             that left its continuation: a marker is a crossfade over one hop into s_j, not a cut
 * Consequences: with M = 0 the call IS wbx_clip_stretch — positions, info and samples, bit for bit.  A segment's positions
 * depend on nothing outside it but the source: the chain starts at the pinned s_j (its first step's blend partner c_k comes
 * from the segment before).  A marker cuts the chain, so the segments are searched side by side, one workgroup each.
 * dst_clip, positions_out (the K positions, copied at the end of the call), stats_of_result and the ordering are
 * wbx_clip_stretch's.  info (may be NULL): steps = K; searched_steps; candidates; max_shift = max |p_k - a_k|; segments = S;
 * longest_segment_steps = max K_j; launches, the kernel launches of the call (= wbx_warp_launches).
 * Launches: round r walks steps [r S_r, (r + 1) S_r) of every segment that has them, S_r = wbx_stretch_launch_steps(n, N,
 * D), one 512-lane workgroup per such segment, in slices of at most wbx_warp_launch_segments() workgroups; one overlap-add
 * launch covers the call after all searches.
 * Refused before any device call, nothing allocated, dst_clip and the outputs untouched.  First everything
 * wbx_clip_stretch refuses for (n, m, N, D, dst == src), with the same statuses.  Next WBX_ERR_INVALID: NULL markers with
 * n_markers > 0, n_markers > 65535, a column that is not strictly ascending, a frame that is 0 or not below n / m, a
 * non-NULL positions_out with positions_cap < K.  Next WBX_ERR_UNSUPPORTED: a segment with m_j > 8 n_j or n_j > 8 m_j, K >
 * 2^22.  Last the clip, as wbx_clip_stretch judges it.  The whole-range ratio rule of the stretch is not applied on its own;
 * the segments' rule replaces it (with M = 0 they are the same rule).
 * Host-only, no device (wbx_warp.h, which a C++ compiler takes alone): wbx_warp_check, the status a call gets before its
 * clip is looked at; wbx_warp_steps (0 for a window or markers the call refuses); wbx_warp_segments (fills S records;
 * WBX_ERR_INVALID for NULL out, cap < S, such a window or markers); wbx_warp_max_markers (65535); wbx_warp_max_steps (2^22);
 * wbx_warp_launch_segments; wbx_warp_launches (0 for a call wbx_warp_check refuses).
 * wbx_warp_ms: as wbx_stretch_ms, for the context's last completed warp call.  For tools/bench_warp.py.
 * Not offered: transient detection inside the call, holding more than the natural continuation after a marker, a
 * time-varying pitch, warping at render time, more than 2 channels. */
typedef struct wbx_warp_marker {        /* 16 bytes */
  uint64_t src_frame;
  uint64_t out_frame;
} wbx_warp_marker;
typedef struct wbx_warp_info {          /* 40 bytes */
  uint64_t steps;
  uint64_t searched_steps;
  uint64_t candidates;
  uint32_t max_shift;
  uint32_t launches;
  uint32_t segments;
  uint32_t longest_segment_steps;
} wbx_warp_info;
typedef struct wbx_warp_segment {       /* 32 bytes */
  uint64_t src_frame;                   /* s_j */
  uint64_t out_frame;                   /* t_j */
  uint64_t first_step;                  /* base_j */
  uint64_t steps;                       /* K_j */
} wbx_warp_segment;
wbx_status wbx_warp_check(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                          uint32_t window_frames, uint32_t tolerance_frames);
uint64_t wbx_warp_steps(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                        uint32_t window_frames);
wbx_status wbx_warp_segments(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                             uint32_t window_frames, wbx_warp_segment* out /* [n_markers + 1] */, size_t cap_segments);
uint32_t wbx_warp_max_markers(void);
uint64_t wbx_warp_max_steps(void);
uint32_t wbx_warp_launch_segments(void);
uint64_t wbx_warp_launches(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                           uint32_t window_frames, uint32_t tolerance_frames);
wbx_status wbx_warp_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_warp(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                         uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers, uint32_t window_frames,
                         uint32_t tolerance_frames, int32_t* positions_out, size_t positions_cap, wbx_warp_info* info,
                         wbx_clip_stats* stats_of_result);

/* Pitch-shifting a clip: frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2 channels transposed
 * into a NEW F32 clip of out_frames frames — another PITCH, by the ratio num / den (above 1: up), at a length of the
 * caller's choice (out_frames = n_frames is the plain transposition) — without the samples leaving HBM.  The result keeps
 * the source's RATE, so it plays at speed 1.0 through the unity row mode.  No reference counterpart.  The result is, by
 * definition and BIT FOR BIT, the composition of two texts above; tests/pitch_model.py is their two models one after the
 * other.
 *   ratio     g = gcd(num, den), L = den / g, M = num / g: the plan of wbx_resample_plan(num, den, quality) (H, T, table)
 *   length    m = out_frames; the intermediate has m' = ceil(m * M / L) frames (wbx_pitch_mid_frames)
 *   stretch   y'[c][g], g in [0, m'), is what "Stretching a clip" STORES for wbx_clip_stretch(the range, out_frames = m',
 *             window_frames, tolerance_frames): fp32 values, the same positions p_k, k < K' = ceil(m' / Hs), the copy
 *             branch or the blend rounded once to fp32
 *   output    frame j in [0, m), each channel: what "Converting a clip's sample rate" STORES for frame j of converting the
 *             m'-frame intermediate with (L, M, quality): t = j * M, i = t div L, p = t mod L, T fp64 multiply-adds in
 *             ascending tap order over y'[c][i - (H - 1) + k], y' zero outside [0, m'), one rounding to fp32, a NaN as
 *             0x7FC00000.  Only the first m of that conversion's frames are kept; floor((m - 1) * M / L) < m' always
 *             holds, so every kept frame lies inside the intermediate
 * The intermediate is never stored: the searches fill one buffer of all K' positions, and ONE further launch feeds the filter
 * straight from the overlap-add; nothing of m' frames is allocated in the pool.
 * dst_clip becomes a new F32 pool clip of m frames (plus the pool's 16 zero frames of padding) with the source's channels
 * and rate, replaced or allocated as wbx_clip_derive does it, on the same stream and behind the same ordering; one edit,
 * conversion, filter, convolution, limit, dynamics, stretch or pitch call runs at a time.  positions_out (may be NULL): the
 * K' positions, copied once after the last search launch.  info (may be NULL): steps = K', searched_steps, candidates and
 * max_shift of the stretch to m' frames as in wbx_stretch_info; mid_frames = m'; launches, the kernel launches of the call
 * (the searches and one more); L, M.  stats_of_result (may be NULL): wbx_clip_measure of the whole result.
 * Refused before any device call, nothing allocated, dst_clip untouched; the sizes are judged before the clip is looked at,
 * in this order.  WBX_ERR_INVALID: an unknown source, dst_clip equal to the source; n_frames or out_frames of 0, num or den
 * of 0, num == den after reduction (a ratio of 1 is wbx_clip_stretch's job: the filter is no identity), an unknown quality,
 * out_frames >= 2^31 - 16.  WBX_ERR_UNSUPPORTED: num > 4 den or den > 4 num (two octaves either way), what
 * wbx_resample_plan refuses (L > 1280, T > 512).  Then everything wbx_clip_stretch refuses for (n_frames, m', window_frames,
 * tolerance_frames), with its status — WBX_ERR_INVALID: n_frames or m' >= 2^31 - 16, the window, the tolerance, a non-NULL
 * positions_out with positions_cap < K'; WBX_ERR_UNSUPPORTED: m' > 8 n_frames or n_frames > 8 m'.  WBX_ERR_UNSUPPORTED:
 * K' > wbx_pitch_max_steps() (2^22: the positions take at most 16 MB + 4 B).  Then the clip — WBX_ERR_UNSUPPORTED: not F32
 * or more than 2 channels; WBX_ERR_INVALID: a range past the clip.  WBX_ERR_OOM as for wbx_clip_derive.
 * Host-only, no device (wbx_pitch.h, which a C++ compiler takes alone): wbx_pitch_mid_frames (any out_frames: the product
 * in 128 bits, 2^64 - 1 where it does not fit; 0 where the call would refuse the RATIO), wbx_pitch_max_steps,
 * wbx_pitch_launch_shape (wbx_resample_launch_shape of the call's last launch: the conversion by M / L to out_frames frames;
 * WBX_ERR_UNSUPPORTED for a ratio or a plan the call refuses, WBX_ERR_INVALID for out_frames of 0 or >= 2^31 - 16 or a NULL
 * pointer).
 * wbx_pitch_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed pitch call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_pitch.py; nothing else reads it.
 * Not offered: formant preservation, pitch correction over time (detection is "Tracking a clip's pitch" below), ratios
 * beyond two octaves, pitch shifting at render time, unlinked stereo, more than 2 channels, in-place edits. */
typedef struct wbx_pitch_info {         /* 48 bytes */
  uint64_t steps;
  uint64_t searched_steps;
  uint64_t candidates;
  uint64_t mid_frames;
  uint32_t max_shift;
  uint32_t launches;
  uint32_t L;
  uint32_t M;
} wbx_pitch_info;
uint64_t wbx_pitch_mid_frames(uint64_t out_frames, uint32_t num, uint32_t den);
uint32_t wbx_pitch_max_steps(void);
wbx_status wbx_pitch_launch_shape(uint32_t num, uint32_t den, int quality, uint64_t out_frames, uint32_t* tile, uint32_t* span,
                                  uint32_t* n_tiles, uint32_t* grid);
wbx_status wbx_pitch_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_pitch(wbx_ctx* ctx, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                          uint64_t out_frames, uint32_t num, uint32_t den, int quality, uint32_t window_frames,
                          uint32_t tolerance_frames, int32_t* positions_out, size_t positions_cap, wbx_pitch_info* info,
                          wbx_clip_stats* stats_of_result);

/* Tracking a clip's pitch: the period of frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2
 * channels, one record per hop, by YIN's cumulative-mean-normalized difference in the time domain — without the samples
 * leaving HBM.  A MEASUREMENT, like wbx_clip_loudness: nothing is allocated in the pool and no clip is created.  No
 * reference counterpart.  The arithmetic is part of the interface; tests/f0_model.py restates it in numpy, operation for
 * operation, and the records equal it BIT FOR BIT.  Every operator below is ONE IEEE fp64 operation in the order written;
 * nothing is fused (where both factors are fp32 values the product is exact, so an fma there is the same thing).
 *   input     x and the detector d exactly as in "Stretching a clip": x[c][g] the range's fp32 samples as doubles, what is
 *             not finite entering as 0.0, zero outside [0, n), nothing beside the range ever read; mono d = x[0], stereo
 *             d = (float)(0.5 * (x[0] + x[1]))
 *   shape     W = window_frames, a multiple of 8 in [64, 8192]; tau_max in [8, 4095]; tau_min in [2, tau_max - 1];
 *             H = hop_frames in [1, 2^20]; threshold finite, in (0, 1].
 *             hops = n >= W + tau_max ? (n - W - tau_max) / H + 1 : 0 (wbx_f0_hops): only complete frames count, and
 *             hops == 0 is no error
 *   per hop h with t = h * H, for every lag tau in [0, tau_max]:
 *             r = 0; E = 0; for j = 0 .. W - 1 ascending: r = r + d[t+j] * d[t+j+tau]; E = E + d[t+j+tau] * d[t+j+tau]
 *             E0 = E(0) (which equals r(0) bit for bit)
 *             dd(tau) = (E0 + E(tau)) - (2.0 * r(tau)); a dd < 0.0 becomes 0.0; dd(0) is 0.0
 *   mean      the cumulative mean in runs of 8 lags — the two-level order IS the definition, not an approximation of a flat
 *             sum (it is what a lane that owns 8 lags computes, and it shortens the serial chain eightfold): tau = 8 g + i,
 *             lags above tau_max counting 0.0; P(g,0) = dd(8g), P(g,i) = P(g,i-1) + dd(8g+i); T(g) = P(g,7); B(0) = 0.0,
 *             B(g) = B(g-1) + T(g-1); S(tau) = B(g) + P(g,i).
 *             c(0) = 1.0; for tau >= 1: c(tau) = (S(tau) == 0.0) ? 1.0 : (dd(tau) * (double)tau) / S(tau)
 *   pick      lag = the lowest tau in [tau_min, tau_max - 1] with c(tau) < threshold and c(tau+1) >= c(tau); then
 *             voiced = 1 (YIN's "first dip below the threshold, walked down to its minimum", as a predicate that needs no
 *             walk).  If there is none: voiced = 0 and lag = the tau of that interval with the least c, the lowest among
 *             equals
 *   refine    a = c(lag-1), b = c(lag), g = c(lag+1); den = (a + g) - (2.0 * b);
 *             off = (den > 0.0 && a >= b && g >= b) ? (0.5 * (a - g)) / den : 0.0; period = (double)lag + off
 *   record    wbx_f0_frame: period, dip = b, energy = E0, lag, voiced
 * No NaN can arise and nothing overflows.  Silence gives c == 1 everywhere, voiced = 0, lag = tau_min, off = 0.  The
 * frequency is rate / period: the caller's division, not part of the contract.
 * The call runs on the edits' stream behind wbx_clip_derive's ordering, one edit or measurement at a time, in launches of
 * at most wbx_f0_launch_hops(window_frames, tau_max) hops — max(1, wbx_f0_launch_terms() / (W * (tau_max + 1))), whole
 * eights where there are 8 or more — and returns when frames_out holds all hops records, copied once after the last launch.
 * info (may be NULL): hops; voiced_hops; terms = hops * W * (tau_max + 1); launches.
 * Refused before any device call, frames_out untouched; the sizes are judged before the clip is looked at, in this order.
 * WBX_ERR_INVALID: an unknown clip; n_frames of 0 or >= 2^31 - 16; a window, lag bound, hop or threshold outside the ranges
 * above (a NaN threshold included); a NULL frames_out with hops > 0; frames_cap < hops.  WBX_ERR_UNSUPPORTED:
 * hops > wbx_f0_max_hops() (2^20: the records take at most 32 MB).  Then the clip — WBX_ERR_UNSUPPORTED: not F32 or more
 * than 2 channels; WBX_ERR_INVALID: a range past the clip.
 * Host-only, no device (wbx_f0.h, which a C++ compiler takes alone): wbx_f0_hops (0 for a shape the call refuses),
 * wbx_f0_check (the argument check above without the clip: its status), wbx_f0_max_hops, wbx_f0_launch_terms,
 * wbx_f0_launch_hops (at least 1; 0 for a shape the call refuses).
 * wbx_f0_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed f0 call (layer 1's or layer 2's).  A completed wbx_clip_tempo counts as one: after it the figure is that of the
 * tempo call's f0 launches over the novelty, without its energy and novelty passes.  WBX_ERR_INVALID for NULL arguments
 * or when none has completed.  For tools/bench_f0.py and tools/bench_onsets.py; nothing else reads it.
 * Not offered: polyphonic material, pitch correction over time, a smoothed or Viterbi track, tracking at render time,
 * unlinked stereo, more than 2 channels (onsets and tempo are "Finding a clip's onsets and tempo" below). */
typedef struct wbx_f0_frame {           /* 32 bytes */
  double period;
  double dip;
  double energy;
  uint32_t lag;
  uint32_t voiced;
} wbx_f0_frame;
typedef struct wbx_f0_info {            /* 32 bytes */
  uint64_t hops;
  uint64_t voiced_hops;
  uint64_t terms;
  uint32_t launches;
  uint32_t _pad;
} wbx_f0_info;
uint64_t wbx_f0_hops(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames, uint32_t tau_max);
wbx_status wbx_f0_check(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max,
                        double threshold, int has_frames_out, size_t frames_cap);
uint64_t wbx_f0_max_hops(void);
uint64_t wbx_f0_launch_terms(void);
uint32_t wbx_f0_launch_hops(uint32_t window_frames, uint32_t tau_max);
wbx_status wbx_f0_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_f0(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                       uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max, double threshold, wbx_f0_frame* frames_out,
                       size_t frames_cap, wbx_f0_info* info);

/* Aligning two clips: by how many frames clip B lags clip A, and whether its polarity is flipped, from the cross-correlation
 * of a template of A — frames [a_first, a_first + n) of the reference clip — with frames [b_first, b_first + m) of the
 * clip to be aligned, over signed lags, without the samples leaving HBM.  A MEASUREMENT, like wbx_clip_loudness and
 * wbx_clip_f0: nothing is allocated in the pool and no clip is created.  No reference counterpart.  The arithmetic is part
 * of the interface; tests/align_model.py restates it in numpy, operation for operation, and info and the curve equal it
 * BIT FOR BIT.  Every operator below is ONE IEEE fp64 operation in the order written; nothing is fused (where both factors
 * are fp32 values the product is exact, so an fma there is the same thing).
 *   input     each clip a resident F32 clip of 1 or 2 channels (the counts may differ), each through "Stretching a clip"'s
 *             linked detector on its own: mono d = x[0], stereo d = (float)(0.5 * (x[0] + x[1])), what is not finite
 *             entering as 0.0.  da[i] for i in [0, n); db[i] is zero outside [0, m); nothing beside either range is ever read
 *   shape     n a multiple of 8 in [64, 2^24]; m in [1, 2^31 - 16); lags are signed, lag_min <= lag_max, both in
 *             [-2^24, 2^24]; lags = lag_max - lag_min + 1 <= 2^17 (wbx_align_max_lags).  C = 2048 terms per chunk
 *             (wbx_align_chunk_frames); chunks = ceil(n / C) (wbx_align_chunks); the last chunk has n - (chunks - 1) * C
 *             terms, a multiple of 8
 *   per lag L, per chunk k — a partial, from rest:
 *             pr = 0; pE = 0; for i = k*C .. min((k+1)*C, n) - 1 ascending:
 *             pr = pr + da[i] * db[i+L]; pE = pE + db[i+L] * db[i+L]
 *   per lag L — the fold:
 *             r = 0; E = 0; for k = 0 .. chunks - 1 ascending: r = r + pr(L,k); E = E + pE(L,k)
 *             The two-level order IS the definition, not an approximation of a flat sum, as the cumulative mean of
 *             "Tracking a clip's pitch" is: it is what lets the chunks of a long template run side by side.
 *             Ea is the same two-level sum of da[i] * da[i]
 *   score     score(L) = (E == 0.0) ? 0.0 : (r * |r|) / E — square-root free, its arg-max that of r / sqrt(E);
 *             with WBX_ALIGN_EITHER_POLARITY in flags: score(L) = (E == 0.0) ? 0.0 : (r * r) / E
 *   pick      lag = the L with the greatest score, the LOWEST L among equals; silence gives lag = lag_min.
 *             inverted = r(lag) < 0.0
 *   refine    only when lag - 1 and lag + 1 both lie in [lag_min, lag_max]: a = score(lag-1), b = score(lag),
 *             g = score(lag+1); den = (2.0 * b) - (a + g);
 *             offset = (den > 0.0 && b >= a && b >= g) ? (0.5 * (g - a)) / den : 0.0.  Otherwise offset = 0.0.
 *             offset is an estimate whose magnitude is at most 0.5; the contract is that it equals the model, and no
 *             sub-sample accuracy is claimed
 *   info      wbx_align_info: lag, inverted, offset, score, r, energy = E at the lag, ref_energy = Ea,
 *             confidence = (Ea == 0.0) ? 0.0 : score / Ea, which lies in [-1, 1] up to rounding (Cauchy-Schwarz);
 *             lags, chunks, terms = lags * n, launches
 *   curve     curve_out (may be NULL): records of 16 bytes {r, energy}, one per lag from lag_min upward;
 *             curve_cap >= lags where it is not NULL
 * No NaN can arise and nothing overflows.  A and B may be the same clip.
 * The call runs on the edits' stream behind wbx_clip_derive's ordering, one edit or measurement at a time, in bands of at
 * most wbx_align_band_chunks(lags) chunks — what a device stage of 2^22 partials (64 MB, made at first use) holds, and at
 * most 2^39 terms — each band one launch for the partials and one that folds them onto the running r and E, the bands
 * continuing the same ascending chain, so that the cut into bands does not change a bit.  wbx_align_launches(n, lags) =
 * 2 * bands + 2: Ea's partials first, the pick last.  info and the curve are copied out once at the end.
 * Refused before any device call, info and curve_out untouched; the sizes are judged before the clips are looked at, in
 * this order.  WBX_ERR_INVALID: an unknown clip (the reference first); n_frames not a multiple of 8 in [64, 2^24];
 * m_frames of 0 or >= 2^31 - 16; lag_min, then lag_max, outside [-2^24, 2^24]; lag_min > lag_max; unknown flag bits; info
 * and curve_out both NULL; curve_cap < lags with a curve_out.  WBX_ERR_UNSUPPORTED: lags > 2^17.  Then the clips —
 * WBX_ERR_UNSUPPORTED: the reference, then the clip, not F32 or of more than 2 channels; different sample rates;
 * WBX_ERR_INVALID: the reference's range, then the clip's, past its clip.
 * Host-only, no device (wbx_align.h, which a C++ compiler takes alone): wbx_align_check (the argument check above without
 * the clips: its status), wbx_align_chunks (0 for an n the call refuses), wbx_align_max_lags, wbx_align_chunk_frames,
 * wbx_align_band_chunks (at least 1; 0 for lags of 0 or above 2^17), wbx_align_launches (0 for a refused shape).
 * wbx_align_ms: device milliseconds between two events on the edits' stream around the launches of the context's last
 * completed align call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.  For
 * tools/bench_align.py; nothing else reads it.
 * Not offered: more than 2 channels, unlinked stereo, an alignment that drifts over time, alignment at render time. */
#define WBX_ALIGN_EITHER_POLARITY 1u
typedef struct wbx_align_info {         /* 80 bytes */
  int32_t lag;
  uint32_t inverted;
  double offset;
  double score;
  double r;
  double energy;
  double ref_energy;
  double confidence;
  uint32_t lags;
  uint32_t chunks;
  uint64_t terms;
  uint32_t launches;
  uint32_t _pad;
} wbx_align_info;
typedef struct wbx_align_point {        /* 16 bytes */
  double r;
  double energy;
} wbx_align_point;
wbx_status wbx_align_check(uint64_t n_frames, uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags, int has_info,
                           int has_curve_out, size_t curve_cap);
uint32_t wbx_align_chunks(uint64_t n_frames);
uint64_t wbx_align_max_lags(void);
uint32_t wbx_align_chunk_frames(void);
uint32_t wbx_align_band_chunks(uint64_t lags);
uint32_t wbx_align_launches(uint64_t n_frames, uint64_t lags);
wbx_status wbx_align_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_align(wbx_ctx* ctx, uint32_t ref_clip, uint64_t a_first, uint64_t n_frames, uint32_t clip, uint64_t b_first,
                          uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags, wbx_align_info* info,
                          wbx_align_point* curve_out, size_t curve_cap);

/* Finding a clip's onsets and tempo: an onset-strength curve (the "novelty") of frames [first_frame, first_frame + n_frames)
 * of a resident F32 clip of 1 or 2 channels, one value per hop, from the rise of two hop energies — the signal's and its
 * first difference's, which weighs the high end — the onsets picked from it, and its period tracked by "Tracking a clip's
 * pitch" with hops in the place of frames: the tempo.  MEASUREMENTS, like wbx_clip_loudness and wbx_clip_f0: nothing is
 * allocated in the pool and no clip is created.  No reference counterpart.  The arithmetic is part of the interface;
 * tests/onset_model.py restates it in numpy, operation for operation, and the records equal it BIT FOR BIT.  Every operator
 * below is ONE IEEE fp64 operation in the order written; nothing is fused unless stated.
 *   input     x and the detector d exactly as in "Stretching a clip": what is not finite enters as 0.0; mono d = x[0],
 *             stereo d = (float)(0.5 * (x[0] + x[1])).  d[-1] = 0.0: the frame before the range is never read, and neither is
 *             anything after it
 *   shape     H = hop_frames, a multiple of 64 in [64, 16384]; q = H / 64.  floor_power finite, in [1e-30, 1];
 *             floor = (double)H * floor_power.  hops = n / H (wbx_onset_hops): only complete hops count, and hops == 0 is no
 *             error.  n in [1, 2^31 - 16); hops at most wbx_onset_max_hops() = 2^20
 *   energies  per hop h and run i = 0 .. 63, over frames t = h H + i q + j, j ascending, from a = b = 0.0:
 *             a = a + d[t] * d[t] (the product is exact, so an fma is the same thing);
 *             e = d[t] - d[t-1]; b = b + (e * e) (the product rounded before the addition: NOT an fma).
 *             The 64 run sums are added as a balanced tree of adjacent pairs: s0[i] = a_i, s(k+1)[i] = sk[2i] + sk[2i+1],
 *             A(h) = s6[0]; B(h) the same way from b_i (an xor butterfly over a wave computes exactly this)
 *   novelty   for X in {A, B}: ref = max(X(h-1), X(h-2), X(h-3)), hops before 0 counting 0.0; up = X(h) - ref, an up that
 *             is not > 0.0 becoming 0.0; rise = up / ((X(h) + ref) + floor).  o(h) = (float)(rise_A + rise_B), in [0, 2]: below 2 before
 *             the roundings, 2.0 where the floor vanishes beside both energies.
 *             ((a - b) / (a + b) is tanh of half the log ratio: a rise measure that does not depend on the level and needs
 *             no log.)  No NaN can arise; silence gives o == 0
 *   pick      on the host, from the records (wbx_onset_pick is this alone).  onset(h) = 1 iff o(h) >= threshold; no
 *             o(g) >= o(h) for g in [h-w, h); no o(g) > o(h) for g in (h, h+w] (the earliest of equals wins); and
 *             (double)o(h) >= m / cnt + delta, m the ascending fp64 sum of o over [max(0, h-a), min(hops-1, h+a)] and cnt
 *             its length.  threshold in (0, 2], delta in [0, 2], w in [0, 64], a in [0, 256]
 *   record    wbx_onset_frame: energy = A, edge_energy = B, novelty = o as a double, onset.  An onset's frame is h H
 *   tempo     wbx_clip_tempo computes o on the device and runs wbx_clip_f0's arithmetic over it as a mono F32 range of
 *             `hops` frames: window window_hops, hop step_hops, lags lag_min .. lag_max, threshold; wbx_f0_frame records
 *             whose periods are in hops, bit-equal to that arithmetic on o.  The novelty never visits the host.
 *             bpm = 60 rate / (H period): the caller's division.  The lag range decides the octave, as it does for any
 *             autocorrelation tempo estimate
 * Both calls run on the edits' stream behind wbx_clip_derive's ordering, one edit or measurement at a time, and return
 * when the records are in frames_out.  wbx_onset_info: hops; onsets (the records with onset = 1); launches (2 where there
 * are hops).  wbx_clip_tempo's info is wbx_clip_f0's.
 * Refused before any device call, outputs untouched; the sizes are judged before the clip is looked at, in this order.
 * WBX_ERR_INVALID: an unknown clip; n_frames of 0 or >= 2^31 - 16; hop_frames, floor_power, threshold, delta, w or a outside
 * the ranges above (NaNs included); a NULL frames_out with hops > 0; frames_cap < hops.  WBX_ERR_UNSUPPORTED:
 * hops > wbx_onset_max_hops().  Then the clip — WBX_ERR_UNSUPPORTED: not F32 or more than 2 channels; WBX_ERR_INVALID: a
 * range past the clip.  wbx_clip_tempo judges n_frames, hop_frames, floor_power and the number of hops first, then
 * wbx_f0_check's rules with n = hops (a range without a complete hop: the shape alone), then the clip; zero hops give
 * WBX_OK and no records.
 * Host-only, no device (wbx_onset.h, which a C++ compiler takes alone): wbx_onset_hops (0 for a hop length the call
 * refuses), wbx_onset_check (the argument check above without the clip: its status), wbx_onset_max_hops, wbx_onset_pick
 * (sets frames[h].onset from frames[h].novelty and counts into *onsets, which may be NULL; WBX_ERR_INVALID for pick
 * arguments out of range or NULL frames with hops > 0).
 * wbx_onset_ms: device milliseconds between two events on the edits' stream around the energy pass of the context's last
 * completed onsets or tempo call (layer 1's or layer 2's).  WBX_ERR_INVALID for NULL arguments or when none has completed.
 * For tools/bench_onsets.py; nothing else reads it.
 * Not offered: beat phase or downbeats, a tempo prior against octave errors, sample-accurate onset refinement, detection
 * at render time, unlinked stereo, more than 2 channels. */
typedef struct wbx_onset_frame {        /* 32 bytes */
  double energy;
  double edge_energy;
  double novelty;
  uint32_t onset;
  uint32_t _pad;
} wbx_onset_frame;
typedef struct wbx_onset_info {         /* 24 bytes */
  uint64_t hops;
  uint64_t onsets;
  uint32_t launches;
  uint32_t _pad;
} wbx_onset_info;
uint64_t wbx_onset_hops(uint64_t n_frames, uint32_t hop_frames);
wbx_status wbx_onset_check(uint64_t n_frames, uint32_t hop_frames, double floor_power, double threshold, double delta, uint32_t w,
                           uint32_t a, int has_frames_out, size_t frames_cap);
uint64_t wbx_onset_max_hops(void);
wbx_status wbx_onset_pick(wbx_onset_frame* frames, uint64_t hops, double threshold, double delta, uint32_t w, uint32_t a,
                          uint64_t* onsets);
wbx_status wbx_onset_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_onsets(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                           double floor_power, double threshold, double delta, uint32_t w, uint32_t a,
                           wbx_onset_frame* frames_out, size_t frames_cap, wbx_onset_info* info);
wbx_status wbx_clip_tempo(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                          double floor_power, uint32_t window_hops, uint32_t step_hops, uint32_t lag_min, uint32_t lag_max,
                          double threshold, wbx_f0_frame* frames_out, size_t frames_cap, wbx_f0_info* info);

/* Seeing a clip's spectrum: the power of frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2
 * channels at n_bins frequencies, one row of cells per hop, as a DIRECT transform — ascending dot products of the clip's
 * frames with the rows of a host-built basis that lives in the pool as an ordinary mono F32 clip — without the samples
 * leaving HBM.  No FFT (its rounding depends on its factorisation), no sin and no log on the device: bins may sit at any
 * frequencies (linear, logarithmic for a constant-Q view, semitones for a chromagram, a few bands), each with its own window
 * length, and the cells are reproducible bit for bit.  A MEASUREMENT, like wbx_clip_loudness and wbx_clip_f0: nothing is
 * allocated in the pool and no clip is created.  No reference counterpart.  The arithmetic is part of the interface;
 * tests/spectrum_model.py restates it in numpy, operation for operation, and the cells equal it BIT FOR BIT.  Every operator
 * below is ONE IEEE fp64 operation in the order written; nothing is fused unless stated.
 *   input     channel 0 or 1: d[g] = the channel's fp32 sample; WBX_SPECTRUM_MID: "Tracking a clip's pitch"'s detector as it
 *             is — mono the sample, stereo d = (float)(0.5 * ((double)L + (double)R)).  A sample that is not finite reads as
 *             0 (each channel's before the mid is formed).  Nothing beside the range is ever read
 *   shape     W = window_frames, a multiple of 4 in [32, 8192]; H = hop_frames in [1, 65536]; B = n_bins in [1, 1024] with
 *             B * W <= 2^21.  hops = n >= W ? (n - W) / H + 1 : 0 (wbx_spectrum_hops): only complete frames count, and
 *             hops == 0 is no error.  n in [1, 2^31 - 16)
 *   basis     a resident MONO F32 clip of exactly 2 * B * W frames (wbx_spectrum_basis_frames; 16 MB at most), i-major:
 *             frame (i * B + b) * 2 holds C_b[i], the next frame S_b[i] — consecutive lanes that own consecutive bins read
 *             consecutive words.  The call does not inspect its words: a row with non-finite words gives non-finite or
 *             otherwise unspecified powers in its own bin, and nothing else is affected
 *   cell      for hop h and bin b, from re = im = 0.0, for i = 0 .. W - 1 ascending:
 *             re = re + d[h H + i] * C_b[i];  im = im + d[h H + i] * S_b[i]
 *             (both factors are fp32 values, so each product is exact in fp64 and an fma IS the same thing);
 *             p = (re * re) + (im * im): two rounded products and one rounded sum, NOT fused;  power[h][b] = (float)p
 *   output    hop-major float[hops][B] in host memory.  No sqrt and no log: magnitudes and decibels are the caller's business
 * wbx_spectrum_basis (host-only, no libm: "Converting a clip's sample rate"'s sinpi and I0) writes such a basis into
 * out[2 * B * W]: bin b has frequency freqs[b] in [0, 0.5] cycles per frame and its own window of L_b = lengths[b] frames in
 * [4, W] (lengths NULL: all W), centred in W at offset (W - L_b) / 2 and zero outside.  For j = 0 .. L_b - 1:
 *             w[j] = 1.0 (WBX_WINDOW_RECT); s * s with s = sinpi(((double)j + 0.5) / (double)L) (WBX_WINDOW_HANN, "Stretching a
 *             clip"'s form); I0(beta * sqrt(max(0.0, 1.0 - u * u))) / I0(beta) with u = ((double)(2 j + 1) - (double)L) / (double)L
 *             (WBX_WINDOW_KAISER, kaiser_beta in [0, 20]; ignored by the other kinds);
 *             sum = the ascending fp64 sum of w; wn = w[j] / sum — so a full-scale sine on a bin has power 0.25;
 *             t = freqs[b] * (double)j; t = t - floor(t); C = (float)(wn * sinpi(2.0 * t + 0.5)); S = (float)(0.0 - (wn * sinpi(2.0 * t)))
 *             at i = (W - L_b) / 2 + j.
 * wbx_spectrum_log_freqs (host-only): out[b] = f_min / exp2(0.0 - ((double)b / bins_per_octave)) with "Dynamics of a clip"'s
 * plain-fp64 exp2 — f_min * 2^(b / bins_per_octave) without libm; f_min in (0, 0.5], bins_per_octave positive and finite;
 * what exceeds 0.5 becomes 0.5 and is counted into *clamped (may be NULL).
 * The call runs on the edits' stream behind wbx_clip_derive's ordering, one edit or measurement at a time, in launches of
 * at most wbx_spectrum_launch_hops(window_frames, n_bins) hops — whole thirty-twos such that hops * W * 2 B stays within
 * wbx_spectrum_launch_terms() and the device-side stage for a launch's cells within 2^22 cells — each launch's cells copied
 * out before the next; it returns when power_out holds all of them.  info (may be NULL): hops; bins; launches.
 * Refused before any device call, power_out and info untouched; the sizes are judged before the clips are looked at, in this
 * order.  WBX_ERR_INVALID: an unknown clip; n_frames of 0 or >= 2^31 - 16; a channel that is none of the three; a window,
 * bin count, product or hop outside the ranges above; a NULL power_out with hops > 0; cells_cap < hops * B.
 * WBX_ERR_UNSUPPORTED: hops > 2^20; hops * B > wbx_spectrum_max_cells() (2^25: 128 MB at the host).  Then the source —
 * WBX_ERR_UNSUPPORTED: not F32 or more than 2 channels; WBX_ERR_INVALID: channel 1 of a mono clip, a range past the clip.
 * Then the basis — WBX_ERR_INVALID: an unknown clip; WBX_ERR_UNSUPPORTED: not F32 or not mono; WBX_ERR_INVALID: a length
 * other than 2 * B * W frames.
 * Host-only, no device (wbx_spectrum.h, which a C++ compiler takes alone): wbx_spectrum_hops (0 for a window or hop the
 * call refuses), wbx_spectrum_check (the argument check above without the clips: its status), wbx_spectrum_max_cells,
 * wbx_spectrum_launch_terms, wbx_spectrum_launch_hops and wbx_spectrum_basis_frames (0 for a shape the call refuses),
 * wbx_spectrum_basis and wbx_spectrum_log_freqs (WBX_ERR_INVALID for arguments outside the ranges above, NaNs and NULL
 * included; out untouched).
 * wbx_spectrum_ms: device milliseconds of the launches of the context's last completed spectrum call (layer 1's or layer
 * 2's), each between two events on the edits' stream, added up; the copies between them do not count.  WBX_ERR_INVALID for
 * NULL arguments or when none has completed.  For tools/bench_spectrum.py; nothing else reads it.
 * Not offered: phase output or complex cells, a reassigned or phase-vocoder spectrum, anything with an FFT, a spectrum at
 * render time or on live tracks, more than 2 channels, per-channel spectra in one call. */
#define WBX_SPECTRUM_MID 2u
enum { WBX_WINDOW_RECT = 0, WBX_WINDOW_HANN = 1, WBX_WINDOW_KAISER = 2 };
typedef struct wbx_spectrum_info {      /* 16 bytes */
  uint64_t hops;
  uint32_t bins;
  uint32_t launches;
} wbx_spectrum_info;
uint64_t wbx_spectrum_hops(uint64_t n_frames, uint32_t window_frames, uint32_t hop_frames);
wbx_status wbx_spectrum_check(uint64_t n_frames, uint32_t channel, uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames,
                              int has_power_out, size_t cells_cap);
uint64_t wbx_spectrum_max_cells(void);
uint64_t wbx_spectrum_launch_terms(void);
uint32_t wbx_spectrum_launch_hops(uint32_t window_frames, uint32_t n_bins);
uint64_t wbx_spectrum_basis_frames(uint32_t window_frames, uint32_t n_bins);
wbx_status wbx_spectrum_basis(uint32_t window_frames, uint32_t n_bins, const double* freqs, const uint32_t* lengths,
                              int window_kind, double kaiser_beta, float* out);
wbx_status wbx_spectrum_log_freqs(double f_min, double bins_per_octave, uint32_t n_bins, double* out, uint32_t* clamped);
wbx_status wbx_spectrum_ms(wbx_ctx* ctx, double* out);
wbx_status wbx_clip_spectrum(wbx_ctx* ctx, uint32_t clip, uint64_t first_frame, uint64_t n_frames, uint32_t channel,
                             uint32_t basis_clip, uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames, float* power_out,
                             size_t cells_cap, wbx_spectrum_info* info);

/* Waveform peak mip-maps of a resident clip: WaveformVisual::create + summarize_for_mipmaps_impl<T>
 * (src/gfx/waveform_visual.cpp:9-246).  quality: 0 = Low (int8_t), 1 = High (int16_t) (waveform_visual.h:11-14).
 * Level l holds, per channel, mip_data_count(l) values = ordered (first, second) min/max pairs of chunks of
 * 2^(2l+1) samples; layout of a level [channels][mip_data_count] like the reference's upload buffer (:206-226).
 * Formats: I16, I32, F32 (the reference's switch has no other case). */
uint32_t wbx_mip_levels(uint64_t frames);                          /* number of levels (:195 while count/4^l > 64) */
uint64_t wbx_mip_data_count(uint64_t frames, uint32_t level);      /* :197-199 */
wbx_status wbx_clip_build_mipmaps(wbx_ctx* ctx, uint32_t clip, int quality);
wbx_status wbx_clip_fetch_mipmap(wbx_ctx* ctx, uint32_t clip, uint32_t level, void* dst);
/* device pointer + element count of a level (what WaveformMipmap{data, count} holds for the renderer) */
wbx_status wbx_clip_mipmap_device(wbx_ctx* ctx, uint32_t clip, uint32_t level, const void** data, uint64_t* count);

/* Track -> sub-bus routing (extension of the reference, which has no buses: SURVEY §8(a) A13).
 * track_bus[t] in [0, n_buses) or -1 (straight to master).  NULL / n_buses 0 = reference behaviour. */
wbx_status wbx_set_routing(wbx_ctx* ctx, uint32_t n_tracks, const int32_t* track_bus, uint32_t n_buses);

/* How a render of n_blocks blocks is summed, with the routing as it stands (after the last render / wbx_set_routing):
 * workgroup-level groups per block, the longest of them, and whether that IS the reference's order (every member list —
 * all tracks, or the tracks of each bus — added sequentially by one workgroup: engine.cpp:1600-1617, bit-exact master). */
wbx_status wbx_render_order(wbx_ctx* ctx, uint32_t n_blocks, uint32_t* n_groups, uint32_t* longest_group, int* reference_order);
/* PCI bus id ("0000:05:00.0") and marketing / arch name of the ctx's device (multi-GPU hosts log which rank got which). */
wbx_status wbx_device_info(wbx_ctx* ctx, char* pci_bus_id, size_t n_pci, char* name, size_t n_name);

/* Mix K blocks of n_tracks tracks.  segs[] holds the Sampler::stream calls grouped by (block, track):
 * those of (b, t) are segs[seg_offsets[b*n_tracks+t] .. seg_offsets[b*n_tracks+t+1]).  gains[(b*n_tracks+t)*2+c]
 * = fl(volume*pan_coeffs[c]) (0 when muted), the factor of track.cpp:728-731.  Asynchronous. */
wbx_status wbx_submit(wbx_ctx* ctx, uint32_t n_blocks, uint32_t n_tracks, const wbx_segment* segs,
                      const uint32_t* seg_offsets, const float* gains);

/* Results of the last submit (blocks until done).  Any pointer may be NULL.
 *  master_planar[c] : K*F floats, block after block (the AudioBuffer the audio thread hands to process)
 *  peaks            : [K][N][C]  max|x| per track/channel/block (VUMeter::push_samples, vu_meter.h:20-25); NaN samples
 *                     are ignored (the reference's running maximum restarts after a NaN, an order-dependent result)
 *  buses            : [K][n_buses][C][F] bus sums */
wbx_status wbx_fetch(wbx_ctx* ctx, float* const* master_planar, float* peaks, float* buses);
wbx_status wbx_fetch_interleaved(wbx_ctx* ctx, int out_format, void* dst);  /* K*F*C interleaved samples */
/* Let later submits / renders leave their master as interleaved samples of a device format (WBX_OUT_*; 0 = planar fp32
 * again): the conversion of core/audio_format_conv.cpp:5-91 becomes the epilogue of the sum kernel — no separate
 * conversion launch, no planar master in between.  The master target (the ctx's own buffer or wbx_set_master_target's,
 * then at least K*F*C samples of the format) holds [K*F][C] samples, packed 24-bit as the reference writes it (see
 * WBX_OUT_I24).  wbx_fetch_interleaved of the same format is then a plain copy; wbx_fetch's planar master is not
 * available.  Not with a multi-GPU exchange (partial masters stay planar fp32). */
wbx_status wbx_set_master_format(wbx_ctx* ctx, int out_format);
wbx_status wbx_sync(wbx_ctx* ctx);
/* Waits like wbx_sync and reports what no other call may have had the chance to: a render of >= 1024 blocks that adds in
 * the reference's order as chained 128-track pieces checks every hand-over between its workgroups, and a failed one makes
 * that render's master INVALID (WBX_ERR_DEVICE; later renders walk whole member lists instead).  wbx_fetch,
 * wbx_fetch_interleaved, wbx_engine_process, wbx_engine_fetch_plan and wbx_dist_sync return that status themselves; a
 * host that reads a caller-owned master target (wbx_set_master_target) directly — it never fetches — must call this
 * (or one of those) before it trusts the buffer.  The failure is latched: every render since the last report counts.
 * Replaces nothing in the reference (engine.cpp:1600-1617 is one thread, one order). */
wbx_status wbx_render_status(wbx_ctx* ctx);
/* Order `stream` (a hipStream_t; NULL = the ctx stream) after every kernel that writes the results of the last
 * submit / render (master, bus sums, peaks).  The sum of a render runs on a stream of its own beside the next mix:
 * work the CALLER enqueues that reads a caller-owned master target (wbx_set_master_target) — a collective, a copy,
 * an own kernel — must be ordered with this call first; wbx_fetch*, wbx_sync, wbx_partial_master, wbx_finalize_master*
 * and the wbx_dist_* calls do it themselves.  Device-side ordering only: the host does not block. */
wbx_status wbx_master_ready(wbx_ctx* ctx, void* stream);

/* Multi-GPU: the un-clamped partial master of the last submit, on the device, [K][C][F] fp32 ... */
wbx_status wbx_partial_master(wbx_ctx* ctx, void** device_ptr, size_t* n_floats);
/* ... and, on the root after the RCCL reduce, the clamp of engine.cpp:1627-1636 over a device buffer.
 * `stream`: hipStream_t to launch on (e.g. the stream that waited for the collective), NULL = the ctx stream. */
wbx_status wbx_finalize_master(wbx_ctx* ctx, void* device_partial, uint32_t n_blocks, int clamp, void* stream);
/* Out of place: clamp (or just move) the reduced master into `dst`, which may be device memory or pinned,
 * device-mapped host memory — the final master then leaves the GPU as the kernel's own stores. */
wbx_status wbx_finalize_master_into(wbx_ctx* ctx, const void* device_partial, void* dst, uint32_t n_blocks, int clamp,
                                    void* stream);
wbx_status wbx_set_clamp(wbx_ctx* ctx, int clamp_on_submit); /* 0: leave the master un-clamped (shard mode) */
/* Write the master of later submits/renders into a caller-owned DEVICE buffer of at least
 * max_blocks*C*F floats (e.g. the send buffer of the RCCL reduce); NULL restores the ctx-owned one. */
wbx_status wbx_set_master_target(wbx_ctx* ctx, void* device_buffer);
/* Start the master of later submits / renders from a running sum instead of the cleared buffer: `device_buffer`
 * ([max_blocks][C][F] floats, device memory or pinned device-mapped host memory, 16-byte aligned) holds the UN-clamped
 * master of the engine that owns the tracks BEFORE this one's in the session's track order; the first group in summation
 * order continues from it, so that a session split over several engines (several GPUs: WBX_DIST_CHAIN does exactly this
 * over RCCL; or one GPU, to go beyond max_tracks) is added in the reference's strictly sequential order
 * (engine.cpp:1600-1617) across the split.  NULL restores the cleared start.  Not with sub-buses. */
wbx_status wbx_set_master_init(wbx_ctx* ctx, const void* device_buffer);

/* ---- multi-GPU: tracks sharded over one process per GPU, ONE exchange per render ---------------
 * The reference has no distributed code; this is the path's only exchange step: every rank mixes its own contiguous
 * track range into an un-clamped partial master, the partials are summed onto rank 0 over RCCL (xGMI), and the clamp
 * of engine.cpp:1627-1636 runs there, after the sum.  Protocol per rank:
 *     wbx_shard_tracks(N, world, rank, &first, &count);          // which tracks this rank builds its session from
 *     rank 0: wbx_dist_new_id(&id) and hand the 128 bytes to the other ranks (file, socket, MPI, ...)
 *     wbx_dist_init(ctx, &id, rank, world, WBX_DIST_REDUCE);      // collective: returns when every rank has called
 *     loop: wbx_engine_render / wbx_submit;  wbx_dist_exchange(ctx, dst);      // dst: rank 0 only
 *     wbx_dist_sync(ctx);  ...  wbx_dist_shutdown(ctx);
 * After wbx_dist_init the ctx writes its (un-clamped) masters into an internal ring of three device buffers, so up
 * to two further renders may be issued while an exchange is in flight; nothing in the loop blocks the host.
 * WBX_DIST_REDUCE: one ncclReduce(sum) — RCCL's summation order is implementation-defined (inside the 1e-6 RMS budget).
 * WBX_DIST_ORDERED: ncclGather + a fixed-order add on the root, (((0 + p0) + p1) + ...) in rank = track order:
 * bit-reproducible on any topology (SURVEY §7 hard part 8).  Both add SHARD sums, which is not the reference's
 * track-after-track association: at 32768 tracks the difference leaves the 1e-6 RMS budget once the master runs at
 * mix-bus level (profiles/r03_level_probe.txt).
 * WBX_DIST_CHAIN: the reference's order across GPUs — rank g receives the running un-clamped master of rank g-1, its mix
 * continues that sum with its own tracks, rank g+1 gets the result; the LAST rank clamps and holds the result
 * (wbx_dist_result_rank; its wbx_dist_exchange takes `dst`).  With renders of >= 1024 blocks (whole-list walks) the
 * master is bit-identical to a single engine over all tracks.  The ranks form a pipeline over consecutive renders: same
 * throughput, a render's latency grows with the world size.  Not with sub-buses.
 * wbx_dist_init fails with WBX_ERR_FAILED when the collective start-up does not complete within
 * WBX_DIST_INIT_TIMEOUT_S seconds (environment, default 60, 0 = wait for ever). */
#define WBX_DIST_ID_BYTES 128
typedef struct wbx_dist_id {
  char bytes[WBX_DIST_ID_BYTES];
} wbx_dist_id;
enum { WBX_DIST_REDUCE = 0, WBX_DIST_ORDERED = 1, WBX_DIST_CHAIN = 2 };
void wbx_shard_tracks(uint32_t n_tracks, uint32_t world, uint32_t rank, uint32_t* first, uint32_t* count);
wbx_status wbx_dist_new_id(wbx_dist_id* out);
wbx_status wbx_dist_init(wbx_ctx* ctx, const wbx_dist_id* id, uint32_t rank, uint32_t world, int mode);
wbx_status wbx_dist_info(wbx_ctx* ctx, uint32_t* rank, uint32_t* world, int* mode);
wbx_status wbx_dist_result_rank(wbx_ctx* ctx, uint32_t* rank);   /* 0 (reduce / ordered) or world - 1 (chain) */
/* dst (the result rank only): [K][C][F] floats, device memory or pinned device-mapped host memory, 16-byte aligned */
wbx_status wbx_dist_exchange(wbx_ctx* ctx, void* dst);
/* average ms one exchange took on its own stream, over the exchanges completed so far (after wbx_dist_sync) */
wbx_status wbx_dist_exchange_time(wbx_ctx* ctx, double* ms_avg, uint64_t* n_exchanges);
/* every rank hands in `bytes` (<= 4096) bytes of host memory and gets all ranks' bytes in rank order; also a barrier */
wbx_status wbx_dist_allgather(wbx_ctx* ctx, const void* send, void* recv, size_t bytes);
wbx_status wbx_dist_sync(wbx_ctx* ctx);                  /* host waits for the renders and exchanges issued so far */
wbx_status wbx_dist_barrier(wbx_ctx* ctx);               /* all ranks */
wbx_status wbx_dist_max(wbx_ctx* ctx, double* value);    /* max over all ranks, in place (also a barrier) */
wbx_status wbx_dist_shutdown(wbx_ctx* ctx);

/* Render-ahead bound for asynchronous hosts: call after each submit / render; the host waits until the render issued
 * `max_ahead` (1..63) calls earlier has left the main stream.  Far deeper queues stall inside the HIP runtime. */
wbx_status wbx_pace(wbx_ctx* ctx, uint32_t max_ahead);

/* Pinned, device-mapped host memory (hipHostMalloc): a destination for wbx_set_master_target / wbx_dist_exchange /
 * wbx_finalize_master_into that the GPU writes with plain stores. */
wbx_status wbx_host_alloc(size_t bytes, void** out);
wbx_status wbx_host_free(void* p);

/* Timing of the dominant kernel (HIP events on the ctx stream): average ms per launch since reset. */
wbx_status wbx_kernel_time(wbx_ctx* ctx, int reset, double* mix_ms_avg, uint64_t* mix_launches);
/* Average ms from the end of the mix kernel to the end of the sum kernel over the same launches (launch gap + the
 * group/bus/master sum including its stores to a host-resident master target); read before resetting. */
wbx_status wbx_tail_time(wbx_ctx* ctx, double* tail_ms_avg);
/* ... and the mean idle time between two consecutive mix launches (end time stamp of one to start time stamp of the next, over
 * the pairs timed since the last reset of wbx_kernel_time; *gaps: how many) — what a step spends outside its dominant kernel
 * while renders run back to back. */
wbx_status wbx_gap_time(wbx_ctx* ctx, double* gap_ms_avg, uint64_t* gaps);
/* The template instance of the dominant kernel that the last render launched, as rocprofv3 prints it
 * ("wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 128>"); "" before the first render. */
const char* wbx_kernel_name(wbx_ctx* ctx);
/* The one resampling ratio the last render's mix was told about (MixArgs::uniform_speed: every linearly resampled row of the
 * render plays at exactly this Sampler::playback_speed_, sampler.h:24 — the hoisted-product chunk modes), 0.0 when the
 * session holds more than one ratio, none, or the plan came through layer 1.  Introspection, like wbx_kernel_name. */
double wbx_render_uniform_speed(wbx_ctx* ctx);
/* What wbx_create's probe found: the number of XCDs a launch's workgroup ids are dealt to round-robin (8 on MI355X; 4 / 2 / 1 in
 * other partition modes) — the layout the chained 128-track pieces of long renders and the segmented sequencer rest on — or 0:
 * not such a layout; the context then walks whole member lists and plans by one lane per track (same results).  Introspection. */
uint32_t wbx_xcd_count(wbx_ctx* ctx);

/* ---- layer 2: the engine surface -----------------------------------------------------------
 * Mirrors wb::Engine / wb::Track (src/engine/engine.h, track.h).  Beats are doubles as in the
 * reference; all seek / sample-index math is done in the reference's order in fp64/int64. */
wbx_status wbx_engine_create(const wbx_config* cfg, wbx_engine** out);  /* + set_audio_channel_config, engine.cpp:43-57 */
void wbx_engine_destroy(wbx_engine* e);
/* Engine::set_audio_channel_config (engine.cpp:43-57) on a live engine — a new block size, channel count or device
 * rate (the audio backend was reconfigured).  Tracks, clips, samples and the transport stay. */
wbx_status wbx_engine_set_audio_channel_config(wbx_engine* e, uint32_t output_channels, uint32_t buffer_size,
                                               uint32_t sample_rate);
/* message of the last failed wbx_engine_* / wbx_track_* call made by the CALLING thread */
const char* wbx_engine_last_error(const wbx_engine* e);
wbx_ctx* wbx_engine_ctx(wbx_engine* e);

wbx_status wbx_engine_set_bpm(wbx_engine* e, double bpm);                       /* engine.cpp:24-30 */
wbx_status wbx_engine_set_playhead_position(wbx_engine* e, double beat);       /* engine.cpp:32-41 */
wbx_status wbx_engine_add_track(wbx_engine* e, uint32_t* track_out);           /* engine.cpp:200-208 */
wbx_status wbx_engine_set_buses(wbx_engine* e, uint32_t n_buses);              /* extension A13 */
wbx_status wbx_track_set_volume(wbx_engine* e, uint32_t track, float db);      /* track.cpp:47-57 */
wbx_status wbx_track_set_pan(wbx_engine* e, uint32_t track, float pan);        /* track.cpp:59-68 */
wbx_status wbx_track_set_mute(wbx_engine* e, uint32_t track, int mute);        /* track.cpp:70-79 */
/* Engine::delete_track (engine.cpp:210-218), move_track (:228-243; the order is the summation order),
 * solo_track (:245-262; toggles the UI solo flag and mutes / unmutes the other tracks through set_mute).
 * Track indices above a deleted / between moved slots shift exactly as the reference's vector does. */
wbx_status wbx_engine_delete_track(wbx_engine* e, uint32_t slot);
wbx_status wbx_engine_clear_all(wbx_engine* e);                       /* Engine::clear_all, engine.cpp:59-66 */
wbx_status wbx_engine_move_track(wbx_engine* e, uint32_t from_slot, uint32_t to_slot);
wbx_status wbx_engine_solo_track(wbx_engine* e, uint32_t slot);
/* extension A13: bus < 0 or >= the configured number of buses routes the track straight into the master */
wbx_status wbx_track_set_bus(wbx_engine* e, uint32_t track, int32_t bus);

/* Effect slot of a track (Track::plugin_instance, track.h:124; call site track.cpp:645-662; attach / detach
 * Engine::add_plugin_to_track / delete_plugin_from_track, engine.h:227-229).  The reference's effects are third-party
 * VST3 binaries whose arithmetic is not part of this path: the slot is kept in the boundary so that a host can
 * describe such a session, but nothing is processed through it — attaching a plugin returns WBX_ERR_UNIMPLEMENTED
 * (PluginResult::Unimplemented) and leaves the slot empty; detaching and querying always succeed.
 * wbx_plugin_process_info has the fields of PluginProcessInfo (plughost/plugin_interface.h:77-90) with the
 * AudioBuffer<float>* members flattened to planar channel arrays. */
typedef struct wbx_plugin_process_info {
  uint32_t sample_count;
  uint32_t input_buffer_count;
  uint32_t output_buffer_count;
  uint32_t n_channels;
  float* const* input_buffer;       /* [n_channels][sample_count] */
  float* const* output_buffer;
  void* input_event_list;           /* MidiEventList*, unused (MIDI is out of scope) */
  double sample_rate;
  double tempo;
  double project_time_in_ppq;
  int64_t project_time_in_samples;
  int32_t playing;
} wbx_plugin_process_info;
typedef struct wbx_plugin {
  void* userdata;
  int (*process)(void* userdata, wbx_plugin_process_info* info);   /* PluginInterface::process, :146; returns a status */
} wbx_plugin;
wbx_status wbx_engine_add_plugin_to_track(wbx_engine* e, uint32_t track, const wbx_plugin* plugin);
wbx_status wbx_engine_delete_plugin_from_track(wbx_engine* e, uint32_t track);
wbx_status wbx_track_get_plugin(wbx_engine* e, uint32_t track, const wbx_plugin** plugin_out);   /* always NULL today */
/* Sample assets (SampleAsset, engine/assets_table.h:22-35): upload once, reference by id from clips. */
wbx_status wbx_engine_add_sample(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames,
                                 const void* const* planar, uint32_t* sample_out);
/* the same from interleaved decoder output (wbx_clip_upload_interleaved) */
wbx_status wbx_engine_add_sample_interleaved(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate,
                                             uint64_t frames, const void* interleaved, uint32_t* sample_id);
wbx_status wbx_engine_add_sample_synth(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate,
                                       uint64_t frames, uint64_t seed, uint32_t key_track, float amp,
                                       uint32_t* sample_out);
/* drop a sample no clip names any more (under the editor lock: use this, not wbx_clip_free, on an engine's pool) */
wbx_status wbx_engine_delete_sample(wbx_engine* e, uint32_t sample);
/* Engine::add_audio_clip (engine.cpp:293-309 -> add_to_cliplist :409-461).  A clip that overlaps existing ones
 * trims / splits / deletes them through reserve_track_region (engine.cpp:478-569), like the reference. */
wbx_status wbx_engine_add_audio_clip(wbx_engine* e, uint32_t track, double min_time, double max_time,
                                     double start_offset, uint32_t sample, double speed, float gain);

/* Clip edits (UI thread in the reference).  `clip` is the index in the track's clip list, which is kept sorted
 * by min_time (Track::update_clip_ordering, track.cpp:159-180): indices change after every edit. */
typedef struct wbx_clip_info {
  double min_time, max_time;   /* beats */
  double start_offset;         /* samples */
  double speed;                /* AudioClip::speed */
  float gain;                  /* AudioClip::gain */
  uint32_t sample;
} wbx_clip_info;
wbx_status wbx_engine_move_clip(wbx_engine* e, uint32_t track, uint32_t clip, double relative_pos);   /* engine.cpp:346-363 */
wbx_status wbx_engine_resize_clip(wbx_engine* e, uint32_t track, uint32_t clip, double relative_pos, double resize_limit,
                                  double min_length, int left_side, int shift, int stretch);          /* engine.cpp:365-398 */
wbx_status wbx_engine_delete_clip(wbx_engine* e, uint32_t track, uint32_t clip);                       /* engine.cpp:400-407 */
wbx_status wbx_engine_delete_region(wbx_engine* e, uint32_t track, double min_time, double max_time);  /* engine.cpp:463-475 */
wbx_status wbx_engine_set_clip_gain(wbx_engine* e, uint32_t track, uint32_t clip, float gain);         /* engine.cpp:1460-1464 */
wbx_status wbx_engine_clip_count(wbx_engine* e, uint32_t track, uint32_t* count);
wbx_status wbx_engine_get_clip(wbx_engine* e, uint32_t track, uint32_t clip, wbx_clip_info* out);
/* The clip placement arithmetic by itself (src/engine/clip_edit.h:10-150; audio clips), fp64, host-only. */
void wbx_calc_move_clip(double clip_min, double clip_max, double relative_pos, double min_move, double* new_min,
                        double* new_max);
void wbx_calc_resize_clip(double clip_min, double clip_max, double clip_start_offset, double clip_speed, double sample_rate,
                          double sample_count, double relative_pos, double resize_limit, double min_length,
                          double min_resize_pos, double beat_duration, int is_min, int shift, int stretch,
                          int clamp_at_resize_pos, double* out_min, double* out_max, double* out_start_offset,
                          double* out_speed);
double wbx_calc_clip_shift(double start_offset, double relative_pos, double beat_duration, double sample_rate);
double wbx_shift_clip_content(double start_offset, double speed, double sample_rate, double relative_pos,
                              double beat_duration);
wbx_status wbx_engine_play(wbx_engine* e);                                      /* engine.cpp:68-80 */
wbx_status wbx_engine_stop(wbx_engine* e);                                      /* engine.cpp:82-93 */

/* Engine::process (engine.cpp:1576-1654): one block into out_planar[c][0..F). */
wbx_status wbx_engine_process(wbx_engine* e, float* const* out_planar);
/* Engine::process and the audio back end's conversion to the device's sample format in one call (the call site
 * audio_io_pulseaudio.cpp:419-461: process(), then output_buffer.interleave_samples_to(buffer, 0, n, format) ->
 * core/audio_format_conv.cpp:5-91): dst receives the block as F*C interleaved samples of `out_format` (WBX_OUT_*), the
 * conversion running as the epilogue of the sum kernel — one launch fewer than process + wbx_fetch_interleaved. */
wbx_status wbx_engine_process_interleaved(wbx_engine* e, int out_format, void* dst);
/* Engine::process(input_buffer, output_buffer, sample_rate) with its input buffer (engine.cpp:1576, the recorder tap
 * :1638-1649): in_planar[c][0..F) for c < n_in_channels.  Without a take running the input is not read (no monitoring:
 * engine.cpp:1625 leaves it out of the master); wbx_engine_process / _interleaved during a take record silence, and so does
 * a call whose n_in_channels is below the highest recorded channel + 1: the whole block is silence in every take, the
 * channels the short buffer does hold included (WBX_RECORD_SILENCE). */
wbx_status wbx_engine_process_in(wbx_engine* e, const float* const* in_planar, uint32_t n_in_channels, float* const* out_planar);
wbx_status wbx_engine_process_interleaved_in(wbx_engine* e, const float* const* in_planar, uint32_t n_in_channels,
                                             int out_format, void* dst);
/* K consecutive blocks in one device pass (render-ahead / offline): sequencing, mixing, summing and
 * clamping all on the device.  Asynchronous; results via wbx_fetch(wbx_engine_ctx(e), ...).
 * Refused (WBX_ERR_UNSUPPORTED) while recording. */
wbx_status wbx_engine_render(wbx_engine* e, uint32_t n_blocks);

/* ---- recording: Engine::record / stop_record / arm_track_recording / set_track_input (engine.cpp:95-200),
 * Track::prepare_record / stop_record (track.cpp:234-246).  Takes live in HBM from the first frame: every played block's
 * input is captured on the device into chunks of the clip pool, and stop_record gathers each take into one clip.
 * TrackInputType (track_input.h:10-15); MIDI input is refused (WBX_ERR_UNSUPPORTED). */
enum { WBX_INPUT_NONE = 0, WBX_INPUT_MIDI = 1, WBX_INPUT_EXTERNAL_STEREO = 2, WBX_INPUT_EXTERNAL_MONO = 3 };
/* a take's status bits (wbx_record_info.status) */
enum {
  WBX_RECORD_OVERFLOW = 1,   /* some block found no room (or its staging slot busy): its frames are silence in the take */
  WBX_RECORD_SILENCE = 2     /* some block came through a process call without (all of) the recorded input channels */
};
/* the input_channels argument of Engine::set_audio_channel_config (engine.cpp:43-48; num_input_channels): the highest
 * input channel a track may record is input_channels - 1 (checked at wbx_engine_record).  Default 0. */
wbx_status wbx_engine_set_input_channels(wbx_engine* e, uint32_t input_channels);
/* Engine::set_track_input (engine.cpp:145-198).  ExternalMono index i records input channel i, ExternalStereo index i
 * channels 2i and 2i+1 (engine.cpp:1642-1643); several tracks may share an input, each gets its own copy of the take.
 * Changes during a take take effect at the next wbx_engine_record. */
wbx_status wbx_track_set_input(wbx_engine* e, uint32_t track, int type, uint32_t index, int armed);
wbx_status wbx_engine_arm_track_recording(wbx_engine* e, uint32_t track, int armed);   /* engine.cpp:140-143 */
/* Engine::record (engine.cpp:95-105): nothing while recording and playing; otherwise recording starts and play() runs —
 * every armed track with an input starts a take at playhead_start (the transport restarts from there also when it was
 * already running, as in the reference).  WBX_ERR_UNSUPPORTED on a redirected master / multi-GPU context,
 * WBX_ERR_INVALID when an armed track's input lies past wbx_engine_set_input_channels. */
wbx_status wbx_engine_record(wbx_engine* e);
/* Engine::stop_record (engine.cpp:107-138): each take becomes an F32 sample at the session rate (1 or 2 channels, the
 * frames written) and a clip add_audio_clip(track, record_min_time, record_max_time, 0.0, sample, speed 1.0, gain 1.0f)
 * puts on its track (overlap trimming included); a take of no frames adds nothing.  Playback continues.  Returns
 * WBX_ERR_OVERFLOW (clips still made) when a take has WBX_RECORD_OVERFLOW.  wbx_engine_stop calls it first
 * (engine.cpp:83-84).  Deleting a recording track (or wbx_engine_clear_all) discards its take: its storage goes back to the
 * clip pool with the delete (wbx_clip_pool_stats), no later block is written into it, and stop_record makes no clip of it. */
wbx_status wbx_engine_stop_record(wbx_engine* e);
wbx_status wbx_engine_is_recording(wbx_engine* e, int* recording);
typedef struct wbx_record_info {
  int32_t recording;          /* Track::input_attr.recording */
  int32_t armed;              /* input_attr.armed */
  int32_t input_type;         /* WBX_INPUT_* */
  uint32_t input_index;
  double min_time, max_time;  /* record_min_time / record_max_time (track.h:100-101; 0 when not recording) */
  uint64_t frames;            /* frames written into the track's latest take (running or finished) */
  uint32_t status;            /* WBX_RECORD_* of that take */
  uint32_t _pad;
} wbx_record_info;
wbx_status wbx_engine_record_info(wbx_engine* e, uint32_t track, wbx_record_info* out);
/* Take storage: chunks of `frames` frames (default 65536, audio_record_chunk_size / 4, engine.h:36); the engine's
 * recorder thread keeps `spare_chunks` (default 2) chunks ahead of every take's write position (wbx_engine_record
 * reserves the first ones).  Not while recording. */
wbx_status wbx_engine_set_record_chunk(wbx_engine* e, uint32_t frames, uint32_t spare_chunks);
/* ---- bouncing: tracks, buses and the master into GPU-resident clips (stems, freeze, export; no reference counterpart —
 * its export dialog, ui/export_audio_dlg.cpp / engine/export_prop.h, has nothing behind it).
 * Render [min_time, max_time) (beats) offline and keep n_src signals of it as F32 samples of the session rate and channel
 * count in the engine's clip pool; samples_out[i] is an engine sample id usable in wbx_engine_add_audio_clip,
 * wbx_clip_download, wbx_clip_build_mipmaps, wbx_engine_delete_sample.  No host copy of the audio is made anywhere.
 *   length    n_frames = (uint64_t)beat_to_samples(max_time - min_time, sample_rate, beat_duration) (core_math.h:209-212,
 *             truncated as engine.cpp:1583 does) at the tempo in force at the call; ceil(n_frames / F) blocks are rendered,
 *             the frames of the last block past n_frames are dropped; every sample has exactly n_frames frames (*frames_out,
 *             may be NULL) plus the pool's 16 zero frames of padding
 *   rendered  is, by definition, what   wbx_engine_set_playhead_position(min_time), wbx_engine_play, K blocks,
 *             wbx_engine_stop, wbx_engine_set_playhead_position(the playhead before the call)   renders; the transport,
 *             sampler and sequencer state, parameter rings and edit count afterwards are what that sequence leaves, and the
 *             blocks of a bounce count into wbx_engine_levels like those of any render.  More blocks than
 *             wbx_config.max_blocks are rendered in consecutive passes whose sampler state continues, like consecutive
 *             wbx_engine_render calls; the samples do not depend on where the passes are cut
 *   sources   WBX_BOUNCE_TRACK, post-fader: the block buffer Track::process leaves — the stream calls summed in order
 *             (sampler.cpp:56,152), times fl(volume * pan_coeffs[c]) (track.cpp:728-731; 0 when muted: a negative sample
 *             becomes -0.0f as in the reference); pre-fader: the same buffer before that multiplication.  WBX_BOUNCE_BUS:
 *             the bus sum as wbx_fetch reports it.  WBX_BOUNCE_MASTER (index 0): the master as wbx_fetch reports it,
 *             clamped.  The same signal may be named more than once; order and duplicates of src[] are kept
 *   refusals  (nothing published, transport untouched, wbx_clip_pool_stats unchanged)  WBX_ERR_UNSUPPORTED while playing or
 *             recording, on a redirected master (wbx_set_master_target, wbx_set_master_init; wbx_set_master_format when the
 *             master is a source) or a multi-GPU context, and for a range of 2^31-16 frames or more; WBX_ERR_INVALID for n_src == 0, max_time <= min_time, a range of no
 *             frame, a track or bus index out of range, a tap on a bus or the master; the pool's own status (WBX_ERR_OOM,
 *             WBX_ERR_DEVICE) when it cannot hold n_src more samples — what had been allocated goes back to the pool
 *             (bytes_live as before; slabs the pool took from the driver for it stay reserved, empty, until the context
 *             goes — under wbx_clip_pool_limit none is taken); WBX_ERR_OVERFLOW when the pool's 2^24 sample ids would run out
 * Takes the editor lock for its duration, like every other edit call.  A device error in the middle of the passes returns
 * that error with the transport stopped at the playhead before the call and nothing published. */
enum { WBX_BOUNCE_TRACK = 0, WBX_BOUNCE_BUS = 1, WBX_BOUNCE_MASTER = 2 };
enum { WBX_TAP_POST_FADER = 0, WBX_TAP_PRE_FADER = 1 };   /* tracks only */
typedef struct wbx_bounce_source {
  int32_t kind;      /* WBX_BOUNCE_* */
  uint32_t index;    /* track or bus; 0 for the master */
  int32_t tap;       /* WBX_TAP_* */
  uint32_t _pad;
} wbx_bounce_source;
wbx_status wbx_engine_bounce(wbx_engine* e, double min_time, double max_time, const wbx_bounce_source* src, uint32_t n_src,
                             uint32_t* samples_out, uint64_t* frames_out);
/* wbx_clip_export of an engine sample (a take's, a bounce's, an uploaded F32 sample), for the editing thread — the audio
 * thread may keep calling wbx_engine_process* meanwhile, playing or recording: an export touches no transport state.  The
 * editor lock is held only to validate the sample, pin it and order the export's stream behind the work enqueued so
 * far; never across a device wait or a chunk copy (the rule of wbx_engine_levels).  While the export is in flight
 * wbx_engine_delete_sample refuses that sample (WBX_ERR_UNSUPPORTED, "sample is being exported"); the pin is dropped
 * when the call returns.  (wbx_engine_clear_all removes tracks, not samples, and needs no such check.)  Allowed on a
 * redirected master and a multi-GPU context: it reads the local clip pool only.  Arguments, refusals and results are
 * wbx_clip_export's. */
wbx_status wbx_engine_export_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, int out_format,
                                    uint32_t flags, void* dst, wbx_export_stats* stats);
/* wbx_clip_measure / wbx_clip_derive of engine samples, for the editing thread, under wbx_engine_export_sample's rules: the
 * audio thread may keep calling wbx_engine_process* meanwhile, playing or recording; the calls touch no transport state
 * and do not count as edits of the session.  The editor lock is held only to validate the sample, copy its storage
 * description out, set or clear the pin, order the edit's stream and register the new sample; never across a device
 * wait.  While a call is in flight wbx_engine_delete_sample refuses its source (WBX_ERR_UNSUPPORTED, "sample is being
 * edited" — said before "still referenced by a clip": the pin passes by itself).  Arguments, results and refusals are wbx_clip_measure's and wbx_clip_derive's.
 *   derive     *new_sample is a fresh sample id, registered as a bounce's results are: usable at once in
 *              wbx_engine_add_audio_clip, wbx_engine_export_sample, wbx_clip_build_mipmaps, wbx_engine_delete_sample
 *   normalize  measures [first_frame, first_frame + n_frames), takes gain = target_peak / max(peak[0], peak[1]) as ONE IEEE
 *              fp32 division on the host (*gain_used, may be NULL) and derives that range with it (WBX_CH_KEEP, no fade).
 *              The result's peak is fl(peak * gain), which may differ from target_peak by one ulp.  A silent range
 *              (peak == 0) or one whose peak is not finite is WBX_ERR_INVALID and creates no sample */
wbx_status wbx_engine_measure_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                     wbx_clip_stats* stats);
wbx_status wbx_engine_derive_sample(wbx_engine* e, uint32_t sample, const wbx_clip_edit_desc* desc, uint32_t* new_sample);
wbx_status wbx_engine_normalize_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                       float target_peak, uint32_t* new_sample, float* gain_used);
/* wbx_clip_resample of an engine sample, under wbx_engine_derive_sample's rules to the letter: editing thread, the audio
 * thread may keep calling wbx_engine_process*; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin, never across a device wait; wbx_engine_delete_sample refuses the source meanwhile ("sample is being edited");
 * no transport state is touched.  *new_sample is a fresh sample id registered with sample_rate = dst_rate and
 * wbx_resample_frames(...) frames: placed by wbx_engine_add_audio_clip at speed 1.0 in a session of that rate it plays
 * through the unity row mode.  Arguments and refusals are wbx_clip_resample's. */
wbx_status wbx_engine_resample_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                      uint32_t dst_rate, int quality, uint32_t* new_sample);
/* wbx_clip_splice of engine samples (a part's src_clip is a sample id), under wbx_engine_derive_sample's rules to the
 * letter: editing thread, the audio thread may keep calling wbx_engine_process*; the editor lock is held only to validate,
 * to copy every source's storage description out, to pin, to order the stream, to publish and to unpin, never across a
 * device wait; no transport state is touched and no edit is counted.  EVERY distinct source of the call is pinned for
 * its life: wbx_engine_delete_sample refuses each of them meanwhile ("sample is being edited", asked before "still
 * referenced by a clip").  *new_sample is a fresh sample id registered at the sources' common rate.  Arguments and
 * refusals are wbx_clip_splice's (there is no dst_clip to collide with). */
wbx_status wbx_engine_splice_samples(wbx_engine* e, uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts,
                                     uint32_t n_parts, uint32_t* new_sample);
/* wbx_clip_loudness of an engine sample, under wbx_engine_measure_sample's rules to the letter: editing thread, the audio
 * thread may keep calling wbx_engine_process*; the editor lock is held only to validate, pin, order the stream and unpin,
 * never across a device wait; wbx_engine_delete_sample refuses the source meanwhile ("sample is being edited"); no
 * transport state is touched and no edit is counted.  Arguments, results and refusals are wbx_clip_loudness's.
 *   normalize  measures the range (with true peak when true_peak_ceiling, linear, is not 0), takes
 *              g = (float)pow(10.0, (target_lufs - integrated) / 20.0) and, with a ceiling,
 *              g = min(g, ceiling / max(true_peak[0], true_peak[1])) as ONE IEEE fp32 division on the host (*gain_used, may be
 *              NULL), and derives that range with it (WBX_CH_KEEP, no fade) as wbx_engine_normalize_sample does: *new_sample is
 *              a fresh sample id.  WBX_ERR_INVALID, and no sample, when `integrated` is not finite (a silent range, one
 *              shorter than 4 hops), when the gain is not finite and positive, or for a negative or NaN ceiling */
wbx_status wbx_engine_loudness_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t flags,
                                      wbx_loudness* out, double* hop_energy, size_t cap_doubles);
wbx_status wbx_engine_normalize_loudness_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                double target_lufs, float true_peak_ceiling, uint32_t* new_sample,
                                                float* gain_used);
/* wbx_clip_filter of an engine sample, under wbx_engine_derive_sample's rules to the letter: editing thread, the audio
 * thread may keep calling wbx_engine_process*; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin, never across a device wait; wbx_engine_delete_sample refuses the source meanwhile ("sample is being edited");
 * no transport state is touched and no edit is counted.  *new_sample is a fresh sample id registered at the source's rate
 * with n_frames + tail_frames frames.  Arguments and refusals are wbx_clip_filter's (there is no dst_clip to collide with). */
wbx_status wbx_engine_filter_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                    uint64_t tail_frames, const double* coef, uint32_t n_stages, uint32_t* new_sample);
/* wbx_clip_convolve of two engine samples, under wbx_engine_filter_sample's rules: BOTH the source and the response are
 * pinned for the call, so wbx_engine_delete_sample refuses either meanwhile ("sample is being edited"); the editor lock is
 * held only to validate, pin, order the stream, publish and unpin.  *new_sample is a fresh sample id registered at the
 * source's rate with out_frames frames and max(source, response) channels.  Arguments and refusals are wbx_clip_convolve's
 * (there is no dst_clip to collide with). */
wbx_status wbx_engine_convolve_sample(wbx_engine* e, uint32_t sample, uint32_t ir_sample, uint64_t first_frame,
                                      uint64_t n_frames, uint64_t ir_first, uint64_t ir_frames, uint64_t out_first,
                                      uint64_t out_frames, double gain, uint32_t* new_sample,
                                      wbx_clip_stats* stats_of_result);
/* wbx_clip_limit of an engine sample, under wbx_engine_filter_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile ("sample is being edited"); the editor lock is held only to validate, pin,
 * order the stream, publish and unpin.  *new_sample is a fresh sample id registered at the source's rate with n_frames
 * frames and the source's channels.  Arguments and refusals are wbx_clip_limit's (there is no dst_clip to collide with). */
wbx_status wbx_engine_limit_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, float ceiling,
                                   double drive, uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames,
                                   uint32_t* new_sample, wbx_limit_stats* limit_stats, wbx_clip_stats* stats_of_result);
/* wbx_clip_dynamics of an engine sample, keyed by itself (key_sample == WBX_DYN_NO_KEY) or by another sample, under
 * wbx_engine_convolve_sample's rules: the source and the key are pinned for the call (one id where they are the same
 * sample), so wbx_engine_delete_sample refuses them meanwhile; the editor lock is held only to validate, pin, order the
 * stream, publish and unpin.  *new_sample is a fresh sample id registered at the source's rate with n_frames frames and the
 * source's channels.  Arguments and refusals are wbx_clip_dynamics' (there is no dst_clip to collide with). */
wbx_status wbx_engine_dynamics_sample(wbx_engine* e, uint32_t sample, uint32_t key_sample, uint64_t first_frame,
                                      uint64_t n_frames, uint64_t key_first, int sense, const double* table, double drive,
                                      double key_gain, double makeup, uint32_t lookahead_frames, uint32_t hold_frames,
                                      uint32_t release_frames, uint32_t* new_sample, wbx_dynamics_stats* dynamics_stats,
                                      wbx_clip_stats* stats_of_result);
/* wbx_clip_saturate of an engine sample, under wbx_engine_limit_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with n_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_saturate's (there is no dst_clip to collide with). */
wbx_status wbx_engine_saturate_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t os,
                                      int quality, const double* table, double drive, double makeup, uint32_t* new_sample,
                                      wbx_saturate_stats* saturate_stats, wbx_clip_stats* stats_of_result);
/* wbx_clip_varispeed of an engine sample, under wbx_engine_limit_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with out_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_varispeed's (there is no dst_clip to collide with). */
wbx_status wbx_engine_varispeed_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                       uint64_t out_frames, const int64_t* knots, uint64_t n_knots, uint32_t knot_shift,
                                       int quality, uint32_t guard_num, uint32_t guard_den, uint32_t* new_sample,
                                       wbx_clip_stats* stats_of_result);
/* wbx_clip_denoise of an engine sample, under wbx_engine_limit_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with n_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_denoise's (there is no dst_clip to collide with). */
wbx_status wbx_engine_denoise_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                     uint32_t window_frames, uint32_t smooth_hops, uint32_t smooth_bins, const double* thr,
                                     double floor, uint32_t* new_sample, wbx_denoise_stats* stats);
/* wbx_clip_denoise_profile of an engine sample, under wbx_engine_spectrum_sample's rules: the sample is pinned for the
 * call; no sample is made.  Arguments and refusals are wbx_clip_denoise_profile's. */
wbx_status wbx_engine_denoise_profile_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                             uint32_t window_frames, double* sums_out, uint64_t* hops_out);
/* wbx_clip_stretch of an engine sample, under wbx_engine_limit_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with out_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_stretch's (there is no dst_clip to collide with, and no positions). */
wbx_status wbx_engine_stretch_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames,
                                     uint32_t window_frames, uint32_t tolerance_frames, wbx_stretch_info* info,
                                     uint32_t* new_sample);
/* wbx_clip_warp of an engine sample, under wbx_engine_stretch_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with out_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_warp's (there is no dst_clip to collide with, and no positions). */
wbx_status wbx_engine_warp_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames,
                                  const wbx_warp_marker* markers, uint32_t n_markers, uint32_t window_frames,
                                  uint32_t tolerance_frames, wbx_warp_info* info, uint32_t* new_sample);
/* wbx_clip_pitch of an engine sample, under wbx_engine_stretch_sample's rules: the source is pinned for the call, so
 * wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream, publish
 * and unpin.  *new_sample is a fresh sample id registered at the source's rate with out_frames frames and the source's
 * channels.  Arguments and refusals are wbx_clip_pitch's (there is no dst_clip to collide with, and no positions). */
wbx_status wbx_engine_pitch_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames,
                                   uint32_t num, uint32_t den, int quality, uint32_t window_frames, uint32_t tolerance_frames,
                                   wbx_pitch_info* info, uint32_t* new_sample);
/* wbx_clip_f0 of an engine sample, beside wbx_engine_loudness_sample and under its rules: the sample is pinned for the
 * call, so wbx_engine_delete_sample refuses it meanwhile; the editor lock is held only to validate, pin, order the stream
 * and unpin, never across the device wait, so the call may run beside the audio thread.  Arguments and refusals are
 * wbx_clip_f0's. */
wbx_status wbx_engine_f0_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                                uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max, double threshold,
                                wbx_f0_frame* frames_out, size_t frames_cap, wbx_f0_info* info);
/* wbx_clip_spectrum of engine samples, under wbx_engine_f0_sample's rules: the sample AND the basis sample are pinned for
 * the call (one id where they are the same), so wbx_engine_delete_sample refuses either meanwhile; the editor lock is held
 * only to validate, pin, order the stream and unpin, never across the device waits, so the call may run beside the audio
 * thread.  Arguments and refusals are wbx_clip_spectrum's. */
wbx_status wbx_engine_spectrum_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t channel,
                                      uint32_t basis_sample, uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames,
                                      float* power_out, size_t cells_cap, wbx_spectrum_info* info);
/* wbx_clip_align of engine samples, under wbx_engine_spectrum_sample's rules: the reference sample AND the sample to be
 * aligned are pinned for the call (one id where they are the same), so wbx_engine_delete_sample refuses either meanwhile;
 * the editor lock is held only to validate, pin, order the stream and unpin, never across the device wait, so the call may
 * run beside the audio thread.  Arguments and refusals are wbx_clip_align's. */
wbx_status wbx_engine_align_samples(wbx_engine* e, uint32_t ref_sample, uint64_t a_first, uint64_t n_frames, uint32_t sample,
                                    uint64_t b_first, uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags,
                                    wbx_align_info* info, wbx_align_point* curve_out, size_t curve_cap);
/* wbx_clip_onsets and wbx_clip_tempo of an engine sample, under wbx_engine_f0_sample's rules: pinned for the call, the
 * editor lock held only to validate and pin.  Arguments and refusals are the clip calls'. */
wbx_status wbx_engine_onsets_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                                    double floor_power, double threshold, double delta, uint32_t w, uint32_t a,
                                    wbx_onset_frame* frames_out, size_t frames_cap, wbx_onset_info* info);
wbx_status wbx_engine_tempo_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                                   double floor_power, uint32_t window_hops, uint32_t step_hops, uint32_t lag_min,
                                   uint32_t lag_max, double threshold, wbx_f0_frame* frames_out, size_t frames_cap,
                                   wbx_f0_info* info);
/* Upper bound in bytes on what the clip pool reserves from the driver (slabs and clips with an allocation of their own);
 * 0 = none (the default).  A clip that would take the pool past it fails with WBX_ERR_OOM. */
wbx_status wbx_clip_pool_limit(wbx_ctx* ctx, uint64_t max_bytes_reserved);

/* Transport after the last process/render (engine.h:44-46), for bit-exact checks. */
wbx_status wbx_engine_transport(wbx_engine* e, double* playhead, double* sample_position, int* playing);
/* VUMeter::level per track/channel: max since the last call (vu_meter.h:20-40). levels: [n_tracks][C]. */
wbx_status wbx_engine_levels(wbx_engine* e, float* levels, uint32_t n_tracks);

/* What the last process / render took from the state it shares with the UI thread (the threading contract is the
 * reference's: one audio thread in process / render holding the editor lock — Engine::editor_lock, engine.cpp:1587-1651
 * — one UI thread whose edits take the same lock while Track::set_volume / set_pan / set_mute go through a per-track
 * single-producer ring of 64 messages, track.cpp:47-79, core/queue.h:142-196):
 *   edits_seen  number of locked edit calls (clip / track / transport edits, play, stop) completed before it
 *   drained     [n_tracks] cumulative parameter messages the audio thread has taken from each track's ring
 * Together with the UI thread's own log this reconstructs the exact state every block was rendered from. */
wbx_status wbx_engine_thread_stats(wbx_engine* e, uint64_t* edits_seen, uint64_t* drained, uint32_t n_tracks);

/* How the device sequencer planned the renders so far (diagnostic; no reference counterpart — Track::process_event,
 * track.cpp:258-451, is one thread).  Long renders of sessions cut into clips are planned by one lane per (track, SEGMENT of
 * the render) instead of one lane per track: a segment's lane works out the state its first block starts from by itself, and
 * the lane that completes a track checks every seam against the state the segment before really ended with, planning again —
 * in one walk, from the true state — whatever follows a seam that did not hold (results are the one-walk plan's either way).
 *   out[0]  renders planned by segments     out[1]  tracks that had a seam that did not hold
 *   out[2]  segments planned again          out[3]  segments per track of the last such render */
wbx_status wbx_engine_sequencer_stats(wbx_engine* e, uint64_t out[4]);

/* How wbx_engine_process — the audio callback, audio_io_pulseaudio.cpp:396-466 calling Engine::process once per device
 * period — has run so far (diagnostic; no reference counterpart).  A block is ONE launch where an instance exists for the
 * block shape; its sum is spread over all workgroups behind a barrier that needs the whole grid resident at once.  A workgroup
 * that waits there too long (a CU mask, a device shared with another process) gives up; the block is then mixed and summed
 * again through three launches — its result is the same — and the engine stops spreading.
 *   out[0]  blocks that ran as one launch       out[1]  ... of those, with the sum spread over the workgroups
 *   out[2]  blocks mixed again after a give-up  out[3]  1 when the engine has stopped spreading */
wbx_status wbx_engine_callback_stats(wbx_engine* e, uint64_t out[4]);

/* Engine::perf_measurer (engine.h:64, core/timing.h:54-67): Engine::process times itself (ScopedPerformanceCounter,
 * engine.cpp:1577) and ends with perf_measurer.update(duration_ms, audio_buffer_duration_ms) (engine.cpp:1653) — usage moves a
 * quarter of the way towards duration / period; the UI shows get_usage(), clamped to [0, 1] (ui/control_bar.cpp:54).  Here every
 * wbx_engine_process / wbx_engine_process_interleaved call feeds its own wall time (launch, device pass, copy-out) and the
 * period of its block, period_to_ms(buffer_size_to_period(block_frames, sample_rate)) (engine.cpp:52, engine/audio_io.h:187-195).
 * Any thread.  last_block_ms (may be NULL): what the last update was fed.  Batch renders (wbx_engine_render) do not feed it:
 * the reference has no such call. */
wbx_status wbx_engine_perf_usage(wbx_engine* e, double* usage, double* last_block_ms);
/* the arithmetic behind it, host-only: PerformanceMeasurer::update (timing.h:57-62), ::get_usage (timing.h:64-66),
 * Engine::audio_buffer_duration_ms (engine.cpp:52) */
double wbx_calc_perf_update(double usage, double duration_ms, double period_ms);
double wbx_calc_perf_usage(double usage);
double wbx_calc_buffer_period_ms(uint32_t buffer_size, uint32_t sample_rate);

/* The plan the device sequencer produced for the last process/render: one record per Sampler::stream
 * call, ordered by (block, track, call).  For seek-math parity checks (bit patterns, not tolerances). */
typedef struct wbx_plan_record {
  uint32_t block, track;
  uint32_t buffer_offset, num_samples;   /* as handed to Sampler::stream */
  uint32_t num_actual;                   /* after the clip-tail limit, sampler.cpp:102-104 */
  uint32_t sample;
  double sample_offset;                  /* Sampler::sample_offset_ before the call */
  double playback_speed;
  float gain;
  uint32_t _pad;
} wbx_plan_record;
wbx_status wbx_engine_fetch_plan(wbx_engine* e, wbx_plan_record* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* WBX_H */
