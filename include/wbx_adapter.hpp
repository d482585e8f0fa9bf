// wbx_adapter.hpp — header-only C++ adapter over the C ABI (wbx.h) with the reference's own shapes.
//
// A reference maintainer who wants the MI355X path behind the existing C++ host replaces `wb::Engine
// g_engine` (src/engine/engine.cpp:1715, engine.h:273) by `wbx::Engine`: same method names, argument
// meaning and buffer type as
//   wb::AudioBuffer<float>                         src/core/audio_buffer.h:14-175
//   wb::Engine::set_audio_channel_config/set_bpm/add_track/add_audio_clip/play/stop/process
//                                                   src/engine/engine.h:68-113,235-239
//   wb::Engine::record/stop_record/arm_track_recording/set_track_input, wb::TrackInputType
//                                                   src/engine/engine.cpp:95-200, track_input.h:10-15
//   wb::Track::set_volume/set_pan/set_mute          src/engine/track.h:137-139
// Compiles with any C++17 compiler (no HIP headers needed); link against libwbx.so.
#pragma once
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "wbx.h"

namespace wbx {

enum class AudioFormat : int {   // values of the reference's enum, src/core/audio_format.h:7-20 (= WBX_FMT_* / WBX_OUT_*)
  I16 = WBX_OUT_I16, I24 = WBX_OUT_I24, I24_X8 = WBX_OUT_I24_X8, I32 = WBX_OUT_I32, F32 = WBX_OUT_F32
};

// Planar sample buffer with the reference's fields, layout and semantics (audio_buffer.h:14-175): the first 16 channel
// pointers live inside the object (`internal_channel_buffers`), `channel_buffers` points at them or, beyond 16
// channels, at a heap array; every channel is a separate 32-byte aligned, zero-filled allocation.
template <typename T>
struct AudioBuffer {
  static_assert(sizeof(T) == 4, "the mix path is fp32");
  static constexpr uint32_t internal_buffer_capacity = 16;
  static constexpr uint32_t alignment = 32;

  uint32_t n_samples{};
  uint32_t n_channels{};
  uint32_t channel_capacity = internal_buffer_capacity;
  T* internal_channel_buffers[internal_buffer_capacity]{};
  T** channel_buffers{};

  AudioBuffer() : channel_buffers(internal_channel_buffers) {}
  AudioBuffer(uint32_t sample_count, uint32_t channel_count) : n_samples(sample_count), channel_buffers(internal_channel_buffers) {
    resize_channel_array_(channel_count);
    for (uint32_t i = 0; i < n_channels; i++) channel_buffers[i] = alloc_channel(sample_count);
  }
  AudioBuffer(const AudioBuffer&) = delete;
  AudioBuffer& operator=(const AudioBuffer&) = delete;
  ~AudioBuffer() {
    for (uint32_t i = 0; i < n_channels; i++) std::free(channel_buffers[i]);
    if (channel_buffers != internal_channel_buffers) std::free(channel_buffers);
  }
  T* get_write_pointer(uint32_t channel, uint32_t sample_offset = 0) {
    assert(channel < n_channels && "Channel out of range");
    return channel_buffers[channel] + sample_offset;
  }
  const T* get_read_pointer(uint32_t channel, uint32_t sample_offset = 0) const {
    assert(channel < n_channels && "Channel out of range");
    return channel_buffers[channel] + sample_offset;
  }
  void set_sample(uint32_t channel, uint32_t sample_offset, T sample) const { channel_buffers[channel][sample_offset] = sample; }
  void mix_sample(uint32_t channel, uint32_t sample_offset, T sample) const { channel_buffers[channel][sample_offset] += sample; }
  void clear() {   // audio_buffer.h:67-71
    for (uint32_t i = 0; i < n_channels; i++) std::memset(channel_buffers[i], 0, n_samples * sizeof(T));
  }
  void mix(const AudioBuffer<T>& other) {   // audio_buffer.h:73-82: iterates THIS buffer's channels
    assert(n_samples == other.n_samples);
    for (uint32_t i = 0; i < n_channels; i++)
      for (uint32_t j = 0; j < n_samples; j++) channel_buffers[i][j] += other.channel_buffers[i][j];
  }
  // resize(samples, clear): keeps the old contents unless `clear`, zero-fills the growth (audio_buffer.h:84-110)
  void resize(uint32_t samples, bool clear = false) {
    if (samples == n_samples) return;
    for (uint32_t i = 0; i < n_channels; i++) {
      T* fresh = alloc_channel(samples);
      if (!clear) std::memcpy(fresh, channel_buffers[i], (samples < n_samples ? samples : n_samples) * sizeof(T));
      std::free(channel_buffers[i]);
      channel_buffers[i] = fresh;
    }
    n_samples = samples;
  }
  // resize_channel(count): new channels are zeroed, dropped ones freed (audio_buffer.h:112-132)
  void resize_channel(uint32_t channel_count) {
    assert(n_samples != 0);
    if (channel_count == n_channels) return;
    const uint32_t old = n_channels;
    for (uint32_t i = channel_count; i < old; i++) {
      std::free(channel_buffers[i]);
      channel_buffers[i] = nullptr;
    }
    resize_channel_array_(channel_count);
    for (uint32_t i = old; i < channel_count; i++) channel_buffers[i] = alloc_channel(n_samples);
  }
  // planar -> interleaved (audio_buffer.h:143-160).  The fp32 case is a copy and stays on the host
  // (convert_to_interleaved_f32, audio_format_conv.cpp:79-91); the integer device formats are produced on the GPU from
  // the master it already holds: wbx_fetch_interleaved(ctx, WBX_OUT_*, dst) — nothing of the path computes on the CPU.
  void interleave_samples_to(void* dst, uint32_t offset, uint32_t count, AudioFormat format = AudioFormat::F32) const {
    assert(format == AudioFormat::F32 && "integer formats: wbx_fetch_interleaved");
    (void)format;
    float* out = static_cast<float*>(dst);
    for (uint32_t c = 0; c < n_channels; c++)
      for (uint32_t i = 0; i < count; i++) out[(size_t)i * n_channels + c] = channel_buffers[c][offset + i];
  }
  // interleaved f32 -> planar (convert_to_deinterleaved_f32, audio_format_conv.cpp:93-105; the reference has no other case)
  void deinterleave_samples_from(const void* src, uint32_t dst_offset, uint32_t count, AudioFormat format = AudioFormat::F32) {
    assert(format == AudioFormat::F32);
    (void)format;
    const float* in = static_cast<const float*>(src);
    for (uint32_t c = 0; c < n_channels; c++)
      for (uint32_t i = 0; i < count; i++) channel_buffers[c][dst_offset + i] = in[(size_t)i * n_channels + c];
  }
  // audio_buffer.h:162-174 (the pointer array moves to the heap beyond `channel_capacity` channels)
  void resize_channel_array_(uint32_t channel_count) {
    if (channel_count > channel_capacity) {
      T** grown = static_cast<T**>(std::calloc(channel_count, sizeof(T*)));
      assert(grown && "Cannot allocate memory for audio channel array");
      std::memcpy(grown, channel_buffers, (n_channels < channel_count ? n_channels : channel_count) * sizeof(T*));
      if (channel_buffers != internal_channel_buffers) std::free(channel_buffers);
      channel_buffers = grown;
      channel_capacity = channel_count;
    }
    n_channels = channel_count;
  }

 private:
  static T* alloc_channel(uint32_t samples) {
    T* p = static_cast<T*>(std::aligned_alloc(alignment, ((samples * sizeof(T) + alignment - 1) / alignment) * alignment + alignment));
    assert(p && "Cannot allocate memory for audio buffer");
    std::memset(p, 0, samples * sizeof(T));
    return p;
  }
};

struct Error : std::runtime_error {
  wbx_status status;
  Error(wbx_status s, const std::string& what) : std::runtime_error(what), status(s) {}
};

struct Engine;

// The audio-side half of engine/vu_meter.h (push_samples, :20-30) runs on the GPU as running per-track maxima;
// Engine::fetch_levels() moves them in here with the reference's CAS-max.  update() / get_value() keep the UI code that
// is written against Track::level_meter compiling unchanged (ui/controls.cpp: level_meter[c].update(...), .get_value()).
struct VUMeter {
  std::atomic<float> level{0.0f};
  float current_level = 0.0f;   // vu_meter.h:18
  void push_level(float peak) {   // the CAS-max tail of VUMeter::push_samples, vu_meter.h:26-29
    float seen = level.load(std::memory_order_relaxed);
    while (seen < peak && !level.compare_exchange_weak(seen, peak, std::memory_order_release, std::memory_order_relaxed)) {
    }
  }
  // the maximum since the last call; resets it (what the host's own VUMeter::update starts from)
  float take_level() { return level.exchange(0.0f, std::memory_order_acq_rel); }
  // UI rate, vu_meter.h:32-44: the meter jumps up to a new maximum at once and falls back towards the newest one through a
  // one-pole release whose time constant is 1 / (frame_rate * speed) frames
  void update(float frame_rate, float speed) {
    const float peak = take_level();
    if (peak > current_level) {
      current_level = peak;
      return;
    }
    const float release = 1.0f - std::exp(-1.0f / (frame_rate * speed));
    current_level += (peak - current_level) * release;
  }
  float get_value() const { return current_level; }
};

struct Track {   // track.h:110-139
  Engine* engine{};
  uint32_t index{};
  std::string name;
  VUMeter level_meter[2]{};             // track.h:121
  const wbx_plugin* plugin_instance{};  // track.h:124: the effect slot, always empty in this path
  Track(Engine* e, uint32_t i, std::string n) : engine(e), index(i), name(std::move(n)) {}
  void set_volume(float db);
  void set_pan(float pan);
  void set_mute(bool mute);
};

enum class TrackInputType : int {   // track_input.h:10-15 (= WBX_INPUT_*); Midi is refused by set_track_input
  None = WBX_INPUT_NONE, Midi = WBX_INPUT_MIDI, ExternalStereo = WBX_INPUT_EXTERNAL_STEREO, ExternalMono = WBX_INPUT_EXTERNAL_MONO
};

struct AudioClip {   // clip.h:39-45: the asset is a sample id returned by Engine::add_sample
  uint32_t asset{};
  double speed = 1.0;
  float gain = 1.0f;
};

struct Engine {
  wbx_engine* h{};
  uint32_t num_input_channels = 0, num_output_channels = 0, audio_buffer_size = 0, audio_sample_rate = 0;
  std::vector<std::unique_ptr<Track>> tracks;
  // device-side limits, fixed when the engine is first configured (not part of the reference's surface)
  uint32_t max_tracks = 4096, max_blocks = 1;
  int device = 0;
  // The audio path has no exceptions in the reference (Engine::process returns void, failures are asserts): process()
  // never throws — a failed block leaves silence in the output buffer and latches its status here.
  std::atomic<wbx_status> process_status{WBX_OK};
  std::string process_error;   // written by the audio thread only
  // engine.h:33 / :64 — the block's period in ms (engine.cpp:52) and the load figure process() keeps (engine.cpp:1653):
  // `g_engine.perf_measurer.get_usage()` of ui/control_bar.cpp:54 reads the same here
  double audio_buffer_duration_ms = 0;
  struct PerformanceMeasurer {
    Engine* owner;
    double get_usage() const {
      double u = 0.0;
      return (owner->h && wbx_engine_perf_usage(owner->h, &u, nullptr) == WBX_OK) ? u : 0.0;
    }
  } perf_measurer{this};

  // set_audio_channel_config(in, out, buffer_size, sample_rate), engine.cpp:43-57.  The first call creates the device
  // context; later calls (the audio backend was reconfigured) resize it in place — tracks and clips stay, as in the
  // reference.
  void set_audio_channel_config(uint32_t input_channels, uint32_t output_channels, uint32_t buffer_size, uint32_t sample_rate) {
    if (!h) {
      wbx_config cfg{};
      cfg.device = device;
      cfg.max_tracks = max_tracks;
      cfg.max_blocks = max_blocks;
      cfg.block_frames = buffer_size;
      cfg.channels = output_channels;
      cfg.sample_rate = sample_rate;
      check(wbx_engine_create(&cfg, &h), "wbx_engine_create");
    } else {
      check(wbx_engine_set_audio_channel_config(h, output_channels, buffer_size, sample_rate), "set_audio_channel_config");
    }
    check(wbx_engine_set_input_channels(h, input_channels), "set_audio_channel_config");
    num_input_channels = input_channels;
    num_output_channels = output_channels;
    audio_buffer_size = buffer_size;
    audio_sample_rate = sample_rate;
    audio_buffer_duration_ms = wbx_calc_buffer_period_ms(buffer_size, sample_rate);
  }
  ~Engine() {
    if (h) wbx_engine_destroy(h);
  }
  void set_bpm(double bpm) { check(wbx_engine_set_bpm(h, bpm), "set_bpm"); }
  void set_playhead_position(double beat) { check(wbx_engine_set_playhead_position(h, beat), "set_playhead_position"); }
  Track* add_track(const std::string& name) {
    uint32_t idx = 0;
    check(wbx_engine_add_track(h, &idx), "add_track");
    tracks.emplace_back(new Track(this, idx, name));
    return tracks.back().get();
  }
  // engine.cpp:210-262
  void delete_track(uint32_t slot) {
    check(wbx_engine_delete_track(h, slot), "delete_track");
    tracks.erase(tracks.begin() + slot);
    for (uint32_t i = 0; i < tracks.size(); i++) tracks[i]->index = i;
  }
  void move_track(uint32_t from_slot, uint32_t to_slot) {
    check(wbx_engine_move_track(h, from_slot, to_slot), "move_track");
    auto t = std::move(tracks[from_slot]);
    tracks.erase(tracks.begin() + from_slot);
    tracks.insert(tracks.begin() + to_slot, std::move(t));
    for (uint32_t i = 0; i < tracks.size(); i++) tracks[i]->index = i;
  }
  void solo_track(uint32_t slot) { check(wbx_engine_solo_track(h, slot), "solo_track"); }
  void clear_all() {   // engine.cpp:59-66
    check(wbx_engine_clear_all(h), "clear_all");
    tracks.clear();
  }
  // decoded clip audio -> HBM (what SampleAsset / Sample hold in the reference: assets_table.h:22-35, sample.h:18-28)
  uint32_t add_sample(int format, uint32_t channels, uint32_t sample_rate, uint64_t frames, const void* const* planar) {
    uint32_t id = 0;
    check(wbx_engine_add_sample(h, format, channels, sample_rate, frames, planar, &id), "add_sample");
    return id;
  }
  // the same from a decoder's interleaved frames (what Sample::load_file reads: sample.cpp:154-183); the
  // deinterleave of sample.cpp:29-43 runs on the GPU
  uint32_t add_sample_interleaved(int format, uint32_t channels, uint32_t sample_rate, uint64_t frames, const void* interleaved) {
    uint32_t id = 0;
    check(wbx_engine_add_sample_interleaved(h, format, channels, sample_rate, frames, interleaved, &id), "add_sample_interleaved");
    return id;
  }
  // Engine::add_audio_clip(track, name, min_time, max_time, start_offset, clip_info), engine.h:106-113
  void add_audio_clip(Track* track, const std::string& /*name*/, double min_time, double max_time, double start_offset,
                      const AudioClip& clip_info) {
    check(wbx_engine_add_audio_clip(h, track->index, min_time, max_time, start_offset, clip_info.asset, clip_info.speed,
                                    clip_info.gain),
          "add_audio_clip");
  }
  void play() { check(wbx_engine_play(h), "play"); }
  void stop() { check(wbx_engine_stop(h), "stop"); }
  // Bounce (no reference counterpart: its export dialog has nothing behind it): render [min_time, max_time) offline and
  // keep the named signals — tracks post- or pre-fader, buses, the master — as sample ids usable in add_audio_clip
  // (AudioClip::asset), wbx_clip_download and wbx_engine_delete_sample.  Returns the ids in the order of `sources`;
  // *frames (optional) receives every sample's length.  Semantics and refusals: wbx_engine_bounce, wbx.h.
  std::vector<uint32_t> bounce(double min_time, double max_time, const std::vector<wbx_bounce_source>& sources,
                               uint64_t* frames = nullptr) {
    std::vector<uint32_t> ids(sources.size());
    check(wbx_engine_bounce(h, min_time, max_time, sources.data(), (uint32_t)sources.size(), ids.data(), frames), "bounce");
    return ids;
  }
  // Export a sample (a take's, a bounce's, any F32 sample) as interleaved samples of a device format (WBX_OUT_*) into
  // `dst` — wbx_export_bytes(out_format, channels, n_frames) bytes of host memory — and return the range's statistics
  // (peak, samples beyond +-1, NaNs per channel, of the source values).  Packed 24-bit is true interleave here (every
  // channel, unlike the callback's writer).  Editing thread; the audio thread may keep calling process().  A long sample
  // may be streamed into a file by calls with advancing first_frame.  Semantics and refusals: wbx_clip_export, wbx.h.
  wbx_export_stats export_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, int out_format, void* dst,
                                 bool clamp = true) {
    wbx_export_stats stats{};
    check(wbx_engine_export_sample(h, sample, first_frame, n_frames, out_format, clamp ? (uint32_t)WBX_EXPORT_CLAMP : 0u, dst, &stats),
          "export_sample");
    return stats;
  }
  // Measure and edit samples where they live (wbx.h "Editing clips"): peak / RMS / DC material of a range; a NEW sample
  // derived by trim, reverse, channel mode, gain and fades; a new sample normalized to a peak (*gain_used: the factor).
  // Editing thread; the audio thread may keep calling process().  The ids go where a bounce's go.
  wbx_clip_stats measure_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames) {
    wbx_clip_stats stats{};
    check(wbx_engine_measure_sample(h, sample, first_frame, n_frames, &stats), "measure_sample");
    return stats;
  }
  uint32_t derive_sample(uint32_t sample, const wbx_clip_edit_desc& desc) {
    uint32_t id = 0;
    check(wbx_engine_derive_sample(h, sample, &desc, &id), "derive_sample");
    return id;
  }
  uint32_t normalize_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, float target_peak, float* gain_used = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_normalize_sample(h, sample, first_frame, n_frames, target_peak, &id, gain_used), "normalize_sample");
    return id;
  }
  // A NEW sample holding the range converted to dst_rate by the band-limited filter of wbx.h "Converting a clip's sample
  // rate" (quality: WBX_SRC_FAST / GOOD / BEST) — conform an imported file to the session rate once, or make the copy of a
  // bounce that leaves at another rate.  Editing thread, like derive_sample; the id goes where a bounce's go.
  uint32_t resample_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t dst_rate, int quality = WBX_SRC_GOOD) {
    uint32_t id = 0;
    check(wbx_engine_resample_sample(h, sample, first_frame, n_frames, dst_rate, quality, &id), "resample_sample");
    return id;
  }
  // A NEW sample holding the range run through a cascade of 1 .. 8 biquads (wbx.h "Filtering a clip"; coef is
  // [n_stages][b0 b1 b2 a1 a2], designed by wbx_filter_design or the caller's own), tail_frames of ring-out appended: a
  // high-pass against rumble, a notch, a corrective EQ baked into a stem.  Editing thread, like derive_sample.
  uint32_t filter_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t tail_frames, const double* coef,
                         uint32_t n_stages) {
    uint32_t id = 0;
    check(wbx_engine_filter_sample(h, sample, first_frame, n_frames, tail_frames, coef, n_stages, &id), "filter_sample");
    return id;
  }
  // A NEW sample holding frames [out_first, out_first + out_frames) of the range convolved with the range of ir_sample,
  // the impulse response, times gain (wbx.h "Convolving a clip"): a room or cabinet on a stem, a linear-phase FIR from
  // wbx_fir_design uploaded as a mono sample (out_first = (taps - 1) / 2 drops its delay).  Both samples are pinned for
  // the call.  Editing thread, like derive_sample.
  uint32_t convolve_sample(uint32_t sample, uint32_t ir_sample, uint64_t first_frame, uint64_t n_frames, uint64_t ir_first,
                           uint64_t ir_frames, uint64_t out_first, uint64_t out_frames, double gain = 1.0,
                           wbx_clip_stats* stats_of_result = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_convolve_sample(h, sample, ir_sample, first_frame, n_frames, ir_first, ir_frames, out_first, out_frames,
                                     gain, &id, stats_of_result), "convolve_sample");
    return id;
  }
  // A NEW sample holding the range through a look-ahead peak limiter (wbx.h "Limiting a clip"): drive (linear) in, then no
  // sample above ceiling (linear), with lookahead / hold / release in frames; no delay, the source's length.  The source is
  // pinned for the call.  Editing thread, like derive_sample.
  uint32_t limit_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, float ceiling, double drive,
                        uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames,
                        wbx_limit_stats* limit_stats = nullptr, wbx_clip_stats* stats_of_result = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_limit_sample(h, sample, first_frame, n_frames, ceiling, drive, lookahead_frames, hold_frames, release_frames,
                                  &id, limit_stats, stats_of_result), "limit_sample");
    return id;
  }
  // A NEW sample holding the range through a table-driven compressor, expander, gate or ducker (wbx.h "Dynamics of a
  // clip"): table = WBX_DYN_TABLE gains over level (wbx_dynamics_table, or hand-drawn), sense WBX_DYN_COMPRESS or
  // WBX_DYN_GATE, the level taken from the sample itself or from key_sample (WBX_DYN_NO_KEY: itself), lookahead / hold /
  // release in frames; no delay, the source's length.  Source and key are pinned for the call.  Editing thread, like
  // derive_sample.
  uint32_t dynamics_sample(uint32_t sample, uint32_t key_sample, uint64_t first_frame, uint64_t n_frames, uint64_t key_first,
                           int sense, const double* table, double drive, double key_gain, double makeup,
                           uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames,
                           wbx_dynamics_stats* dynamics_stats = nullptr, wbx_clip_stats* stats_of_result = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_dynamics_sample(h, sample, key_sample, first_frame, n_frames, key_first, sense, table, drive, key_gain, makeup,
                                     lookahead_frames, hold_frames, release_frames, &id, dynamics_stats, stats_of_result),
          "dynamics_sample");
    return id;
  }
  // A NEW sample holding the range through an oversampled table waveshaper (wbx.h "Saturating a clip"): table =
  // WBX_SAT_TABLE outputs over the driven level (wbx_saturate_table, or hand-drawn), os 1, 2, 4 or 8 at quality
  // WBX_SRC_*, drive in and makeup out (linear); no delay, the source's length, NO ceiling guarantee (limit_sample gives
  // one).  The source is pinned for the call.  Editing thread, like derive_sample.
  uint32_t saturate_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, const double* table, double drive = 1.0,
                           double makeup = 1.0, uint32_t os = 4, int quality = WBX_SRC_GOOD,
                           wbx_saturate_stats* saturate_stats = nullptr, wbx_clip_stats* stats_of_result = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_saturate_sample(h, sample, first_frame, n_frames, os, quality, table, drive, makeup, &id, saturate_stats,
                                     stats_of_result), "saturate_sample");
    return id;
  }
  // A NEW sample of out_frames frames holding the range read along a position curve (wbx.h "Reading a clip along a
  // position curve"): knots[i] = the position of output frame i << knot_shift in 2^-32 source frames relative to
  // first_frame, n_knots = ceil(out_frames / 2^knot_shift) + 1; guard_num / guard_den >= 1 = the fastest speed protected
  // from aliasing.  The source's rate and channels.  The source is pinned for the call.  Editing thread, like derive_sample.
  uint32_t varispeed_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames, const int64_t* knots,
                            uint64_t n_knots, uint32_t knot_shift, int quality = WBX_SRC_GOOD, uint32_t guard_num = 1,
                            uint32_t guard_den = 1, wbx_clip_stats* stats_of_result = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_varispeed_sample(h, sample, first_frame, n_frames, out_frames, knots, n_knots, knot_shift, quality, guard_num,
                                      guard_den, &id, stats_of_result), "varispeed_sample");
    return id;
  }
  // A NEW sample holding the range through the spectral gate (wbx.h "Reducing a clip's noise"): thr = channels x
  // (window_frames / 2 + 1) power thresholds (wbx_denoise_threshold of denoise_profile_sample's sums), floor the linear
  // gain of a closed cell; no delay, the source's length.  The source is pinned for the call.  Editing thread, like
  // derive_sample.
  uint32_t denoise_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames, const double* thr,
                          double floor = 0.1, uint32_t smooth_hops = 2, uint32_t smooth_bins = 1, wbx_denoise_stats* stats = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_denoise_sample(h, sample, first_frame, n_frames, window_frames, smooth_hops, smooth_bins, thr, floor, &id, stats),
          "denoise_sample");
    return id;
  }
  // The noise profile of the range: sums_out[channels x (window_frames / 2 + 1)] and the number of complete windows they
  // were added over.  A measurement: no sample is made.  Editing thread.
  uint64_t denoise_profile_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames, double* sums_out) {
    uint64_t hops = 0;
    check(wbx_engine_denoise_profile_sample(h, sample, first_frame, n_frames, window_frames, sums_out, &hops), "denoise_profile_sample");
    return hops;
  }
  // A NEW sample of out_frames frames holding the range time-stretched by WSOLA (wbx.h "Stretching a clip"): another
  // length at the same pitch; window_frames a multiple of 8 in 32 .. 8192, tolerance_frames 0 .. 4096.  The source is
  // pinned for the call.  Editing thread, like derive_sample.
  uint32_t stretch_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames, uint32_t window_frames,
                          uint32_t tolerance_frames, wbx_stretch_info* info = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_stretch_sample(h, sample, first_frame, n_frames, out_frames, window_frames, tolerance_frames, info, &id),
          "stretch_sample");
    return id;
  }
  // A NEW sample of out_frames frames holding the range warped along time markers (wbx.h "Warping a clip"): source frame
  // markers[i].src_frame of the range sounds at output frame markers[i].out_frame, WSOLA in between.  Pinned and threaded
  // as for stretch_sample.
  uint32_t warp_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames,
                       const std::vector<wbx_warp_marker>& markers, uint32_t window_frames, uint32_t tolerance_frames,
                       wbx_warp_info* info = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_warp_sample(h, sample, first_frame, n_frames, out_frames, markers.empty() ? nullptr : markers.data(),
                                 (uint32_t)markers.size(), window_frames, tolerance_frames, info, &id),
          "warp_sample");
    return id;
  }
  // A NEW sample of out_frames frames holding the range transposed by num / den (wbx.h "Pitch-shifting a clip"): another
  // pitch at the source's rate, out_frames = n_frames keeping the length; quality one of WBX_SRC_*, window and tolerance
  // as for stretch_sample.  The source is pinned for the call.  Editing thread, like derive_sample.
  uint32_t pitch_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint64_t out_frames, uint32_t num, uint32_t den,
                        int quality, uint32_t window_frames, uint32_t tolerance_frames, wbx_pitch_info* info = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_pitch_sample(h, sample, first_frame, n_frames, out_frames, num, den, quality, window_frames, tolerance_frames,
                                  info, &id),
          "pitch_sample");
    return id;
  }
  // The period track of a sample's range where it lives (wbx.h "Tracking a clip's pitch"): one wbx_f0_frame per hop — the
  // period in frames (the frequency is the sample's rate over it), the dip, the energy, whether the hop is voiced.  Lags
  // tau_min .. tau_max bound the periods looked for; threshold in (0, 1], 0.15 being YIN's.  The sample is pinned for the
  // call.  Editing thread, like measure_sample.
  std::vector<wbx_f0_frame> f0_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t window_frames,
                                      uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max, double threshold = 0.15,
                                      wbx_f0_info* info = nullptr) {
    const uint64_t hops = wbx_f0_hops(n_frames, window_frames, hop_frames, tau_max);
    // the call's own argument check first, so that a refused call (2^31 hops of one frame, say) allocates no records
    const wbx_status pre = wbx_f0_check(n_frames, window_frames, hop_frames, tau_min, tau_max, threshold, 1, (size_t)hops);
    if (pre != WBX_OK) throw Error(pre, std::string("f0_sample: ") + wbx_status_string(pre));
    std::vector<wbx_f0_frame> out((size_t)hops);
    check(wbx_engine_f0_sample(h, sample, first_frame, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold,
                               out.empty() ? nullptr : out.data(), out.size(), info),
          "f0_sample");
    return out;
  }
  // The spectrum of a sample's range where it lives (wbx.h "Seeing a clip's spectrum"): hop-major power[hops][n_bins] at the
  // frequencies of basis_sample, a mono F32 sample of wbx_spectrum_basis's 2 * n_bins * window_frames words.  channel 0, 1
  // or WBX_SPECTRUM_MID.  Both samples are pinned for the call.  Editing thread, like measure_sample.
  std::vector<float> spectrum_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t channel, uint32_t basis_sample,
                                     uint32_t window_frames, uint32_t n_bins, uint32_t hop_frames, wbx_spectrum_info* info = nullptr) {
    const uint64_t hops = wbx_spectrum_hops(n_frames, window_frames, hop_frames);
    // the call's own argument check first, so that a refused call allocates no cells
    const wbx_status pre = wbx_spectrum_check(n_frames, channel, window_frames, n_bins, hop_frames, 1, (size_t)(hops * n_bins));
    if (pre != WBX_OK) throw Error(pre, std::string("spectrum_sample: ") + wbx_status_string(pre));
    std::vector<float> out((size_t)(hops * n_bins));
    check(wbx_engine_spectrum_sample(h, sample, first_frame, n_frames, channel, basis_sample, window_frames, n_bins, hop_frames,
                                     out.empty() ? nullptr : out.data(), out.size(), info),
          "spectrum_sample");
    return out;
  }
  // By how many frames a sample lags a reference sample, where both live (wbx.h "Aligning two clips"): the template
  // [a_first, a_first + n_frames) of ref_sample (n_frames a multiple of 8 in 64 .. 2^24) against [b_first, b_first + m_frames)
  // of sample over the signed lags lag_min .. lag_max; flags 0 or WBX_ALIGN_EITHER_POLARITY.  `curve` (may be NULL) is
  // resized to one {r, energy} per lag.  Both samples are pinned for the call.  Editing thread, like measure_sample.
  wbx_align_info align_samples(uint32_t ref_sample, uint64_t a_first, uint64_t n_frames, uint32_t sample, uint64_t b_first,
                               uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags = 0,
                               std::vector<wbx_align_point>* curve = nullptr) {
    const size_t lags = lag_max >= lag_min ? (size_t)(lag_max - lag_min) + 1u : 0u;
    // the call's own argument check first, so that a refused call allocates no curve
    const wbx_status pre = wbx_align_check(n_frames, m_frames, lag_min, lag_max, flags, 1, curve != nullptr, lags);
    if (pre != WBX_OK) throw Error(pre, std::string("align_samples: ") + wbx_status_string(pre));
    if (curve) curve->assign(lags, wbx_align_point{0.0, 0.0});
    wbx_align_info info{};
    check(wbx_engine_align_samples(h, ref_sample, a_first, n_frames, sample, b_first, m_frames, lag_min, lag_max, flags, &info,
                                   curve ? curve->data() : nullptr, curve ? curve->size() : 0),
          "align_samples");
    return info;
  }
  // The onsets of a sample's range where it lives (wbx.h "Finding a clip's onsets and tempo"): one wbx_onset_frame per hop
  // of hop_frames frames (a multiple of 64) — the two energies, the onset strength and whether the hop is an onset, whose
  // frame is then first_frame + h * hop_frames.  The sample is pinned for the call.  Editing thread, like measure_sample.
  std::vector<wbx_onset_frame> onsets_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames = 256,
                                             double floor_power = 1e-9, double threshold = 0.3, double delta = 0.1, uint32_t w = 3,
                                             uint32_t a = 8, wbx_onset_info* info = nullptr) {
    const uint64_t hops = wbx_onset_hops(n_frames, hop_frames);
    // the call's own argument check first, so that a refused call allocates no records
    const wbx_status pre = wbx_onset_check(n_frames, hop_frames, floor_power, threshold, delta, w, a, 1, (size_t)hops);
    if (pre != WBX_OK) throw Error(pre, std::string("onsets_sample: ") + wbx_status_string(pre));
    std::vector<wbx_onset_frame> out((size_t)hops);
    check(wbx_engine_onsets_sample(h, sample, first_frame, n_frames, hop_frames, floor_power, threshold, delta, w, a,
                                   out.empty() ? nullptr : out.data(), out.size(), info),
          "onsets_sample");
    return out;
  }
  // ... and the period track of its onset strength, which stays on the device: one wbx_f0_frame per window of window_hops
  // hops every step_hops, with the period in hops — bpm = 60 * rate / (hop_frames * period).  Lags lag_min .. lag_max bound
  // the tempi looked for and decide the octave.
  std::vector<wbx_f0_frame> tempo_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t hop_frames,
                                         uint32_t window_hops, uint32_t step_hops, uint32_t lag_min, uint32_t lag_max,
                                         double threshold = 0.5, double floor_power = 1e-9, wbx_f0_info* info = nullptr) {
    const uint64_t hops = wbx_onset_hops(n_frames, hop_frames);
    const uint64_t windows = hops <= wbx_onset_max_hops() ? wbx_f0_hops(hops, window_hops, step_hops, lag_max) : 0;
    std::vector<wbx_f0_frame> out((size_t)windows);
    check(wbx_engine_tempo_sample(h, sample, first_frame, n_frames, hop_frames, floor_power, window_hops, step_hops, lag_min,
                                  lag_max, threshold, out.empty() ? nullptr : out.data(), out.size(), info),
          "tempo_sample");
    return out;
  }
  // BS.1770 loudness of a sample's range where it lives (wbx.h "Measuring a clip's loudness"): integrated, momentary and
  // short-term maxima, loudness range, with WBX_LOUD_TRUE_PEAK the oversampled peak — and a NEW sample brought to a target
  // (-14, -16, -23 LUFS) under a true-peak ceiling (linear, 0 = none; *gain_used: the factor).  Editing thread, like
  // measure_sample and normalize_sample.
  wbx_loudness loudness_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t flags = 0) {
    wbx_loudness out{};
    check(wbx_engine_loudness_sample(h, sample, first_frame, n_frames, flags, &out, nullptr, 0), "loudness_sample");
    return out;
  }
  uint32_t normalize_loudness_sample(uint32_t sample, uint64_t first_frame, uint64_t n_frames, double target_lufs,
                                     float true_peak_ceiling = 0.0f, float* gain_used = nullptr) {
    uint32_t id = 0;
    check(wbx_engine_normalize_loudness_sample(h, sample, first_frame, n_frames, target_lufs, true_peak_ceiling, &id, gain_used),
          "normalize_loudness_sample");
    return id;
  }
  // A NEW sample made of parts of other samples (wbx.h "Splicing clips"): takes comped, two samples crossfaded (two
  // overlapping parts, one fading out, one fading in), samples joined, a loop repeated, silence inserted.  A part's src_clip
  // is a sample id.  Editing thread, like derive_sample; every source is pinned for the call; the id goes where a bounce's go.
  uint32_t splice_samples(uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts) {
    uint32_t id = 0;
    check(wbx_engine_splice_samples(h, channels, n_frames, parts, n_parts, &id), "splice_samples");
    return id;
  }
  // recording, engine.cpp:95-200: the takes are captured on the device from process()'s input buffer and become clips
  // on their tracks at stop_record (a take that lost blocks still does; stop_record then throws with WBX_ERR_OVERFLOW)
  void record() { check(wbx_engine_record(h), "record"); }
  void stop_record() { check(wbx_engine_stop_record(h), "stop_record"); }
  void arm_track_recording(uint32_t slot, bool armed) { check(wbx_engine_arm_track_recording(h, slot, armed ? 1 : 0), "arm_track_recording"); }
  void set_track_input(uint32_t slot, TrackInputType type, uint32_t index, bool armed) {
    check(wbx_track_set_input(h, slot, static_cast<int>(type), index, armed ? 1 : 0), "set_track_input");
  }
  bool is_recording() const {
    int r = 0;
    check(wbx_engine_is_recording(h, &r), "is_recording");
    return r != 0;
  }
  // void Engine::process(const AudioBuffer<float>&, AudioBuffer<float>&, double), engine.h:235-239
  // Audio thread.  Never throws: on a failure the block is silence and process_status / process_error say why.
  // The input buffer is what a running take records (engine.cpp:1638-1649); it never reaches the output (no monitoring).
  void process(const AudioBuffer<float>& input_buffer, AudioBuffer<float>& output_buffer, double sample_rate) noexcept {
    assert(output_buffer.n_samples == audio_buffer_size && output_buffer.n_channels == num_output_channels);
    assert(sample_rate == (double)audio_sample_rate);
    (void)sample_rate;
    const wbx_status st =
        input_buffer.n_channels != 0
            ? wbx_engine_process_in(h, input_buffer.channel_buffers, input_buffer.n_channels, output_buffer.channel_buffers)
            : wbx_engine_process(h, output_buffer.channel_buffers);
    if (st != WBX_OK) {
      output_buffer.clear();
      process_error = wbx_engine_last_error(h);
      process_status.store(st, std::memory_order_release);
    }
  }
  // process() and the back end's output_buffer.interleave_samples_to(dst, 0, audio_buffer_size, format)
  // (audio_io_pulseaudio.cpp:419-461, audio_buffer.h:143-160) in one call: the device-format conversion of
  // core/audio_format_conv.cpp runs on the GPU as the last step of the block.  Never throws (see process()).
  void process_interleaved(void* dst, AudioFormat format) noexcept {
    const wbx_status st = wbx_engine_process_interleaved(h, static_cast<int>(format), dst);
    if (st != WBX_OK) {
      const size_t eb = format == AudioFormat::I16 ? 2 : format == AudioFormat::I24 ? 3 : 4;
      std::memset(dst, 0, (size_t)audio_buffer_size * num_output_channels * eb);
      process_error = wbx_engine_last_error(h);
      process_status.store(st, std::memory_order_release);
    }
  }
  // UI thread, once per frame before the host's meters decay (Track::level_meter[c].take_level()): the running per-track maxima the GPU kept since
  // the last call (VUMeter::push_samples, vu_meter.h:20-30) go into the tracks' meters
  void fetch_levels() {
    if (tracks.empty()) return;
    std::vector<float> lv(tracks.size() * num_output_channels);
    check(wbx_engine_levels(h, lv.data(), (uint32_t)tracks.size()), "fetch_levels");
    for (size_t t = 0; t < tracks.size(); t++)
      for (uint32_t c = 0; c < num_output_channels && c < 2; c++) tracks[t]->level_meter[c].push_level(lv[t * num_output_channels + c]);
  }
  // Engine::add_plugin_to_track / delete_plugin_from_track (engine.h:227-229): the slot exists, processing through it
  // is PluginResult::Unimplemented — returns nullptr like the reference does when a plugin cannot be opened
  const wbx_plugin* add_plugin_to_track(Track* track, const wbx_plugin* plugin) {
    if (wbx_engine_add_plugin_to_track(h, track->index, plugin) != WBX_OK) return nullptr;
    track->plugin_instance = nullptr;
    return nullptr;
  }
  void delete_plugin_from_track(Track* track) {
    check(wbx_engine_delete_plugin_from_track(h, track->index), "delete_plugin_from_track");
    track->plugin_instance = nullptr;
  }
  void check(wbx_status s, const char* where) const {
    if (s != WBX_OK) throw Error(s, std::string(where) + ": " + (h ? wbx_engine_last_error(h) : wbx_status_string(s)));
  }
};

inline void Track::set_volume(float db) { engine->check(wbx_track_set_volume(engine->h, index, db), "Track::set_volume"); }
inline void Track::set_pan(float pan) { engine->check(wbx_track_set_pan(engine->h, index, pan), "Track::set_pan"); }
inline void Track::set_mute(bool mute) { engine->check(wbx_track_set_mute(engine->h, index, mute ? 1 : 0), "Track::set_mute"); }

}  // namespace wbx
