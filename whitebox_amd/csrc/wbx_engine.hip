// wbx_engine.hip — layer 2 of libwbx.so (wbx_engine): the reference's Engine / Track surface.
//
// The host keeps what the UI thread edits (clip lists, parameters, transport: wbx_host.h, plain C++ shared with the
// CPU-only test harness), the device keeps what the audio thread mutates per block (sequencer + sampler state) and does
// all per-block work.  Threading is the reference's (wbx_host.h): one audio thread in wbx_engine_process / _render
// holding the editor lock for its host side, one UI thread whose edits take the same lock and whose
// wbx_track_set_volume / _pan / _mute go through the per-track SPSC ring without it.
#include <chrono>
#include <condition_variable>
#include <thread>

#include "wbx_ctx.h"
#include "wbx_host.h"
#include "wbx_seq.h"

using namespace wbx;

struct wbx_engine {
  wbx_ctx* ctx = nullptr;
  HostSession hs;
  EngineKnobs knobs;                    // WBX_PLAN_SEG / WBX_PLAN_LANES, read once at wbx_engine_create (wbx_knobs.h)
  // pinned host buffers the plan kernel reads in place (one 16-B / 8-B read per lane): state patches and per-track
  // gains reach the device without a copy and, above all, without a stream synchronisation that would drain the
  // renders the audio thread has run ahead by.  Rings of three; a buffer is refilled only after the plan kernel that
  // last read it has finished (PinnedSlot, wbx_res.h: wait before the refill, mark behind the plan).
  PinnedSlot<DPatch> patch[kRing];
  uint32_t patch_seq = 0;
  PinnedSlot<float> gains[kRing];       // [N][2] fl(volume * pan_coeffs[c])
  uint32_t tables_cap = 0;              // tracks all six buffers hold (ensure_pinned_tables grows them together)
  int gains_slot = -1;                  // the buffer plans currently read
  std::vector<float> gains_tmp;
  // the one-block callback reads the gains from a device copy (refreshed, in stream order, only when a parameter changed):
  // a read of pinned host memory is the longest round trip in its sequencer's latency chain
  DevBuf<float> d_gains_cb;
  uint64_t gains_gen = 0, d_gains_cb_gen = ~0ull;   // how often the pinned gains were rebuilt / which build the copy mirrors
  // the per-block transport records of a batch render (PlanArgs::times): K dependent additions, done here on the host — it
  // repeats that arithmetic anyway to keep its own transport — and moved in front of the plan by a kernel that reads this
  // pinned table (one lane of the GPU beside a running mix took 0.15-0.2 ms for 2048 blocks).  A ring of eight: the host
  // runs at most that many renders ahead of the sequencer before it waits for a table's copy.
  static constexpr int kTimesRing = 8;
  PinnedSlot<DBlockTime> times[kTimesRing];   // (each grown by the render that needs it larger)
  uint32_t times_seq = 0;
  // Engine::process (one block per call): pinned, device-mapped host staging the sum kernel writes the block into
  // and the plan status lands in — the callback path then needs no copy-engine transfer at all
  PinnedBuf<float> h_block;             // [C][F]
  PinnedBuf<uint32_t> h_status;         // kStatusWords: plan counters [0..4); the one-launch callback's give-up word [7] and
                                        // completion word [8], each holding the sequence number of the launch that wrote it
  static constexpr uint32_t kStatusWords = 9;
  uint32_t cb_seq = 0;                  // ... of the last launch
  uint32_t cb_give_ups = 0;             // one-launch callbacks mixed again because a workgroup gave up at the spread barrier
  bool plan_status_on_host = false;     // the counters of the last plan are in h_status (the device copy was cleared)
  size_t d_clips_count = 0;
  bool clips_uploaded = false;          // the device holds a clip table (its internal_state_changed flags are live)
  // the sequencer cut along the time axis (wbx_seq.h plan_segment): seam states of the render being planned — one buffer, the
  // two plan kernels that use it run back to back on one stream — and its running statistics
  DevBuf<DTrackState> d_seam;           // [2][N][segments]: guesses, end states
  DevBuf<uint32_t> d_seg_stats;         // [2] tracks with a seam that did not hold, segments planned again
  DevBuf<uint32_t> d_seg_ticket;        // [max_tracks] SegArgs::ticket (all zero between launches)
  hipStream_t seam_stream = nullptr;    // the stream that used d_seam last
  Event seam_done;
  bool table_flags = false;             // the uploaded clip table holds a set internal_state_changed flag (segmented plans off)
  PinnedBuf<uint32_t> h_flags_left;     // pinned: how many of them are left — the sequencer counts down as it clears them
  uint64_t seg_renders = 0;             // renders planned by segments so far
  uint32_t seg_last_segs = 0;           // ... segments per track of the last one
  uint32_t state_tracks = 0;            // tracks that have device state
  std::vector<DClip> flat;              // staging of the clip table upload
  std::vector<uint32_t> first;

  DevBuf<DClip> d_clips;
  DevBuf<uint32_t> d_clip_first;
  // [max_tracks], allocated once by the first render.  Invariant: the slots from state_tracks on are all-zero (a track
  // added later starts from cleared state without any device work: no allocation, no copy, no synchronisation on the
  // audio thread).  permute_tracks_locked keeps it.
  DevBuf<DTrackState> d_state;
  DevBuf<float> d_levels;               // [max_tracks][2] running maxima, same invariant
  // wbx_engine_levels (UI thread): the take kernel runs on a stream of its own into this pinned block; the editor lock
  // is held only while the take is ENQUEUED behind the renders in flight, never across the wait for it
  Stream levels_stream;
  Event levels_ev;
  // the sequencer of render n+1 continues from the per-track state render n's left: on one stream that is the stream's
  // order; when the stream changes (short renders plan on the main stream, batch renders on the plan stream) the new one
  // waits for this event, recorded at the old one's tail
  hipStream_t last_plan_stream = nullptr;
  Event plan_handover;
  PinnedBuf<uint32_t> h_levels;         // [max_tracks][2]

  // ---- recording (wbx_engine_record ... ; semantics in wbx_host.h, HostSession::takes) ----
  // A take is a table of chunks of the clip pool (F32, rec_chunk frames, zeroed when taken) in HBM.  The audio thread copies
  // each played block's input into a pinned staging slot and launches record_capture_kernel on the upload stream, which
  // writes it into the chunks by absolute frame; the engine's recorder thread keeps rec_spare chunks ahead of every take's
  // write position; stop_record gathers the chunks into one clip.
  static constexpr int kRecSlots = 8;
  uint32_t rec_chunk = 65536, rec_spare = 2;   // wbx_engine_set_record_chunk (audio_record_chunk_size / 4, engine.h:36)
  struct RecTake {
    std::vector<ClipSlot> chunks;              // the recorder thread's while the take runs (under rec_mu)
    uint32_t channels = 1;
    bool discarded = false;                    // its track went (rec_discard_takes_locked): no chunks, none to come (under rec_mu)
    std::atomic<uint32_t> ready{0};            // chunks whose table entry is enqueued ahead of any capture that uses it
  };
  std::unique_ptr<RecTake[]> rec_takes;
  uint32_t rec_n = 0, rec_table_cap = 0, rec_in_ch = 0, rec_F = 0;
  DevBuf<RecChunk> d_rec_table;                // [rec_n][rec_table_cap]
  PinnedBuf<RecChunk> h_rec_table;             // pinned source of the table writes, same shape
  PinnedBuf<uint32_t> h_rec_stage;             // pinned [kRecSlots][rec_slot_words]: samples, then the take descriptors
  size_t rec_slot_words = 0;
  PinnedSlot<uint32_t> rec_stage[kRecSlots];   // slot i is h_rec_stage + i * rec_slot_words (one allocation: their own buffers
                                               // stay empty); done: the capture that read the slot last
  uint32_t rec_slot = 0;
  std::thread rec_thread;
  std::atomic<bool> rec_run{false};
  std::atomic<uint64_t> rec_written{0};        // frames of the takes the audio thread has dealt with (all takes alike)
  std::mutex rec_mu;                           // the recorder thread's sleep, and every take's chunk list while that thread runs
  std::condition_variable rec_cv;
  std::atomic<wbx_status> rec_thread_err{WBX_OK};
  uint64_t rec_captures = 0;                   // capture launches so far (diagnostic)
  // wbx_engine_export_sample: the sample an export in flight reads (under the editor lock; one export at a time,
  // wbx_ctx::export_mu) — wbx_engine_delete_sample refuses it until the export is over
  static constexpr uint32_t kNoExport = ~0u;
  uint32_t export_pin = kNoExport;
  // wbx_engine_measure_sample / derive_sample / normalize_sample: the source of the edit in flight (under the editor lock;
  // one edit at a time, wbx_ctx::fx_mu), refused by wbx_engine_delete_sample in the same way
  uint32_t edit_pin = kNoExport;
  // wbx_engine_splice_samples: every distinct source of the splice in flight (same lock, same mutex, refused the same way)
  std::vector<uint32_t> edit_pins;
};

namespace {

// The message of the last failed engine call made by the CALLING thread: the UI thread and the audio thread fail
// independently, one shared string would be a data race.
thread_local std::string tls_err;

wbx_status efail(wbx_engine*, wbx_status s, const char* what) {
  tls_err = what;
  return s;
}

// a failed layer-1 call made under the lock: take its message along
wbx_status cfail(wbx_engine* e, wbx_status s) {
  if (s != WBX_OK) tls_err = e->ctx->err;
  return s;
}

#define WBX_EHIP(e, call)                                           \
  do {                                                              \
    hipError_t _e = (call);                                         \
    if (_e != hipSuccess) {                                         \
      tls_err = std::string(#call) + ": " + hipGetErrorString(_e);  \
      return WBX_ERR_DEVICE;                                        \
    }                                                               \
  } while (0)

// a step that has left its own message behind
#define WBX_STEP(call)                  \
  do {                                  \
    const wbx_status _s = (call);       \
    if (_s != WBX_OK) return _s;        \
  } while (0)

bool sample_in_use_cb(void* owner, uint32_t sample) { return static_cast<wbx_engine*>(owner)->hs.sample_referenced(sample); }

}  // namespace

extern "C" wbx_status wbx_engine_create(const wbx_config* cfg, wbx_engine** out) {
  if (!cfg || !out) return WBX_ERR_INVALID;
  *out = nullptr;
  wbx_ctx* c = nullptr;
  wbx_status st = wbx_create(cfg, &c);
  if (st != WBX_OK) return st;
  wbx_engine* e = new (std::nothrow) wbx_engine();
  if (!e) {
    wbx_destroy(c);
    return WBX_ERR_OOM;
  }
  e->ctx = c;
  e->hs.max_tracks = cfg->max_tracks;
  e->hs.dst_rate = cfg->sample_rate;
  e->knobs = EngineKnobs::from_env();
  e->hs.plan_lanes_knob = e->knobs.plan_lanes;
  c->owner = e;
  c->sample_in_use = sample_in_use_cb;
  if (e->levels_stream.create(hipStreamNonBlocking) != hipSuccess || e->levels_ev.ensure(kDevEventFlags) != hipSuccess ||
      e->h_levels.ensure((size_t)cfg->max_tracks * 2) != hipSuccess) {
    wbx_engine_destroy(e);
    return WBX_ERR_OOM;
  }
  *out = e;
  return WBX_OK;
}

namespace {
void rec_release(wbx_engine* e);
void rec_discard_takes_locked(wbx_engine* e);
}

// The waits, then the engine's own holders (they go with `delete e`), then the context's: the engine's pinned tables and
// events are used by work on the context's streams, so they are dropped first and the streams last.
extern "C" void wbx_engine_destroy(wbx_engine* e) {
  if (!e) return;
  wbx_ctx* c = e->ctx;
  if (c) {
    (void)hipSetDevice(c->cfg.device);
    rec_release(e);   // a take still running is discarded
    (void)hipStreamSynchronize(c->plan_stream);
    (void)sync_main(c);
  }
  if (e->levels_stream) (void)hipStreamSynchronize(e->levels_stream);
  delete e;
  wbx_destroy(c);
}

// Engine::set_audio_channel_config (engine.cpp:43-57) on a live engine: new block size / channel count / device rate,
// tracks, clips, samples and the transport stay — like the reference, which only resizes its mixing buffers.  Sampler
// state of clips that are playing keeps the playback speed it was started with (Sampler::reset_state ran with the
// old rate), as in the reference.
extern "C" wbx_status wbx_engine_set_audio_channel_config(wbx_engine* e, uint32_t output_channels, uint32_t buffer_size,
                                                          uint32_t sample_rate) {
  if (!e) return WBX_ERR_INVALID;
  if (output_channels < 1 || output_channels > 2 || buffer_size < 4 || (buffer_size & 3u) || buffer_size > 32768 || sample_rate == 0)
    return efail(e, WBX_ERR_INVALID, "set_audio_channel_config: channels 1-2, buffer size a multiple of 4 up to 32768");
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  wbx_ctx* c = e->ctx;
  if (c->cfg.channels == output_channels && c->cfg.block_frames == buffer_size && c->cfg.sample_rate == sample_rate) return WBX_OK;
  if (c->dist) return efail(e, WBX_ERR_UNSUPPORTED, "set_audio_channel_config: shut the multi-GPU exchange down first (its buffers have the old shape)");
  if (e->hs.recording) return efail(e, WBX_ERR_UNSUPPORTED, "set_audio_channel_config: not while recording (stop_record first)");
  (void)hipSetDevice(c->cfg.device);
  WBX_EHIP(e, hipStreamSynchronize(c->plan_stream));
  WBX_EHIP(e, join_sum(c));
  WBX_EHIP(e, hipStreamSynchronize(c->sum_stream));
  WBX_EHIP(e, sync_main(c));
  WBX_EHIP(e, hipStreamSynchronize(e->levels_stream));   // (a meter read in flight: d_levels is cleared below)
  drain_events(c);
  c->cfg.channels = output_channels;
  c->cfg.block_frames = buffer_size;
  c->cfg.sample_rate = sample_rate;
  // everything whose size or row pitch depends on C or F is dropped and re-grown by the next render
  for (auto& B : c->pb) {
    B.rows.release();
    B.gen_list.release();
    B.saved.release();
    B.gen_cap = 0;
    B.consumed_valid = false;
  }
  for (auto& P : c->d_partial2) P.release();
  for (auto& v : c->sum_valid) v = false;
  c->sum_pending = -1;
  c->d_master.release();
  c->d_buses.release();
  for (auto& P : c->d_peaks) P.release();
  c->buses_clean = false;
  c->d_zero.release();
  WBX_EHIP(e, c->d_zero.ensure(buffer_size + 8));
  WBX_EHIP(e, hipMemset(c->d_zero.p, 0, (buffer_size + 8) * sizeof(float)));
  c->last_K = 0;
  e->h_block.release();
  if (e->d_levels.p) WBX_EHIP(e, hipMemset(e->d_levels.p, 0, e->d_levels.cap * sizeof(float)));
  // the destination rate enters every clip's playback speed: which clips the hot loop streams directly is re-derived
  e->hs.set_dst_rate_locked(sample_rate);
  return WBX_OK;
}

extern "C" const char* wbx_engine_last_error(const wbx_engine* e) {
  if (!e) return "null engine";
  return tls_err.c_str();
}

extern "C" wbx_ctx* wbx_engine_ctx(wbx_engine* e) { return e ? e->ctx : nullptr; }

extern "C" wbx_status wbx_engine_set_bpm(wbx_engine* e, double bpm) {   // engine.cpp:24-30: an atomic store, no lock
  if (!e || !(bpm > 0.0)) return WBX_ERR_INVALID;
  e->hs.set_bpm(bpm);
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_set_playhead_position(wbx_engine* e, double beat) {   // engine.cpp:32-41
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.set_playhead_position_locked(beat);
  e->hs.note_edit_locked();
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_add_track(wbx_engine* e, uint32_t* track_out) {   // engine.cpp:200-208
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (e->hs.n_tracks() >= e->ctx->cfg.max_tracks) return efail(e, WBX_ERR_INVALID, "max_tracks reached");
  const uint32_t t = e->hs.add_track_locked();
  if (track_out) *track_out = t;
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_set_buses(wbx_engine* e, uint32_t n_buses) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.n_buses = n_buses;
  e->hs.routing_dirty = true;
  e->hs.note_edit_locked();
  return WBX_OK;
}

// Track::set_volume / set_pan / set_mute (track.cpp:47-79): UI thread, no lock — a message into the track's ring,
// applied by the audio thread at the start of its next block.  Like the reference's, the producer yields while the
// ring (63 usable entries) is full: it needs a running audio thread to make progress then.
extern "C" wbx_status wbx_track_set_volume(wbx_engine* e, uint32_t t, float db) {
  if (!e || !e->hs.valid_track(t)) return WBX_ERR_INVALID;
  e->hs.set_volume(t, db);
  return WBX_OK;
}

extern "C" wbx_status wbx_track_set_pan(wbx_engine* e, uint32_t t, float pan) {
  if (!e || !e->hs.valid_track(t)) return WBX_ERR_INVALID;
  e->hs.set_pan(t, pan);
  return WBX_OK;
}

extern "C" wbx_status wbx_track_set_mute(wbx_engine* e, uint32_t t, int mute) {
  if (!e || !e->hs.valid_track(t)) return WBX_ERR_INVALID;
  e->hs.set_mute(t, mute != 0);
  return WBX_OK;
}

namespace {

// new track i = old track order[i] (order.size() = new track count): the per-track device state (sequencer,
// sampler, running levels) follows its Track object, as the pointers in the reference's vector do
wbx_status permute_tracks_locked(wbx_engine* e, const std::vector<uint32_t>& order) {
  wbx_ctx* c = e->ctx;
  (void)hipSetDevice(c->cfg.device);
  WBX_EHIP(e, hipStreamSynchronize(c->plan_stream));
  WBX_EHIP(e, join_sum(c));
  WBX_EHIP(e, sync_main(c));
  // (a meter read of the UI thread may still be in flight on its own stream — wbx_engine_levels drops the editor lock
  //  before it waits: its exchange-with-zero must not land in the slots rewritten below)
  WBX_EHIP(e, hipStreamSynchronize(e->levels_stream));
  const uint32_t new_n = (uint32_t)order.size();
  if (e->state_tracks) {
    const uint32_t C = c->cfg.channels;
    std::vector<DTrackState> st(e->state_tracks), st2(std::max<size_t>(new_n, 1));
    std::vector<float> lv((size_t)e->state_tracks * C), lv2((size_t)std::max<uint32_t>(new_n, 1) * C, 0.0f);
    WBX_EHIP(e, hipMemcpy(st.data(), e->d_state.p, st.size() * sizeof(DTrackState), hipMemcpyDeviceToHost));
    WBX_EHIP(e, hipMemcpy(lv.data(), e->d_levels.p, lv.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < new_n; i++) {
      if (order[i] < e->state_tracks) {
        st2[i] = st[order[i]];
        for (uint32_t ch = 0; ch < C; ch++) lv2[(size_t)i * C + ch] = lv[(size_t)order[i] * C + ch];
      } else {
        st2[i] = DTrackState{};   // a track added since the last render
      }
    }
    WBX_EHIP(e, hipMemset(e->d_state.p, 0, e->d_state.cap * sizeof(DTrackState)));
    WBX_EHIP(e, hipMemset(e->d_levels.p, 0, e->d_levels.cap * sizeof(float)));
    if (new_n) {
      WBX_EHIP(e, hipMemcpy(e->d_state.p, st2.data(), (size_t)new_n * sizeof(DTrackState), hipMemcpyHostToDevice));
      WBX_EHIP(e, hipMemcpy(e->d_levels.p, lv2.data(), (size_t)new_n * C * sizeof(float), hipMemcpyHostToDevice));
    }
    e->state_tracks = new_n;
  }
  e->hs.permute_tracks_locked(order);
  rec_discard_takes_locked(e);   // a recording track that went: its take's chunks go back to the pool now
  return WBX_OK;
}

}  // namespace

extern "C" wbx_status wbx_engine_delete_track(wbx_engine* e, uint32_t slot) {   // engine.cpp:210-218
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(slot)) return WBX_ERR_INVALID;
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < e->hs.n_tracks(); i++)
    if (i != slot) order.push_back(i);
  return permute_tracks_locked(e, order);
}

extern "C" wbx_status wbx_engine_clear_all(wbx_engine* e) {   // engine.cpp:59-66: every track goes
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  return permute_tracks_locked(e, std::vector<uint32_t>{});
}

extern "C" wbx_status wbx_engine_move_track(wbx_engine* e, uint32_t from_slot, uint32_t to_slot) {   // engine.cpp:228-243
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(from_slot) || !e->hs.valid_track(to_slot)) return WBX_ERR_INVALID;
  if (from_slot == to_slot) return WBX_OK;
  std::vector<uint32_t> order(e->hs.n_tracks());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  order.erase(order.begin() + from_slot);
  order.insert(order.begin() + to_slot, from_slot);
  return permute_tracks_locked(e, order);
}

extern "C" wbx_status wbx_engine_solo_track(wbx_engine* e, uint32_t slot) {   // engine.cpp:245-262 (no lock: messages only)
  if (!e || !e->hs.valid_track(slot)) return WBX_ERR_INVALID;
  e->hs.solo_track(slot);
  return WBX_OK;
}

extern "C" wbx_status wbx_track_set_bus(wbx_engine* e, uint32_t t, int32_t bus) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(t)) return WBX_ERR_INVALID;
  e->hs.tracks[t]->bus = bus;
  e->hs.routing_dirty = true;
  return WBX_OK;
}

// ---- effect slot: kept in the boundary, nothing processed through it ----
extern "C" wbx_status wbx_engine_add_plugin_to_track(wbx_engine* e, uint32_t track, const wbx_plugin* plugin) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  if (plugin)
    return efail(e, WBX_ERR_UNIMPLEMENTED, "effect processing is not part of this path (third-party VST3 arithmetic): the slot stays empty");
  e->hs.tracks[track]->plugin = nullptr;
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_delete_plugin_from_track(wbx_engine* e, uint32_t track) {   // engine.h:229
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  e->hs.tracks[track]->plugin = nullptr;
  return WBX_OK;
}

extern "C" wbx_status wbx_track_get_plugin(wbx_engine* e, uint32_t track, const wbx_plugin** plugin_out) {
  if (!e || !plugin_out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  *plugin_out = static_cast<const wbx_plugin*>(e->hs.tracks[track]->plugin);
  return WBX_OK;
}

namespace {

// Sample assets (SampleAsset, engine/assets_table.h:22-35).  The reference decodes a file outside the editor lock and
// only links the finished asset in; here the id is reserved under the lock, the audio goes to HBM on the upload
// stream without it, and the finished slot is published under the lock again — the audio thread never waits for a
// transfer.
wbx_status add_sample_common(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames,
                             const ClipFill& f, uint32_t* sample_out) {
  if (!e || !sample_out) return WBX_ERR_INVALID;
  wbx_ctx* c = e->ctx;
  uint32_t id;
  {
    LockGuard g(e->hs.editor_lock);
    id = (uint32_t)c->clips.size();
    c->clips.emplace_back();            // reserved, unused until published
    e->hs.samples.resize(c->clips.size());
  }
  ClipSlot s;
  wbx_status st = clip_build(c, s, format, channels, sample_rate, frames, f, c->upload_stream);
  if (st == WBX_OK && hipStreamSynchronize(c->upload_stream) != hipSuccess) {
    clip_release(c, s);
    st = WBX_ERR_DEVICE;
  }
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (st != WBX_OK) return cfail(e, st);
  st = clip_publish(c, id, s);
  if (st != WBX_OK) return cfail(e, st);
  SampleMeta& m = e->hs.samples[id];
  m.format = (uint32_t)format;
  m.channels = channels;
  m.sample_rate = sample_rate;
  m.count = frames;
  m.used = true;
  *sample_out = id;
  return WBX_OK;
}

}  // namespace

extern "C" wbx_status wbx_engine_add_sample(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate,
                                            uint64_t frames, const void* const* planar, uint32_t* sample_out) {
  ClipFill f{};
  f.kind = CLIP_SRC_PLANAR;
  f.planar = planar;
  return add_sample_common(e, format, channels, sample_rate, frames, f, sample_out);
}

extern "C" wbx_status wbx_engine_add_sample_interleaved(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate,
                                                        uint64_t frames, const void* interleaved, uint32_t* sample_out) {
  ClipFill f{};
  f.kind = CLIP_SRC_INTERLEAVED_HOST;
  f.interleaved = interleaved;
  return add_sample_common(e, format, channels, sample_rate, frames, f, sample_out);
}

extern "C" wbx_status wbx_engine_add_sample_synth(wbx_engine* e, int format, uint32_t channels, uint32_t sample_rate,
                                                  uint64_t frames, uint64_t seed, uint32_t key_track, float amp,
                                                  uint32_t* sample_out) {
  ClipFill f{};
  f.kind = CLIP_SRC_SYNTH;
  f.seed = seed;
  f.key_track = key_track;
  f.amp = amp;
  return add_sample_common(e, format, channels, sample_rate, frames, f, sample_out);
}

// Drop a sample asset (SampleAsset::release when its last reference goes, assets_table.h:22-35): refused while a clip
// list still names it.  The engine-side form of wbx_clip_free: it takes the editor lock.
extern "C" wbx_status wbx_engine_delete_sample(wbx_engine* e, uint32_t sample) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_sample(sample)) return efail(e, WBX_ERR_INVALID, "unknown sample");
  // the edit pin first: it passes by itself, and a caller told to delete the clips first would do so only to be refused again
  if (e->edit_pin == sample || std::find(e->edit_pins.begin(), e->edit_pins.end(), sample) != e->edit_pins.end())
    return efail(e, WBX_ERR_UNSUPPORTED, "sample is being edited (a measure, derive or normalize call is still reading it)");
  if (e->hs.sample_referenced(sample)) return efail(e, WBX_ERR_INVALID, "sample is still referenced by a clip (delete the clips first)");
  if (e->export_pin == sample) return efail(e, WBX_ERR_UNSUPPORTED, "sample is being exported (wbx_engine_export_sample is still reading it)");
  const wbx_status st = wbx_clip_free(e->ctx, sample);
  if (st != WBX_OK) return cfail(e, st);
  e->hs.samples[sample] = SampleMeta{};
  return WBX_OK;
}

// Side calls on engine samples: wbx_engine_export_sample (wbx_clip_export; wbx.h), and measuring and editing them (the
// wbx_clip_* calls of wbx.h "Editing clips" and after, each on an engine sample).  Editing thread; the audio thread may be
// in wbx_engine_process* all the while.  Nothing here touches the transport or counts as an edit (no note_edit_locked): a
// render sees a new sample only once a clip names it.  Every entry point is the same pinned call, written once in
// SamplePin below; what stands in an entry point is what is its own: the call struct, the samples it names, its check, its
// run and, for a producer, what the new sample is registered as.
namespace {

// (editor lock held) `slot` becomes the pool's next sample, an F32 one, known to the session's sample table
wbx_status register_sample_locked(wbx_engine* e, ClipSlot& slot, uint32_t channels, uint32_t rate, uint64_t frames, uint32_t* id) {
  wbx_ctx* c = e->ctx;
  const uint32_t next = (uint32_t)c->clips.size();
  const wbx_status st = clip_publish(c, next, slot);
  if (st != WBX_OK) return st;
  if (e->hs.samples.size() < c->clips.size()) e->hs.samples.resize(c->clips.size());
  e->hs.samples[next] = SampleMeta{WBX_FMT_F32, channels, rate, frames, true};
  *id = next;
  return WBX_OK;
}

// One pinned call on engine samples: THE statement of its rules.
//   * The call's mutex — export_mu for an export, fx_mu for everything else — is held for the object's life: one call
//     at a time on its side stream.  hipSetDevice happens on entry.
//   * begin() is the locked half.  Under the editor lock: the sample is validated and its storage description copied out
//     (the pool's table may be reallocated by a later add_sample), check(&msg) judges the call (no device call; it looks
//     up and copies out further samples through slot_locked()), a producer is refused where the pool's 2^24 ids would run
//     out, and only then the pin is written — export_pin or edit_pin, or for a call of several samples the set
//     edit_pins — against wbx_engine_delete_sample.  A refusal pins nothing and goes through efail.
//   * What needs the heap is made by the caller BEFORE begin() and freed after the lock is released: the distinct ids
//     of a set (begin() swaps them in, the destructor swaps them out again).
//   * read() and make() are the unlocked half: the side stream and its staging are created without the lock, the stream is
//     ordered behind what is enqueued under it, and run() — kernels, device waits, host copies, a new clip's allocation —
//     works without it: the editor lock is NEVER held across a device wait (the rule of wbx_engine_levels, what the
//     *_beside_the_audio_thread tests hold).  make() then registers the new sample under the lock.  A failure's text goes
//     to tls_err.  A call may run more than once under its one pin (the normalizations measure, then derive).
//   * The destructor drops the pin on every path out.
struct SamplePin {
  using Step = wbx_status(wbx_ctx*, std::string*);
  wbx_engine* e;
  std::lock_guard<std::mutex> one;
  uint32_t wbx_engine::* word;
  Step *prepare, *order_side;
  bool pinned = false, pinned_set = false;
  ClipSrc src;
  uint32_t rate = 0;
  enum Side { kEdit, kExport };
  explicit SamplePin(wbx_engine* e_, Side side = kEdit)
      : e(e_), one(side == kExport ? e_->ctx->export_mu : e_->ctx->fx_mu),
        word(side == kExport ? &wbx_engine::export_pin : &wbx_engine::edit_pin),
        prepare(side == kExport ? export_prepare : clipfx_prepare), order_side(side == kExport ? export_order : clipfx_order) {
    (void)hipSetDevice(e->ctx->cfg.device);
  }
  ~SamplePin() {
    if (!pinned && !pinned_set) return;
    std::vector<uint32_t> gone;                            // (the set's storage is freed after the lock)
    LockGuard g(e->hs.editor_lock);
    if (pinned) e->*word = wbx_engine::kNoExport;
    if (pinned_set) gone.swap(e->edit_pins);
  }
  // (editor lock held) a sample's slot in the pool, null for an id that names none
  const ClipSlot* slot_locked(uint32_t id) const { return e->hs.valid_sample(id) ? find_clip(e->ctx, id) : nullptr; }
  // `unknown`: what an id that names no sample is told (null: the call names its samples in its check alone, a splice);
  // `full`: what a producer is told where the ids would run out (null: a measurer); `set`: the distinct ids to pin (null:
  // `sample` alone)
  template <class Check>
  wbx_status begin(uint32_t sample, const char* unknown, const char* full, std::vector<uint32_t>* set, Check&& check) {
    LockGuard g(e->hs.editor_lock);
    if (unknown) {
      const ClipSlot* s = slot_locked(sample);
      if (!s) return efail(e, WBX_ERR_INVALID, unknown);
      src = clip_src(*s);
      rate = s->d.sample_rate;
    }
    const char* msg = "";
    const wbx_status st = check(&msg);
    if (st != WBX_OK) return efail(e, st, msg);
    if (full && e->ctx->clips.size() >= (1u << 24)) return efail(e, WBX_ERR_OVERFLOW, full);
    if (set) {
      e->edit_pins.swap(*set);
      pinned_set = true;
    } else {
      e->*word = sample;
      pinned = true;
    }
    return WBX_OK;
  }
  // a run that makes no sample: run(&why)
  template <class Run>
  wbx_status read(Run&& run) {
    std::string why;
    wbx_status st = order(&why);
    if (st == WBX_OK) st = run(&why);
    if (st != WBX_OK) tls_err = why;
    return st;
  }
  // a run that fills a new clip, run(slot, &why), which becomes the pool's next sample of `channels` x `frames` at `new_rate`
  template <class Run>
  wbx_status make(uint32_t channels, uint32_t new_rate, uint64_t frames, uint32_t* new_sample, Run&& run) {
    ClipSlot slot;
    return read([&](std::string* why) {
      wbx_status st = run(slot, why);
      if (st != WBX_OK) return st;
      LockGuard g(e->hs.editor_lock);
      st = register_sample_locked(e, slot, channels, new_rate, frames, new_sample);
      if (st != WBX_OK) *why = e->ctx->err;
      return st;
    });
  }

 private:
  wbx_status order(std::string* why) {                     // the side stream: made without the lock, ordered under it
    const wbx_status st = prepare(e->ctx, why);
    if (st != WBX_OK) return st;
    LockGuard g(e->hs.editor_lock);
    return order_side(e->ctx, why);
  }
};

// the ids a call of two samples pins, made before the lock: one id where both are the same sample
std::vector<uint32_t> distinct_pair(uint32_t a, uint32_t b) {
  std::vector<uint32_t> ids{a};
  if (b != a) ids.push_back(b);
  return ids;
}

// what derive_sample and the two normalizations end in: the range derived by `d`, registered at the source's rate
wbx_status derive_pinned(SamplePin& p, const wbx_clip_edit_desc& d, uint32_t out_channels, uint32_t* new_sample) {
  return p.make(out_channels, p.rate, d.n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return clipfx_derive_run(p.e->ctx, p.src, p.rate, d, out_channels, slot, nullptr, why);
  });
}

}  // namespace

// the one call on the export's mutex, pin and stream
extern "C" wbx_status wbx_engine_export_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                               int out_format, uint32_t flags, void* dst, wbx_export_stats* stats) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e, SamplePin::kExport);
  const wbx_status st = p.begin(sample, "export: unknown sample", nullptr, nullptr, [&](const char** msg) {
    return export_check(p.src, first_frame, n_frames, out_format, flags, dst, msg);
  });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return export_run(e->ctx, p.src, first_frame, n_frames, out_format, flags, dst, stats, why); });
}

extern "C" wbx_status wbx_engine_measure_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                wbx_clip_stats* stats) {
  if (!e) return WBX_ERR_INVALID;
  if (!stats) return efail(e, WBX_ERR_INVALID, "measure_sample: stats is NULL");
  SamplePin p(e);
  const wbx_status st = p.begin(sample, "measure_sample: unknown sample", nullptr, nullptr,
                                [&](const char** msg) { return clipfx_check_range(p.src, first_frame, n_frames, msg); });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return clipfx_measure_run(e->ctx, p.src, first_frame, n_frames, stats, why); });
}

extern "C" wbx_status wbx_engine_derive_sample(wbx_engine* e, uint32_t sample, const wbx_clip_edit_desc* desc, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "derive_sample: new_sample is NULL");
  SamplePin p(e);
  uint32_t out_channels = 0;
  const wbx_status st = p.begin(sample, "derive_sample: unknown sample", "derive_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) { return clipfx_check_derive(p.src, desc, &out_channels, msg); });
  if (st != WBX_OK) return st;
  return derive_pinned(p, *desc, out_channels, new_sample);
}

// two runs under one pin: the range's peak, then the range derived at target_peak over it
extern "C" wbx_status wbx_engine_normalize_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                  float target_peak, uint32_t* new_sample, float* gain_used) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "normalize_sample: new_sample is NULL");
  SamplePin p(e);
  wbx_clip_edit_desc d{};
  d.first_frame = first_frame;
  d.n_frames = n_frames;
  d.channel_mode = WBX_CH_KEEP;
  uint32_t out_channels = 0;
  wbx_status st = p.begin(sample, "normalize_sample: unknown sample", "normalize_sample: the pool's sample ids (2^24) would run out", nullptr,
                          [&](const char** msg) { return clipfx_check_derive(p.src, &d, &out_channels, msg); });
  if (st != WBX_OK) return st;
  wbx_clip_stats m{};
  st = p.read([&](std::string* why) { return clipfx_measure_run(e->ctx, p.src, first_frame, n_frames, &m, why); });
  if (st != WBX_OK) return st;
  const float peak = out_channels > 1 && m.peak[1] > m.peak[0] ? m.peak[1] : m.peak[0];
  if (!(peak > 0.0f) || !std::isfinite(peak)) return efail(e, WBX_ERR_INVALID, "normalize_sample: the range is silent, or its peak is not finite");
  d.gain = target_peak / peak;   // one IEEE fp32 division (no fast-math in this build)
  st = derive_pinned(p, d, out_channels, new_sample);
  if (st != WBX_OK) return st;
  if (gain_used) *gain_used = d.gain;
  return WBX_OK;
}

// registered at dst_rate, with the conversion's n_out frames
extern "C" wbx_status wbx_engine_resample_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                 uint32_t dst_rate, int quality, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "resample_sample: new_sample is NULL");
  SamplePin p(e);
  ResamplePlan plan;
  uint64_t n_out = 0;
  const wbx_status st = p.begin(sample, "resample_sample: unknown sample", "resample_sample: the pool's sample ids (2^24) would run out",
                                nullptr, [&](const char** msg) {
    return resample_check(p.src, p.rate, first_frame, n_frames, dst_rate, quality, &plan, &n_out, msg);
  });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, dst_rate, n_out, new_sample, [&](ClipSlot& slot, std::string* why) {
    return resample_run(e->ctx, p.src, plan, quality, first_frame, n_frames, n_out, dst_rate, slot, nullptr, why);
  });
}

// registered at the source's rate, with the range's frames and the tail's
extern "C" wbx_status wbx_engine_filter_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                               uint64_t tail_frames, const double* coef, uint32_t n_stages, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "filter_sample: new_sample is NULL");
  SamplePin p(e);
  const wbx_status st = p.begin(sample, "filter_sample: unknown sample", "filter_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) {
    return filter_check_call(p.src, first_frame, n_frames, tail_frames, coef, n_stages, msg);
  });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, n_frames + tail_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return filter_run(e->ctx, p.src, p.rate, first_frame, n_frames, tail_frames, coef, n_stages, slot, nullptr, why);
  });
}

// pins the source and the response; registered at the source's rate, with the check's channels and the window's frames
extern "C" wbx_status wbx_engine_convolve_sample(wbx_engine* e, uint32_t sample, uint32_t ir_sample, uint64_t first_frame,
                                                 uint64_t n_frames, uint64_t ir_first, uint64_t ir_frames, uint64_t out_first,
                                                 uint64_t out_frames, double gain, uint32_t* new_sample, wbx_clip_stats* stats_of_result) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "convolve_sample: new_sample is NULL");
  SamplePin p(e);
  const ConvolveCall k{first_frame, n_frames, ir_first, ir_frames, out_first, out_frames, gain};
  std::vector<uint32_t> distinct = distinct_pair(sample, ir_sample);
  ClipSrc ir;
  uint32_t ch = 0;
  const wbx_status st = p.begin(sample, "convolve_sample: unknown sample", "convolve_sample: the pool's sample ids (2^24) would run out",
                                &distinct, [&](const char** msg) -> wbx_status {
    const ClipSlot* r = p.slot_locked(ir_sample);
    if (!r) return *msg = "convolve_sample: unknown response sample", WBX_ERR_INVALID;
    ir = clip_src(*r);
    return convolve_check(p.src, p.rate, ir, r->d.sample_rate, k, &ch, msg);
  });
  if (st != WBX_OK) return st;
  return p.make(ch, p.rate, out_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return convolve_run(e->ctx, p.src, ir, p.rate, k, slot, stats_of_result, why);
  });
}

// registered at the source's rate, with the range's frames
extern "C" wbx_status wbx_engine_limit_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, float ceiling,
                                              double drive, uint32_t lookahead_frames, uint32_t hold_frames, uint32_t release_frames,
                                              uint32_t* new_sample, wbx_limit_stats* limit_stats, wbx_clip_stats* stats_of_result) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "limit_sample: new_sample is NULL");
  SamplePin p(e);
  const LimitCall k{first_frame, n_frames, ceiling, drive, lookahead_frames, hold_frames, release_frames};
  const wbx_status st = p.begin(sample, "limit_sample: unknown sample", "limit_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) { return limit_check(p.src, k, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return limit_run(e->ctx, p.src, p.rate, k, slot, limit_stats, stats_of_result, why);
  });
}

// registered at the source's rate, with the range's frames
extern "C" wbx_status wbx_engine_saturate_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames, uint32_t os,
                                                 int quality, const double* table, double drive, double makeup, uint32_t* new_sample,
                                                 wbx_saturate_stats* saturate_stats, wbx_clip_stats* stats_of_result) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "saturate_sample: new_sample is NULL");
  SamplePin p(e);
  const SatCall k{first_frame, n_frames, os, quality, table, drive, makeup};
  const wbx_status st = p.begin(sample, "saturate_sample: unknown sample", "saturate_sample: the pool's sample ids (2^24) would run out",
                                nullptr, [&](const char** msg) { return saturate_check(&p.src, false, k, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return saturate_run(e->ctx, p.src, p.rate, k, slot, saturate_stats, stats_of_result, why);
  });
}

// registered at the source's rate, with out_frames frames
extern "C" wbx_status wbx_engine_varispeed_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                  uint64_t out_frames, const int64_t* knots, uint64_t n_knots, uint32_t knot_shift,
                                                  int quality, uint32_t guard_num, uint32_t guard_den, uint32_t* new_sample,
                                                  wbx_clip_stats* stats_of_result) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "varispeed_sample: new_sample is NULL");
  SamplePin p(e);
  const VsCall k{first_frame, n_frames, out_frames, knots, n_knots, knot_shift, quality, guard_num, guard_den};
  VsPlan plan;
  const wbx_status st = p.begin(sample, "varispeed_sample: unknown sample", "varispeed_sample: the pool's sample ids (2^24) would run out",
                                nullptr, [&](const char** msg) { return varispeed_check(&p.src, false, k, &plan, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, out_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return varispeed_run(e->ctx, p.src, p.rate, k, plan, slot, stats_of_result, why);
  });
}

// registered at the source's rate, with the range's frames
extern "C" wbx_status wbx_engine_denoise_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                uint32_t window_frames, uint32_t smooth_hops, uint32_t smooth_bins, const double* thr,
                                                double floor, uint32_t* new_sample, wbx_denoise_stats* stats) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "denoise_sample: new_sample is NULL");
  SamplePin p(e);
  const DenCall k{first_frame, n_frames, window_frames, smooth_hops, smooth_bins, thr, floor};
  const wbx_status st = p.begin(sample, "denoise_sample: unknown sample", "denoise_sample: the pool's sample ids (2^24) would run out",
                                nullptr, [&](const char** msg) { return denoise_check(&p.src, false, k, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return denoise_run(e->ctx, p.src, p.rate, k, slot, stats, why);
  });
}

// a measurement: the sample pinned, no sample made
extern "C" wbx_status wbx_engine_denoise_profile_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                        uint32_t window_frames, double* sums_out, uint64_t* hops_out) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const wbx_status st = p.begin(sample, "denoise_profile_sample: unknown sample", nullptr, nullptr, [&](const char** msg) {
    return denoise_profile_check(&p.src, first_frame, n_frames, window_frames, sums_out != nullptr, hops_out != nullptr, msg);
  });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return denoise_profile_run(e->ctx, p.src, first_frame, n_frames, window_frames, sums_out, hops_out, why); });
}

// pins the source and the key (no key with WBX_DYN_NO_KEY: the source alone); registered at the source's rate, with the
// range's frames
extern "C" wbx_status wbx_engine_dynamics_sample(wbx_engine* e, uint32_t sample, uint32_t key_sample, uint64_t first_frame,
                                                 uint64_t n_frames, uint64_t key_first, int sense, const double* table, double drive,
                                                 double key_gain, double makeup, uint32_t lookahead_frames, uint32_t hold_frames,
                                                 uint32_t release_frames, uint32_t* new_sample, wbx_dynamics_stats* dynamics_stats,
                                                 wbx_clip_stats* stats_of_result) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "dynamics_sample: new_sample is NULL");
  SamplePin p(e);
  const bool keyed = key_sample != WBX_DYN_NO_KEY;
  const DynCall k{first_frame, n_frames, key_first, keyed, sense, table, drive, key_gain, makeup, lookahead_frames, hold_frames, release_frames};
  std::vector<uint32_t> distinct = distinct_pair(sample, keyed ? key_sample : sample);
  ClipSrc key{};
  double lo = 1.0;
  const wbx_status st = p.begin(sample, "dynamics_sample: unknown sample", "dynamics_sample: the pool's sample ids (2^24) would run out",
                                &distinct, [&](const char** msg) -> wbx_status {
    uint32_t key_rate = p.rate;
    if (keyed) {
      const ClipSlot* r = p.slot_locked(key_sample);
      if (!r) return *msg = "dynamics_sample: unknown key sample", WBX_ERR_INVALID;
      key = clip_src(*r);
      key_rate = r->d.sample_rate;
    }
    return dynamics_check(p.src, p.rate, keyed ? &key : nullptr, key_rate, k, &lo, msg);
  });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return dynamics_run(e->ctx, p.src, keyed ? &key : nullptr, p.rate, k, lo, slot, dynamics_stats, stats_of_result, why);
  });
}

// registered at the source's rate, with out_frames frames
extern "C" wbx_status wbx_engine_stretch_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                uint64_t out_frames, uint32_t window_frames, uint32_t tolerance_frames,
                                                wbx_stretch_info* info, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "stretch_sample: new_sample is NULL");
  SamplePin p(e);
  const StretchCall k{first_frame, n_frames, out_frames, window_frames, tolerance_frames, false, 0};
  const wbx_status st = p.begin(sample, "stretch_sample: unknown sample", "stretch_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) { return stretch_check(p.src, k, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, out_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return stretch_run(e->ctx, p.src, p.rate, k, slot, nullptr, info, nullptr, why);
  });
}

// registered at the source's rate, with out_frames frames
extern "C" wbx_status wbx_engine_warp_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                             uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                                             uint32_t window_frames, uint32_t tolerance_frames, wbx_warp_info* info,
                                             uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "warp_sample: new_sample is NULL");
  SamplePin p(e);
  const WarpCall k{first_frame, n_frames, out_frames, markers, n_markers, window_frames, tolerance_frames, false, 0};
  const wbx_status st = p.begin(sample, "warp_sample: unknown sample", "warp_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) { return warp_check(p.src, k, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, out_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return warp_run(e->ctx, p.src, p.rate, k, slot, nullptr, info, nullptr, why);
  });
}

// registered at the source's rate, with out_frames frames
extern "C" wbx_status wbx_engine_pitch_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                              uint64_t out_frames, uint32_t num, uint32_t den, int quality, uint32_t window_frames,
                                              uint32_t tolerance_frames, wbx_pitch_info* info, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "pitch_sample: new_sample is NULL");
  SamplePin p(e);
  const PitchCall k{first_frame, n_frames, out_frames, num, den, quality, window_frames, tolerance_frames, false, 0};
  ResamplePlan plan;
  StretchCall sk{};
  const wbx_status st = p.begin(sample, "pitch_sample: unknown sample", "pitch_sample: the pool's sample ids (2^24) would run out", nullptr,
                                [&](const char** msg) { return pitch_check(p.src, k, &plan, &sk, msg); });
  if (st != WBX_OK) return st;
  return p.make(p.src.channels, p.rate, out_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return pitch_run(e->ctx, p.src, p.rate, k, plan, sk, slot, nullptr, info, nullptr, why);
  });
}

extern "C" wbx_status wbx_engine_loudness_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                 uint32_t flags, wbx_loudness* out, double* hop_energy, size_t cap_doubles) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  LoudnessPlan plan;
  const wbx_status st = p.begin(sample, "loudness_sample: unknown sample", nullptr, nullptr, [&](const char** msg) {
    return loudness_check(p.src, p.rate, first_frame, n_frames, flags, out, hop_energy, cap_doubles, &plan, msg);
  });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return loudness_run(e->ctx, p.src, plan, first_frame, n_frames, out, hop_energy, why); });
}

extern "C" wbx_status wbx_engine_f0_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                           uint32_t window_frames, uint32_t hop_frames, uint32_t tau_min, uint32_t tau_max,
                                           double threshold, wbx_f0_frame* frames_out, size_t frames_cap, wbx_f0_info* info) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const F0Call k{first_frame, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold, frames_out != nullptr, frames_cap};
  const wbx_status st = p.begin(sample, "f0_sample: unknown sample", nullptr, nullptr,
                                [&](const char** msg) { return f0_check_call(p.src, k, msg); });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return f0_run(e->ctx, p.src, k, frames_out, info, why); });
}

// pins the source and the basis; an unknown basis is the check's to refuse
extern "C" wbx_status wbx_engine_spectrum_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                 uint32_t channel, uint32_t basis_sample, uint32_t window_frames, uint32_t n_bins,
                                                 uint32_t hop_frames, float* power_out, size_t cells_cap, wbx_spectrum_info* info) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const SpecCall k{first_frame, n_frames, channel, window_frames, n_bins, hop_frames, power_out != nullptr, cells_cap};
  std::vector<uint32_t> distinct = distinct_pair(sample, basis_sample);
  ClipSrc basis{};
  const wbx_status st = p.begin(sample, "spectrum_sample: unknown sample", nullptr, &distinct, [&](const char** msg) {
    const ClipSlot* b = p.slot_locked(basis_sample);
    if (b) basis = clip_src(*b);
    return spectrum_check_call(p.src, b ? &basis : nullptr, k, msg);
  });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return spectrum_run(e->ctx, p.src, basis, k, power_out, info, why); });
}

// pins the reference and the sample; an unknown sample is the check's to refuse
extern "C" wbx_status wbx_engine_align_samples(wbx_engine* e, uint32_t ref_sample, uint64_t a_first, uint64_t n_frames, uint32_t sample,
                                               uint64_t b_first, uint64_t m_frames, int64_t lag_min, int64_t lag_max, uint32_t flags,
                                               wbx_align_info* info, wbx_align_point* curve_out, size_t curve_cap) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const AlignCall k{a_first, n_frames, b_first, m_frames, lag_min, lag_max, flags, info != nullptr, curve_out != nullptr, curve_cap};
  std::vector<uint32_t> distinct = distinct_pair(ref_sample, sample);
  ClipSrc other{};
  const wbx_status st = p.begin(ref_sample, "align_samples: unknown reference sample", nullptr, &distinct, [&](const char** msg) {
    const ClipSlot* b = p.slot_locked(sample);
    if (b) other = clip_src(*b);
    return align_check_call(&p.src, p.rate, b ? &other : nullptr, b ? b->d.sample_rate : 0u, k, msg);
  });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return align_run(e->ctx, p.src, other, k, info, curve_out, why); });
}

extern "C" wbx_status wbx_engine_onsets_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                               uint32_t hop_frames, double floor_power, double threshold, double delta, uint32_t w,
                                               uint32_t a, wbx_onset_frame* frames_out, size_t frames_cap, wbx_onset_info* info) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const OnsetCall k{first_frame, n_frames, hop_frames, floor_power, threshold, delta, w, a, frames_out != nullptr, frames_cap};
  const wbx_status st = p.begin(sample, "onsets_sample: unknown sample", nullptr, nullptr,
                                [&](const char** msg) { return onset_check_call(p.src, k, msg); });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return onset_run(e->ctx, p.src, k, frames_out, info, why); });
}

extern "C" wbx_status wbx_engine_tempo_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                              uint32_t hop_frames, double floor_power, uint32_t window_hops, uint32_t step_hops,
                                              uint32_t lag_min, uint32_t lag_max, double threshold, wbx_f0_frame* frames_out,
                                              size_t frames_cap, wbx_f0_info* info) {
  if (!e) return WBX_ERR_INVALID;
  SamplePin p(e);
  const OnsetCall k{first_frame, n_frames, hop_frames, floor_power, 0.0, 0.0, 0u, 0u, false, 0};
  F0Call track{0, 0, window_hops, step_hops, lag_min, lag_max, threshold, frames_out != nullptr, frames_cap};
  const wbx_status st = p.begin(sample, "tempo_sample: unknown sample", nullptr, nullptr,
                                [&](const char** msg) { return tempo_check_call(p.src, k, &track, msg); });
  if (st != WBX_OK) return st;
  return p.read([&](std::string* why) { return tempo_run(e->ctx, p.src, k, track, frames_out, info, why); });
}

// two runs under one pin: the range's loudness (and true peak under a ceiling), then the range derived at the gain that
// brings its integrated loudness to target_lufs
extern "C" wbx_status wbx_engine_normalize_loudness_sample(wbx_engine* e, uint32_t sample, uint64_t first_frame, uint64_t n_frames,
                                                           double target_lufs, float true_peak_ceiling, uint32_t* new_sample,
                                                           float* gain_used) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "normalize_loudness_sample: new_sample is NULL");
  if (!(true_peak_ceiling >= 0.0f)) return efail(e, WBX_ERR_INVALID, "normalize_loudness_sample: a negative ceiling, or a NaN");
  SamplePin p(e);
  wbx_clip_edit_desc d{};
  d.first_frame = first_frame;
  d.n_frames = n_frames;
  d.channel_mode = WBX_CH_KEEP;
  uint32_t out_channels = 0;
  LoudnessPlan plan;
  wbx_loudness m{};
  wbx_status st = p.begin(sample, "normalize_loudness_sample: unknown sample",
                          "normalize_loudness_sample: the pool's sample ids (2^24) would run out", nullptr, [&](const char** msg) {
    const wbx_status ok = loudness_check(p.src, p.rate, first_frame, n_frames, true_peak_ceiling > 0.0f ? (uint32_t)WBX_LOUD_TRUE_PEAK : 0u,
                                         &m, nullptr, 0, &plan, msg);
    return ok == WBX_OK ? clipfx_check_derive(p.src, &d, &out_channels, msg) : ok;
  });
  if (st != WBX_OK) return st;
  st = p.read([&](std::string* why) { return loudness_run(e->ctx, p.src, plan, first_frame, n_frames, &m, nullptr, why); });
  if (st != WBX_OK) return st;
  if (!std::isfinite(m.integrated)) return efail(e, WBX_ERR_INVALID, "normalize_loudness_sample: the range has no integrated loudness (silent, or shorter than 4 hops)");
  float g = (float)std::pow(10.0, (target_lufs - m.integrated) / 20.0);
  if (true_peak_ceiling > 0.0f) {
    const float peak = out_channels > 1 && m.true_peak[1] > m.true_peak[0] ? m.true_peak[1] : m.true_peak[0];
    const float top = true_peak_ceiling / peak;   // one IEEE fp32 division (no fast-math in this build)
    if (top < g) g = top;
  }
  if (!(g > 0.0f) || !std::isfinite(g)) return efail(e, WBX_ERR_INVALID, "normalize_loudness_sample: the gain is not finite and positive");
  d.gain = g;
  st = derive_pinned(p, d, out_channels, new_sample);
  if (st != WBX_OK) return st;
  if (gain_used) *gain_used = g;
  return WBX_OK;
}

// pins every distinct source the parts name (its check names them: no sample of its own); the tile table is built between
// the locked half and the run, without the lock; registered at the sources' common rate
extern "C" wbx_status wbx_engine_splice_samples(wbx_engine* e, uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts,
                                                uint32_t n_parts, uint32_t* new_sample) {
  if (!e) return WBX_ERR_INVALID;
  if (!new_sample) return efail(e, WBX_ERR_INVALID, "splice_samples: new_sample is NULL");
  SamplePin p(e);
  SplicePlan plan;
  // made before the lock: the distinct source ids (of a list not yet checked: nothing is pinned where the check refuses
  // it) and room for the storage descriptions
  std::vector<uint32_t> distinct;
  std::vector<ClipSrc> srcs;
  if (parts && n_parts && n_parts <= kSpliceMaxParts) {
    distinct.reserve(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) distinct.push_back(parts[i].src_clip);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    srcs.resize(n_parts);
  }
  wbx_status st = p.begin(0, nullptr, "splice_samples: the pool's sample ids (2^24) would run out", &distinct, [&](const char** msg) {
    wbx_splice_source tmp{};
    const auto source_of = [&](uint32_t id) -> const wbx_splice_source* {
      const ClipSlot* s = p.slot_locked(id);
      if (!s) return nullptr;
      tmp = wbx_splice_source{s->d.channels, s->d.sample_rate, s->d.count, (int32_t)s->d.format, 0u};
      return &tmp;
    };
    const wbx_status ok = splice_check(channels, n_frames, parts, n_parts, source_of, &plan.rate, msg);
    if (ok == WBX_OK)
      for (uint32_t i = 0; i < n_parts; i++) srcs[i] = clip_src(e->ctx->clips[parts[i].src_clip]);
    return ok;
  });
  if (st != WBX_OK) return st;
  const char* msg = "";
  st = splice_plan_table(n_frames, parts, n_parts, &plan, &msg);
  if (st != WBX_OK) return efail(e, st, msg);
  return p.make(channels, plan.rate, n_frames, new_sample, [&](ClipSlot& slot, std::string* why) {
    return splice_run(e->ctx, srcs.data(), parts, n_parts, plan, channels, n_frames, slot, nullptr, why);
  });
}

// Engine::add_audio_clip -> add_to_cliplist, engine.cpp:293-309, :409-461
extern "C" wbx_status wbx_engine_add_audio_clip(wbx_engine* e, uint32_t track, double min_time, double max_time,
                                                double start_offset, uint32_t sample, double speed, float gain) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  if (!e->hs.valid_sample(sample) && sample < e->ctx->clips.size() && e->ctx->clips[sample].used) {
    // a clip the host put into the engine's pool through layer 1 (wbx_clip_upload on wbx_engine_ctx): adopt it
    const DSample& d = e->ctx->clips[sample].d;
    if (e->hs.samples.size() <= sample) e->hs.samples.resize(sample + 1);
    e->hs.samples[sample] = SampleMeta{d.format, d.channels, d.sample_rate, d.count, true};
  }
  if (!e->hs.valid_sample(sample)) return efail(e, WBX_ERR_INVALID, "unknown sample");
  if (!(min_time <= max_time)) return efail(e, WBX_ERR_INVALID, "min_time > max_time");
  e->hs.add_audio_clip_locked(track, min_time, max_time, start_offset, sample, speed, gain);
  return WBX_OK;
}

// Engine::move_clip, engine.cpp:346-363
extern "C" wbx_status wbx_engine_move_clip(wbx_engine* e, uint32_t track, uint32_t clip, double relative_pos) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track) || clip >= e->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  e->hs.move_clip_locked(track, clip, relative_pos);
  return WBX_OK;
}

// Engine::resize_clip, engine.cpp:365-398
extern "C" wbx_status wbx_engine_resize_clip(wbx_engine* e, uint32_t track, uint32_t clip, double relative_pos,
                                             double resize_limit, double min_length, int left_side, int shift,
                                             int stretch) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track) || clip >= e->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  e->hs.resize_clip_locked(track, clip, relative_pos, resize_limit, min_length, left_side != 0, shift != 0, stretch != 0);
  return WBX_OK;
}

// Engine::delete_clip, engine.cpp:400-407
extern "C" wbx_status wbx_engine_delete_clip(wbx_engine* e, uint32_t track, uint32_t clip) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track) || clip >= e->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  e->hs.delete_clip_locked(track, clip);
  return WBX_OK;
}

// Engine::delete_region, engine.cpp:463-475
extern "C" wbx_status wbx_engine_delete_region(wbx_engine* e, uint32_t track, double min, double max) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track) || !(min <= max)) return WBX_ERR_INVALID;
  e->hs.delete_region_locked(track, min, max);
  return WBX_OK;
}

// Engine::set_clip_gain, engine.cpp:1460-1464
extern "C" wbx_status wbx_engine_set_clip_gain(wbx_engine* e, uint32_t track, uint32_t clip, float gain) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  if (!e->hs.valid_track(track) || clip >= e->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  e->hs.set_clip_gain_locked(track, clip, gain);
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_clip_count(wbx_engine* e, uint32_t track, uint32_t* count) {
  if (!e || !count) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  *count = (uint32_t)e->hs.tracks[track]->clips.size();
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_get_clip(wbx_engine* e, uint32_t track, uint32_t clip, wbx_clip_info* out) {
  if (!e || !out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track) || clip >= e->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  const DClip& d = e->hs.tracks[track]->clips[clip].d;
  out->min_time = d.min_time;
  out->max_time = d.max_time;
  out->start_offset = d.start_offset;
  out->speed = d.speed;
  out->gain = d.gain;
  out->sample = d.sample;
  return WBX_OK;
}

// the clip placement arithmetic on its own (engine/clip_edit.h:10-150), for hosts that preview an edit
extern "C" void wbx_calc_move_clip(double clip_min, double clip_max, double relative_pos, double min_move, double* new_min,
                                   double* new_max) {
  edit::calc_move_clip(clip_min, clip_max, relative_pos, min_move, new_min, new_max);
}

extern "C" void wbx_calc_resize_clip(double clip_min, double clip_max, double clip_start_offset, double clip_speed,
                                     double sample_rate, double sample_count, double relative_pos, double resize_limit,
                                     double min_length, double min_resize_pos, double beat_duration, int is_min, int shift,
                                     int stretch, int clamp_at_resize_pos, double* out_min, double* out_max,
                                     double* out_start_offset, double* out_speed) {
  const edit::ResizeResult r = edit::calc_resize_clip(clip_min, clip_max, clip_start_offset, clip_speed, sample_rate,
                                                      sample_count, relative_pos, resize_limit, min_length, min_resize_pos,
                                                      beat_duration, is_min != 0, shift != 0, stretch != 0,
                                                      clamp_at_resize_pos != 0);
  *out_min = r.min;
  *out_max = r.max;
  *out_start_offset = r.start_offset;
  *out_speed = r.speed;
}

extern "C" double wbx_calc_clip_shift(double start_offset, double relative_pos, double beat_duration, double sample_rate) {
  return edit::calc_clip_shift(start_offset, relative_pos, beat_duration, sample_rate);
}

extern "C" double wbx_shift_clip_content(double start_offset, double speed, double sample_rate, double relative_pos,
                                         double beat_duration) {
  return edit::shift_clip_content(start_offset, speed, sample_rate, relative_pos, beat_duration);
}

extern "C" wbx_status wbx_engine_play(wbx_engine* e) {   // engine.cpp:68-80
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  e->hs.play_locked();
  e->hs.note_edit_locked();
  return WBX_OK;
}

namespace {
wbx_status stop_record_impl(wbx_engine* e);
}

extern "C" wbx_status wbx_engine_stop(wbx_engine* e) {   // engine.cpp:82-93, Track::stop track.cpp:249-256
  if (!e) return WBX_ERR_INVALID;
  const wbx_status rs = stop_record_impl(e);   // engine.cpp:83-84 (an overflow is the take's status, not the stop's)
  LockGuard g(e->hs.editor_lock);
  e->hs.stop_locked();
  e->hs.note_edit_locked();
  return rs == WBX_ERR_OVERFLOW ? WBX_OK : rs;
}

namespace {

// the host waits for both streams a render uses: what a step does before it replaces a buffer that work in flight may read
hipError_t sync_plan_and_main(wbx_ctx* c) {
  const hipError_t he = hipStreamSynchronize(c->plan_stream);
  return he != hipSuccess ? he : sync_main(c);
}

// (re)allocate the three pinned patch and gain buffers at once — pinning memory synchronises the device, so it must
// not happen in mid-run
wbx_status ensure_pinned_tables(wbx_engine* e, uint32_t N) {
  wbx_ctx* c = e->ctx;
  if (e->tables_cap >= N) return WBX_OK;
  WBX_EHIP(e, sync_plan_and_main(c));
  const uint32_t cap = std::max<uint32_t>(N, c->cfg.max_tracks);
  for (int i = 0; i < kRing; i++) {
    WBX_EHIP(e, e->patch[i].buf.ensure(cap));
    WBX_EHIP(e, e->gains[i].buf.ensure((size_t)cap * 2));
    e->patch[i].forget();
    e->gains[i].forget();
    WBX_EHIP(e, e->patch[i].done.ensure(kDevEventFlags));
    WBX_EHIP(e, e->gains[i].done.ensure(kDevEventFlags));
  }
  e->tables_cap = cap;
  e->gains_slot = -1;
  e->hs.gains_dirty = true;   // the buffers are new: fill one
  return WBX_OK;
}

// ---- the steps of render_locked (below), in the order it takes them --------------------------------------------------

// Engine::process with an empty track list: output_buffer.clear() and the transport advance (engine.cpp:1598, :1619-1623) —
// silence — or, with a running master to continue (wbx_set_master_init; WBX_DIST_CHAIN on a rank whose shard is empty: more
// ranks than tracks, or all of its tracks deleted), that sum handed on unchanged: the receive must be posted like any other
// render's, or the previous rank's send is never matched and the sum of all earlier ranks is lost
wbx_status render_empty_session(wbx_engine* e, uint32_t K, float* master_target, int master_format, double beat_duration) {
  wbx_ctx* c = e->ctx;
  const uint32_t C = c->cfg.channels, F = c->cfg.block_frames;
  hipStream_t s = c->stream;
  WBX_EHIP(e, join_sum(c));
  WBX_EHIP(e, c->d_master.ensure((size_t)K * C * F));
  const bool continues = c->master_init || dist_receives_running_sum(c);
  if (master_format && (c->dist || continues))
    return efail(e, WBX_ERR_UNSUPPORTED, "an empty session continues a running master / feeds a multi-GPU exchange in planar fp32 only");
  hipError_t me = hipSuccess;
  float* master = begin_master(c, master_target, s, &me);
  WBX_EHIP(e, me);
  if (continues) {
    wbx_status ist = WBX_OK;
    const float* init = c->dist ? dist_mix_init(c, K, s, &ist) : c->master_init;
    if (ist != WBX_OK) return cfail(e, ist);
    launch_clamp_into(init, master, (size_t)K * C * F, c->clamp ? 1 : 0, s);   // (the clamp follows the last addition: none here)
    if (c->dist) WBX_EHIP(e, dist_mix_issued(c, s));
    WBX_EHIP(e, hipGetLastError());
  } else {   // (all-zero bytes are silence in every output format; packed 24-bit counts its 3 bytes per sample)
    const size_t eb = master_format ? out_format_bytes(master_format) : sizeof(float);
    WBX_EHIP(e, hipMemsetAsync(master, 0, (size_t)K * C * F * eb, s));
  }
  c->last_master = master;
  c->last_master_format = master_format;
  c->last_master_on_host = false;
  c->last_K = K;
  c->last_N = 0;
  e->hs.advance_transport_locked(K, F, beat_duration);
  return WBX_OK;
}

// parameters: drain the message rings (process_track_messages track.cpp:773-779) and apply them (track.cpp:618-643); the
// factor used per sample is fl(volume * pan_coeffs[c]) (track.cpp:728-731)
wbx_status refresh_gains(wbx_engine* e) {
  if (!e->hs.drain_params_locked()) return WBX_OK;
  const int slot = (e->gains_slot + 1) % kRing;
  WBX_EHIP(e, e->gains[slot].wait());   // its last reader, >= 2 changes ago
  e->hs.build_gains_locked(e->gains_tmp);
  std::memcpy(e->gains[slot].buf.p, e->gains_tmp.data(), e->gains_tmp.size() * sizeof(float));
  e->gains_slot = slot;
  e->gains_gen++;
  return WBX_OK;
}

// clip lists: the table is replaced whole when an edit touched it
wbx_status upload_clip_table(wbx_engine* e, uint32_t N) {
  HostSession& hs = e->hs;
  if (!hs.clips_dirty) return WBX_OK;
  WBX_EHIP(e, sync_plan_and_main(e->ctx));
  // Clip::internal_state_changed is cleared by the sequencer on the device (track.cpp:373,392,418): before
  // the table is replaced, take the live flags back for every clip no edit has touched since the last upload
  if (e->clips_uploaded && e->d_clips_count) {
    std::vector<DClip> live(e->d_clips_count);
    WBX_EHIP(e, hipMemcpy(live.data(), e->d_clips.p, live.size() * sizeof(DClip), hipMemcpyDeviceToHost));
    hs.merge_live_flags_locked(live.data(), live.size());
  }
  hs.flatten_clips_locked(e->flat, e->first);
  WBX_EHIP(e, e->d_clips.ensure(std::max<size_t>(1, e->flat.size())));
  WBX_EHIP(e, e->d_clip_first.ensure(N + 1));
  e->d_clips_count = e->flat.size();
  e->clips_uploaded = true;
  WBX_EHIP(e, e->h_flags_left.ensure(16));
  uint32_t set_flags = 0;   // (both streams were drained above: nothing counts down right now)
  for (const DClip& dc : e->flat) set_flags += dc.internal_state_changed != 0 ? 1u : 0u;
  *e->h_flags_left.p = set_flags;
  e->table_flags = set_flags != 0u;
  if (!e->flat.empty()) WBX_EHIP(e, hipMemcpy(e->d_clips.p, e->flat.data(), e->flat.size() * sizeof(DClip), hipMemcpyHostToDevice));
  WBX_EHIP(e, hipMemcpy(e->d_clip_first.p, e->first.data(), e->first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return WBX_OK;
}

// per-track device state: allocated once at max_tracks capacity; tracks added since the last render find their slots cleared
// already (wbx_engine::d_state)
wbx_status ensure_track_state(wbx_engine* e, uint32_t N) {
  wbx_ctx* c = e->ctx;
  if (e->state_tracks >= N) return WBX_OK;
  if (e->d_state.cap < N) {
    WBX_EHIP(e, sync_plan_and_main(c));
    WBX_EHIP(e, e->d_state.ensure(std::max<size_t>(N, c->cfg.max_tracks)));
    WBX_EHIP(e, e->d_levels.ensure((size_t)c->cfg.max_tracks * 2));
    WBX_EHIP(e, hipMemset(e->d_state.p, 0, e->d_state.cap * sizeof(DTrackState)));
    WBX_EHIP(e, hipMemset(e->d_levels.p, 0, e->d_levels.cap * sizeof(float)));
  }
  e->state_tracks = N;
  return WBX_OK;
}

// pending state edits (play / stop / clip-list changes) into the next pinned patch buffer; *slot: which, -1 = none pending
wbx_status take_patches(wbx_engine* e, int* slot) {
  *slot = -1;
  if (!e->hs.patches_pending) return WBX_OK;
  *slot = (int)(e->patch_seq++ % kRing);
  WBX_EHIP(e, e->patch[*slot].wait());
  e->hs.take_patches_locked(e->patch[*slot].buf.p);
  return WBX_OK;
}

// routing, layer 1's tables and its result buffers
wbx_status upload_routing_and_tables(wbx_engine* e, uint32_t K, uint32_t N) {
  wbx_ctx* c = e->ctx;
  HostSession& hs = e->hs;
  if (hs.routing_dirty || c->routing_tracks != N) {
    std::vector<int32_t> tb(N);
    for (uint32_t t = 0; t < N; t++) tb[t] = hs.tracks[t]->bus;
    WBX_STEP(cfail(e, wbx_set_routing(c, N, hs.n_buses ? tb.data() : nullptr, hs.n_buses)));
    hs.routing_dirty = false;
  }
  WBX_STEP(cfail(e, upload_tables(c, N)));
  return cfail(e, ensure_result_buffers(c, K, N));
}

// A device observation, not a decision: the sequencer counts h_flags_left down as it clears the table's flags
void refresh_table_flags(wbx_engine* e) {
  if (e->table_flags && e->h_flags_left.p && *reinterpret_cast<volatile uint32_t*>(e->h_flags_left.p) == 0u)
    e->table_flags = false;   // every flag of the table has been cleared by a plan that is over
}

// rows for the track-blocks the hot loop cannot stream directly, pool chunks, and the plan's templates
wbx_status ensure_plan_capacity(wbx_engine* e, uint32_t K, uint32_t N, const RenderPlan& plan, double beat_duration) {
  wbx_ctx* c = e->ctx;
  HostSession& hs = e->hs;
  const double block_beats = ((double)c->cfg.block_frames / (double)c->cfg.sample_rate) / beat_duration;
  WBX_STEP(cfail(e, ensure_gen_capacity(c, hs.gen_rows_hint(K, c->shape.masked_rows, block_beats) * (plan.double_rows ? 2u : 1u))));
  if (plan.pool_slack) WBX_STEP(cfail(e, ensure_pool_slack(c)));
  return cfail(e, ensure_template_capacity(c, std::max(hs.template_hint(K, plan.n_segs), (size_t)2 * N)));   // (2 N: the one-launch callback's static pairs)
}

// the plan stream `ps` behind the last readers of what this render's plan and mix will write
wbx_status order_plan_stream(wbx_engine* e, const RenderPlan& plan, hipStream_t ps, RenderCall* call) {
  wbx_ctx* c = e->ctx;
  wbx_ctx::PlanBuf& B = PB(c);
  if (B.consumed_valid) WBX_EHIP(e, hipStreamWaitEvent(ps, B.consumed, 0));   // the mix that read this buffer two renders ago
  const int pp = (int)(c->render_seq % kRing);
  if (plan.beside && c->sum_valid[pp]) {   // ... and the sum that read the partial buffer this render's mix will write
    WBX_EHIP(e, hipStreamWaitEvent(ps, c->partial_free[pp], 0));   // (the sum KERNEL: not the copy-out of its master behind it)
    call->plan_waits_partial = true;
  }
  return WBX_OK;
}

// the sequencer's arguments over the current plan buffer (times: set by stage_transport_table; reads only)
PlanArgs plan_args(const wbx_engine* e, uint32_t K, uint32_t N, const RenderPlan& plan, int patch_slot, bool playing, double beat_duration) {
  wbx_ctx* c = e->ctx;
  const HostSession& hs = e->hs;
  const wbx_ctx::PlanBuf& B = PB(c);
  PlanArgs a{};
  a.clips = e->d_clips.p;
  a.clip_first = e->d_clip_first.p;
  a.samples = c->d_samples.p;
  a.state = e->d_state.p;
  a.patch = patch_slot >= 0 ? e->patch[patch_slot].buf.p : nullptr;
  a.gains = e->gains[e->gains_slot].buf.p;
  a.rows = B.prows.p;
  a.tmpl = B.tmpl.p;
  a.tmpl_count = B.counters.p + 3;
  a.tmpl_cap = B.tmpl_cap;
  a.pool = B.pool.p;
  a.pool_count = B.counters.p;
  a.status = B.counters.p + 1;
  a.gen_list = B.gen_list.p;
  a.gen_count = B.counters.p + 2;
  a.gen_cap = B.gen_cap;
  a.pool_chunks = B.pool_chunks;
  a.n_tracks = N;
  a.n_blocks = K;
  a.block_frames = c->cfg.block_frames;
  a.channels = c->cfg.channels;
  a.sample_rate = (double)c->cfg.sample_rate;
  a.playing = playing ? 1u : 0u;
  a.clips_changed = hs.clips_edited ? 1u : 0u;
  a.flags_left = e->h_flags_left.p;
  // clip boundaries inside a block stay in the hot loop when the mix instance of this render can take them
  a.masked_rows = c->shape.masked_rows;
  a.tmpl_reserve = plan.tmpl_reserve;
  a.lanes = hs.plan_lanes(K);
  a.playhead = hs.playhead;
  a.sample_position = hs.sample_position;
  a.beat_duration = beat_duration;
  a.times = nullptr;
  return a;
}

// the plan's four counters to zero, and — where the plan reads it from device memory — the transport table in front of it
wbx_status stage_transport_table(wbx_engine* e, uint32_t K, const RenderPlan& plan, PlanArgs* a, hipStream_t ps) {
  wbx_ctx::PlanBuf& B = PB(e->ctx);
  B.counters_zero = false;
  e->plan_status_on_host = false;
  if (plan.device_times) {
    WBX_EHIP(e, B.times.ensure(K));
    a->times = B.times.p;
    auto& T = e->times[e->times_seq++ % wbx_engine::kTimesRing];
    WBX_EHIP(e, T.wait());   // its copy of 8 renders ago (long over)
    WBX_EHIP(e, T.buf.ensure(K));
    WBX_EHIP(e, T.done.ensure(kDevEventFlags));
    block_times(*a, T.buf.p);   // wbx_seq.h: the source the device compiles
    launch_times_copy(T.buf.p, B.times.p, K, plan.zeroing == RenderPlan::TIMES_COPY ? B.counters.p : nullptr, ps);
    WBX_EHIP(e, T.mark(ps));
  }
  if (plan.zeroing == RenderPlan::MEMSET) WBX_EHIP(e, hipMemsetAsync(B.counters.p, 0, 4 * sizeof(uint32_t), ps));
  return WBX_OK;
}

// the sequencer of render n+1 continues from the per-track state render n's left: `ps` behind the stream that planned last
// (found by the random-pieces test once it left renders unfetched: a batch render's plan, on the idle plan stream, overtook
//  the plan of a short render still queued on the main stream behind earlier mixes and read the state before that one had
//  written it)
wbx_status hand_plan_stream_over(wbx_engine* e, hipStream_t ps) {
  if (e->last_plan_stream && e->last_plan_stream != ps) {
    WBX_EHIP(e, e->plan_handover.ensure(kDevEventFlags));
    WBX_EHIP(e, hipEventRecord(e->plan_handover, e->last_plan_stream));
    WBX_EHIP(e, hipStreamWaitEvent(ps, e->plan_handover, 0));
  }
  e->last_plan_stream = ps;
  return WBX_OK;
}

// the seam states of a plan by segments: one buffer, behind its last user
wbx_status ensure_seam_buffers(wbx_engine* e, uint32_t N, size_t per, hipStream_t ps) {
  wbx_ctx* c = e->ctx;
  if (e->seam_stream && e->seam_stream != ps) {   // (its last user ran on the other stream)
    WBX_EHIP(e, e->seam_done.ensure(kDevEventFlags));
    WBX_EHIP(e, hipEventRecord(e->seam_done, e->seam_stream));
    WBX_EHIP(e, hipStreamWaitEvent(ps, e->seam_done, 0));
  }
  if (e->d_seam.cap < 2 * per) {
    if (e->seam_stream) WBX_EHIP(e, hipStreamSynchronize(e->seam_stream));
    WBX_EHIP(e, e->d_seam.ensure(2 * per));
  }
  if (!e->d_seg_stats.p) {
    WBX_EHIP(e, e->d_seg_stats.ensure(2));
    WBX_EHIP(e, hipMemsetAsync(e->d_seg_stats.p, 0, 2 * sizeof(uint32_t), ps));
  }
  if (e->d_seg_ticket.cap < N) {
    if (e->seam_stream) WBX_EHIP(e, hipStreamSynchronize(e->seam_stream));
    const size_t cap = std::max<size_t>(N, c->cfg.max_tracks);
    WBX_EHIP(e, e->d_seg_ticket.ensure(cap));
    WBX_EHIP(e, hipMemsetAsync(e->d_seg_ticket.p, 0, e->d_seg_ticket.cap * sizeof(uint32_t), ps));
  }
  e->seam_stream = ps;
  return WBX_OK;
}

// the sequencer of this render: one lane per track, or — long renders of sessions cut into clips — per (track, segment); the
// one-launch callback has none (its mix launch plans for itself) and reads the gains from the device copy
wbx_status launch_sequencer(wbx_engine* e, uint32_t N, const RenderPlan& plan, PlanArgs* a, hipStream_t ps) {
  wbx_ctx* c = e->ctx;
  PB(c).static_tmpl = plan.static_tmpl;
  if (plan.static_tmpl) {
    if (e->d_gains_cb_gen != e->gains_gen || e->d_gains_cb.cap < (size_t)N * 2) {
      WBX_EHIP(e, e->d_gains_cb.ensure(std::max<size_t>((size_t)c->cfg.max_tracks, N) * 2));
      WBX_EHIP(e, hipMemcpyAsync(e->d_gains_cb.p, e->gains[e->gains_slot].buf.p, (size_t)N * 2 * sizeof(float), hipMemcpyHostToDevice, ps));
      e->d_gains_cb_gen = e->gains_gen;
    }
    a->gains = e->d_gains_cb.p;
  }
  if (plan.sequencer == RenderPlan::SEGMENTS) {
    // one lane per (track, segment); the lane that completes a track checks its seams; the seam states live in one buffer
    const size_t per = (size_t)N * plan.n_segs;
    WBX_STEP(ensure_seam_buffers(e, N, per, ps));
    SegArgs g{e->d_seam.p, e->d_seam.p + per, e->d_seg_stats.p, e->d_seg_ticket.p, plan.seg_len, plan.n_segs};
    launch_plan_segments(*a, g, plan.beside, ps);
    e->seg_renders++;
    e->seg_last_segs = plan.n_segs;
  } else if (plan.sequencer == RenderPlan::PLAIN) {
    launch_plan(*a, ps);
  }
  return WBX_OK;
}

// behind the sequencer on `ps`: the marks of the pinned buffers it read (a process block waits for its render: none), the
// pre-render pass, and the event a mix on another stream waits for
wbx_status finish_plan(wbx_engine* e, const RenderPlan& plan, int patch_slot, bool callback, hipStream_t ps, bool plan_event) {
  wbx_ctx* c = e->ctx;
  if (!callback) {
    if (patch_slot >= 0) WBX_EHIP(e, e->patch[patch_slot].mark(ps));
    WBX_EHIP(e, e->gains[e->gains_slot].mark(ps));   // (re-recorded by every plan that reads the buffer)
  }
  if (!plan.skip_pre_render) WBX_STEP(cfail(e, launch_pre_render(c, ps)));
  if (plan_event) WBX_EHIP(e, hipEventRecord(PB(c).planned, ps));   // (plan and mix on one stream: the mix simply follows)
  return WBX_OK;
}

// mix (main stream, or the alternate one for every other batch render) + sum, after the plan
wbx_status launch_mix(wbx_engine* e, uint32_t K, uint32_t N, RenderCall* call, const PlanArgs& a, bool plan_event, bool* launched_as_one) {
  wbx_ctx* c = e->ctx;
  wbx_ctx::PlanBuf& B = PB(c);
  if (plan_event) WBX_EHIP(e, hipStreamWaitEvent(call->mix_stream, B.planned, 0));
  c->levels_target = reinterpret_cast<uint32_t*>(e->d_levels.p);
  const int mix_parity = (int)(c->render_seq % kRing);
  if (c->shape.cb_one_launch) {   // (only a process block's shape says so: h_status is there)
    call->plan = &a;
    call->done_word = e->h_status.p + 8;
    call->gave_up_word = e->h_status.p + 7;
    if (++e->cb_seq == 0u) ++e->cb_seq;   // (0 is what the completion and election words hold before any launch)
    call->seq = e->cb_seq;
  }
  WBX_STEP(cfail(e, launch_mix_sum(c, K, N, *call, launched_as_one)));
  B.consumed = c->mix_done[mix_parity];   // recorded right after the mix: the plan buffer is free before the sum runs
  B.consumed_valid = !*launched_as_one;   // (the one-launch callback records no event: wbx_engine_process waits for the launch itself)
  return WBX_OK;
}

// What one render_locked call reports beside its status
struct RenderResult {
  bool one_launch = false;          // the block ran as the one-launch callback
  bool pre_render_skipped = false;  // the render left the pre-render launch out (expecting an empty queue)
};

// the audio thread's render, editor lock held by the caller.  `process`: the one block of wbx_engine_process, which waits
// for it before it returns (the pinned tables need no completion events) — where its master and its plan status go; null:
// a batch render, a bounce pass.  *result (if asked for): RenderResult
wbx_status render_locked(wbx_engine* e, uint32_t K, const RenderCall* process = nullptr, RenderResult* result = nullptr) {
  wbx_ctx* c = e->ctx;
  HostSession& hs = e->hs;
  tls_err.clear();
  if (K > c->cfg.max_blocks) return efail(e, WBX_ERR_INVALID, "n_blocks above wbx_config.max_blocks");
  const uint32_t N = hs.n_tracks();
  (void)hipSetDevice(c->cfg.device);
  hs.render_edit_seq = hs.edit_seq;
  // engine.cpp:1579,1585: the tempo and the play state are read once per block
  const double beat_duration = hs.beat_duration.load(std::memory_order_relaxed);
  const bool playing = hs.playing.load(std::memory_order_relaxed);
  if (N == 0)
    return render_empty_session(e, K, process ? process->master : c->master_target, process ? process->format : c->master_format, beat_duration);

  // -- what the sequencer and the mix read: pinned tables, gains, clip lists, per-track state, patches, routing
  int patch_slot = -1;
  WBX_STEP(ensure_pinned_tables(e, N));
  WBX_STEP(refresh_gains(e));
  WBX_STEP(upload_clip_table(e, N));
  WBX_STEP(ensure_track_state(e, N));
  WBX_STEP(take_patches(e, &patch_slot));
  WBX_STEP(upload_routing_and_tables(e, K, N));

  // -- the mix instance of this render and what follows from it (wbx_shape.h): decided here, once, behind upload_tables (which
  //    reads the clip table's formats) and in front of everything that plans or launches for this render
  c->session = hs.shape_facts();
  c->shape = render_shape(c, K, N, process && !hs.any_slow_clip);

  // -- ... and how it is planned (wbx_shape.h: choose_plan), in front of everything that is sized, ordered or launched for the plan
  refresh_table_flags(e);
  PlanFacts pf;
  pf.K = K, pf.N = N;
  pf.playing = playing, pf.callback = process != nullptr, pf.any_slow_clip = hs.any_slow_clip, pf.cut = hs.cut_tracks != 0;
  pf.table_flags = e->table_flags, pf.seg_broken = c->seg_broken;
  pf.masked_rows = c->shape.masked_rows, pf.cb_one_launch = c->shape.cb_one_launch;
  pf.counters_zero = c->pb[(c->cur + 1) % kRing].counters_zero;   // (the buffer this render plans into)
  const RenderPlan plan = choose_plan(e->knobs, c->ck, c->knobs, pf);
  WBX_STEP(ensure_plan_capacity(e, K, N, plan, beat_duration));

  // -- plan (sequencer on the device) + pre-render on the plan stream, into the other plan buffer; it may run
  //    while the mix of the previous render is still busy on the main stream
  c->cur = (c->cur + 1) % kRing;
  hipStream_t ps = plan.beside ? c->plan_stream : c->stream;
  RenderCall call = process ? *process : RenderCall{};
  call.mix_stream = pick_mix_stream(c, K, true);   // main stream, or the alternate one for every other batch render
  const bool plan_event = ps != call.mix_stream;   // the mix runs on another stream than its plan
  WBX_STEP(order_plan_stream(e, plan, ps, &call));
  PlanArgs a = plan_args(e, K, N, plan, patch_slot, playing, beat_duration);
  hs.clips_edited = false;   // (PlanArgs::clips_changed has taken it)
  WBX_STEP(stage_transport_table(e, K, plan, &a, ps));
  WBX_STEP(hand_plan_stream_over(e, ps));
  WBX_STEP(launch_sequencer(e, N, plan, &a, ps));
  WBX_STEP(finish_plan(e, plan, patch_slot, process != nullptr, ps, plan_event));

  RenderResult r;
  r.pre_render_skipped = plan.skip_pre_render;
  WBX_STEP(launch_mix(e, K, N, &call, a, plan_event, &r.one_launch));
  if (result) *result = r;

  // -- transport: the host repeats the arithmetic of Engine::process (engine.cpp:1578-1585, :1619-1623) that
  //    the plan kernel performs for its K blocks, so both sides hold the same playhead / sample_position bits
  hs.advance_transport_locked(K, c->cfg.block_frames, beat_duration);
  return WBX_OK;
}

}  // namespace

extern "C" wbx_status wbx_engine_render(wbx_engine* e, uint32_t K) {
  if (!e || K == 0) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (e->hs.recording) return efail(e, WBX_ERR_UNSUPPORTED, "wbx_engine_render: not while recording (takes are captured per process call)");
  return render_locked(e, K);
}

// ---- bouncing ----------------------------------------------------------------------------------------------------------
// wbx_engine_bounce: the range is rendered by the ordinary passes (render_locked: sequencer, pre-render, mix, sum — the
// levels and every bit of state are then those of the defining sequence, HostSession::bounce_locked), and behind each pass
// stem_kernel (wbx_bounce.hip) writes the signals asked for into their destination clips from the pass's own plan and
// result buffers.  The host waits for each pass: the plan buffers, the gain row and the result buffers a stem kernel reads
// are then never handed to a later render before it is done, and the pass's plan status is looked at like wbx_fetch does.
namespace {

struct BounceDev {
  wbx_engine* e;
  const wbx_bounce_source* src;
  uint32_t n_src;
  std::vector<ClipSlot> slots;
  DevBuf<StemSrc> d_src;
  DevBuf<float> d_gains;
  uint64_t n_frames = 0;
  bool uploaded = false;

  ~BounceDev() {
    d_src.release();
    d_gains.release();
  }
  wbx_status alloc(uint32_t i, uint64_t frames) {
    wbx_ctx* c = e->ctx;
    if (slots.empty()) slots.resize(n_src);
    n_frames = frames;
    ClipFill fill{};
    fill.kind = CLIP_SRC_NONE;   // the stem kernel writes every frame; only the padding is cleared
    return cfail(e, clip_build(c, slots[i], WBX_FMT_F32, c->cfg.channels, c->cfg.sample_rate, frames, fill, c->stream));
  }
  void release(uint32_t i) {
    (void)sync_main(e->ctx);   // (nothing may still write the clip)
    clip_release(e->ctx, slots[i]);
  }
  uint32_t publish(uint32_t i) {
    uint32_t id = 0;   // (a fresh id below 2^24 — wbx_engine_bounce checked the room for all of them — cannot fail)
    (void)register_sample_locked(e, slots[i], slots[i].d.channels, e->ctx->cfg.sample_rate, n_frames, &id);
    return id;
  }
  wbx_status pass(uint32_t first_block, uint32_t k) {
    wbx_ctx* c = e->ctx;
    const uint32_t C = c->cfg.channels, F = c->cfg.block_frames;
    wbx_status st = render_locked(e, k);
    if (st != WBX_OK) return st;
    const uint32_t N = e->hs.n_tracks();
    hipStream_t s = c->stream;
    // the main stream behind this pass's sum (the event wbx_master_ready uses) and a mix on the alternate stream
    WBX_EHIP(e, join_sum(c));
    WBX_EHIP(e, join_alt(c));
    if (!uploaded) {
      std::vector<StemSrc> h(n_src);
      for (uint32_t i = 0; i < n_src; i++) {
        h[i].dst[0] = (float*)slots[i].d.ch[0];
        h[i].dst[1] = (float*)slots[i].d.ch[1];
        h[i].kind = (uint32_t)src[i].kind;
        h[i].index = src[i].index;
        h[i].tap = (uint32_t)src[i].tap;
        h[i]._pad = 0;
      }
      WBX_EHIP(e, d_src.ensure(n_src));
      WBX_EHIP(e, hipMemcpy(d_src.p, h.data(), h.size() * sizeof(StemSrc), hipMemcpyHostToDevice));
      uploaded = true;
    }
    wbx_ctx::PlanBuf& B = PB(c);
    StemArgs a{};
    a.src = d_src.p;
    a.first_frame = (uint64_t)first_block * F;
    a.n_frames = n_frames;
    a.n_src = n_src;
    a.n_blocks = k;
    a.n_tracks = N;
    a.block_frames = F;
    a.channels = C;
    if (N) {   // (an empty session has no plan: its master is silence, it has no track to name)
      WBX_EHIP(e, d_gains.ensure(std::max<size_t>((size_t)N * 2, 2)));
      WBX_EHIP(e, hipMemcpyAsync(d_gains.p, e->gains[e->gains_slot].buf.p, (size_t)N * 2 * sizeof(float), hipMemcpyHostToDevice, s));
      a.rows = B.prows.p;
      a.tmpl = B.tmpl.p;
      a.tmpl_cap = B.tmpl_cap;
      a.pool = B.pool.p;
      a.pool_chunks = B.pool_chunks;
      a.gains = d_gains.p;
      a.n_buses = c->n_buses;
      a.buses = c->n_buses ? c->last_buses : nullptr;
    }
    a.master = c->last_master;
    if ((uint64_t)n_src * k > 0x7FFFFFFFull) return efail(e, WBX_ERR_UNSUPPORTED, "bounce: more than 2^31 (source, block) pairs in one pass");
    launch_stem(a, s);
    WBX_EHIP(e, hipGetLastError());
    WBX_EHIP(e, sync_main(c));
    drain_events(c);
    if (N) {
      uint32_t pc[4] = {0, 0, 0, 0};
      WBX_EHIP(e, hipMemcpy(pc, B.counters.p, sizeof(pc), hipMemcpyDeviceToHost));
      st = plan_status_to_error(c, pc[1]);
      if (st == WBX_OK) st = render_status(c);
      if (st != WBX_OK) return cfail(e, st);
    }
    return WBX_OK;
  }
};

}  // namespace

extern "C" wbx_status wbx_engine_bounce(wbx_engine* e, double min_time, double max_time, const wbx_bounce_source* src,
                                        uint32_t n_src, uint32_t* samples_out, uint64_t* frames_out) {
  if (!e) return WBX_ERR_INVALID;
  wbx_ctx* c = e->ctx;
  LockGuard g(e->hs.editor_lock);
  tls_err.clear();
  (void)hipSetDevice(c->cfg.device);
  bool master_src = false;
  for (uint32_t i = 0; src && i < n_src; i++) master_src |= src[i].kind == WBX_BOUNCE_MASTER;
  const bool redirected = c->master_target || c->dist || c->master_init || (master_src && c->master_format);
  if ((uint64_t)c->clips.size() + n_src > (1u << 24)) return efail(e, WBX_ERR_OVERFLOW, "bounce: the pool's sample ids (2^24) would run out");
  BounceDev dev{e, src, n_src};
  const char* why = "";
  const wbx_status st = e->hs.bounce_locked(min_time, max_time, src, n_src, c->cfg.block_frames, c->cfg.max_blocks, redirected,
                                            dev, samples_out, frames_out, &why);
  if (st != WBX_OK && why[0]) return efail(e, st, why);
  return st;
}

// ---- recording ---------------------------------------------------------------------------------------------------------
// Engine::record / stop_record / arm_track_recording / set_track_input (engine.cpp:95-200) and the recorder tap of
// Engine::process (engine.cpp:1638-1649).  Who records what, record_min_time / record_max_time and the frame count are the
// host session's (wbx_host.h); the audio lives in HBM from the first frame on:
//   audio thread  copies the block's recorded input channels into a pinned staging slot (kRecSlots of them, each with the
//                 event of the capture that read it last) and launches record_capture_kernel on the upload stream — never
//                 the mix streams, and it does not wait for it;
//   recorder      the engine's own thread: keeps rec_spare chunks (clip pool extents, zeroed) ahead of every take's write
//                 position and enqueues their table entries on the same stream before it publishes them;
//   stop_record   waits for that stream, gathers each take's chunks into one F32 clip (with the 16 zero frames of padding),
//                 frees the chunks and adds the clip through the edit path (add_audio_clip, overlap trimming included).
// A block that finds a chunk missing (the recorder fell behind, or the table is full) or its staging slot still being read
// is not written: its frames stay silent (chunks start zeroed; missing chunks gather as zeros) and the take's status
// latches WBX_RECORD_OVERFLOW.  The frame count and record_max_time advance all the same.

namespace {

uint32_t rec_chunks_needed(const wbx_engine* e, uint64_t written) {   // chunks the next block touches, plus the spare ones
  const uint64_t need = (written + e->rec_F + e->rec_chunk - 1) / e->rec_chunk + e->rec_spare;
  return (uint32_t)std::min<uint64_t>(need, e->rec_table_cap);
}

// take chunks from the clip pool until every take holds what `written` asks for (the recorder thread, and record())
wbx_status rec_fill(wbx_engine* e, uint64_t written) {
  wbx_ctx* c = e->ctx;
  const uint32_t need = rec_chunks_needed(e, written);
  for (uint32_t k = 0; k < e->rec_n; k++) {
    wbx_engine::RecTake& t = e->rec_takes[k];
    while (true) {
      std::lock_guard<std::mutex> lk(e->rec_mu);   // (per chunk: rec_discard_takes_locked never waits for a whole fill)
      if (t.discarded || t.chunks.size() >= need) break;
      ClipSlot s;
      ClipFill f{};
      f.kind = CLIP_SRC_ZERO;
      const wbx_status st = clip_build(c, s, WBX_FMT_F32, t.channels, c->cfg.sample_rate, e->rec_chunk, f, c->upload_stream);
      if (st != WBX_OK) return st;
      const size_t i = (size_t)k * e->rec_table_cap + t.chunks.size();
      e->h_rec_table.p[i].ch[0] = (uint32_t*)s.d.ch[0];
      e->h_rec_table.p[i].ch[1] = (uint32_t*)s.d.ch[1];
      if (hipMemcpyAsync(e->d_rec_table.p + i, e->h_rec_table.p + i, sizeof(RecChunk), hipMemcpyHostToDevice, c->upload_stream) !=
          hipSuccess) {
        clip_release(c, s);
        return WBX_ERR_DEVICE;
      }
      t.chunks.push_back(std::move(s));
      t.ready.store((uint32_t)t.chunks.size(), std::memory_order_release);   // (the entry's copy is enqueued: captures see it)
    }
  }
  return WBX_OK;
}

void rec_thread_main(wbx_engine* e) {
  (void)hipSetDevice(e->ctx->cfg.device);
  while (e->rec_run.load(std::memory_order_acquire)) {
    const wbx_status st = rec_fill(e, e->rec_written.load(std::memory_order_acquire));
    if (st != WBX_OK) e->rec_thread_err.store(st, std::memory_order_relaxed);   // the blocks that find no room say overflow
    std::unique_lock<std::mutex> lk(e->rec_mu);
    e->rec_cv.wait_for(lk, std::chrono::milliseconds(st == WBX_OK ? 2 : 20));
  }
}

// Deleting a recording track (or clear_all) discards its take: the host session has cut the take loose from its track
// (permute_tracks_locked); here its chunks go back to the pool — once the captures in flight are through with them — and it
// gets no more (rec_fill), so wbx_clip_pool_stats shows the discard at once and rec_capture_locked finds no chunk ready to
// write the take's later blocks into.  The UI thread, editor lock held (no capture is being issued meanwhile).
void rec_discard_takes_locked(wbx_engine* e) {
  if (!e->hs.recording || !e->rec_n || e->hs.takes.size() != e->rec_n) return;
  bool waited = false;
  for (uint32_t k = 0; k < e->rec_n; k++) {
    wbx_engine::RecTake& t = e->rec_takes[k];
    if (e->hs.takes[k].track || t.discarded) continue;
    {
      std::lock_guard<std::mutex> lk(e->rec_mu);
      t.discarded = true;
      t.ready.store(0, std::memory_order_release);
    }
    if (!waited) (void)hipStreamSynchronize(e->ctx->upload_stream);   // captures and zero fills that still touch the chunks
    waited = true;
    std::lock_guard<std::mutex> lk(e->rec_mu);
    for (auto& s : t.chunks) clip_release(e->ctx, s);
    t.chunks.clear();
  }
}

// stop the recorder thread, wait for every capture, free what the takes hold (the UI thread; no take running)
void rec_release(wbx_engine* e) {
  if (e->rec_thread.joinable()) {
    e->rec_run.store(false, std::memory_order_release);
    e->rec_cv.notify_one();
    e->rec_thread.join();
  }
  if (e->ctx->upload_stream) (void)hipStreamSynchronize(e->ctx->upload_stream);
  for (uint32_t k = 0; k < e->rec_n; k++)
    for (auto& s : e->rec_takes[k].chunks) clip_release(e->ctx, s);
  e->rec_takes.reset();
  e->rec_n = 0;
}

// the audio thread, editor lock held, after the block's launches: the recorder tap (engine.cpp:1638-1649)
void rec_capture_locked(wbx_engine* e, const float* const* in, uint32_t n_in) {
  HostSession& hs = e->hs;
  if (!hs.capture_due()) return;
  wbx_ctx* c = e->ctx;
  const uint32_t F = e->rec_F;
  // a call without (all of) the recorded input channels records silence in every take — the host session counts it as a
  // silent block (REC_SILENCE), so no channel of it may be staged, the ones the short buffer does hold included
  const bool silence = !in || n_in < e->rec_in_ch;
  const uint64_t start = hs.capture_block_locked(F, silence);
  const uint32_t slot = e->rec_slot;
  const bool slot_free = e->rec_stage[slot].idle();
  uint32_t* stage = e->h_rec_stage.p + slot * e->rec_slot_words;
  uint32_t* desc = stage + (size_t)e->rec_in_ch * F;
  const uint64_t last_chunk = (start + F - 1) / e->rec_chunk;
  bool any = false;
  for (uint32_t k = 0; k < e->rec_n; k++) {
    const Take& tk = hs.takes[k];
    uint32_t d = 0;
    // (a discarded take — its track was deleted — holds no chunk and gets none: `ready` is 0, it is never written again)
    if (slot_free && e->rec_takes[k].ready.load(std::memory_order_acquire) > last_chunk)
      d = tk.ch0 << 2 | tk.channels;
    else if (tk.track)
      hs.take_status_locked(k, REC_OVERFLOW);
    if (slot_free) desc[k] = d;
    any |= d != 0u;
  }
  if (any) {
    for (uint32_t ch = 0; ch < e->rec_in_ch; ch++) {
      if (!silence && in[ch])   // (a null row of a full-width buffer stages zeros for that channel alone, without REC_SILENCE)
        std::memcpy(stage + (size_t)ch * F, in[ch], (size_t)F * sizeof(float));
      else
        std::memset(stage + (size_t)ch * F, 0, (size_t)F * sizeof(float));
    }
    RecCaptureArgs a{};
    a.stage = stage;
    a.desc = desc;
    a.table = e->d_rec_table.p;
    a.start = start;
    a.frames = F;
    a.in_channels = e->rec_in_ch;
    a.n_takes = e->rec_n;
    a.table_cap = e->rec_table_cap;
    a.chunk_frames = e->rec_chunk;
    launch_record_capture(a, c->upload_stream);
    if (hipGetLastError() != hipSuccess || e->rec_stage[slot].mark(c->upload_stream) != hipSuccess) {
      for (uint32_t k = 0; k < e->rec_n; k++) hs.take_status_locked(k, REC_OVERFLOW);
    } else {
      e->rec_slot = (slot + 1) % wbx_engine::kRecSlots;
      e->rec_captures++;
    }
  }
  e->rec_written.store(start + F, std::memory_order_release);
  const uint32_t need = rec_chunks_needed(e, start + F);
  for (uint32_t k = 0; k < e->rec_n; k++)
    if (hs.takes[k].track && e->rec_takes[k].ready.load(std::memory_order_relaxed) < need) {
      e->rec_cv.notify_one();
      break;
    }
}

// Engine::stop_record (engine.cpp:107-141); the UI thread
wbx_status stop_record_impl(wbx_engine* e) {
  wbx_ctx* c = e->ctx;
  std::vector<FinishedTake> fin;
  {
    LockGuard g(e->hs.editor_lock);
    if (!e->hs.recording) return WBX_OK;
    fin = e->hs.stop_record_locked();   // recording ends with the block in progress; every track's stop_record
    e->hs.note_edit_locked();
  }
  if (e->rec_thread.joinable()) {
    e->rec_run.store(false, std::memory_order_release);
    e->rec_cv.notify_one();
    e->rec_thread.join();
  }
  (void)hipSetDevice(c->cfg.device);
  wbx_status st = hipStreamSynchronize(c->upload_stream) == hipSuccess ? WBX_OK : WBX_ERR_DEVICE;
  // gather: one F32 clip per take (a take that captured no frame adds no clip), chunk after chunk, device to device
  std::vector<ClipSlot> built(fin.size());
  for (size_t i = 0; i < fin.size() && st == WBX_OK; i++) {
    const FinishedTake& f = fin[i];
    if (f.frames == 0) continue;
    if (f.frames >= 2147483632ull) {
      st = efail(e, WBX_ERR_UNSUPPORTED, "stop_record: a take longer than 2^31-16 frames");
      break;
    }
    ClipFill fill{};
    fill.kind = CLIP_SRC_ZERO;
    st = cfail(e, clip_build(c, built[i], WBX_FMT_F32, f.channels, c->cfg.sample_rate, f.frames, fill, c->upload_stream));
    const wbx_engine::RecTake& t = e->rec_takes[f.take];
    for (size_t j = 0; st == WBX_OK && j < t.chunks.size() && (uint64_t)j * e->rec_chunk < f.frames; j++) {
      const uint64_t at = (uint64_t)j * e->rec_chunk;
      const uint64_t n = std::min<uint64_t>(e->rec_chunk, f.frames - at);
      for (uint32_t ch = 0; ch < f.channels && st == WBX_OK; ch++)
        if (hipMemcpyAsync((char*)built[i].d.ch[ch] + at * sizeof(float), t.chunks[j].d.ch[ch], n * sizeof(float),
                           hipMemcpyDeviceToDevice, c->upload_stream) != hipSuccess)
          st = efail(e, WBX_ERR_DEVICE, "stop_record: gathering a take");
    }
  }
  if (st == WBX_OK && hipStreamSynchronize(c->upload_stream) != hipSuccess) st = efail(e, WBX_ERR_DEVICE, "stop_record: gather");
  rec_release(e);
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  bool overflow = false;
  for (size_t i = 0; i < fin.size(); i++) {
    if (!built[i].used) continue;
    const int32_t t = e->hs.track_index(fin[i].track);
    if (st != WBX_OK || t < 0) {   // (the track went while the take was gathered: its take is discarded)
      clip_release(c, built[i]);
      continue;
    }
    // Sample from the take -> SampleAsset -> add_audio_clip(track, record_min_time, record_max_time, 0.0, {speed 1, gain 1})
    uint32_t id = 0;
    const wbx_status ps = register_sample_locked(e, built[i], fin[i].channels, c->cfg.sample_rate, fin[i].frames, &id);
    if (ps != WBX_OK) {
      st = cfail(e, ps);
      continue;
    }
    e->hs.add_audio_clip_locked((uint32_t)t, fin[i].min_time, fin[i].max_time, 0.0, id, 1.0, 1.0f);
    overflow |= (fin[i].status & REC_OVERFLOW) != 0u;
  }
  e->hs.takes.clear();
  if (st == WBX_OK && overflow) return efail(e, WBX_ERR_OVERFLOW, "stop_record: a take lost blocks (no chunk was ready for them)");
  return st;
}

}  // namespace

// Engine::record (engine.cpp:95-105): the take list and its first chunks are made before the transport (re)starts, so
// the first block already has room; the recorder thread runs until stop_record.
extern "C" wbx_status wbx_engine_record(wbx_engine* e) {
  if (!e) return WBX_ERR_INVALID;
  wbx_ctx* c = e->ctx;
  std::vector<uint32_t> widths;
  uint32_t in_ch = 0;
  {
    LockGuard g(e->hs.editor_lock);
    if (e->hs.recording && e->hs.playing.load(std::memory_order_relaxed)) return WBX_OK;
    if (c->master_target || c->dist)
      return efail(e, WBX_ERR_UNSUPPORTED, "record: not with a redirected master / a multi-GPU exchange");
    if (!e->hs.record_inputs_valid()) return efail(e, WBX_ERR_INVALID, "record: a track input lies past the input channel count");
    for (auto& tp : e->hs.tracks) {
      const TrackRecord& r = tp->rec;
      if (!r.armed || r.in_type == INPUT_NONE) continue;
      widths.push_back(HostSession::input_width(r.in_type));
      in_ch = std::max(in_ch, HostSession::input_first_channel(r.in_type, r.in_index) + widths.back());
    }
  }
  rec_release(e);   // (nothing is left of an earlier take; a no-op normally)
  (void)hipSetDevice(c->cfg.device);
  const uint32_t n = (uint32_t)widths.size();
  if (n) {
    const uint32_t F = c->cfg.block_frames;
    e->rec_F = F;
    e->rec_in_ch = in_ch;
    // the table covers the longest clip the pool holds (2^31-17 frames), at most 65536 chunks per take
    e->rec_table_cap = (uint32_t)std::min<uint64_t>(65536u, (2147483631ull + e->rec_chunk - 1) / e->rec_chunk + 1);
    const size_t table = (size_t)n * e->rec_table_cap;
    WBX_EHIP(e, e->d_rec_table.ensure(table));
    WBX_EHIP(e, e->h_rec_table.ensure(table));
    e->rec_slot_words = align_up((size_t)in_ch * F + n, 64);
    WBX_EHIP(e, e->h_rec_stage.ensure(e->rec_slot_words * wbx_engine::kRecSlots));
    for (auto& S : e->rec_stage) {
      WBX_EHIP(e, S.done.ensure(hipEventDisableTiming));
      S.forget();
    }
    e->rec_slot = 0;
    e->rec_takes.reset(new wbx_engine::RecTake[n]);
    e->rec_n = n;
    for (uint32_t k = 0; k < n; k++) e->rec_takes[k].channels = widths[k];
    e->rec_written.store(0, std::memory_order_relaxed);
    e->rec_thread_err.store(WBX_OK, std::memory_order_relaxed);
    wbx_status st = rec_fill(e, 0);
    if (st == WBX_OK && hipStreamSynchronize(c->upload_stream) != hipSuccess) st = WBX_ERR_DEVICE;
    if (st != WBX_OK) {
      rec_release(e);
      return cfail(e, st);
    }
  }
  LockGuard g(e->hs.editor_lock);
  e->hs.note_edit_locked();
  e->hs.record_locked();   // (the same take list: only this thread arms tracks or sets inputs)
  if (n) {
    e->rec_run.store(true, std::memory_order_release);
    e->rec_thread = std::thread(rec_thread_main, e);
  }
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_stop_record(wbx_engine* e) {
  if (!e) return WBX_ERR_INVALID;
  return stop_record_impl(e);
}

extern "C" wbx_status wbx_engine_is_recording(wbx_engine* e, int* recording) {
  if (!e || !recording) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  *recording = e->hs.recording ? 1 : 0;
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_set_input_channels(wbx_engine* e, uint32_t input_channels) {
  if (!e) return WBX_ERR_INVALID;
  if (input_channels > 1024) return efail(e, WBX_ERR_INVALID, "set_input_channels: at most 1024");
  LockGuard g(e->hs.editor_lock);
  e->hs.input_channels = input_channels;
  return WBX_OK;
}

extern "C" wbx_status wbx_track_set_input(wbx_engine* e, uint32_t track, int type, uint32_t index, int armed) {
  if (!e) return WBX_ERR_INVALID;
  if (type == WBX_INPUT_MIDI) return efail(e, WBX_ERR_UNSUPPORTED, "set_track_input: MIDI input is not supported");
  if (type != WBX_INPUT_NONE && type != WBX_INPUT_EXTERNAL_STEREO && type != WBX_INPUT_EXTERNAL_MONO)
    return efail(e, WBX_ERR_INVALID, "set_track_input: input type");
  if (index > 0xFFFFFFu) return efail(e, WBX_ERR_INVALID, "set_track_input: index above 2^24-1 (TrackInput::as_packed_u32)");
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  e->hs.set_track_input_locked(track, (uint32_t)type, index, armed != 0);
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_arm_track_recording(wbx_engine* e, uint32_t track, int armed) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  const TrackRecord& r = e->hs.tracks[track]->rec;
  e->hs.set_track_input_locked(track, r.in_type, r.in_index, armed != 0);
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_record_info(wbx_engine* e, uint32_t track, wbx_record_info* out) {
  if (!e || !out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (!e->hs.valid_track(track)) return WBX_ERR_INVALID;
  const TrackRecord& r = e->hs.tracks[track]->rec;
  *out = wbx_record_info{};
  out->recording = r.recording ? 1 : 0;
  out->armed = r.armed ? 1 : 0;
  out->input_type = (int32_t)r.in_type;
  out->input_index = r.in_index;
  out->min_time = r.min_time;
  out->max_time = r.max_time;
  out->frames = r.last_frames;
  out->status = r.last_status;
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_set_record_chunk(wbx_engine* e, uint32_t frames, uint32_t spare_chunks) {
  if (!e) return WBX_ERR_INVALID;
  if (frames < 1 || frames > (1u << 24) || spare_chunks > 4096)
    return efail(e, WBX_ERR_INVALID, "set_record_chunk: 1 to 2^24 frames, at most 4096 spare chunks");
  LockGuard g(e->hs.editor_lock);
  if (e->hs.recording) return efail(e, WBX_ERR_UNSUPPORTED, "set_record_chunk: not while recording");
  e->rec_chunk = frames;
  e->rec_spare = spare_chunks;
  return WBX_OK;
}

namespace {
wbx_status process_block(wbx_engine* e, float* const* out_planar, int out_format, void* out_il, const float* const* in,
                         uint32_t n_in);
}

extern "C" wbx_status wbx_engine_process(wbx_engine* e, float* const* out_planar) {   // engine.cpp:1576-1654
  if (!e || !out_planar) return WBX_ERR_INVALID;
  return process_block(e, out_planar, 0, nullptr, nullptr, 0);
}

// Engine::process(input_buffer, output_buffer, sample_rate) with its input buffer: in_planar[c][0..F) for c < n_in_channels
extern "C" wbx_status wbx_engine_process_in(wbx_engine* e, const float* const* in_planar, uint32_t n_in_channels,
                                            float* const* out_planar) {
  if (!e || !in_planar || !out_planar) return WBX_ERR_INVALID;
  return process_block(e, out_planar, 0, nullptr, in_planar, n_in_channels);
}

// Engine::process + the back end's conversion to the device format (audio_io_pulseaudio.cpp:419-461:
// output_buffer.interleave_samples_to(buffer, 0, n, output_sample_format) -> core/audio_format_conv.cpp:5-91) in one
// call: the conversion is the epilogue of the sum kernel, the block arrives interleaved — no planar round trip, no extra
// launch.  dst: F * C samples of the format (packed 24-bit: the reference's bytes, see WBX_OUT_I24).
extern "C" wbx_status wbx_engine_process_interleaved(wbx_engine* e, int out_format, void* dst) {
  if (!e || !dst) return WBX_ERR_INVALID;
  if (!out_format_bytes(out_format)) return efail(e, WBX_ERR_UNSUPPORTED, "interleaved output format");
  return process_block(e, nullptr, out_format, dst, nullptr, 0);
}

// ... and with the input buffer of Engine::process (the recorder tap reads it, engine.cpp:1638-1649)
extern "C" wbx_status wbx_engine_process_interleaved_in(wbx_engine* e, const float* const* in_planar, uint32_t n_in_channels,
                                                        int out_format, void* dst) {
  if (!e || !in_planar || !dst) return WBX_ERR_INVALID;
  if (!out_format_bytes(out_format)) return efail(e, WBX_ERR_UNSUPPORTED, "interleaved output format");
  return process_block(e, nullptr, out_format, dst, in_planar, n_in_channels);
}

namespace {

wbx_status process_block_locked(wbx_engine* e, float* const* out_planar, int out_format, void* out_il, const float* const* in,
                                uint32_t n_in);

wbx_status process_block(wbx_engine* e, float* const* out_planar, int out_format, void* out_il, const float* const* in,
                         uint32_t n_in) {
  const auto t_in = std::chrono::steady_clock::now();   // ScopedPerformanceCounter, engine.cpp:1577
  LockGuard g(e->hs.editor_lock);   // held for the whole block, like editor_lock in Engine::process (engine.cpp:1587-1651)
  const wbx_status st = process_block_locked(e, out_planar, out_format, out_il, in, n_in);
  // perf_measurer.update(duration, audio_buffer_duration_ms), engine.cpp:1653 (there behind the unlock; one writer either way)
  e->hs.perf_update(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count(), e->ctx->cfg.block_frames);
  return st;
}

wbx_status process_block_locked(wbx_engine* e, float* const* out_planar, int out_format, void* out_il, const float* const* in,
                                uint32_t n_in) {
  wbx_ctx* c = e->ctx;
  if (c->master_target || c->dist) {   // the caller redirected the master: leave it there and fetch the ordinary way
    if (out_format) return efail(e, WBX_ERR_UNSUPPORTED, "wbx_engine_process_interleaved: not with a redirected master / a multi-GPU exchange");
    wbx_status st = render_locked(e, 1);
    if (st != WBX_OK) return st;
    rec_capture_locked(e, in, n_in);
    return cfail(e, wbx_fetch(c, out_planar, nullptr, nullptr));
  }
  const uint32_t C = c->cfg.channels, F = c->cfg.block_frames;
  WBX_EHIP(e, e->h_block.ensure((size_t)C * F));
  if (!e->h_status.p) {
    WBX_EHIP(e, e->h_status.ensure(wbx_engine::kStatusWords));
    std::memset(e->h_status.p, 0, wbx_engine::kStatusWords * sizeof(uint32_t));
  }
  RenderCall block;                       // what every pass over this block shares:
  block.master = e->h_block.p;            // sum_kernel's stores go over PCIe into the staging block, in the caller's format,
  block.format = out_format;
  block.status = e->h_status.p;           // and it drops the plan status next to it ...
  RenderCall first = block;
  first.clear_counters = true;            // ... the first pass clearing the counters for the buffer's next plan
  RenderResult rendered;
  wbx_status st = render_locked(e, 1, &first, &rendered);
  // the recorder tap, once per played block whichever path the block takes below (one launch, mixed again after a
  // give-up, three launches): launched on the upload stream beside the block's kernels, not waited for
  if (st == WBX_OK) rec_capture_locked(e, in, n_in);
  const bool one_launch = st == WBX_OK && rendered.one_launch;
  if (st == WBX_OK && e->hs.n_tracks() != 0) {
    if (one_launch) {
      // the kernel's own word: master and status are in host memory when it reads this launch's number.  Polled — no
      // completion signal between the device and the return of the callback; a launch that never reports (a device fault)
      // falls through to the stream's own error after two seconds
      volatile uint32_t* flag = e->h_status.p + 8;
      const uint32_t seq = e->cb_seq;
      const auto t0 = std::chrono::steady_clock::now();
      uint32_t spins = 0;
      while (*flag != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xFFFFu) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
          (void)sync_main(c);
          if (*flag != seq) {   // the launch never reported: start the ticket count afresh
            st = efail(e, WBX_ERR_DEVICE, "the one-launch callback did not report its block");
            if (c->d_cb_done.p) (void)hipMemset(c->d_cb_done.p, 0, kCbDoneWords * sizeof(uint32_t));
            c->cb_base = c->cb_base2 = 0;
          }
          break;
        }
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    } else if (hipError_t he = sync_main(c); he != hipSuccess) {
      st = WBX_ERR_DEVICE;
    }
    if (st == WBX_OK) {
      PB(c).counters_zero = e->h_status.p[2] == 0u;   // (sum_kernel cleared them unless something was queued)
      e->plan_status_on_host = true;
    }
    if (st == WBX_OK && one_launch && e->h_status.p[7] == e->cb_seq) {
      // A workgroup of the spread sum gave up waiting for the rest of its grid (the grid was not resident at once: a CU mask
      // the attribute does not show, a device shared with another process): shares of the master were added from incomplete
      // group sums.  The launch itself is over (its flag is the LAST workgroup's) and the plan is intact — the counters were
      // copied, and cleared, only by a workgroup that had seen every sequencer lane finished (workgroup 0 with the full count,
      // else the reporter, which does not clear: wbx_callback.h) —: mix and sum the block again through three launches, and
      // keep to "the last workgroup adds everything" from here on.  h_status holds the plan's counters already; this sum must
      // not drop the device's copy over them (workgroup 0 may have cleared it: an overflow bit of this block would be lost).
      c->cb_no_spread = true;
      e->cb_give_ups++;
      RenderCall again = block;
      again.status = nullptr;   // (no status destination)
      st = launch_mix_sum(c, 1, e->hs.n_tracks(), again);
      if (st == WBX_OK && sync_main(c) != hipSuccess) st = WBX_ERR_DEVICE;
      PB(c).counters_zero = false;
      if (st != WBX_OK) tls_err = c->err;
    }
    if (st == WBX_OK && rendered.pre_render_skipped && e->h_status.p[2] != 0u) {
      // the block did queue records for the pre-render pass: run it now and mix again (the plan is untouched; the
      // first pass counted those records as silence, so the running levels hold nothing wrong; the status is dropped
      // again, the counters stay: `block` as it is)
      st = launch_pre_render(c, c->stream);
      if (st == WBX_OK) st = launch_mix_sum(c, 1, e->hs.n_tracks(), block);
      if (st == WBX_OK && sync_main(c) != hipSuccess) st = WBX_ERR_DEVICE;
      PB(c).counters_zero = false;
      if (st != WBX_OK) tls_err = c->err;
    }
  }
  if (st != WBX_OK) return st;
  if (!one_launch) WBX_EHIP(e, sync_main(c));
  for (int i = 0; i < kRing; i++) e->patch[i].forget(), e->gains[i].forget();   // every plan that read them is over
  drain_events(c);
  if (out_format == 0) {
    for (uint32_t ch = 0; ch < C; ch++) std::memcpy(out_planar[ch], e->h_block.p + (size_t)ch * F, F * sizeof(float));
  } else if (out_format == WBX_OUT_I24) {   // (the reference's writer leaves the other 3*F*(C-1) bytes of the block untouched)
    std::memcpy(out_il, e->h_block.p, (size_t)F * 3);
  } else {
    std::memcpy(out_il, e->h_block.p, (size_t)F * C * out_format_bytes(out_format));
  }
  c->last_master_on_host = true;   // set after launch_mix_sum cleared it: the master of this block is e->h_block
  if (e->hs.n_tracks() == 0) return WBX_OK;
  return cfail(e, plan_status_to_error(c, e->h_status.p[1]));
}

}  // namespace

extern "C" wbx_status wbx_engine_transport(wbx_engine* e, double* playhead, double* sample_position, int* playing) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (playhead) *playhead = e->hs.playhead;
  if (sample_position) *sample_position = e->hs.sample_position;
  if (playing) *playing = e->hs.playing.load(std::memory_order_relaxed) ? 1 : 0;
  return WBX_OK;
}

// VUMeter::level of every track: the maximum since the last call, reset by the call (VUMeter::update's
// `level.exchange(0.0f)`, vu_meter.h:33).  UI thread.  Tracks that have not been through a render yet (just added, or
// the audio callback is not running) read 0.  The reference's meters are lock-free atomics; here the editor lock is held
// only while the take is enqueued behind the renders issued so far (two stream calls), never across the device wait —
// the audio thread's next block is not held up by a meter read.
extern "C" wbx_status wbx_engine_levels(wbx_engine* e, float* levels, uint32_t n_tracks) {
  if (!e || !levels) return WBX_ERR_INVALID;
  wbx_ctx* c = e->ctx;
  (void)hipSetDevice(c->cfg.device);
  uint32_t have = 0, C = 0;
  {
    LockGuard g(e->hs.editor_lock);
    C = c->cfg.channels;
    have = std::min(n_tracks, e->state_tracks);
    if (have) {
      // every render issued before this call is covered: the take is ordered after the mixes in flight
      WBX_EHIP(e, join_alt(c));
      WBX_EHIP(e, hipEventRecord(e->levels_ev, c->stream));
      WBX_EHIP(e, hipStreamWaitEvent(e->levels_stream, e->levels_ev, 0));
      launch_levels_take(reinterpret_cast<uint32_t*>(e->d_levels.p), e->h_levels.p, have * C, e->levels_stream);
    }
  }
  if (have) {
    WBX_EHIP(e, hipStreamSynchronize(e->levels_stream));
    std::memcpy(levels, e->h_levels.p, (size_t)have * C * sizeof(float));
  }
  if (n_tracks > have) std::memset(levels + (size_t)have * C, 0, (size_t)(n_tracks - have) * C * sizeof(float));
  return WBX_OK;
}

// What the last process / render took from the shared state: the number of locked edits that had completed when it
// took the editor lock, and per track the cumulative count of parameter messages it (and its predecessors) drained.
// With the UI thread's own log of what it issued this reconstructs, block by block, the exact state the audio thread
// rendered from (tests/test_gpu_threads.py).
extern "C" wbx_status wbx_engine_thread_stats(wbx_engine* e, uint64_t* edits_seen, uint64_t* drained, uint32_t n_tracks) {
  if (!e) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  if (edits_seen) *edits_seen = e->hs.render_edit_seq;
  if (drained) {
    if (n_tracks > e->hs.n_tracks()) return WBX_ERR_INVALID;
    for (uint32_t t = 0; t < n_tracks; t++) drained[t] = e->hs.tracks[t]->drained;
  }
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_sequencer_stats(wbx_engine* e, uint64_t out[4]) {
  if (!e || !out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  uint32_t st[2] = {0u, 0u};
  if (e->d_seg_stats.p && e->seam_stream) {
    WBX_EHIP(e, hipStreamSynchronize(e->seam_stream));
    WBX_EHIP(e, hipMemcpy(st, e->d_seg_stats.p, sizeof(st), hipMemcpyDeviceToHost));
  }
  out[0] = e->seg_renders;
  out[1] = st[0];
  out[2] = st[1];
  out[3] = e->seg_last_segs;
  return WBX_OK;
}

// Engine::perf_measurer.get_usage() (core/timing.h:64-66; read by ui/control_bar.cpp:54): the share of its period the audio
// callback has been taking, an exponential average over wbx_engine_process / _process_interleaved calls, clamped to [0, 1].
// Any thread.  last_block_ms (optional): the wall time of the last call, what the last update was fed.
extern "C" wbx_status wbx_engine_perf_usage(wbx_engine* e, double* usage, double* last_block_ms) {
  if (!e || !usage) return WBX_ERR_INVALID;
  *usage = e->hs.perf_get_usage();
  if (last_block_ms) {
    LockGuard g(e->hs.editor_lock);
    *last_block_ms = e->hs.last_block_ms;
  }
  return WBX_OK;
}
// the arithmetic behind it, host-only (tests hold it to the reference's PerformanceMeasurer and period helpers bit for bit)
extern "C" double wbx_calc_perf_update(double usage, double duration_ms, double period_ms) { return HostSession::perf_step(usage, duration_ms, period_ms); }
extern "C" double wbx_calc_perf_usage(double usage) { return HostSession::perf_clamped(usage); }
extern "C" double wbx_calc_buffer_period_ms(uint32_t buffer_size, uint32_t sample_rate) { return HostSession::buffer_period_ms(buffer_size, sample_rate); }

extern "C" wbx_status wbx_engine_callback_stats(wbx_engine* e, uint64_t out[4]) {
  if (!e || !out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  out[0] = e->ctx->cb_launches;
  out[1] = e->ctx->cb_spread_launches;
  out[2] = e->cb_give_ups;
  out[3] = e->ctx->cb_no_spread ? 1u : 0u;
  return WBX_OK;
}

extern "C" wbx_status wbx_engine_fetch_plan(wbx_engine* e, wbx_plan_record* out, size_t cap, size_t* n_out) {
  if (!e || !n_out) return WBX_ERR_INVALID;
  LockGuard g(e->hs.editor_lock);
  wbx_ctx* c = e->ctx;
  if (c->last_K == 0) return efail(e, WBX_ERR_FAILED, "nothing rendered");
  const uint32_t K = c->last_K, N = c->last_N;
  uint32_t pc[4] = {0, 0, 0, 0};
  WBX_EHIP(e, sync_main(c));
  if (e->plan_status_on_host)
    std::memcpy(pc, e->h_status.p, sizeof(pc));
  else
    WBX_EHIP(e, hipMemcpy(pc, PB(c).counters.p, sizeof(pc), hipMemcpyDeviceToHost));
  std::vector<DRow> rows((size_t)K * N);
  const uint32_t nt = std::min(PB(c).static_tmpl ? 2u * N : pc[3], PB(c).tmpl_cap);
  std::vector<DTrackBlock> tmpl(nt);
  if (!rows.empty()) WBX_EHIP(e, hipMemcpy(rows.data(), PB(c).prows.p, rows.size() * sizeof(DRow), hipMemcpyDeviceToHost));
  if (nt) WBX_EHIP(e, hipMemcpy(tmpl.data(), PB(c).tmpl.p, nt * sizeof(DTrackBlock), hipMemcpyDeviceToHost));
  // templates the pre-render pass rewrote: put the sequencer's originals back
  const uint32_t ng = std::min(pc[2], PB(c).gen_cap);
  if (ng) {
    std::vector<uint32_t> idx(ng);
    std::vector<DTrackBlock> saved(ng);
    WBX_EHIP(e, hipMemcpy(idx.data(), PB(c).gen_list.p, ng * sizeof(uint32_t), hipMemcpyDeviceToHost));
    WBX_EHIP(e, hipMemcpy(saved.data(), PB(c).saved.p, ng * sizeof(DTrackBlock), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < ng; i++)
      if (idx[i] < tmpl.size()) tmpl[idx[i]] = saved[i];
  }
  const uint32_t used = std::min(pc[0], PB(c).pool_chunks);
  std::vector<DSeg> pool((size_t)used * kChunk);
  if (used) WBX_EHIP(e, hipMemcpy(pool.data(), PB(c).pool.p, pool.size() * sizeof(DSeg), hipMemcpyDeviceToHost));
  const size_t n = plan_records(K, N, rows.data(), tmpl.data(), tmpl.size(), pool.data(), used, out, cap);
  *n_out = n;
  // (every status bit the way wbx_fetch reports it — bit 7, the segmented sequencer's XCD check, included; bit 3, "more
  //  boundary rows than pre-render rows", concerns the audio, not the records handed out here)
  return cfail(e, plan_status_to_error(c, pc[1] & ~8u));
}
