// host_sim.cpp — TEST HARNESS: the host side of layer 2 without a device.
//
// Compiles the product's own host headers — wbx_host.h (session state, SPSC parameter rings, editor lock, clip edits)
// and wbx_seq.h (the clip sequencer: the very source plan_kernel runs one lane per track) — with plain g++ and runs the
// sequencer track by track on the CPU.  No per-sample work exists here and nothing of this is linked into libwbx.so;
// it gives the seek math and the clip-edit logic CPU-side coverage against the oracle (tests/test_host_sim.py) and,
// built with -fsanitize=thread -DHOST_SIM_MAIN, a ThreadSanitizer run of the UI-thread / audio-thread contract.
//
//   g++ -std=c++20 -O2 -ffp-contract=off -shared -fPIC host_sim.cpp -o libwbxhostsim.so
//   g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=thread -DHOST_SIM_MAIN host_sim.cpp -o host_tsan -lpthread
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/wbx.h"
#include "../../whitebox_amd/csrc/wbx_host.h"
#include "../../whitebox_amd/csrc/wbx_seq.h"
#include "../../whitebox_amd/csrc/wbx_shape.h"

using namespace wbx;

struct HostSim {
  HostSession hs;
  uint32_t block_frames = 512, channels = 2, max_blocks = 1;
  // what lives in HBM in the product
  std::vector<DSample> samples;
  std::vector<DClip> clips;
  std::vector<uint32_t> clip_first;
  std::vector<DTrackState> state;
  std::vector<float> gains;
  std::vector<DPatch> patch;
  // the plan of the last render
  std::vector<DRow> rows;
  std::vector<DTrackBlock> tmpl;
  std::vector<DSeg> pool;
  std::vector<uint32_t> gen_list;
  uint32_t counters[4] = {0, 0, 0, 0};
  uint32_t last_K = 0, last_N = 0;
  bool clips_uploaded = false;
  uint32_t masked_rows = 0;   // plan as for a mix instance that takes partial rows / ROW_PAIRs in its hot loop
  // the sequencer cut along the time axis (wbx_seq.h plan_segment / plan_check_seams): blocks per segment (0: one walk per
  // track), and what the seam check found — renders planned that way, tracks with a seam that did not hold, segments redone
  uint32_t seg_len = 0;
  bool table_flags = false;
  uint32_t flags_left = 0;    // set internal_state_changed flags of the table (the sequencer counts down as it clears them)
  uint64_t seg_renders = 0, seg_tracks_redone = 0, seg_segments_redone = 0, seg_lanes = 0;
};

extern "C" {

HostSim* hsim_create(uint32_t max_tracks, uint32_t max_blocks, uint32_t block_frames, uint32_t channels, uint32_t sample_rate) {
  HostSim* s = new HostSim();
  s->hs.max_tracks = max_tracks;
  s->hs.dst_rate = sample_rate;
  s->block_frames = block_frames;
  s->channels = channels;
  s->max_blocks = max_blocks;
  return s;
}
void hsim_destroy(HostSim* s) { delete s; }
void hsim_set_masked_rows(HostSim* s, uint32_t on) { s->masked_rows = on; }
void hsim_set_segments(HostSim* s, uint32_t seg_len) { s->seg_len = seg_len; }
void hsim_segment_stats(HostSim* s, uint64_t* out4) {
  out4[0] = s->seg_renders;
  out4[1] = s->seg_tracks_redone;
  out4[2] = s->seg_segments_redone;
  out4[3] = s->seg_lanes;
}

// (row flags, template kind) of every (block, track) of the last render — how the sequencer classified each track-block
int hsim_row_kinds(HostSim* s, uint32_t* flags, uint32_t* kinds, size_t cap) {
  const size_t n = (size_t)s->last_K * s->last_N;
  if (cap < n) return WBX_ERR_INVALID;
  for (size_t i = 0; i < n; i++) {
    flags[i] = s->rows[i].flags;
    kinds[i] = s->rows[i].tmpl < s->tmpl.size() ? s->tmpl[s->rows[i].tmpl].kind : 0xFFu;
  }
  return WBX_OK;
}

int hsim_set_bpm(HostSim* s, double bpm) {
  if (!(bpm > 0.0)) return WBX_ERR_INVALID;
  s->hs.set_bpm(bpm);
  return WBX_OK;
}
int hsim_set_playhead_position(HostSim* s, double beat) {
  LockGuard g(s->hs.editor_lock);
  s->hs.set_playhead_position_locked(beat);
  s->hs.note_edit_locked();
  return WBX_OK;
}
int hsim_add_track(HostSim* s, uint32_t* out) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (s->hs.n_tracks() >= s->hs.max_tracks) return WBX_ERR_INVALID;
  const uint32_t t = s->hs.add_track_locked();
  if (out) *out = t;
  return WBX_OK;
}
int hsim_track_set_volume(HostSim* s, uint32_t t, float db) {
  if (!s->hs.valid_track(t)) return WBX_ERR_INVALID;
  s->hs.set_volume(t, db);
  return WBX_OK;
}
int hsim_track_set_pan(HostSim* s, uint32_t t, float pan) {
  if (!s->hs.valid_track(t)) return WBX_ERR_INVALID;
  s->hs.set_pan(t, pan);
  return WBX_OK;
}
int hsim_track_set_mute(HostSim* s, uint32_t t, int m) {
  if (!s->hs.valid_track(t)) return WBX_ERR_INVALID;
  s->hs.set_mute(t, m != 0);
  return WBX_OK;
}
int hsim_solo_track(HostSim* s, uint32_t t) {
  if (!s->hs.valid_track(t)) return WBX_ERR_INVALID;
  s->hs.solo_track(t);
  return WBX_OK;
}

static int permute(HostSim* s, const std::vector<uint32_t>& order) {
  std::vector<DTrackState> st2(order.size());
  for (size_t i = 0; i < order.size(); i++) st2[i] = order[i] < s->state.size() ? s->state[order[i]] : DTrackState{};
  s->state = st2;
  s->hs.permute_tracks_locked(order);
  return WBX_OK;
}
int hsim_delete_track(HostSim* s, uint32_t slot) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(slot)) return WBX_ERR_INVALID;
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < s->hs.n_tracks(); i++)
    if (i != slot) order.push_back(i);
  return permute(s, order);
}
int hsim_move_track(HostSim* s, uint32_t from, uint32_t to) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(from) || !s->hs.valid_track(to)) return WBX_ERR_INVALID;
  if (from == to) return WBX_OK;
  std::vector<uint32_t> order(s->hs.n_tracks());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  order.erase(order.begin() + from);
  order.insert(order.begin() + to, from);
  return permute(s, order);
}

// a sample asset: only what the sequencer reads of it (rate, length, format); the channel pointers are fake addresses
int hsim_add_sample(HostSim* s, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames, uint32_t* out) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  const uint32_t id = (uint32_t)s->samples.size();
  DSample d{};
  d.ch[0] = (const void*)(((uintptr_t)id + 1u) << 32);
  d.ch[1] = channels > 1 ? (const void*)((((uintptr_t)id + 1u) << 32) + (1u << 31)) : d.ch[0];
  d.count = frames;
  d.format = (uint32_t)format;
  d.channels = channels;
  d.sample_rate = sample_rate;
  s->samples.push_back(d);
  s->hs.samples.push_back(SampleMeta{(uint32_t)format, channels, sample_rate, frames, true});
  *out = id;
  return WBX_OK;
}

int hsim_add_audio_clip(HostSim* s, uint32_t track, double mn, double mx, double so, uint32_t sample, double speed, float gain) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || !s->hs.valid_sample(sample) || !(mn <= mx)) return WBX_ERR_INVALID;
  s->hs.add_audio_clip_locked(track, mn, mx, so, sample, speed, gain);
  return WBX_OK;
}
int hsim_move_clip(HostSim* s, uint32_t track, uint32_t clip, double rel) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || clip >= s->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  s->hs.move_clip_locked(track, clip, rel);
  return WBX_OK;
}
int hsim_resize_clip(HostSim* s, uint32_t track, uint32_t clip, double rel, double limit, double min_length, int left, int shift,
                     int stretch) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || clip >= s->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  s->hs.resize_clip_locked(track, clip, rel, limit, min_length, left != 0, shift != 0, stretch != 0);
  return WBX_OK;
}
int hsim_delete_clip(HostSim* s, uint32_t track, uint32_t clip) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || clip >= s->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  s->hs.delete_clip_locked(track, clip);
  return WBX_OK;
}
int hsim_delete_region(HostSim* s, uint32_t track, double mn, double mx) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || !(mn <= mx)) return WBX_ERR_INVALID;
  s->hs.delete_region_locked(track, mn, mx);
  return WBX_OK;
}
int hsim_set_clip_gain(HostSim* s, uint32_t track, uint32_t clip, float gain) {
  LockGuard g(s->hs.editor_lock);
  s->hs.note_edit_locked();
  if (!s->hs.valid_track(track) || clip >= s->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  s->hs.set_clip_gain_locked(track, clip, gain);
  return WBX_OK;
}
int hsim_clip_count(HostSim* s, uint32_t track, uint32_t* n) {
  LockGuard g(s->hs.editor_lock);
  if (!s->hs.valid_track(track)) return WBX_ERR_INVALID;
  *n = (uint32_t)s->hs.tracks[track]->clips.size();
  return WBX_OK;
}
int hsim_get_clip(HostSim* s, uint32_t track, uint32_t clip, wbx_clip_info* out) {
  LockGuard g(s->hs.editor_lock);
  if (!s->hs.valid_track(track) || clip >= s->hs.tracks[track]->clips.size()) return WBX_ERR_INVALID;
  const DClip& d = s->hs.tracks[track]->clips[clip].d;
  *out = wbx_clip_info{d.min_time, d.max_time, d.start_offset, d.speed, d.gain, d.sample};
  return WBX_OK;
}
int hsim_play(HostSim* s) {
  LockGuard g(s->hs.editor_lock);
  s->hs.play_locked();
  s->hs.note_edit_locked();
  return WBX_OK;
}
int hsim_stop(HostSim* s) {
  LockGuard g(s->hs.editor_lock);
  s->hs.stop_locked();
  s->hs.note_edit_locked();
  return WBX_OK;
}

// the audio thread's render: the host side of wbx_engine_render (wbx_engine.hip render_locked) with the plan kernel's
// work done here, track by track
int hsim_render(HostSim* s, uint32_t K) {
  if (K == 0 || K > s->max_blocks) return WBX_ERR_INVALID;
  LockGuard g(s->hs.editor_lock);
  HostSession& hs = s->hs;
  const uint32_t N = hs.n_tracks(), F = s->block_frames;
  hs.render_edit_seq = hs.edit_seq;
  const double beat_duration = hs.beat_duration.load(std::memory_order_relaxed);
  const bool playing = hs.playing.load(std::memory_order_relaxed);
  s->last_K = K;
  s->last_N = N;
  if (N == 0) {
    hs.advance_transport_locked(K, F, beat_duration);
    return WBX_OK;
  }
  if (hs.drain_params_locked()) hs.build_gains_locked(s->gains);
  if (hs.clips_dirty) {
    if (s->clips_uploaded && !s->clips.empty()) hs.merge_live_flags_locked(s->clips.data(), s->clips.size());
    hs.flatten_clips_locked(s->clips, s->clip_first);
    s->clips_uploaded = true;
    s->flags_left = 0;
    for (const DClip& dc : s->clips) s->flags_left += dc.internal_state_changed != 0 ? 1u : 0u;
    s->table_flags = s->flags_left != 0u;
  }
  if (s->state.size() < N) s->state.resize(N, DTrackState{});
  const DPatch* patch = nullptr;
  if (hs.patches_pending) {
    s->patch.resize(N);
    hs.take_patches_locked(s->patch.data());
    patch = s->patch.data();
  }
  hs.routing_dirty = false;
  s->rows.assign((size_t)K * N, DRow{});
  // (the conditions of choose_plan, wbx_shape.h, with a forced segment length)
  if (s->table_flags && s->flags_left == 0u) s->table_flags = false;
  const uint32_t L = (s->seg_len && s->seg_len < K && playing && !s->table_flags) ? s->seg_len : 0u;
  const uint32_t S = L ? (K + L - 1u) / L : 1u;
  s->tmpl.assign(hs.template_hint(K, S) + 64, DTrackBlock{});
  s->gen_list.assign(hs.gen_rows_hint(K) + 64, 0u);
  const uint32_t pool_chunks = (uint32_t)std::max<size_t>(1024, (size_t)s->max_blocks * hs.max_tracks / 8);
  s->pool.assign((size_t)pool_chunks * kChunk, DSeg{});
  std::memset(s->counters, 0, sizeof(s->counters));
  PlanArgs a{};
  a.clips = s->clips.data();
  a.clip_first = s->clip_first.data();
  a.samples = s->samples.data();
  a.state = s->state.data();
  a.patch = patch;
  a.gains = s->gains.data();
  a.rows = s->rows.data();
  a.tmpl = s->tmpl.data();
  a.tmpl_count = &s->counters[3];
  a.tmpl_cap = (uint32_t)s->tmpl.size();
  a.pool = s->pool.data();
  a.pool_count = &s->counters[0];
  a.status = &s->counters[1];
  a.gen_list = s->gen_list.data();
  a.gen_count = &s->counters[2];
  a.gen_cap = (uint32_t)s->gen_list.size();
  a.pool_chunks = pool_chunks;
  a.n_tracks = N;
  a.n_blocks = K;
  a.block_frames = F;
  a.channels = s->channels;
  a.sample_rate = (double)hs.dst_rate;
  a.playing = playing ? 1u : 0u;
  a.clips_changed = hs.clips_edited ? 1u : 0u;
  a.flags_left = &s->flags_left;
  hs.clips_edited = false;
  a.masked_rows = s->masked_rows;
  a.tmpl_reserve = template_reserve(K);
  a.playhead = hs.playhead;
  a.sample_position = hs.sample_position;
  a.beat_duration = beat_duration;
  std::vector<DBlockTime> times(K);
  block_times(a, times.data());
  if (L) {
    // every lane of plan_seg_kernel, in an order no lane may rely on (segments backwards, tracks forwards), then the seam pass
    a.tmpl_reserve = kSegmentTemplateReserve;
    std::vector<DTrackState> guess((size_t)N * S), ends((size_t)N * S);
    const DBlockTime* tv = times.data();
    for (uint32_t sg = S; sg-- > 0u;)
      for (uint32_t t = 0; t < N; t++) plan_segment(a, t, sg, L, S, tv, &guess[(size_t)t * S + sg], &ends[(size_t)t * S + sg]);
    for (uint32_t t = 0; t < N; t++) {
      const uint32_t bad = plan_check_seams(a, t, S, guess.data(), ends.data(), [](const DTrackState* p) { return *p; });
      if (bad < S) {
        plan_redo_track(a, t, bad, L, tv, ends[(size_t)t * S + bad - 1u]);
        s->seg_tracks_redone += 1u;
        s->seg_segments_redone += S - bad;
      }
    }
    s->seg_renders++;
    s->seg_lanes += (uint64_t)N * (S - 1u);
  } else {
    for (uint32_t t = 0; t < N; t++) plan_track(a, t, times.data());
  }
  hs.advance_transport_locked(K, F, beat_duration);
  return WBX_OK;
}

// The shape of a render of K blocks of this session (wbx_shape.h: the mix instance and what follows from it): the session's
// facts as render_locked fills them (HostSession::shape_facts), the clip table's as upload_tables derives them, the group
// size as wbx_create resolves it, the knobs read from the environment by the reader wbx_create calls.  The harness has no
// routing: the caller says how many buses there are and how many tracks the longest member list holds.
struct HsimShape {
  char mix[64], callback[64];   // the instances' names as nm -C spells them
  uint32_t family, masked_rows, walks_lists, chained, blocks_per_workgroup, mix_sb, cb_one_launch, cb_lane_span;
};
int hsim_render_shape(HostSim* s, uint32_t K, uint32_t group_size, uint32_t n_buses, uint32_t longest_list, int process_block, HsimShape* out) {
  if (K == 0 || K > s->max_blocks) return WBX_ERR_INVALID;
  LockGuard g(s->hs.editor_lock);
  ShapeFacts f;
  f.channels = s->channels;
  f.block_frames = s->block_frames;
  f.auto_group = group_size == 0;
  f.group_size = group_size ? group_size : s->max_blocks == 1 ? kStage / 2 : kStage;
  f.session = s->hs.shape_facts();
  for (const DSample& d : s->samples) {
    if (d.format != FMT_F32) f.integer_clips = true;
    if (d.format != FMT_I16) f.non16_clips = true;
  }
  f.n_buses = n_buses;
  f.longest_list = longest_list;
  f.n_blocks = K;
  f.n_tracks = s->hs.n_tracks();
  f.callback = process_block != 0 && !s->hs.any_slow_clip;
  const RenderShape r = choose_shape(ShapeKnobs::from_env(), f);
  r.mix.name(out->mix, sizeof(out->mix));
  r.cb.name(out->callback, sizeof(out->callback));
  out->family = (uint32_t)r.family;
  out->masked_rows = r.masked_rows;
  out->walks_lists = r.walks_lists;
  out->chained = r.chained;
  out->blocks_per_workgroup = r.blocks_per_workgroup;
  out->mix_sb = r.mix.SB;
  out->cb_one_launch = r.cb_one_launch;
  out->cb_lane_span = r.cb_lane_span;
  return WBX_OK;
}

// ShapeKnobs::from_env() as the environment stands now (wbx_knobs.h), field by field in the struct's order
struct HsimKnobs {
  int32_t ragged_off, cb_any_off, masked_rows_off, chain_off, no_lean16, no_fam3, no_cl2, callback_unfused, force_cut, force_g,
      packed_x, mix_variant, cb_u, exact_min_blocks;
};
void hsim_shape_knobs(HsimKnobs* out) {
  const ShapeKnobs k = ShapeKnobs::from_env();
  *out = HsimKnobs{k.ragged_off, k.cb_any_off, k.masked_rows_off, k.chain_off, k.no_lean16, k.no_fam3, k.no_cl2, k.callback_unfused,
                   k.force_cut, k.force_g, k.packed_x, k.mix_variant, k.cb_u, (int32_t)k.exact_min_blocks};
}

// How a render is issued (wbx_shape.h: choose_issue).  The numbers are passed as they are; the boolean facts and the five
// CtxKnobs that enter (and `overlap`, which must not) as one word — bit 0 chained, 1 cb_one_launch, 2 callback_plan, 3 dist,
// 4 init, 5 target_set, 6 target_on_host, 7 mix_on_main, 8 cb_no_spread, 9 sum_overlap, 10 profiling, 11 mix_alternate,
// 12 cu_mask, 13 overlap (kIssueBits of them).
constexpr uint32_t kIssueBits = 14;
struct HsimIssue {
  uint32_t sum_beside, fused, timed, one_launch, by_kernel_event, spread;
  uint64_t stage_bytes;
};
static RenderIssue issue_of(uint32_t K, uint32_t n_groups, uint32_t n_buses, uint32_t tiles, uint32_t F, uint32_t C, int format, uint32_t n_cus,
                            uint32_t bits) {
  IssueFacts f;
  f.K = K, f.n_groups = n_groups, f.n_buses = n_buses, f.tiles = tiles, f.block_frames = F, f.channels = C;
  f.master_format = format;
  f.n_cus = n_cus;
  f.chained = bits >> 0 & 1u, f.cb_one_launch = bits >> 1 & 1u, f.callback_plan = bits >> 2 & 1u, f.dist = bits >> 3 & 1u;
  f.init = bits >> 4 & 1u, f.target_set = bits >> 5 & 1u, f.target_on_host = bits >> 6 & 1u, f.mix_on_main = bits >> 7 & 1u;
  f.cb_no_spread = bits >> 8 & 1u;
  CtxKnobs k;
  k.sum_overlap = bits >> 9 & 1u, k.profiling = bits >> 10 & 1u, k.mix_alternate = bits >> 11 & 1u, k.cu_mask = bits >> 12 & 1u;
  k.overlap = bits >> 13 & 1u;
  return choose_issue(k, f);
}
void hsim_render_issue(uint32_t K, uint32_t n_groups, uint32_t n_buses, uint32_t tiles, uint32_t F, uint32_t C, int format, uint32_t n_cus,
                       uint32_t bits, HsimIssue* out) {
  const RenderIssue r = issue_of(K, n_groups, n_buses, tiles, F, C, format, n_cus, bits);
  *out = HsimIssue{r.sum_beside, r.fused, r.timed, r.one_launch, r.by_kernel_event, r.spread, r.stage_bytes};
}
// ... for every value of the word at once: flags[bits] = sum_beside | fused << 1 | timed << 2 | one_launch << 3 |
// by_kernel_event << 4 | spread << 5, stage[bits] = stage_bytes (1 << kIssueBits entries each)
void hsim_render_issue_all(uint32_t K, uint32_t n_groups, uint32_t n_buses, uint32_t tiles, uint32_t F, uint32_t C, int format, uint32_t n_cus,
                           uint8_t* flags, uint64_t* stage) {
  for (uint32_t bits = 0; bits < (1u << kIssueBits); bits++) {
    const RenderIssue r = issue_of(K, n_groups, n_buses, tiles, F, C, format, n_cus, bits);
    flags[bits] = (uint8_t)(r.sum_beside | r.fused << 1 | r.timed << 2 | r.one_launch << 3 | r.by_kernel_event << 4 | r.spread << 5);
    stage[bits] = r.stage_bytes;
  }
}

// How a render is planned (wbx_shape.h: choose_plan).  K, N, EngineKnobs::plan_seg and the shape's masked_rows are passed as
// they are; the boolean facts and knobs as one word — bit 0 playing, 1 callback, 2 any_slow_clip, 3 cut, 4 table_flags,
// 5 seg_broken, 6 cb_one_launch, 7 counters_zero, 8 overlap, 9 force_cut (kPlanBits of them).
constexpr uint32_t kPlanBits = 10;
struct HsimPlan {
  uint32_t seg_len, n_segs, tmpl_reserve, flags;   // flags: plan_flags below
};
static RenderPlan plan_of(uint32_t K, uint32_t N, int plan_seg, uint32_t masked_rows, uint32_t bits) {
  PlanFacts f;
  f.K = K, f.N = N, f.masked_rows = masked_rows;
  f.playing = bits >> 0 & 1u, f.callback = bits >> 1 & 1u, f.any_slow_clip = bits >> 2 & 1u, f.cut = bits >> 3 & 1u;
  f.table_flags = bits >> 4 & 1u, f.seg_broken = bits >> 5 & 1u, f.cb_one_launch = bits >> 6 & 1u, f.counters_zero = bits >> 7 & 1u;
  EngineKnobs ek;
  ek.plan_seg = plan_seg;
  CtxKnobs ck;
  ck.overlap = bits >> 8 & 1u;
  ShapeKnobs sk;
  sk.force_cut = bits >> 9 & 1u;
  return choose_plan(ek, ck, sk, f);
}
// beside | device_times << 1 | skip_pre_render << 2 | static_tmpl << 3 | double_rows << 4 | pool_slack << 5 | sequencer << 6
// (0 plain, 1 segments, 2 none) | zeroing << 8 (0 nobody, 1 the times-copy kernel, 2 a memset)
static uint32_t plan_flags(const RenderPlan& r) {
  return (uint32_t)r.beside | (uint32_t)r.device_times << 1 | (uint32_t)r.skip_pre_render << 2 | (uint32_t)r.static_tmpl << 3 |
         (uint32_t)r.double_rows << 4 | (uint32_t)r.pool_slack << 5 | (uint32_t)r.sequencer << 6 | (uint32_t)r.zeroing << 8;
}
void hsim_render_plan(uint32_t K, uint32_t N, int plan_seg, uint32_t masked_rows, uint32_t bits, HsimPlan* out) {
  const RenderPlan r = plan_of(K, N, plan_seg, masked_rows, bits);
  *out = HsimPlan{r.seg_len, r.n_segs, r.tmpl_reserve, plan_flags(r)};
}
// ... for every value of the word at once (1 << kPlanBits entries)
void hsim_render_plan_all(uint32_t K, uint32_t N, int plan_seg, uint32_t masked_rows, HsimPlan* out) {
  for (uint32_t bits = 0; bits < (1u << kPlanBits); bits++) hsim_render_plan(K, N, plan_seg, masked_rows, bits, out + bits);
}

// plan status bits of the last render (PlanArgs::status) and the number of templates / pre-render rows it used
int hsim_plan_counters(HostSim* s, uint32_t* out4) {
  std::memcpy(out4, s->counters, sizeof(s->counters));
  return WBX_OK;
}
uint32_t hsim_template_capacity(HostSim* s) { return (uint32_t)s->tmpl.size(); }

int hsim_fetch_plan(HostSim* s, wbx_plan_record* out, size_t cap, size_t* n_out) {
  LockGuard g(s->hs.editor_lock);
  const uint32_t used = std::min<uint32_t>(s->counters[0], (uint32_t)(s->pool.size() / kChunk));
  const size_t nt = std::min<size_t>(s->counters[3], s->tmpl.size());
  *n_out = plan_records(s->last_K, s->last_N, s->rows.data(), s->tmpl.data(), nt, s->pool.data(), used, out, cap);
  if (s->counters[1] & 3u) return WBX_ERR_OVERFLOW;
  if (s->counters[1] & 16u) return WBX_ERR_OVERFLOW;
  return WBX_OK;
}

// the gains the mix would use: [N][2] fl(volume * pan_coeffs[c]) after the last render's drain
int hsim_gains(HostSim* s, float* out, uint32_t n_tracks) {
  LockGuard g(s->hs.editor_lock);
  if (n_tracks * 2 > s->gains.size()) return WBX_ERR_INVALID;
  std::memcpy(out, s->gains.data(), (size_t)n_tracks * 2 * sizeof(float));
  return WBX_OK;
}

int hsim_transport(HostSim* s, double* playhead, double* sample_position, int* playing) {
  LockGuard g(s->hs.editor_lock);
  *playhead = s->hs.playhead;
  *sample_position = s->hs.sample_position;
  *playing = s->hs.playing.load() ? 1 : 0;
  return WBX_OK;
}

int hsim_thread_stats(HostSim* s, uint64_t* edits_seen, uint64_t* drained, uint32_t n_tracks) {
  LockGuard g(s->hs.editor_lock);
  if (edits_seen) *edits_seen = s->hs.render_edit_seq;
  if (drained) {
    if (n_tracks > s->hs.n_tracks()) return WBX_ERR_INVALID;
    for (uint32_t t = 0; t < n_tracks; t++) drained[t] = s->hs.tracks[t]->drained;
  }
  return WBX_OK;
}

}  // extern "C"

#ifdef HOST_SIM_MAIN
// ThreadSanitizer driver: one UI thread hammering Track::set_volume / set_pan / set_mute (lock-free rings) and clip
// edits (editor lock) while the audio thread renders block after block — the reference's two-thread contract.  Checks
// on top of TSan's race detection: every message pushed is eventually drained, in order per track (the last value of
// each parameter wins), and the edit counter the audio thread saw never runs backwards.
#include <atomic>
#include <cmath>
int main() {
  const uint32_t N = 24, BLOCKS = 3000;
  HostSim* s = hsim_create(N, 1, 128, 2, 48000);
  hsim_set_bpm(s, 120.0);
  uint32_t smp = 0;
  hsim_add_sample(s, WBX_FMT_F32, 2, 44100, 200000, &smp);
  for (uint32_t t = 0; t < N; t++) {
    uint32_t id;
    hsim_add_track(s, &id);
    for (int k = 0; k < 4; k++) hsim_add_audio_clip(s, t, 0.05 * k + 0.001 * t, 0.05 * k + 0.04, 10.0 * k, smp, k & 1 ? 0.5 : 1.0, 1.0f);
  }
  hsim_play(s);
  std::atomic<bool> stop{false};
  std::atomic<uint64_t> pushed{0};
  float last_db[N];
  for (uint32_t t = 0; t < N; t++) last_db[t] = 0.0f;
  std::thread ui([&] {
    uint64_t i = 0;
    while (!stop.load(std::memory_order_relaxed)) {
      const uint32_t t = (uint32_t)(i * 7u % N);
      const float db = -0.25f * (float)(i % 97u);
      hsim_track_set_volume(s, t, db);
      last_db[t] = db;
      hsim_track_set_pan(s, t, (float)((int)(i % 21u) - 10) * 0.1f);
      if (i % 5u == 0) hsim_track_set_mute(s, t, (int)((i / 5u) & 1u));
      pushed.fetch_add(i % 5u == 0 ? 3 : 2, std::memory_order_relaxed);
      if (i % 3u == 0) {
        uint32_t n = 0;
        hsim_clip_count(s, t, &n);
        if (n) {
          if (i % 9u == 0)
            hsim_move_clip(s, t, (uint32_t)(i % n), ((i & 1u) ? 1.0 : -1.0) * 0.003);
          else
            hsim_set_clip_gain(s, t, (uint32_t)(i % n), 0.5f + 0.01f * (float)(i % 50u));
        }
      }
      if (i % 997u == 0) hsim_set_bpm(s, 100.0 + (double)(i % 40u));
      i++;
    }
  });
  uint64_t prev_seen = 0;
  bool ok = true;
  for (uint32_t b = 0; b < BLOCKS; b++) {
    if (hsim_render(s, 1) != WBX_OK) ok = false;
    uint64_t seen = 0;
    hsim_thread_stats(s, &seen, nullptr, 0);
    if (seen < prev_seen) ok = false;
    prev_seen = seen;
    if (b == BLOCKS / 2) {
      hsim_stop(s);
      hsim_play(s);
    }
  }
  stop.store(true);
  ui.join();
  hsim_render(s, 1);   // drains what the UI thread pushed last
  uint64_t drained[N], total = 0;
  hsim_thread_stats(s, nullptr, drained, N);
  for (uint32_t t = 0; t < N; t++) total += drained[t];
  // Track::Track pushes three messages per track (track.cpp:22-27)
  if (total != pushed.load() + 3ull * N) {
    std::printf("drained %llu of %llu messages\n", (unsigned long long)total, (unsigned long long)(pushed.load() + 3ull * N));
    ok = false;
  }
  for (uint32_t t = 0; t < N; t++)
    if (s->hs.tracks[t]->volume != db_to_linear(last_db[t])) ok = false;
  hsim_destroy(s);
  std::printf(ok ? "host_tsan ok\n" : "host_tsan FAILED\n");
  return ok ? 0 : 1;
}
#endif

#ifdef HOST_SIM_KNOBS_MAIN
// wbx_knobs.h and wbx_shape.h stand-alone, for a build with -fsanitize=address,undefined: every reader with the environment
// empty and with each switch set, choose_shape and choose_issue over a sweep of sessions and render lengths under each
// setting, and choose_plan over every value of its fact word.
#include <array>
#include <cstdlib>
#include <iterator>
int main() {
  static const char* const kShape[][2] = {{"WBX_RAGGED", "0"}, {"WBX_CB_ANY", "0"}, {"WBX_MASKED_ROWS", "0"}, {"WBX_CHAIN", "0"},
      {"WBX_NO_LEAN16", "1"}, {"WBX_NO_FAM3", "1"}, {"WBX_NO_CL2", "1"}, {"WBX_CALLBACK_FUSED", "0"}, {"WBX_FORCE_CUT", "1"},
      {"WBX_FORCE_G", "1"}, {"WBX_PACKED_X", "1"}, {"WBX_MIX_VARIANT", "1023"}, {"WBX_CB_U", "8"}, {"WBX_EXACT_MIN_BLOCKS", "0"}};
  static const char* const kOther[][2] = {{"WBX_OVERLAP", "0"}, {"WBX_SUM_OVERLAP", "0"}, {"WBX_MIX_ALT", "1"}, {"WBX_KERNEL_TIMER", "0"},
      {"WBX_CB_SPIN_BOUND", "0"}, {"WBX_NO_UNIFORM", "1"}, {"WBX_CB_FENCED", "1"}, {"WBX_FAST_PARTIAL", "0"}, {"WBX_XCD_PROBE_FAIL", "1"},
      {"WBX_DBG_CLOCK", "1"}, {"WBX_CB_DBG", "1"}, {"HSA_CU_MASK", "0:0-7"}, {"WBX_PLAN_SEG", "-5"}, {"WBX_PLAN_LANES", "16"},
      {"WBX_DIST_INIT_TIMEOUT_S", "2.5"}};
  for (auto& kv : kShape) unsetenv(kv[0]);
  for (auto& kv : kOther) unsetenv(kv[0]);
  unsetenv("ROC_GLOBAL_CU_MASK");
  bool ok = true;
  auto flat = [] {
    HsimKnobs h;
    hsim_shape_knobs(&h);
    return h;
  };
  const HsimKnobs d = flat();
  ok = ok && std::memcmp(&d, std::array<int32_t, 14>{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 1024}.data(), sizeof d) == 0;
  uint64_t shapes = 0, issues = 0;
  auto sweep = [&] {   // choose_shape over sessions x block shapes x render lengths, the knobs as the environment sets them
    const ShapeKnobs k = ShapeKnobs::from_env();
    for (uint32_t bits = 0; bits < 64u; bits++)
      for (uint32_t F : {128u, 256u, 480u, 512u, 1024u})
        for (uint32_t C : {1u, 2u})
          for (uint32_t K : {1u, 8u, 256u, 2048u}) {
            ShapeFacts f;
            f.channels = C;
            f.block_frames = F;
            f.auto_group = true;
            f.group_size = K == 1u ? kStage / 2 : kStage;
            f.session.window_clips = bits & 1u;
            f.session.stride_clips = bits & 2u;
            f.session.taps_clips = bits & 2u;
            f.session.lean16_clips = bits & 4u;
            f.session.cut_tracks = bits & 8u;
            f.session.host_sequenced = false;
            f.integer_clips = bits & 16u;
            f.non16_clips = !(bits & 4u);
            f.n_buses = (bits & 32u) ? 2u : 0u;
            f.longest_list = 4096u;
            f.n_blocks = K;
            f.n_tracks = 4096u;
            f.callback = K == 1u;
            char name[96];
            const RenderShape r = choose_shape(k, f);
            r.mix.name(name, sizeof name);
            r.cb.name(name, sizeof name);
            shapes += r.mix.key() != 0u;
            // ... and how that render is issued (choose_issue): no group, one, more than the spread limit, over a thinned fact word
            for (uint32_t n_groups : {0u, 1u, 257u})
              for (uint32_t bits = 0; bits < (1u << kIssueBits); bits += 331u) {
                const RenderIssue is = issue_of(K, n_groups, f.n_buses, r.tiles, F, C, (bits & 1u) ? WBX_OUT_I16 : 0, K == 8u ? 64u : 304u,
                                                bits ^ (r.chained ? 1u : 0u));
                issues += is.stage_bytes != 0u || is.sum_beside || !is.spread;
              }
          }
  };
  sweep();
  // choose_issue over every value of the fact word, at both sides of the 4 MiB staging edge (blocks of 512 x 2 in 16 bits:
  // 2048 of them are 4 MiB, 2047 are not) and of the spread limit
  for (uint32_t K : {1u, 7u, 8u, 2047u, 2048u})
    for (uint32_t n_groups : {0u, 1u, 256u, 257u})
      for (int format : {0, (int)WBX_OUT_I16, (int)WBX_OUT_I24})
        for (uint32_t bits = 0; bits < (1u << kIssueBits); bits++) {
          const RenderIssue is = issue_of(K, n_groups, bits & 2u, 1u + (bits & 1u), 512u, 2u, format, 256u, bits);
          issues += is.stage_bytes != 0u || is.sum_beside || !is.spread;
          if (is.stage_bytes != 0u && (K < 2047u || format == (int)WBX_OUT_I24 || (K == 2047u && format == (int)WBX_OUT_I16))) ok = false;
        }
  // choose_plan over every value of its fact word: segments never in a callback and always shorter than the render, the
  // counters zeroed by somebody exactly when they are not zero yet
  uint64_t plans = 0;
  for (uint32_t K : {1u, 7u, 8u, 127u, 128u, 2048u, 1u << 20})
    for (uint32_t N : {0u, 1u, 256u, 4096u, 1u << 20})
      for (int plan_seg : {-1, 0, 16, 128, 0x7FFFFFFF})
        for (uint32_t masked_rows : {0u, 4u})
          for (uint32_t bits = 0; bits < (1u << kPlanBits); bits++) {
            const RenderPlan p = plan_of(K, N, plan_seg, masked_rows, bits);
            plans += p.seg_len != 0u;
            if (p.seg_len >= K || (p.seg_len != 0u && (bits & 2u)) || (uint64_t)p.n_segs * (p.seg_len ? p.seg_len : K) < K) ok = false;
            if ((p.zeroing == RenderPlan::NOBODY) != ((bits >> 7 & 1u) != 0u) || plan_flags(p) >> 10) ok = false;
          }
  ok = ok && plans != 0u;
  for (size_t i = 0; i < std::size(kShape); i++) {   // each switch flips its own field and no other
    setenv(kShape[i][0], kShape[i][1], 1);
    const HsimKnobs h = flat();
    for (size_t j = 0; j < 14; j++) {
      const bool same = reinterpret_cast<const int32_t*>(&h)[j] == reinterpret_cast<const int32_t*>(&d)[j];
      if (same != (i != j)) ok = false, std::printf("%s: field %zu\n", kShape[i][0], j);
    }
    sweep();
    unsetenv(kShape[i][0]);
  }
  const CtxKnobs c0 = CtxKnobs::from_env();
  const EngineKnobs e0 = EngineKnobs::from_env();
  ok = ok && c0.overlap && c0.sum_overlap && !c0.mix_alternate && c0.profiling && c0.cb_spin_bound == 40000u && !c0.no_uniform &&
       !c0.cb_fenced && !c0.fast_partial_off && !c0.xcd_probe_fail && !c0.dbg_clock && !c0.cb_dbg && !c0.cu_mask;
  ok = ok && e0.plan_seg == -1 && e0.plan_lanes == 0u && dist_init_timeout_s() == 60.0;
  for (auto& kv : kOther) setenv(kv[0], kv[1], 1);
  const CtxKnobs c1 = CtxKnobs::from_env();
  const EngineKnobs e1 = EngineKnobs::from_env();
  ok = ok && !c1.overlap && !c1.sum_overlap && c1.mix_alternate && !c1.profiling && c1.cb_spin_bound == 0u && c1.no_uniform &&
       c1.cb_fenced && c1.fast_partial_off && c1.xcd_probe_fail && c1.dbg_clock && c1.cb_dbg && c1.cu_mask;
  ok = ok && e1.plan_seg == 0 && e1.plan_lanes == 16u && dist_init_timeout_s() == 2.5;   // (WBX_PLAN_SEG: max(0, atoi))
  setenv("WBX_PLAN_LANES", "3", 1);
  ok = ok && EngineKnobs::from_env().plan_lanes == 0u;   // (not a power of two up to 64: ignored)
  ok = ok && issues != 0u;
  std::printf(ok ? "host_knobs ok %llu %llu\n" : "host_knobs FAILED %llu %llu\n", (unsigned long long)shapes, (unsigned long long)issues);
  return ok ? 0 : 1;
}
#endif
