// wbx_runtime.hip — layer 1 of libwbx.so (wbx_ctx): clip pool in HBM, routing, plan upload, launches, result fetch.
// Layer 2 (the engine surface) lives in wbx_engine.hip, the multi-GPU exchange in wbx_dist.hip.
//
// There is no CPU implementation of the mix in this library: without a gfx950 device the create calls
// fail with WBX_ERR_NO_DEVICE.
#include "wbx_ctx.h"
#include "wbx_seq.h"

using namespace wbx;

namespace wbx {

// make the main stream wait for the sum that is still running beside it (device-side; a following
// sync_main(c) then covers it)
hipError_t join_sum(wbx_ctx* c) {
  if (c->sum_pending < 0) return hipSuccess;
  const hipError_t e = hipStreamWaitEvent(c->stream, c->sum_done[c->sum_pending], 0);
  c->sum_pending = -1;
  return e;
}

// the same for a mix that runs on the alternate stream
hipError_t join_alt(wbx_ctx* c) {
  if (c->alt_pending < 0) return hipSuccess;
  const hipError_t e = hipStreamWaitEvent(c->stream, c->mix_done[c->alt_pending], 0);
  c->alt_pending = -1;
  return e;
}

hipError_t sync_main(wbx_ctx* c) {
  hipError_t e = join_sum(c);
  if (e == hipSuccess) e = join_alt(c);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  return e;
}

// which stream the next mix runs on: batch renders of layer 2 alternate (see wbx_ctx::alt_stream)
hipStream_t pick_mix_stream(const wbx_ctx* c, uint32_t K, bool alternate) {
  const bool alt = alternate && c->ck.mix_alternate && c->alt_stream && K >= kOverlapMinBlocks && c->cur_mix_stream == c->stream;
  return alt ? c->alt_stream : c->stream;
}

// the kernel timer's pending launches -> the totals; `upto` > 0: only the oldest `upto` of them (a full ring: the newer half
// stays pending, so the submitting thread never waits for the launch it has just issued — waiting for THAT drained the whole
// run-ahead every 64 renders: ~9 us per step of a 0.4 ms render)
void drain_events(wbx_ctx* c, int upto) {
  const int n = (upto > 0 && upto < c->ev_pending) ? upto : c->ev_pending;
  for (int i = 0; i < n; i++) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev[i][0], c->ev[i][1]) == hipSuccess) {
      c->mix_ms_total += ms;
      c->mix_launches++;
      if (hipEventElapsedTime(&ms, c->ev[i][1], c->ev[i][2]) == hipSuccess) c->tail_ms_total += ms;
      // the idle time between two consecutive mixes (end of one to start of the next, the kernels' own time stamps): what a
      // step spends outside its dominant kernel while the device runs back to back
      if (i > 0 && hipEventElapsedTime(&ms, c->ev[i - 1][1], c->ev[i][0]) == hipSuccess && ms >= 0.0f && ms < 50.0f) {
        c->gap_ms_total += ms;
        c->gap_count++;
      }
    }
  }
  for (int i = n; i < c->ev_pending; i++)   // (the handles change places: every slot keeps three valid events)
    for (int k = 0; k < 3; k++) std::swap(c->ev[i - n][k], c->ev[i][k]);
  c->ev_pending -= n;
}

// Routing tables.  `order`: the direct tracks in index order, then the members of bus 0, bus 1, ... — the order the sums
// run in.  Two group sets over it: `groups` cuts every member list into workgroup-sized pieces of group_size tracks
// (the master is the in-order sum of the piece sums), `groups_exact` keeps every member list whole — one workgroup walks
// all direct tracks of its block in track order, which IS the reference's summation (engine.cpp:1600-1617,
// audio_buffer.h:73-82: bit-exact master).  Which set a render takes: RenderShape::walks_lists (wbx_shape.h).
void build_routing(wbx_ctx* c, uint32_t n_tracks) {
  uint32_t G = c->cfg.group_size;
  // the callback configuration: the one block's latency is a chain of dependent work per workgroup (≈0.4 us a track row), so
  // the library cuts a session into MANY small groups and lets the spread sum of callback_kernel add them (tools/cb_groups.py,
  // profiles/r04_callback_groups.txt — us per 512-frame block, one group / the choice below: 24 tracks 27.6 / 25.9, 64 tracks
  // 42.9 / 25.6, 256 tracks 48.2 (64-track groups) / 26.1, 1024 tracks 47.0 / 30.5).  Up to 16 tracks: one group, whose
  // workgroup stores the master itself.  Up to 64 tracks: one track per group — the master is then the in-order sum of the
  // track buffers, which IS the reference's summation (engine.cpp:1600-1617), bit for bit as with one group.  Above that
  // groups of 4 / 8 / 16 (at most ≈64 workgroups below 1024 tracks: past that the ticket barrier's cost grows faster than
  // the rows per workgroup shrink; 4096 tracks: 256 workgroups, one per CU).
  if (c->auto_group && c->cfg.max_blocks == 1)
    G = n_tracks <= 16u ? kStage / 2 : n_tracks <= 64u ? 1u : n_tracks <= 256u ? 4u : n_tracks <= 512u ? 8u : kStage / 8;
  c->order.clear();
  c->groups.clear();
  c->groups_exact.clear();
  auto emit = [&](const std::vector<uint32_t>& members, int32_t bus) {
    const uint32_t base = (uint32_t)c->order.size();
    for (uint32_t t : members) c->order.push_back(t);
    for (size_t i = 0; i < members.size(); i += G) {
      DGroup g{};
      g.first = base + (uint32_t)i;
      g.count = (uint32_t)std::min<size_t>(G, members.size() - i);
      g.bus = bus;
      g.flags = (i ? GROUP_CHAIN_IN : 0u) | (i + G < members.size() ? GROUP_CHAIN_OUT : 0u);   // its place in the list (chained renders)
      c->groups.push_back(g);
    }
    if (!members.empty()) {
      DGroup g{};
      g.first = base;
      g.count = (uint32_t)members.size();
      g.bus = bus;
      c->groups_exact.push_back(g);
    }
  };
  std::vector<uint32_t> direct;
  std::vector<std::vector<uint32_t>> per_bus(c->n_buses);
  for (uint32_t t = 0; t < n_tracks; t++) {
    int32_t bus = (c->n_buses && t < c->track_bus.size()) ? c->track_bus[t] : -1;
    if (bus >= 0 && (uint32_t)bus < c->n_buses)
      per_bus[bus].push_back(t);
    else
      direct.push_back(t);
  }
  emit(direct, -1);
  for (uint32_t u = 0; u < c->n_buses; u++) emit(per_bus[u], (int32_t)u);
  c->routing_tracks = n_tracks;
  c->routing_dirty = true;
  // every bus exactly one group and nothing routed straight to the master: group g's partial sum IS bus g's sum, so
  // the bus output can alias the partial buffer instead of being written a second time by the sum kernel
  auto aliases = [&](const std::vector<DGroup>& gs) {
    if (c->n_buses == 0 || gs.size() != c->n_buses) return false;
    for (size_t g = 0; g < gs.size(); g++)
      if (gs[g].bus != (int32_t)g) return false;
    return true;
  };
  c->buses_alias_partials = aliases(c->groups);
  c->buses_alias_exact = aliases(c->groups_exact);
  c->longest_list = 0;
  for (auto& g : c->groups_exact) c->longest_list = std::max(c->longest_list, g.count);
}

// the shape of a render of K blocks of N tracks (wbx_shape.h): the session's facts as the caller left them in the context, the
// clip table's and the routing's as they stand
RenderShape render_shape(const wbx_ctx* c, uint32_t K, uint32_t N, bool callback) {
  ShapeFacts f;
  f.channels = c->cfg.channels;
  f.block_frames = c->cfg.block_frames;
  f.group_size = c->cfg.group_size;
  f.auto_group = c->auto_group;
  f.session = c->session;
  f.integer_clips = c->has_integer_clips;
  f.non16_clips = c->has_non16_clips;
  f.n_buses = c->n_buses;
  f.longest_list = c->longest_list;
  f.n_blocks = K;
  f.n_tracks = N;
  f.callback = callback;
  f.chain_broken = c->chain_broken;
  f.mix_alternate = c->ck.mix_alternate;
  f.dist = c->dist != nullptr;
  return choose_shape(c->knobs, f);
}

wbx_status upload_tables(wbx_ctx* c, uint32_t n_tracks) {
  if (c->routing_tracks != n_tracks) {
    build_routing(c, n_tracks);
    c->buses_clean = false;
  }
  if (c->routing_dirty) {
    WBX_HIP(c, join_sum(c));                          // a sum beside the main stream may still read d_groups
    WBX_HIP(c, sync_main(c));
    WBX_HIP(c, c->d_order.ensure(std::max<size_t>(1, c->order.size())));
    WBX_HIP(c, c->d_groups.ensure(std::max<size_t>(1, c->groups.size() + c->groups_exact.size())));   // [groups | groups_exact]
    if (!c->order.empty())
      WBX_HIP(c, hipMemcpyAsync(c->d_order.p, c->order.data(), c->order.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                c->stream));
    if (!c->groups.empty())
      WBX_HIP(c, hipMemcpyAsync(c->d_groups.p, c->groups.data(), c->groups.size() * sizeof(DGroup),
                                hipMemcpyHostToDevice, c->stream));
    if (!c->groups_exact.empty())
      WBX_HIP(c, hipMemcpyAsync(c->d_groups.p + c->groups.size(), c->groups_exact.data(),
                                c->groups_exact.size() * sizeof(DGroup), hipMemcpyHostToDevice, c->stream));
    WBX_HIP(c, sync_main(c));   // host vectors may change right after
    c->routing_dirty = false;
  }
  if (c->samples_dirty) {
    std::vector<DSample> tab(c->clips.size());
    c->has_integer_clips = false;
    c->has_non16_clips = false;
    for (size_t i = 0; i < c->clips.size(); i++) {
      tab[i] = c->clips[i].d;
      if (c->clips[i].used && c->clips[i].d.format != FMT_F32) c->has_integer_clips = true;
      if (c->clips[i].used && c->clips[i].d.format != FMT_I16) c->has_non16_clips = true;
    }
    WBX_HIP(c, c->d_samples.ensure(std::max<size_t>(1, tab.size())));
    if (!tab.empty()) WBX_HIP(c, hipMemcpy(c->d_samples.p, tab.data(), tab.size() * sizeof(DSample), hipMemcpyHostToDevice));
    c->samples_dirty = false;
  }
  return WBX_OK;
}

wbx_status ensure_result_buffers(wbx_ctx* c, uint32_t K, uint32_t N) {
  const size_t CF = (size_t)c->cfg.channels * c->cfg.block_frames;
  for (auto& B : c->pb)
    if (B.prows.cap < (size_t)K * N) {
      WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
      WBX_HIP(c, sync_main(c));
      WBX_HIP(c, B.prows.ensure((size_t)K * N));
    }
  const size_t need_partial = (size_t)K * std::max<size_t>(1, c->groups.size()) * CF;
  if (c->d_partial2[0].cap < need_partial || c->d_master.cap < (size_t)K * CF ||
      c->d_peaks[0].cap < (size_t)K * N * c->cfg.channels || (c->n_buses && c->d_buses.cap < (size_t)K * c->n_buses * CF)) {
    WBX_HIP(c, join_sum(c));                          // a sum may still be using the buffers about to be replaced
    WBX_HIP(c, sync_main(c));
    for (auto& v : c->sum_valid) v = false;
  }
  for (auto& P : c->d_partial2) WBX_HIP(c, P.ensure(need_partial));
  WBX_HIP(c, c->d_master.ensure((size_t)K * CF));
  for (auto& P : c->d_peaks) WBX_HIP(c, P.ensure((size_t)K * N * c->cfg.channels));
  if (c->n_buses && c->d_buses.cap < (size_t)K * c->n_buses * CF) {
    WBX_HIP(c, sync_main(c));
    WBX_HIP(c, c->d_buses.ensure((size_t)K * c->n_buses * CF));
    c->buses_clean = false;
  }
  return WBX_OK;
}

// room for `n` templates in both plan buffers (grow-only)
wbx_status ensure_template_capacity(wbx_ctx* c, size_t n) {
  n = std::max<size_t>(n, 64);
  for (auto& B : c->pb) {
    if (n <= B.tmpl_cap) continue;
    WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
    WBX_HIP(c, sync_main(c));
    WBX_HIP(c, B.tmpl.ensure(n));
    B.tmpl_cap = (uint32_t)n;
  }
  return WBX_OK;
}

// room for `rows` pre-rendered generic track-blocks (grow-only)
wbx_status ensure_gen_capacity(wbx_ctx* c, size_t rows) {
  rows = std::max<size_t>(rows, 64);
  const size_t row_floats = (size_t)c->cfg.channels * (c->cfg.block_frames + 8);
  for (auto& B : c->pb) {
    if (rows <= B.gen_cap) continue;
    WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
    WBX_HIP(c, sync_main(c));
    WBX_HIP(c, B.gen_list.ensure(rows));
    WBX_HIP(c, B.rows.ensure(rows * row_floats));
    WBX_HIP(c, B.saved.ensure(rows));
    B.gen_cap = (uint32_t)rows;
  }
  return WBX_OK;
}

// The overflow pool (stream calls 3.. of a block) at twice its default size, once: a render planned by segments leaves the
// chunks of replaced segments allocated (grow-only; a host that set wbx_config.max_segments keeps exactly that budget).
wbx_status ensure_pool_slack(wbx_ctx* c) {
  if (c->cfg.max_segments) return WBX_OK;
  const size_t chunks = 2 * std::max<size_t>(1024, (size_t)c->cfg.max_blocks * c->cfg.max_tracks / 8);
  for (auto& B : c->pb) {
    if (chunks <= B.pool_chunks) continue;
    WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
    WBX_HIP(c, sync_main(c));
    WBX_HIP(c, B.pool.ensure(chunks * kChunk));
    B.pool_chunks = (uint32_t)chunks;
  }
  return WBX_OK;
}

// pre-render of the queued generic records of the current plan buffer
wbx_status launch_pre_render(wbx_ctx* c, hipStream_t on) {
  const uint32_t C = c->cfg.channels, F = c->cfg.block_frames;
  GenArgs ga{};
  ga.tmpl = PB(c).tmpl.p;
  ga.pool = PB(c).pool.p;
  ga.gen_list = PB(c).gen_list.p;
  ga.gen_count = PB(c).counters.p + 2;
  ga.rows = PB(c).rows.p;
  ga.saved = PB(c).saved.p;
  ga.gen_cap = PB(c).gen_cap;
  ga.block_frames = F;
  ga.channels = C;
  launch_gen(ga, c->shape.gen_grid, on);
  WBX_HIP(c, hipGetLastError());
  return WBX_OK;
}

// where the master of the render about to be issued goes; `writer` is the stream its last writer runs on
float* begin_master(wbx_ctx* c, float* target, hipStream_t writer, hipError_t* err) {
  *err = hipSuccess;
  if (c->dist) return dist_begin_render(c, writer, err);
  return target ? target : c->d_master.p;
}

namespace {

// the group set of a render: workgroup-sized pieces, or the whole member lists (the reference's summation order)
struct GroupSet {
  const DGroup* d_groups;
  uint32_t n_groups;
  bool buses_alias;
};
GroupSet render_groups(const wbx_ctx* c) {
  const bool whole = c->shape.walks_lists && !c->shape.chained;
  return {c->d_groups.p + (whole ? c->groups.size() : 0), (uint32_t)(whole ? c->groups_exact.size() : c->groups.size()),
          whole ? c->buses_alias_exact : c->buses_alias_partials};
}

// the facts choose_issue decides from (wbx_shape.h): the render's shape, the call, the context's state
IssueFacts issue_facts(const wbx_ctx* c, uint32_t K, uint32_t n_groups, const RenderCall& call, hipStream_t ms) {
  const RenderShape& sh = c->shape;
  IssueFacts f;
  f.K = K;
  f.n_groups = n_groups;
  f.n_buses = c->n_buses;
  f.tiles = sh.tiles;
  f.block_frames = c->cfg.block_frames;
  f.channels = c->cfg.channels;
  f.chained = sh.chained;
  f.cb_one_launch = sh.cb_one_launch;
  f.callback_plan = call.plan != nullptr;
  f.master_format = call.master ? call.format : c->master_format;
  f.mix_on_main = ms == c->stream;
  f.dist = c->dist != nullptr;
  f.init = c->master_init != nullptr || dist_receives_running_sum(c);   // (what dist_mix_init will hand the mix: non-null)
  f.target_set = call.master != nullptr || c->master_target != nullptr;
  f.target_on_host = c->master_target_on_host;   // (the setter's finding; wbx_engine_process's one block is never staged)
  f.cb_no_spread = c->cb_no_spread;
  f.n_cus = c->n_cus;
  return f;
}

// step 1: the mix's arguments (what goes with the choice of streams and launches is filled in by the caller)
MixArgs mix_args(wbx_ctx* c, uint32_t K, uint32_t N, const GroupSet& g, const RenderIssue& is, const RenderCall& call, int pp,
                 float* peaks, const float* init, float* master_dst) {
  const RenderShape& sh = c->shape;
  MixArgs m{};
  m.rows = PB(c).prows.p;
  m.tmpl = PB(c).tmpl.p;
  m.zero_page = c->d_zero.p;
  m.pool = PB(c).pool.p;
  m.order = c->d_order.p;
  m.groups = g.d_groups;
  m.partial = c->d_partial2[pp].p;
  m.peaks = peaks;
  m.levels = c->levels_target;
  m.init = init;
  m.n_tracks = N;
  m.n_groups = g.n_groups;
  m.block_frames = c->cfg.block_frames;
  m.channels = c->cfg.channels;
  m.lane_span = sh.lane_span;
  m.fast_partial = c->ck.fast_partial_off ? 0u : 1u;
  m.tiles = sh.tiles;
  m.n_blocks = K;
  m.masked_rows = sh.masked_rows ? 1u : 0u;
  // one resampling ratio for every window row of this render (layer 2's word; MODE_WNU / WINU: the products fl(j * speed)
  // hoisted out of the track loop).  WBX_NO_UNIFORM=1 withholds it.  [Round 3's split of this function lost this line: the
  // modes were carried but never taken until round 5 — SQ_INSTS_VALU_MUL_F64 of the r03-r05 PMC passes shows it.]
  m.uniform_speed = c->ck.no_uniform ? 0.0 : sh.uniform_speed;
  if (is.fused) {   // (the mix workgroup clamps and stores the master itself, and drops the plan status like the sum would)
    m.fused_master = master_dst;
    m.fused_clamp = c->clamp ? 1u : 0u;
    m.fused_status_src = call.status ? PB(c).counters.p : nullptr;
    m.fused_status_dst = call.status;
    m.fused_zero_status = (call.status && call.clear_counters) ? 1u : 0u;
  }
  return m;
}

// step 2: the sum's arguments
SumArgs sum_args(wbx_ctx* c, const GroupSet& g, const RenderCall& call, int pp, float* master_dst, int format) {
  SumArgs s{};
  s.partial = c->d_partial2[pp].p;
  s.groups = g.d_groups;
  s.master = master_dst;
  if (format) {   // the device format is the sum's epilogue: interleaved samples instead of planar fp32
    s.out_il = master_dst;
    s.out_format = (uint32_t)format;
  }
  s.buses = (c->n_buses && !g.buses_alias) ? c->d_buses.p : nullptr;
  s.n_groups = g.n_groups;
  s.n_buses = c->n_buses;
  s.block_frames = c->cfg.block_frames;
  s.channels = c->cfg.channels;
  s.clamp = c->clamp ? 1u : 0u;
  s.chain = c->shape.chained ? 1u : 0u;
  s.status_src = call.status ? PB(c).counters.p : nullptr;
  s.status_dst = call.status;
  s.zero_status = (call.status && call.clear_counters) ? 1u : 0u;
  return s;
}

}  // namespace

// mix + sum over the current plan buffer: what is launched, on which streams and with which waits between them is decided
// once (choose_issue, wbx_shape.h); then the mix's arguments, the sum's arguments, and the issue
wbx_status launch_mix_sum(wbx_ctx* c, uint32_t K, uint32_t N, const RenderCall& call, bool* one_launch) {
  if (one_launch) *one_launch = false;
  const uint32_t C = c->cfg.channels;
  const RenderShape& sh = c->shape;
  const GroupSet g = render_groups(c);
  hipStream_t ms = call.mix_stream ? call.mix_stream : c->stream;   // the main stream, or the alternate one (pick_mix_stream)
  c->cur_mix_stream = ms;
  float* const target = call.master ? call.master : c->master_target;
  const int format = call.master ? call.format : c->master_format;
  const RenderIssue is = choose_issue(c->ck, issue_facts(c, K, g.n_groups, call, ms));
  hipStream_t ss = is.sum_beside ? c->sum_stream : c->stream;
  const int pp = (int)(c->render_seq % kRing);
  const int pk = ms == c->stream ? 0 : 1;         // the mix stream's peaks buffer
  // this partial buffer was last read by the sum of kRing renders ago; the engine path has already made the PLAN
  // stream wait for that sum (the mix waits for the plan), which keeps the barrier off the main stream
  if (c->sum_valid[pp] && !call.plan_waits_partial) WBX_HIP(c, hipStreamWaitEvent(ms, c->partial_free[pp], 0));
  c->last_peaks = c->d_peaks[pk].p;
  // (argument checks first: once dist_mix_init has posted this render's receive, a failure would leave it unmatched)
  if (format && c->dist) return fail(c, WBX_ERR_UNSUPPORTED, "wbx_set_master_format: a multi-GPU partial master stays planar fp32");
  if (c->n_buses && (c->master_init || dist_receives_running_sum(c)))
    return fail(c, WBX_ERR_UNSUPPORTED, "a running master (wbx_set_master_init / WBX_DIST_CHAIN) cannot be continued through sub-buses");
  // where this render's master goes (the ctx's own buffer, the caller's target, or the multi-GPU ring slot) and what its
  // sum starts from (zero; wbx_set_master_init's running sum; chain mode: the previous rank's, received for this render)
  hipError_t me = hipSuccess;
  float* const master_home = begin_master(c, target, ss, &me);
  WBX_HIP(c, me);
  wbx_status ist = WBX_OK;
  const float* init = c->dist ? dist_mix_init(c, K, ms, &ist) : c->master_init;
  if (ist != WBX_OK) return ist;
  // A short render's sum runs on the main stream (and a one-group session's mix stores the master itself): neither may
  // overtake the sum of a batch render that is still pending on the sum stream — they write the same master (and bus)
  // buffers, and the late one would overwrite the head of the short render's blocks.  (Found by the edit scripts once they
  // stopped fetching every render: nobody had made the main stream wait, because a fetch in between always had.)
  if (ss == c->stream) WBX_HIP(c, join_sum(c));
  MixArgs m = mix_args(c, K, N, g, is, call, pp, c->d_peaks[pk].p, init, master_home);
  c->last_uniform_speed = m.uniform_speed;
  if (sh.chained) {   // one "sum is out" word per (workgroup column, group), tagged with this render's epoch: no clearing
    const size_t words = (size_t)K * m.tiles * g.n_groups;   // between renders (a memset here waits out the previous sum)
    const size_t had = c->d_chain.cap;
    WBX_HIP(c, c->d_chain.ensure(words));
    c->chain_epoch = (c->chain_epoch + 1u) & 0x0FFFFFFFu;
    if (c->d_chain.cap != had || c->chain_epoch == 0u) {   // fresh storage, or the tag wrapped: start over from zeroed words
      WBX_HIP(c, hipMemsetAsync(c->d_chain.p, 0, c->d_chain.cap * sizeof(uint32_t), ms));
      if (c->chain_epoch == 0u) c->chain_epoch = 1u;
    }
    m.chain_epoch = c->chain_epoch;
    m.chain = c->d_chain.p;
    m.chain_status = PB(c).counters.p + 1;
    m.chain_sticky = c->d_sticky_status.p;
  }
  if (c->ck.dbg_clock) {   // diagnostic: per-workgroup start / end times of the mix
    c->dbg_wgs = (size_t)K * g.n_groups * m.tiles;
    WBX_HIP(c, c->d_dbg.ensure(4 * c->dbg_wgs));
    m.dbg_clock = c->d_dbg.p;
  }
  if (m.tiles > 1) WBX_HIP(c, hipMemsetAsync(m.peaks, 0, (size_t)K * N * C * sizeof(float), ms));
  if (is.one_launch) {   // (the callback instance's own lane space: one 256-lane workgroup per block)
    m.lane_span = sh.cb_lane_span;
    m.tiles = 1u;
  }
  if (g.n_groups && !is.one_launch) {
    if (is.timed && c->ev_pending == kEventRing) {   // the older half: 32 launches behind the newest, over long ago
      WBX_HIP(c, hipEventSynchronize(c->ev[kEventRing / 2 - 1][2]));
      drain_events(c, kEventRing / 2);
    }
    // the timer's two events ride on the kernel's own dispatch packet (start / end time stamps of the kernel itself): no
    // event packets between two mixes
    const char* name = launch_mix(sh.mix, m, sh.grid_z, ms, is.timed ? c->ev[c->ev_pending][0] : nullptr,
                                  is.timed ? c->ev[c->ev_pending][1] : nullptr);
    if (!name) return fail(c, WBX_ERR_FAILED, "the render's mix instance is not compiled in");
    c->mix_kernel_name = name;
    if (c->dist) WBX_HIP(c, dist_mix_issued(c, ms));
  }
  // the plan buffer is free as soon as the MIX has read it: releasing it before the sum lets the next plan run
  // beside sum_kernel (the GPU is nearly idle there) instead of competing with the next mix for CU slots — started
  // together with a mix, the one-wave-per-track plan kernel is starved until that mix drains
  if (!is.one_launch && !is.by_kernel_event) WBX_HIP(c, hipEventRecord(c->mix_done[pp], ms));   // (one launch: no event at all, below)
  if (ms != c->stream) c->alt_pending = pp;
  // (a master bound for pinned host memory leaves a batch render through a staging buffer and the copy engine: choose_issue)
  float* master_dst = master_home;
  if (is.stage_bytes) {
    WBX_HIP(c, c->d_stage[pp].ensure((size_t)(is.stage_bytes + 3u) / 4u));
    master_dst = c->d_stage[pp].p;
  }
  const SumArgs s = sum_args(c, g, call, pp, master_dst, format);
  c->last_master_format = format;
  c->last_master = master_home;
  c->last_master_on_host = false;
  c->last_buses = c->n_buses ? (g.buses_alias ? c->d_partial2[pp].p : c->d_buses.p) : nullptr;
  if (is.by_kernel_event) {   // (the mix on the main stream, its sum beside it: ss is the sum stream)
    WBX_HIP(c, hipStreamWaitEvent(ss, c->ev[c->ev_pending][1], 0));   // the kernel's own completion ...
    WBX_HIP(c, hipEventRecord(c->mix_done[pp], ss));                   // ... and, over here, "the mix has read its plan buffer"
  } else if (ss != ms) {
    WBX_HIP(c, hipStreamWaitEvent(ss, c->mix_done[pp], 0));   // (an earlier pending sum is ordered before this one by ss)
  }
  if (c->n_buses && !g.buses_alias && !c->buses_clean) {
    // buses without member groups must read as zero; every bus that has members is rewritten by each render, so the
    // buffer only needs clearing when the routing or the allocation changed (64 MB per render saved on config 4).
    // On the SUM's stream, in front of the sum: cleared on the mix stream behind the mix, it raced with a sum that runs
    // beside (renders of 8 blocks and more) and could wipe the bus sums of the first render after a routing change —
    // found by the randomised sessions once they drew renders that long.
    WBX_HIP(c, hipMemsetAsync(c->d_buses.p, 0, c->d_buses.cap * sizeof(float), ss));
    c->buses_clean = true;
  }
  if (ss == c->stream && ms != c->stream) c->alt_pending = -1;            // (the main stream has just joined that mix)
  if (is.one_launch) {
    // sequencer + mix + sum in one dispatch; the kernel itself tells the host when master and status are out (call.done_word)
    if (!c->d_cb_done.p) {
      WBX_HIP(c, c->d_cb_done.ensure(kCbDoneWords));   // (two spread counters: wbx_callback.h)
      WBX_HIP(c, hipMemsetAsync(c->d_cb_done.p, 0, kCbDoneWords * sizeof(uint32_t), ms));
      c->cb_base = c->cb_base2 = 0;
    }
    unsigned long long* cb_dbg = nullptr;
    if (c->ck.cb_dbg) {   // diagnostic: the phases of every workgroup (tools/cb_clocks.py)
      c->dbg_wgs = ((size_t)6 * m.n_groups + 3) / 4;
      WBX_HIP(c, c->d_dbg.ensure(4 * c->dbg_wgs));
      cb_dbg = c->d_dbg.p;
    }
    m.partial_through = c->ck.cb_fenced ? 0u : 1u;
    const char* name = launch_callback(sh.cb, m, *call.plan, s, c->d_cb_done.p, c->cb_base, c->cb_base2, is.spread, call.gave_up_word,
                                       c->ck.cb_spin_bound, call.done_word, call.seq, cb_dbg, ms);
    if (!name) return fail(c, WBX_ERR_FAILED, "the render's callback instance is not compiled in");
    c->mix_kernel_name = name;
    // (a one-group block takes no ticket; a grid larger than the device — "the last workgroup adds everything" — only the
    //  first one: the second counter has a base of its own, or the first spread launch after such a block would wait for a
    //  count that wrapped)
    if (!is.fused) c->cb_base += m.n_groups;
    if (is.spread) c->cb_base2 += m.n_groups;
    c->cb_launches++;
    if (is.spread) c->cb_spread_launches++;
    if (one_launch) *one_launch = true;
    // (no event behind it: wbx_engine_process waits for the launch's own word before it returns, nothing can overlap it)
  } else if (!is.fused) {
    launch_sum(s, K, ss);
  }
  if (is.sum_beside) WBX_HIP(c, hipEventRecord(c->partial_free[pp], ss));   // (in front of the staged master's copy: wbx_ctx.h)
  if (is.stage_bytes) WBX_HIP(c, hipMemcpyAsync(master_home, master_dst, (size_t)is.stage_bytes, hipMemcpyDeviceToHost, ss));
  if (m.n_groups && is.timed) {
    WBX_HIP(c, hipEventRecord(c->ev[c->ev_pending][2], ss));
    c->ev_pending++;
  }
  if (is.sum_beside) {
    WBX_HIP(c, hipEventRecord(c->sum_done[pp], ss));
    c->sum_valid[pp] = true;
    c->sum_pending = pp;
  }
  c->render_seq++;
  WBX_HIP(c, hipGetLastError());
  c->last_K = K;
  c->last_N = N;
  return WBX_OK;
}

}  // namespace wbx

// =================================================================================================
// library
// =================================================================================================
extern "C" const char* wbx_version(void) { return "wbx 0.1 (gfx950)"; }

extern "C" int wbx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; i++) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
  }
  return ok;
}

extern "C" const char* wbx_status_string(wbx_status s) {
  switch (s) {
    case WBX_OK: return "ok";
    case WBX_ERR_FAILED: return "failed";
    case WBX_ERR_UNIMPLEMENTED: return "unimplemented";
    case WBX_ERR_UNSUPPORTED: return "unsupported";
    case WBX_ERR_INVALID: return "invalid argument";
    case WBX_ERR_NO_DEVICE: return "no gfx950 device";
    case WBX_ERR_DEVICE: return "HIP error";
    case WBX_ERR_OOM: return "out of memory";
    case WBX_ERR_OVERFLOW: return "segment plan overflow";
    default: return "unknown";
  }
}

// =================================================================================================
// layer 1
// =================================================================================================
extern "C" wbx_status wbx_create(const wbx_config* cfg, wbx_ctx** out) {
  if (!cfg || !out) return WBX_ERR_INVALID;
  *out = nullptr;
  if (cfg->channels < 1 || cfg->channels > 2 || cfg->block_frames < 4 || (cfg->block_frames & 3u) ||
      cfg->block_frames > 32768 || cfg->max_tracks == 0 || cfg->max_blocks == 0 || cfg->max_blocks > 4096 ||
      cfg->sample_rate == 0)
    return WBX_ERR_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || cfg->device < 0 || cfg->device >= n) return WBX_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return WBX_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return WBX_ERR_NO_DEVICE;   // kernels exist for gfx950 only
  if (hipSetDevice(cfg->device) != hipSuccess) return WBX_ERR_NO_DEVICE;

  wbx_ctx* c = new (std::nothrow) wbx_ctx();
  if (!c) return WBX_ERR_OOM;
  c->cfg = *cfg;
  // default 128: one staging round per workgroup; a context that can only render one block per call (the audio
  // callback) takes many small groups instead — one group up to 16 tracks, ONE TRACK per group up to 64 (both: the
  // reference's summation order, bit for bit), 4 / 8 / 16 tracks above 64 / 256 / 512 (build_routing) — more workgroups
  // for the one block, whose mix is a latency chain per workgroup; the block's group sums are added by the callback
  // kernel's spread sum (by sum_kernel when the block shape takes the three-launch path).
  c->auto_group = c->cfg.group_size == 0;
  if (c->cfg.group_size == 0) c->cfg.group_size = c->cfg.max_blocks == 1 ? kStage / 2 : kStage;
  c->knobs = ShapeKnobs::from_env();   // every environment switch is read here (wbx_knobs.h), none on a render path
  c->ck = CtxKnobs::from_env();
  c->n_cus = (uint32_t)std::max(prop.multiProcessorCount, 0);
  if (cfg->stream) {
    c->stream.adopt((hipStream_t)cfg->stream);
  } else if (c->stream.create(hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return WBX_ERR_DEVICE;
  }
  for (int i = 0; i < kEventRing; i++) {
    // (timing events: only their time stamps are read — no release to the system behind the kernel that carries them)
    if (c->ev[i][0].ensure(hipEventReleaseToDevice) != hipSuccess || c->ev[i][1].ensure(hipEventReleaseToDevice) != hipSuccess ||
        c->ev[i][2].ensure(hipEventReleaseToDevice) != hipSuccess) {
      wbx_destroy(c);
      return WBX_ERR_DEVICE;
    }
  }
  {
    // The sequencer runs beside the mix of the previous render.  It is a few dozen latency-bound waves (one
    // lane per track): at low or equal priority they starve behind the 16 mix waves of their CU and the
    // plan becomes the critical path, so the plan stream gets the HIGHEST priority — the issue slots it
    // takes from the bandwidth-bound mix are negligible.  (WBX_OVERLAP=0 runs everything on the main stream.)
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (c->plan_stream.create_with_priority(hipStreamNonBlocking, hi) != hipSuccess) {
      wbx_destroy(c);
      return WBX_ERR_DEVICE;
    }
    // the sum stream: highest priority as well — its few hundred small workgroups start while the next mix floods
    // the device.  (WBX_SUM_OVERLAP=0 keeps the sum on the main stream.)
    bool ok = c->sum_stream.create_with_priority(hipStreamNonBlocking, hi) == hipSuccess;
    for (int i = 0; i < kRing && ok; i++)
      ok = c->mix_done[i].ensure(kDevEventFlags) == hipSuccess && c->sum_done[i].ensure(hipEventDisableTiming) == hipSuccess &&
           c->partial_free[i].ensure(kDevEventFlags) == hipSuccess;
    if (ok) ok = c->upload_stream.create(hipStreamNonBlocking) == hipSuccess;
    // measured (tools/ab_alt.sh): with consecutive mixes on alternating streams the two kernels share the device for
    // their whole length (each takes 1.05-1.2 ms instead of 0.74) and the step time does not move — off by default
    if (ok) ok = c->alt_stream.create(hipStreamNonBlocking) == hipSuccess;
    // the workgroup-id -> XCD layout the chained pieces and the segmented sequencer rest on, probed before anything relies on it
    if (ok && (!probe_xcd_layout(c->stream, &c->n_xcds) || c->ck.xcd_probe_fail)) {
      c->n_xcds = 0;
      c->chain_broken = true;
      c->seg_broken = true;
    }
    if (!ok) {
      wbx_destroy(c);
      return WBX_ERR_DEVICE;
    }
  }
  size_t chunks = cfg->max_segments ? (cfg->max_segments + kChunk - 1) / kChunk
                                    : std::max<size_t>(1024, (size_t)cfg->max_blocks * cfg->max_tracks / 8);
  for (auto& B : c->pb) {
    B.pool_chunks = (uint32_t)chunks;
    if (B.pool.ensure(chunks * kChunk) != hipSuccess || B.counters.ensure(4) != hipSuccess ||
        B.planned.ensure(kDevEventFlags) != hipSuccess) {
      wbx_destroy(c);
      return WBX_ERR_OOM;
    }
    (void)hipMemset(B.counters.p, 0, 4 * sizeof(uint32_t));
  }
  if (c->d_zero.ensure(cfg->block_frames + 8) != hipSuccess || c->d_sticky_status.ensure(1) != hipSuccess) {
    wbx_destroy(c);
    return WBX_ERR_OOM;
  }
  (void)hipMemset(c->d_sticky_status.p, 0, sizeof(uint32_t));
  (void)hipMemset(c->d_zero.p, 0, (cfg->block_frames + 8) * sizeof(float));
  *out = c;
  return WBX_OK;
}

// What is not ownership: the device, the waits, and the clip pool (whose storage the pool policy owns).  Everything else is
// a holder of wbx_res.h and goes with the context; nothing runs any more when it does.
extern "C" void wbx_destroy(wbx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  dist_destroy(c);
  export_release(c);
  clipfx_release(c);
  if (c->plan_stream) (void)hipStreamSynchronize(c->plan_stream);
  if (c->sum_stream) (void)hipStreamSynchronize(c->sum_stream);
  if (c->alt_stream) (void)hipStreamSynchronize(c->alt_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& s : c->clips) {
    if (s.alloc) (void)hipFree(s.alloc);
    if (s.mip) (void)hipFree(s.mip);
  }
  for (auto& sl : c->slabs)
    if (sl->mem) (void)hipFree(sl->mem);
  delete c;
}

extern "C" const char* wbx_last_error(const wbx_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

namespace wbx {

void clip_release(wbx_ctx* c, ClipSlot& s) {
  if (s.alloc) {
    (void)hipFree(s.alloc);
    c->own_alloc_bytes.fetch_sub(s.stride * s.d.channels, std::memory_order_relaxed);
  }
  if (s.slab) {
    std::lock_guard<std::mutex> g(c->slab_mu);
    pool_give(*s.slab, s.slab_off, s.slab_len);   // (wbx_pool.h)
  }
  if (s.mip) (void)hipFree(s.mip);
  s = ClipSlot{};
}

// Clip audio -> a fresh slot `s` (not yet visible to any render): allocation, the 16 zero frames of tail padding
// (Sample::sample_padding, sample.cpp:127,140) and the fill, all enqueued on `on`.  Touches nothing of the ctx but
// its error string, so layer 2 can run it outside the editor lock on the upload stream.
wbx_status clip_build(wbx_ctx* c, ClipSlot& s, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames,
                      const ClipFill& f, hipStream_t on) {
  const size_t eb = fmt_bytes(format);
  if (!eb) return fail(c, WBX_ERR_UNSUPPORTED, "clip format");
  if (channels < 1 || channels > 2) return fail(c, WBX_ERR_UNSUPPORTED, "clip channel count (1 or 2)");
  if (frames >= 2147483632ull) return fail(c, WBX_ERR_UNSUPPORTED, "clip longer than 2^31-16 frames");
  if (f.kind == CLIP_SRC_PLANAR && !f.planar) return WBX_ERR_INVALID;
  if ((f.kind == CLIP_SRC_INTERLEAVED_HOST || f.kind == CLIP_SRC_INTERLEAVED_DEVICE) && !f.interleaved && frames) return WBX_ERR_INVALID;
  if (f.kind == CLIP_SRC_INTERLEAVED_DEVICE && ((uintptr_t)f.interleaved & 15u))
    return fail(c, WBX_ERR_INVALID, "interleaved device buffer must be 16-byte aligned");
  (void)hipSetDevice(c->cfg.device);
  s = ClipSlot{};
  const size_t stride = align_up((frames + kPad) * eb, 256);   // (varying the distance between a clip's channel rows: no effect)
  {
    const PoolExtent ext = pool_extent(stride * channels, c->slab_seq.fetch_add(1u, std::memory_order_relaxed), true);   // (the gap: wbx_pool.h)
    const size_t need = ext.body + ext.gap;
    PoolTake where;
    {   // where the clip goes is wbx_pool.h's decision; hipMalloc is the slabs' source
      std::lock_guard<std::mutex> g(c->slab_mu);
      where = pool_take(c->slabs, need, stride * channels, c->pool_limit.load(std::memory_order_relaxed),
                        c->own_alloc_bytes.load(std::memory_order_relaxed), true,
                        [](void*, size_t bytes) -> char* {
                          char* mem = nullptr;
                          if (hipMalloc((void**)&mem, bytes) == hipSuccess) return mem;
                          (void)hipGetLastError();   // a device too full for another slab: this clip gets an allocation of its own
                          return nullptr;
                        },
                        nullptr);
    }
    switch (where.where) {
      case POOL_IN_SLAB:
        s.slab = where.slab;
        s.slab_off = where.off;
        s.slab_len = need;
        s.base = where.slab->mem + where.off + ext.gap;
        break;
      case POOL_OWN: {
        WBX_HIP(c, hipMalloc(&s.alloc, stride * channels));
        s.base = s.alloc;
        c->own_alloc_bytes.fetch_add(stride * channels, std::memory_order_relaxed);
        break;
      }
      case POOL_LIMIT:
        return fail(c, WBX_ERR_OOM, "clip pool limit reached (wbx_clip_pool_limit)");
      default:
        return WBX_ERR_OOM;
    }
  }
  s.d.ch[0] = s.base;
  s.d.ch[1] = channels > 1 ? (const void*)((const char*)s.base + stride) : s.base;   // mono wraps (i % channels)
  s.d.count = frames;
  s.d.format = (uint32_t)format;
  s.d.channels = channels;
  s.d.sample_rate = sample_rate;
  s.used = true;
  s.stride = stride;
  hipError_t err = hipSuccess;
  DevBuf<uint8_t> stage[2];
  Event freed[2];
  auto pad_tails = [&]() {   // the padding frames (and the alignment slack) read as zero
    for (uint32_t ch = 0; ch < channels && err == hipSuccess; ch++)
      err = hipMemsetAsync((char*)s.base + stride * ch + frames * eb, 0, stride - frames * eb, on);
  };
  switch (f.kind) {
    case CLIP_SRC_PLANAR:
      pad_tails();
      for (uint32_t ch = 0; ch < channels && err == hipSuccess; ch++)
        err = hipMemcpyAsync((char*)s.base + stride * ch, f.planar[ch], frames * eb, hipMemcpyHostToDevice, on);
      if (err == hipSuccess) err = hipStreamSynchronize(on);   // the caller's arrays may go away
      break;
    case CLIP_SRC_SYNTH:
      for (uint32_t ch = 0; ch < channels; ch++) {
        const uint64_t key = f.seed ^ ((uint64_t)f.key_track << 40) ^ ((uint64_t)ch << 32);
        launch_synth((char*)s.base + stride * ch, frames, key, f.amp, format, on);   // writes the padding as well
      }
      err = hipGetLastError();
      break;
    case CLIP_SRC_ZERO:
      for (uint32_t ch = 0; ch < channels && err == hipSuccess; ch++) err = hipMemsetAsync((char*)s.base + stride * ch, 0, stride, on);
      break;
    case CLIP_SRC_NONE:
      pad_tails();
      break;
    case CLIP_SRC_INTERLEAVED_DEVICE:
      pad_tails();
      if (err == hipSuccess) {
        launch_deinterleave(f.interleaved, s.base, (char*)s.base + (channels > 1 ? stride : 0), frames, channels, (uint32_t)eb, on);
        err = hipGetLastError();
      }
      break;
    default: {   // CLIP_SRC_INTERLEAVED_HOST
      pad_tails();
      // chunks of the decoder's interleaved output go host -> device staging -> transposed into the channel rows;
      // two staging buffers so the copy of chunk i+1 overlaps the transposition of chunk i
      const uint64_t chunk_frames = (uint64_t)4 << 20;   // a multiple of 4 frames: lane groups never straddle chunks
      const size_t chunk_bytes = (size_t)chunk_frames * channels * eb;
      const int nstage = frames > chunk_frames ? 2 : 1;
      for (int i = 0; i < nstage && err == hipSuccess; i++) {
        err = stage[i].ensure(std::min<size_t>(chunk_bytes, std::max<size_t>(16, (size_t)frames * channels * eb)));
        if (err == hipSuccess) err = freed[i].ensure(hipEventDisableTiming);
      }
      uint64_t done = 0;
      for (int i = 0; done < frames && err == hipSuccess; i++) {
        const uint64_t n = std::min<uint64_t>(chunk_frames, frames - done);
        const int b = i % nstage;
        if (i >= nstage) err = hipEventSynchronize(freed[b]);
        if (err == hipSuccess)
          err = hipMemcpyAsync(stage[b].p, (const char*)f.interleaved + (size_t)done * channels * eb, (size_t)n * channels * eb,
                               hipMemcpyHostToDevice, on);
        if (err == hipSuccess) {
          launch_deinterleave(stage[b].p, (char*)s.base + (size_t)done * eb,
                              (char*)s.base + (channels > 1 ? stride : 0) + (size_t)done * eb, n, channels, (uint32_t)eb, on);
          err = hipEventRecord(freed[b], on);
        }
        done += n;
      }
      if (err == hipSuccess) err = hipStreamSynchronize(on);
      else (void)hipStreamSynchronize(on);   // nothing may still read the staging buffers, freed at the function's end
      break;
    }
  }
  if (err != hipSuccess) {
    (void)hipStreamSynchronize(on);
    clip_release(c, s);
    return fail(c, WBX_ERR_DEVICE, "clip upload", err);
  }
  return WBX_OK;
}

// make slot `clip` of the pool hold `s` (an earlier clip of that id is freed once the device is done with it)
wbx_status clip_publish(wbx_ctx* c, uint32_t clip, ClipSlot& s) {
  if (clip >= (1u << 24)) {
    clip_release(c, s);
    return fail(c, WBX_ERR_INVALID, "clip id");
  }
  if (clip >= c->clips.size()) c->clips.resize(clip + 1);
  ClipSlot& dst = c->clips[clip];
  if (dst.base) {
    (void)hipStreamSynchronize(c->plan_stream);
    (void)join_sum(c);
    (void)sync_main(c);
    clip_release(c, dst);
  }
  dst = std::move(s);
  s = ClipSlot{};
  c->samples_dirty = true;
  return WBX_OK;
}

}  // namespace wbx

static wbx_status clip_create(wbx_ctx* c, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate, uint64_t frames,
                              const ClipFill& f) {
  if (!c) return WBX_ERR_INVALID;
  if (clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  ClipSlot s;
  wbx_status st = clip_build(c, s, format, channels, sample_rate, frames, f, c->stream);
  if (st != WBX_OK) return st;
  return clip_publish(c, clip, s);
}

extern "C" wbx_status wbx_clip_upload(wbx_ctx* c, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                                      uint64_t frames, const void* const* planar) {
  if (!c || !planar) return WBX_ERR_INVALID;
  ClipFill f{};
  f.kind = CLIP_SRC_PLANAR;
  f.planar = planar;
  return clip_create(c, clip, format, channels, sample_rate, frames, f);
}

extern "C" wbx_status wbx_clip_synth(wbx_ctx* c, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                                     uint64_t frames, uint64_t seed, uint32_t key_track, float amp) {
  ClipFill f{};
  f.kind = CLIP_SRC_SYNTH;
  f.seed = seed;
  f.key_track = key_track;
  f.amp = amp;
  return clip_create(c, clip, format, channels, sample_rate, frames, f);
}

// ---- clip ingest (dsp/sample.cpp:29-43, :112-197) ------------------------------------------------
extern "C" wbx_status wbx_clip_ingest_device(wbx_ctx* c, uint32_t clip, int format, uint32_t channels, uint32_t sample_rate,
                                             uint64_t frames, const void* device_interleaved) {
  ClipFill f{};
  f.kind = CLIP_SRC_INTERLEAVED_DEVICE;
  f.interleaved = device_interleaved;
  return clip_create(c, clip, format, channels, sample_rate, frames, f);
}

extern "C" wbx_status wbx_clip_upload_interleaved(wbx_ctx* c, uint32_t clip, int format, uint32_t channels,
                                                  uint32_t sample_rate, uint64_t frames, const void* interleaved) {
  ClipFill f{};
  f.kind = CLIP_SRC_INTERLEAVED_HOST;
  f.interleaved = interleaved;
  return clip_create(c, clip, format, channels, sample_rate, frames, f);
}

extern "C" wbx_status wbx_clip_download(wbx_ctx* c, uint32_t clip, uint32_t channel, void* dst) {
  if (!c || !dst || clip >= c->clips.size() || !c->clips[clip].used) return WBX_ERR_INVALID;
  const ClipSlot& s = c->clips[clip];
  if (channel >= s.d.channels) return fail(c, WBX_ERR_INVALID, "channel out of range");
  WBX_HIP(c, sync_main(c));
  WBX_HIP(c, hipMemcpy(dst, (const char*)s.base + s.stride * channel, (size_t)s.d.count * fmt_bytes((int)s.d.format), hipMemcpyDeviceToHost));
  return WBX_OK;
}

// ---- waveform mip-maps (gfx/waveform_visual.cpp:9-246) -------------------------------------------
extern "C" uint32_t wbx_mip_levels(uint64_t frames) {
  uint32_t n = 0;
  for (uint64_t sample_count = frames; sample_count > 64; sample_count /= 4) n++;   // :195, :236
  return n;
}

extern "C" uint64_t wbx_mip_data_count(uint64_t frames, uint32_t level) {
  const uint64_t block_count = (uint64_t)1 << (2u * level);   // 2^(current_mip - 1), current_mip = 1 + 2*level
  uint64_t n = frames / block_count;                           // :198
  n += n % 2;                                                  // :199
  return n;
}

extern "C" wbx_status wbx_clip_build_mipmaps(wbx_ctx* c, uint32_t clip, int quality) {
  if (!c || clip >= c->clips.size() || !c->clips[clip].used) return WBX_ERR_INVALID;
  if (quality != 0 && quality != 1) return fail(c, WBX_ERR_INVALID, "quality: 0 (Low, int8) or 1 (High, int16)");
  ClipSlot& s = c->clips[clip];
  const int fmt = (int)s.d.format;
  if (fmt != FMT_I16 && fmt != FMT_I32 && fmt != FMT_F32) return fail(c, WBX_ERR_UNSUPPORTED, "mip-maps: clip format");
  (void)hipSetDevice(c->cfg.device);
  const uint32_t levels = wbx_mip_levels(s.d.count);
  if (levels > 24) return fail(c, WBX_ERR_UNSUPPORTED, "mip-maps: too many levels");
  const int bits = quality ? 16 : 8;
  const size_t esz = bits / 8;
  if (s.mip) {
    WBX_HIP(c, sync_main(c));
    (void)hipFree(s.mip);
    s.mip = nullptr;
  }
  s.mip_off.assign(levels, 0);
  s.mip_count.assign(levels, 0);
  s.mip_bits = bits;
  size_t total = 0;
  for (uint32_t l = 0; l < levels; l++) {
    s.mip_count[l] = wbx_mip_data_count(s.d.count, l);
    s.mip_off[l] = total;
    total += align_up((size_t)s.mip_count[l] * s.d.channels * esz, 256);
  }
  if (!levels) return WBX_OK;
  const uint32_t tiles = (uint32_t)((s.d.count + kMipTile - 1) / kMipTile);
  const size_t nodes_off = total;
  const size_t nodes_per_ch = (size_t)tiles + tiles / 4 + 1;   // tile nodes + ping-pong scratch of the upper levels
  total += nodes_per_ch * s.d.channels * sizeof(MipNode);
  WBX_HIP(c, hipMalloc(&s.mip, total));
  for (uint32_t ch = 0; ch < s.d.channels; ch++) {
    MipArgs a{};
    a.src = (const char*)s.base + s.stride * ch;
    a.count = s.d.count;
    a.n_levels = levels;
    a.n_tiles = tiles;
    a.tile_nodes = (MipNode*)((char*)s.mip + nodes_off) + nodes_per_ch * ch;
    for (uint32_t l = 0; l < levels; l++) {
      a.level_out[l] = (char*)s.mip + s.mip_off[l] + (size_t)s.mip_count[l] * ch * esz;
      a.data_count[l] = s.mip_count[l];
    }
    launch_mip(a, fmt, bits, c->stream);
  }
  WBX_HIP(c, hipGetLastError());
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_mipmap_device(wbx_ctx* c, uint32_t clip, uint32_t level, const void** data, uint64_t* count) {
  if (!c || clip >= c->clips.size() || !c->clips[clip].used) return WBX_ERR_INVALID;
  const ClipSlot& s = c->clips[clip];
  if (!s.mip_bits || level >= s.mip_off.size()) return fail(c, WBX_ERR_INVALID, "no such mip level (call wbx_clip_build_mipmaps)");
  if (data) *data = (const char*)s.mip + s.mip_off[level];
  if (count) *count = s.mip_count[level];
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_fetch_mipmap(wbx_ctx* c, uint32_t clip, uint32_t level, void* dst) {
  const void* p = nullptr;
  uint64_t n = 0;
  wbx_status st = wbx_clip_mipmap_device(c, clip, level, &p, &n);
  if (st != WBX_OK) return st;
  if (!dst) return WBX_ERR_INVALID;
  const ClipSlot& s = c->clips[clip];
  WBX_HIP(c, sync_main(c));
  WBX_HIP(c, hipMemcpy(dst, p, (size_t)n * s.d.channels * (s.mip_bits / 8), hipMemcpyDeviceToHost));
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_free(wbx_ctx* c, uint32_t clip) {
  if (!c || clip >= c->clips.size() || !c->clips[clip].base) return WBX_ERR_INVALID;
  // layer 2: a clip list that still names the sample would make the sequencer hand the mix a dangling pointer
  if (c->sample_in_use && c->sample_in_use(c->owner, clip))
    return fail(c, WBX_ERR_INVALID, "sample is still referenced by a clip (delete the clips first)");
  (void)hipSetDevice(c->cfg.device);
  WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
  WBX_HIP(c, join_sum(c));
  WBX_HIP(c, sync_main(c));
  clip_release(c, c->clips[clip]);
  c->samples_dirty = true;
  return WBX_OK;
}

// clip storage in numbers: slabs allocated, bytes reserved from the driver (slabs + clips with an allocation of their
// own), bytes held by live clips
extern "C" wbx_status wbx_clip_pool_stats(wbx_ctx* c, uint32_t* n_slabs, uint64_t* bytes_reserved, uint64_t* bytes_live) {
  if (!c) return WBX_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->slab_mu);
  uint32_t n = 0;
  uint64_t reserved = 0, live = 0;
  pool_slab_stats(c->slabs, &n, &reserved, &live);   // (wbx_pool.h)
  for (auto& s : c->clips)
    if (s.alloc) {
      reserved += s.stride * s.d.channels;
      live += s.stride * s.d.channels;
    }
  if (n_slabs) *n_slabs = n;
  if (bytes_reserved) *bytes_reserved = reserved;
  if (bytes_live) *bytes_live = live;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_pool_limit(wbx_ctx* c, uint64_t max_bytes_reserved) {
  if (!c) return WBX_ERR_INVALID;
  c->pool_limit.store(max_bytes_reserved, std::memory_order_relaxed);
  return WBX_OK;
}

extern "C" wbx_status wbx_set_routing(wbx_ctx* c, uint32_t n_tracks, const int32_t* track_bus, uint32_t n_buses) {
  if (!c || n_tracks > c->cfg.max_tracks) return WBX_ERR_INVALID;
  if (track_bus && n_buses) {
    c->track_bus.assign(track_bus, track_bus + n_tracks);
    c->n_buses = n_buses;
  } else {
    c->track_bus.clear();
    c->n_buses = 0;
  }
  build_routing(c, n_tracks);
  c->buses_clean = false;
  return WBX_OK;
}

// how a render of n_blocks blocks is summed, with the routing as it stands (the last render's, or wbx_set_routing's)
extern "C" wbx_status wbx_render_order(wbx_ctx* c, uint32_t n_blocks, uint32_t* n_groups, uint32_t* longest_group,
                                       int* reference_order) {
  if (!c || n_blocks == 0) return WBX_ERR_INVALID;
  const RenderShape sh = render_shape(c, n_blocks, c->last_N, false);
  const bool chained = sh.chained, whole = sh.walks_lists && !chained;
  const std::vector<DGroup>& gs = whole ? c->groups_exact : c->groups;
  uint32_t longest = 0;
  for (auto& g : gs) longest = std::max(longest, g.count);
  if (n_groups) *n_groups = (uint32_t)gs.size();
  if (longest_group) *longest_group = longest;
  // (chained: the pieces are workgroup-sized, the additions are one sequence per member list all the same)
  if (reference_order) *reference_order = (whole || chained || gs.size() == c->groups_exact.size()) ? 1 : 0;
  return WBX_OK;
}

extern "C" wbx_status wbx_device_info(wbx_ctx* c, char* pci_bus_id, size_t n_pci, char* name, size_t n_name) {
  if (!c) return WBX_ERR_INVALID;
  if (pci_bus_id && n_pci) {
    pci_bus_id[0] = 0;
    WBX_HIP(c, hipDeviceGetPCIBusId(pci_bus_id, (int)n_pci, c->cfg.device));
  }
  if (name && n_name) {
    hipDeviceProp_t p;
    WBX_HIP(c, hipGetDeviceProperties(&p, c->cfg.device));
    std::snprintf(name, n_name, "%s (%s)", p.name, p.gcnArchName);
  }
  return WBX_OK;
}

// diagnostic (not in wbx.h; WBX_DBG_CLOCK=1): start / end wall-clock ticks (100 MHz) of every workgroup of the last mix
extern "C" wbx_status wbx_debug_wg_clocks(wbx_ctx* c, unsigned long long* out, size_t cap, size_t* n_wgs) {
  if (!c || !n_wgs) return WBX_ERR_INVALID;
  *n_wgs = c->dbg_wgs;
  if (!out || !c->d_dbg.p) return WBX_OK;
  WBX_HIP(c, sync_main(c));
  WBX_HIP(c, hipMemcpy(out, c->d_dbg.p, std::min(cap, 4 * c->dbg_wgs) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return WBX_OK;
}

extern "C" wbx_status wbx_set_clamp(wbx_ctx* c, int on) {
  if (!c) return WBX_ERR_INVALID;
  c->clamp = on != 0;
  return WBX_OK;
}

size_t wbx::out_format_bytes(int fmt) {
  switch (fmt) {
    case WBX_OUT_I16: return 2;
    case WBX_OUT_I24: return 3;
    case WBX_OUT_I24_X8:
    case WBX_OUT_I32:
    case WBX_OUT_F32: return 4;
    default: return 0;
  }
}

extern "C" wbx_status wbx_set_master_format(wbx_ctx* c, int out_format) {
  if (!c) return WBX_ERR_INVALID;
  if (out_format != 0 && out_format_bytes(out_format) == 0) return fail(c, WBX_ERR_UNSUPPORTED, "interleaved output format");
  c->master_format = out_format;
  return WBX_OK;
}

// ---- export: a resident F32 clip -> interleaved device-format samples in host memory (wbx.h "Export") ------------------
// kernel: wbx_export.hip.  The range goes through kExportSlots staging chunks: chunk k's kernel writes the slot's device
// buffer, the copy engine moves it into the slot's pinned buffer (or straight into a pinned dst), and while the host copies
// chunk k out of its slot the kernels and transfers of chunks k+1 and k+2 are already enqueued.
extern "C" uint64_t wbx_export_bytes(int out_format, uint32_t channels, uint64_t n_frames) {
  return (uint64_t)out_format_bytes(out_format) * channels * n_frames;
}

extern "C" wbx_status wbx_set_export_chunk(wbx_ctx* c, uint32_t frames) {
  if (!c) return WBX_ERR_INVALID;
  if (frames && (frames < 8u || (frames & 7u) || frames > kExportChunkMax))
    return fail(c, WBX_ERR_INVALID, "export chunk: a multiple of 8 frames, 8 .. 2^24 (0: the default)");
  c->export_chunk.store(frames, std::memory_order_relaxed);
  return WBX_OK;
}

wbx_status wbx::export_check(const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, int out_format, uint32_t flags,
                             const void* dst, const char** why) {
  *why = "";
  if (!dst) return *why = "export: dst is NULL", WBX_ERR_INVALID;
  if (flags & ~(uint32_t)WBX_EXPORT_CLAMP) return *why = "export: unknown flags", WBX_ERR_INVALID;
  if (n_frames == 0) return *why = "export: no frames", WBX_ERR_INVALID;
  if (first_frame > src.frames || n_frames > src.frames - first_frame) return *why = "export: the range ends past the clip", WBX_ERR_INVALID;
  if (!out_format_bytes(out_format)) return *why = "export: unknown output format", WBX_ERR_UNSUPPORTED;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "export: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "export: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

static void export_free_slots(wbx_ctx* c) {
  ExportStage& x = c->exp;
  if (x.side.stream) (void)hipStreamSynchronize(x.side.stream);
  for (int i = 0; i < kExportSlots; i++) {
    x.d_slot[i].release();
    x.h_slot[i].buf.release();
    x.d_stats[i].release();
  }
  x.h_stats.release();
  x.chunk = 0;
}

void wbx::export_release(wbx_ctx* c) {
  side_release(c->exp.side);
  c->exp = ExportStage{};
}

// ---- side streams (wbx_ctx.h SideStream) ------------------------------------------------------------------------------
hipError_t wbx::side_prepare(wbx_ctx* c, SideStream& s) {
  if (s.stream) return hipSuccess;
  hipError_t e = s.stream.create(hipStreamNonBlocking);
  if (e == hipSuccess) e = s.after_main.ensure(kDevEventFlags);
  if (e == hipSuccess) e = s.after_upload.ensure(kDevEventFlags);
  if (e != hipSuccess) side_release(s);
  return e;
}

// the stream behind everything enqueued so far on the streams that write the pool's clips: the main stream (with the sum
// and the alternate mix joined to it, as sync_main does) and the upload stream.  Enqueues only: the host does not wait.
hipError_t wbx::side_order(wbx_ctx* c, SideStream& s) {
  hipError_t e = join_sum(c);
  if (e == hipSuccess) e = join_alt(c);
  if (e == hipSuccess) e = hipEventRecord(s.after_main, c->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, s.after_main, 0);
  if (e == hipSuccess && c->upload_stream) {
    e = hipEventRecord(s.after_upload, c->upload_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, s.after_upload, 0);
  }
  return e;
}

void wbx::side_release(SideStream& s) {
  if (s.stream) (void)hipStreamSynchronize(s.stream);
  s = SideStream{};
}

wbx_status wbx::export_prepare(wbx_ctx* c, std::string* why) {
  ExportStage& x = c->exp;
  (void)hipSetDevice(c->cfg.device);
  hipError_t e = side_prepare(c, x.side);
  for (int i = 0; i < kExportSlots && e == hipSuccess; i++)
    e = x.h_slot[i].done.ensure(hipEventDisableTiming);
  if (e != hipSuccess) {
    export_release(c);
    return stage_fail(why, WBX_ERR_DEVICE, "export: stream and events", e);
  }
  uint32_t want = c->export_chunk.load(std::memory_order_relaxed);
  if (!want) want = kExportChunkDefault;
  if (x.chunk != want) {
    export_free_slots(c);
    const size_t bytes = (size_t)want * 8u;   // two channels of 32 bits: the widest frame
    for (int i = 0; i < kExportSlots && e == hipSuccess; i++) {
      e = x.d_slot[i].ensure(bytes);
      if (e == hipSuccess) e = x.h_slot[i].buf.ensure(bytes);
      if (e == hipSuccess) e = x.d_stats[i].ensure(8);
    }
    if (e == hipSuccess) e = x.h_stats.ensure(kExportSlots * 8);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      export_free_slots(c);
      return stage_fail(why, WBX_ERR_OOM, "export: staging slots", e);
    }
    x.chunk = want;
  }
  return WBX_OK;
}

wbx_status wbx::export_order(wbx_ctx* c, std::string* why) {
  const hipError_t e = side_order(c, c->exp.side);
  return e == hipSuccess ? WBX_OK : stage_fail(why, WBX_ERR_DEVICE, "export: ordering after the pool's writers", e);
}

static bool export_dst_is_pinned(const void* dst, size_t bytes) {
  for (const char* p : {(const char*)dst, (const char*)dst + bytes - 1}) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    if (at.type != hipMemoryTypeHost) return false;
  }
  return true;
}

wbx_status wbx::export_run(wbx_ctx* c, const ClipSrc& src, uint64_t first_frame, uint64_t n_frames, int out_format,
                           uint32_t flags, void* dst, wbx_export_stats* stats, std::string* why) {
  ExportStage& x = c->exp;
  const hipStream_t on = x.side.stream;
  const uint32_t C = src.channels;
  const size_t fb = out_format_bytes(out_format) * C;          // bytes of a frame in dst
  const uint64_t chunk = x.chunk, n_chunks = (n_frames + chunk - 1) / chunk;
  const bool to_dst = export_dst_is_pinned(dst, (size_t)n_frames * fb);   // the copy engine writes dst itself
  wbx_export_stats acc{};
  auto issue = [&](uint64_t k) -> hipError_t {
    const int b = (int)(k % kExportSlots);
    const uint64_t at = k * chunk;
    const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n_frames - at);
    hipError_t e = hipMemsetAsync(x.d_stats[b].p, 0, 8 * sizeof(uint32_t), on);
    if (e != hipSuccess) return e;
    ExportArgs a{};
    for (uint32_t ch = 0; ch < C; ch++) a.src[ch] = clip_row(src, ch) + first_frame + at;
    if (C == 1) a.src[1] = a.src[0];
    a.dst = x.d_slot[b].p;
    a.stats = x.d_stats[b].p;
    a.n_frames = m;
    a.channels = C;
    a.format = (uint32_t)out_format;
    a.flags = flags;
    launch_export(a, on);
    e = hipGetLastError();
    if (e == hipSuccess)
      e = hipMemcpyAsync(to_dst ? (void*)((char*)dst + (size_t)at * fb) : x.h_slot[b].buf.p, x.d_slot[b].p, (size_t)m * fb,
                         hipMemcpyDeviceToHost, on);
    if (e == hipSuccess) e = hipMemcpyAsync(x.h_stats.p + 8 * b, x.d_stats[b].p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, on);
    if (e == hipSuccess) e = x.h_slot[b].mark(on);
    return e;
  };
  hipError_t e = hipSuccess;
  for (uint64_t k = 0; k < std::min<uint64_t>(kExportSlots - 1, n_chunks) && e == hipSuccess; k++) e = issue(k);
  for (uint64_t k = 0; k < n_chunks && e == hipSuccess; k++) {
    const int b = (int)(k % kExportSlots);
    e = x.h_slot[b].wait();
    if (e != hipSuccess) break;
    const uint32_t* hs = x.h_stats.p + 8 * b;
    for (uint32_t ch = 0; ch < C; ch++) {
      float pk;
      std::memcpy(&pk, hs + ch, sizeof(float));
      if (pk > acc.peak[ch]) acc.peak[ch] = pk;
      acc.over[ch] += hs[2 + ch];
      acc.nans[ch] += hs[4 + ch];
    }
    if (k + kExportSlots - 1 < n_chunks) e = issue(k + kExportSlots - 1);   // (its slot was emptied one iteration ago)
    if (!to_dst) {
      const uint64_t at = k * chunk;
      std::memcpy((char*)dst + (size_t)at * fb, x.h_slot[b].buf.p, (size_t)std::min<uint64_t>(chunk, n_frames - at) * fb);
    }
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(on);   // nothing may still write a slot or dst
    return stage_fail(why, WBX_ERR_DEVICE, "export", e);
  }
  if (stats) *stats = acc;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_export(wbx_ctx* c, uint32_t clip, uint64_t first_frame, uint64_t n_frames, int out_format,
                                      uint32_t flags, void* dst, wbx_export_stats* stats) {
  if (!c) return WBX_ERR_INVALID;
  const ClipSlot* s = find_clip(c, clip);
  if (!s) return fail(c, WBX_ERR_INVALID, "export: unknown clip");
  const ClipSrc src = clip_src(*s);
  const char* msg = "";
  wbx_status st = export_check(src, first_frame, n_frames, out_format, flags, dst, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  std::lock_guard<std::mutex> g(c->export_mu);
  std::string why;
  st = export_prepare(c, &why);
  if (st == WBX_OK) st = export_order(c, &why);
  if (st == WBX_OK) st = export_run(c, src, first_frame, n_frames, out_format, flags, dst, stats, &why);
  if (st != WBX_OK) c->err = why;
  return st;
}

extern "C" wbx_status wbx_set_master_init(wbx_ctx* c, const void* device_buffer) {
  if (!c) return WBX_ERR_INVALID;
  if ((uintptr_t)device_buffer & 15u) return fail(c, WBX_ERR_INVALID, "wbx_set_master_init: the buffer must be 16-byte aligned");
  c->master_init = (const float*)device_buffer;
  return WBX_OK;
}

extern "C" wbx_status wbx_set_master_target(wbx_ctx* c, void* device_buffer) {
  if (!c) return WBX_ERR_INVALID;
  c->master_target = (float*)device_buffer;
  c->master_target_on_host = false;
  if (device_buffer) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, device_buffer) == hipSuccess) c->master_target_on_host = at.type == hipMemoryTypeHost;
    else (void)hipGetLastError();
  }
  return WBX_OK;
}

extern "C" wbx_status wbx_submit(wbx_ctx* c, uint32_t K, uint32_t N, const wbx_segment* segs, const uint32_t* seg_offsets,
                                 const float* gains) {
  if (!c || !seg_offsets || !gains || K == 0 || N == 0) return WBX_ERR_INVALID;
  if (K > c->cfg.max_blocks || N > c->cfg.max_tracks) return fail(c, WBX_ERR_INVALID, "K or N above the configured maximum");
  (void)hipSetDevice(c->cfg.device);
  WBX_HIP(c, hipStreamSynchronize(c->plan_stream));
  wbx_status st = upload_tables(c, N);
  if (st != WBX_OK) return st;
  st = ensure_result_buffers(c, K, N);
  if (st != WBX_OK) return st;
  WBX_HIP(c, sync_main(c));   // staging vectors are reused
  const uint32_t F = c->cfg.block_frames, C = c->cfg.channels;
  c->h_tb.assign((size_t)K * N, DTrackBlock{});
  c->h_rows.assign((size_t)K * N, DRow{});
  c->h_pool.clear();
  std::vector<uint32_t> gen_idx;
  uint32_t chunks = 0;
  for (size_t bt = 0; bt < (size_t)K * N; bt++) {
    DTrackBlock& tb = c->h_tb[bt];
    tb.g[0] = gains[bt * 2 + 0];
    tb.g[1] = gains[bt * 2 + (C > 1 ? 1 : 0)];
    const uint32_t s0 = seg_offsets[bt], s1 = seg_offsets[bt + 1];
    if (s1 < s0) return fail(c, WBX_ERR_INVALID, "seg_offsets not monotone");
    if (s1 - s0 > kMaxSegs) return fail(c, WBX_ERR_OVERFLOW, "more than 16 segments in one track-block");
    if (s1 != s0 && !segs) return WBX_ERR_INVALID;
    for (uint32_t i = s0; i < s1; i++) {
      const wbx_segment& sg = segs[i];
      if (sg.clip >= c->clips.size() || !c->clips[sg.clip].used) return fail(c, WBX_ERR_INVALID, "segment names an unknown clip");
      // the ABI is the trust boundary: a negative / NaN position or a non-positive / NaN speed would index outside the clip
      if (!(sg.sample_offset >= 0.0) || !(sg.playback_speed > 0.0) || !(sg.playback_speed < 1e12))
        return fail(c, WBX_ERR_INVALID, "segment needs sample_offset >= 0 and 0 < playback_speed < 1e12");
      // the prologue of Sampler::stream (sampler.cpp:99-104) through the shared walker
      DTrackState ts{};
      ts.cur_type = EV_PLAY;
      ts.cur_sample = 0;
      ts.cur_gain = sg.gain;
      ts.playback_speed = sg.playback_speed;
      ts.sample_offset = sg.sample_offset;
      DSeg d{};
      BlockWalker w{};
      DTrackBlock scratch{};
      TrackCache tc{};
      tc.clip_idx = tc.next_idx = tc.smp_idx = tc.fin_tmpl = 0xFFFFFFFFu;
      uint32_t pc = 0, stbits = 0;
      w.st = &ts;
      w.cache = &tc;
      w.samples = &c->clips[sg.clip].d;
      w.tb = &scratch;
      w.pool = &d;
      w.pool_count = &pc;
      w.pool_chunks = 0;
      w.status = &stbits;
      w.n_samples = F;
      w.n_channels = C;
      w.dst_rate = (double)c->cfg.sample_rate;
      w.start_sample = 0;
      w.nseg = 0;
      w.chunk = 0xFFFFFFFFu;
      w.stream(sg.num_samples, sg.buffer_offset);
      d = get_seg0(scratch);
      d.sample = sg.clip;
      const uint32_t k = i - s0;
      if (k == 0) {
        set_seg0(&tb, d);
      } else {
        if (k == 1) {
          tb.extra = chunks++;
          c->h_pool.resize((size_t)chunks * kChunk);
        }
        c->h_pool[(size_t)tb.extra * kChunk + (k - 1)] = d;
      }
    }
    tb.nseg = (uint8_t)(s1 - s0);
    tb.kind = classify(tb, F);
    if (tb.kind == KIND_GENERIC) gen_idx.push_back((uint32_t)bt);
    // host-sequenced plans use one template per track-block: row bt -> template bt, position inside the template
    DRow& row = c->h_rows[bt];
    row.pos = tb.pos;
    row.tmpl = tb.nseg ? (uint32_t)bt : 0xFFFFFFFFu;
    row.flags = tb.kind == KIND_SILENT ? ROW_SILENT : 0u;
  }
  st = ensure_gen_capacity(c, gen_idx.size());
  if (st != WBX_OK) return st;
  st = ensure_template_capacity(c, (size_t)K * N);
  if (st != WBX_OK) return st;
  {
    uint32_t counters[4] = {0u, 0u, (uint32_t)gen_idx.size(), (uint32_t)((size_t)K * N)};
    WBX_HIP(c, hipMemcpyAsync(PB(c).counters.p, counters, sizeof(counters), hipMemcpyHostToDevice, c->stream));
    if (!gen_idx.empty())
      WBX_HIP(c, hipMemcpyAsync(PB(c).gen_list.p, gen_idx.data(), gen_idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    WBX_HIP(c, sync_main(c));   // counters / gen_idx are stack / local storage
  }
  if (chunks > PB(c).pool_chunks) {
    WBX_HIP(c, PB(c).pool.ensure((size_t)chunks * kChunk));
    PB(c).pool_chunks = chunks;
  }
  WBX_HIP(c, hipMemcpyAsync(PB(c).tmpl.p, c->h_tb.data(), c->h_tb.size() * sizeof(DTrackBlock), hipMemcpyHostToDevice, c->stream));
  WBX_HIP(c, hipMemcpyAsync(PB(c).prows.p, c->h_rows.data(), c->h_rows.size() * sizeof(DRow), hipMemcpyHostToDevice, c->stream));
  if (!c->h_pool.empty())
    WBX_HIP(c, hipMemcpyAsync(PB(c).pool.p, c->h_pool.data(), c->h_pool.size() * sizeof(DSeg), hipMemcpyHostToDevice, c->stream));
  RenderCall call;
  call.mix_stream = pick_mix_stream(c, K, false);   // host-sequenced plans are uploaded on the main stream: their mix follows there
  // host-sequenced plans say nothing about their clips, send every partial row through the pre-render pass and make no
  // promise about their playback speeds
  c->session = SessionFacts{};
  c->shape = render_shape(c, K, N, false);
  st = launch_pre_render(c, c->stream);
  if (st != WBX_OK) return st;
  return launch_mix_sum(c, K, N, call);
}

extern "C" wbx_status wbx_sync(wbx_ctx* c) {
  if (!c) return WBX_ERR_INVALID;
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  return WBX_OK;
}

extern "C" wbx_status wbx_master_ready(wbx_ctx* c, void* stream) {
  if (!c) return WBX_ERR_INVALID;
  hipStream_t on = stream ? (hipStream_t)stream : c->stream;
  if (on == c->stream) {
    WBX_HIP(c, join_sum(c));
    return WBX_OK;
  }
  if (c->sum_pending >= 0) {   // the sum runs on its own stream: its event orders any stream
    WBX_HIP(c, hipStreamWaitEvent(on, c->sum_done[c->sum_pending], 0));
  } else {                     // everything is on the main stream: mark where it stands now
    WBX_HIP(c, c->ready_ev.ensure(hipEventDisableTiming));
    WBX_HIP(c, hipEventRecord(c->ready_ev, c->stream));
    WBX_HIP(c, hipStreamWaitEvent(on, c->ready_ev, 0));
  }
  return WBX_OK;
}

wbx_status wbx::plan_status_to_error(wbx_ctx* c, uint32_t bits) {
  if (bits & 3u) return fail(c, WBX_ERR_OVERFLOW, "segment plan overflow (raise wbx_config.max_segments)");
  if (bits & 8u) return fail(c, WBX_ERR_OVERFLOW, "more boundary / non-fp32 track-blocks than pre-render rows");
  if (bits & 16u) return fail(c, WBX_ERR_OVERFLOW, "plan template array full");
  if (bits & 128u) {
    // the segmented sequencer planned a track again over rows its first versions of which were written behind another L2
    // (the workgroup-id -> XCD layout plan_seg_kernel rests on did not hold on this device): the rows of that render are in
    // doubt, it says so, and the engine plans by one lane per track from here on
    c->seg_broken = true;
    return fail(c, WBX_ERR_DEVICE, "the segmented sequencer's lanes of one track ran on more than one XCD and a seam was planned again: "
                                   "this render is invalid, later renders are planned by one lane per track");
  }
  if (bits & 96u) {
    // the chained hand-over rests on in-order workgroup dispatch and on a block's pieces sharing an XCD; a render that saw
    // either fail says so — its results are invalid — and the context walks whole lists from here on (same order of
    // additions, no hand-over between workgroups)
    c->chain_broken = true;
    return fail(c, WBX_ERR_DEVICE, (bits & 32u) ? "a chained workgroup gave up waiting for its predecessor's running sum: this render is invalid, "
                                                    "later renders walk whole lists"
                                                  : "a chained workgroup ran on another XCD than its predecessor: this render is invalid, later "
                                                    "renders walk whole lists");
  }
  return WBX_OK;
}

// Chained renders report a failed hand-over through a word of the context that outlives their plan buffers: read it (the
// streams are idle), clear it, turn it into the error — and into whole-list walks from then on.
wbx_status wbx::render_status(wbx_ctx* c) {
  if (!c->d_sticky_status.p || c->chain_epoch == 0u) return WBX_OK;   // (no chained render so far)
  uint32_t bits = 0;
  WBX_HIP(c, hipMemcpy(&bits, c->d_sticky_status.p, sizeof(bits), hipMemcpyDeviceToHost));
  if (!bits) return WBX_OK;
  WBX_HIP(c, hipMemset(c->d_sticky_status.p, 0, sizeof(uint32_t)));
  return plan_status_to_error(c, bits & 96u);
}

extern "C" wbx_status wbx_render_status(wbx_ctx* c) {
  if (!c) return WBX_ERR_INVALID;
  (void)hipSetDevice(c->cfg.device);
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  return render_status(c);
}

extern "C" wbx_status wbx_fetch(wbx_ctx* c, float* const* master_planar, float* peaks, float* buses) {
  if (!c) return WBX_ERR_INVALID;
  if (c->last_K == 0) return fail(c, WBX_ERR_FAILED, "nothing submitted");
  WBX_HIP(c, join_sum(c));
  const uint32_t K = c->last_K, N = c->last_N, C = c->cfg.channels, F = c->cfg.block_frames;
  if (master_planar && c->last_master_format)
    return fail(c, WBX_ERR_INVALID, "the last render left its master in a device format (wbx_set_master_format): wbx_fetch_interleaved");
  if (master_planar) {
    // device [K][C][F] -> host planar[c][b*F + j]
    for (uint32_t ch = 0; ch < C; ch++)
      if (c->last_master_on_host) {   // Engine::process: the block is already on the host
        WBX_HIP(c, sync_main(c));
        for (uint32_t b = 0; b < K; b++)
          std::memcpy(master_planar[ch] + (size_t)b * F, c->last_master + ((size_t)b * C + ch) * F, F * sizeof(float));
      } else {
        WBX_HIP(c, hipMemcpy2DAsync(master_planar[ch], F * sizeof(float), c->last_master + (size_t)ch * F,
                                    (size_t)C * F * sizeof(float), F * sizeof(float), K, hipMemcpyDeviceToHost, c->stream));
      }
  }
  if (peaks) WBX_HIP(c, hipMemcpyAsync(peaks, c->last_peaks, (size_t)K * N * C * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (buses) {
    if (!c->n_buses) return fail(c, WBX_ERR_INVALID, "no buses configured");
    WBX_HIP(c, hipMemcpyAsync(buses, c->last_buses, (size_t)K * c->n_buses * C * F * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  uint32_t pc[4] = {0, 0, 0, 0};
  WBX_HIP(c, hipMemcpy(pc, PB(c).counters.p, sizeof(pc), hipMemcpyDeviceToHost));
  const wbx_status rs = render_status(c);   // (an earlier, unfetched render's failure counts too)
  const wbx_status ps = plan_status_to_error(c, pc[1]);
  return ps != WBX_OK ? ps : rs;
}

extern "C" wbx_status wbx_fetch_interleaved(wbx_ctx* c, int out_format, void* dst) {
  if (!c || !dst) return WBX_ERR_INVALID;
  if (c->last_K == 0) return fail(c, WBX_ERR_FAILED, "nothing submitted");
  WBX_HIP(c, join_sum(c));
  const size_t eb = out_format_bytes(out_format);
  if (!eb) return fail(c, WBX_ERR_UNSUPPORTED, "interleaved output format");
  const uint32_t K = c->last_K, C = c->cfg.channels, F = c->cfg.block_frames;
  if (c->last_master_format) {   // the sum kernel already wrote this format (wbx_set_master_format): a copy
    if (c->last_master_format != out_format) return fail(c, WBX_ERR_INVALID, "the last render's master is in another device format");
    if (c->last_master_on_host) {
      WBX_HIP(c, sync_main(c));
      if (out_format == WBX_OUT_I24)
        for (uint32_t b = 0; b < K; b++) std::memcpy((char*)dst + (size_t)b * F * C * 3, (const char*)c->last_master + (size_t)b * F * C * 3, (size_t)F * 3);
      else
        std::memcpy(dst, c->last_master, (size_t)K * F * C * eb);
      return render_status(c);
    }
    if (out_format == WBX_OUT_I24)
      WBX_HIP(c, hipMemcpy2DAsync(dst, (size_t)F * C * 3, c->last_master, (size_t)F * C * 3, (size_t)F * 3, K, hipMemcpyDeviceToHost, c->stream));
    else
      WBX_HIP(c, hipMemcpyAsync(dst, c->last_master, (size_t)K * F * C * eb, hipMemcpyDeviceToHost, c->stream));
    WBX_HIP(c, sync_main(c));
    return render_status(c);
  }
  if (out_format == WBX_OUT_I24) {
    // convert_f32_to_interleaved_i24 (audio_format_conv.cpp:22-43) writes byte 3*i.. of EVERY channel's sample i — the
    // destination index has no channel term — so per converted block the last channel's packed samples fill bytes
    // [0, 3F) and the remaining 3F(C-1) bytes of the block's region are never touched: reproduced as written
    WBX_HIP(c, c->d_conv.ensure((size_t)K * F * 3));
    launch_convert(c->last_master, c->d_conv.p, K, F, C, out_format, c->stream);
    WBX_HIP(c, hipMemcpy2DAsync(dst, (size_t)F * C * 3, c->d_conv.p, (size_t)F * 3, (size_t)F * 3, K, hipMemcpyDeviceToHost, c->stream));
    WBX_HIP(c, sync_main(c));
    return render_status(c);
  }
  const size_t bytes = (size_t)K * F * C * eb;
  WBX_HIP(c, c->d_conv.ensure(bytes));
  launch_convert(c->last_master, c->d_conv.p, K, F, C, out_format, c->stream);   // pinned staging is device-readable too
  WBX_HIP(c, hipMemcpyAsync(dst, c->d_conv.p, bytes, hipMemcpyDeviceToHost, c->stream));
  WBX_HIP(c, sync_main(c));
  return render_status(c);
}

extern "C" wbx_status wbx_partial_master(wbx_ctx* c, void** device_ptr, size_t* n_floats) {
  if (!c || !device_ptr) return WBX_ERR_INVALID;
  if (c->last_K == 0) return fail(c, WBX_ERR_FAILED, "nothing submitted");
  WBX_HIP(c, join_sum(c));
  *device_ptr = c->last_master;
  if (n_floats) *n_floats = (size_t)c->last_K * c->cfg.channels * c->cfg.block_frames;
  return WBX_OK;
}

extern "C" wbx_status wbx_finalize_master(wbx_ctx* c, void* device_partial, uint32_t n_blocks, int clamp, void* stream) {
  if (!c || !device_partial || n_blocks == 0) return WBX_ERR_INVALID;
  hipStream_t on = stream ? (hipStream_t)stream : c->stream;
  if (c->sum_pending >= 0) WBX_HIP(c, hipStreamWaitEvent(on, c->sum_done[c->sum_pending], 0));
  if (clamp) launch_clamp((float*)device_partial, (size_t)n_blocks * c->cfg.channels * c->cfg.block_frames, on);
  WBX_HIP(c, hipGetLastError());
  return WBX_OK;
}

extern "C" wbx_status wbx_finalize_master_into(wbx_ctx* c, const void* device_partial, void* dst, uint32_t n_blocks, int clamp,
                                               void* stream) {
  if (!c || !device_partial || !dst || n_blocks == 0) return WBX_ERR_INVALID;
  if (((uintptr_t)device_partial | (uintptr_t)dst) & 15u) return fail(c, WBX_ERR_INVALID, "finalize: buffers must be 16-byte aligned");
  hipStream_t on = stream ? (hipStream_t)stream : c->stream;
  if (c->sum_pending >= 0) WBX_HIP(c, hipStreamWaitEvent(on, c->sum_done[c->sum_pending], 0));
  launch_clamp_into((const float*)device_partial, (float*)dst, (size_t)n_blocks * c->cfg.channels * c->cfg.block_frames, clamp, on);
  WBX_HIP(c, hipGetLastError());
  return WBX_OK;
}

// Bound how far the submitting thread runs ahead of the device: beyond a few dozen queued renders the HIP runtime
// blocks a launch until its queue has emptied and the device then idles.  Call after each submit / render: the host
// waits (only) until the render issued `max_ahead` calls ago has left the main stream.
extern "C" wbx_status wbx_pace(wbx_ctx* c, uint32_t max_ahead) {
  if (!c || max_ahead == 0 || max_ahead >= kPaceRing) return WBX_ERR_INVALID;
  (void)hipSetDevice(c->cfg.device);
  const uint32_t slot = (uint32_t)(c->pace_seq % kPaceRing);
  WBX_HIP(c, c->pace_ev[slot].ensure(kDevEventFlags));   // (the host waits for "done", reads nothing)
  // (behind the last render's sum when that runs on its own stream: no marker between two mixes)
  hipStream_t where = c->cur_mix_stream ? c->cur_mix_stream : c->stream;
  if (c->sum_pending >= 0 && c->sum_stream && !c->dist) where = c->sum_stream;
  WBX_HIP(c, hipEventRecord(c->pace_ev[slot], where));
  if (c->pace_seq >= max_ahead) WBX_HIP(c, hipEventSynchronize(c->pace_ev[(c->pace_seq - max_ahead) % kPaceRing]));
  c->pace_seq++;
  return WBX_OK;
}

extern "C" wbx_status wbx_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return WBX_ERR_INVALID;
  *out = nullptr;
  if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) return WBX_ERR_OOM;
  std::memset(*out, 0, bytes);
  return WBX_OK;
}

extern "C" wbx_status wbx_host_free(void* p) {
  if (!p) return WBX_OK;
  return hipHostFree(p) == hipSuccess ? WBX_OK : WBX_ERR_DEVICE;
}

extern "C" const char* wbx_kernel_name(wbx_ctx* c) { return c ? c->mix_kernel_name : ""; }
extern "C" double wbx_render_uniform_speed(wbx_ctx* c) { return c ? c->last_uniform_speed : 0.0; }
extern "C" uint32_t wbx_xcd_count(wbx_ctx* c) { return c ? c->n_xcds : 0u; }

extern "C" wbx_status wbx_kernel_time(wbx_ctx* c, int reset, double* mix_ms_avg, uint64_t* mix_launches) {
  if (!c) return WBX_ERR_INVALID;
  WBX_HIP(c, join_sum(c));
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  if (mix_ms_avg) *mix_ms_avg = c->mix_launches ? c->mix_ms_total / (double)c->mix_launches : 0.0;
  if (mix_launches) *mix_launches = c->mix_launches;
  if (reset) {
    c->mix_ms_total = 0.0;
    c->tail_ms_total = 0.0;
    c->mix_launches = 0;
    c->gap_ms_total = 0.0;
    c->gap_count = 0;
  }
  return WBX_OK;
}

extern "C" wbx_status wbx_gap_time(wbx_ctx* c, double* gap_ms_avg, uint64_t* gaps) {
  if (!c || !gap_ms_avg) return WBX_ERR_INVALID;
  WBX_HIP(c, join_sum(c));
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  *gap_ms_avg = c->gap_count ? c->gap_ms_total / (double)c->gap_count : 0.0;
  if (gaps) *gaps = c->gap_count;
  return WBX_OK;
}

extern "C" wbx_status wbx_tail_time(wbx_ctx* c, double* tail_ms_avg) {
  if (!c || !tail_ms_avg) return WBX_ERR_INVALID;
  WBX_HIP(c, join_sum(c));
  WBX_HIP(c, sync_main(c));
  drain_events(c);
  *tail_ms_avg = c->mix_launches ? c->tail_ms_total / (double)c->mix_launches : 0.0;
  return WBX_OK;
}
