// wbx_shape.h — which instance of the hot kernel a render takes, and everything that follows from that choice: one pure
// function from (knobs, facts) to a RenderShape.  Plain C++ (no HIP, no wbx_ctx): the library calls it once per render,
// tests/cpp/host_sim.cpp compiles it with g++ and holds it against the census of compiled instances without a device.
//
// The conditions here are the only copy.  The launchers (wbx_kernels.hip, wbx_mix_fam<N>.hip) look the chosen instance up
// by its template arguments and launch it; they decide nothing.
//
// Beside it, in the same way: choose_issue — how a render's launches are issued (streams, fusing, the one-launch callback,
// the staged master) — from (knobs, facts) to a RenderIssue, called once per launch_mix_sum; and choose_plan — how a render is
// planned (the sequencer's launch and stream, its transport table, counters and reservations) — to a RenderPlan, called once
// per render_locked.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/wbx.h"
#include "wbx_dev.h"
#include "wbx_knobs.h"

namespace wbx {

constexpr uint32_t kOverlapMinBlocks = 8;   // renders shorter than this run plan, mix and sum on the main stream

// (ShapeKnobs, the switches that enter the choice, read once per context at wbx_create: wbx_knobs.h)

// What the session holds.  The defaults are layer 1's, whose host-sequenced plans say nothing about their clips:
// "unknown, assume so".
struct SessionFacts {
  bool window_clips = true;     // a clip that is linearly resampled (playback speed != 1)
  bool stride_clips = true;     // fp32 played faster than recorded, resampled integer PCM above 0.999
  bool taps_clips = true;       // ... of those, rows read with per-frame taps (KIND_STRIDE): the instance must carry MODE_G
  bool lean16_clips = false;    // resampled clips exist and all of them are 16-bit PCM at speeds up to 0.999
  bool cut_tracks = true;       // some track holds more than one clip
  bool host_sequenced = true;   // the plan comes from the host (layer 1): every partial row goes through the pre-render pass
  double uniform_speed = 0.0;   // > 0: every linearly resampled row plays at exactly this speed (MixArgs::uniform_speed)
};

struct ShapeFacts {
  // the configuration
  uint32_t channels = 2, block_frames = 512;
  uint32_t group_size = 0;      // tracks per workgroup-sized piece (the library's choice filled in) ...
  bool auto_group = false;      // ... and whether it was the library's
  // the session, its clip table and its routing
  SessionFacts session;
  bool integer_clips = false;   // a clip asset that is not fp32
  bool non16_clips = false;     // a clip asset that is not 16-bit PCM
  uint32_t n_buses = 0;
  uint32_t longest_list = 0;    // tracks in the longest member list
  // the render
  uint32_t n_blocks = 1, n_tracks = 0;
  bool callback = false;        // the one-block callback of wbx_engine_process, nothing in it for the pre-render pass to wait for
  // the context's state
  bool chain_broken = false;    // a chained render reported a failed hand-over
  bool mix_alternate = false;   // WBX_MIX_ALT=1: two renders' mixes side by side
  bool dist = false;            // a multi-GPU exchange is attached
};

// One instance of mix_kernel / mix_kernel_x / callback_kernel, by its template arguments
struct MixInstance {
  enum Kind : uint8_t { MIX, MIX_X, CALLBACK };
  Kind kind = MIX;
  uint8_t U = 2, FULL = 1, W = 4, FAM = 0, SB = 1, CW = 1, CL = 1, X = 0;
  uint16_t T = 256;             // lanes of its workgroup

  static MixInstance mix(int U, bool FULL, int W, int FAM, int SB, int CW, int CL, int T) {
    return {MIX, (uint8_t)U, (uint8_t)FULL, (uint8_t)W, (uint8_t)FAM, (uint8_t)SB, (uint8_t)CW, (uint8_t)CL, 0, (uint16_t)T};
  }
  static MixInstance mix_x(int U, int W, int FAM, int SB, int CW, int X) {
    return {MIX_X, (uint8_t)U, 1, (uint8_t)W, (uint8_t)FAM, (uint8_t)SB, (uint8_t)CW, 1, (uint8_t)X, 256};
  }
  static MixInstance callback(int U, int FAM) { return {CALLBACK, (uint8_t)U, 1, 0, (uint8_t)FAM, 1, 1, 1, 0, 256}; }

  uint64_t key() const {
    return (uint64_t)kind | (uint64_t)U << 8 | (uint64_t)FULL << 16 | (uint64_t)W << 20 | (uint64_t)FAM << 24 | (uint64_t)SB << 28 |
           (uint64_t)CW << 32 | (uint64_t)CL << 36 | (uint64_t)X << 40 | (uint64_t)T << 44;
  }
  // as nm -C and rocprofv3 spell it
  void name(char* out, size_t n) const {
    if (kind == MIX)
      std::snprintf(out, n, "wbx::mix_kernel<%d, %s, %d, %d, %d, %d, %d, %d>", U, FULL ? "true" : "false", W, FAM, SB, CW, CL, T);
    else if (kind == MIX_X)
      std::snprintf(out, n, "wbx::mix_kernel_x<%d, %d, %d, %d, %d, %d>", U, W, FAM, SB, CW, X);
    else
      std::snprintf(out, n, "wbx::callback_kernel<%d, %d>", U, FAM);
  }
};

struct RenderShape {
  int family = 1;               // which chunk modes the instance carries: 0 fp32 + integer PCM at unity speed; 1 everything (also
                                // the pipelined modes for chunks that mix storage formats with resampled rows); 2 sessions of
                                // 16-bit PCM only, resampled at speeds up to 0.999 or not at all; 3 = 1 without the per-frame taps
  MixInstance mix;              // the batch instance (also what a callback block takes when it runs as three launches)
  uint32_t lane_span = 0;       // MixArgs::lane_span / tiles of that instance
  uint32_t tiles = 1;
  uint32_t grid_z = 1;          // its grid: (ceil(K / mix.SB), groups, grid_z)
  uint32_t blocks_per_workgroup = 1;   // ... of the instance the grouped order launches: what the whole-list threshold counts
  uint32_t resident = 1;        // ... and how many of its workgroups the device holds at once, in units of 1024
  bool walks_lists = false;     // the render takes the member lists whole (the reference's summation order) ...
  bool chained = false;         // ... as chained workgroup-sized pieces
  uint32_t masked_rows = 0;     // PlanArgs::masked_rows: the partial-coverage rows the sequencer may hand the hot loop
  uint32_t gen_grid = 0;        // bound of the pre-render grid, in four-wave units
  double uniform_speed = 0.0;
  bool cb_one_launch = false;   // a one-block render of wbx_engine_process runs as ONE launch (wbx_callback.h) ...
  uint32_t cb_lane_span = 0;    // ... with this lane space (0: no instance fits the block) ...
  MixInstance cb;               // ... through this instance
};

// The lane space of the instance a block of F = 4 * S4 frames and C channels takes (MixArgs::lane_span): lanes per channel and
// block.  The instances are cut for blocks of 128 frames (stereo), 256, 512, 1024 ... — what the reference's settings dialog
// offers (ui/settings.cpp:22-24) — but the block a device back end really opens is its period, realigned to 32 frames
// (config.cpp:146-149,217-222): 480 frames for WASAPI's 10 ms at 48 kHz, 416 at 44.1 kHz, 960 for 20 ms.  Such a block takes
// the next shape above it; its surplus lanes clone the block's last four frames (wbx_mix.h).  WBX_RAGGED=0: the general
// instance of earlier rounds instead (A/B aid).
// (`ragged_off`: WBX_RAGGED=0 as the context read it when it was created (wbx_knobs.h): the plan-time and launch-time choices
//  of one context cannot disagree)
inline uint32_t native_lane_span(uint32_t C, uint32_t S4, bool ragged_off) {
  const uint32_t lanes = C * S4;
  const bool exact = ((lanes % 256u == 0u) && (S4 % 64u == 0u)) || (C == 2u && S4 == 32u) ||
                     (S4 % 64u == 0u && (lanes == 128u || lanes == 64u));
  if (exact || ragged_off) return S4;
  if (C == 2u) return S4 <= 32u ? 32u : S4 <= 64u ? 64u : S4 <= 128u ? 128u : S4 <= 256u ? 256u : (S4 + 127u) / 128u * 128u;
  return S4 <= 64u ? 64u : S4 <= 128u ? 128u : S4 <= 256u ? 256u : (S4 + 255u) / 256u * 256u;
}

// Does a render of n_blocks short blocks (shorter than a 256-lane workgroup) of a session cut into clips take the PACKED
// masked-row instance (mix_kernel_x) instead of one block per workgroup?  Measured (tools/ab.py packed, profiles/r04_ab_packed.txt):
// 128-frame stereo (four blocks per workgroup) +5-9 % over the one-wave instance; 256-frame stereo / 512-frame mono (two blocks)
// 6-13 % BEHIND theirs — those keep one block per workgroup.  Renders of a few blocks: one workgroup per block is the shorter
// chain.  WBX_PACKED_X=0|1: A/B aid, tests (1 = every shape that has a packed instance) — `forced` is what the context read
// when it was created (-1: unset).
inline int packed_masked_variant(uint32_t n_blocks, bool stereo128, int forced) {
  if (forced >= 0) return forced;
  return (stereo128 && n_blocks >= 8u) ? 1 : 0;
}

inline RenderShape choose_shape(const ShapeKnobs& k, const ShapeFacts& f) {
  const SessionFacts& ses = f.session;
  const uint32_t K = f.n_blocks, C = f.channels;
  const uint32_t S4 = native_lane_span(C, f.block_frames >> 2, k.ragged_off), lanes = C * S4;   // (the instance's lane space)
  const uint32_t F = 4u * S4;                                                                    // (... and its block size)
  const bool cut = ses.cut_tracks || k.force_cut;
  const bool short_render = K < kOverlapMinBlocks;   // (the callback path)
  RenderShape r;
  r.lane_span = S4;
  r.tiles = (lanes + 255u) / 256u;
  r.uniform_speed = ses.uniform_speed;

  // -- the block shapes the instances are cut for: whole 256-lane workgroups, or one of the short blocks
  const bool full = (lanes % 256u == 0u) && (S4 % 64u == 0u);
  const bool st128 = C == 2u && S4 == 32u;               // 128-frame stereo: one block per wave, a channel per half-wave
  const bool st256 = C == 2u && S4 == 64u;               // 256-frame stereo
  const bool two = S4 % 64u == 0u && lanes == 128u;      // 256-frame stereo (a wave per channel), 512-frame mono
  const bool four = S4 == 64u && lanes == 64u;           // 256-frame mono
  const bool short_ok = st128 || two || four;

  // -- the family
  if (k.force_g)
    r.family = 1;
  else if (ses.lean16_clips && !f.non16_clips && !k.no_lean16)
    r.family = 2;
  else if (ses.stride_clips || (ses.window_clips && f.integer_clips))
    r.family = (ses.taps_clips || k.no_fam3) ? 1 : 3;
  else
    r.family = 0;
  const int fam = r.family;

  // fp32 sessions of one clip per track with resampled clips (c3), chained renders of 2048 blocks and more: the two-channels-per-
  // lane instance with ONE row per pipeline batch, <1,true,3,0,1,1,2,128>.  Round 2 measured these sessions 3 % slower through
  // the CL = 2 instances — at 256-block renders in the grouped order; at 2048 chained blocks, with the one-ratio modes taken
  // again, five alternating runs on one box (profiles/r05_ab_c3_instances.txt) read 0.711 of the roofline for it, 0.701 for
  // <2,true,3,..,2,128>, 0.694 for the one-channel-per-wave <2,true,4,..,1,256>; at 1024 and 256 blocks nothing to choose.
  auto long_chained_window_render = [&](bool chained) {
    return C == 2u && F == 512u && chained && K >= 2048u && ses.window_clips && !f.integer_clips && !cut &&
           !ses.stride_clips && !f.n_buses;
  };

  // stereo sessions with integer-PCM clips or with tracks cut into several clips, blocks of 256 / 512 / 1024 frames: the
  // instances with both channels of a frame in one lane (position and masked-row arithmetic once per frame, one set of record
  // scalars for both channels).  Measured (tools/ab_cl2.sh, tools/ab_masked.sh, tools/ab_blocks.sh; slab-allocated sessions):
  // integer PCM +2-10 %, sessions cut into clips +5-11 % (2 x at 256 frames, where the other instances have no masked
  // rows), fp32 sessions of one clip per track 3-8 % slower (they fetch 1.06 x their bytes instead of 1.02 x) — those keep
  // one channel per wave.
  auto two_channels_per_lane = [&](bool whole, bool chained) {
    if (k.mix_variant) return k.mix_variant >= 1000;
    if (C != 2u || k.no_cl2) return false;
    if (!(F == 512u || F == 1024u || F == 256u)) return false;
    // the callback path (a handful of workgroups, each a chain of dependent rows): a wave per channel half — four waves share
    // the chain instead of two (measured, 4096 / 64 tracks: 16-bit resampled 53 -> 51 / 55 -> 49 us, cut into clips 63 -> 58 /
    // 66 -> 58, 24-bit 55 -> 53 / 58 -> 53).  256-frame blocks keep the one-wave instances: only those take their masked rows.
    if (short_render && F != 256u) return false;
    // a render whose workgroups walk whole member lists of many staged chunks: the half-size workgroups of these instances
    // put six of them on a CU, and the walk runs 15 % faster than through the four-wave ones (c3, 1024 blocks: 2.94 vs 3.43 ms)
    if (whole && f.longest_list > 2u * kStage) return true;
    if (long_chained_window_render(chained)) return true;
    return f.integer_clips || cut;
  };

  // -- the instance, and what goes with it, of a render that walks the member lists whole / chained / in the grouped order
  struct Pick {
    MixInstance inst;
    uint32_t masked_rows, resident;
  };
  auto pick = [&](bool whole, bool chained) {
    Pick p{};
    // variant = 10*U + W: U tracks per pipeline stage, W = waves per SIMD the register budget is capped for; >= 1000: both
    // channels of a frame per lane.
    // (unity-speed fp32 sessions: four rows per pipeline batch at three waves per SIMD, <4,true,3,..> — round 2's choice at
    //  256-block renders; in renders of >= 2048 blocks of large sessions two rows at four waves, <2,true,4,..>, is ahead:
    //  c4 0.72-0.75 of the roofline against 0.67-0.69, u4096 0.755-0.777 against 0.746-0.763, one box, alternating
    //  (profiles/r05_ab_c3_instances.txt); 256-track sessions: nothing to choose)
    const bool long_large = K >= 2048u && f.n_tracks >= 1024u;
    const int v = k.mix_variant                        ? k.mix_variant
                  : two_channels_per_lane(whole, chained) ? (long_chained_window_render(chained) ? 1013 : 1023)
                                                       : ((ses.window_clips || f.integer_clips || long_large) ? 24 : 43);
    const bool cl2 = v >= 1000 && C == 2u;
    // stereo 256-frame blocks with both channels per lane: one wave = one block (the lean families only)
    const bool one_wave_cl2 = cl2 && st256 && (fam == 0 || fam == 2);

    // Can the instance take masked rows (partial-coverage records, ROW_PAIRs) in its hot loop, and which
    // (PlanArgs::masked_rows)?  The whole-workgroup-per-block instances do; of the short blocks the one-wave instance above,
    // and — for a session with tracks cut into clips — the one-block-per-workgroup and packed instances of families 0 and 1.
    // The others keep the instances that put 2 or 4 blocks into a workgroup.
    // 4: the everything family — every row kind it streams, also as a masked row; 3: sessions of 16-bit PCM only — also
    // their resampled rows; 1: fp32 rows, unity or resampled; 2: also integer PCM at unity speed (family 0 holds no resampled
    // integer clip).
    const bool takes = full || one_wave_cl2 || (cut && short_ok);
    p.masked_rows = (!takes || ses.host_sequenced || k.masked_rows_off) ? 0u
                    : (fam == 1 || fam == 3)                            ? 4u
                    : fam == 2                                          ? 3u
                    : f.integer_clips                                   ? 2u
                                                                        : 1u;
    const bool masked = p.masked_rows != 0u;
    p.resident = 1u;
    if (!full) {
      // Families 2 and 3 have no short-block instances and family 0 none for odd shapes: those renders are NAMED an instance
      // of the everything family, which holds all of their modes.
      const int sfam = fam == 0 ? 0 : 1;
      const int sb = st128 ? 4 : two ? 2 : 4, cw = st128 ? 2 : 1;
      if (!short_ok) {
        p.inst = MixInstance::mix(2, false, 1, 1, 1, 1, 1, 256);   // any block shape: lane predicates, records read from LDS per lane
      } else if (masked && packed_masked_variant(K, st128, k.packed_x) && !(one_wave_cl2 && fam == 2)) {
        // short blocks of a session cut into clips, renders of 8 blocks and more: the packed instances that take masked rows
        // (2 or 4 blocks per workgroup like the ones below, the staging of the one-block instances per sub-block)
        p.inst = MixInstance::mix_x(2, 4, sfam, sb, cw, 1);
      } else if (one_wave_cl2) {
        p.inst = MixInstance::mix(2, true, 3, fam, 1, 1, 2, 64);
        // (a cut session's is counted like the wave-per-channel instance it replaced: the threshold as it was measured)
        p.resident = (cut && !k.masked_rows_off) ? 2u : 3u;
      } else if (masked) {
        // short blocks of a session cut into clips: one block per workgroup (a wave, or two), the instances that take the
        // sequencer's masked rows — clip boundaries stay in the hot loop instead of going through the pre-render pass
        p.inst = MixInstance::mix(2, true, 3, sfam, 1, cw, 1, two ? 128 : 64);
        p.resident = lanes <= 64u ? 3u : 2u;
      } else {
        // blocks shorter than a workgroup whose waves are still channel-uniform: 2 or 4 consecutive blocks per workgroup, same
        // code as the full instances
        p.inst = MixInstance::mix(2, true, 4, sfam, sb, cw, 1, 256);
      }
    } else if (fam == 1 || (fam == 3 && !(cl2 && S4 == 128u))) {
      // (W = 4 although this instance spills a few registers there: at W = 3 it is 5-10 % slower.  Family 3 holds only the
      //  512-frame instance with both channels per lane: every other shape is named the everything family's)
      p.inst = MixInstance::mix(2, true, 4, 1, 1, 1, 1, 256);
    } else if (fam == 3) {
      // one row per pipeline batch: with two, this family's widest modes spill 84 B per lane at three waves per SIMD
      // (measured, one box: i24r 0.650 -> 0.690 of the roofline, mixr 0.501 -> 0.530, cut into clips +2-3 %; two waves per SIMD
      // without spills — <2,true,2,...> — 0.62 / 0.51, <4,true,2,...> 0.61 / 0.48).  WBX_MIX_VARIANT=1022: two rows per batch.
      p.inst = MixInstance::mix(v == 1022 ? 2 : 1, true, 3, 3, 1, 1, 2, 128);
    } else if (cl2 && S4 == 128u) {
      // stereo 512-frame blocks with both channels of a frame in one lane (workgroups of 128 lanes = one block; 26 KiB of LDS
      // each: three waves per SIMD).  1042: twice the rows in flight per wave at two waves per SIMD (whole-list walks of 1024
      // blocks: four workgroups per CU)
      p.inst = MixInstance::mix(v == 1013 ? 1 : v == 1042 ? 4 : 2, true, v == 1042 ? 2 : 3, fam, 1, 1, 2, 128);
    } else if (cl2 && S4 == 256u) {
      p.inst = MixInstance::mix(2, true, 3, fam, 1, 1, 2, 256);   // ... and 1024-frame ones: workgroups of 256 lanes = one block
    } else if (fam == 2) {
      p.inst = MixInstance::mix(2, true, 4, 2, 1, 1, 1, 256);
    } else {
      // (tuning knob WBX_MIX_VARIANT; every variant computes identical results.  1/6, 2/5, 2/6, 4/4, 4/5 spill and were
      //  10-60 % slower)
      p.inst = v == 43 ? MixInstance::mix(4, true, 3, 0, 1, 1, 1, 256)
               : v == 82 ? MixInstance::mix(8, true, 2, 0, 1, 1, 1, 256)
                         : MixInstance::mix(2, true, 4, 0, 1, 1, 1, 256);
    }
    return p;
  };

  // -- Does the render take the member lists whole (one workgroup per member list and block)?  Only when the library
  // picks the grouping (wbx_config.group_size == 0) and the render is long enough to fill the device with one workgroup
  // per block: the parallelism that track groups give a short render comes from the K blocks of a long one.  Measured on
  // c3 (profiles/): from about a thousand blocks per render on, whole-list walks run at the grouped order's rate.
  // What counts is the number of workgroup COLUMNS, not of blocks: the instances for blocks shorter than a workgroup put 2 or 4
  // consecutive blocks into one, and a 1024-block render of 128-frame blocks through them is 256 columns — 256 chains, or 256
  // walks, on a device that holds a thousand workgroups (measured: 0.30 of the roofline instead of 0.60).
  // (-> blocks per workgroup of the instance the grouped order launches; `resident`: how many workgroups of that instance the
  //  device holds at once, in units of the 1024 that the four-wave instances come to.  A chained piece waits for its
  //  predecessor while it occupies a slot: with fewer columns than resident workgroups several pieces of a block are resident
  //  TOGETHER and all but one of them wait — measured on the one-wave instances, 3072 resident: 0.25 of the roofline at 1024
  //  columns, 0.45 at 2048, against 0.6 unchained)
  const Pick grouped = pick(false, false);
  r.blocks_per_workgroup = grouped.inst.SB;
  r.resident = grouped.resident;
  r.walks_lists = f.auto_group && k.exact_min_blocks != 0u && K / r.blocks_per_workgroup >= k.exact_min_blocks * r.resident;
  // ... and of those, which chain the workgroup-sized pieces instead of walking a list in one workgroup: the same order of
  // additions, but scheduled like the grouped order (many short workgroups, dispatched dynamically) — a static assignment of
  // one long walk per workgroup ends when its slowest shader engine does (profiles/r03_wg_clocks.txt: 25-40 % behind the mean).
  // (a reported hand-over failure: whole-list walks from then on.  WBX_MIX_ALT=1 runs two renders' mixes side by side, and
  //  the words of both would share one buffer with only the epoch to tell them apart: render i+1's pieces overwrite words
  //  render i's successors still poll — no chaining there.  K a multiple of 32: every instance's grid then has an x extent
  //  that is a multiple of 8, which keeps the pieces of a block on one XCD — what the chain's L2-level hand-over rests on;
  //  other lengths walk the lists whole)
  r.chained = r.walks_lists && !(k.chain_off || f.chain_broken || f.mix_alternate) && f.longest_list > f.group_size && (K % 32u) == 0u;
  const Pick p = r.walks_lists ? pick(!r.chained, r.chained) : grouped;
  r.mix = p.inst;
  r.masked_rows = p.masked_rows;
  r.grid_z = p.inst.CL == 2 ? 1u : r.tiles;
  // the pre-render pass, one wave per queued row, grid-stride: no more workgroups than the device holds at once (256 CUs x 6
  // workgroups at the kernel's register budget), or the surplus would start when the first ones have finished their whole share
  // (a plan made for a masked-row mix instance queues only what is left over: blocks with three or more stream calls,
  //  overlapping calls — a handful per render at most)
  r.gen_grid = short_render ? 64u * K : r.masked_rows ? 128u : 1536u;

  // -- Does a one-block render of wbx_engine_process run as ONE launch (wbx_callback.h)?  Blocks that are exactly one 256-lane
  // workgroup (512-frame stereo, 1024-frame mono), no multi-GPU exchange — and every block that FITS one: the callback is a
  // latency path — what counts is one dispatch instead of three, not how many of the workgroup's lanes own frames — so a 128-
  // or 256-frame stereo block (the low-latency settings of ui/settings.cpp:22-24) runs through the same 256-lane instance with
  // lane_span = 256 / C, its surplus lanes cloning the block's last four frames (wbx_mix.h).
  if (lanes == 256u && (S4 % 64u) == 0u)
    r.cb_lane_span = S4;
  else if (!k.cb_any_off && !k.ragged_off && C * (f.block_frames >> 2) <= 256u)
    r.cb_lane_span = 256u / C;
  r.cb_one_launch = f.callback && K == 1u && !k.callback_unfused && !f.dist && r.cb_lane_span != 0u && !k.mix_variant;
  // (a callback workgroup is a latency chain — one pipeline batch per memory round trip — and has a CU to itself.  Measured,
  //  16 tracks per workgroup: the rows that pad the last pipeline batch are rendered like real ones, and a callback workgroup
  //  is bound by instruction issue — U = 2: 11.3 us, 4: 11.6, 8: 13.4.  Family 3 = 1 without the per-frame taps: one instance
  //  serves both)
  r.cb = fam == 0 ? MixInstance::callback(k.cb_u == 8 ? 8 : k.cb_u == 4 ? 4 : 2, 0) : MixInstance::callback(2, fam == 2 ? 2 : 1);
  return r;
}

// ---- how a render is issued -------------------------------------------------------------------------------------------
// Which streams the mix and the sum of a render take, which launches it is made of and what is recorded between them: one
// pure function from (knobs, facts) to a RenderIssue, called once at the top of launch_mix_sum (wbx_runtime.hip), which
// then only fills arguments and issues.  tests/test_host_logic.py holds it against the rules written out again.

struct IssueFacts {
  // the render and its RenderShape (tiles: the shape's value, before the callback instance overrides it)
  uint32_t K = 1, n_groups = 0, n_buses = 0, tiles = 1, block_frames = 512, channels = 2;
  bool chained = false, cb_one_launch = false;
  // the call (RenderCall, wbx_ctx.h)
  bool callback_plan = false;   // the caller handed the sequencer's arguments in: the block may run as one launch
  int master_format = 0;        // 0 planar fp32, else WBX_OUT_*
  bool mix_on_main = true;      // the mix runs on the main stream (not the alternate one)
  // the context's state
  bool dist = false;            // a multi-GPU exchange is attached
  bool init = false;            // the sum continues a running master (wbx_set_master_init, chain mode's received sum)
  bool target_set = false, target_on_host = false;   // the master goes to a caller's buffer / ... which is pinned host memory
  bool cb_no_spread = false;    // a spread launch gave up before: "the last workgroup adds" from then on
  uint32_t n_cus = 0;
};

struct RenderIssue {
  bool sum_beside = false;      // the sum runs on the sum stream, beside the next mix
  bool fused = false;           // the mix workgroup clamps and stores the master itself: no sum launch
  bool timed = false;           // the kernel timer's events ride on this render
  bool one_launch = false;      // sequencer + mix + sum as ONE launch (wbx_callback.h)
  bool by_kernel_event = false; // the sum stream waits for the mix kernel's own stop event, mix_done is recorded over there
  bool spread = false;          // every workgroup of the one launch adds a share of the master
  uint64_t stage_bytes = 0;     // > 0: the master leaves through a device staging buffer and one copy of this many bytes
};

// The spread sum's ticket barrier needs every workgroup of the grid resident at once: at most one per CU the process may use.
// A CU mask (HSA_CU_MASK / ROC_GLOBAL_CU_MASK) takes CUs away without the attribute saying so: no spreading then.  (A device
// shared with another process can still hold workgroups back; the barrier's wait is bounded, a give-up is reported and the
// block is mixed again through three launches — wbx_engine_process — and the context stops spreading.)
// `n_cus`, `cu_mask`: the device's CU count and CtxKnobs::cu_mask, as wbx_create found them.
inline uint32_t callback_spread_limit(uint32_t n_cus, bool cu_mask) { return cu_mask ? 0u : (n_cus < 256u ? n_cus : 256u); }

inline RenderIssue choose_issue(const CtxKnobs& k, const IssueFacts& f) {
  RenderIssue r;
  // short renders (the one-block callback path above all) keep everything on the main stream: the cross-stream
  // hand-overs cost more than the few microseconds of overlap they could buy
  r.sum_beside = k.sum_overlap && f.K >= kOverlapMinBlocks;
  // A short render of a session that is one group (the callback configuration up to 64 tracks; no sub-buses, planar fp32
  // master, nothing to continue): the mix workgroup clamps and stores the master itself — the sum kernel is not launched
  r.fused = f.K < kOverlapMinBlocks && f.n_groups == 1u && f.n_buses == 0u && f.tiles == 1u && !f.master_format && !f.dist && !f.init &&
            !f.chained;
  // the kernel timer is for batch renders; the one-block callback path skips its three event records
  r.timed = k.profiling && f.K > 1u;
  r.one_launch = f.callback_plan && f.n_groups != 0u && f.cb_one_launch;
  // (round 6) When the kernel carries the timer's stop event and its sum runs on the sum stream, THAT event is what the sum
  // stream waits for, and mix_done — what later plans wait for — is recorded over there: no marker packet behind the mix on
  // its own stream, where the next mix queues (every packet between two mixes is a round trip of the command processor to
  // the queue in host memory, behind whatever the copy engine is posting; what the marker cost: EXPERIMENTS.md, round 6).
  r.by_kernel_event = f.n_groups != 0u && !r.one_launch && r.timed && !f.dist && !k.mix_alternate && f.mix_on_main && r.sum_beside;
  // A master bound for pinned host memory leaves a batch render through a device staging buffer and the copy engine.  Stored
  // by the sum kernel itself, its megabytes of posted writes fill the GPU's upstream queue in a few microseconds and drain at
  // the PCIe rate; the command processor's own reads of host memory (the next dispatch packet, its signals) wait behind
  // them, and the next mix started only when the sum had ended — 0.15 ms per 2048-block render.  (One-block callbacks keep
  // the direct stores: 4 KB, and no second operation in the latency path.  Packed 24-bit too: its writer leaves part of
  // the target untouched, which a whole-buffer copy would not.)
  if (r.sum_beside && !f.dist && f.target_set && f.target_on_host && f.master_format != WBX_OUT_I24) {
    // (from 4 MB: below, the copy's fixed cost on the sum stream outweighs the hold-up — a 256-track session rendering 256
    //  blocks at a time lost a quarter of its rate to it, and gains a quarter at 2048)
    const uint64_t bytes = (uint64_t)f.K * f.block_frames * f.channels * (f.master_format == WBX_OUT_I16 ? 2u : 4u);
    if (bytes >= (4u << 20)) r.stage_bytes = bytes;
  }
  // every workgroup adds a share of the master when the whole grid is resident at once (at most one workgroup per CU: two
  // fit)
  r.spread = r.one_launch && !r.fused && !f.cb_no_spread && f.n_groups <= callback_spread_limit(f.n_cus, k.cu_mask);
  return r;
}

// ---- how a render is planned ------------------------------------------------------------------------------------------
// Which sequencer launch a render takes, where it runs, where its transport table lives, who zeroes its counters, how much it
// reserves and whether the pre-render launch is left out: one pure function from (knobs, facts) to a RenderPlan, called once by
// render_locked (wbx_engine.hip) behind render_shape and in front of everything that is sized, ordered or launched for the
// plan.  tests/test_host_logic.py holds it against the rules written out again.

// Templates a sequencer lane reserves at a time (PlanArgs::tmpl_reserve; every track may strand part of a reservation) when it
// walks all K blocks of its track, and when the sequencer is cut along the time axis (a lane plans seg_len blocks, not K: a
// smaller reservation strands less)
inline uint32_t template_reserve(uint32_t K) { return K >= 64u ? 32u : K >= 8u ? 8u : 1u; }
constexpr uint32_t kSegmentTemplateReserve = 8u;

struct PlanFacts {
  uint32_t K = 1, N = 0;        // blocks and tracks of the render
  bool playing = false;         // the transport runs
  bool callback = false;        // a process block (the one block of wbx_engine_process)
  bool any_slow_clip = false;   // HostSession::any_slow_clip
  bool cut = false;             // some track holds more than one clip (HostSession::cut_tracks)
  bool table_flags = false;     // the uploaded clip table still holds a set internal_state_changed flag
  bool seg_broken = false;      // a segmented plan failed before (wbx_ctx::seg_broken)
  uint32_t masked_rows = 0;     // the render's RenderShape: masked_rows ...
  bool cb_one_launch = false;   // ... and cb_one_launch
  bool counters_zero = false;   // the plan buffer's four counters are zero already
};

struct RenderPlan {
  enum Sequencer : uint8_t { PLAIN, SEGMENTS, NONE };   // plan_kernel; plan_seg_kernel; none: the one launch plans for itself
  enum Zeroing : uint8_t { NOBODY, TIMES_COPY, MEMSET };
  uint32_t seg_len = 0;         // blocks per segment when the sequencer is cut along the time axis, 0: one lane per track
  uint32_t n_segs = 1;          // segments per track
  bool beside = false;          // the plan runs on the plan stream, beside the previous mix
  bool device_times = false;    // the transport table goes to device memory (PlanArgs::times), copied in front of the plan
  Zeroing zeroing = NOBODY;     // who clears the plan's four counters
  bool skip_pre_render = false; // the pre-render launch is left out (expecting an empty queue)
  Sequencer sequencer = PLAIN;
  uint32_t tmpl_reserve = 1;    // PlanArgs::tmpl_reserve
  bool static_tmpl = false;     // track t owns templates 2t, 2t + 1 (PlanBuf::static_tmpl)
  bool double_rows = false;     // room for both versions of every pre-render row
  bool pool_slack = false;      // ... and of every pool chunk (ensure_pool_slack)
};

// seg_len — blocks per segment when the sequencer of this render is cut along the time axis (wbx_seq.h: plan_segment), 0 = one
// lane per track walks all K blocks.  Taken by batch renders of sessions with tracks cut into clips — a chain of dependent
// look-ups per clip boundary and lane: c3 cut into 5.3-block clips planned 2048 blocks in 5.4 ms (4.4 ms for 128-frame blocks,
// in front of a 2.6 ms mix) — while the transport runs and no clip carries a set internal_state_changed flag (the sequencer
// clears those in passing, track.cpp:373,392,418: the run-up of one lane and the real walk of another would race for them).
// About 16 k lanes: segments of K * N / 24576 blocks rounded up to a power of two, at least 32 (measured, profiles/
// r04_ab_seglen.txt: 256 tracks best at 32-64 blocks — 16 and 128 are 9-15 % slower —, 4096 tracks x 2048 short blocks at 512).
// WBX_PLAN_SEG=0: off; =<n>: segments of n blocks (A/B aid, tests).
inline RenderPlan choose_plan(const EngineKnobs& ek, const CtxKnobs& ck, const ShapeKnobs& sk, const PlanFacts& f) {
  RenderPlan r;
  const uint32_t K = f.K;
  if (ek.plan_seg != 0 && f.playing && !f.table_flags && !f.callback && f.N != 0u && !f.seg_broken) {
    if (ek.plan_seg > 0) {
      r.seg_len = (uint32_t)ek.plan_seg;
    } else if (f.cut && K >= 128u) {
      // (also where the one-lane walk would hide behind the previous mix — c3 / 16-bit sessions cut into 5.3- or 20-block clips
      //  at 512 frames: the segment lanes are done early, the next mix starts 0.06 instead of 0.15 ms behind its predecessor,
      //  steps 0-3 % shorter, never longer: profiles/r04_ab_planseg.txt)
      r.seg_len = 32u;
      while ((uint64_t)(K / r.seg_len) * f.N > 24576u && r.seg_len < K) r.seg_len *= 2u;
    }
    if (r.seg_len >= K) r.seg_len = 0u;
  }
  const bool segmented = r.seg_len != 0u;
  r.n_segs = segmented ? (K + r.seg_len - 1u) / r.seg_len : 1u;
  r.beside = ck.overlap && K >= kOverlapMinBlocks;
  // Batch render of a session whose tracks are single clips (a steady run per track, a handful of look-ups): the transport
  // records live in device memory and the sequencer takes the register-capped instance — nothing in LDS, a wave no larger
  // than a mix wave, so it runs BESIDE the previous mix instead of in the drain at its end.  Sessions cut into clips
  // search the records all the time: theirs stay in LDS (device-memory latency tripled their plan) with the roomy instance.
  // (cut sessions keep the LDS table.  Measured again in round 4, with the run end estimated instead of searched: plan of c3
  //  cut into 5.3-block clips 5.4 ms from LDS, 10.9 ms from device memory, 4 / 2 / 1 tracks per wave 12-25 ms: every record
  //  look-up at a clip boundary is a memory round trip for its lane)
  r.device_times = segmented || (r.beside && !(f.cut || sk.force_cut));
  // the plan's four counters start from zero: cleared by the kernel that brings the transport table in front of the plan when
  // there is one, else by a memset — a 16-byte fill is a launch of its own, ~50 us beside a running mix, at the head of the
  // chain fill -> table -> plan -> pre-render that a short render's mix waits for
  r.zeroing = f.counters_zero ? RenderPlan::NOBODY : r.device_times ? RenderPlan::TIMES_COPY : RenderPlan::MEMSET;
  // The one-block callback of a session whose clip boundaries stay in the hot loop: the pre-render queue is empty
  // unless a block holds three or more stream calls or overlapping ones.  Leave the launch out; wbx_engine_process
  // looks at the queue counter afterwards and repeats pre-render + mix for the (rare) block that needed it.
  // (sessions whose boundary blocks do go through the pre-render pass take the same bet when the block can be one launch:
  //  a steady block — nearly all — wins two launches, a boundary block pays the repeat)
  r.skip_pre_render = f.callback && !f.any_slow_clip && (f.masked_rows != 0u || f.cb_one_launch);
  // ... and then sequencer, mix and sum are ONE launch (wbx_callback.h): every mix workgroup plans its own tracks first, the
  // last one to finish sums the block and tells the host
  r.sequencer = segmented ? RenderPlan::SEGMENTS : f.cb_one_launch ? RenderPlan::NONE : RenderPlan::PLAIN;
  // (one launch: track t owns templates 2t, 2t + 1 — no allocation round trip in the latency chain)
  r.static_tmpl = f.cb_one_launch;
  r.tmpl_reserve = f.cb_one_launch ? 0u : segmented ? kSegmentTemplateReserve : template_reserve(K);
  // (segments: a track whose seam missed is planned again from there, and what its replaced segments queued / took from the
  //  pool / reserved stays allocated and unused — room for both versions of every row, so that a miss on a session that leans
  //  on the pre-render pass cannot turn into a capacity error)
  r.double_rows = r.pool_slack = segmented;
  return r;
}

}  // namespace wbx
