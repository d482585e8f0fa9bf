// wbx_knobs.h — every environment switch the library reads, and the only place that calls getenv.  Plain C++ (no HIP, no
// wbx_ctx): tests/cpp/host_sim.cpp compiles it with g++.
//
// Each struct is filled ONCE, by from_env() where its owner is created (wbx_create, wbx_engine_create; a test sets the
// variable and creates a new context): no render, upload or audio-callback path calls getenv, and what a context decides at
// plan time cannot disagree with what it launches.  Facts a context LEARNS while it runs (cb_no_spread, chain_broken,
// seg_broken) are state, not switches: they stay in wbx_ctx.  DESIGN.md holds the table of all switches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>

namespace wbx {

namespace env {
inline bool is(const char* name, char what) {   // set, and its first character is `what`
  const char* v = std::getenv(name);
  return v && v[0] == what;
}
inline bool present(const char* name) { return std::getenv(name) != nullptr; }
}  // namespace env

// The switches that enter the choice of a render's mix instance (wbx_shape.h: choose_shape)
struct ShapeKnobs {
  bool ragged_off = false;        // WBX_RAGGED=0: blocks between the instances' shapes take the general instance
  bool cb_any_off = false;        // WBX_CB_ANY=0: the one-launch callback only for blocks that are exactly one 256-lane workgroup
  bool masked_rows_off = false;   // WBX_MASKED_ROWS=0: every clip boundary through the pre-render pass
  bool chain_off = false;         // WBX_CHAIN=0: long renders walk whole member lists instead of chaining 128-track pieces
  bool no_lean16 = false;         // WBX_NO_LEAN16: sessions of 16-bit PCM only through family 1
  bool no_fam3 = false;           // WBX_NO_FAM3: resampled-integer sessions through family 1
  bool no_cl2 = false;            // WBX_NO_CL2: never both channels of a frame in one lane
  bool callback_unfused = false;  // WBX_CALLBACK_FUSED=0: the one-block callback as three launches (results are identical)
  bool force_cut = false;         // WBX_FORCE_CUT=1: an uncut session through the instances a session cut into clips takes
  bool force_g = false;           // WBX_FORCE_G: always the everything family
  int packed_x = -1;              // WBX_PACKED_X=0|1: the packed masked-row instances off / on for every shape (-1: the library's choice)
  int mix_variant = 0;            // WBX_MIX_VARIANT=10*U+W (>= 1000: both channels per lane) forces a kernel variant (results
                                  // are identical); 0 = chosen per render
  int cb_u = 0;                   // WBX_CB_U=2|4|8: rows per pipeline batch of the lean callback instance
  uint32_t exact_min_blocks = 1024;   // renders of at least this many workgroup columns walk whole member lists when the
                                      // library picks the grouping (WBX_EXACT_MIN_BLOCKS; 0 = never)

  static ShapeKnobs from_env() {
    ShapeKnobs k;
    k.ragged_off = env::is("WBX_RAGGED", '0');
    k.cb_any_off = env::is("WBX_CB_ANY", '0');
    k.masked_rows_off = env::is("WBX_MASKED_ROWS", '0');
    k.chain_off = env::is("WBX_CHAIN", '0');
    k.no_lean16 = env::present("WBX_NO_LEAN16");
    k.no_fam3 = env::present("WBX_NO_FAM3");
    k.no_cl2 = env::present("WBX_NO_CL2");
    k.callback_unfused = env::is("WBX_CALLBACK_FUSED", '0');
    k.force_cut = env::is("WBX_FORCE_CUT", '1');
    if (const char* v = std::getenv("WBX_FORCE_G")) k.force_g = std::atoi(v) != 0;
    if (const char* v = std::getenv("WBX_PACKED_X")) k.packed_x = std::atoi(v) != 0 ? 1 : 0;
    if (const char* v = std::getenv("WBX_MIX_VARIANT")) k.mix_variant = std::atoi(v);
    if (const char* v = std::getenv("WBX_CB_U")) k.cb_u = std::atoi(v);
    if (const char* v = std::getenv("WBX_EXACT_MIN_BLOCKS")) k.exact_min_blocks = (uint32_t)std::atoi(v);
    return k;
  }
};

// What a context consults beside the shape's switches: stream layout, diagnostics, and the switches that reach into a kernel
struct CtxKnobs {
  bool overlap = true;            // WBX_OVERLAP=0: the sequencer on the main stream instead of beside the previous mix
  bool sum_overlap = true;        // WBX_SUM_OVERLAP=0: the sum on the main stream
  bool mix_alternate = false;     // WBX_MIX_ALT=1: consecutive batch renders' mixes on alternating streams (wbx_ctx.h: alt_stream)
  bool profiling = true;          // WBX_KERNEL_TIMER=0: no HIP-event kernel timer
  uint32_t cb_spin_bound = 40000; // WBX_CB_SPIN_BOUND: polls of the spread barrier before a workgroup gives up (~50 ms; tests: 0
                                  // forces the give-up path)
  bool no_uniform = false;        // WBX_NO_UNIFORM=1: MixArgs::uniform_speed withheld (the one-ratio modes off)
  bool cb_fenced = false;         // WBX_CB_FENCED=1: release / acquire fences in the one-launch callback
  bool fast_partial_off = false;  // WBX_FAST_PARTIAL=0: every partial stream call through the clamped masked arithmetic
  bool xcd_probe_fail = false;    // WBX_XCD_PROBE_FAIL=1: the XCD layout probe counts as failed (tests take the fallback path)
  bool dbg_clock = false;         // WBX_DBG_CLOCK: per-workgroup start / end times of the mix (tools/wg_clocks.py)
  bool cb_dbg = false;            // WBX_CB_DBG: the phases of every workgroup of the one-launch callback (tools/cb_clocks.py)
  bool cu_mask = false;           // HSA_CU_MASK / ROC_GLOBAL_CU_MASK is set: CUs are taken away without the device's attribute
                                  // saying so — the callback's spread sum is off (wbx_shape.h: callback_spread_limit)

  static CtxKnobs from_env() {
    CtxKnobs k;
    k.overlap = !env::is("WBX_OVERLAP", '0');
    k.sum_overlap = !env::is("WBX_SUM_OVERLAP", '0');
    k.mix_alternate = env::is("WBX_MIX_ALT", '1');
    if (const char* v = std::getenv("WBX_KERNEL_TIMER")) k.profiling = std::atoi(v) != 0;
    if (const char* v = std::getenv("WBX_CB_SPIN_BOUND")) k.cb_spin_bound = (uint32_t)std::atoi(v);
    k.no_uniform = env::is("WBX_NO_UNIFORM", '1');
    k.cb_fenced = env::is("WBX_CB_FENCED", '1');
    k.fast_partial_off = env::is("WBX_FAST_PARTIAL", '0');
    k.xcd_probe_fail = env::is("WBX_XCD_PROBE_FAIL", '1');
    k.dbg_clock = env::present("WBX_DBG_CLOCK");
    k.cb_dbg = env::present("WBX_CB_DBG");
    for (const char* name : {"HSA_CU_MASK", "ROC_GLOBAL_CU_MASK"}) {
      const char* m = std::getenv(name);
      if (m && m[0]) k.cu_mask = true;
    }
    return k;
  }
};

// Layer 2's own (wbx_engine_create)
struct EngineKnobs {
  int plan_seg = -1;              // WBX_PLAN_SEG: 0 the segmented sequencer off, n > 0 segments of n blocks, -1 unset (A/B aid, tests)
  uint32_t plan_lanes = 0;        // WBX_PLAN_LANES=1|2|4|..|64: tracks per wave of the sequencer (0: unset, 64).  Tuning knob; measured
                                  // on c3 cut into clips of 5.3 / 20 blocks: 64, 32, 16 and 8 tracks per wave within 2 % of each other

  static EngineKnobs from_env() {
    EngineKnobs k;
    if (const char* v = std::getenv("WBX_PLAN_SEG")) k.plan_seg = std::max(0, std::atoi(v));
    if (const char* v = std::getenv("WBX_PLAN_LANES")) {
      const int n = std::atoi(v);
      if (n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 32 || n == 64) k.plan_lanes = (uint32_t)n;
    }
    return k;
  }
};

// WBX_DIST_INIT_TIMEOUT_S: seconds wbx_dist_init waits for the communicator's rendezvous (<= 0: for ever)
inline double dist_init_timeout_s() {
  const char* t = std::getenv("WBX_DIST_INIT_TIMEOUT_S");
  return t ? std::atof(t) : 60.0;
}

}  // namespace wbx
