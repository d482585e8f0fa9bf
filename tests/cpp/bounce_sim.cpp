// bounce_sim.cpp — TEST HARNESS: the host code of wbx_engine_bounce (wbx_host.h, HostSession::bounce_locked) without a device.
//
// Compiles the product's own HostSession and drives bounce_locked the way wbx_engine.hip does, with a device stand-in that
// only keeps a log: which destination clips were allocated, which passes were rendered (each advancing the transport through
// advance_transport_locked, as render_locked does), what was published and what was released.  tests/test_bounce_model.py
// holds the output to tests/bounce_util.py's BounceModel and to the oracle's beat_to_samples, doubles compared as bit patterns.
//
//   g++ -std=c++20 -O2 -ffp-contract=off bounce_sim.cpp -o bounce_sim
//
// Script lines:  frames F | rate R | max_blocks M | tracks N | buses N | bpm X | playhead X | play | stop | block |
//                recording 0|1 | redirected 0|1 | fail_alloc I (-1: none) |
//                bounce MIN_BITS MAX_BITS N_SRC (KIND INDEX TAP)...      (the two times as 16 hex digits)
// Output per line: "status S"; a bounce adds
//   "bounce S N_FRAMES N_PASSES (FIRST K)... | N_PUB (KIND INDEX TAP ID)... | N_REL I..."   and every line ends with
//   "transport PLAYHEAD_BITS START_BITS SAMPLE_POSITION_BITS PLAYING EDITS"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wbx.h"
#include "../../whitebox_amd/csrc/wbx_host.h"

using namespace wbx;

namespace {

uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}
double from_bits(uint64_t u) {
  double v;
  std::memcpy(&v, &u, 8);
  return v;
}

struct SimDev {
  HostSession& hs;
  uint32_t F;
  int fail_alloc_at;
  std::vector<uint64_t> allocated;                    // frames of destination i
  std::vector<std::pair<uint32_t, uint32_t>> passes;  // (first block, blocks)
  std::vector<uint32_t> released, published;
  uint32_t next_id = 100;
  wbx_status alloc(uint32_t i, uint64_t frames) {
    if ((int)i == fail_alloc_at) return WBX_ERR_OOM;
    if (allocated.size() != i) return WBX_ERR_FAILED;   // in order, once each
    allocated.push_back(frames);
    return WBX_OK;
  }
  wbx_status pass(uint32_t first, uint32_t k) {
    if (!hs.playing.load()) return WBX_ERR_FAILED;      // the passes run between play() and stop()
    passes.emplace_back(first, k);
    hs.advance_transport_locked(k, F, hs.beat_duration.load());
    return WBX_OK;
  }
  uint32_t publish(uint32_t i) {
    published.push_back(i);
    return next_id + i;
  }
  void release(uint32_t i) { released.push_back(i); }
};

}  // namespace

int main() {
  HostSession hs;
  uint32_t F = 512, max_blocks = 8;
  bool redirected = false;
  int fail_alloc = -1;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    int st = WBX_OK;
    if (op == "frames") {
      in >> F;
    } else if (op == "rate") {
      in >> hs.dst_rate;
    } else if (op == "max_blocks") {
      in >> max_blocks;
    } else if (op == "tracks") {
      int n;
      in >> n;
      LockGuard g(hs.editor_lock);
      for (int i = 0; i < n; i++) hs.add_track_locked();
    } else if (op == "buses") {
      in >> hs.n_buses;
    } else if (op == "bpm") {
      double b;
      in >> b;
      hs.set_bpm(b);
    } else if (op == "playhead") {
      double b;
      in >> b;
      LockGuard g(hs.editor_lock);
      hs.set_playhead_position_locked(b);
      hs.note_edit_locked();
    } else if (op == "play") {
      LockGuard g(hs.editor_lock);
      hs.play_locked();
      hs.note_edit_locked();
    } else if (op == "stop") {
      LockGuard g(hs.editor_lock);
      hs.stop_locked();
      hs.note_edit_locked();
    } else if (op == "block") {
      LockGuard g(hs.editor_lock);
      hs.advance_transport_locked(1, F, hs.beat_duration.load());
    } else if (op == "recording") {
      int r;
      in >> r;
      hs.recording = r != 0;
    } else if (op == "redirected") {
      int r;
      in >> r;
      redirected = r != 0;
    } else if (op == "fail_alloc") {
      in >> fail_alloc;
    } else if (op == "bounce") {
      uint64_t lo, hi;
      uint32_t n;
      in >> std::hex >> lo >> hi >> std::dec >> n;
      std::vector<wbx_bounce_source> src(n);
      for (auto& s : src) {
        in >> s.kind >> s.index >> s.tap;
        s._pad = 0;
      }
      std::vector<uint32_t> ids(n + 1, 0xDEADu);
      uint64_t frames = 0;
      const char* why = "";
      SimDev dev{hs, F, fail_alloc};
      {
        LockGuard g(hs.editor_lock);
        st = hs.bounce_locked(from_bits(lo), from_bits(hi), n ? src.data() : nullptr, n, F, max_blocks, redirected, dev, ids.data(),
                              &frames, &why);
      }
      std::printf("bounce %d %" PRIu64 " %zu", st, frames, dev.passes.size());
      for (auto& p : dev.passes) std::printf(" %u %u", p.first, p.second);
      std::printf(" | %zu", dev.published.size());
      for (uint32_t i : dev.published) std::printf(" %d %u %d %u", src[i].kind, src[i].index, src[i].tap, ids[i] - dev.next_id);
      std::printf(" | %zu", dev.released.size());
      for (uint32_t i : dev.released) std::printf(" %u", i);
      for (uint64_t f : dev.allocated)
        if (f != frames && st == WBX_OK) st = WBX_ERR_FAILED;   // every destination has n_frames frames
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
    std::printf("status %d\n", st);
    std::printf("transport %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %" PRIu64 "\n", bits(hs.playhead), bits(hs.playhead_start),
                bits(hs.sample_position), hs.playing.load() ? 1 : 0, hs.edit_seq);
  }
  return 0;
}
