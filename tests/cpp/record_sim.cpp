// record_sim.cpp — TEST HARNESS: the recording half of the host session (wbx_host.h) without a device.
//
// Compiles the product's own HostSession and drives it the way wbx_engine.hip does — record / stop_record / play / stop /
// set_track_input / process, with the transport advance and the recorder tap of every block — from a script on stdin, and
// prints what stop_record hands to add_audio_clip plus which input block each F frames of every take came from.
// tests/test_record_model.py holds the output to tests/record_model.py (the reference's semantics in plain Python), with
// record_min_time / record_max_time compared as bit patterns.  Frames themselves exist only on the device.
//
//   g++ -std=c++20 -O2 -ffp-contract=off record_sim.cpp -o record_sim
//
// Script lines (one call each):  tracks N | inputs N | bpm X | playhead X | input SLOT TYPE INDEX ARMED | arm SLOT ARMED |
//                                record | stop_record | play | stop | block I (I < 0: no input) | delete SLOT | clear_all
// Before the calls, optionally:  chunk N | capacity N   take storage in chunks of N frames, at most N of them per take.  The
//                                device half decides which block is lost (rec_capture_locked: the block's last frame lies in a
//                                chunk the take does not have); the harness restates that one comparison and hands the
//                                verdict to the host session as the device half does (take_status_locked), so what is checked
//                                here is what the HOST code makes of it: status latched, frames and record_max_time advancing,
//                                stop_record's WBX_ERR_OVERFLOW with the clip still made.
// Output: one "status S" line per call; for every clip stop_record makes:
//   clip TRACK MIN_BITS MAX_BITS CH0 CHANNELS STATUS N_BLOCKS B0 B1 ...   (block -1: silence)
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

struct RecordSim {
  HostSession hs;
  uint32_t F = 512;
  uint64_t chunk = 65536, capacity = ~0ull;   // "chunk" / "capacity" lines
  // what lives in HBM in the product: which input block each block of every take holds (-1: silence)
  std::vector<std::vector<int64_t>> take_blocks;

  int add_tracks(int n) {
    LockGuard g(hs.editor_lock);
    for (int i = 0; i < n; i++) hs.add_track_locked();
    return WBX_OK;
  }
  // wbx_engine_stop_record: stop_record_locked, one F32 sample and add_audio_clip per take that has frames
  int stop_record() {
    LockGuard g(hs.editor_lock);
    if (!hs.recording) return WBX_OK;
    std::vector<FinishedTake> fin = hs.stop_record_locked();
    int st = WBX_OK;
    for (const FinishedTake& f : fin) {
      if (f.frames == 0) continue;
      const int32_t t = hs.track_index(f.track);
      if (t < 0) continue;
      const uint32_t id = (uint32_t)hs.samples.size();
      hs.samples.push_back(SampleMeta{WBX_FMT_F32, f.channels, hs.dst_rate, f.frames, true});
      hs.add_audio_clip_locked((uint32_t)t, f.min_time, f.max_time, 0.0, id, 1.0, 1.0f);
      const Take& tk = hs.takes[f.take];
      std::printf("clip %d %016" PRIx64 " %016" PRIx64 " %u %u %u %zu", t, bits(f.min_time), bits(f.max_time), tk.ch0, tk.channels,
                  f.status, take_blocks[f.take].size());
      for (int64_t b : take_blocks[f.take]) std::printf(" %" PRId64, b);
      std::printf("\n");
      if (f.status & REC_OVERFLOW) st = WBX_ERR_OVERFLOW;
    }
    hs.takes.clear();
    take_blocks.clear();
    return st;
  }
  int record() {
    LockGuard g(hs.editor_lock);
    if (hs.recording && hs.playing.load()) return WBX_OK;
    if (!hs.record_inputs_valid()) return WBX_ERR_INVALID;
    hs.record_locked();
    take_blocks.assign(hs.takes.size(), {});
    return WBX_OK;
  }
  // wbx_engine_process: render_locked's transport advance, then the recorder tap (rec_capture_locked)
  int block(int64_t input) {
    LockGuard g(hs.editor_lock);
    hs.advance_transport_locked(1, F, hs.beat_duration.load());
    if (!hs.capture_due()) return WBX_OK;
    const uint64_t at = hs.capture_block_locked(F, input < 0);
    const bool lost = (at + F - 1) / chunk >= capacity;
    for (size_t k = 0; k < take_blocks.size(); k++) {
      auto& tb = take_blocks[k];
      if (tb.size() * F != at) return WBX_ERR_FAILED;   // every take is written at the frame it has reached
      if (lost && hs.takes[k].track) hs.take_status_locked(k, REC_OVERFLOW);
      tb.push_back(lost ? -1 : input);
    }
    return WBX_OK;
  }
};

}  // namespace

int main() {
  RecordSim sim;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    int st = WBX_OK;
    HostSession& hs = sim.hs;
    if (op == "frames") {
      in >> sim.F;
      continue;
    } else if (op == "rate") {
      in >> hs.dst_rate;
      continue;
    } else if (op == "chunk") {
      in >> sim.chunk;
      continue;
    } else if (op == "capacity") {
      in >> sim.capacity;
      continue;
    } else if (op == "tracks") {
      int n;
      in >> n;
      st = sim.add_tracks(n);
    } else if (op == "inputs") {
      LockGuard g(hs.editor_lock);
      in >> hs.input_channels;
    } else if (op == "bpm") {
      double b;
      in >> b;
      hs.set_bpm(b);
    } else if (op == "playhead") {
      double b;
      in >> b;
      LockGuard g(hs.editor_lock);
      hs.set_playhead_position_locked(b);
    } else if (op == "input" || op == "arm") {
      uint32_t slot, type = 0, index = 0, armed;
      in >> slot;
      if (op == "input") in >> type >> index;
      in >> armed;
      LockGuard g(hs.editor_lock);
      if (type == INPUT_MIDI) {
        st = WBX_ERR_UNSUPPORTED;
      } else if (!hs.valid_track(slot)) {
        st = WBX_ERR_INVALID;
      } else {
        if (op == "arm") type = hs.tracks[slot]->rec.in_type, index = hs.tracks[slot]->rec.in_index;
        hs.set_track_input_locked(slot, type, index, armed != 0);
      }
    } else if (op == "record") {
      st = sim.record();
    } else if (op == "stop_record") {
      st = sim.stop_record();
    } else if (op == "play") {
      LockGuard g(hs.editor_lock);
      hs.play_locked();
    } else if (op == "stop") {
      sim.stop_record();
      LockGuard g(hs.editor_lock);
      hs.stop_locked();
    } else if (op == "block") {
      int64_t b;
      in >> b;
      st = sim.block(b);
    } else if (op == "delete" || op == "clear_all") {
      LockGuard g(hs.editor_lock);
      std::vector<uint32_t> order;
      uint32_t slot = ~0u;
      if (op == "delete") in >> slot;
      if (op == "delete" && !hs.valid_track(slot)) {
        st = WBX_ERR_INVALID;
      } else {
        if (op == "delete")
          for (uint32_t i = 0; i < hs.n_tracks(); i++)
            if (i != slot) order.push_back(i);
        hs.permute_tracks_locked(order);
      }
    } else {
      std::fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
    std::printf("status %d\n", st);
  }
  return 0;
}
