// wbx_splice.h — the host half of wbx_clip_splice (wbx.h "Splicing clips"): the refusals of a part list and the tile table
// the kernel walks.  Plain C++ (no HIP, no wbx_ctx): the library calls it once per splice, wbx_splice_plan exports it for
// ctypes tests, and tests/cpp/splice_plan_main.cpp compiles it with g++ alone.
//
// The output is cut into tiles of kSpliceTile frames, a wave's share.  tile_off[t] .. tile_off[t + 1] index tile_parts[],
// the indices of the parts that touch tile t, ascending — which is the list's order, the order of the additions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/wbx.h"

namespace wbx {

constexpr uint32_t kSpliceTile = 512;
constexpr uint32_t kSpliceMaxParts = 65536;
constexpr uint64_t kSpliceMaxEntries = 1ull << 24;
constexpr uint64_t kSpliceMaxFrames = (1ull << 31) - 16;   // n_frames stays below it, like every pool clip's length

struct SplicePlan {
  uint32_t rate = 0;                  // the sources' common sample rate
  uint64_t n_tiles = 0, n_entries = 0;
  std::vector<uint32_t> tile_off;     // [n_tiles + 1]
  std::vector<uint32_t> tile_parts;   // [n_entries]
};

// channels a part yields (0: the mode does not fit a source of `src_channels`, or is unknown: *known says which)
inline uint32_t splice_mode_channels(int32_t mode, uint32_t src_channels, bool* known) {
  uint32_t need = 0, out = 0;
  *known = true;
  switch (mode) {
    case WBX_CH_KEEP: out = src_channels; break;
    case WBX_CH_SWAP: need = 2, out = 2; break;
    case WBX_CH_LEFT:
    case WBX_CH_RIGHT:
    case WBX_CH_MONO_MIX: need = 2, out = 1; break;
    case WBX_CH_DUAL_MONO: need = 1, out = 2; break;
    default: *known = false; return 0;
  }
  return need && need != src_channels ? 0 : out;
}

// The refusals of wbx.h "Splicing clips" that need no context (every one but dst_clip == a source): the call's own
// arguments first, then the parts in list order, the first refusal found wins.  source_of(id) gives the wbx_splice_source
// of a clip, or nullptr where there is no such clip.  On WBX_OK *rate is the common rate.
template <class SourceOf>
inline wbx_status splice_check(uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts,
                               SourceOf source_of, uint32_t* rate, const char** why) {
  if (!parts || n_parts == 0) return *why = "clip splice: no parts", WBX_ERR_INVALID;
  if (n_frames == 0) return *why = "clip splice: no frames", WBX_ERR_INVALID;
  if (n_frames >= kSpliceMaxFrames) return *why = "clip splice: the result would have 2^31 - 16 frames or more", WBX_ERR_INVALID;
  if (channels < 1 || channels > 2) return *why = "clip splice: channels (1 or 2)", WBX_ERR_INVALID;
  if (n_parts > kSpliceMaxParts) return *why = "clip splice: more than 65536 parts", WBX_ERR_UNSUPPORTED;
  uint32_t common = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const wbx_splice_part& p = parts[i];
    const wbx_splice_source* s = source_of(p.src_clip);
    if (!s || s->channels == 0) return *why = "clip splice: unknown source clip", WBX_ERR_INVALID;
    if (p.n_frames == 0) return *why = "clip splice: a part with no frames", WBX_ERR_INVALID;
    if (p.first_frame > s->frames || p.n_frames > s->frames - p.first_frame) return *why = "clip splice: a part's range ends past its clip", WBX_ERR_INVALID;
    if (p.at > n_frames || p.n_frames > n_frames - p.at) return *why = "clip splice: a part ends past the result", WBX_ERR_INVALID;
    if (p.flags & ~(uint32_t)WBX_EDIT_REVERSE) return *why = "clip splice: unknown flags", WBX_ERR_INVALID;
    if (p.fade_in_shape < WBX_FADE_LINEAR || p.fade_in_shape > WBX_FADE_SMOOTH || p.fade_out_shape < WBX_FADE_LINEAR ||
        p.fade_out_shape > WBX_FADE_SMOOTH)
      return *why = "clip splice: unknown fade shape", WBX_ERR_INVALID;
    if (p.fade_in > p.n_frames || p.fade_out > p.n_frames) return *why = "clip splice: a fade longer than its part", WBX_ERR_INVALID;
    bool known = false;
    const uint32_t fits = s->channels <= 2 ? s->channels : 2u;   // (a wider source is refused below, whatever the mode)
    const uint32_t out = splice_mode_channels(p.channel_mode, fits, &known);
    if (!known) return *why = "clip splice: unknown channel mode", WBX_ERR_INVALID;
    if (s->format != (int32_t)WBX_FMT_F32) return *why = "clip splice: a source's storage format is not F32", WBX_ERR_UNSUPPORTED;
    if (s->channels > 2) return *why = "clip splice: source channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
    if (out == 0) return *why = "clip splice: a channel mode does not fit its source's channel count", WBX_ERR_INVALID;
    if (out != channels) return *why = "clip splice: a part's channel mode does not yield the result's channel count", WBX_ERR_INVALID;
    if (i == 0) common = s->sample_rate;
    else if (s->sample_rate != common) return *why = "clip splice: the sources' sample rates differ (convert first: wbx_clip_resample)", WBX_ERR_INVALID;
  }
  *rate = common;
  return WBX_OK;
}

inline uint64_t splice_tiles(uint64_t n_frames) { return (n_frames + kSpliceTile - 1) / kSpliceTile; }

// entries of the table of a CHECKED part list (at + n_frames <= the result's length < 2^31): at most 65536 * 2^22
inline uint64_t splice_entries(const wbx_splice_part* parts, uint32_t n_parts) {
  uint64_t n = 0;
  for (uint32_t i = 0; i < n_parts; i++) n += (parts[i].at + parts[i].n_frames - 1) / kSpliceTile - parts[i].at / kSpliceTile + 1;
  return n;
}

// the table of a checked part list whose entries fit: a counting sort by tile, stable in the part index
inline void splice_table(uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts, uint32_t* tile_off, uint32_t* tile_parts) {
  const uint64_t n_tiles = splice_tiles(n_frames);
  for (uint64_t t = 0; t <= n_tiles; t++) tile_off[t] = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const uint64_t t0 = parts[i].at / kSpliceTile, t1 = (parts[i].at + parts[i].n_frames - 1) / kSpliceTile;
    for (uint64_t t = t0; t <= t1; t++) tile_off[t + 1]++;
  }
  for (uint64_t t = 0; t < n_tiles; t++) tile_off[t + 1] += tile_off[t];
  // tile_off[t] now is tile t's first entry; fill through a cursor kept in place and shift back afterwards
  for (uint32_t i = 0; i < n_parts; i++) {
    const uint64_t t0 = parts[i].at / kSpliceTile, t1 = (parts[i].at + parts[i].n_frames - 1) / kSpliceTile;
    for (uint64_t t = t0; t <= t1; t++) tile_parts[tile_off[t]++] = i;
  }
  for (uint64_t t = n_tiles; t > 0; t--) tile_off[t] = tile_off[t - 1];
  tile_off[0] = 0;
}

// tiles and entries of the table of a checked part list, or the refusal of one that would be too long: the one home of
// that bound (the library, layer 2 and wbx_splice_plan all come through here)
inline wbx_status splice_table_size(uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts, uint64_t* n_tiles,
                                    uint64_t* n_entries, const char** why) {
  *n_tiles = splice_tiles(n_frames);
  *n_entries = splice_entries(parts, n_parts);
  if (*n_entries > kSpliceMaxEntries) return *why = "clip splice: the tile table would have more than 2^24 entries", WBX_ERR_UNSUPPORTED;
  return WBX_OK;
}

// the table of a checked part list into *plan (layer 2 checks under the editor lock and builds the table without it)
inline wbx_status splice_plan_table(uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts, SplicePlan* plan,
                                    const char** why) {
  const wbx_status st = splice_table_size(n_frames, parts, n_parts, &plan->n_tiles, &plan->n_entries, why);
  if (st != WBX_OK) return st;
  plan->tile_off.resize((size_t)plan->n_tiles + 1);
  plan->tile_parts.resize((size_t)plan->n_entries);
  splice_table(n_frames, parts, n_parts, plan->tile_off.data(), plan->tile_parts.data());
  return WBX_OK;
}

template <class SourceOf>
inline wbx_status splice_plan(uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts,
                              SourceOf source_of, SplicePlan* plan, const char** why) {
  const wbx_status st = splice_check(channels, n_frames, parts, n_parts, source_of, &plan->rate, why);
  return st == WBX_OK ? splice_plan_table(n_frames, parts, n_parts, plan, why) : st;
}

}  // namespace wbx
