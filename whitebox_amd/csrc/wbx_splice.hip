// wbx_splice.hip — splice_kernel: parts of resident planar F32 clips — each a wbx_clip_derive edit placed at an output frame —
// assigned and added, in list order, into ONE new planar F32 clip (wbx.h "Splicing clips"), and layer 1's calls on top of it.
//
// No reference counterpart: AudioClip::fade_start / fade_end (engine/clip.h:41-42) are read by nothing and
// Engine::reserve_track_region (engine.cpp:478-569) trims overlapping clips, never blends them.  The arithmetic is written
// out in wbx.h, planned by wbx_splice.h (host-only) and mirrored by tests/splice_model.py.  A part's value is clipfx_kernel's,
// operation for operation (one fp32 multiply by the gain, one per fade with the weight of fade_weight()); parts are joined by
// one fp32 addition each in list order; a NaN is stored as 0x7FC00000.  (wbx_clip_derive stores a part's NaN as that NaN
// already; any NaN added to anything stays a NaN, so replacing once, before the store, gives the same bits.)
//
// Lane ownership is clipfx_kernel's: a lane owns 8 consecutive OUTPUT frames of every output channel and stores them as two
// whole 16-B nontemporal words per channel; a wave owns one 512-frame tile and strides over the tiles by the grid, so one
// launch covers any length.  Per tile the wave walks the tile's entries of tile_parts[] (wbx_splice.h), ascending = list order:
//   descriptor  wave-uniform loads (the tile, hence every index, is the same in all lanes)
//   inside      a lane whose 8 frames all lie inside the part loads two 16-B words per source row through the 4-byte aligned
//               type; a reversed part loads the MIRRORED words and reverses them in registers
//   edge        a lane that straddles the part's first or last frame loads its frames one by one, each guarded
//   nothing outside [first_frame, first_frame + n) of a source is read: a part may start at frame 0 of a slab's first clip
//   fades       weights (one fp64 division per frame) only where the tile intersects the part's fade regions — wave-uniform
//   MONO_MIX    a wave-uniform branch per part (the second row is loaded only there), not an instance
// Every frame of the result is stored, one no part covers as +0.0f.  No LDS, no scratch.
#include "wbx_ctx.h"

namespace wbx {

namespace {

template <int CO>
__global__ void __launch_bounds__(256) splice_kernel(SpliceArgs a) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t step = gridDim.x * 4u;                      // (n_tiles < 2^22, step <= 2^14: tile + step does not wrap)
  for (uint32_t tile = blockIdx.x * 4u + wave; tile < a.n_tiles; tile += step) {
    const uint32_t base = tile * kSpliceTile;                // < n_frames < 2^31
    const uint32_t j0 = base + lane * 8u;                    // the lane's first output frame (<= 2^31 - 8)
    float acc[CO][8];
#pragma unroll
    for (int c = 0; c < CO; c++)
#pragma unroll
      for (int i = 0; i < 8; i++) acc[c][i] = 0.0f;
    uint32_t have = 0u;                                      // bit i: a part has covered frame j0 + i

    const uint32_t e1 = a.tile_off[tile + 1u];
    for (uint32_t e = a.tile_off[tile]; e < e1; e++) {
      const SplicePartDev& P = a.parts[a.tile_parts[e]];
      const uint32_t n = P.n, fade_in = P.fade_in, fade_out = P.fade_out, bits = P.bits;
      const float gain = P.gain;
      const bool rev = (bits & kSpliceReversed) != 0u, mix = CO == 1 && (bits & kSpliceMonoMix) != 0u;
      const uint32_t out_from = n - fade_out;                // the part's frames from here on are in its fade-out
      // the tile's frames inside the part, in the part's frame numbers [tk0, tk1): wave-uniform
      const int32_t rel = (int32_t)base - (int32_t)P.at;     // (both below 2^31)
      const uint32_t tk0 = rel > 0 ? (uint32_t)rel : 0u;
      const int64_t tend = (int64_t)rel + (int64_t)kSpliceTile;   // (64 bits: base may be 2^31 - 512; > 0, the part touches the tile)
      const uint32_t tk1 = tend < (int64_t)n ? (uint32_t)tend : n;
      const bool faded = tk0 < fade_in || (fade_out && tk1 > out_from);

      const int32_t k0 = rel + (int32_t)(lane * 8u);         // the part's frame number of output frame j0
      if (k0 >= (int32_t)n || k0 <= -8) continue;            // none of the lane's frames is in the part
      const bool full = k0 >= 0 && (uint32_t)k0 + 8u <= n;
      uint32_t in = 0xFFu;                                   // bit i: frame j0 + i is in the part
      if (!full) {
        in = 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) in |= (k0 + i >= 0 && k0 + i < (int32_t)n) ? 1u << i : 0u;
      }

      float x[2][8];                                         // the source frames of output frames j0 .. j0 + 7, in output order
#pragma unroll
      for (int r = 0; r < 2; r++) {
        if (r == 1 && CO == 1 && !mix) break;                // (wave-uniform: a mono part reads one row)
        const float* row = P.src[r];
        if (r == 1 && row == P.src[0]) {                     // (wave-uniform) DUAL_MONO, LEFT, RIGHT: one row on both channels, read once
#pragma unroll
          for (int i = 0; i < 8; i++) x[1][i] = x[0][i];
          break;
        }
        if (full) {
          const uint32_t k = (uint32_t)k0;
          const float* p = rev ? row + (n - 8u - k) : row + k;   // reversed: source frames n - 8 - k .. n - 1 - k
          const f4u lo = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p));
          const f4u hi = __builtin_nontemporal_load(reinterpret_cast<const f4u*>(p + 4));
          if (rev) {
            x[r][7] = lo.x, x[r][6] = lo.y, x[r][5] = lo.z, x[r][4] = lo.w;
            x[r][3] = hi.x, x[r][2] = hi.y, x[r][1] = hi.z, x[r][0] = hi.w;
          } else {
            x[r][0] = lo.x, x[r][1] = lo.y, x[r][2] = lo.z, x[r][3] = lo.w;
            x[r][4] = hi.x, x[r][5] = hi.y, x[r][6] = hi.z, x[r][7] = hi.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const uint32_t k = (uint32_t)(k0 + i);           // read only where bit i of `in` is set: k in [0, n)
            x[r][i] = (in >> i & 1u) ? row[rev ? n - 1u - k : k] : 0.0f;
          }
        }
      }

      float win[8], wout[8];
      if (faded) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const uint32_t k = (uint32_t)(k0 + i);
          const bool on = (in >> i & 1u) != 0u;
          win[i] = (on && k < fade_in) ? fade_weight(k, fade_in, bits & 3u) : 1.0f;
          wout[i] = (on && k >= out_from) ? fade_weight(n - 1u - k, fade_out, bits >> kSpliceShapeOutShift & 3u) : 1.0f;
        }
      }

#pragma unroll
      for (int c = 0; c < CO; c++) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          float y = x[c][i];
          if (CO == 1 && mix) y = __fmul_rn(__fadd_rn(x[0][i], x[1][i]), 0.5f);
          y = __fmul_rn(y, gain);
          if (faded) {
            const uint32_t k = (uint32_t)(k0 + i);
            const bool on = (in >> i & 1u) != 0u;
            if (on && k < fade_in) y = __fmul_rn(y, win[i]);
            if (on && k >= out_from) y = __fmul_rn(y, wout[i]);
          }
          const bool first = (have >> i & 1u) == 0u;         // the first covering part assigns, every later one adds
          if (in >> i & 1u) acc[c][i] = first ? y : __fadd_rn(acc[c][i], y);
        }
      }
      have |= in;
    }

    if (j0 >= a.n_frames) continue;
    const uint32_t left = a.n_frames - j0;
#pragma unroll
    for (int c = 0; c < CO; c++) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) v[i] = acc[c][i] != acc[c][i] ? __uint_as_float(kCanonNaN) : acc[c][i];   // (uncovered: still +0.0f)
      float* out = a.dst[c] + j0;
      if (left >= 8u) {
        __builtin_nontemporal_store(f4v{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4v*>(out));
        __builtin_nontemporal_store(f4v{v[4], v[5], v[6], v[7]}, reinterpret_cast<f4v*>(out) + 1);
      } else {                                               // the result's last lane: only the frames inside it
#pragma unroll
        for (int i = 0; i < 8; i++)
          if ((uint32_t)i < left) out[i] = v[i];
      }
    }
  }
}

}  // namespace

// 2 instances: 1 and 2 output channels
void launch_splice(const SpliceArgs& a, hipStream_t s) {
  const dim3 grid(std::min<uint32_t>((a.n_tiles + 3u) / 4u, 4096u));   // 4 waves, one tile each, per workgroup and stride
  if (a.channels == 2u) hipLaunchKernelGGL((splice_kernel<2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((splice_kernel<1>), grid, dim3(256), 0, s, a);
}

// ---- layer 1: the descriptors, the run ----------------------------------------------------------------------------------------

// a part as the kernel reads it: the rows its output channels read, moved to the part's first source frame in 64 bits
static SplicePartDev splice_part_dev(const ClipSrc& src, const wbx_splice_part& p) {
  const float* row[2] = {clip_row(src, 0) + p.first_frame, clip_row(src, 1) + p.first_frame};
  SplicePartDev d{};
  switch (p.channel_mode) {
    case WBX_CH_SWAP: d.src[0] = row[1], d.src[1] = row[0]; break;
    case WBX_CH_RIGHT: d.src[0] = d.src[1] = row[1]; break;
    case WBX_CH_LEFT:
    case WBX_CH_DUAL_MONO: d.src[0] = d.src[1] = row[0]; break;
    default: d.src[0] = row[0], d.src[1] = row[1]; break;    // KEEP, MONO_MIX
  }
  d.n = (uint32_t)p.n_frames;
  d.at = (uint32_t)p.at;
  d.fade_in = (uint32_t)p.fade_in;
  d.fade_out = (uint32_t)p.fade_out;
  d.gain = p.gain;
  d.bits = (uint32_t)p.fade_in_shape | (uint32_t)p.fade_out_shape << kSpliceShapeOutShift |
           ((p.flags & WBX_EDIT_REVERSE) ? kSpliceReversed : 0u) | (p.channel_mode == WBX_CH_MONO_MIX ? kSpliceMonoMix : 0u);
  return d;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status splice_run(wbx_ctx* c, const ClipSrc* srcs, const wbx_splice_part* parts, uint32_t n_parts, const SplicePlan& plan,
                      uint32_t channels, uint64_t n_frames, ClipSlot& slot, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, channels, plan.rate, n_frames, why);
  if (st != WBX_OK) return st;
  std::vector<SplicePartDev> dev(n_parts);                   // the uploads' sources: alive until the stream has been waited for
  for (uint32_t i = 0; i < n_parts; i++) dev[i] = splice_part_dev(srcs[i], parts[i]);
  SpliceStage& x = c->splice;
  hipError_t e = x.parts.ensure(n_parts);
  if (e == hipSuccess) e = x.tile_off.ensure(plan.tile_off.size());
  if (e == hipSuccess) e = x.tile_parts.ensure(plan.tile_parts.size());
  if (e == hipSuccess) e = hipMemcpyAsync(x.parts.p, dev.data(), n_parts * sizeof(SplicePartDev), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(x.tile_off.p, plan.tile_off.data(), plan.tile_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(x.tile_parts.p, plan.tile_parts.data(), plan.tile_parts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) {
    SpliceArgs a{};
    a.parts = x.parts.p;
    a.tile_off = x.tile_off.p;
    a.tile_parts = x.tile_parts.p;
    a.dst[0] = (float*)slot.d.ch[0];
    a.dst[1] = (float*)slot.d.ch[1];
    a.n_frames = (uint32_t)n_frames;
    a.n_tiles = (uint32_t)plan.n_tiles;
    a.channels = channels;
    launch_splice(a, on);
    e = hipGetLastError();
  }
  const hipError_t w = hipStreamSynchronize(on);             // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip splice", e);
  }
  return clipfx_measure_result(c, slot, n_frames, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_splice_plan(uint32_t channels, uint64_t n_frames, const wbx_splice_part* parts, uint32_t n_parts,
                                      const wbx_splice_source* sources, uint32_t n_sources, uint64_t* n_tiles, uint64_t* n_entries,
                                      uint32_t* tile_off, size_t cap_off, uint32_t* tile_parts, size_t cap_parts) {
  const char* msg = "";
  uint32_t rate = 0;
  const auto source_of = [&](uint32_t id) { return sources && id < n_sources ? &sources[id] : nullptr; };
  wbx_status st = splice_check(channels, n_frames, parts, n_parts, source_of, &rate, &msg);
  if (st != WBX_OK) return st;
  uint64_t tiles = 0, entries = 0;
  st = splice_table_size(n_frames, parts, n_parts, &tiles, &entries, &msg);
  if (st != WBX_OK) return st;
  if (tile_off && tile_parts) {
    if (cap_off < tiles + 1 || cap_parts < entries) return WBX_ERR_INVALID;
    splice_table(n_frames, parts, n_parts, tile_off, tile_parts);
  }
  if (n_tiles) *n_tiles = tiles;
  if (n_entries) *n_entries = entries;
  return WBX_OK;
}

extern "C" wbx_status wbx_clip_splice(wbx_ctx* c, uint32_t dst_clip, uint32_t channels, uint64_t n_frames,
                                      const wbx_splice_part* parts, uint32_t n_parts, wbx_clip_stats* stats_of_result) {
  if (!c) return WBX_ERR_INVALID;
  const char* msg = "";
  SplicePlan plan;
  wbx_splice_source tmp{};
  const auto source_of = [&](uint32_t id) -> const wbx_splice_source* {
    const ClipSlot* s = find_clip(c, id);
    if (!s) return nullptr;
    tmp = wbx_splice_source{s->d.channels, s->d.sample_rate, s->d.count, (int32_t)s->d.format, 0u};
    return &tmp;
  };
  wbx_status st = splice_check(channels, n_frames, parts, n_parts, source_of, &plan.rate, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  for (uint32_t i = 0; i < n_parts; i++)
    if (parts[i].src_clip == dst_clip) return fail(c, WBX_ERR_INVALID, "clip splice: the result may not replace a source");
  if (dst_clip >= (1u << 24)) return fail(c, WBX_ERR_INVALID, "clip id");
  st = splice_plan_table(n_frames, parts, n_parts, &plan, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  std::vector<ClipSrc> srcs(n_parts);
  for (uint32_t i = 0; i < n_parts; i++) srcs[i] = clip_src(c->clips[parts[i].src_clip]);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return splice_run(c, srcs.data(), parts, n_parts, plan, channels, n_frames, slot, stats_of_result, why);
  });
}
