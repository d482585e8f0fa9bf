// wbx_bounce.hip — stem_kernel: what a render pass computed per track, per bus and for the master, kept as clip audio.
//
// The post-fader buffer of a track (mixing_buffer after Track::process, engine.cpp:1602-1616, track.cpp:728-731) exists
// only in registers inside the mix kernel.  A bounce (wbx_engine_bounce) renders its range through the ordinary sequencer,
// pre-render pass, mix and sum, and this kernel — behind them, reading the same plan — writes the signals asked for into
// their destination clips: a track's buffer rendered again from its plan row with the arithmetic of render_generic /
// sample_at (wbx_render.h: the stream calls added in order into a cleared buffer, sampler.cpp:56,152, then — post-fader —
// one multiplication by fl(volume * pan_coeffs[c]), track.cpp:728-731), a bus sum or the clamped master copied out of the
// pass's result buffers.  Nothing of it lives in the mix, sum or callback kernels.
//
// One workgroup of four waves per (signal, block) — the grid follows the signals asked for, not the session — no LDS, no
// barrier: every wave reads the signal's descriptor, its 16-B plan row and the 64-B template(s) one dword per lane and
// broadcasts them into scalar registers (as gen_kernel does), so kind, format and speed branches are wave-uniform.  Each
// lane owns four consecutive frames of one channel and stores them with one 16-B nontemporal store (the destination is
// written once and not read again by this pass); the frames of the range's last block that lie past the clip's length are
// dropped, so the clip's 16 zero frames of padding stay zero.
#include "wbx_ctx.h"
#include "wbx_render.h"

namespace wbx {

namespace {

// a 64-B plan template from sixteen broadcast dwords of `w`, lanes base .. base + 15 (wave-uniform, scalar registers)
__device__ __forceinline__ DTrackBlock record_from_lanes(uint32_t w, int base) {
  auto rl = [&](int k) { return (uint32_t)__builtin_amdgcn_readlane((int)w, base + k); };
  DTrackBlock rec;
  rec.src[0] = (const void*)(((uint64_t)rl(1) << 32) | rl(0));
  rec.src[1] = (const void*)(((uint64_t)rl(3) << 32) | rl(2));
  rec.pos = __longlong_as_double((long long)(((uint64_t)rl(5) << 32) | rl(4)));
  rec.speed = __longlong_as_double((long long)(((uint64_t)rl(7) << 32) | rl(6)));
  rec.gain = __uint_as_float(rl(8));
  rec.g[0] = __uint_as_float(rl(9));
  rec.g[1] = __uint_as_float(rl(10));
  const uint32_t q = rl(11), h = rl(12), m = rl(13);
  rec.nseg = (uint8_t)(q & 0xFFu);
  rec.kind = (uint8_t)((q >> 8) & 0xFFu);
  rec.dst_start = (uint16_t)(q >> 16);
  rec.len = (uint16_t)(h & 0xFFFFu);
  rec.req_len = (uint16_t)(h >> 16);
  rec.format = (uint8_t)(m & 0xFFu);
  rec.flags = (uint8_t)((m >> 8) & 0xFFu);
  rec._pad = (uint16_t)(m >> 16);
  rec.sample = rl(14);
  rec.extra = rl(15);
  return rec;
}

// What the mix renders from one template: a record the pre-render pass has been through (rewritten in place as a unity
// read of its scratch row; nseg and extra still describe the original calls) or any record the hot loop streams itself is
// ONE stream call, the inline one; only a record still KIND_GENERIC carries its further calls in the pool.
__device__ __forceinline__ bool stem_record(DTrackBlock& r, uint32_t pool_chunks) {
  const uint8_t kind = r.kind & KIND_MASK;
  if (kind == KIND_SILENT || r.nseg == 0u) return false;
  if (kind != KIND_GENERIC) r.nseg = 1;
  else if (r.nseg > 1u && r.extra >= pool_chunks) return false;   // (never: the plan reports a pool overflow instead)
  return true;
}

__global__ void __launch_bounds__(256) stem_kernel(StemArgs a) {
  const uint32_t K = a.n_blocks;
  const uint32_t s = blockIdx.x / K, b = blockIdx.x - s * K;   // (signal, block): uniform
  if (s >= a.n_src) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t F = a.block_frames, C = a.channels, S4 = F >> 2;
  const uint64_t at = a.first_frame + (uint64_t)b * F;          // the block's first frame in the destination clips
  if (at >= a.n_frames) return;
  const uint32_t valid = (uint32_t)(a.n_frames - at < (uint64_t)F ? a.n_frames - at : (uint64_t)F);
  float* dst[2];
  uint32_t kind, index, tap;
  {
    const uint32_t w = reinterpret_cast<const uint32_t*>(a.src + s)[lane & 7u];
    auto rl = [&](int k) { return (uint32_t)__builtin_amdgcn_readlane((int)w, k); };
    dst[0] = (float*)(((uint64_t)rl(1) << 32) | rl(0));
    dst[1] = (float*)(((uint64_t)rl(3) << 32) | rl(2));
    kind = rl(4);
    index = rl(5);
    tap = rl(6);
  }
  auto store = [&](uint32_t c, uint32_t j0, const f4& v) {   // frames j0 .. j0 + 3 of channel c; j0 < valid
    float* p = (c ? dst[1] : dst[0]) + at + j0;              // 16-B aligned: 256-B aligned rows, F a multiple of 4
    if (j0 + 4u <= valid) {
      __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p));
    } else {
      const float e[4] = {v.x, v.y, v.z, v.w};
      for (uint32_t i = 0; j0 + i < valid; i++) p[i] = e[i];
    }
  };

  if (kind != 0u) {   // WBX_BOUNCE_BUS / WBX_BOUNCE_MASTER: a strided copy out of the pass's results
    const float* base = kind == 1u ? (a.buses && index < a.n_buses ? a.buses + ((size_t)b * a.n_buses + index) * C * F : nullptr)
                                   : (a.master ? a.master + (size_t)b * C * F : nullptr);
    for (uint32_t slot = threadIdx.x; slot < C * S4; slot += 256u) {
      const uint32_t c = slot / S4, j0 = (slot - c * S4) * 4u;
      if (j0 >= valid) continue;
      const f4 v = base ? *reinterpret_cast<const f4*>(base + (size_t)c * F + j0) : f4{0.0f, 0.0f, 0.0f, 0.0f};
      store(c, j0, v);
    }
    return;
  }

  // WBX_BOUNCE_TRACK: the track's plan row of this block, its template(s), the gain row
  if (index >= a.n_tracks) return;
  DRow row;
  {
    const uint32_t w = reinterpret_cast<const uint32_t*>(a.rows + (size_t)b * a.n_tracks + index)[lane & 3u];
    auto rl = [&](int k) { return (uint32_t)__builtin_amdgcn_readlane((int)w, k); };
    row.pos = __longlong_as_double((long long)(((uint64_t)rl(1) << 32) | rl(0)));
    row.tmpl = rl(2);
    row.flags = rl(3);
  }
  const bool pair = (row.flags & ROW_PAIR) != 0u;
  const bool have = !(row.flags & ROW_SILENT) && row.tmpl < a.tmpl_cap && (!pair || row.tmpl + 1u < a.tmpl_cap);
  DTrackBlock r0{}, r1{};
  bool on0 = false, on1 = false;
  if (have) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(a.tmpl + row.tmpl)[pair ? (lane & 31u) : (lane & 15u)];
    r0 = record_from_lanes(w, 0);
    // a template shared by a run of blocks: the position is the row's.  Only plan_steady_run (wbx_seq.h) sets ROW_POS, on
    // rows whose flags are ROW_POS alone — one whole-block call — so a ROW_PAIR never carries it and its second template
    // always holds its own position (the plan read-back, wbx_seq.h "fetch", applies it to the first record only, too).
    if (row.flags & ROW_POS) r0.pos = row.pos;
    on0 = stem_record(r0, a.pool_chunks);
    if (pair) {                                   // a clip boundary inside the block: the second call is the template behind
      r1 = record_from_lanes(w, 16);
      on1 = stem_record(r1, a.pool_chunks);
    }
  }
  float g0, g1;   // the track's pair of the gain row, broadcast like the records
  {
    const uint32_t w = reinterpret_cast<const uint32_t*>(a.gains + (size_t)index * 2u)[lane & 1u];
    g0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w, 0));
    g1 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)w, 1));
  }
  const bool post = tap == 0u;   // WBX_TAP_POST_FADER
  for (uint32_t slot = threadIdx.x; slot < C * S4; slot += 256u) {
    const uint32_t c = slot / S4, j0 = (slot - c * S4) * 4u;
    if (j0 >= valid) continue;
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};              // the cleared mixing buffer (engine.cpp:1602)
    if (on0) v = render_generic(r0, a.pool, c, j0);
    if (on1) {                                    // the two calls of a pair do not overlap: each frame takes one addition
      const f4 u = render_generic(r1, a.pool, c, j0);
      v = f4{__fadd_rn(v.x, u.x), __fadd_rn(v.y, u.y), __fadd_rn(v.z, u.z), __fadd_rn(v.w, u.w)};
    }
    if (post) {                                   // dsp::apply_gain, track.cpp:728-731 (0 when muted: -x becomes -0)
      const float g = c ? g1 : g0;
      v = f4{__fmul_rn(v.x, g), __fmul_rn(v.y, g), __fmul_rn(v.z, g), __fmul_rn(v.w, g)};
    }
    store(c, j0, v);
  }
}

}  // namespace

void launch_stem(const StemArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(stem_kernel, dim3(a.n_src * a.n_blocks), dim3(256), 0, s, a);
}

}  // namespace wbx
