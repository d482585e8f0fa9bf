// wbx_warp.hip — warp_search_kernel and warp_ola_kernel: a frame range of a resident planar F32 clip warped along time
// markers by WSOLA into a new planar F32 clip (wbx.h "Warping a clip"), and layer 1's calls on top of them.
//
// No reference counterpart.  The arithmetic is written out in wbx.h and mirrored by tests/warp_model.py.
//   the search   a marker pins a position whatever came before it, so it cuts the chain of "Stretching a clip": the
//             segments between markers are independent chains.  ONE workgroup of 512 lanes walks the steps of ITS segment
//             that belong to the launch's round, in order; blockIdx.x indexes the launch's list of segment ids.  The
//             searched step is wbx_wsola.h's, the same code stretch_search_kernel runs.  The pinned step (i = 0) is taken
//             unscored.  The position before a round's first step comes from the call's position table in device memory
//             (all K <= 2^22 positions stay resident), written by the same segment's workgroup of the round before —
//             an earlier launch on the same stream.  The anchor advances incrementally from the segment's (n_j, m_j)
//   the record   searched, candidates and max_shift are added into one device record with integer atomics: free of order
//   overlap-add  grid-wide, a lane per 16-B word of the result.  The lane finds its segment by bisecting the segment
//             table's output column, derives its step, and takes p_k and c_k = p_{k-1} + l_{k-1} from the position table
//             and the segment table; a word that straddles a step or a segment end resolves each frame.  Whole 16-B
//             stores, the result's ragged last word frame by frame
// Nothing waits on another workgroup anywhere.
#include "wbx_ctx.h"
#include "wbx_wsola.h"

#include <cstring>

namespace wbx {

namespace {

using namespace wsola;

template <int CH>
__global__ void __launch_bounds__(kLanes) warp_search_kernel(WarpArgs a) {
  __shared__ Lds lds;
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x >= a.count) return;
  // (everything below up to the staging is the same in every lane)
  const uint32_t j = a.ids[blockIdx.x];
  if (j >= a.S) return;
  const wbx_warp_segment g = a.seg[j], g1 = a.seg[j + 1u];
  const int64_t n = (int64_t)a.n, Hs = (int64_t)a.Hs, D = (int64_t)a.D;
  const int64_t s_j = (int64_t)g.src_frame;
  const uint64_t n_j = g1.src_frame - g.src_frame, m_j = g1.out_frame - g.out_frame;
  const uint64_t i0 = (uint64_t)a.round * a.round_steps;
  const uint64_t i1 = i0 + a.round_steps < g.steps ? i0 + a.round_steps : g.steps;
  if (i0 >= i1) return;
  const uint64_t hop = (uint64_t)a.Hs * n_j;                   // (< 2^12 * 2^31)
  const uint64_t qn = hop / m_j, rn = hop % m_j;
  const uint64_t at = i0 * hop;                                // i0 Hs < m_j < 2^31 and n_j < 2^31: below 2^62
  int64_t anchor = s_j + (int64_t)(at / m_j);
  uint64_t rem = at % m_j;
  int64_t p = i0 == 0u ? 0 : (int64_t)a.pos[g.first_step + i0 - 1u];
  uint32_t max_shift = 0u;
  uint64_t searched = 0ull, scored = 0ull;
  for (uint64_t i = i0; i < i1; i++) {
    if (i == 0u) {                                             // pinned: never scored
      p = s_j;
    } else {
      const int64_t c = p + Hs;
      const int64_t lo = anchor - D > 0 ? anchor - D : 0, hi = anchor + D < n - 1 ? anchor + D : n - 1;
      if (lo <= c && c <= hi) {
        p = c;
      } else if (lo == hi) {                                   // one candidate: its score is the greatest
        p = lo;
        searched++, scored++;
      } else {
        const uint32_t ncand = (uint32_t)(hi - lo) + 1u;
        p = wsola_search<CH>(lds, a.src[0], a.src[1], n, a.Hs, c, lo, ncand, tid);
        searched++, scored += ncand;
      }
    }
    const int64_t shift = p > anchor ? p - anchor : anchor - p;
    max_shift = (uint32_t)shift > max_shift ? (uint32_t)shift : max_shift;
    if (tid == 0u) a.pos[g.first_step + i] = (int32_t)p;
    anchor += (int64_t)qn;
    rem += rn;
    if (rem >= m_j) rem -= m_j, anchor++;
  }
  if (tid == 0u) {
    if (searched) atomicAdd(&a.rec->searched, (unsigned long long)searched), atomicAdd(&a.rec->candidates, (unsigned long long)scored);
    if (max_shift) atomicMax(&a.rec->max_shift, max_shift);
  }
}

// x[c][g] of the text: zero outside [0, n), what is not finite as 0.0
__device__ __forceinline__ double x_at(const float* __restrict__ row, int64_t g, int64_t n) { return g < n ? sample_in(row[g]) : 0.0; }

// the step an output frame o < m lies in: its position, its continuation, its length and o's offset inside it
struct WarpAt {
  int64_t p, c;
  uint32_t l, off;
};
__device__ __forceinline__ WarpAt warp_at(const WarpArgs& a, uint32_t o) {
  const wbx_warp_segment* __restrict__ seg = a.seg;
  uint32_t lo = 0u, hi = a.S;                                  // t_lo <= o < t_hi (t_0 = 0, t_S = m)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg[mid].out_frame <= (uint64_t)o) lo = mid;
    else hi = mid;
  }
  const uint32_t t_j = (uint32_t)seg[lo].out_frame, t_next = (uint32_t)seg[lo + 1u].out_frame;
  const uint32_t i = (o - t_j) / a.Hs, start = t_j + i * a.Hs;
  const uint64_t k = seg[lo].first_step + i;
  WarpAt w;
  w.l = t_next - start < a.Hs ? t_next - start : a.Hs;
  w.off = o - start;
  w.p = (int64_t)a.pos[k];
  if (k == 0u) {
    w.c = 0;
  } else if (i > 0u) {
    w.c = (int64_t)a.pos[k - 1u] + (int64_t)a.Hs;
  } else {                                                     // the last step of the segment before: the only short one
    const uint64_t m_prev = seg[lo].out_frame - seg[lo - 1u].out_frame;
    w.c = (int64_t)a.pos[k - 1u] + (int64_t)(m_prev - (seg[lo - 1u].steps - 1u) * a.Hs);
  }
  return w;
}

template <int CH>
__global__ void __launch_bounds__(256) warp_ola_kernel(WarpArgs a) {
  const uint64_t word = (uint64_t)blockIdx.x * 256u + threadIdx.x;   // the lane's 16-B word of the result
  const uint64_t j0 = 4u * word;                                // its first frame
  if (j0 >= (uint64_t)a.m) return;
  const int64_t n = (int64_t)a.n;
  const double* __restrict__ up = a.win;
  const double* __restrict__ dn = a.win + a.Hs;
  const uint32_t left = a.m - (uint32_t)j0;
  float y[CH][4];
  WarpAt w = warp_at(a, (uint32_t)j0);
#pragma unroll
  for (int f = 0; f < 4; f++) {
    if ((uint32_t)f >= left) {
#pragma unroll
      for (int ch = 0; ch < CH; ch++) y[ch][f] = 0.0f;
      continue;
    }
    if (f > 0 && ++w.off >= w.l) w = warp_at(a, (uint32_t)j0 + (uint32_t)f);   // past a step's or a segment's end
    const uint32_t i = w.off;
#pragma unroll
    for (int ch = 0; ch < CH; ch++) {
      const float* __restrict__ row = a.src[ch];
      const double xp = x_at(row, w.p + (int64_t)i, n);
      y[ch][f] = w.p == w.c ? __double2float_rn(xp)
                            : __double2float_rn(__dadd_rn(__dmul_rn(up[i], xp), __dmul_rn(dn[i], x_at(row, w.c + (int64_t)i, n))));
    }
  }
#pragma unroll
  for (int ch = 0; ch < CH; ch++) {
    float* out = a.dst[ch] + j0;
    if (left >= 4u) {
      __builtin_nontemporal_store(f4{y[ch][0], y[ch][1], y[ch][2], y[ch][3]}, reinterpret_cast<f4*>(out));
    } else {                                                   // the result's last word: only the frames inside it
#pragma unroll
      for (int f = 0; f < 4; f++)
        if ((uint32_t)f < left) out[f] = y[ch][f];
    }
  }
}

}  // namespace

void launch_warp_search(const WarpArgs& a, hipStream_t s) {
  if (a.channels == 2u) hipLaunchKernelGGL(warp_search_kernel<2>, dim3(a.count), dim3(kLanes), 0, s, a);
  else hipLaunchKernelGGL(warp_search_kernel<1>, dim3(a.count), dim3(kLanes), 0, s, a);
}
void launch_warp_ola(const WarpArgs& a, hipStream_t s) {
  const uint32_t blocks = (uint32_t)(((uint64_t)a.m / 4u + 1u + 255u) / 256u);
  if (a.channels == 2u) hipLaunchKernelGGL(warp_ola_kernel<2>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(warp_ola_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
}

// ---- layer 1: the check (no device call), the run ---------------------------------------------------------------------------

// The arithmetic of the call first — it needs no clip of that size to be refused — then the clip
wbx_status warp_check(const ClipSrc& src, const WarpCall& k, const char** why) {
  const wbx_status st = warp_check_args(k, why);
  if (st != WBX_OK) return st;
  if (src.format != (uint32_t)WBX_FMT_F32) return *why = "clip warp: the clip's storage format is not F32", WBX_ERR_UNSUPPORTED;
  if (src.channels < 1 || src.channels > 2) return *why = "clip warp: clip channel count (1 or 2)", WBX_ERR_UNSUPPORTED;
  if (k.first_frame > src.frames || k.n_frames > src.frames - k.first_frame)
    return *why = "clip warp: the range ends past the clip", WBX_ERR_INVALID;
  return WBX_OK;
}

// `slot` becomes the new clip (built on the edit stream; complete when this returns WBX_OK, released otherwise)
wbx_status warp_run(wbx_ctx* c, const ClipSrc& src, uint32_t rate, const WarpCall& k, ClipSlot& slot, int32_t* positions_out,
                    wbx_warp_info* info, wbx_clip_stats* stats, std::string* why) {
  const hipStream_t on = c->fx.side.stream;
  const wbx_status st = clipfx_blank_clip(c, slot, src.channels, rate, k.out_frames, why);
  if (st != WBX_OK) return st;
  WarpStage& z = c->wrp;
  StretchStage& zs = c->str;                                   // the window table is the stretch's
  const uint32_t N = k.window, Hs = N / 2u, S = k.n_markers + 1u;
  const uint64_t n = k.n_frames, m = k.out_frames;
  WarpArgs a{};
  for (uint32_t i = 0; i < 2; i++) {
    a.src[i] = clip_row(src, i) + k.first_frame;
    a.dst[i] = (float*)slot.d.ch[i % src.channels];
  }
  a.n = (uint32_t)n, a.m = (uint32_t)m;
  a.Hs = Hs, a.D = k.tolerance;
  a.S = S;
  a.channels = src.channels;
  z.timed = false;
  hipError_t e = hipSuccess;
  for (Event& ev : z.mark)
    if (e == hipSuccess) e = ev.ensure(hipEventDefault);
  // the plan, on the host: the segment table with its closing record, then the ids of every search launch
  if (e == hipSuccess) e = z.h_seg.ensure((size_t)S + 1u);
  WarpPlan plan;
  uint64_t K = 0;
  if (e == hipSuccess) {
    (void)warp_segments(n, m, k.markers, k.n_markers, N, z.h_seg.p, (size_t)S);
    K = z.h_seg.p[S - 1u].first_step + z.h_seg.p[S - 1u].steps;
    z.h_seg.p[S] = wbx_warp_segment{n, m, K, 0};
    plan = warp_plan(z.h_seg.p, S, stretch_launch_steps(n, N, k.tolerance));
    e = z.h_ids.ensure(plan.ids.size());
  }
  if (e == hipSuccess) std::memcpy(z.h_ids.p, plan.ids.data(), plan.ids.size() * sizeof(uint32_t));
  const bool fresh = zs.win_of != N;
  if (e == hipSuccess && fresh) {
    zs.win_of = 0;                                             // (no table until this one's upload has completed)
    e = zs.h_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) e = zs.d_win.ensure(kStretchMaxWindow);
    if (e == hipSuccess) (void)stretch_window(N, zs.h_win.p, N);
  }
  if (e == hipSuccess) e = z.d_pos.ensure((size_t)K);
  if (e == hipSuccess && positions_out) e = z.h_pos.ensure((size_t)K);
  if (e == hipSuccess) e = z.d_seg.ensure((size_t)S + 1u);
  if (e == hipSuccess) e = z.d_ids.ensure(plan.ids.size());
  if (e == hipSuccess) e = z.d_rec.ensure(1);
  if (e == hipSuccess) e = z.h_rec.ensure(1);
  if (e == hipSuccess) e = hipEventRecord(z.mark[0], on);
  if (e == hipSuccess && fresh) e = hipMemcpyAsync(zs.d_win.p, zs.h_win.p, (size_t)N * sizeof(double), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_seg.p, z.h_seg.p, ((size_t)S + 1u) * sizeof(wbx_warp_segment), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.d_ids.p, z.h_ids.p, plan.ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, on);
  if (e == hipSuccess) e = hipMemsetAsync(z.d_rec.p, 0, sizeof(WarpRecord), on);
  if (e == hipSuccess) {
    a.pos = z.d_pos.p;
    a.seg = z.d_seg.p;
    a.rec = z.d_rec.p;
    a.win = zs.d_win.p;
    a.round_steps = plan.round_steps;
  }
  uint64_t launches = 0;
  for (size_t i = 0; i < plan.launches.size() && e == hipSuccess; i++) {
    const WarpLaunch& l = plan.launches[i];
    a.ids = z.d_ids.p + l.first;
    a.round = l.round;
    a.count = l.count;
    launch_warp_search(a, on);
    e = hipGetLastError();
    launches++;
  }
  if (e == hipSuccess) {
    launch_warp_ola(a, on);
    e = hipGetLastError();
    launches++;
  }
  if (e == hipSuccess) e = hipEventRecord(z.mark[1], on);
  if (e == hipSuccess) e = hipMemcpyAsync(z.h_rec.p, z.d_rec.p, sizeof(WarpRecord), hipMemcpyDeviceToHost, on);
  if (e == hipSuccess && positions_out) e = hipMemcpyAsync(z.h_pos.p, z.d_pos.p, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, on);
  const hipError_t w = hipStreamSynchronize(on);               // (also after a failure: nothing may still write the new clip)
  if (e == hipSuccess) e = w;
  if (e != hipSuccess) {
    if (fresh) zs.win_of = 0;
    clip_release(c, slot);
    return stage_fail(why, WBX_ERR_DEVICE, "clip warp", e);
  }
  zs.win_of = N;
  z.timed = true;
  if (positions_out) std::memcpy(positions_out, z.h_pos.p, (size_t)K * sizeof(int32_t));
  if (info) {
    const WarpRecord& t = z.h_rec.p[0];
    info->steps = K;
    info->searched_steps = t.searched;
    info->candidates = t.candidates;
    info->max_shift = t.max_shift;
    info->launches = (uint32_t)launches;
    info->segments = S;
    info->longest_segment_steps = (uint32_t)plan.longest;
  }
  return clipfx_measure_result(c, slot, m, stats, why);
}

}  // namespace wbx

extern "C" wbx_status wbx_warp_check(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                                     uint32_t window_frames, uint32_t tolerance_frames) {
  return wbx::warp_check_sizes(n_frames, out_frames, markers, n_markers, window_frames, tolerance_frames);
}
extern "C" uint64_t wbx_warp_steps(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                                   uint32_t window_frames) {
  return wbx::warp_steps(n_frames, out_frames, markers, n_markers, window_frames);
}
extern "C" wbx_status wbx_warp_segments(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                                        uint32_t window_frames, wbx_warp_segment* out, size_t cap_segments) {
  return wbx::warp_segments(n_frames, out_frames, markers, n_markers, window_frames, out, cap_segments);
}
extern "C" uint32_t wbx_warp_max_markers(void) { return wbx::kWarpMaxMarkers; }
extern "C" uint64_t wbx_warp_max_steps(void) { return wbx::kWarpMaxSteps; }
extern "C" uint32_t wbx_warp_launch_segments(void) { return wbx::kWarpLaunchSegments; }
extern "C" uint64_t wbx_warp_launches(uint64_t n_frames, uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers,
                                      uint32_t window_frames, uint32_t tolerance_frames) {
  return wbx::warp_launches(n_frames, out_frames, markers, n_markers, window_frames, tolerance_frames);
}

extern "C" wbx_status wbx_warp_ms(wbx_ctx* c, double* out) {
  return wbx::stage_ms(c, &wbx_ctx::wrp, "warp time: no warp call has completed on this context", out);
}

extern "C" wbx_status wbx_clip_warp(wbx_ctx* c, uint32_t src_clip, uint32_t dst_clip, uint64_t first_frame, uint64_t n_frames,
                                    uint64_t out_frames, const wbx_warp_marker* markers, uint32_t n_markers, uint32_t window_frames,
                                    uint32_t tolerance_frames, int32_t* positions_out, size_t positions_cap, wbx_warp_info* info,
                                    wbx_clip_stats* stats_of_result) {
  using namespace wbx;
  if (!c) return WBX_ERR_INVALID;
  wbx_status st = clipfx_check_ids(c, src_clip, dst_clip, "clip warp: unknown source clip", "clip warp: the result may not replace its source");
  if (st != WBX_OK) return st;
  const ClipSrc src = clip_src(c->clips[src_clip]);
  const uint32_t rate = c->clips[src_clip].d.sample_rate;
  const WarpCall k{first_frame, n_frames, out_frames, markers, n_markers, window_frames, tolerance_frames, positions_out != nullptr,
                   positions_cap};
  const char* msg = "";
  st = warp_check(src, k, &msg);
  if (st != WBX_OK) return fail(c, st, msg);
  return clipfx_into_clip(c, dst_clip, [&](ClipSlot& slot, std::string* why) {
    return warp_run(c, src, rate, k, slot, positions_out, info, stats_of_result, why);
  });
}
