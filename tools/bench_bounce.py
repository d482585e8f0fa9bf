#!/usr/bin/env python3
"""Bouncing in numbers (MEASUREMENTS.md "Bouncing", profiles/bounce_c3.json): the c3 session (4096 stereo tracks, 44.1 kHz
clips in a 48 kHz session, gain + pan) over K blocks of 512 frames —

  render      wbx_engine_render(K) of the session: what a render costs without keeping anything per track
  stems_all   wbx_engine_bounce of all 4096 tracks (post-fader) over the same range
  stems_3     ... of 3 tracks: the cost follows the sources asked for, not the session

Wall times on one GPU: warm-up, then `--repeats` rounds in the order render, stems_all, stems_all, render (A B B A) with the
3-track bounce behind each round; median and spread (min .. max) per figure.  Kernel times come from a run of its own under
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_bounce.py --repeats 2
(stem_kernel, and the mix kernel beside it).  The JSON line this prints carries the algorithmic bytes of the stem pass
(`stem_pass_bytes`) for the bandwidth figure.  `render` is this tree's wbx_engine_render: the same kernels as the parent
commit's, which a bounce leaves byte-identical."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from whitebox_amd import synth
    from whitebox_amd.engine import build_engine

    N, K, F = a.tracks, a.blocks, 512
    spec = synth.make_session("c3", N, src_rate=44100, n_blocks=K, seed=0x5EED0003)
    eng = build_engine(spec, max_blocks=K, device_synth=True)
    unit = (F / spec.sample_rate) / (60.0 / spec.bpm)
    lo, hi = 0.0, K * unit
    all_src = [("track", t) for t in range(N)]
    few_src = [("track", t) for t in (0, N // 2, N - 1)]

    def render():
        eng.set_playhead_position(lo)
        eng.play()
        eng.ctx.sync()
        t0 = time.perf_counter()
        eng.render(K)
        eng.ctx.sync()
        dt = time.perf_counter() - t0
        eng.stop()
        return dt

    def bounce(src):
        eng.ctx.sync()
        t0 = time.perf_counter()
        ids, n = eng.bounce(lo, hi, src)
        dt = time.perf_counter() - t0           # (the call returns when the samples are complete)
        for i in ids:
            eng.delete_sample(i)
        return dt, n

    for _ in range(a.warmup):
        render()
        bounce(all_src)
        bounce(few_src)
    t = {"render": [], "stems_all": [], "stems_3": []}
    n_frames = 0
    for _ in range(a.repeats):
        t["render"].append(render())
        t["stems_all"].append(bounce(all_src)[0])
        d, n_frames = bounce(all_src)
        t["stems_all"].append(d)
        t["render"].append(render())
        t["stems_3"].append(bounce(few_src)[0])

    def fig(v):
        return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}

    C = spec.channels
    clip_bytes = N * 2 * 4 * n_frames * (44100 / 48000)          # stereo fp32 clips, each source frame read once
    out = {"session": "c3", "tracks": N, "blocks": K, "block_frames": F, "n_frames": n_frames, "device": eng.ctx.device_info(),
           "mix_kernel": eng.ctx.kernel_name(),
           "render": fig(t["render"]), "stems_all": fig(t["stems_all"]), "stems_3": fig(t["stems_3"]),
           "stems_all_over_render": statistics.median(t["stems_all"]) / statistics.median(t["render"]),
           "stems_3_over_render": statistics.median(t["stems_3"]) / statistics.median(t["render"]),
           "stem_pass_bytes": {"clip_read": clip_bytes, "stem_write": N * C * 4 * n_frames},
           "destination_bytes": N * C * 4 * (n_frames + 16)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
