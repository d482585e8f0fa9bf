#!/usr/bin/env python3
"""Warping a clip in numbers (MEASUREMENTS.md "Warping a clip"): the F32 clips of tools/bench_stretch.py — 2^22 and 2^24
frames at 48 kHz, mono and stereo — through wbx_clip_warp to 2/3, 1.5 and 2 times their length with N = 2048 and D = 512,
along markers in proportion: s_j = j n / S, t_j = j m / S for S in {1, 16, 256, 4096} segments.  Each call is timed on the
device between two events around its launches (wbx_warp_ms).  Beside every call, in the same process and alternating with it,
wbx_clip_stretch of the same range to the same length (wbx_stretch_ms).  Per cell:
  scored terms/s       candidates * Hs of the call's info over the whole call's device time
  searched / steps     of the call's info
  launches             of the call's info
  over_stretch         the call's device time over the stretch's
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RATIOS = {"2/3": (2, 3), "1.5": (3, 2), "2": (2, 1)}


def fig(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1 << 22, 1 << 24])
    ap.add_argument("--segments", type=int, nargs="*", default=[1, 16, 256, 4096])
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--tolerance", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W
    from bench_stretch import material

    ctx = W.MixContext(4, block=512)
    SRC, DST = 1, 9                                            # the results replace each other in DST
    N, D, Hs = a.window, a.tolerance, a.window // 2
    L = W.lib()
    out = {"rate": a.rate, "window": N, "tolerance": D, "device": ctx.device_info(), "launch_terms": L.wbx_stretch_launch_terms(),
           "launch_segments": L.wbx_warp_launch_segments()}
    res = []
    for n in a.frames:
        for ch in a.channels:
            ctx.clip_upload(SRC, "f32", a.rate, material(np, ch, n, 0x57E + ch))
            for name, (num, den) in RATIOS.items():
                m = n * num // den
                for S in a.segments:
                    mk = [(j * n // S, j * m // S) for j in range(1, S)]
                    warp, stretch, info, s_info = [], [], None, None
                    for i in range(a.repeats + 1):             # alternating; the first pair warms
                        info = ctx.clip_warp(SRC, DST, 0, n, m, mk, N, D)
                        w = ctx.warp_ms()
                        s_info = ctx.clip_stretch(SRC, DST, 0, n, m, N, D)
                        s = ctx.stretch_ms()
                        if i:
                            warp.append(w)
                            stretch.append(s)
                    r = {"frames": n, "channels": ch, "ratio": name, "out_frames": m, "segments": S, "info": info, "device": fig(warp),
                         "stretch_device": fig(stretch), "stretch_info": s_info, "launch_steps": L.wbx_stretch_launch_steps(n, N, D)}
                    ms = r["device"]["median_ms"]
                    r["scored_terms"] = info["candidates"] * Hs
                    r["scored_terms_per_s"] = r["scored_terms"] / (ms * 1e-3)
                    r["stretch_scored_terms_per_s"] = s_info["candidates"] * Hs / (r["stretch_device"]["median_ms"] * 1e-3)
                    r["searched_over_steps"] = info["searched_steps"] / info["steps"]
                    r["launches"] = info["launches"]
                    r["over_stretch"] = ms / r["stretch_device"]["median_ms"]
                    r["times_real_time"] = m / (ms * 1e-3) / a.rate
                    res.append(r)
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
