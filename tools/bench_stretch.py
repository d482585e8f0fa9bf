#!/usr/bin/env python3
"""Stretching a clip in numbers (MEASUREMENTS.md "Stretching a clip"): F32 clips of 2^22 and 2^24 frames at 48 kHz, mono and
stereo (a few sines and noise), through wbx_clip_stretch to 2/3, 1.5 and 2 times their length with N = 2048 and D = 512.
Each call is timed on the device between two events around its launches (wbx_stretch_ms).  Beside every call, in the same
process and alternating with it, the same call with D = 0: plain overlap-add, the same steps walked and the same frames
written, nothing scored — its time is the overlap-add's (and the walk's), and the difference is the search's:
  scored terms/s   candidates * Hs of the call's info over that difference
  frames/s         out_frames over the D = 0 call's time
  whole call       out_frames over the whole call's time, and as a multiple of real time at 48 kHz
  searched_steps / steps of the call's info
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = {"2/3": (2, 3), "1.5": (3, 2), "2": (2, 1)}


def fig(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def material(np, channels, n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    planes = []
    for c in range(channels):
        v = 0.1 * rng.standard_normal(n)
        for period, amp in ((218.2 + 11 * c, 0.4), (72.7, 0.2), (36.1 + c, 0.1)):
            v += amp * np.sin(2 * np.pi * i / period)
        planes.append(v.astype(np.float32))
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1 << 22, 1 << 24])
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--tolerance", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    SRC, DST = 1, 9                                            # the results replace each other in DST
    N, D, Hs = a.window, a.tolerance, a.window // 2
    out = {"rate": a.rate, "window": N, "tolerance": D, "device": ctx.device_info(),
           "launch_terms": W.lib().wbx_stretch_launch_terms(), "band_steps": W.lib().wbx_stretch_band_steps()}
    res = []
    for n in a.frames:
        for ch in (1, 2):
            ctx.clip_upload(SRC, "f32", a.rate, material(np, ch, n, 0x57E + ch))
            for name, (num, den) in RATIOS.items():
                m = n * num // den
                whole, plain, info = [], [], None
                for i in range(a.repeats + 1):                 # alternating; the first pair warms
                    info = ctx.clip_stretch(SRC, DST, 0, n, m, N, D)
                    w = ctx.stretch_ms()
                    ctx.clip_stretch(SRC, DST, 0, n, m, N, 0)
                    p = ctx.stretch_ms()
                    if i:
                        whole.append(w)
                        plain.append(p)
                r = {"frames": n, "channels": ch, "ratio": name, "out_frames": m, "info": info, "device": fig(whole), "plain_device": fig(plain),
                     "launch_steps": W.lib().wbx_stretch_launch_steps(n, N, D)}
                search_ms = r["device"]["median_ms"] - r["plain_device"]["median_ms"]
                r["search_ms"] = search_ms
                r["scored_terms"] = info["candidates"] * Hs
                r["scored_terms_per_s"] = r["scored_terms"] / (search_ms * 1e-3) if search_ms > 0 else None
                r["us_per_searched_step"] = 1e3 * search_ms / info["searched_steps"] if info["searched_steps"] else None
                r["ola_frames_per_s"] = m / (r["plain_device"]["median_ms"] * 1e-3)
                r["frames_per_s"] = m / (r["device"]["median_ms"] * 1e-3)
                r["times_real_time"] = r["frames_per_s"] / a.rate
                r["searched_over_steps"] = info["searched_steps"] / info["steps"]
                res.append(r)
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
