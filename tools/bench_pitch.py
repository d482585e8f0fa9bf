#!/usr/bin/env python3
"""Transposing a clip in numbers (MEASUREMENTS.md "Transposing a clip"): a stereo F32 clip of 2^22 frames at 48 kHz (a few
sines and noise) through wbx_clip_pitch at its own length with N = 2048, D = 512 and WBX_SRC_GOOD, at the ratios 3/2, 2/3
and 1265/1194.  Each call is timed on the device between two events around its launches (wbx_pitch_ms) and on the host
around the whole call, which ends in a wait for the device.
Beside it, for the two ratios the interface could express before (a rate of 32 000 and of 72 000 Hz) and ALTERNATING with
it in the same process: the two-call composition, wbx_clip_stretch to mid_frames frames into a temporary clip, then
wbx_clip_resample of that clip.  The stretch is timed on the device (wbx_stretch_ms); the conversion has no device timer, so
its figure is the host's clock around the call (it ends in a wait for the device: launch, allocation and wait included), as
tools/bench_resample.py takes it.  Both whole paths are also given as host time.
  composition_ms   the stretch's device ms + the conversion's host ms
  fused_over_composition   wbx_pitch_ms over that
  spread           (max - min) of the composition's repeats
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = {"3/2": (3, 2, 32000), "2/3": (2, 3, 72000), "1265/1194": (1265, 1194, None)}   # (num, den, the composition's rate)


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
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--tolerance", type=int, default=512)
    ap.add_argument("--quality", default="good")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    SRC, DST, TMP, DST2 = 1, 9, 10, 11                         # the results replace each other
    n, ch, N, D = a.frames, a.channels, a.window, a.tolerance
    ctx.clip_upload(SRC, "f32", a.rate, material(np, ch, n, 0x917 + ch))
    out = {"frames": n, "channels": ch, "rate": a.rate, "window": N, "tolerance": D, "quality": a.quality, "device": ctx.device_info()}

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return r, 1e3 * (time.perf_counter() - t0)

    res = []
    for name, (num, den, rate2) in RATIOS.items():
        mid = W.pitch_mid_frames(n, num, den)
        dev, host, st_dev, rs_host, comp, comp_host, info = [], [], [], [], [], [], None
        for i in range(a.repeats + 1):                         # alternating; the first round warms (tables, extents)
            info, h = timed(lambda: ctx.clip_pitch(SRC, DST, 0, n, n, num, den, a.quality, N, D))
            d = ctx.pitch_ms()
            if rate2:
                _, hs = timed(lambda: ctx.clip_stretch(SRC, TMP, 0, n, mid, N, D))
                s = ctx.stretch_ms()
                _, hr = timed(lambda: ctx.clip_resample(TMP, DST2, 0, mid, rate2, a.quality))
            if i:
                dev.append(d)
                host.append(h)
                if rate2:
                    st_dev.append(s), rs_host.append(hr), comp.append(s + hr), comp_host.append(hs + hr)
        r = {"ratio": name, "num": num, "den": den, "mid_frames": mid, "info": info, "device": fig(dev), "host": fig(host),
             "frames_per_s": n / (statistics.median(dev) * 1e-3)}
        r["times_real_time"] = r["frames_per_s"] / a.rate
        r["searched_over_steps"] = info["searched_steps"] / info["steps"]
        r["scored_terms"] = info["candidates"] * (N // 2)
        if rate2:
            r["composition"] = {"rate": rate2, "stretch_device": fig(st_dev), "resample_host": fig(rs_host), "sum": fig(comp),
                                "host": fig(comp_host), "temporary_bytes": mid * ch * 4}
            r["fused_over_composition"] = r["device"]["median_ms"] / r["composition"]["sum"]["median_ms"]
            r["composition_spread_ms"] = max(comp) - min(comp)
            r["fused_minus_composition_ms"] = r["device"]["median_ms"] - r["composition"]["sum"]["median_ms"]
        res.append(r)
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
