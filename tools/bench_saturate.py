#!/usr/bin/env python3
"""Saturating a clip in numbers (MEASUREMENTS.md "Saturating a clip"): a stereo clip of 2^24 frames at 48 kHz (a few sines and
noise) through wbx_clip_saturate with a tanh table at os = 2 / 4 / 8, WBX_SRC_GOOD.  The fused call is timed on the device
between two events around its launches (wbx_saturate_ms) and on the host around the whole call, which returns after its
stream has drained.  In the same process the two existing wbx_clip_resample calls of the same material — up to rate * os,
back to rate — are timed on the host: their kernels are untouched by the fused call; they are the yardstick, not the code
under test.
  ratio            the fused call's host time over the two conversions' together (the target: at most 1)
  fma_per_s        2 Z os (2 + 2 Z / tile) fp64 fmas per frame and channel over the device time
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fig(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def material(np, channels, n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    planes = []
    for c in range(channels):
        v = 0.1 * rng.standard_normal(n)
        for period, amp in ((218.2 + 11 * c, 0.4), (72.7, 0.2), (13.7 + c, 0.1)):
            v += amp * np.sin(2 * np.pi * i / period)
        planes.append(v.astype(np.float32))
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--os", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--quality", default="good")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W
    from whitebox_amd import _ffi

    ctx = W.MixContext(4, block=512)
    n, ch = a.frames, 2
    ctx.clip_upload(1, "f32", a.rate, material(np, ch, n, 0x5A))
    tab = W.saturate_table("tanh", 0.1)
    Z = {0: 12, 1: 24, 2: 48}[_ffi.SRC_QUALITY.get(a.quality, a.quality)]
    out = {"rate": a.rate, "frames": n, "channels": ch, "quality": a.quality, "device": ctx.device_info()}
    res = []
    for os_ in a.os:
        shape = W.saturate_launch_shape(os_, a.quality, ch, n)
        dev, host, up, down, stats = [], [], [], [], None
        for i in range(a.repeats + 1):                         # the first round warms (tables, stages, the pool's slabs)
            t0 = time.perf_counter()
            stats = ctx.clip_saturate(1, 2, 0, n, tab, os=os_, quality=a.quality, drive=2.0, makeup=0.8)
            h = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.clip_resample(1, 3, 0, n, a.rate * os_, a.quality)
            u = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.clip_resample(3, 4, 0, n * os_, a.rate, a.quality)
            d = 1e3 * (time.perf_counter() - t0)
            if i:
                dev.append(ctx.saturate_ms()), host.append(h), up.append(u), down.append(d)
        for k in (2, 3, 4):
            ctx.L.wbx_clip_free(ctx.h, k)
        fmas = 2.0 * Z * os_ * (2.0 + 2.0 * Z / shape["tile"]) * n * ch
        two = statistics.median(up) + statistics.median(down)
        res.append({"os": os_, "shape": shape, "stats": stats, "device": fig(dev), "host": fig(host), "resample_up": fig(up),
                    "resample_down": fig(down), "two_calls_ms": two, "ratio": statistics.median(host) / two, "fmas": fmas,
                    "fma_per_s": fmas / (statistics.median(dev) * 1e-3)})
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
