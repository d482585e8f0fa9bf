#!/usr/bin/env python3
"""Aligning two clips in numbers (MEASUREMENTS.md "Aligning two clips"): a stereo reference and a mono clip at 48 kHz (a few
sines and noise, the clip a delayed copy with noise of its own) through wbx_clip_align at (n, lags) = (2^16, 4097),
(2^20, 513) and (2^22, 2^17), the lags centred on zero.  Each call is timed on the device between two events around its
launches (wbx_align_ms) and on the host around the whole call, which ends in a wait for the device and the copy of info.
  terms_per_s      lags * n over the device time — to be read beside tools/bench_f0.py's figure for W = 1024, lags to 1023:
                   the turn is the same
  ms_per_launch    the device time over the call's launches (2 per band, and 2)
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
        for period, amp in ((218.2 + 11 * c, 0.4), (72.7, 0.2), (36.1 + c, 0.1)):
            v += amp * np.sin(2 * np.pi * i / period)
        planes.append(v.astype(np.float32))
    return planes


def shape(text):
    n, lags = (int(v) for v in text.split(":"))
    return n, lags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=shape, nargs="+", default=[(1 << 16, 4097), (1 << 20, 513), (1 << 22, 1 << 17)],
                    help="n:lags pairs")
    ap.add_argument("--delay", type=int, default=37)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    L = W.lib()
    out = {"rate": a.rate, "delay": a.delay, "chunk_frames": int(L.wbx_align_chunk_frames()), "device": ctx.device_info()}
    res = []
    for n, lags in a.shapes:
        lo = -(lags // 2)
        hi = lo + lags - 1
        m = n + hi
        ref = material(np, 2, n, 0xA1)
        mid = (0.5 * (ref[0].astype(np.float64) + ref[1])).astype(np.float32)
        rng = np.random.default_rng(0xA2)
        clip = (0.02 * rng.standard_normal(m)).astype(np.float32)
        clip[a.delay:a.delay + n] += mid[:m - a.delay]
        ctx.clip_upload(1, "f32", a.rate, ref)
        ctx.clip_upload(2, "f32", a.rate, [clip])
        dev, host, info = [], [], None
        for i in range(a.repeats + 1):                         # the first round warms (the stage)
            t0 = time.perf_counter()
            info, _ = ctx.clip_align(1, 0, n, 2, 0, m, lo, hi)
            h = 1e3 * (time.perf_counter() - t0)
            if i:
                dev.append(ctx.align_ms()), host.append(h)
        ms = statistics.median(dev)
        res.append({"n": n, "lags": lags, "info": info, "band_chunks": int(L.wbx_align_band_chunks(lags)), "device": fig(dev),
                    "host": fig(host), "terms_per_s": info["terms"] / (ms * 1e-3), "ms_per_launch": ms / info["launches"]})
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
