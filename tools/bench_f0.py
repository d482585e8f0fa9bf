#!/usr/bin/env python3
"""Tracking a clip's pitch in numbers (MEASUREMENTS.md "Tracking a clip's pitch"): stereo F32 clips of 2^22 and 2^24 frames at
48 kHz (a few sines and noise) through wbx_clip_f0 with W in {1024, 2048}, tau_max in {511, 1023, 4095}, tau_min = 24,
H = 512 and a threshold of 0.15.  Each call is timed on the device between two events around its launches (wbx_f0_ms) and on
the host around the whole call, which ends in a wait for the device and the copy of the records.
  terms_per_s      hops * W * (tau_max + 1) over the device time
  times_real_time  the range's seconds over the device time
  epilogue_share   what of the device time does not grow with the window: the two windows of a (frames, tau_max) pair give
                   a line t(W); its value at W = 0 — staging the lags' part of the span, the per-hop epilogue, the launches
                   — over t(W)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1 << 22, 1 << 24])
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--windows", type=int, nargs=2, default=[1024, 2048])
    ap.add_argument("--tau-max", type=int, nargs="+", default=[511, 1023, 4095])
    ap.add_argument("--tau-min", type=int, default=24)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--threshold", type=float, default=0.15)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    L = W.lib()
    out = {"channels": a.channels, "rate": a.rate, "hop": a.hop, "tau_min": a.tau_min, "threshold": a.threshold,
           "launch_terms": int(L.wbx_f0_launch_terms()), "device": ctx.device_info()}
    res = []
    for n in a.frames:
        ctx.clip_upload(1, "f32", a.rate, material(np, a.channels, n, 0xF0 + a.channels))
        for tau_max in a.tau_max:
            pair = []
            for Wn in a.windows:
                dev, host, info = [], [], None
                for i in range(a.repeats + 1):                 # the first round warms (the record buffers)
                    t0 = time.perf_counter()
                    _, info = ctx.clip_f0(1, 0, n, Wn, a.hop, a.tau_min, tau_max, a.threshold)
                    h = 1e3 * (time.perf_counter() - t0)
                    if i:
                        dev.append(ctx.f0_ms()), host.append(h)
                ms = statistics.median(dev)
                r = {"frames": n, "window": Wn, "tau_max": tau_max, "info": info, "launch_hops": int(L.wbx_f0_launch_hops(Wn, tau_max)),
                     "device": fig(dev), "host": fig(host), "terms_per_s": info["terms"] / (ms * 1e-3),
                     "times_real_time": (n / a.rate) / (ms * 1e-3), "ms_per_launch": ms / info["launches"]}
                pair.append(r)
            (w1, t1), (w2, t2) = [(r["window"], r["device"]["median_ms"]) for r in pair]
            at0 = t1 - (t2 - t1) * w1 / (w2 - w1)
            for r in pair:
                r["epilogue_share"] = at0 / r["device"]["median_ms"]
            res += pair
    out["results"] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
