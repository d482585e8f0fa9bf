#!/usr/bin/env python3
"""Reading a clip along a position curve in numbers (MEASUREMENTS.md "Reading a clip along a position curve"): 2^24 stereo
output frames at the constant speed 147 / 160 (knot_shift 8), guard 1, WBX_SRC_GOOD, through wbx_clip_varispeed.  The call
is timed on the device between two events around its uploads and its launch (wbx_varispeed_ms) and on the host around the
whole call, which returns after its stream has drained.  In the same process, ALTERNATING with it, wbx_clip_resample
converts the same range of the same clip 44100 -> 48000 at GOOD — the same T = 48 taps and the same number of output frames
— timed on the host: its kernel is untouched by this call; it is the yardstick, not the code under test.
  ratio            the varispeed call's host time over the conversion's (expected: within 4 — twice the fma, and a
                   per-lane table row instead of a coalesced one)
  fma_per_s        2 T fp64 fmas per output frame and channel over the device time
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24, help="output frames")
    ap.add_argument("--quality", default="good")
    ap.add_argument("--knot-shift", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    ch, g = 2, a.knot_shift
    n = a.frames * 147 // 160                                    # the range whose conversion has a.frames output frames
    out = W.resample_frames(44100, 48000, n)
    ctx.clip_synth(1, "f32", ch, 44100, n, 0x7A5EED, 3, 0.5)
    G = 1 << g
    knots = np.array([((i * G * 147) << 32) // 160 for i in range((out + G - 1) // G + 1)], dtype=np.int64)
    plan = W.varispeed_plan(a.quality)
    tiles = W.varispeed_tiles(knots, g, n, out, a.quality)
    dev, host, conv = [], [], []
    for i in range(a.repeats + 1):                               # the first round warms (tables, stages, the pool's slabs)
        t0 = time.perf_counter()
        ctx.clip_varispeed(1, 2, 0, n, out, knots, g, a.quality)
        h = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.clip_resample(1, 3, 0, n, 48000, a.quality)
        r = 1e3 * (time.perf_counter() - t0)
        if i:
            dev.append(ctx.varispeed_ms()), host.append(h), conv.append(r)
    for k in (2, 3):
        ctx.L.wbx_clip_free(ctx.h, k)
    fmas = 2.0 * plan["T"] * out * ch
    res = {"source_frames": n, "out_frames": out, "channels": ch, "quality": a.quality, "knot_shift": g, "knots": len(knots),
           "plan": plan, "tiles": len(tiles), "span": max(t[3] for t in tiles), "device": ctx.device_info(),
           "varispeed_device": fig(dev), "varispeed_host": fig(host), "resample_host": fig(conv),
           "ratio": statistics.median(host) / statistics.median(conv),
           "ratio_device_over_resample_host": statistics.median(dev) / statistics.median(conv), "fmas": fmas,
           "fma_per_s": fmas / (statistics.median(dev) * 1e-3)}
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
