#!/usr/bin/env python3
"""Converting a clip's sample rate in numbers (MEASUREMENTS.md "Converting a clip's sample rate"): a stereo F32 clip of 2^24
frames at 44.1 kHz converted to 48 kHz through wbx_clip_resample at each quality (FAST / GOOD / BEST: 24 / 48 / 96 taps),
each call timed on the host from entry to return (the call waits for its result; the coefficient table is on the device
after the warm-up call), against
  D  wbx_clip_derive of the same clip, whole, forward, gain only: one read and one write of HBM through the same stream,
     ordering and allocation path — the bandwidth yardstick a conversion would meet if its arithmetic were free
frames/s are OUTPUT frames over the median; GB/s are algorithmic bytes over the median: the source range read once plus the
result written once (the table and the tiles' overlapping source spans are not counted).  Order A B C D D C B A per repeat,
median and spread.  One JSON line.  No speed is asserted anywhere."""
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
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--src-rate", type=int, default=44100)
    ap.add_argument("--dst-rate", type=int, default=48000)
    a = ap.parse_args()
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    n, ch = a.frames, 2
    n_out = W.resample_frames(a.src_rate, a.dst_rate, n)
    assert n_out, "the library refuses this conversion"
    ctx = W.MixContext(4, block=512)
    src, dst = 1, 2                                          # the results replace each other in `dst`
    ctx.clip_synth(src, "f32", ch, a.src_rate, n, 0x5AC, 0, 0.7)
    ctx.sync()
    copy = W.edit_desc(0, n, False, "keep", 0.5)
    steps = {q: (lambda q=q: ctx.clip_resample(src, dst, 0, n, a.dst_rate, q), (n + n_out) * ch * 4, n_out) for q in ("fast", "good", "best")}
    steps["D_derive"] = (lambda: ctx.clip_derive(src, dst, copy), 2 * n * ch * 4, n)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    for f, _, _ in steps.values():   # warm: stream, tables, the pool's extents for the results
        timed(f)
    t = {k: [] for k in steps}
    for _ in range(a.repeats):
        for k in list(steps) + list(steps)[::-1]:
            t[k].append(timed(steps[k][0]))

    def fig(v, b, frames):
        med = statistics.median(v)
        return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v), "bytes": b,
                "frames_per_s": frames / med, "GBps": b / med / 1e9}

    res = {k: fig(t[k], steps[k][1], steps[k][2]) for k in steps}
    for q in ("fast", "good", "best"):
        res[q]["plan"] = W.resample_plan(a.src_rate, a.dst_rate, q)
        res[q + "_over_D"] = res[q]["median_ms"] / res["D_derive"]["median_ms"]
    out = {"frames": n, "frames_out": n_out, "channels": ch, "src_rate": a.src_rate, "dst_rate": a.dst_rate,
           "device": ctx.device_info(), "results": res}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
