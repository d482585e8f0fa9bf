#!/usr/bin/env python3
"""Filtering a clip in numbers (MEASUREMENTS.md "Filtering a clip"): a stereo F32 clip of 2^24 frames at 48 kHz through
wbx_clip_filter with cascades of 1, 4 and 8 stages (the first a 20 Hz high-pass), each call timed on the host from entry to
return (the call waits for its result), and its three launches timed on the device between events (wbx_filter_phase_ms):
the zero-state runs, the serial carry over the chunks, the runs from the carried states — against
  D  wbx_clip_derive of the same clip, whole, forward, gain only: one read and one write of HBM through the same stream,
     ordering and allocation path — the bandwidth yardstick a filter would meet if its recurrence were free
frames/s are frames over the median; the carry's time is also given per chunk of 512 frames, which is what its one wave
spends on one step of its serial walk.  Order A B C D D C B A per repeat, median and spread.  One JSON line.  No speed is
asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("state", "carry", "apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    n, ch, rate = a.frames, 2, a.rate
    kinds = [("highpass", 20.0, 0.7071067811865476, 0.0), ("peak", 1000.0, 8.0, 12.0), ("peak", 60.0, 30.0, -20.0),
             ("lowpass", 0.4 * rate, 0.7071067811865476, 0.0), ("lowshelf", 120.0, 0.8, 6.0), ("notch", 50.0, 12.0, 0.0),
             ("highshelf", 0.2 * rate, 0.7, -6.0), ("allpass", 300.0, 2.0, 0.0)]
    coef = [W.filter_design(rate, k, f, q, g) for k, f, q, g in kinds]
    ctx = W.MixContext(4, block=512)
    src, dst = 1, 2                                          # the results replace each other in `dst`
    ctx.clip_synth(src, "f32", ch, rate, n, 0xF117, 0, 0.7)
    ctx.sync()
    copy = W.edit_desc(0, n, False, "keep", 0.5)
    chunks = -(-n // int(W.lib().wbx_filter_chunk_frames()))
    phase = {}

    def filt(S):
        ctx.clip_filter(src, dst, 0, n, coef[:S])
        phase.setdefault(S, []).append(ctx.filter_phase_ms())

    steps = {"S%d" % S: (lambda S=S: filt(S)) for S in (1, 4, 8)}
    steps["D_derive"] = lambda: ctx.clip_derive(src, dst, copy)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    for f in steps.values():         # warm: stream, stage buffers, the pool's extents for the results
        timed(f)
    phase.clear()
    t = {k: [] for k in steps}
    for _ in range(a.repeats):
        for k in list(steps) + list(steps)[::-1]:
            t[k].append(timed(steps[k]))

    def fig(v):
        med = statistics.median(v)
        return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v), "frames_per_s": n / med}

    res = {k: fig(t[k]) for k in steps}
    res["D_derive"]["GBps"] = 2 * n * ch * 4 / (res["D_derive"]["median_ms"] * 1e-3) / 1e9
    for S in (1, 4, 8):
        r = res["S%d" % S]
        for i, name in enumerate(PHASES):
            ms = [p[i] for p in phase[S]]
            med = statistics.median(ms)
            r[name] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "frames_per_s": n / (med * 1e-3) if med else None}
        r["carry"]["us_per_chunk"] = 1e3 * r["carry"]["median_ms"] / max(1, chunks - 1)
        r["over_D"] = r["median_ms"] / res["D_derive"]["median_ms"]
    out = {"frames": n, "channels": ch, "rate": rate, "chunks": chunks, "device": ctx.device_info(), "results": res}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
