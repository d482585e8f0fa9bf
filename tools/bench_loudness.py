#!/usr/bin/env python3
"""Measuring a clip's loudness in numbers (MEASUREMENTS.md "Loudness"): stereo F32 clips of 10 s, 10 min and 60 min at 48 kHz
measured through wbx_clip_loudness without and with the true peak (L, LT), each call timed on the host from entry to return
(the call waits for its result and runs the gate; the 4x table is on the device after the warm-up call), against
  M  wbx_clip_measure of the same range: the existing one-pass reader — what reading the range once costs through the same
     stream and ordering
frames/s are source frames over the median; GB/s are algorithmic bytes over the median: the range read once (the K filter's
two hops of run-in per hop, which triple its reads, and the peak tiles' overlapping spans are not counted).  L is bound by the
latency of its fp64 recurrence, not by bandwidth: its GB/s says how far from a streaming read it is, not how well it streams.
Order L LT M M LT L per repeat, median and spread.  One JSON line.  No speed is asserted anywhere."""
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
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 600.0, 3600.0])
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ch = 2
    ctx = W.MixContext(4, block=512)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    def fig(v, b, frames):
        med = statistics.median(v)
        return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v), "bytes": b,
                "frames_per_s": frames / med, "GBps": b / med / 1e9}

    results = []
    for i, sec in enumerate(a.seconds):
        n, clip = int(round(sec * a.rate)), 1 + i
        ctx.clip_synth(clip, "f32", ch, a.rate, n, 0x10AD + i, 0, 0.25)
        ctx.sync()
        last = {}
        steps = {"L": lambda: last.update(L=ctx.clip_loudness(clip, ch, a.rate, 0, n)),
                 "LT": lambda: last.update(LT=ctx.clip_loudness(clip, ch, a.rate, 0, n, true_peak=True)),
                 "M": lambda: last.update(M=ctx.clip_measure(clip, ch, 0, n))}
        for f in steps.values():   # warm: stream, table, buffers
            timed(f)
        t = {k: [] for k in steps}
        for _ in range(a.repeats):
            for k in list(steps) + list(steps)[::-1]:
                t[k].append(timed(steps[k]))
        res = {k: fig(t[k], n * ch * 4, n) for k in steps}
        res["L_over_M"] = res["L"]["median_ms"] / res["M"]["median_ms"]
        res["LT_over_M"] = res["LT"]["median_ms"] / res["M"]["median_ms"]
        res["times_real_time_L"] = sec / (res["L"]["median_ms"] * 1e-3)
        lt = last["LT"]
        results.append({"seconds": sec, "frames": n, "hops": lt["hops"], "integrated": lt["integrated"], "range_lu": lt["range_lu"],
                        "true_peak": [float(p) for p in lt["true_peak"]], "sample_peak": [float(p) for p in last["M"]["peak"]],
                        "results": res})
        ctx.L.wbx_clip_free(ctx.h, clip)
    out = {"rate": a.rate, "channels": ch, "device": ctx.device_info(), "clips": results}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
