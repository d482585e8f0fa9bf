#!/usr/bin/env python3
"""Finding a clip's onsets and tempo in numbers (MEASUREMENTS.md "Finding a clip's onsets and tempo"): a stereo F32 clip of
2^24 frames at 48 kHz (noise bursts over a tone) through wbx_clip_onsets at H in {64, 256, 320, 4096}, and a 5-minute clip
through wbx_clip_tempo.
  energy     device milliseconds between two events around onset_energy_kernel's launch (wbx_onset_ms) and the range's bytes
             over them: the pass's read rate
  onsets     host milliseconds around the whole wbx_clip_onsets call: both passes, the wait, the copy of the records, the pick
  measure    host milliseconds around wbx_clip_measure of the same range — the project's existing read-once kernel — which
             has no device timer: a whole call, wait and the copy of its statistics included.  Its bytes over that time is a
             LOWER bound of its kernel's read rate
  tempo      host milliseconds around a whole wbx_clip_tempo call (H = 256, windows of 1024 hops every 64, lags 56 .. 188), and
             of that the energy pass (wbx_onset_ms) and the f0 launches over the novelty (wbx_f0_ms)
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
        env = np.where((i + 1000 * c) % 24000 < 3000, 0.5, 0.01)   # a burst every half second: 120 bpm at 48 kHz
        planes.append((env * rng.standard_normal(n) + 0.05 * np.sin(2 * np.pi * i / (91.3 + c))).astype(np.float32))
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--hops", type=int, nargs="+", default=[64, 256, 320, 4096])
    ap.add_argument("--tempo-seconds", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rate", type=int, default=48000)
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    n, ch = a.frames, a.channels
    nbytes = n * ch * 4
    ctx.clip_upload(1, "f32", a.rate, material(np, ch, n, 0x0A5E))
    out = {"frames": n, "channels": ch, "rate": a.rate, "bytes": nbytes, "device": ctx.device_info()}
    res = []
    for H in a.hops:
        dev, host, meas, info = [], [], [], None
        for i in range(a.repeats + 1):                          # the first round warms (the stage's buffers)
            t0 = time.perf_counter()
            _, info = ctx.clip_onsets(1, 0, n, H)
            t1 = time.perf_counter()
            ctx.clip_measure(1, ch, 0, n)
            t2 = time.perf_counter()
            if i:
                dev.append(ctx.onsets_ms()), host.append(1e3 * (t1 - t0)), meas.append(1e3 * (t2 - t1))
        ms, mm = statistics.median(dev), statistics.median(meas)
        res.append({"hop": H, "q": H // 64, "info": info, "energy": fig(dev), "energy_GBps": nbytes / (ms * 1e-3) / 1e9,
                    "onsets": fig(host), "measure": fig(meas), "measure_GBps_at_least": nbytes / (mm * 1e-3) / 1e9})
    out["results"] = res
    tn = int(a.tempo_seconds * a.rate)
    ctx.clip_upload(2, "f32", a.rate, material(np, ch, tn, 0x7E0))
    host, energy, track, info, rec = [], [], [], None, None
    for i in range(a.repeats + 1):
        t0 = time.perf_counter()
        rec, info = ctx.clip_tempo(2, 0, tn, 256, 1e-9, 1024, 64, 56, 188, 0.5)
        t1 = time.perf_counter()
        if i:
            host.append(1e3 * (t1 - t0)), energy.append(ctx.onsets_ms()), track.append(ctx.f0_ms())
    voiced = rec["period"][rec["voiced"] != 0]
    out["tempo"] = {"frames": tn, "seconds": a.tempo_seconds, "info": info, "call": fig(host), "energy": fig(energy), "f0": fig(track),
                    "bpm": 60.0 * a.rate / (256 * float(np.median(voiced))) if voiced.size else None}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
