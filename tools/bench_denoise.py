#!/usr/bin/env python3
"""Reducing a clip's noise in numbers (MEASUREMENTS.md "Reducing a clip's noise"): a stereo F32 clip of 2^24 frames at
48 kHz (a few sines over noise) through wbx_clip_denoise at W in {512, 1024, 2048}, S = 2, F = 1, floor 0.1, against the
threshold of a profile of its first second at strength 3.  Each call is timed on the device between two events around all
of its launches (wbx_denoise_ms) and on the host around the whole call.
  madds_per_s      hops * channels * 4 B W over the device time: the multiply-adds of the analysis' and the synthesis' chains
  times_real_time  the range's seconds over the device time
In the same run the yardstick: spectrum_kernel's multiply-adds per second at the same W, H = W / 4 and B = W / 2 bins (the
spectrum call takes at most 1024), from tools/bench_spectrum.py run as a child process once this one has closed its
context — the same product.  One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import subprocess
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
        v = 0.01 * rng.standard_normal(n)
        for period, amp in ((218.2 + 11 * c, 0.4), (72.7, 0.2), (36.1 + c, 0.1)):
            v[48000:] += amp * np.sin(2 * np.pi * i[48000:] / period)
        planes.append(v.astype(np.float32))
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--windows", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--smooth-hops", type=int, default=2)
    ap.add_argument("--smooth-bins", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--no-spectrum", action="store_true", help="leave the yardstick out")
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    n, ch = a.frames, a.channels
    out = {"frames": n, "channels": ch, "rate": a.rate, "smooth_hops": a.smooth_hops, "smooth_bins": a.smooth_bins, "device": ctx.device_info()}
    ctx.clip_upload(1, "f32", a.rate, material(np, ch, n, 0xDE01 + ch))
    res = []
    for Wn in a.windows:
        B = Wn // 2 + 1
        sums, hops = ctx.clip_denoise_profile(1, ch, 0, 48000, Wn)
        profile_ms = ctx.denoise_ms()
        thr = W.denoise_threshold(sums, hops, 3.0)
        dev, host, st = [], [], None
        for i in range(a.repeats + 1):                           # the first round warms (the tables, the stage buffers)
            t0 = time.perf_counter()
            st = ctx.clip_denoise(1, 2, 0, n, Wn, thr, floor=0.1, smooth_hops=a.smooth_hops, smooth_bins=a.smooth_bins)
            h = 1e3 * (time.perf_counter() - t0)
            if i:
                dev.append(ctx.denoise_ms()), host.append(h)
            else:
                first_host = h
        ms = statistics.median(dev)
        madds = st["hops"] * ch * 4 * B * Wn
        res.append({"window": Wn, "stats": st, "band_hops": W.denoise_band_hops(Wn, ch), "device": fig(dev), "host": fig(host),
                    "first_call_host_ms": first_host, "profile_of_a_second_ms": profile_ms, "madds": madds,
                    "madds_per_s": madds / (ms * 1e-3), "times_real_time": (n / a.rate) / (ms * 1e-3)})
    out["results"] = res
    ctx.close()
    if not a.no_spectrum:
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_spectrum.py"), "--no-convolve", "--repeats", "3"]
        for Wn in a.windows:
            cmd += ["--shape", str(Wn), str(Wn // 4), str(Wn // 2)]
        line = subprocess.check_output(cmd, timeout=600).decode().strip().split("\n")[-1]
        spec = {r["window"]: r for r in json.loads(line)["results"]}
        for r in res:
            s = spec[r["window"]]
            r["spectrum"] = {"bins": s["bins"], "hop": s["hop"], "device": s["device"], "madds_per_s": s["madds_per_s"]}
            r["of_spectrum"] = r["madds_per_s"] / s["madds_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
