#!/usr/bin/env python3
"""Seeing a clip's spectrum in numbers (MEASUREMENTS.md "Seeing a clip's spectrum"): a stereo F32 clip of 2^22 frames at
48 kHz (a few sines and noise) through wbx_clip_spectrum, channel mid, against Hann bases of logarithmically spaced bins at
(W, H, B) = (2048, 512, 1024), (8192, 2048, 256) and (256, 64, 64).  Each call is timed on the device between two events
around each of its launches, added up (wbx_spectrum_ms), and on the host around the whole call, which waits for the device
after every launch and copies the cells out.
  madds_per_s      hops * W * 2 B over the device time: the multiply-adds of the two chains of every cell
  times_real_time  the range's seconds over the device time
In the same run the yardstick: convolve_kernel's multiply-adds per second on the same device, from tools/bench_convolve.py
(2^20 frames, 96 000 taps, stereo) run as a child process once this one has closed its context — the same fma work per term.
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2048, 512, 1024), (8192, 2048, 256), (256, 64, 64)]


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
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("W", "H", "B"), help="default: the three of the docstring")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--no-convolve", action="store_true", help="leave the yardstick out")
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    ctx = W.MixContext(4, block=512)
    L = W.lib()
    n = a.frames
    out = {"frames": n, "channels": a.channels, "rate": a.rate, "launch_terms": int(L.wbx_spectrum_launch_terms()), "device": ctx.device_info()}
    ctx.clip_upload(1, "f32", a.rate, material(np, a.channels, n, 0x5BEC + a.channels))
    res = []
    for Wn, H, B in (a.shape or SHAPES):
        freqs, clamped = W.spectrum_log_freqs(20.0 / a.rate, B / 9.5, B)       # 20 Hz upwards over 9.5 octaves
        ctx.clip_upload(2, "f32", a.rate, [W.spectrum_basis(Wn, freqs, None, "hann")])
        dev, host, info = [], [], None
        for i in range(a.repeats + 1):                           # the first round warms (the stage buffers)
            t0 = time.perf_counter()
            _, info = ctx.clip_spectrum(1, 0, n, 2, Wn, B, H)
            h = 1e3 * (time.perf_counter() - t0)
            if i:
                dev.append(ctx.spectrum_ms()), host.append(h)
        ms = statistics.median(dev)
        madds = info["hops"] * Wn * 2 * B
        res.append({"window": Wn, "hop": H, "bins": B, "clamped": clamped, "info": info, "launch_hops": int(L.wbx_spectrum_launch_hops(Wn, B)),
                    "device": fig(dev), "host": fig(host), "madds": madds, "madds_per_s": madds / (ms * 1e-3),
                    "times_real_time": (n / a.rate) / (ms * 1e-3), "ms_per_launch": ms / max(info["launches"], 1)})
    out["results"] = res
    ctx.close()
    if not a.no_convolve:
        line = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "bench_convolve.py"), "--frames", str(1 << 20), "--taps", "96000",
                                        "--repeats", "3"], timeout=600).decode().strip().split("\n")[-1]
        conv = [r for r in json.loads(line)["results"] if r["channels"] == 2][0]
        out["convolve"] = {"frames": conv["frames"], "taps": conv["taps"], "channels": 2, "device": conv["device"], "madds_per_s": conv["madds_per_s"]}
        for r in res:
            r["of_convolve"] = r["madds_per_s"] / conv["madds_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
