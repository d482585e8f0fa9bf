#!/usr/bin/env python3
"""Convolving a clip in numbers (MEASUREMENTS.md "Convolving a clip"): F32 clips of 2^20 and 2^24 frames at 48 kHz through
wbx_clip_convolve with responses of 255, 4096, 96 000 and 2^20 taps (decaying noise), mono (1 x 1) and stereo (2 x 2), the
whole ring-out.  Each call is timed on the host from entry to return (it waits for its result) and on the device between
two events around its launches (wbx_convolve_ms).  multiply-adds per second are n_frames * taps * channels — the products of
a sample with a tap, each exactly once — over the device time; the interface's own count, out_frames * taps * channels,
also charges the taps that fall outside the range and that the kernel skips or adds as zeros.  Beside them
  D      wbx_clip_derive of the same clip, whole, forward, gain only: the bandwidth yardstick
  --cap  one call at the work cap, 2^46 multiply-adds by the interface's count: stereo, 2^20 taps, 2^25 output frames
  --beside  the callback's block time (wbx_engine_process on an audio thread, host time per block) alone, with
         wbx_engine_filter_sample calls running beside it (the yardstick: four stages over 2^22 stereo frames) and with
         wbx_engine_convolve_sample calls beside it (16 384 taps over the same frames)
A combination whose count would pass the cap is left out.  One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 1 << 46
FP64_CEILING = 256 * 64 * 2.4e9      # CUs x fp64 multiply-adds per clock x the published peak clock: 3.9e13 / s (unverified here)


def response(np, taps, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, taps) * np.exp(-np.arange(taps) * 4.0 / taps)).astype(np.float32)


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def fig(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def beside(W, np, blocks, rate):
    from whitebox_amd import synth
    from whitebox_amd.engine import build_engine
    spec = synth.make_session("convbench", 32, n_blocks=blocks, block=512, seed=0xC0417B)
    FR = 1 << 22
    rng = np.random.default_rng(7)
    planes = [rng.uniform(-0.5, 0.5, FR).astype(np.float32) for _ in range(2)]
    taps = response(np, 1 << 14, 9)
    coef = [W.filter_design(spec.sample_rate, "highpass", 20.0), W.filter_design(spec.sample_rate, "peak", 1000.0, 8.0, 12.0),
            W.filter_design(spec.sample_rate, "lowshelf", 120.0, 0.8, 6.0), W.filter_design(spec.sample_rate, "notch", 50.0, 12.0, 0.0)]
    out = {}
    for mode in ("alone", "filter", "convolve", "convolve", "filter", "alone"):
        eng = build_engine(spec, max_blocks=1)
        big = eng.add_sample("f32", spec.sample_rate, planes)
        room = eng.add_sample("f32", spec.sample_rate, [taps])
        stop, calls = threading.Event(), [0]

        def editor():
            while not stop.is_set():
                if mode == "filter":
                    new = eng.filter_sample(big, coef, tail_frames=0)
                else:
                    new = eng.convolve_sample(big, room, out_frames=FR)
                eng.delete_sample(new)
                calls[0] += 1

        buf = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        for _ in range(20):                                   # warm
            eng.process(None, buf, float(spec.sample_rate))
        th = threading.Thread(target=editor) if mode != "alone" else None
        if th:
            th.start()
            time.sleep(0.05)
        ms = []
        for _ in range(blocks - 20):
            ms.append(1e3 * timed(lambda: eng.process(None, buf, float(spec.sample_rate))))
        stop.set()
        if th:
            th.join()
        eng.close()
        ms.sort()
        r = out.setdefault(mode, {"blocks": 0, "calls_beside": 0, "median_ms": [], "p99_ms": [], "max_ms": []})
        r["blocks"] += len(ms)
        r["calls_beside"] += calls[0]
        r["median_ms"].append(statistics.median(ms))
        r["p99_ms"].append(ms[int(0.99 * (len(ms) - 1))])
        r["max_ms"].append(ms[-1])
    return {"tracks": 32, "block": 512, "frames_beside": FR, "taps_beside": 1 << 14, "stages_beside": 4, "runs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1 << 20, 1 << 24])
    ap.add_argument("--taps", type=int, nargs="*", default=[255, 4096, 96000, 1 << 20])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--cap", action="store_true")
    ap.add_argument("--beside", type=int, default=0, metavar="BLOCKS")
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    rate = a.rate
    ctx = W.MixContext(4, block=512)
    SRC, IRC, DST = {1: 1, 2: 2}, {1: 3, 2: 4}, 9           # the results replace each other in DST
    res = []
    for n in a.frames:
        for ch in (1, 2):
            ctx.clip_synth(SRC[ch], "f32", ch, rate, n, 0xC0417, 0, 0.7)
        ctx.sync()
        copy = W.edit_desc(0, n, False, "keep", 0.5)
        derive = {}
        for ch in (1, 2):
            ctx.clip_derive(SRC[ch], DST, copy)               # warm
            derive[ch] = fig([1e3 * timed(lambda: ctx.clip_derive(SRC[ch], DST, copy)) for _ in range(2 * a.repeats)])
        for taps in a.taps:
            for ch in (1, 2):
                if (n + taps - 1) * taps * ch > CAP:
                    continue
                ctx.clip_upload(IRC[ch], "f32", rate, [response(np, taps, 11 + k) for k in range(ch)])
                call, dev = [], []
                for i in range(a.repeats + 1):
                    t = 1e3 * timed(lambda: ctx.clip_convolve(SRC[ch], IRC[ch], DST, 0, n, 0, taps))
                    if i:                                     # the first call warms: stage buffer, the pool's extent
                        call.append(t)
                        dev.append(ctx.convolve_ms())
                r = {"frames": n, "taps": taps, "channels": ch, "call": fig(call), "device": fig(dev), "derive": derive[ch]}
                r["madds"] = n * taps * ch
                r["madds_by_the_interface"] = (n + taps - 1) * taps * ch
                r["madds_per_s"] = r["madds"] / (r["device"]["median_ms"] * 1e-3)
                r["of_fp64_ceiling"] = r["madds_per_s"] / FP64_CEILING
                r["over_derive"] = r["call"]["median_ms"] / derive[ch]["median_ms"]
                res.append(r)
    out = {"rate": rate, "fp64_ceiling_madds_per_s": FP64_CEILING, "device": ctx.device_info(), "results": res}
    if a.cap:
        taps, n_out = 1 << 20, 1 << 25
        n = n_out - taps + 1
        ctx.clip_synth(SRC[2], "f32", 2, rate, n, 0xCA9, 0, 0.7)
        ctx.sync()
        ctx.clip_upload(IRC[2], "f32", rate, [response(np, taps, 21 + k) for k in range(2)])
        t = 1e3 * timed(lambda: ctx.clip_convolve(SRC[2], IRC[2], DST, 0, n, 0, taps))
        dev = ctx.convolve_ms()
        out["at_the_cap"] = {"frames": n, "taps": taps, "channels": 2, "out_frames": n_out, "madds_by_the_interface": n_out * taps * 2,
                             "madds": n * taps * 2, "call_ms": t, "device_ms": dev, "madds_per_s": n * taps * 2 / (dev * 1e-3)}
    ctx.close()
    if a.beside:
        out["beside_the_callback"] = beside(W, np, a.beside, rate)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
