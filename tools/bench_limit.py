#!/usr/bin/env python3
"""Limiting a clip in numbers (MEASUREMENTS.md "Limiting a clip"): F32 clips of 2^20 and 2^24 frames at 48 kHz through
wbx_clip_limit with ramps of 4800, 48 000 and 2^20 terms (look-ahead 72 frames, no hold, the rest release), mono and stereo,
on two kinds of material:
  dense   noise of +-0.7 under a ceiling of 0.001: every frame is limited, every segment of the ramp is walked
  music   noise of +-0.1 with a burst of 64 samples of +-0.9 every half second under a ceiling of 0.5: a segment is walked
          only where its staged span holds a burst, most are skipped by the vote
Each call is timed on the host from entry to return (it waits for its result) and on the device between two events around
its launches (wbx_limit_ms).  terms per second are n_frames * (A + H + R) — the interface's count, which also charges the
terms that reach outside the range or that a skipped segment never computes — over the device time; a term is one fp64
addition and one fp64 minimum.  Beside them, in the same run
  D      wbx_clip_derive of the same clip, whole, forward, gain only: the bandwidth yardstick
  C      wbx_clip_convolve of the same clip with a response of as many taps as the ramp has terms (tools/bench_convolve.py's
         measurement: multiply-adds per second over wbx_convolve_ms), and the ratio terms/s : multiply-adds/s
The dense mono call of 2^24 frames with 2^20 terms IS a call at the work cap (2^44 terms).
  --beside  the callback's block time (wbx_engine_process on an audio thread, host time per block) alone and with
         wbx_engine_limit_sample calls running beside it (16 384 terms, dense, over 2^22 stereo frames)
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

CAP = 1 << 44
LOOKAHEAD = 72


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def fig(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "n": len(v)}


def material(np, kind, channels, n, rate, seed):
    rng = np.random.default_rng(seed)
    if kind == "dense":
        return [rng.uniform(-0.7, 0.7, n).astype(np.float32) for _ in range(channels)]
    planes = [rng.uniform(-0.1, 0.1, n).astype(np.float32) for _ in range(channels)]
    for p in planes:
        for at in range(rate // 4, n - 64, rate // 2):
            p[at:at + 64] *= np.float32(9.0)
    return planes


def beside(W, np, blocks):
    from whitebox_amd import synth
    from whitebox_amd.engine import build_engine
    spec = synth.make_session("limitbench", 32, n_blocks=blocks, block=512, seed=0x11417B)
    FR = 1 << 22
    planes = material(np, "dense", 2, FR, spec.sample_rate, 7)
    out = {}
    for mode in ("alone", "limit", "limit", "alone"):
        eng = build_engine(spec, max_blocks=1)
        big = eng.add_sample("f32", spec.sample_rate, planes)
        stop, calls = threading.Event(), [0]

        def editor():
            while not stop.is_set():
                new, _ = eng.limit_sample(big, ceiling_db=-60.0, shape=(LOOKAHEAD, 0, (1 << 14) - LOOKAHEAD))
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
    return {"tracks": 32, "block": 512, "frames_beside": FR, "terms_beside": 1 << 14, "runs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1 << 20, 1 << 24])
    ap.add_argument("--terms", type=int, nargs="*", default=[4800, 48000, 1 << 20])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--beside", type=int, default=0, metavar="BLOCKS")
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    rate = a.rate
    ctx = W.MixContext(4, block=512)
    SRC, IRC, DST = 1, 3, 9                                   # the results replace each other in DST
    res = []
    for n in a.frames:
        convolve = {}                                         # mono, on the dense clip: what the mono rows are set against
        for ch in (1, 2):
            for kind, ceiling in (("dense", 0.001), ("music", 0.5)):
                ctx.clip_upload(SRC, "f32", rate, material(np, kind, ch, n, rate, 0x11417 + ch))
                copy = W.edit_desc(0, n, False, "keep", 0.5)
                ctx.clip_derive(SRC, DST, copy)               # warm
                derive = fig([1e3 * timed(lambda: ctx.clip_derive(SRC, DST, copy)) for _ in range(2 * a.repeats)])
                for terms in a.terms:
                    if n * terms > CAP:
                        continue
                    if terms not in convolve and ch == 1 and (n + terms - 1) * terms <= (1 << 46):
                        rng = np.random.default_rng(terms)
                        ctx.clip_upload(IRC, "f32", rate, [(rng.uniform(-1.0, 1.0, terms) * np.exp(-np.arange(terms) * 4.0 / terms)).astype(np.float32)])
                        dev = []
                        for i in range(a.repeats + 1):
                            ctx.clip_convolve(SRC, IRC, DST, 0, n, 0, terms)
                            if i:
                                dev.append(ctx.convolve_ms())
                        convolve[terms] = {"device": fig(dev), "madds_per_s": n * terms / (statistics.median(dev) * 1e-3)}
                    call, dev, ls = [], [], None
                    for i in range(a.repeats + 1):
                        t0 = time.perf_counter()
                        ls = ctx.clip_limit(SRC, DST, 0, n, ceiling, 1.0, LOOKAHEAD, 0, terms - LOOKAHEAD)
                        t = 1e3 * (time.perf_counter() - t0)
                        if i:                                 # the first call warms: the table's upload, the stage, the pool's extent
                            call.append(t)
                            dev.append(ctx.limit_ms())
                    r = {"frames": n, "terms": terms, "channels": ch, "material": kind, "limited_frames": ls["limited_frames"],
                         "call": fig(call), "device": fig(dev), "derive": derive}
                    r["terms_by_the_interface"] = n * terms
                    r["terms_per_s"] = n * terms / (r["device"]["median_ms"] * 1e-3)
                    r["over_derive"] = r["call"]["median_ms"] / derive["median_ms"]
                    if terms in convolve:
                        r["convolve_same_taps"] = convolve[terms]
                        r["terms_per_madd"] = r["terms_per_s"] / convolve[terms]["madds_per_s"]
                    res.append(r)
    out = {"rate": rate, "lookahead": LOOKAHEAD, "device": ctx.device_info(), "results": res}
    ctx.close()
    if a.beside:
        out["beside_the_callback"] = beside(W, np, a.beside)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
