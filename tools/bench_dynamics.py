#!/usr/bin/env python3
"""Dynamics of a clip in numbers (MEASUREMENTS.md "Dynamics of a clip"), the twin of tools/bench_limit.py: F32 clips of
2^24 frames at 48 kHz through wbx_clip_dynamics with ramps of 48 000 terms (look-ahead 72 frames, no hold, the rest
release), mono and stereo, in both senses, keyed by the clip itself and by a second clip, on two kinds of material:
  dense   noise of +-0.7 through a table no level of which is at rest (compress: threshold -60 dB; gate: threshold 0 dB, no
          floor): every segment of the ramp is walked
  music   noise of +-0.1 with a burst of 64 samples of +-0.9 every half second (compress: threshold -12 dB; gate: threshold
          -14 dB, 10:1, floor -40 dB): the noise is at rest in both senses, a segment is walked only where its staged span
          holds a burst, most are skipped by the vote
Each call is timed on the device between two events around its launches (wbx_dynamics_ms); terms per second are
n_frames * (A + H + R), the interface's count, over that time.  Beside every figure, in the same process and ALTERNATING
with it call by call, wbx_clip_limit on the same material with the same ramp (wbx_limit_ms; dense: ceiling 0.001, music:
ceiling 0.5): the limiter's kernels are what the dynamics kernels are shaped after, and the compress sense runs their
instruction mix.  --spread N first repeats the dense mono limiter N times: the run-to-run spread the comparison is read
against.  --cap adds one dense mono call at the work cap (2^24 frames x 2^20 terms = 2^44) in each sense.
One JSON line.  No speed is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 1 << 44
LOOKAHEAD = 72


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--terms", type=int, nargs="*", default=[48000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--spread", type=int, default=0, metavar="N")
    ap.add_argument("--cap", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import whitebox_amd as W

    rate, n = a.rate, a.frames
    ctx = W.MixContext(4, block=512)
    SRC, KEYC, DST = 1, 3, 9                                   # the results replace each other in DST
    tables = {("dense", "compress"): W.dynamics_table("compress", -60.0, 4.0, 0.0), ("dense", "gate"): W.dynamics_table("gate", 0.0, 2.0, 0.0),
              ("music", "compress"): W.dynamics_table("compress", -12.0, 4.0, 6.0), ("music", "gate"): W.dynamics_table("gate", -14.0, 10.0, 0.0, -40.0)}
    ceilings = {"dense": 0.001, "music": 0.5}
    out = {"rate": rate, "frames": n, "lookahead": LOOKAHEAD, "device": ctx.device_info()}

    def limit(terms, kind):
        ctx.clip_limit(SRC, DST, 0, n, ceilings[kind], 1.0, LOOKAHEAD, 0, terms - LOOKAHEAD)
        return ctx.limit_ms()

    def dynamics(terms, kind, sense, keyed):
        ds = ctx.clip_dynamics(SRC, DST, 0, n, tables[(kind, sense)], sense, KEYC if keyed else None, 0, 1.0, 1.0, 1.0, LOOKAHEAD, 0,
                               terms - LOOKAHEAD)
        return ctx.dynamics_ms(), ds["reduced_frames"]

    if a.spread:
        ctx.clip_upload(SRC, "f32", rate, material(np, "dense", 1, n, rate, 0xD1A + 1))
        terms = a.terms[0]
        limit(terms, "dense")                                  # warm
        ms = [limit(terms, "dense") for _ in range(a.spread)]
        out["limiter_spread"] = {"terms": terms, "device": fig(ms), "terms_per_s": [n * terms / (m * 1e-3) for m in ms]}
    res = []
    for ch in (1, 2):
        for kind in ("dense", "music"):
            ctx.clip_upload(SRC, "f32", rate, material(np, kind, ch, n, rate, 0xD1A + ch))
            ctx.clip_upload(KEYC, "f32", rate, material(np, kind, 3 - ch, n, rate, 0x4E1 + ch))   # the key has the other channel count
            for terms in a.terms:
                if n * terms > CAP:
                    continue
                for sense in ("compress", "gate"):
                    for keyed in (False, True):
                        lim, dyn, reduced = [], [], 0
                        for i in range(a.repeats + 1):         # alternating; the first pair warms
                            l = limit(terms, kind)
                            d, reduced = dynamics(terms, kind, sense, keyed)
                            if i:
                                lim.append(l)
                                dyn.append(d)
                        r = {"terms": terms, "channels": ch, "material": kind, "sense": sense, "keyed": keyed, "reduced_frames": reduced,
                             "device": fig(dyn), "limit_device": fig(lim)}
                        r["terms_per_s"] = n * terms / (r["device"]["median_ms"] * 1e-3)
                        r["limit_terms_per_s"] = n * terms / (r["limit_device"]["median_ms"] * 1e-3)
                        r["over_limit"] = r["terms_per_s"] / r["limit_terms_per_s"]
                        res.append(r)
    out["results"] = res
    if a.cap and n * (1 << 20) <= CAP:
        ctx.clip_upload(SRC, "f32", rate, material(np, "dense", 1, n, rate, 0xD1A + 1))
        out["at_the_cap"] = []
        for sense in ("compress", "gate"):
            ms, _ = dynamics(1 << 20, "dense", sense, False)
            out["at_the_cap"].append({"sense": sense, "terms": 1 << 20, "device_ms": ms, "terms_per_s": n * (1 << 20) / (ms * 1e-3)})
        out["at_the_cap"].append({"sense": "limit", "terms": 1 << 20, "device_ms": limit(1 << 20, "dense")})
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
