#!/usr/bin/env python3
"""Editing clips in numbers (MEASUREMENTS.md "Editing clips", profiles/clipfx_2p24.json): a stereo F32 clip of 2^24 frames
(128 MiB) measured, derived forward, derived reversed (both with gain and two fades of 2^16 frames) through layer 1 and
normalized through wbx_engine_normalize_sample (its new sample is deleted again outside the timed part), each call timed on
the host from entry to return (the calls wait for their result), against
  H  download + host edit + upload   the only route before: wbx_clip_download per channel, the numpy model's arithmetic
                                     for the REVERSED edit (reverse, gain, fades), wbx_clip_upload of the result; the
                                     forward edit has no host twin here: it is the same trips and arithmetic less the flip
  Y  a device copy of the same bytes  torch: 128 MiB read + 128 MiB written, the yardstick a one-read-one-write pass has
GB/s are algorithmic bytes over the median: read for measure, read + write for a derive, two reads + one write for normalize.
Order A B B A per repeat, median and spread.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host-route", action="store_true", help="leave route H out (profiling runs)")
    a = ap.parse_args()
    import torch   # first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import numpy as np
    import whitebox_amd as W
    from whitebox_amd.engine import Engine
    import clipfx_model as M

    n, ch, fade = a.frames, 2, min(1 << 16, a.frames)
    eng = Engine(4, buffer_size=512)
    ctx = eng.ctx
    src = eng.add_sample_synth("f32", ch, 48000, n, 0xC11F, 0, 0.7)
    ctx.sync()
    dst = src + 1                                            # layer 1's results replace each other here
    nbytes = n * ch * 4
    fwd = W.edit_desc(0, n, False, "keep", 0.5, fade, fade, "smooth", "smooth")
    rev = W.edit_desc(0, n, True, "keep", 0.5, fade, fade, "smooth", "smooth")

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        dt = time.perf_counter() - t0
        while made:
            eng.delete_sample(made.pop())
        return dt, r

    def derive(desc):
        ctx.clip_derive(src, dst, desc)

    made = []

    def normalize():
        made.append(eng.normalize_sample(src, 0.5, n_frames=n)[0])

    def host_route():
        planes = [ctx.clip_download(src, c, n, np.float32) for c in range(ch)]
        out = M.derive(planes, 0, n, True, M.KEEP, 0.5, fade, fade, M.SMOOTH, M.SMOOTH)
        ctx.clip_upload(dst, "f32", 48000, out)

    dev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dev2 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def yard():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev2.copy_(dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    steps = {"measure": (lambda: ctx.clip_measure(src, ch, 0, n), nbytes), "derive_forward": (lambda: derive(fwd), 2 * nbytes),
             "derive_reversed": (lambda: derive(rev), 2 * nbytes), "normalize": (normalize, 3 * nbytes)}
    for f, _ in steps.values():   # warm: stream, statistics block, the pool's extents for the results
        timed(f)
    yard()
    t = {k: [] for k in list(steps) + ["Y", "H"]}
    for _ in range(a.repeats):
        for k in list(steps) + list(steps)[::-1]:
            t[k].append(timed(steps[k][0])[0])
        t["Y"].append(yard())
        if not a.no_host_route:
            t["H"].append(timed(host_route)[0])

    def fig(v, b):
        med = statistics.median(v)
        return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v), "bytes": b, "GBps": b / med / 1e9}

    res = {k: fig(t[k], steps[k][1]) for k in steps}
    res["Y_device_copy"] = fig(t["Y"], 2 * nbytes)
    if t["H"]:
        res["H_download_host_edit_upload"] = fig(t["H"], 2 * nbytes)
        res["derive_reversed_over_H"] = res["derive_reversed"]["median_ms"] / res["H_download_host_edit_upload"]["median_ms"]
    res["derive_forward_over_Y"] = res["derive_forward"]["median_ms"] / res["Y_device_copy"]["median_ms"]
    res["derive_reversed_over_forward"] = res["derive_reversed"]["median_ms"] / res["derive_forward"]["median_ms"]
    out = {"frames": n, "channels": ch, "source_bytes": nbytes, "fade_frames": fade, "device": ctx.device_info(), "results": res}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
