#!/usr/bin/env python3
"""Splicing clips in numbers (MEASUREMENTS.md "Splicing clips"): two stereo F32 clips of 2^24 frames (128 MiB each) in one
process, each call timed on the host from entry to return (the calls wait for their result):
  a  clip_derive with KEEP, gain 1, no fade      the unchanged baseline: one read, one write of the same bytes as b
  b  a one-part splice of the same range
  c  a two-part join with a 4096-frame crossfade (two sources read, 2n - 4096 frames written)
  d  a 64-part comp: parts of n / 64 frames taken in turn from the two sources, each 256 frames longer than its slot and
     faded over that overlap (n frames written)
  e  what c costs without the call: wbx_clip_download per source and channel, the numpy model's arithmetic,
     wbx_clip_upload of the result
GB/s are algorithmic bytes (every source frame of a part read once, every output frame written once) over the median.
Order a b c d d c b a per repeat, median and spread.  One JSON line."""
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
    ap.add_argument("--no-host-route", action="store_true", help="leave route e out (profiling runs)")
    a = ap.parse_args()
    import torch   # noqa: F401  first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import numpy as np
    import whitebox_amd as W
    from whitebox_amd.engine import Engine
    import splice_model as S

    n, ch, xf, lap = a.frames, 2, 4096, 256
    eng = Engine(4, buffer_size=512)
    ctx = eng.ctx
    A = eng.add_sample_synth("f32", ch, 48000, n, 0x5B11CE, 0, 0.7)
    B = eng.add_sample_synth("f32", ch, 48000, n, 0x5B11CF, 1, 0.7)
    ctx.sync()
    dst = B + 1                                              # layer 1's results replace each other here
    fb = ch * 4                                              # bytes per frame
    sp = W.splice_part
    keep = W.edit_desc(0, n)
    one = [sp(A, 0, n)]
    join = [sp(A, 0, n, 0, fade_out=xf), sp(B, 0, n, n - xf, fade_in=xf)]
    slot = n // 64
    comp = [sp((A, B)[i % 2], i * slot, slot + (lap if i < 63 else 0), i * slot, fade_in=lap if i else 0, fade_out=lap if i < 63 else 0,
               fade_in_shape="smooth", fade_out_shape="smooth") for i in range(64)]
    comp_read = sum(p.n_frames for p in comp)

    def host_route():
        planes = {k: [ctx.clip_download(k, c, n, np.float32) for c in range(ch)] for k in (A, B)}
        out = S.splice(planes, ch, 2 * n - xf, [S.Part(A, 0, n, 0, fade_out=xf), S.Part(B, 0, n, n - xf, fade_in=xf)])
        ctx.clip_upload(dst, "f32", 48000, out)

    steps = {"a_derive_keep": (lambda: ctx.clip_derive(A, dst, keep), 2 * n * fb),
             "b_splice_one_part": (lambda: ctx.clip_splice(dst, ch, n, one), 2 * n * fb),
             "c_join_crossfade": (lambda: ctx.clip_splice(dst, ch, 2 * n - xf, join), (2 * n + 2 * n - xf) * fb),
             "d_comp_64_parts": (lambda: ctx.clip_splice(dst, ch, 64 * slot, comp), (comp_read + 64 * slot) * fb)}

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    for f, _ in steps.values():   # warm: stream, the descriptor buffers, the pool's extents for the results
        timed(f)
    t = {k: [] for k in list(steps) + ["e"]}
    for _ in range(a.repeats):
        for k in list(steps) + list(steps)[::-1]:
            t[k].append(timed(steps[k][0]))
        if not a.no_host_route:
            t["e"].append(timed(host_route))

    def fig(v, b):
        med = statistics.median(v)
        return {"median_ms": 1e3 * med, "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v), "bytes": b, "GBps": b / med / 1e9}

    res = {k: fig(t[k], steps[k][1]) for k in steps}
    if t["e"]:
        res["e_download_numpy_upload"] = fig(t["e"], steps["c_join_crossfade"][1])
        res["c_over_e_time"] = res["c_join_crossfade"]["median_ms"] / res["e_download_numpy_upload"]["median_ms"]
    for k in ("b_splice_one_part", "c_join_crossfade", "d_comp_64_parts"):
        res[k[0] + "_over_a_GBps"] = res[k]["GBps"] / res["a_derive_keep"]["GBps"]
    out = {"frames": n, "channels": ch, "source_bytes": n * fb, "crossfade_frames": xf, "device": ctx.device_info(), "results": res}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
