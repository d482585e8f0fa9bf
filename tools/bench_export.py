#!/usr/bin/env python3
"""Exporting in numbers (MEASUREMENTS.md "Exporting", profiles/export_2p24.json): a stereo F32 clip of 2^24 frames (128 MiB,
5.8 minutes at 48 kHz) resident in HBM, brought to the host as interleaved device-format samples —

  A  download+host   the only route before wbx_clip_export: wbx_clip_download per channel (a synchronous copy into pageable
                     memory), then the oracle's converter (oracle/wb_oracle.c wbo_f32_to_interleaved_*, the reference's loop)
                     on one host thread; packed 24-bit additionally strips the fourth byte of the i24_x8 words with numpy,
                     since the reference's own packed writer drops a channel
  B  export          wbx_clip_export with the clamp, into pageable memory and into wbx_host_alloc memory
  Y  yardstick       a plain device -> pinned-host copy of the same number of bytes (torch, the copy engine)

for I16, packed I24 and F32.  One process; per format, after a warm-up, `--repeats` rounds in the order A B B A (B: pageable
then pinned inside each B), the yardstick behind each round; median and spread (min .. max) per figure, and the ratios B / A
and B / Y of the medians.  The export's kernel time comes from a run of its own under
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_export.py --repeats 1 --no-host-route
--chunk (frames per staging chunk) is the A/B aid of EXPERIMENTS.md."""
import argparse
import ctypes as C
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
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--no-host-route", action="store_true", help="leave route A out (profiling runs)")
    a = ap.parse_args()
    import torch   # first: it ships its own HIP runtime, which libwbx.so must bind to as well
    import numpy as np
    import whitebox_amd as W
    from whitebox_amd import _ffi
    import oracle_ffi as O

    n, ch = a.frames, 2
    L = W.lib()
    ctx = W.MixContext(4, block=512)
    ctx.clip_synth(0, "f32", ch, 48000, n, 0xE4907, 0, 1.05)
    if a.chunk:
        ctx.set_export_chunk(a.chunk)
    ctx.sync()

    def route_a(fmt):
        t0 = time.perf_counter()
        planes = [ctx.clip_download(0, c, n, np.float32) for c in range(ch)]
        t1 = time.perf_counter()
        name = "i24_x8" if fmt == "i24" else fmt
        out = np.empty(n * ch, dtype=_ffi.OUT_DTYPE[name])
        getattr(O.lib(), "wbo_f32_to_interleaved_" + name)(out.ctypes.data, O.planar_ptrs(planes), 0, n, ch)
        if fmt == "i24":
            out = np.ascontiguousarray(out.view(np.uint8).reshape(-1, 4)[:, :3])
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0

    def route_b(fmt, buf):
        t0 = time.perf_counter()
        _, st = ctx.clip_export(0, fmt, ch, 0, n, clamp=True, out=buf)
        return time.perf_counter() - t0, st

    def fig(v):
        return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}

    res = {}
    for fmt in ("i16", "i24", "f32"):
        nbytes = L.wbx_export_bytes(_ffi.OUT_FMT[fmt], ch, n)
        page = np.zeros(nbytes, dtype=np.uint8)
        p = C.c_void_p()
        assert L.wbx_host_alloc(nbytes, C.byref(p)) == 0
        pinned = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))
        dev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()

        def yard():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.copy_(dev, non_blocking=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        route_b(fmt, page)
        _, st = route_b(fmt, pinned)
        assert np.array_equal(page, pinned)
        yard()
        t = {"A": [], "A_download": [], "B_pageable": [], "B_pinned": [], "Y": []}
        for _ in range(a.repeats):
            order = "BB" if a.no_host_route else "ABBA"
            for step in order:
                if step == "A":
                    d, dl = route_a(fmt)
                    t["A"].append(d)
                    t["A_download"].append(dl)
                else:
                    t["B_pageable"].append(route_b(fmt, page)[0])
                    t["B_pinned"].append(route_b(fmt, pinned)[0])
            t["Y"].append(yard())
        r = {k: fig(v) for k, v in t.items() if v}
        r["bytes"] = nbytes
        med = lambda k: statistics.median(t[k])
        if t["A"]:
            r["B_pageable_over_A"] = med("B_pageable") / med("A")
            r["B_pinned_over_A"] = med("B_pinned") / med("A")
        r["B_pageable_over_Y"] = med("B_pageable") / med("Y")
        r["B_pinned_over_Y"] = med("B_pinned") / med("Y")
        r["B_pinned_GBps"] = nbytes / med("B_pinned") / 1e9
        r["Y_GBps"] = nbytes / med("Y") / 1e9
        r["stats"] = st
        res[fmt] = r
        del pinned
        assert L.wbx_host_free(p) == 0
    out = {"frames": n, "channels": ch, "source_bytes": n * ch * 4, "chunk_frames": a.chunk or (1 << 20),
           "device": ctx.device_info(), "formats": res}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
