"""Per-block cost of recording on the audio thread: wall time of wbx_engine_process(_in) at 4096 tracks (512-frame stereo
blocks, the one-launch callback) without a take, then with 16 armed tracks recording 8 stereo inputs (two tracks per input),
blocks interleaved A/B so that drift hits both sides alike.  Prints one JSON summary line (and writes it to --out).

    python tools/record_latency.py [--tracks 4096] [--armed 16] [--blocks 300] [--rounds 6] [--out FILE]
    python tools/record_latency.py --trace KERNEL_TRACE.csv     # no GPU: summarise a rocprofv3 --kernel-trace of a run

The trace summary says how many capture kernels (record_capture_kernel) started while a callback kernel was running (they
overlap it) and how many queued behind one."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import whitebox_amd as W  # noqa: E402
from whitebox_amd import synth  # noqa: E402
from whitebox_amd.engine import build_engine  # noqa: E402


def timed_blocks(eng, inb, out, n):
    ts = np.empty(n)
    for i in range(n):
        t0 = time.perf_counter()
        eng.process(inb, out, 48000.0)
        ts[i] = time.perf_counter() - t0
    return ts * 1e6


def trace_summary(path):
    import bisect
    import csv
    rows = list(csv.DictReader(open(path)))
    cap = [r for r in rows if "record_capture_kernel" in r["Kernel_Name"]]
    cb = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "callback_kernel" in r["Kernel_Name"])
    starts = [c[0] for c in cb]
    inside = after = 0
    for r in cap:
        s = int(r["Start_Timestamp"])
        i = bisect.bisect_right(starts, s) - 1
        if i >= 0 and cb[i][1] > s:
            inside += 1
        else:
            after += 1
    dur = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in cap)
    return {"captures": len(cap), "callbacks": len(cb), "captures_starting_inside_a_callback": inside,
            "captures_starting_outside": after, "capture_queues": sorted({r["Queue_Id"] for r in cap}),
            "callback_queues": sorted({r["Queue_Id"] for r in rows if "callback_kernel" in r["Kernel_Name"]}),
            "capture_ns_median": dur[len(dur) // 2] if dur else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="")
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--armed", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(trace_summary(a.trace)))
        return
    spec = synth.make_session("reclat", a.tracks, n_blocks=a.blocks + 80, seed=0xEC1A)   # clips play through every timed block
    n_in = a.armed                                    # stereo inputs 0 .. armed/2 - 1, two tracks on each
    plain, rec = [], []
    for mode in ("plain", "rec") * a.rounds:
        eng = build_engine(spec, max_blocks=1, device_synth=True)
        eng.set_audio_channel_config(n_in, 2, 512, 48000)
        for k in range(a.armed):
            eng.set_track_input(k * (a.tracks // a.armed), "external_stereo", k // 2, True)
        out = W.AudioBuffer(512, 2)
        inb = W.AudioBuffer(512, n_in)
        for ch in range(n_in):
            inb.channel_buffers[ch][:] = np.random.default_rng(ch).standard_normal(512).astype(np.float32) * 0.1
        if mode == "rec":
            eng.record()
        else:
            eng.play()
        timed_blocks(eng, inb, out, 64)              # warm-up
        (rec if mode == "rec" else plain).append(timed_blocks(eng, inb, out, a.blocks))
        if mode == "rec":
            info = eng.record_info(0)
            assert info["status"] == 0, info
            eng.stop_record()
        eng.close()
    p, r = np.concatenate(plain), np.concatenate(rec)
    res = {"tracks": a.tracks, "armed": a.armed, "block_frames": 512, "blocks_per_side": int(p.size),
           "plain_us_median": round(float(np.median(p)), 2), "rec_us_median": round(float(np.median(r)), 2),
           "plain_us_p99": round(float(np.percentile(p, 99)), 2), "rec_us_p99": round(float(np.percentile(r, 99)), 2),
           "added_us_median": round(float(np.median(r) - np.median(p)), 2),
           "added_us_mean": round(float(r.mean() - p.mean()), 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
