"""Host model of wbx_clip_onsets, wbx_clip_tempo, wbx_onset_hops / _check / _pick (include/wbx.h "Finding a clip's onsets and
tempo") in numpy, the header's formulas operation for operation.  Every fp64 step is one IEEE operation: a run's two sums
take their frames in ascending order (one vector step per column, the runs and the hops side by side; no np.sum, whose order
is not fixed), the square of a detector value is exact in fp64 while the square of a difference is rounded before it is
added, the 64 run sums are added as a balanced tree of adjacent pairs, and the pick's local mean is an ascending sum.  Every
bit of the library's records must come out of this; the tempo records are f0_model.track's over the novelty."""
import numpy as np

import f0_model as F0
import stretch_model as ST

F32, F64 = np.float32, np.float64
MIN_HOP, MAX_HOP, MAX_HOPS, MAX_FRAMES = 64, 16384, 1 << 20, (1 << 31) - 16
MIN_FLOOR, MAX_FLOOR, MAX_W, MAX_A = 1e-30, 1.0, 64, 256
INVALID, UNSUPPORTED = -4, -3
DTYPE = np.dtype([("energy", "<f8"), ("edge_energy", "<f8"), ("novelty", "<f8"), ("onset", "<u4"), ("_pad", "<u4")])
DEFAULTS = dict(H=256, floor_power=1e-9, threshold=0.3, delta=0.1, w=3, a=8)


def hop_ok(H):
    return MIN_HOP <= H <= MAX_HOP and H % 64 == 0


def hops(n, H):
    """wbx_onset_hops: only complete hops count; 0 for a hop length the call refuses"""
    return n // H if hop_ok(H) else 0


def check_sizes(n, H, floor_power):
    if n == 0 or n >= MAX_FRAMES or not hop_ok(H):
        return INVALID
    if not (floor_power >= MIN_FLOOR and floor_power <= MAX_FLOOR):   # (a NaN fails both)
        return INVALID
    return 0


def check(n, H, floor_power, threshold, delta, w, a, has_out=True, cap=None):
    """wbx_onset_check: the status a call gets before its clip is looked at (0: none); cap None = as many as there are hops"""
    if check_sizes(n, H, floor_power):
        return INVALID
    if not (threshold > 0.0 and threshold <= 2.0) or not (delta >= 0.0 and delta <= 2.0):
        return INVALID
    if not 0 <= w <= MAX_W or not 0 <= a <= MAX_A:
        return INVALID
    h = hops(n, H)
    if h > 0 and not has_out:
        return INVALID
    if cap is not None and cap < h:
        return INVALID
    if h > MAX_HOPS:
        return UNSUPPORTED
    return 0


def tempo_check(n, H, floor_power, W, step, lag_min, lag_max, threshold, has_out=True, cap=None):
    """wbx_clip_tempo's argument check: the sizes, the number of hops, then wbx_f0_check's rules with n = hops (no hops: the
    shape alone)"""
    if check_sizes(n, H, floor_power):
        return INVALID
    h = hops(n, H)
    if h > MAX_HOPS:
        return UNSUPPORTED
    return F0.check(max(h, 1), W, step, lag_min, lag_max, threshold, has_out, cap)


def energies(d, H):
    """(A, B) of the complete hops of detector values `d` (fp64 values that are fp32 values)"""
    d = np.asarray(d, dtype=F64)
    nh, q = hops(len(d), H), H // 64
    if nh == 0:
        return np.zeros(0, dtype=F64), np.zeros(0, dtype=F64)
    cur = d[:nh * H].reshape(nh, 64, q)
    before = np.concatenate([[F64(0.0)], d[:nh * H - 1]]).reshape(nh, 64, q)      # d[t-1], d[-1] = 0.0
    a = np.zeros((nh, 64), dtype=F64)
    b = np.zeros((nh, 64), dtype=F64)
    for j in range(q):
        a = a + cur[:, :, j] * cur[:, :, j]
        e = cur[:, :, j] - before[:, :, j]
        b = b + (e * e)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
        b = b[:, 0::2] + b[:, 1::2]
    return a[:, 0].copy(), b[:, 0].copy()


def rise(X, floor):
    z = np.concatenate([np.zeros(3, dtype=F64), X])
    ref = np.maximum(np.maximum(z[2:-1], z[1:-2]), z[0:-3])      # X(h-1), X(h-2), X(h-3)
    up = X - ref
    up = np.where(up > 0.0, up, F64(0.0))
    return up / ((X + ref) + floor)


def novelty(A, B, H, floor_power):
    """o(h) as float32"""
    floor = F64(H) * F64(floor_power)
    return (rise(A, floor) + rise(B, floor)).astype(F32)


def pick(o, threshold, delta, w, a):
    """onset(h) as uint32 from the novelty (float32 values)"""
    o = np.asarray(o, dtype=F32).astype(F64)
    n = len(o)
    on = o >= F64(threshold)
    for k in range(1, w + 1):
        earlier = np.concatenate([np.full(k, -1.0), o[:n - k]]) if k < n else np.full(n, -1.0)
        later = np.concatenate([o[k:], np.full(k, -1.0)]) if k < n else np.full(n, -1.0)
        on &= ~(earlier >= o) & ~(later > o)
    m = np.zeros(n, dtype=F64)
    cnt = np.zeros(n, dtype=np.int64)
    idx = np.arange(n)
    for k in range(-a, a + 1):                                   # ascending g = h + k
        ok = (idx + k >= 0) & (idx + k < n)
        m = np.where(ok, m + o[np.clip(idx + k, 0, max(n - 1, 0))], m) if n else m
        cnt += ok
    if n:
        on &= o >= m / cnt.astype(F64) + F64(delta)
    return on.astype(np.uint32)


def records(d, H, floor_power, threshold, delta, w, a):
    A, B = energies(d, H)
    o = novelty(A, B, H, floor_power)
    rec = np.zeros(len(A), dtype=DTYPE)
    rec["energy"], rec["edge_energy"], rec["novelty"] = A, B, o.astype(F64)
    rec["onset"] = pick(o, threshold, delta, w, a)
    return rec


def detector_of(planes, first, n):
    return ST.detector(ST.inputs([np.asarray(p)[first:first + n] for p in planes]))


def onsets_clip(planes, first, n, H=256, floor_power=1e-9, threshold=0.3, delta=0.1, w=3, a=8):
    """wbx_clip_onsets of frames [first, first + n) of a clip given as its channel planes: (records, info)"""
    rec = records(detector_of(planes, first, n), H, floor_power, threshold, delta, w, a)
    return rec, {"hops": len(rec), "onsets": int(rec["onset"].sum()), "launches": 2 if len(rec) else 0}


def tempo_clip(planes, first, n, H, floor_power, W, step, lag_min, lag_max, threshold, only=None):
    """wbx_clip_tempo: f0_model.track over the novelty as a signal whose frames are hops: (records, info)"""
    A, B = energies(detector_of(planes, first, n), H)
    o = novelty(A, B, H, floor_power).astype(F64)
    rec = F0.track(o, W, step, lag_min, lag_max, threshold, only)
    total = F0.hops(len(o), W, step, lag_max)
    info = {"hops": total, "terms": total * W * (lag_max + 1)}
    if only is None:
        info["voiced_hops"] = int(rec["voiced"].sum())
    return rec, info


# ---- the material the tests share ---------------------------------------------------------------------------------------------
def drum_loop(bpm, rate=48000, seconds=14.0, seed=1):
    """(x as float32, the true onset frames): kick and snare on the beats, noise-burst hats on the eighths, two steady sines
    underneath, noise at 1e-3"""
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    i = np.arange(n, dtype=F64)
    x = 0.05 * np.sin(2 * np.pi * 110.0 * i / rate) + 0.04 * np.sin(2 * np.pi * 329.63 * i / rate) + 1e-3 * rng.standard_normal(n)
    beat = 60.0 * rate / bpm
    at, k = [], 0
    while True:
        t = int(round(k * beat / 2.0))
        if t + rate // 5 >= n:
            break
        m = rate // 5
        j = np.arange(m, dtype=F64)
        if k % 2 == 0 and (k // 2) % 2 == 0:                     # kick: a falling sine
            hit = 0.8 * np.sin(2 * np.pi * (50.0 * j / rate + 60.0 * (1.0 - np.exp(-j / (0.02 * rate))) * 0.02)) * np.exp(-j / (0.06 * rate))
        elif k % 2 == 0:                                         # snare: a tone and noise
            hit = (0.3 * np.sin(2 * np.pi * 190.0 * j / rate) + 0.5 * rng.standard_normal(m)) * np.exp(-j / (0.04 * rate))
        else:                                                    # hat: a short noise burst
            hit = 0.25 * rng.standard_normal(m) * np.exp(-j / (0.012 * rate))
        x[t:t + m] += hit
        at.append(t)
        k += 1
    return x.astype(F32), np.asarray(at, dtype=np.int64)
