"""Host model of wbx_clip_stretch, wbx_stretch_steps / _anchor / _window (include/wbx.h "Stretching a clip") in numpy, the
header's formulas operation for operation.  Every fp64 step is one IEEE operation: the two chains of a candidate's score run
in ascending term order (one vector `s = s + t[i] * span[i : i + candidates]` per term, the candidates side by side; no
np.dot, whose order is not fixed), the products of fp32 values are exact in fp64, the arg-max takes the lowest of equal
candidates (np.argmax: the first).  Positions, window and every output sample of the library must reproduce every bit."""
import numpy as np

import resample_model as RS

F32, F64 = np.float32, np.float64
MIN_WINDOW, MAX_WINDOW, MAX_TOLERANCE = 32, 8192, 4096
MAX_FRAMES, MAX_RATIO = (1 << 31) - 16, 8
INVALID, UNSUPPORTED = -4, -3


class Refused(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(status)


def window_ok(N):
    return MIN_WINDOW <= N <= MAX_WINDOW and N % 8 == 0


def steps(m, N):
    """wbx_stretch_steps: K = ceil(m / Hs); 0 for a window the call refuses"""
    return -(-m // (N // 2)) if window_ok(N) else 0


def anchor(k, n, m, N):
    """wbx_stretch_anchor: a_k = floor(k Hs n / m) (Python integers: exact)"""
    return (k * (N // 2) * n) // m if window_ok(N) and m else 0


def window(N):
    """wbx_stretch_window: (w_up, w_dn), Hs doubles each"""
    if not window_ok(N):
        raise Refused(INVALID)
    t = RS.sinpi(np.arange(N // 2, dtype=F64) / F64(N))
    up = t * t
    return up, F64(1.0) - up


def check_args(n, m, N, D, positions_cap=None):
    """wbx_stretch.h's stretch_check_args: the status a call gets before its clip is looked at (0: none)"""
    if n == 0 or m == 0:
        return INVALID
    if n >= MAX_FRAMES or m >= MAX_FRAMES:
        return INVALID
    if not window_ok(N):
        return INVALID
    if not 0 <= D <= MAX_TOLERANCE:
        return INVALID
    if positions_cap is not None and positions_cap < steps(m, N):
        return INVALID
    if m > MAX_RATIO * n or n > MAX_RATIO * m:
        return UNSUPPORTED
    return 0


def inputs(planes):
    """x[c][i]: the (double) of the range's fp32 samples, what is not finite entering as 0.0"""
    out = []
    for p in planes:
        v = np.asarray(p, dtype=F32).astype(F64)
        out.append(np.where(np.isfinite(v), v, F64(0.0)))
    return out


def detector(x):
    """d as fp64 values that are fp32 values: mono x[0]; stereo (float)(0.5 * (x[0] + x[1])), one rounding"""
    if len(x) == 1:
        return x[0]
    return (F64(0.5) * (x[0] + x[1])).astype(F32).astype(F64)


def positions(d, m, N, D):
    """(p, info): the K positions as int32 and {"steps", "searched_steps", "candidates", "max_shift"}"""
    n, Hs = len(d), N // 2
    K = steps(m, N)
    dz = np.concatenate([d, np.zeros(Hs + 2 * MAX_TOLERANCE + 1, dtype=F64)])   # zero outside [0, n)
    p = np.zeros(K, dtype=np.int32)
    prev, searched, scored, max_shift = -Hs, 0, 0, 0
    for k in range(K):
        a = anchor(k, n, m, N)
        c = prev + Hs
        lo, hi = max(a - D, 0), min(a + D, n - 1)
        if lo <= c <= hi:
            prev = c
        else:
            cand = hi - lo + 1
            t = dz[c:c + Hs] if c < n else np.zeros(Hs, dtype=F64)
            s, E = np.zeros(cand, dtype=F64), np.zeros(cand, dtype=F64)
            for i in range(Hs):                                 # ascending terms, the candidates side by side
                w = dz[lo + i:lo + i + cand]
                s = s + t[i] * w
                E = E + w * w
            with np.errstate(divide="ignore", invalid="ignore"):
                score = np.where(E == 0.0, F64(0.0), (s * np.abs(s)) / np.where(E == 0.0, F64(1.0), E))
            prev = lo + int(np.argmax(score))                   # (numpy: the first of equal maxima)
            searched += 1
            scored += cand
        p[k] = prev
        max_shift = max(max_shift, abs(prev - a))
    return p, {"steps": K, "searched_steps": searched, "candidates": scored, "max_shift": max_shift}


def overlap_add(x, p, m, N):
    """the result's fp32 planes from the positions"""
    n, Hs = len(x[0]), N // 2
    up, dn = window(N)
    out = []
    for xc in x:
        xz = np.concatenate([xc, np.zeros(2 * Hs, dtype=F64)])
        y = np.zeros(len(p) * Hs, dtype=F32)
        prev = -Hs
        for k, pk in enumerate(p):
            pk, c = int(pk), prev + Hs
            a = xz[pk:pk + Hs]
            y[k * Hs:(k + 1) * Hs] = a.astype(F32) if pk == c else ((up * a) + (dn * xz[c:c + Hs])).astype(F32)
            prev = pk
        out.append(y[:m].copy())
    return out


def stretch_clip(src, first, n, m, N=2048, D=512):
    """src: a list of fp32 planes (1 or 2).  (the result's planes, the positions, the info without its launches)"""
    x = inputs([q[first:first + n] for q in src])
    p, info = positions(detector(x), m, N, D)
    return overlap_add(x, p, m, N), p, info
