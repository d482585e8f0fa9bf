"""Host model of wbx_clip_denoise, wbx_clip_denoise_profile, wbx_denoise_tables / _threshold / _hops / _profile_hops /
_band_hops / _launches / _check (include/wbx.h "Reducing a clip's noise") in numpy, the header's formulas operation for
operation.  Every fp64 step is one IEEE operation: the chains run in ascending term order (one vector `re = re + d[j] *
AC[:, j]` per term, the hops and the bins side by side; no np.dot, whose order is not fixed), the products of fp32 values are
exact in fp64, the box is added cell by cell in the stated order with absent cells left out, and the four hops of an output
frame are added in hop order before the one rounding.  The tables are built from resample_model's sinpi, as the header
builds them from its own.  Every bit of the library's tables, thresholds, sums, statistics and samples must come out of this."""
import numpy as np

import resample_model as RS

F32, F64 = np.float32, np.float64
MIN_WINDOW, MAX_WINDOW = 64, 2048
MAX_S, MAX_F = 4, 8
MAX_FRAMES = (1 << 31) - 16
STAGE_WORDS = 1 << 22
LEAD = 3
BAND_SLACK = 2 * MAX_S + LEAD
INVALID, UNSUPPORTED = -4, -3


def window_ok(W):
    return MIN_WINDOW <= W <= MAX_WINDOW and W & (W - 1) == 0


def frames_ok(n):
    return 1 <= n < MAX_FRAMES


def hops(n, W):
    """wbx_denoise_hops: T = ceil(n / H) + 3; 0 where refused"""
    if not frames_ok(n) or not window_ok(W):
        return 0
    H = W // 4
    return -(-n // H) + LEAD


def profile_hops(n, W):
    """wbx_denoise_profile_hops: complete windows only; 0 where refused"""
    if not frames_ok(n) or not window_ok(W) or n < W:
        return 0
    return (n - W) // (W // 4) + 1


def band_hops(W, channels):
    if not window_ok(W) or channels not in (1, 2):
        return 0
    return STAGE_WORDS // (W * channels) - BAND_SLACK


def launches(n, W, channels):
    per = band_hops(W, channels)
    if not per or not frames_ok(n):
        return 0
    blocks = -(-n // (W // 4))
    return -(-blocks // per)


def check(n, W, S, F, thr, channels, floor):
    """wbx_denoise_check: the status of the sizes and parameters alone, in the header's order (0: none); thr None = NULL"""
    if n == 0 or n >= MAX_FRAMES:
        return INVALID
    if not window_ok(W):
        return INVALID
    if S > MAX_S or F > MAX_F:
        return INVALID
    if thr is None:
        return INVALID
    t = np.asarray(thr, dtype=F64).reshape(-1)[:(2 if channels == 2 else 1) * (W // 2 + 1)]
    if not np.all(np.isfinite(t) & (t >= 0.0)):
        return INVALID
    if not (0.0 <= floor <= 1.0):
        return INVALID
    return 0


def profile_check(n, W):
    if n == 0 or n >= MAX_FRAMES or not window_ok(W) or n < W:
        return INVALID
    return 0


# ---- the tables -----------------------------------------------------------------------------------------------------------------
_TABLES = {}


def tables(W):
    """wbx_denoise_tables: (AC, AS, YC, YS), float32 [B][W] each"""
    if W in _TABLES:
        return _TABLES[W]
    assert window_ok(W)
    B = W // 2 + 1
    Wd = F64(W)
    j = np.arange(W, dtype=np.int64)
    s = RS.sinpi((j.astype(F64) + F64(0.5)) / Wd)
    t = j.astype(F64) / Wd
    c_of = RS.sinpi(F64(2.0) * t + F64(0.5))
    z_of = RS.sinpi(F64(2.0) * t)
    m = (np.arange(B, dtype=np.int64)[:, None] * j[None, :]) % W
    c, z = c_of[m], z_of[m]
    e = np.ones((B, 1), dtype=F64)
    e[0, 0] = e[B - 1, 0] = 0.5
    sc, sz = s[None, :] * c, s[None, :] * z
    AC = (sc / Wd).astype(F32)
    AS = (F64(0.0) - (sz / Wd)).astype(F32)
    YC = (e * sc).astype(F32)
    YS = (F64(0.0) - (e * sz)).astype(F32)
    _TABLES[W] = (AC, AS, YC, YS)
    return _TABLES[W]


def threshold(sums, n_hops, strength):
    """wbx_denoise_threshold"""
    return F64(strength) * (np.asarray(sums, dtype=F64) / F64(n_hops))


# ---- the call -------------------------------------------------------------------------------------------------------------------
def inputs(x):
    """a channel's frames as fp64 values that are fp32 values, what is not finite as 0.0"""
    x = np.asarray(x, dtype=F32)
    return np.where(np.isfinite(x), x, F32(0.0)).astype(F64)


def cells(x, W, starts, chunk=2048):
    """(r, i) float32 [len(starts)][B]: the cells of the hops that start at range frames `starts` (any sign); x = inputs(...)"""
    AC, AS, _, _ = tables(W)
    AC, AS = np.ascontiguousarray(AC.astype(F64).T), np.ascontiguousarray(AS.astype(F64).T)   # [j][k]
    n, B = len(x), W // 2 + 1
    starts = np.asarray(starts, dtype=np.int64)
    r, i = np.zeros((len(starts), B), dtype=F32), np.zeros((len(starts), B), dtype=F32)
    for at in range(0, len(starts), chunk):
        st = starts[at:at + chunk]
        re = np.zeros((len(st), B), dtype=F64)
        im = np.zeros_like(re)
        for j in range(W):
            g = st + j
            ok = (g >= 0) & (g < n)
            d = np.where(ok, x[np.clip(g, 0, n - 1)], F64(0.0))[:, None]
            re = re + d * AC[j][None, :]
            im = im + d * AS[j][None, :]
        r[at:at + chunk], i[at:at + chunk] = re.astype(F32), im.astype(F32)
    return r, i


def power(r, i):
    r, i = r.astype(F64), i.astype(F64)
    return (r * r) + (i * i)


def gate(r, i, S, F, thr, floor):
    """the masked cells and the open flags of ALL hops of a channel: r, i [T][B], thr [B]"""
    T, B = r.shape
    p = power(r, i)
    q = np.zeros((T, B), dtype=F64)
    for dt in range(-S, S + 1):
        for dk in range(-F, F + 1):
            t0, t1 = max(0, -dt), min(T, T - dt)               # the cells (t, k) whose (t + dt, k + dk) is present
            k0, k1 = max(0, -dk), min(B, B - dk)
            if t0 < t1 and k0 < k1:
                q[t0:t1, k0:k1] = q[t0:t1, k0:k1] + p[t0 + dt:t1 + dt, k0 + dk:k1 + dk]
    t, k = np.arange(T)[:, None], np.arange(B)[None, :]
    count = (np.minimum(t + S, T - 1) - np.maximum(t - S, 0) + 1) * (np.minimum(k + F, B - 1) - np.maximum(k - F, 0) + 1)
    q = q / count.astype(F64)
    th = np.asarray(thr, dtype=F64)[None, :]
    is_open = q > th
    with np.errstate(divide="ignore", invalid="ignore"):
        v = F64(1.0) - (th / q)
    fl = F64(floor)
    g = np.where(is_open, np.where(v > fl, v, fl), fl)
    return (g * r.astype(F64)).astype(F32), (g * i.astype(F64)).astype(F32), is_open


def chains(mr, mi, W, chunk=2048):
    """a [hops][W] float64: the synthesis chains of masked cells [hops][B]"""
    _, _, YC, YS = tables(W)
    YC, YS = YC.astype(F64), YS.astype(F64)
    B = W // 2 + 1
    a = np.zeros((mr.shape[0], W), dtype=F64)
    for at in range(0, mr.shape[0], chunk):
        acc = np.zeros((min(chunk, mr.shape[0] - at), W), dtype=F64)
        cr, ci = mr[at:at + chunk].astype(F64), mi[at:at + chunk].astype(F64)
        for k in range(B):
            acc = acc + cr[:, k:k + 1] * YC[k][None, :]
            acc = acc + ci[:, k:k + 1] * YS[k][None, :]
        a[at:at + chunk] = acc
    return a


def overlap_add(a, n, W):
    """out float32 [n]: ((a_0 + a_1) + a_2) + a_3 over the four hops of a frame, rounded once"""
    H = W // 4
    f = np.arange(n, dtype=np.int64)
    t0, r = f // H, f % H
    acc = a[t0, r + 3 * H]
    for u in range(1, 4):
        acc = acc + a[t0 + u, r + (3 - u) * H]
    with np.errstate(over="ignore"):
        return acc.astype(F32)


def denoise_channel(x, W, S, F, thr, floor):
    """one channel's range (float32 [n]) through the call: (out float32 [n], open cells)"""
    x = inputs(x)
    n, H = len(x), W // 4
    T = hops(n, W)
    r, i = cells(x, W, (np.arange(T, dtype=np.int64) - LEAD) * H)
    mr, mi, is_open = gate(r, i, S, F, thr, floor)
    return overlap_add(chains(mr, mi, W), n, W), int(is_open.sum())


def denoise_clip(planes, first, n, W, S, F, thr, floor):
    """wbx_clip_denoise of frames [first, first + n) of a clip given as its channel planes: (planes of the result, stats
    without bands)"""
    C, B = len(planes), W // 2 + 1
    thr = np.asarray(thr, dtype=F64).reshape(C, B)
    outs, n_open = [], 0
    for c in range(C):
        o, k = denoise_channel(np.asarray(planes[c])[first:first + n], W, S, F, thr[c], floor)
        outs.append(o)
        n_open += k
    T = hops(n, W)
    return outs, {"hops": T, "cells": T * B * C, "open_cells": n_open}


def profile_clip(planes, first, n, W):
    """wbx_clip_denoise_profile: (sums float64 [channels * B], hops)"""
    Hn, B = profile_hops(n, W), W // 2 + 1
    sums = np.zeros((len(planes), B), dtype=F64)
    for c, pl in enumerate(planes):
        r, i = cells(inputs(np.asarray(pl)[first:first + n]), W, np.arange(Hn, dtype=np.int64) * (W // 4))
        p = power(r, i)
        acc = np.zeros(B, dtype=F64)
        for h in range(Hn):
            acc = acc + p[h]
        sums[c] = acc
    return sums.reshape(-1), Hn
