"""Host model of wbx_clip_f0, wbx_f0_hops / _check / _launch_hops (include/wbx.h "Tracking a clip's pitch") in numpy, the
header's formulas operation for operation.  Every fp64 step is one IEEE operation: the two chains of a lag run in ascending
term order (one vector `r = r + d[t+j] * d[t+j : t+j+tau_max+1]` per term, the lags and the hops side by side; no np.dot,
whose order is not fixed), the products of fp32 values are exact in fp64, the cumulative mean is summed in runs of 8 lags and
then across the runs — the two-level order the header defines — and both minima of the pick take the lowest of equal lags.
Every bit of the library's records must come out of this."""
import numpy as np

import stretch_model as ST

F32, F64 = np.float32, np.float64
MIN_WINDOW, MAX_WINDOW = 64, 8192
MIN_TAU_MAX, MAX_TAU_MAX = 8, 4095
MAX_HOP, MAX_HOPS, MAX_FRAMES = 1 << 20, 1 << 20, (1 << 31) - 16
INVALID, UNSUPPORTED = -4, -3
DTYPE = np.dtype([("period", "<f8"), ("dip", "<f8"), ("energy", "<f8"), ("lag", "<u4"), ("voiced", "<u4")])


def shape_ok(W, H, tau_min, tau_max):
    return (MIN_WINDOW <= W <= MAX_WINDOW and W % 8 == 0 and MIN_TAU_MAX <= tau_max <= MAX_TAU_MAX and 2 <= tau_min < tau_max
            and 1 <= H <= MAX_HOP)


def hops(n, W, H, tau_max):
    """wbx_f0_hops: only complete frames count; 0 for a shape the call refuses"""
    if not shape_ok(W, H, 2, tau_max):
        return 0
    return (n - W - tau_max) // H + 1 if n >= W + tau_max else 0


def check(n, W, H, tau_min, tau_max, threshold, has_out=True, cap=None):
    """wbx_f0_check: the status a call gets before its clip is looked at (0: none); cap None = as many as there are hops"""
    if n == 0 or n >= MAX_FRAMES:
        return INVALID
    if not (MIN_WINDOW <= W <= MAX_WINDOW and W % 8 == 0):
        return INVALID
    if not MIN_TAU_MAX <= tau_max <= MAX_TAU_MAX:
        return INVALID
    if not 2 <= tau_min < tau_max:
        return INVALID
    if not 1 <= H <= MAX_HOP:
        return INVALID
    if not (threshold > 0.0 and threshold <= 1.0):              # (a NaN fails both)
        return INVALID
    h = hops(n, W, H, tau_max)
    if h > 0 and not has_out:
        return INVALID
    if cap is not None and cap < h:
        return INVALID
    if h > MAX_HOPS:
        return UNSUPPORTED
    return 0


def launch_hops(W, tau_max, launch_terms):
    """wbx_f0_launch_hops: max(1, launch_terms // (W * (tau_max + 1))), whole eights where there are 8 or more"""
    if not shape_ok(W, 1, 2, tau_max):
        return 0
    h = launch_terms // (W * (tau_max + 1))
    return max(1, h) if h < 8 else min(MAX_HOPS, h & ~7)


def launches(n_hops, W, tau_max, launch_terms):
    per = launch_hops(W, tau_max, launch_terms)
    return -(-n_hops // per) if per else 0


def difference(d, ts, W, tau_max):
    """(dd, E0) of the hops that start at frames `ts`: dd [len(ts)][tau_max + 1]"""
    ts = np.asarray(ts, dtype=np.int64)
    lag = np.arange(tau_max + 1, dtype=np.int64)
    r = np.zeros((len(ts), tau_max + 1), dtype=F64)
    E = np.zeros_like(r)
    for j in range(W):
        w = d[(ts + j)[:, None] + lag[None, :]]
        r = r + d[ts + j][:, None] * w
        E = E + w * w
    E0 = E[:, 0].copy()
    dd = (E0[:, None] + E) - (F64(2.0) * r)
    dd = np.where(dd < 0.0, F64(0.0), dd)
    dd[:, 0] = 0.0
    return dd, E0


def run_sums(dd):
    """S(tau) of one hop in the header's two-level order; dd [tau_max + 1]"""
    runs = -(-len(dd) // 8)
    v = np.zeros(8 * runs, dtype=F64)                           # lags above tau_max count 0.0
    v[:len(dd)] = dd
    v = v.reshape(runs, 8)
    P = np.zeros_like(v)
    P[:, 0] = v[:, 0]
    for i in range(1, 8):
        P[:, i] = P[:, i - 1] + v[:, i]
    B = np.zeros(runs, dtype=F64)
    for g in range(1, runs):
        B[g] = B[g - 1] + P[g - 1, 7]
    return (B[:, None] + P).reshape(-1)[:len(dd)]


def mean_normalized(dd):
    """c(tau) of one hop"""
    S = run_sums(dd)
    tau = np.arange(len(dd), dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(S == 0.0, F64(1.0), (dd * tau) / S)
    c[0] = 1.0
    return c


def pick(c, tau_min, tau_max, threshold):
    """(lag, voiced)"""
    lo = c[tau_min:tau_max]                                     # tau in [tau_min, tau_max - 1]
    dip = np.flatnonzero((lo < threshold) & (c[tau_min + 1:tau_max + 1] >= lo))
    if dip.size:
        return tau_min + int(dip[0]), 1
    return tau_min + int(np.argmin(lo)), 0                      # (np.argmin: the first of equals)


def refine(c, lag):
    a, b, g = c[lag - 1], c[lag], c[lag + 1]
    den = (a + g) - (F64(2.0) * b)
    off = (F64(0.5) * (a - g)) / den if (den > 0.0 and a >= b and g >= b) else F64(0.0)
    return F64(lag) + off, b


def track(d, W, H, tau_min, tau_max, threshold, only=None, chunk=64):
    """The records of detector values `d` (fp64 values that are fp32 values, what is not finite already 0.0): a DTYPE array
    of all hops — or, with `only` (hop indices), of those hops in that order: hops are independent"""
    n = len(d)
    total = hops(n, W, H, tau_max)
    which = list(range(total)) if only is None else [int(h) for h in only]
    assert all(0 <= h < total for h in which)
    out = np.zeros(len(which), dtype=DTYPE)
    d = np.asarray(d, dtype=F64)
    for at in range(0, len(which), chunk):
        part = which[at:at + chunk]
        dd, E0 = difference(d, [h * H for h in part], W, tau_max)
        for i in range(len(part)):
            c = mean_normalized(dd[i])
            lag, voiced = pick(c, tau_min, tau_max, F64(threshold))
            period, dip = refine(c, lag)
            out[at + i] = (period, dip, E0[i], lag, voiced)
    return out


def f0_clip(planes, first, n, W, H, tau_min, tau_max, threshold, only=None):
    """wbx_clip_f0 of frames [first, first + n) of a clip given as its channel planes: (records, info)"""
    x = ST.inputs([np.asarray(p)[first:first + n] for p in planes])
    rec = track(ST.detector(x), W, H, tau_min, tau_max, threshold, only)
    total = hops(n, W, H, tau_max)
    info = {"hops": total, "terms": total * W * (tau_max + 1)}
    if only is None:
        info["voiced_hops"] = int(rec["voiced"].sum())
    return rec, info
