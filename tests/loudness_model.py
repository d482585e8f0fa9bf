"""Host model of wbx_clip_loudness (include/wbx.h "Measuring a clip's loudness"): hop arithmetic, the K-weighting
coefficients, the segmented filter, the gate and the true peak in numpy, the header's formulas operation for operation —
what tests/resample_model.py is for the rate conversion.  Every fp64 step is one IEEE operation (no libm but the final
log10s, no pairwise summation), so the library's coefficients, the device's hop energies and every power and count of the
gate must reproduce every bit."""
import math

import numpy as np

import resample_model as R

F32, F64 = np.float32, np.float64
MIN_RATE, MAX_RATE = 8000, 384000
TRIG_TERMS = 13
PI = F64(3.141592653589793)
ABS_GATE = F64(1.1724653045822981e-07)
SHORT_HOPS, RANGE_STEP = 30, 10
TRUE_PEAK = 1
FIELDS_EXACT = ("gated_power", "hops", "blocks", "blocks_gated", "hop_frames")
FIELDS_LUFS = ("integrated", "momentary_max", "short_term_max", "range_lu")


def hop_frames(rate):
    return (rate + 5) // 10


def hops(rate, n):
    return n // hop_frames(rate)


def oversampling(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def tan_pi(f0, rate):
    y = (PI * F64(f0)) / F64(rate)
    y2 = y * y
    s = c = F64(1.0)
    for n in range(TRIG_TERMS, 0, -1):
        s = F64(1.0) - (s * y2) / F64((2 * n) * (2 * n + 1))
        c = F64(1.0) - (c * y2) / F64((2 * n - 1) * (2 * n))
    return (y * s) / c


def _stages(rate, tan):
    Q, Vh, Vb = F64(0.7071752369554196), F64(1.5848647011308556), F64(1.2587209302325617)
    K = F64(tan(1681.974450955533, rate))
    KQ, KK = K / Q, K * K
    a0 = (F64(1.0) + KQ) + KK
    out = [((Vh + Vb * KQ) + KK) / a0, (F64(2.0) * (KK - Vh)) / a0, ((Vh - Vb * KQ) + KK) / a0,
           (F64(2.0) * (KK - F64(1.0))) / a0, ((F64(1.0) - KQ) + KK) / a0]
    Q = F64(0.5003270373238773)
    K = F64(tan(38.13547087602444, rate))
    KQ, KK = K / Q, K * K
    a0 = (F64(1.0) + KQ) + KK
    out += [F64(1.0), F64(-2.0), F64(1.0), (F64(2.0) * (KK - F64(1.0))) / a0, ((F64(1.0) - KQ) + KK) / a0]
    return np.array(out, dtype=F64)


def coefficients(rate):
    """[10] float64: stage 1's b0 b1 b2 a1 a2, stage 2's"""
    return _stages(rate, tan_pi)


def coefficients_libm(rate):
    """the same formulas over math.tan: the independent yardstick of the series"""
    return _stages(rate, lambda f0, r: math.tan(math.pi * f0 / r))


def _clean(plane, first, n):
    x = np.asarray(plane[first:first + n], dtype=F32).astype(F64)
    x[np.isnan(x)] = 0.0
    return x


def _biquad(c, x, st):
    """one direct-form-I step of every lane: st = [x1, x2, y1, y2]"""
    y = ((((c[0] * x + c[1] * st[0]) + c[2] * st[1]) - c[3] * st[2]) - c[4] * st[3])
    st[1], st[0], st[3], st[2] = st[0], x, st[2], y
    return y


def hop_energies(planes, first, n, rate):
    """[C][hops] float64: every hop's filter run from rest two hops earlier (the specification, not an approximation)"""
    hop, H = hop_frames(rate), hops(rate, n)
    C = len(planes)
    E = np.zeros((C, H), dtype=F64)
    if H == 0:
        return E
    co = coefficients(rate)
    xp = np.zeros((C, (H + 2) * hop), dtype=F64)                  # two hops of zeros in front: frames below 0
    for ch in range(C):
        xp[ch, 2 * hop:] = _clean(planes[ch], first, H * hop)
    base = np.arange(H, dtype=np.int64) * hop
    s1 = [np.zeros((C, H), dtype=F64) for _ in range(4)]
    s2 = [np.zeros((C, H), dtype=F64) for _ in range(4)]
    with np.errstate(all="ignore"):
        for t in range(3 * hop):
            v = _biquad(co[5:], _biquad(co[:5], xp[:, base + t], s1), s2)
            if t >= 2 * hop:
                E = E + v * v
    return E


def sequential_energies(plane, first, n, rate):
    """[hops] float64 of ONE channel by one sequential pass of the same two stages (python floats are IEEE doubles)"""
    hop, H = hop_frames(rate), hops(rate, n)
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (float(v) for v in coefficients(rate))
    x = _clean(plane, first, H * hop).tolist()
    E = [0.0] * H
    x1 = x2 = y1 = y2 = u1 = u2 = v1 = v2 = 0.0
    for i, xv in enumerate(x):
        y = ((((b0 * xv + b1 * x1) + b2 * x2) - a1 * y1) - a2 * y2)
        x2, x1, y2, y1 = x1, xv, y1, y
        v = ((((c0 * y + c1 * u1) + c2 * u2) - d1 * v1) - d2 * v2)
        u2, u1, v2, v1 = u1, y, v1, v
        E[i // hop] = E[i // hop] + v * v
    return np.array(E, dtype=F64)


def lufs(power):
    return -0.691 + 10.0 * math.log10(power) if power > 0.0 else -math.inf


def gate(E, hop):
    """E: [C][hops] float64 -> every field of wbx_loudness but true_peak and oversampling"""
    E = np.asarray(E, dtype=F64)
    C, H = E.shape
    blocks = H - 3 if H >= 4 else 0
    out = dict(hops=H, hop_frames=hop, blocks=blocks)
    z = np.zeros(blocks, dtype=F64)
    if blocks:
        s = [((E[c, 0:blocks] + E[c, 1:blocks + 1]) + E[c, 2:blocks + 2]) + E[c, 3:blocks + 3] for c in range(C)]
        z = (s[0] + s[1] if C > 1 else s[0]) / F64(4 * hop)
    zmax = F64(0.0)
    for v in z:
        if v > zmax:
            zmax = v
    total, count = F64(0.0), 0
    for v in z:
        if v > ABS_GATE:
            total, count = total + v, count + 1
    gated, passed = F64(0.0), 0
    if count:
        rel = (total / F64(count)) * F64(0.1)
        total = F64(0.0)
        for v in z:
            if v > ABS_GATE and v > rel:
                total, passed = total + v, passed + 1
        if passed:
            gated = total / F64(passed)
    out.update(gated_power=float(gated), blocks_gated=passed, integrated=lufs(float(gated)), momentary_max=lufs(float(zmax)))

    windows = H - SHORT_HOPS + 1 if H >= SHORT_HOPS else 0
    w = np.zeros(windows, dtype=F64)
    if windows:
        for c in range(C):
            s = np.zeros(windows, dtype=F64)
            for k in range(SHORT_HOPS):                           # ascending k, never numpy's pairwise sum
                s = s + E[c, k:k + windows]
            w = s / F64(SHORT_HOPS * hop) if c == 0 else w + s / F64(SHORT_HOPS * hop)
    wmax = F64(0.0)
    for v in w:
        if v > wmax:
            wmax = v
    out["short_term_max"] = lufs(float(wmax))
    kept = [v for v in w[::RANGE_STEP] if v > ABS_GATE]
    rng = 0.0
    if kept:
        total = F64(0.0)
        for v in kept:
            total = total + v
        rel = (total / F64(len(kept))) * F64(0.01)
        s = sorted(v for v in kept if v > rel)
        if len(s) >= 2:
            top = float(len(s) - 1)
            rng = 10.0 * math.log10(float(s[int(top * 0.95 + 0.5)] / s[int(top * 0.10 + 0.5)]))
    out["range_lu"] = rng
    return out


def true_peak(planes, first, n, rate):
    """[C] float32: the largest |value| among the range's own samples and its oversampled rendering (NaNs never raise it)"""
    factor = oversampling(rate)
    peaks = []
    up = R.resample(planes, first, n, rate, factor * rate, R.GOOD) if factor > 1 else [np.zeros(0, dtype=F32)] * len(planes)
    for plane, y in zip(planes, up):
        both = np.concatenate([np.abs(np.asarray(plane[first:first + n], dtype=F32)), np.abs(y), np.zeros(1, dtype=F32)])
        peaks.append(F32(np.nanmax(both)))
    return peaks


def measure(planes, first, n, rate, flags=0):
    out = gate(hop_energies(planes, first, n, rate), hop_frames(rate))
    tp = true_peak(planes, first, n, rate) if flags & TRUE_PEAK else []
    out["true_peak"] = [float(v) for v in tp] + [0.0] * (2 - len(tp))
    out["oversampling"] = oversampling(rate) if flags & TRUE_PEAK else 0
    return out


def normalize_gain(integrated, target_lufs, ceiling=0.0, peaks=()):
    g = F32(math.pow(10.0, (target_lufs - integrated) / 20.0))
    if ceiling:
        g = min(g, F32(ceiling) / F32(max(peaks)))
    return F32(g)
