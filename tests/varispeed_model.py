"""Host model of wbx_clip_varispeed (include/wbx.h "Reading a clip along a position curve"): the plan, the two tables, the
positions, the tiles, the ordered check and the call in numpy, the header's formulas operation for operation — what
tests/resample_model.py is for the conversion, whose row formula this shares.  Every fp64 step is one IEEE operation, so
the library's tables and the device's output must reproduce every bit.  Positions are Python integers (no overflow to
think about); they equal the library's 64-bit arithmetic inside the call's bounds."""
import math

import numpy as np

import resample_model as RM

F32, F64 = np.float32, np.float64
FAST, GOOD, BEST = range(3)
PHASES = {FAST: 256, GOOD: 512, BEST: 2048}
MAX_KNOTS, MAX_FRAMES, MARGIN = 1 << 22, (1 << 31) - 16, 1 << 16
TILE_MAX, SPAN_MAX = 1024, 4096
INVALID, UNSUPPORTED, OK = -4, -3, 0
Refused = RM.Refused


def plan(quality, guard_num=1, guard_den=1):
    """{H, T, P, s, cutoff, beta}; Refused(status) as wbx_varispeed_plan refuses"""
    if quality not in RM.QUALITY or guard_num == 0 or guard_den == 0 or guard_num < guard_den:
        raise Refused(INVALID)
    Z, beta, frac = RM.QUALITY[quality]
    g = math.gcd(guard_num, guard_den)
    M, L = guard_num // g, guard_den // g
    H = (Z * M + L - 1) // L if L < M else Z
    if 2 * H > RM.MAX_TAPS:
        raise Refused(UNSUPPORTED)
    rho = F64(L) / F64(M) if L < M else F64(1.0)
    P = PHASES[quality]
    return dict(H=H, T=2 * H, P=P, s=32 - (P.bit_length() - 1), cutoff=F64(frac) * rho, beta=F64(beta))


def tables(quality, guard_num=1, guard_den=1):
    """(h float32[P + 1][T], D float32[P][T])"""
    p = plan(quality, guard_num, guard_den)
    k = np.arange(p["T"], dtype=np.int64)[None, :] - (p["H"] - 1)
    frac = np.arange(p["P"] + 1, dtype=F64)[:, None] / F64(p["P"])          # row P: exactly 1.0
    d = k.astype(F64) - frac
    u = d / F64(p["H"])
    w = F64(1.0) - u * u
    w = np.where(w < 0.0, F64(0.0), w)
    v = ((p["cutoff"] * RM.sinc(p["cutoff"] * d)) * RM.i0(p["beta"] * np.sqrt(w))) / RM.i0(p["beta"])
    total = np.zeros(p["P"] + 1, dtype=F64)
    for kk in range(p["T"]):                                      # ascending k, never numpy's pairwise sum
        total = total + v[:, kk]
    h = (v / total[:, None]).astype(F32)
    D = (h[1:].astype(F64) - h[:-1].astype(F64)).astype(F32)
    return h, D


def n_knots(out_frames, g):
    return (out_frames + (1 << g) - 1 >> g) + 1


def position(knots, g, j):
    """Python integers; >> floors, as the library's arithmetic shift does"""
    i, r = j >> g, j & ((1 << g) - 1)
    k0 = int(knots[i])
    return k0 if r == 0 else k0 + (((int(knots[i + 1]) - k0) * r) >> g)


def positions(knots, g, j0, j1):
    """int64 array of the positions of output frames [j0, j1) (inside a checked call everything fits 63 bits)"""
    kn = np.asarray(knots, dtype=np.int64)
    j = np.arange(j0, j1, dtype=np.int64)
    i, r = j >> g, j & ((1 << g) - 1)
    nxt = kn[np.minimum(i + 1, len(kn) - 1)]
    return kn[i] + (((nxt - kn[i]) * r) >> g)                      # numpy's >> on int64 is arithmetic


def check(knots, n_kn, g, n_frames, out_frames, quality, guard_num, guard_den):
    """(status, reason) in the header's order; reason is a short tag, "" when accepted"""
    if n_frames == 0 or out_frames == 0 or n_frames >= MAX_FRAMES or out_frames >= MAX_FRAMES:
        return INVALID, "frames"
    if g < 4 or g > 10:
        return INVALID, "knot_shift"
    if knots is None:
        return INVALID, "null"
    K = n_knots(out_frames, g)
    if n_kn != K:
        return INVALID, "n_knots"
    if quality not in RM.QUALITY:
        return INVALID, "quality"
    if guard_num == 0 or guard_den == 0 or guard_num < guard_den:
        return INVALID, "guard"
    if K > MAX_KNOTS:
        return UNSUPPORTED, "knots"
    try:
        p = plan(quality, guard_num, guard_den)
    except Refused as e:
        return e.status, "taps"
    kn = [int(v) for v in knots]
    lo, hi = -(MARGIN << 32), (n_frames + MARGIN) << 32
    if any(v < lo or v > hi for v in kn):
        return INVALID, "bounds"
    for i in range(K - 1):
        if (abs(kn[i + 1] - kn[i]) >> 32) + 2 + p["T"] > SPAN_MAX:
            return UNSUPPORTED, "interval %d" % i
    return OK, ""


def tiles(knots, out_frames, g, p):
    """[(first_out, n_out, lo_frame, span)]: greedy runs of whole intervals, <= 1024 outputs, max_f - min_f + T <= 4096"""
    f = [int(v) >> 32 for v in knots]
    n_int, per = (out_frames + (1 << g) - 1) >> g, TILE_MAX >> g
    out, i = [], 0
    while i < n_int:
        mn = mx = f[i]
        cnt = 0
        while cnt < per and i + cnt < n_int:
            a, b = min(mn, f[i + cnt + 1]), max(mx, f[i + cnt + 1])
            if cnt and b - a + p["T"] > SPAN_MAX:
                break
            mn, mx, cnt = a, b, cnt + 1
        first = i << g
        out.append((first, min((i + cnt) << g, out_frames) - first, mn - (p["H"] - 1), mx - mn + p["T"]))
        i += cnt
    return out


def varispeed(planes, first, n, out_frames, knots, g, quality, guard_num=1, guard_den=1, window=None, tabs=None):
    """planes: [C] float32 arrays holding at least frames [first, first + n) of the source -> [C] float32 arrays of the
    result, or of its output frames window = (j0, j1) only.  Frames outside the range count as zero."""
    p = plan(quality, guard_num, guard_den)
    H, T, s = p["H"], p["T"], p["s"]
    j0, j1 = (0, out_frames) if window is None else window
    assert 0 <= j0 <= j1 <= out_frames
    h, D = tables(quality, guard_num, guard_den) if tabs is None else tabs
    h, D = h.astype(F64), D.astype(F64)
    pos = positions(knots, g, j0, j1)
    f, fr = pos >> 32, pos & 0xFFFFFFFF
    ph = fr >> s
    t = (fr & ((1 << s) - 1)).astype(F64) * F64(2.0) ** F64(-s)   # exact: at most 24 bits
    lo = int(f.min()) - (H - 1) if len(f) else 0
    hi = int(f.max()) + H + 1 if len(f) else 0
    out = []
    with np.errstate(all="ignore"):
        for plane in planes:
            x = np.zeros(hi - lo, dtype=F64)                      # the range's frames lo .. hi - 1, zero outside [0, n)
            a, b = max(lo, 0), min(hi, n)
            if b > a:
                x[a - lo:b - lo] = np.asarray(plane[first + a:first + b], dtype=F32)
            A = np.zeros(len(pos), dtype=F64)
            B = np.zeros(len(pos), dtype=F64)
            base = f - (H - 1) - lo
            for k in range(T):
                xk = x[base + k]
                A = A + h[ph, k] * xk                             # (fp32 x fp32 is exact in fp64: the device's fma is this)
                B = B + D[ph, k] * xk
            y = np.ascontiguousarray((A + t * B).astype(F32))     # one multiplication, one addition, one rounding
            y.view(np.uint32)[np.isnan(y)] = RM.CANON_NAN
            out.append(y)
    return out


def constant_knots(out_frames, g, num, den, start=0):
    """the knots of the constant speed num / den from position `start` (2^-32 frames): floor(i G num 2^32 / den)"""
    G = 1 << g
    return np.array([start + (i * G * num << 32) // den for i in range(n_knots(out_frames, g))], dtype=np.int64)
