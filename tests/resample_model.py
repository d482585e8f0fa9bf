"""Host model of wbx_clip_resample (include/wbx.h "Converting a clip's sample rate"): the plan, the coefficient table and
the convolution in numpy, the header's formulas operation for operation — what tests/clipfx_model.py is for the edits.
Every fp64 step is one IEEE operation (+ - * / floor sqrt, no libm, no pairwise summation), so the library's table and the
device's output must reproduce every bit.  A NaN result is the quiet NaN 0x7FC00000 (inf - inf is 0xFFC00000 on x86)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
FAST, GOOD, BEST = range(3)
QUALITY = {FAST: (12, 7.0, 0.85), GOOD: (24, 10.0, 0.92), BEST: (48, 14.0, 0.96)}   # Z, beta, frac
MAX_L, MAX_TAPS, MAX_FRAMES = 1280, 512, (1 << 31) - 16
SIN_TERMS, I0_TERMS = 13, 40
PI = F64(3.141592653589793)
CANON_NAN = np.uint32(0x7FC00000)
INVALID, UNSUPPORTED = -4, -3


class Refused(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(status)


def plan(src_rate, dst_rate, quality):
    """{L, M, H, T, cutoff, beta}; Refused(status) as wbx_resample_plan refuses"""
    if quality not in QUALITY or src_rate == 0 or dst_rate == 0 or src_rate == dst_rate:
        raise Refused(INVALID)
    Z, beta, frac = QUALITY[quality]
    g = math.gcd(src_rate, dst_rate)
    L, M = dst_rate // g, src_rate // g
    if L > MAX_L:
        raise Refused(UNSUPPORTED)
    H = (Z * M + L - 1) // L if L < M else Z
    if 2 * H > MAX_TAPS:
        raise Refused(UNSUPPORTED)
    rho = F64(L) / F64(M) if L < M else F64(1.0)
    return dict(L=L, M=M, H=H, T=2 * H, cutoff=F64(frac) * rho, beta=F64(beta))


def out_frames(src_rate, dst_rate, n):
    """ceil(n L / M); 0 where that reaches 2^31 - 16"""
    g = math.gcd(src_rate, dst_rate)
    L, M = dst_rate // g, src_rate // g
    n_out = (n * L + M - 1) // M
    return n_out if n_out < MAX_FRAMES else 0


def sinpi(x):
    x = np.asarray(x, dtype=F64)
    neg = x < 0.0
    a = np.where(neg, F64(0.0) - x, x)
    sign = np.where(neg, F64(-1.0), F64(1.0))
    r = a - F64(2.0) * np.floor(a / F64(2.0))
    hi = r >= 1.0
    r = np.where(hi, r - F64(1.0), r)
    sign = np.where(hi, F64(0.0) - sign, sign)
    r = np.where(r > 0.5, F64(1.0) - r, r)
    y = PI * r
    y2 = y * y
    s = np.ones_like(y)
    for n in range(SIN_TERMS, 0, -1):
        s = F64(1.0) - (s * y2) / F64((2 * n) * (2 * n + 1))
    return sign * (y * s)


def sinc(x):
    x = np.asarray(x, dtype=F64)
    zero = x == 0.0
    den = PI * np.where(zero, F64(1.0), x)
    return np.where(zero, F64(1.0), sinpi(x) / den)


def i0(x):
    h = np.asarray(x, dtype=F64) / F64(2.0)
    t = np.ones_like(h)
    s = np.ones_like(h)
    for k in range(1, I0_TERMS):
        t = (t * h) / F64(k)
        s = s + t * t
    return s


def _distances(p):
    k = np.arange(p["T"], dtype=np.int64)[None, :] - (p["H"] - 1)
    frac = np.arange(p["L"], dtype=F64)[:, None] / F64(p["L"])
    return k.astype(F64) - frac                                   # d[p][k]


def table(src_rate, dst_rate, quality):
    """[L][T] float32, phase order"""
    p = plan(src_rate, dst_rate, quality)
    d = _distances(p)
    u = d / F64(p["H"])
    w = F64(1.0) - u * u
    w = np.where(w < 0.0, F64(0.0), w)
    v = ((p["cutoff"] * sinc(p["cutoff"] * d)) * i0(p["beta"] * np.sqrt(w))) / i0(p["beta"])
    total = np.zeros(p["L"], dtype=F64)
    for k in range(p["T"]):                                       # ascending k, never numpy's pairwise sum
        total = total + v[:, k]
    return (v / total[:, None]).astype(F32)


def table_numpy(src_rate, dst_rate, quality):
    """the same formula through np.sinc / np.i0 / math.fsum, fp64: the independent yardstick of the table"""
    p = plan(src_rate, dst_rate, quality)
    d = _distances(p)
    v = p["cutoff"] * np.sinc(p["cutoff"] * d) * np.i0(p["beta"] * np.sqrt(np.maximum(0.0, 1.0 - (d / p["H"]) ** 2))) / np.i0(p["beta"])
    return v / np.array([math.fsum(row) for row in v])[:, None]


def resample(planes, first, n, src_rate, dst_rate, quality, window=None, tab=None):
    """planes: [C] float32 arrays holding at least frames [first, first + n) of the source -> [C] float32 arrays of the
    result, or of its output frames window = (j0, j1) only.  Frames outside the range count as zero."""
    p = plan(src_rate, dst_rate, quality)
    L, M, H, T = p["L"], p["M"], p["H"], p["T"]
    n_out = out_frames(src_rate, dst_rate, n)
    assert n_out, "refused"
    j0, j1 = (0, n_out) if window is None else window
    assert 0 <= j0 <= j1 <= n_out
    h = (table(src_rate, dst_rate, quality) if tab is None else tab).astype(F64)
    t = np.arange(j0, j1, dtype=np.int64) * M                     # 64-bit positions
    i, ph = t // L, t % L
    lo = int(i[0]) - (H - 1) if len(i) else 0                     # first source frame any tap touches (may be < 0)
    hi = (int(i[-1]) + H + 1) if len(i) else 0
    out = []
    with np.errstate(all="ignore"):
        for plane in planes:
            x = np.zeros(hi - lo, dtype=F64)                      # the range's frames lo .. hi - 1, zero outside [0, n)
            a, b = max(lo, 0), min(hi, n)
            if b > a:
                x[a - lo:b - lo] = np.asarray(plane[first + a:first + b], dtype=F32)
            acc = np.zeros(len(t), dtype=F64)
            base = i - (H - 1) - lo
            for k in range(T):
                acc = acc + h[ph, k] * x[base + k]                # (fp32 x fp32 is exact in fp64: the device's fma is this)
            y = np.ascontiguousarray(acc.astype(F32))
            y.view(np.uint32)[np.isnan(y)] = CANON_NAN
            out.append(y)
    return out
