"""Host model of wbx_clip_limit and wbx_limit_ramp (include/wbx.h "Limiting a clip") in numpy, the header's formulas
operation for operation — what tests/convolve_model.py is for the convolution.  Every fp64 step is one IEEE operation; the
curve's minimum is exact in any order (one vector `y = min(y, need + ramp[k])` per term here), the gain's sum runs in
ascending frame order (one vector `acc = acc + y` per frame of the window), so the library's table, the device's
statistics and every output frame must reproduce every bit."""
import numpy as np

F32, F64 = np.float32, np.float64
TILE, SEGMENT, BAND = 2048, 2048, 1 << 20
MAX_LOOKAHEAD, MAX_HOLD, MAX_RELEASE = 4096, 65536, 1 << 20
MAX_WORK, MAX_FRAMES, MAX_DRIVE = 1 << 44, (1 << 31) - 16, 2.0 ** 32
FLT_MIN = float(np.finfo(F32).tiny)
CANON_NAN = np.uint32(0x7FC00000)
INVALID, UNSUPPORTED = -4, -3


class Refused(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(status)


def shape_ok(A, H, R):
    return 0 <= A <= MAX_LOOKAHEAD and 0 <= H <= MAX_HOLD and 1 <= R <= MAX_RELEASE


def check_args(n, ceiling, drive, A, H, R):
    """wbx_limit.h's limit_check_args: the status a call gets before its clip is looked at (0: none)"""
    c, d = F32(ceiling), F64(drive)
    if n == 0:
        return INVALID
    if not np.isfinite(c) or not c >= F32(FLT_MIN):
        return INVALID
    if not np.isfinite(d) or not abs(d) > 0.0 or not abs(d) <= MAX_DRIVE:
        return INVALID
    if not shape_ok(A, H, R):
        return INVALID
    if n >= MAX_FRAMES:
        return INVALID
    if n * (A + H + R) > MAX_WORK:
        return UNSUPPORTED
    return 0


def ramp(A, H, R):
    """wbx_limit_ramp: table[k + A] = ramp[k], k = -A .. H + R - 1"""
    if not shape_ok(A, H, R):
        raise Refused(INVALID)
    s = F64(1.0) / F64(R)
    k = np.arange(-A, H + R, dtype=np.int64)
    return np.where(k <= H, F64(0.0), (k - H).astype(F64) * s)


def driven(planes, drive):
    """d[c][i]: drive * (double) of the fp32 sample, what is not finite entering as 0.0"""
    out = []
    for p in planes:
        v = np.asarray(p, dtype=F32).astype(F64)
        out.append(F64(drive) * np.where(np.isfinite(v), v, F64(0.0)))
    return out


def gains(planes, ceiling, drive, A, H, R):
    """planes: the RANGE's fp32 planes.  (d, p, need, y, g): y holds the curve frames j = -A .. n - 1 at [j + A]"""
    c = F64(F32(ceiling))
    d = driven(planes, drive)
    n = len(d[0])
    p = np.abs(d[0])
    for q in d[1:]:
        p = np.maximum(p, np.abs(q))
    with np.errstate(divide="ignore"):
        need = np.where(p > c, c / np.where(p > c, p, F64(1.0)), F64(1.0))
    table = ramp(A, H, R)
    K = len(table)
    # needp[K - 1 + i] = need[i], 1.0 outside: curve frame m = j + A, term t = k + A reads needp[K - 1 + m - t]
    needp = np.ones(n + A + 2 * (K - 1), dtype=F64)
    needp[K - 1:K - 1 + n] = need
    y = np.ones(n + A, dtype=F64)
    for t in range(K if np.any(need < 1.0) else 0):             # (need all 1.0: no term is below 1.0)
        y = np.minimum(y, needp[K - 1 - t:K - 1 - t + n + A] + table[t])
    acc = np.zeros(n, dtype=F64)
    for u in range(A + 1):                                      # j = i - A + u ascending
        acc = acc + y[u:u + n]
    g = np.minimum(acc / F64(A + 1), need)
    return d, p, need, y, g


def limit_clip(src, first, n, ceiling, drive=1.0, A=72, H=0, R=4800):
    """src: a list of fp32 planes (1 or 2).  (the result's planes, the statistics as wbx_limit_stats has them)"""
    d, p, need, y, g = gains([q[first:first + n] for q in src], ceiling, drive, A, H, R)
    out = []
    for q in d:
        with np.errstate(over="ignore", invalid="ignore"):
            v = (q * g).astype(F32)
        bits = v.view(np.uint32).copy()
        bits[np.isnan(v)] = CANON_NAN
        out.append(bits.view(F32))
    at = int(np.argmin(g))                                      # (numpy: the first of equal minima)
    stats = {"peak_in": float(p.max()), "min_gain": float(g[at]), "min_gain_frame": at, "limited_frames": int(np.count_nonzero(g < 1.0))}
    return out, stats
