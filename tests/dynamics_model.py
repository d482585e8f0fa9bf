"""Host model of wbx_clip_dynamics, wbx_dynamics_table, wbx_dynamics_check and wbx_dynamics_lookup (include/wbx.h "Dynamics
of a clip") in numpy, the header's formulas operation for operation — what tests/limit_model.py is for the limiter, whose
ramp it uses.  Every fp64 step is one IEEE operation; the curve's minimum / maximum is exact in any order (one vector
operation per term here), the gain's sum runs in ascending frame order, so the library's table, the device's statistics
and every output frame must reproduce every bit."""
import numpy as np

import limit_model as LM

F32, F64 = np.float32, np.float64
TILE, SEGMENT, BAND = LM.TILE, LM.SEGMENT, LM.BAND
COMPRESS, GATE = 0, 1
MIN_EXP, MAX_EXP, CELLS = -40, 8, 64
TABLE = (MAX_EXP - MIN_EXP) * CELLS + 1
MAX_GAIN, MAX_DB = 2.0 ** 32, 1000.0
DB_PER_OCTAVE, TWO_OVER_LN2, LN2, SQRT2 = F64(6.020599913279624), F64(2.8853900817779268), F64(0.6931471805599453), F64(1.4142135623730951)
LOG_TERMS, EXP_TERMS = 12, 16
CANON_NAN = np.uint32(0x7FC00000)
INVALID, UNSUPPORTED = -4, -3
Refused = LM.Refused


# ---- the table's design -------------------------------------------------------------------------------------------------------
def log2_mantissa(m):
    """wbx_dynamics.h's dyn_log2_mantissa on a vector of m in [1, 2)"""
    m = np.asarray(m, dtype=F64)
    big = m > SQRT2
    whole = np.where(big, F64(1.0), F64(0.0))
    m = np.where(big, m / F64(2.0), m)
    s = (m - F64(1.0)) / (m + F64(1.0))
    s2 = s * s
    p = np.full_like(m, F64(1.0) / F64(2 * LOG_TERMS + 1))
    for n in range(LOG_TERMS - 1, -1, -1):
        p = p * s2 + F64(1.0) / F64(2 * n + 1)
    return whole + (s * p) * TWO_OVER_LN2


def exp2(y):
    """dyn_exp2 on a vector of y <= 0 (-inf included)"""
    y = np.asarray(y, dtype=F64)
    zero = y < F64(-1021.0)
    ys = np.where(zero, F64(0.0), y)
    i = np.floor(ys + F64(0.5))
    t = (ys - i) * LN2
    p = np.ones_like(ys)
    for n in range(EXP_TERMS, 0, -1):
        p = F64(1.0) + (p * t) / F64(n)
    scale = ((i.astype(np.int64) + 1023) << 52).view(F64)
    return np.where(zero, F64(0.0), p * scale)


def entry_levels():
    """(e, k) of every entry: its level is 2^e * (1 + k / 64)"""
    t = np.arange(TABLE, dtype=np.int64)
    return t // CELLS + MIN_EXP, t % CELLS


def entry_octaves():
    e, k = entry_levels()
    return e.astype(F64) + log2_mantissa(F64(1.0) + k.astype(F64) / F64(CELLS))


def table(kind, threshold_db, ratio, knee_db=0.0, range_db=-np.inf):
    """wbx_dynamics_table"""
    T_db, ratio, knee, rng = F64(threshold_db), F64(ratio), F64(knee_db), F64(range_db)
    if kind not in (COMPRESS, GATE) or not np.isfinite(T_db) or abs(T_db) > MAX_DB:
        raise Refused(INVALID)
    if not ratio >= 1.0 or (kind == GATE and not np.isfinite(ratio)):
        raise Refused(INVALID)
    if not knee >= 0.0 or not knee <= MAX_DB or not rng <= 0.0:
        raise Refused(INVALID)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        T, W, floor_oct = T_db / DB_PER_OCTAVE, knee / DB_PER_OCTAVE, rng / DB_PER_OCTAVE
        half = W / F64(2.0)
        slope = F64(1.0) / ratio - F64(1.0) if kind == COMPRESS else ratio - F64(1.0)
        over = entry_octaves() - T
        two = F64(2.0) * over
        if kind == COMPRESS:
            one = two <= F64(0.0) - W
            knee_at = ~one & (two < W)
            u = over + half
            y = np.where(knee_at, slope * ((u * u) / (F64(2.0) * W)), slope * over)
        else:
            one = two >= W
            knee_at = ~one & (two > F64(0.0) - W)
            u = over - half
            y = np.where(knee_at, F64(0.0) - slope * ((u * u) / (F64(2.0) * W)), slope * over)
        y = np.where(one, F64(0.0), y)
        y = np.where(y < floor_oct, floor_oct, y)
        return np.where(one, F64(1.0), exp2(y))


def table_check(tab, sense=COMPRESS):
    """wbx_dynamics_check: the smallest entry, or Refused"""
    if tab is None or sense not in (COMPRESS, GATE):
        raise Refused(INVALID)
    tab = np.ascontiguousarray(tab, dtype=F64)
    if tab.shape != (TABLE,) or np.any(tab.view(np.uint64) >> np.uint64(63)) or not np.all(tab <= 1.0):
        raise Refused(INVALID)
    return F64(tab.min())


def lookup(tab, p):
    """wbx_dynamics_lookup on a vector of levels p >= 0"""
    p = np.ascontiguousarray(p, dtype=F64)
    u = p.view(np.uint64)
    m = u & np.uint64((1 << 52) - 1)
    e = (u >> np.uint64(52)).astype(np.int64)
    idx = np.clip((e - (1023 + MIN_EXP)) * CELLS + (m >> np.uint64(46)).astype(np.int64), 0, TABLE - 2)
    f = (m & np.uint64((1 << 46) - 1)).astype(F64) * F64(2.0 ** -46)
    mid = tab[idx] + f * (tab[idx + 1] - tab[idx])
    return np.where(p < F64(2.0 ** -40), tab[0], np.where(p >= F64(256.0), tab[TABLE - 1], mid))


# ---- a call -------------------------------------------------------------------------------------------------------------------
def gain_ok(g):
    g = F64(g)
    return bool(np.isfinite(g) and abs(g) > 0.0 and abs(g) <= MAX_GAIN)


def check_args(n, tab, sense, drive, key_gain, makeup, A, H, R, keyed=False):
    """wbx_dynamics.h's dynamics_check_args: the status a call gets before its clips are looked at (0: none)"""
    if n == 0 or sense not in (COMPRESS, GATE) or tab is None:
        return INVALID
    try:
        table_check(tab, sense)
    except Refused:
        return INVALID
    if not gain_ok(drive) or (keyed and not gain_ok(key_gain)):
        return INVALID
    if not np.isfinite(F64(makeup)) or not F64(makeup) >= 0.0:
        return INVALID
    if not LM.shape_ok(A, H, R) or n >= LM.MAX_FRAMES:
        return INVALID
    if n * (A + H + R) > LM.MAX_WORK:
        return UNSUPPORTED
    return 0


def level(planes, gain):
    d = LM.driven(planes, gain)
    p = np.abs(d[0])
    for q in d[1:]:
        p = np.maximum(p, np.abs(q))
    return d, p


def gains(planes, tab, sense, drive=1.0, A=72, H=0, R=4800, key=None, key_gain=1.0):
    """planes / key: the RANGES' fp32 planes.  (d, p, want, y, g): y holds the curve frames j = -A .. n - 1 at [j + A]"""
    tab = np.ascontiguousarray(tab, dtype=F64)
    d, p = level(planes, drive)
    if key is not None:
        _, p = level(key, key_gain)
    n = len(d[0])
    assert len(p) == n
    want = lookup(tab, p)
    rest = F64(1.0) if sense == COMPRESS else F64(tab.min())
    ramp = LM.ramp(A, H, R)
    K = len(ramp)
    # wantp[K - 1 + i] = want[i], rest outside: curve frame m = j + A, term t = k + A reads wantp[K - 1 + m - t]
    wantp = np.full(n + A + 2 * (K - 1), rest, dtype=F64)
    wantp[K - 1:K - 1 + n] = want
    y = np.full(n + A, rest, dtype=F64)
    for t in range(K if np.any(want != rest) else 0):           # (want all rest: no term moves the curve)
        w = wantp[K - 1 - t:K - 1 - t + n + A]
        y = np.minimum(y, w + ramp[t]) if sense == COMPRESS else np.maximum(y, w - ramp[t])
    acc = np.zeros(n, dtype=F64)
    for u in range(A + 1):                                      # j = i - A + u ascending
        acc = acc + y[u:u + n]
    g = acc / F64(A + 1)
    return d, p, want, y, g


def dynamics_clip(src, first, n, tab, sense, drive=1.0, makeup=1.0, A=72, H=0, R=4800, key=None, key_first=0, key_gain=1.0):
    """src / key: lists of fp32 planes (1 or 2 each).  (the result's planes, the statistics as wbx_dynamics_stats has them)"""
    kp = None if key is None else [q[key_first:key_first + n] for q in key]
    d, p, want, y, g = gains([q[first:first + n] for q in src], tab, sense, drive, A, H, R, kp, key_gain)
    out = []
    for q in d:
        with np.errstate(over="ignore", invalid="ignore"):
            v = ((q * g) * F64(makeup)).astype(F32)
        bits = v.view(np.uint32).copy()
        bits[np.isnan(v)] = CANON_NAN
        out.append(bits.view(F32))
    at = int(np.argmin(g))                                      # (numpy: the first of equal minima)
    return out, {"min_gain": float(g[at]), "min_gain_frame": at, "reduced_frames": int(np.count_nonzero(g < 1.0))}
