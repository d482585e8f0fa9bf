"""Host model of wbx_clip_saturate, wbx_saturate_table, wbx_saturate_check, wbx_saturate_lookup and
wbx_saturate_launch_shape (include/wbx.h "Saturating a clip") in numpy, the header's formulas operation for operation.  The
two conversions are tests/resample_model.py's, used as they are (L = os, M = 1, then L = 1, M = os); the tanh table's exp2
is tests/dynamics_model.py's.  What is restated here: the lookup, the table's design, the statistics, the argument check
and its order, the launch shape, and the composition.  Every fp64 step is one IEEE operation, so the library's table, the
device's statistics and every output sample must reproduce every bit."""
import functools

import numpy as np

import dynamics_model as DM
import resample_model as RM

F32, F64 = np.float32, np.float64
HARD, CUBIC, TANH = range(3)
TABLE, CELLS, EDGE = 16385, F64(1024.0), F64(8192.0)
MAX_GAIN, MAX_BIAS = 2.0 ** 32, 4.0
LOG2E = F64(1.4426950408889634)
CUBIC_C = F64(4.0) / F64(27.0)
MAX_MID = (1 << 31) - 16
TILE_MAX, TILE_STEP, LDS_MAX = 1024, 256, 65536
INVALID, UNSUPPORTED = -4, -3
Refused = RM.Refused
FAST, GOOD, BEST = RM.FAST, RM.GOOD, RM.BEST


# ---- the table's design -------------------------------------------------------------------------------------------------------
def curve(kind, z):
    """f(z) of the three designs on a vector"""
    z = np.asarray(z, dtype=F64)
    if kind == HARD:
        return np.where(z < -1.0, F64(-1.0), np.where(z > 1.0, F64(1.0), z))
    if kind == CUBIC:
        mid = z - (CUBIC_C * z) * (z * z)
        return np.where(z >= 1.5, F64(1.0), np.where(z <= -1.5, F64(-1.0), mid))
    a = np.abs(z)
    e = DM.exp2((F64(-2.0) * a) * LOG2E)
    t = (F64(1.0) - e) / (F64(1.0) + e)
    return np.where(z < 0.0, F64(0.0) - t, t)


def table(kind, bias=0.0):
    """wbx_saturate_table"""
    bias = F64(bias)
    if kind not in (HARD, CUBIC, TANH) or not abs(bias) <= MAX_BIAS:
        raise Refused(INVALID)
    v = (np.arange(TABLE, dtype=F64) - EDGE) / CELLS
    return curve(kind, v + bias) - curve(kind, np.array([bias]))[0]


def check(tab):
    """wbx_saturate_check: 0, or INVALID"""
    tab = np.asarray(tab, dtype=F64)
    with np.errstate(invalid="ignore"):
        return 0 if tab.shape == (TABLE,) and bool(np.all(np.abs(tab) <= MAX_GAIN)) else INVALID


def lookup(tab, d):
    """the lookup on a vector of driven samples d (no NaN) -> (w, past): past where |a| >= 8192"""
    tab = np.asarray(tab, dtype=F64)
    d = np.asarray(d, dtype=F64)
    with np.errstate(all="ignore"):
        a = d * CELLS
        low, high = a <= -EDGE, a >= EDGE
        past = low | high
        safe = np.where(past, F64(0.0), a)
        fl = np.floor(safe)
        idx = fl.astype(np.int64) + 8192
        f = safe - fl
        w = tab[idx] + f * (tab[idx + 1] - tab[idx])
    return np.where(low, tab[0], np.where(high, tab[TABLE - 1], w)), past


# ---- the call -----------------------------------------------------------------------------------------------------------------
def check_args(n, os, quality, tab, drive, makeup):
    """the arithmetic of a call, judged without a clip, in the header's order: 0, INVALID or UNSUPPORTED.  tab None: NULL"""
    if n == 0 or os not in (1, 2, 4, 8) or quality not in RM.QUALITY:
        return INVALID
    if tab is None or check(tab) != 0:
        return INVALID
    drive, makeup = F64(drive), F64(makeup)
    if not (np.isfinite(drive) and 0.0 < abs(drive) <= MAX_GAIN):
        return INVALID
    if not abs(makeup) <= MAX_GAIN:
        return INVALID
    if n * os >= MAX_MID:
        return INVALID
    if os > 1:
        try:
            RM.plan(1, os, quality)
            RM.plan(os, 1, quality)
        except Refused as r:
            return r.status
    return 0


def launch_shape(os, quality, channels, n):
    """wbx_saturate_launch_shape: {tile, mid_span, src_span, lds_bytes, n_tiles}"""
    tile = TILE_MAX
    if os == 1:
        return dict(tile=tile, mid_span=tile, src_span=tile, lds_bytes=0, n_tiles=-(-n // tile))
    Z = RM.QUALITY[quality][0]

    def lds(t):
        return channels * 4 * ((t + 2 * Z) * os + t + 4 * Z)
    while tile > TILE_STEP and lds(tile) > LDS_MAX:
        tile -= TILE_STEP
    return dict(tile=tile, mid_span=(tile + 2 * Z) * os, src_span=tile + 4 * Z - 1, lds_bytes=lds(tile), n_tiles=-(-n // tile))


@functools.lru_cache(maxsize=None)
def _filter(src_rate, dst_rate, quality):
    return RM.table(src_rate, dst_rate, quality)


def shape(u_planes, tab, drive, makeup):
    """[C] float32 arrays of mid samples -> ([C] float32 arrays s, the statistics)"""
    drive, makeup = F64(drive), F64(makeup)
    out, peak, index, beyond = [], F64(-1.0), 0, 0
    with np.errstate(all="ignore"):
        for u in u_planes:
            u = np.asarray(u, dtype=F32)
            d = np.where(np.isfinite(u), drive * u.astype(F64), F64(0.0))
            w, past = lookup(tab, d)
            out.append(np.ascontiguousarray((w * makeup).astype(F32)))
            mag = np.abs(d)
            top = mag.max()
            at = int(np.argmax(mag == top))                        # the lowest j that has it
            if top > peak or (top == peak and at < index):
                peak, index = top, at
            beyond += int(past.sum())
    return out, dict(peak_drive=float(peak), peak_index=index, beyond=beyond)


def saturate(planes, first, n, os, quality, tab, drive=1.0, makeup=1.0):
    """planes: [C] float32 arrays holding at least frames [first, first + n) -> ([C] float32 arrays of n frames, the
    statistics): up, shape, down — the three calls in a row"""
    assert check_args(n, os, quality, tab, drive, makeup) == 0, "refused"
    if os == 1:
        return shape([np.asarray(p[first:first + n], dtype=F32) for p in planes], tab, drive, makeup)
    u = RM.resample(planes, first, n, 1, os, quality, tab=_filter(1, os, quality))
    s, stats = shape(u, tab, drive, makeup)
    return RM.resample(s, 0, n * os, os, 1, quality, tab=_filter(os, 1, quality)), stats
