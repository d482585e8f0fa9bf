"""Host model of wbx_clip_measure / wbx_clip_derive (include/wbx.h "Editing clips"): numpy, fp32 and fp64, the header's
formulas operation for operation — what tests/bounce_util.py and tests/record_model.py are for their features.  Every fp32
step is one numpy float32 operation (IEEE round to nearest, no contraction); the fade position is one fp64 division rounded
to fp32; there is no libm call, so the device must reproduce every bit.  A NaN result is the quiet NaN 0x7FC00000 whatever
produced it: the stored bits then do not depend on a processor's NaN conventions (inf * 0 is 0xFFC00000 on x86)."""
import math

import numpy as np

F32 = np.float32
REVERSE = 1
KEEP, SWAP, LEFT, RIGHT, MONO_MIX, DUAL_MONO = range(6)
LINEAR, SQUARE, SMOOTH = range(3)
MODES_FOR = {1: (KEEP, DUAL_MONO), 2: (KEEP, SWAP, LEFT, RIGHT, MONO_MIX)}
CANON_NAN = np.uint32(0x7FC00000)


def fade_weights(k, length, shape):
    """w(t) for t = (float)((double)k / (double)length), k an integer array"""
    t = (np.asarray(k, dtype=np.float64) / np.float64(length)).astype(F32)
    if shape == LINEAR:
        return t
    tt = (t * t).astype(F32)
    if shape == SQUARE:
        return tt
    assert shape == SMOOTH
    return (tt * (F32(3.0) - (F32(2.0) * t).astype(F32)).astype(F32)).astype(F32)


def out_channels(src_channels, mode):
    assert mode in MODES_FOR[src_channels], "the channel mode does not fit the source"
    return {KEEP: src_channels, SWAP: 2, LEFT: 1, RIGHT: 1, MONO_MIX: 1, DUAL_MONO: 2}[mode]


def derive(planes, first, n, reverse=False, mode=KEEP, gain=1.0, fade_in=0, fade_out=0, shape_in=LINEAR, shape_out=LINEAR):
    """planes: [C] float32 arrays of the whole source clip -> [C'] float32 arrays of n frames"""
    src = [np.asarray(p, dtype=F32) for p in planes]
    assert 0 < n and first + n <= len(src[0]) and fade_in <= n and fade_out <= n
    idx = first + np.arange(n, dtype=np.int64)
    if reverse:
        idx = idx[::-1]
    with np.errstate(all="ignore"):
        if mode == KEEP:
            xs = [p[idx] for p in src]
        elif mode == SWAP:
            xs = [src[1][idx], src[0][idx]]
        elif mode == LEFT:
            xs = [src[0][idx]]
        elif mode == RIGHT:
            xs = [src[1][idx]]
        elif mode == MONO_MIX:
            xs = [((src[0][idx] + src[1][idx]).astype(F32) * F32(0.5)).astype(F32)]
        else:
            assert mode == DUAL_MONO and len(src) == 1
            xs = [src[0][idx], src[0][idx]]
        assert len(xs) == out_channels(len(src), mode)
        j = np.arange(n, dtype=np.int64)
        out = []
        for x in xs:
            y = (x * F32(gain)).astype(F32)
            if fade_in:
                m = j < fade_in
                y[m] = (y[m] * fade_weights(j[m], fade_in, shape_in)).astype(F32)
            if fade_out:
                m = j >= n - fade_out
                y[m] = (y[m] * fade_weights(n - 1 - j[m], fade_out, shape_out)).astype(F32)
            y = np.ascontiguousarray(y, dtype=F32)
            y.view(np.uint32)[np.isnan(y)] = CANON_NAN
            out.append(y)
    return out


def order_key(x):
    """bits of non-NaN floats -> unsigned keys with the floats' order, -0.0 below +0.0"""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def exact_sum(*parts, bits):
    """math.fsum over all of `parts` — the correctly rounded sum — for finite fp64 arrays whose values have at most `bits`
    significant bits each, 2^(53 - bits) values at the most: the values of one binade are multiples of 2^(e - bits) below 2^e,
    so every partial sum of up to 2^(53 - bits) of them is exact in fp64, in any order; math.fsum then adds the few hundred
    binade sums.  (math.fsum over 10^7 values one by one takes a second; this takes a tenth)"""
    groups = []
    for d in parts:
        assert d.dtype == np.float64 and d.size <= 1 << (53 - bits)
        e = np.frexp(d)[1]
        groups.append(np.bincount(e - e.min(), weights=d) if d.size else np.zeros(0))
    return math.fsum(np.concatenate(groups))


def split26(d):
    """Veltkamp's split: d = hi + lo exactly, each part of at most 26 significant bits (d finite, |d| < 2^990)"""
    c = d * np.float64(134217729.0)                               # 2^27 + 1
    hi = c - (c - d)
    return hi, d - hi


def measure(planes, first=0, n=None):
    """the exact fields of wbx_clip_stats per channel, and sum / sum_sq as math.fsum of the fp64 terms (through exact_sum: the
    same correctly rounded value) with `abs_sum` / `abs_sum_sq` (the sums of their magnitudes, for the error bound)"""
    st = {k: [] for k in ("peak", "peak_frame", "min", "max", "over", "nans", "sum", "sum_sq", "abs_sum", "abs_sum_sq")}
    for p in planes:
        x = np.ascontiguousarray(np.asarray(p, dtype=F32)[first:None if n is None else first + n])
        nan = np.isnan(x)
        a = np.abs(x)
        a[nan] = 0
        peak = a.max() if a.size else F32(0)          # max |x| by `a > peak` from 0: NaNs never raise it
        st["peak"].append(F32(peak))
        st["peak_frame"].append(int(np.flatnonzero(a == peak)[0]) if peak > 0 else 0)
        good = x[~nan]
        if good.size:
            k = order_key(good)
            st["min"].append(good[np.argmin(k)])
            st["max"].append(good[np.argmax(k)])
        else:
            st["min"].append(F32(0.0))
            st["max"].append(F32(0.0))
        with np.errstate(invalid="ignore"):
            st["over"].append(int(np.count_nonzero((x > 1.0) | (x < -1.0))))
        st["nans"].append(int(np.count_nonzero(nan)))
        d = good.astype(np.float64)
        with np.errstate(all="ignore"):
            finite = bool(np.all(np.isfinite(d)))
            st["sum"].append(exact_sum(d, bits=24) if finite else float(np.sum(d)))
            st["sum_sq"].append(exact_sum(*split26(d * d), bits=26) if finite else float(np.sum(d * d)))   # (fp32 x fp32 is exact in fp64)
            st["abs_sum"].append(exact_sum(np.abs(d), bits=24) if finite else math.inf)
            st["abs_sum_sq"].append(st["sum_sq"][-1] if finite else math.inf)           # (squares: their own magnitudes)
    return st


EXACT = ("peak", "peak_frame", "min", "max", "over", "nans")


def exact_fields_equal(got, want):
    """peak, min and max as bit patterns (so -0.0 shows), the counters as integers"""
    for k in EXACT:
        for g, w in zip(got[k], want[k]):
            if k in ("peak", "min", "max"):
                if F32(g).tobytes() != F32(w).tobytes():
                    return False
            elif int(g) != int(w):
                return False
    return True


def normalize_gain(target, peak):
    """one IEEE fp32 division"""
    return F32(target) / F32(peak)
