"""Host model of wbx_clip_align and the wbx_align_* host functions (include/wbx.h "Aligning two clips") in numpy, the header's
formulas operation for operation.  Every fp64 step is one IEEE operation: a partial is one np.add.accumulate — strictly
sequential, ascending — over a chunk's exact products (fp32 values times fp32 values) behind a leading 0.0, the chain's rest;
the fold adds the partials chunk by chunk, ascending — the two-level order the header defines; the pick takes the lowest of
equal lags.  The host functions are held as Python integers.  Every bit of the library's info and curve must come out of this."""
import numpy as np

import stretch_model as ST

F32, F64 = np.float32, np.float64
MIN_N, MAX_N, MAX_M = 64, 1 << 24, (1 << 31) - 16
MAX_LAG, MAX_LAGS = 1 << 24, 1 << 17
CHUNK = 2048
STAGE_RECORDS, LAUNCH_TERMS = 1 << 22, 1 << 39
BLOCK_LAGS, WAVE_LAGS = 4096, 512
EITHER = 1
INVALID, UNSUPPORTED = -4, -3
CURVE_DTYPE = np.dtype([("r", "<f8"), ("energy", "<f8")])
INFO_FIELDS = ["lag", "inverted", "offset", "score", "r", "energy", "ref_energy", "confidence", "lags", "chunks", "terms", "launches"]


def n_ok(n):
    return MIN_N <= n <= MAX_N and n % 8 == 0


def chunks(n):
    """wbx_align_chunks: ceil(n / C); 0 for an n the call refuses"""
    return -(-n // CHUNK) if n_ok(n) else 0


def check(n, m, lag_min, lag_max, flags=0, has_info=True, has_curve=False, cap=0):
    """wbx_align_check: the status a call gets before its clips are looked at (0: none)"""
    if not n_ok(n):
        return INVALID
    if not 1 <= m < MAX_M:
        return INVALID
    if not -MAX_LAG <= lag_min <= MAX_LAG:
        return INVALID
    if not -MAX_LAG <= lag_max <= MAX_LAG:
        return INVALID
    if lag_min > lag_max:
        return INVALID
    if flags & ~EITHER:
        return INVALID
    if not has_info and not has_curve:
        return INVALID
    lags = lag_max - lag_min + 1
    if has_curve and cap < lags:
        return INVALID
    if lags > MAX_LAGS:
        return UNSUPPORTED
    return 0


def band_chunks(lags):
    """wbx_align_band_chunks: what the stage holds and what stays within the launch's terms, at least 1; 0 for refused lags"""
    if not 1 <= lags <= MAX_LAGS:
        return 0
    return max(1, min(STAGE_RECORDS // lags, LAUNCH_TERMS // (lags * CHUNK)))


def bands(n, lags):
    c, per = chunks(n), band_chunks(lags)
    return -(-c // per) if c and per else 0


def launches(n, lags):
    """wbx_align_launches: Ea's partials, a partial and a fold launch per band, the pick"""
    b = bands(n, lags)
    return 2 * b + 2 if b else 0


def shape(lags):
    """wbx_align.h's align_shape: (waves of a workgroup, lag blocks)"""
    return -(-min(lags, BLOCK_LAGS) // WAVE_LAGS), -(-lags // BLOCK_LAGS)


def span_words(terms, waves):
    return terms + WAVE_LAGS * waves + 16


def _chain(prod):
    """the ascending chain from rest over the rows of prod [rows][terms]: its last value per row"""
    z = np.zeros((prod.shape[0], 1), dtype=F64)
    return np.add.accumulate(np.concatenate([z, prod], axis=1), axis=1)[:, -1]


def curve(da, db, lag_list, batch=256):
    """(r, E) at the lags of lag_list (any order): da, db the detectors as fp64 values that are fp32 values"""
    da, db = np.asarray(da, dtype=F64), np.asarray(db, dtype=F64)
    n, m = len(da), len(db)
    L = np.asarray(lag_list, dtype=np.int64)
    r, E = np.zeros(len(L), dtype=F64), np.zeros(len(L), dtype=F64)
    for at in range(0, len(L), batch):
        Lb = L[at:at + batch]
        rb, Eb = np.zeros(len(Lb), dtype=F64), np.zeros(len(Lb), dtype=F64)
        for k in range(-(-n // CHUNK)):
            i = np.arange(k * CHUNK, min((k + 1) * CHUNK, n), dtype=np.int64)
            idx = i[None, :] + Lb[:, None]
            inside = (idx >= 0) & (idx < m)
            w = np.where(inside, db[np.clip(idx, 0, m - 1)], F64(0.0))     # zero outside [0, m)
            rb = rb + _chain(da[i][None, :] * w)
            Eb = Eb + _chain(w * w)
        r[at:at + batch], E[at:at + batch] = rb, Eb
    return r, E


def ref_energy(da):
    da = np.asarray(da, dtype=F64)
    Ea = F64(0.0)
    for k in range(-(-len(da) // CHUNK)):
        v = da[k * CHUNK:(k + 1) * CHUNK]
        Ea = Ea + _chain((v * v)[None, :])[0]
    return Ea


def score(r, E, either=False):
    r, E = np.asarray(r, dtype=F64), np.asarray(E, dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(E == 0.0, F64(0.0), (r * (r if either else np.abs(r))) / E)


def pick(r, E, lag_min, Ea, flags=0):
    """the pick and the refine over a WHOLE curve (r, E from lag_min upward): info's computed fields"""
    s = score(r, E, bool(flags & EITHER))
    q = int(np.argmax(s))                                       # (np.argmax: the first of equals)
    off = F64(0.0)
    if 1 <= q and q + 1 < len(s):
        a, b, g = s[q - 1], s[q], s[q + 1]
        den = (F64(2.0) * b) - (a + g)
        if den > 0.0 and b >= a and b >= g:
            off = (F64(0.5) * (g - a)) / den
    Ea = F64(Ea)
    return {"lag": lag_min + q, "inverted": int(r[q] < 0.0), "offset": float(off), "score": float(s[q]), "r": float(r[q]),
            "energy": float(E[q]), "ref_energy": float(Ea), "confidence": float(F64(0.0) if Ea == 0.0 else s[q] / Ea)}


def detector_of(planes, first, count):
    return ST.detector(ST.inputs([np.asarray(p)[first:first + count] for p in planes]))


def align_clips(planes_a, a_first, n, planes_b, b_first, m, lag_min, lag_max, flags=0, only=None):
    """wbx_clip_align of two clips given as their channel planes: (info, curve) — with `only` (lags), (None, the curve at
    those lags): the pick needs every lag"""
    da, db = detector_of(planes_a, a_first, n), detector_of(planes_b, b_first, m)
    lag_list = list(range(lag_min, lag_max + 1)) if only is None else [int(v) for v in only]
    assert all(lag_min <= v <= lag_max for v in lag_list)
    r, E = curve(da, db, lag_list)
    c = np.zeros(len(lag_list), dtype=CURVE_DTYPE)
    c["r"], c["energy"] = r, E
    if only is not None:
        return None, c
    lags = lag_max - lag_min + 1
    info = pick(r, E, lag_min, ref_energy(da), flags)
    info.update(lags=lags, chunks=chunks(n), terms=lags * n, launches=launches(n, lags))
    return info, c
