"""Host model of wbx_clip_spectrum, wbx_spectrum_hops / _check / _launch_hops / _basis_frames, wbx_spectrum_basis and
wbx_spectrum_log_freqs (include/wbx.h "Seeing a clip's spectrum") in numpy, the header's formulas operation for operation.
Every fp64 step is one IEEE operation: the two chains of a cell run in ascending term order (one vector
`re = re + d[t + i] * C[i]` per term, the hops and the bins side by side; no np.dot, whose order is not fixed), the products
of fp32 values are exact in fp64, and the power is two rounded products and a rounded sum.  The basis is built from
resample_model's sinpi and I0 and dynamics_model's exp2, as the header builds it from theirs.  Every bit of the library's
cells, basis words and frequencies must come out of this."""
import numpy as np

import dynamics_model as DM
import resample_model as RS
import stretch_model as ST

F32, F64 = np.float32, np.float64
MIN_WINDOW, MAX_WINDOW = 32, 8192
MAX_HOP, MAX_BINS, MAX_BASIS = 65536, 1024, 1 << 21
MAX_HOPS, MAX_CELLS, MAX_FRAMES = 1 << 20, 1 << 25, (1 << 31) - 16
STAGE_CELLS = 1 << 22
MID = 2
RECT, HANN, KAISER = 0, 1, 2
MAX_BETA = 20.0
INVALID, UNSUPPORTED = -4, -3


def shape_ok(W, B, H):
    return MIN_WINDOW <= W <= MAX_WINDOW and W % 4 == 0 and 1 <= B <= MAX_BINS and B * W <= MAX_BASIS and 1 <= H <= MAX_HOP


def hops(n, W, H):
    """wbx_spectrum_hops: only complete frames count; 0 for a window or hop length the call refuses"""
    if not shape_ok(W, 1, H):
        return 0
    return (n - W) // H + 1 if n >= W else 0


def basis_frames(W, B):
    return 2 * B * W if shape_ok(W, B, 1) else 0


def check(n, channel, W, B, H, has_out=True, cap=None):
    """wbx_spectrum_check: the status a call gets before its clips are looked at (0: none); cap None = as many as there are cells"""
    if n == 0 or n >= MAX_FRAMES:
        return INVALID
    if channel not in (0, 1, MID):
        return INVALID
    if not (MIN_WINDOW <= W <= MAX_WINDOW and W % 4 == 0):
        return INVALID
    if not 1 <= B <= MAX_BINS:
        return INVALID
    if B * W > MAX_BASIS:
        return INVALID
    if not 1 <= H <= MAX_HOP:
        return INVALID
    h = hops(n, W, H)
    if h > 0 and not has_out:
        return INVALID
    if cap is not None and cap < h * B:
        return INVALID
    if h > MAX_HOPS:
        return UNSUPPORTED
    if h * B > MAX_CELLS:
        return UNSUPPORTED
    return 0


def launch_hops(W, B, launch_terms):
    """wbx_spectrum_launch_hops: whole thirty-twos within launch_terms // (2 W B) and STAGE_CELLS // B"""
    if not shape_ok(W, B, 1):
        return 0
    return min(launch_terms // (2 * W * B), STAGE_CELLS // B, MAX_HOPS) & ~31


def launches(n_hops, W, B, launch_terms):
    per = launch_hops(W, B, launch_terms)
    return -(-n_hops // per) if per else 0


# ---- the basis ------------------------------------------------------------------------------------------------------------------
def window(L, kind, beta=0.0):
    """w[j], j = 0 .. L - 1, before the normalisation"""
    j = np.arange(L, dtype=F64)
    Ld = F64(L)
    if kind == RECT:
        return np.ones(L, dtype=F64)
    if kind == HANN:
        s = RS.sinpi((j + F64(0.5)) / Ld)
        return s * s
    assert kind == KAISER
    u = ((F64(2.0) * j + F64(1.0)) - Ld) / Ld                   # (2 j + 1 is exact either way)
    q = F64(1.0) - u * u
    q = np.where(q < 0.0, F64(0.0), q)
    return RS.i0(F64(beta) * np.sqrt(q)) / RS.i0(F64(beta))


def ascending_sum(v):
    acc = F64(0.0)
    for x in v:
        acc = acc + x
    return acc


def basis(W, B, freqs, lengths=None, kind=HANN, beta=0.0):
    """wbx_spectrum_basis: float32[2 B W], i-major; None where the header refuses"""
    freqs = np.asarray(freqs, dtype=F64)
    if not shape_ok(W, B, 1) or len(freqs) != B or kind not in (RECT, HANN, KAISER):
        return None
    if kind == KAISER and not (0.0 <= beta <= MAX_BETA):
        return None
    if not np.all((freqs >= 0.0) & (freqs <= 0.5)):
        return None
    if lengths is not None and not all(4 <= int(L) <= W for L in lengths):
        return None
    out = np.zeros((W, B, 2), dtype=F32)
    cache = {}
    for b in range(B):
        L = W if lengths is None else int(lengths[b])
        if L not in cache:
            w = window(L, kind, beta)
            cache[L] = w / ascending_sum(w)
        wn = cache[L]
        off = (W - L) // 2
        t = freqs[b] * np.arange(L, dtype=F64)
        t = t - np.floor(t)
        t2 = F64(2.0) * t
        out[off:off + L, b, 0] = (wn * RS.sinpi(t2 + F64(0.5))).astype(F32)
        out[off:off + L, b, 1] = (F64(0.0) - (wn * RS.sinpi(t2))).astype(F32)
    return out.reshape(-1)


def log_freqs(f_min, bins_per_octave, n_bins):
    """wbx_spectrum_log_freqs: (frequencies, how many were clamped at 0.5)"""
    y = np.arange(n_bins, dtype=F64) / F64(bins_per_octave)
    with np.errstate(divide="ignore"):
        f = F64(f_min) / DM.exp2(F64(0.0) - y)
    over = ~(f <= 0.5)
    return np.where(over, F64(0.5), f), int(over.sum())


def constant_q_lengths(freqs, W, cycles):
    """Engine.spectrogram_sample's constant_q: a window of `cycles` periods per bin, a multiple of 4 in 4 .. W"""
    out = []
    for f in np.asarray(freqs, dtype=np.float64):
        L = W if f <= 0.0 else int(round(cycles / f))
        out.append(max(4, min(W, L - L % 4)))
    return np.array(out, dtype=np.uint32)


# ---- the cells ------------------------------------------------------------------------------------------------------------------
def detector(planes, channel):
    """d as fp64 values that are fp32 values: a channel with what is not finite as 0.0, or f0's mid"""
    x = ST.inputs(planes)
    if channel == MID:
        return ST.detector(x)
    return x[channel]


def power(d, basis_words, W, B, H, only=None, chunk=256):
    """float32[hops][B] of detector values d — or, with `only` (hop indices), of those hops in that order"""
    total = hops(len(d), W, H)
    which = np.arange(total, dtype=np.int64) if only is None else np.asarray([int(h) for h in only], dtype=np.int64)
    assert np.all((which >= 0) & (which < total))
    tab = np.asarray(basis_words, dtype=F32).astype(F64).reshape(W, B, 2)
    C, S = np.ascontiguousarray(tab[:, :, 0]), np.ascontiguousarray(tab[:, :, 1])
    out = np.zeros((len(which), B), dtype=F32)
    d = np.asarray(d, dtype=F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for at in range(0, len(which), chunk):
            ts = which[at:at + chunk] * H
            re = np.zeros((len(ts), B), dtype=F64)
            im = np.zeros_like(re)
            for i in range(W):
                x = d[ts + i][:, None]
                re = re + x * C[i][None, :]
                im = im + x * S[i][None, :]
            out[at:at + chunk] = ((re * re) + (im * im)).astype(F32)
    return out


def spectrum_clip(planes, first, n, channel, basis_words, W, B, H, only=None):
    """wbx_clip_spectrum of frames [first, first + n) of a clip given as its channel planes: (cells, info without launches)"""
    d = detector([np.asarray(p)[first:first + n] for p in planes], channel)
    return power(d, basis_words, W, B, H, only), {"hops": hops(n, W, H), "bins": B}


def chroma_fold(cells, octaves):
    """Engine.chroma_sample's fold: cells [hops][12 * octaves] of a semitone basis into [hops][12], in fp64, the octaves
    added in ascending order from 0.0"""
    cells = np.asarray(cells, dtype=F32).astype(F64)
    out = np.zeros((cells.shape[0], 12), dtype=F64)
    for o in range(octaves):
        out = out + cells[:, 12 * o:12 * o + 12]
    return out
