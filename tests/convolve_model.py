"""Host model of wbx_clip_convolve and wbx_fir_design (include/wbx.h "Convolving a clip") in numpy, the header's formulas
operation for operation — what tests/filter_model.py is for the biquads.  Every fp64 step is one IEEE operation, the sums
run in ascending tap order (one vector `acc = acc + h[k] * x` per tap; numpy.cumsum for the design's normalisation, which
adds sequentially), so the library's taps and the device's output must reproduce every bit.  The design's sinpi, sinc and I0
are tests/resample_model.py's."""
import numpy as np

import resample_model as RM

F32, F64 = np.float32, np.float64
LOWPASS, HIGHPASS, BANDPASS, BANDSTOP = range(4)
KINDS = {"lowpass": LOWPASS, "highpass": HIGHPASS, "bandpass": BANDPASS, "bandstop": BANDSTOP}
TILE, SEGMENT = 2048, 2048
MAX_TAPS, MAX_WORK, MAX_FRAMES = 1 << 20, 1 << 46, (1 << 31) - 16
FIR_MIN_TAPS, FIR_MAX_TAPS = 3, 65535
CANON_NAN = np.uint32(0x7FC00000)
INVALID, UNSUPPORTED = -4, -3


class Refused(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(status)


def full_frames(n_frames, ir_frames):
    """wbx_convolve_frames"""
    if n_frames == 0 or ir_frames == 0 or ir_frames > MAX_TAPS or n_frames + ir_frames - 1 >= 1 << 64:
        return 0
    return n_frames + ir_frames - 1


def entering(plane):
    """(double) of the fp32 samples, what is not finite as 0.0"""
    v = np.asarray(plane, dtype=F32).astype(F64)
    return np.where(np.isfinite(v), v, F64(0.0))


def convolve_plane(x, h, out_first, out_frames, gain):
    """x, h: the two RANGES (fp32).  fp32 frames [out_first, out_first + out_frames) of the full result"""
    x, h = entering(x), entering(h)
    n, L = len(x), len(h)
    assert 0 < out_frames and out_first + out_frames <= n + L - 1
    # xp[L - 1 + i] = x[i], zero outside: frame m, tap k reads xp[L - 1 + m - k]
    xp = np.zeros(n + 2 * (L - 1), dtype=F64)
    xp[L - 1:L - 1 + n] = x
    acc = np.zeros(out_frames, dtype=F64)
    base = L - 1 + out_first
    for k in range(L):
        acc = acc + h[k] * xp[base - k:base - k + out_frames]
    with np.errstate(over="ignore", invalid="ignore"):
        y = (F64(gain) * acc).astype(F32)
    bits = y.view(np.uint32).copy()
    bits[np.isnan(y)] = CANON_NAN
    return bits.view(F32)


def convolve_clip(src, first, n, ir, ir_first, L, out_first=0, out_frames=None, gain=1.0):
    """src, ir: lists of fp32 planes (1 or 2 each).  The result's planes, max(len(src), len(ir)) of them"""
    if out_frames is None:
        out_frames = n + L - 1 - out_first
    ch = max(len(src), len(ir))
    return [convolve_plane(src[c % len(src)][first:first + n], ir[c % len(ir)][ir_first:ir_first + L], out_first, out_frames, gain)
            for c in range(ch)]


def _lp(t, d, c, beta, i0b):
    u = d / F64(c)
    a = F64(1.0) - u * u
    a = np.where(a < 0.0, F64(0.0), a)
    w = RM.i0(beta * np.sqrt(a)) / i0b
    v = (t * RM.sinc(t * d)) * w
    return v / np.cumsum(v)[-1]


def fir_design(rate, kind, f1, f2=0.0, n_taps=255, beta=8.6):
    """wbx_fir_design: fp32 taps; Refused(INVALID) as the library refuses"""
    kind = KINDS.get(kind, kind)
    band = kind in (BANDPASS, BANDSTOP)
    f1, f2, beta = F64(f1), F64(f2), F64(beta)
    r = F64(rate)
    if rate == 0 or kind not in (LOWPASS, HIGHPASS, BANDPASS, BANDSTOP) or not FIR_MIN_TAPS <= n_taps <= FIR_MAX_TAPS or n_taps % 2 == 0:
        raise Refused(INVALID)
    if not (f1 > 0.0 and f1 < r / F64(2.0)) or (band and not (f2 > 0.0 and f2 < r / F64(2.0) and f2 > f1)):
        raise Refused(INVALID)
    if not (np.isfinite(beta) and 0.0 <= beta <= 14.0):
        raise Refused(INVALID)
    c = (n_taps - 1) // 2
    d = (np.arange(n_taps, dtype=np.int64) - c).astype(F64)
    i0b = RM.i0(beta)
    delta = (d == 0.0).astype(F64)
    lp1 = _lp((F64(2.0) * f1) / r, d, c, beta, i0b)
    if kind == LOWPASS:
        v = lp1
    elif kind == HIGHPASS:
        v = delta - lp1
    else:
        lp2 = _lp((F64(2.0) * f2) / r, d, c, beta, i0b)
        v = lp2 - lp1 if kind == BANDPASS else delta - (lp2 - lp1)
    return v.astype(F32)
