"""Host model of wbx_clip_filter (include/wbx.h "Filtering a clip"): the biquad designs, the test of a cascade, the carry
matrix and the chunked run in numpy, the header's formulas operation for operation — what tests/resample_model.py is for the
conversion.  Every fp64 step is one IEEE operation (+ - * / sqrt, no libm, nothing fused), so the library's coefficients
and matrix and the device's output must reproduce every bit.  The run is vectorised ACROSS chunks: the device's "a lane owns
a chunk" is one elementwise numpy operation per step over all chunks, which changes no bit.  A NaN result is the quiet NaN
0x7FC00000."""
import numpy as np

from resample_model import sinpi

F32, F64 = np.float32, np.float64
CHUNK, MAX_STAGES, MAX_FRAMES = 512, 8, (1 << 31) - 16
LOWPASS, HIGHPASS, BANDPASS, NOTCH, ALLPASS, PEAK, LOWSHELF, HIGHSHELF = range(8)
KINDS = {"lowpass": LOWPASS, "highpass": HIGHPASS, "bandpass": BANDPASS, "notch": NOTCH, "allpass": ALLPASS, "peak": PEAK,
         "lowshelf": LOWSHELF, "highshelf": HIGHSHELF}
CANON_NAN = np.uint32(0x7FC00000)
INVALID, UNSUPPORTED = -4, -3


class Refused(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(status)


def _design(T, sinpi_of, sqrt, rate, kind, f, q, gain):
    """the header's formulas over the number type T with sin(pi x) and sqrt supplied: fp64 + the series for the model,
    longdouble + libm for the comparison"""
    r, f, q, gain = T(rate), T(f), T(q), T(gain)
    t, h = (T(2.0) * f) / r, f / r
    sn, cs = sinpi_of(t), sinpi_of(t + T(0.5))
    sh, ch = sinpi_of(h), sinpi_of(h + T(0.5))
    hm, hp = sh * sh, ch * ch
    omc, opc = T(2.0) * hm, T(2.0) * hp
    alpha = sn / (T(2.0) * q)
    m2cs = T(0.0) - T(2.0) * cs
    one = T(1.0)
    if kind == LOWPASS:
        a0, b, a1, a2 = one + alpha, (hm, omc, hm), m2cs, one - alpha
    elif kind == HIGHPASS:
        a0, b, a1, a2 = one + alpha, (hp, T(0.0) - opc, hp), m2cs, one - alpha
    elif kind == BANDPASS:
        a0, b, a1, a2 = one + alpha, (alpha, T(0.0), T(0.0) - alpha), m2cs, one - alpha
    elif kind == NOTCH:
        a0, b, a1, a2 = one + alpha, (one, m2cs, one), m2cs, one - alpha
    elif kind == ALLPASS:
        a0, b, a1, a2 = one + alpha, (one - alpha, m2cs, one + alpha), m2cs, one - alpha
    elif kind == PEAK:
        A = sqrt(gain)
        aA, aoA = alpha * A, alpha / A
        a0, b, a1, a2 = one + aoA, (one + aA, m2cs, one - aA), m2cs, one - aoA
    else:
        A = sqrt(gain)
        beta = (T(2.0) * sqrt(A)) * alpha
        P, Q = A * omc + opc, A * opc + omc
        if kind == LOWSHELF:
            a0 = Q + beta
            b = (A * (P + beta), (T(2.0) * A) * (A * omc - opc), A * (P - beta))
            a1, a2 = T(0.0) - T(2.0) * (A * opc - omc), Q - beta
        else:
            a0 = P + beta
            b = (A * (Q + beta), T(0.0) - (T(2.0) * A) * (A * opc - omc), A * (Q - beta))
            a1, a2 = T(2.0) * (A * omc - opc), P - beta
    return np.array([b[0] / a0, b[1] / a0, b[2] / a0, a1 / a0, a2 / a0], dtype=T)


def design(rate, kind, f, q=0.7071067811865476, gain=1.0):
    """wbx_filter_design: b0 b1 b2 a1 a2 in fp64; `gain` LINEAR.  Refused(INVALID) as the library refuses"""
    kind = KINDS.get(kind, kind)
    f, q, gain = float(f), float(q), float(gain)
    if kind not in range(8) or rate == 0 or not (0.0 < f < rate / 2.0) or not (np.isfinite(q) and q > 0.0) \
            or not (np.isfinite(gain) and gain > 0.0):
        raise Refused(INVALID)
    return _design(F64, lambda x: F64(sinpi(x)), np.sqrt, rate, kind, f, q, gain)


def design_longdouble(rate, kind, f, q=0.7071067811865476, gain=1.0):
    """the same formulas in numpy.longdouble with libm's sin"""
    LD = np.longdouble
    pi = LD(4.0) * np.arctan(LD(1.0))
    return _design(LD, lambda x: np.sin(pi * x), np.sqrt, rate, KINDS.get(kind, kind), f, q, gain)


def cascade(coef):
    return np.ascontiguousarray(coef, dtype=F64).reshape(-1, 5)


def check(coef):
    """wbx_filter_check: True when the library answers WBX_OK"""
    k = np.asarray(coef, dtype=F64)
    if k.size == 0 or k.size % 5:
        return False
    k = k.reshape(-1, 5)
    if not 1 <= len(k) <= MAX_STAGES or not np.all(np.isfinite(k)):
        return False
    return bool(np.all(np.abs(k[:, 4]) < 1.0) and np.all(np.abs(k[:, 3]) < 1.0 + k[:, 4]))


def four_stages(rate):
    """the cascade of the accuracy figures: a 20 Hz high-pass (poles next to z = 1: the carry matters), two narrow peaks, a low-pass"""
    return np.stack([design(rate, "highpass", 20.0), design(rate, "peak", 1000.0, 8.0, 4.0),
                     design(rate, "peak", 60.0, 30.0, 0.1), design(rate, "lowpass", 0.4 * rate)])


def eight_stages(rate):
    """... and four more: one stage of every remaining kind but the band-pass"""
    return np.concatenate([four_stages(rate), np.stack([design(rate, "lowshelf", 120.0, 0.8, 2.0), design(rate, "notch", 50.0, 12.0),
                                                        design(rate, "highshelf", 0.2 * rate, 0.7, 0.5),
                                                        design(rate, "allpass", 300.0, 2.0)])])


def step(k, v, x):
    """one frame through the cascade, for every lane at once: k [S][5], v a list of D arrays (updated in place), x an array"""
    S = len(k)
    inp = x
    for s in range(S):
        x1, x2, y1, y2 = v[2 * s], v[2 * s + 1], v[2 * s + 2], v[2 * s + 3]
        y = k[s][0] * inp + k[s][1] * x1
        y = y + k[s][2] * x2
        y = y - k[s][3] * y1
        y = y - k[s][4] * y2
        v[2 * s], v[2 * s + 1] = inp, x1
        inp = y
    v[2 * S + 1] = v[2 * S]
    v[2 * S] = inp
    return inp


def run(coef, X, v0=None, want_output=True):
    """rows of X ([lanes][frames], fp64) through the cascade from states v0 ([lanes][D], default rest); returns
    (Y [lanes][frames] fp64 or None, the final states [lanes][D])"""
    k = [[F64(c) for c in row] for row in cascade(coef)]
    D = 2 * len(k) + 2
    lanes, n = X.shape
    v = [np.zeros(lanes, dtype=F64) if v0 is None else v0[:, i].copy() for i in range(D)]
    Y = np.empty((lanes, n), dtype=F64) if want_output else None
    with np.errstate(all="ignore"):
        for t in range(n):
            y = step(k, v, X[:, t])
            if want_output:
                Y[:, t] = y
    return Y, np.stack(v, axis=1)


def transition(coef):
    """wbx_filter_transition: M[i][k], column k the state after CHUNK frames of zero input from e_k (lane k starts at e_k)"""
    D = 2 * len(cascade(coef)) + 2
    _, v = run(coef, np.zeros((D, CHUNK), dtype=F64), np.eye(D, dtype=F64), want_output=False)
    return np.ascontiguousarray(v.T)


def entering(plane, first, n, tail):
    """x[i], i in [0, n + tail): (double) of the range's samples, one that is not finite entering as 0.0; zero in the tail"""
    x = np.zeros(n + tail, dtype=F64)
    r = np.asarray(plane[first:first + n], dtype=F32).astype(F64)
    x[:n] = np.where(np.isfinite(r), r, F64(0.0))
    return x


def to_f32(y):
    with np.errstate(all="ignore"):
        out = y.astype(F32)
    out.view(np.uint32)[np.isnan(out)] = CANON_NAN
    return out


def carried_states(coef, X):
    """t_j for every chunk row of X ([chunks][CHUNK]): t_0 = 0, t_{j+1} = z_j + M t_j, the sum in ascending k from 0.0"""
    k = cascade(coef)
    D = 2 * len(k) + 2
    J = X.shape[0]
    t = np.zeros((J, D), dtype=F64)
    if J > 1:
        _, z = run(coef, X[:-1], want_output=False)
        M = transition(coef)
        with np.errstate(all="ignore"):
            for j in range(J - 1):
                acc = np.zeros(D, dtype=F64)
                for q in range(D):
                    acc = acc + M[:, q] * t[j, q]
                t[j + 1] = z[j] + acc
    return t


def filter_plane(plane, first, n, tail, coef, states=False):
    """one channel of wbx_clip_filter: fp32 [n + tail] (and with `states` the t_j, [chunks][D])"""
    x = entering(plane, first, n, tail)
    total = n + tail
    J = -(-total // CHUNK)
    X = np.zeros(J * CHUNK, dtype=F64)
    X[:total] = x
    X = X.reshape(J, CHUNK)
    t = carried_states(coef, X)
    Y, _ = run(coef, X, t)
    out = to_f32(Y.reshape(-1)[:total])
    return (out, t) if states else out


def filter_clip(planes, first, n, tail, coef):
    assert n > 0 and n + tail < MAX_FRAMES and check(coef)
    return [filter_plane(p, first, n, tail, coef) for p in planes]


def sequential(x, coef, T=float):
    """the one sequential pass over x (fp64 array) in the number type T (float: IEEE fp64; numpy.longdouble: the wider
    reference), direct form I stage by stage; returns an array of T"""
    k = [[T(c) for c in row] for row in cascade(coef)]
    y = [T(a) for a in np.asarray(x, dtype=F64)]
    zero = T(0.0)
    for b0, b1, b2, a1, a2 in k:
        x1 = x2 = y1 = y2 = zero
        out = []
        for xv in y:
            yv = b0 * xv + b1 * x1
            yv = yv + b2 * x2
            yv = yv - a1 * y1
            yv = yv - a2 * y2
            x2, x1, y2, y1 = x1, xv, y1, yv
            out.append(yv)
        y = out
    return np.array(y, dtype=np.longdouble if T is not float else F64)


def response(coef, w):
    """|H(e^{jw})| of a cascade in fp64 (complex128), w in radians per frame"""
    z1 = np.exp(-1j * np.asarray(w, dtype=F64))
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in cascade(coef):
        h = h * ((b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1))
    return np.abs(h)
