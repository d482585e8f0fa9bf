"""Host model of wbx_clip_pitch and wbx_pitch_mid_frames (include/wbx.h "Pitch-shifting a clip"): by definition the
composition of two existing models — tests/stretch_model.py to the intermediate length m', then tests/resample_model.py of
that intermediate by M / L, of which the first m frames are kept — plus the argument check of wbx_pitch.h in Python integers.
Positions, info and every output sample of the library must reproduce every bit."""
import functools
import math

import numpy as np

import resample_model as RS
import stretch_model as ST

MAX_FRAMES, MAX_STEPS, MAX_OCTAVES = (1 << 31) - 16, 1 << 22, 4
INVALID, UNSUPPORTED = -4, -3
Refused = ST.Refused


def ratio(num, den):
    """(L, M) = (den / g, num / g), or None for a ratio the call refuses: a term of 0, a ratio of 1, beyond two octaves,
    L > 1280"""
    if num == 0 or den == 0:
        return None
    g = math.gcd(num, den)
    L, M = den // g, num // g
    if L == M or num > MAX_OCTAVES * den or den > MAX_OCTAVES * num or L > RS.MAX_L:
        return None
    return L, M


def mid_frames(m, num, den):
    """wbx_pitch_mid_frames: m' = ceil(m M / L) (what does not fit 64 bits: 2^64 - 1); 0 where the call would refuse the ratio"""
    r = ratio(num, den)
    if r is None:
        return 0
    L, M = r
    return min((m * M + L - 1) // L, (1 << 64) - 1)


def check_args(n, m, num, den, quality, N, D, positions_cap=None):
    """wbx_pitch.h's pitch_check_args: the status a call gets before its clip is looked at (0: none), in its order"""
    if n == 0 or m == 0 or num == 0 or den == 0:
        return INVALID
    g = math.gcd(num, den)
    if num // g == den // g or quality not in RS.QUALITY or m >= MAX_FRAMES:
        return INVALID
    if num > MAX_OCTAVES * den or den > MAX_OCTAVES * num:
        return UNSUPPORTED
    try:
        RS.plan(num, den, quality)
    except RS.Refused:
        return UNSUPPORTED
    mid = mid_frames(m, num, den)
    st = ST.check_args(n, mid, N, D, positions_cap)
    if st:
        return st
    return UNSUPPORTED if ST.steps(mid, N) > MAX_STEPS else 0


@functools.lru_cache(maxsize=64)
def table(L, M, quality):
    """the conversion's table (RS.table of the reduced ratio), made once per plan"""
    return RS.table(M, L, quality)


def pitch_clip(src, first, n, m, num, den, quality=RS.GOOD, N=2048, D=512):
    """src: a list of fp32 planes (1 or 2).  (the result's planes, the positions of the stretch, the info without its
    launches)"""
    st = check_args(n, m, num, den, quality, N, D)
    if st:
        raise Refused(st)
    L, M = ratio(num, den)
    mid = mid_frames(m, num, den)
    y, p, info = ST.stretch_clip(src, first, n, mid, N, D)
    out = RS.resample(y, 0, mid, num, den, quality, window=(0, m), tab=table(L, M, quality))
    return out, p, dict(info, mid_frames=mid, L=L, M=M)
