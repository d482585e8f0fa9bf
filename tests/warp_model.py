"""Host model of wbx_clip_warp and wbx_warp_check / _steps / _segments / _launches (include/wbx.h "Warping a clip") in numpy,
on top of stretch_model: its inputs, detector, window and scoring are used as they are.  What is new here: the plan (segments
and steps), the positions with their pinned steps, the overlap-add with short last steps, the check and the launch count.
Positions, info and every output sample of the library must reproduce every bit."""
import numpy as np

import stretch_model as SM

F32, F64 = SM.F32, SM.F64
INVALID, UNSUPPORTED = SM.INVALID, SM.UNSUPPORTED
MAX_MARKERS, MAX_STEPS = 65535, 1 << 22
LAUNCH_TERMS, STEP_TERMS, BAND_STEPS = 1 << 30, 1 << 16, 1 << 16   # wbx_stretch.h's bound of one workgroup's launch


def markers_ok(n, m, markers):
    if len(markers) > MAX_MARKERS:
        return False
    s, t = 0, 0
    for a, b in markers:
        if a <= s or b <= t or a >= n or b >= m:
            return False
        s, t = a, b
    return True


def segments(n, m, markers, N):
    """wbx_warp_segments: [(s_j, t_j, base_j, K_j)] for the S = M + 1 segments; (n_j, m_j) follow from the next one"""
    Hs = N // 2
    edges = [(0, 0)] + [(int(a), int(b)) for a, b in markers] + [(n, m)]
    out, base = [], 0
    for j in range(len(edges) - 1):
        Kj = -(-(edges[j + 1][1] - edges[j][1]) // Hs)
        out.append((edges[j][0], edges[j][1], base, Kj))
        base += Kj
    return out


def steps(n, m, markers, N):
    """wbx_warp_steps: K; 0 for a window or markers the call refuses"""
    if not SM.window_ok(N) or n == 0 or m == 0 or not markers_ok(n, m, markers):
        return 0
    return sum(g[3] for g in segments(n, m, markers, N))


def check(n, m, markers, N, D, positions_cap=None):
    """wbx_warp_check: the status a call gets before its clip is looked at (0: none)"""
    if n == 0 or m == 0 or n >= SM.MAX_FRAMES or m >= SM.MAX_FRAMES:
        return INVALID
    if not SM.window_ok(N) or not 0 <= D <= SM.MAX_TOLERANCE:
        return INVALID
    if not markers_ok(n, m, markers):
        return INVALID
    K = steps(n, m, markers, N)
    if positions_cap is not None and positions_cap < K:
        return INVALID
    edges = [(0, 0)] + [(int(a), int(b)) for a, b in markers] + [(n, m)]
    for (s0, t0), (s1, t1) in zip(edges[:-1], edges[1:]):
        if t1 - t0 > SM.MAX_RATIO * (s1 - s0) or s1 - s0 > SM.MAX_RATIO * (t1 - t0):
            return UNSUPPORTED
    if K > MAX_STEPS:
        return UNSUPPORTED
    return 0


def launch_steps(n, N, D):
    """wbx_stretch_launch_steps: the steps one workgroup walks per launch"""
    per_step = min(2 * D + 1, n) * (N // 2) + STEP_TERMS
    return min(max(LAUNCH_TERMS // per_step, 1), BAND_STEPS)


def rounds(n, m, markers, N, D):
    """the live segments of every round: round r holds the segments with K_j > r * S_r"""
    Sr = launch_steps(n, N, D)
    Ks = [g[3] for g in segments(n, m, markers, N)]
    out, r = [], 0
    while True:
        live = sum(1 for k in Ks if k > r * Sr)
        if not live:
            return out
        out.append(live)
        r += 1


def launches(n, m, markers, N, D, launch_segments):
    """wbx_warp_launches: every round in slices of at most launch_segments workgroups, and one overlap-add"""
    if check(n, m, markers, N, D):
        return 0
    return sum(-(-live // launch_segments) for live in rounds(n, m, markers, N, D)) + 1


def positions(d, m, markers, N, D):
    """(p, info): the K positions as int32 and the info without its launches"""
    n, Hs = len(d), N // 2
    segs = segments(n, m, markers, N)
    edges = segs + [(n, m, 0, 0)]
    K = sum(g[3] for g in segs)
    dz = np.concatenate([d, np.zeros(2 * Hs + 2 * SM.MAX_TOLERANCE + 1, dtype=F64)])   # zero outside [0, n)
    p = np.zeros(K, dtype=np.int32)
    searched, scored, max_shift = 0, 0, 0
    for j, (s_j, t_j, base, Kj) in enumerate(segs):
        n_j, m_j = edges[j + 1][0] - s_j, edges[j + 1][1] - t_j
        prev = s_j                                              # i = 0: pinned, never scored (a_k = s_j)
        p[base] = prev
        for i in range(1, Kj):
            a = s_j + (i * Hs * n_j) // m_j
            c = prev + Hs                                       # (only a segment's last step is short: l_{k-1} = Hs)
            lo, hi = max(a - D, 0), min(a + D, n - 1)
            if lo <= c <= hi:
                prev = c
            else:
                cand = hi - lo + 1
                t = dz[c:c + Hs]
                s, E = np.zeros(cand, dtype=F64), np.zeros(cand, dtype=F64)
                for q in range(Hs):                             # ascending terms, the candidates side by side
                    w = dz[lo + q:lo + q + cand]
                    s = s + t[q] * w
                    E = E + w * w
                with np.errstate(divide="ignore", invalid="ignore"):
                    score = np.where(E == 0.0, F64(0.0), (s * np.abs(s)) / np.where(E == 0.0, F64(1.0), E))
                prev = lo + int(np.argmax(score))               # (numpy: the first of equal maxima)
                searched += 1
                scored += cand
            p[base + i] = prev
            max_shift = max(max_shift, abs(prev - a))
    return p, {"steps": K, "searched_steps": searched, "candidates": scored, "max_shift": max_shift, "segments": len(segs),
               "longest_segment_steps": max(g[3] for g in segs)}


def overlap_add(x, p, m, markers, N):
    """the result's fp32 planes from the positions"""
    n, Hs = len(x[0]), N // 2
    up, dn = SM.window(N)
    segs = segments(n, m, markers, N)
    ends = [g[1] for g in segs[1:]] + [m]
    out = []
    for xc in x:
        xz = np.concatenate([xc, np.zeros(2 * Hs, dtype=F64)])
        y = np.zeros(m, dtype=F32)
        prev, prev_l = -Hs, Hs
        for (s_j, t_j, base, Kj), t_end in zip(segs, ends):
            for i in range(Kj):
                o = t_j + i * Hs
                l = min(Hs, t_end - o)
                pk, c = int(p[base + i]), prev + prev_l
                a = xz[pk:pk + l]
                y[o:o + l] = a.astype(F32) if pk == c else ((up[:l] * a) + (dn[:l] * xz[c:c + l])).astype(F32)
                prev, prev_l = pk, l
        out.append(y)
    return out


def warp_clip(src, first, n, m, markers, N=2048, D=512):
    """src: a list of fp32 planes (1 or 2).  (the result's planes, the positions, the info without its launches)"""
    x = SM.inputs([q[first:first + n] for q in src])
    p, info = positions(SM.detector(x), m, markers, N, D)
    return overlap_add(x, p, m, markers, N), p, info
