"""wbx_clip_stretch and wbx_engine_stretch_sample on the device.  Results come back through wbx_clip_download and are compared
BIT FOR BIT (uint32 views: -0.0 shows) with tests/stretch_model.py, the numpy twin of the header's text; the positions and
the info are compared exactly.  Sizes are the smallest at which the kernels can still go wrong: windows of 32, 64 and 256
frames (a lane's 8 candidates, one wave, several waves of candidates), tolerances around Hs, results that end inside a step
and inside a 16-byte word, ranges shorter than a window — and one call each across a search launch's bound, across a band
of positions, and with the widest span the search stages (N = 8192, D = 4096: three passes of 4096 candidates)."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import dynamics_model as DM
import limit_model as LM
import oracle_ffi as O
import stretch_model as M
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 2100 + 300
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
DST = 100
bits = BU.bits


def source(channels, n=SRC_LEN, seed=0x57E, period=41.7):
    """seeded noise + a sine per channel (the channels at different periods)"""
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n)
    return [(0.25 * rng.standard_normal(n) + np.sin(2 * np.pi * i / (period + 9 * c))).astype(np.float32) for c in range(channels)]


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
    yield c
    c.close()


def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def first_bad(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        if bad.size:
            return k, int(bad[0]), int(bad.size), g[bad[0]], w[bad[0]]
    return None


def check_stats(got, want, n, where):
    """wbx_clip_measure's rules: every field but sum / sum_sq exact, those two within any-order fp64 summation's bound"""
    assert FX.exact_fields_equal(got, want), (where, got, {k: want[k] for k in FX.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if np.isfinite(a):
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


def launches_of(n, m, N, D):
    """the kernel launches the header promises: per band of positions its search launches and one overlap-add"""
    L = W.lib()
    B, per, K = L.wbx_stretch_band_steps(), L.wbx_stretch_launch_steps(n, N, D), M.steps(m, N)
    return sum(-(-min(B, K - b) // per) + 1 for b in range(0, K, B))


def run_and_check(c, clip, planes, first, n, m, N, D, dst=DST, stats=True):
    """one call against the model: every position, the info, every output bit and stats_of_result.  Returns (the result's
    planes, the positions, the info)"""
    ch = len(planes)
    want, want_p, want_info = M.stretch_clip(planes, first, n, m, N, D)
    got = c.clip_stretch(clip, dst, first, n, m, N, D, positions=True, stats_channels=ch if stats else 0)
    info, pos = got[0], got[1]
    where = (ch, first, n, m, N, D)
    bad = np.flatnonzero(pos != want_p)
    assert bad.size == 0, (where, "step", int(bad[0]), int(pos[bad[0]]), int(want_p[bad[0]]), bad.size)
    assert info == dict(want_info, launches=launches_of(n, m, N, D)), (where, info, want_info)
    out = download(c, dst, ch, m)
    assert first_bad(out, want) is None, (where, first_bad(out, want))
    if stats:
        check_stats(got[2], FX.measure(want), m, where)
    return out, pos, info


# ---- 1: windows x tolerances x ratios, mono and stereo -----------------------------------------------------------------------------
def lengths(n):
    return [-(-n // 8), n // 4, 2 * n // 3, n, 3 * n // 2, 2 * n, 8 * n, n - 1, n + 1]   # (an eighth rounded up: 8 m >= n)


@pytest.mark.parametrize("D", [0, 1, 24, 40, 4096])
@pytest.mark.parametrize("N", [32, 64, 256])
@pytest.mark.parametrize("channels", [1, 2])
def test_stretch_matrix(ctx, channels, N, D):
    """every ratio of the list at one window and tolerance (D = 40 exceeds Hs at N = 32; D = 4096 runs on 700 frames, so both
    ends clamp the span); the range starts inside the clip and, at the ratios' odd places, ends on its last frame"""
    n = 700 if D == 4096 else 2100
    searched = 0
    for i, m in enumerate(lengths(n)):
        first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
        _, _, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, m, N, D)
        searched += info["searched_steps"]
        if m == n:
            assert info["searched_steps"] == 0
    assert searched > 0


def test_short_ranges_short_results_and_ragged_ends(ctx):
    """n < N, n = 1, m < Hs (one ragged tile), m that ends inside a step and inside a 16-byte word, m = 1"""
    for ch in (1, 2):
        for n, m, N, D in ((10, 40, 32, 8), (31, 17, 64, 24), (1, 1, 32, 0), (1, 8, 32, 4), (1, 5, 256, 96), (100, 13, 32, 8), (100, 127, 256, 40),
                           (20, 3, 256, 0), (500, 777, 64, 24), (500, 130, 64, 1), (500, 1001, 40, 20), (333, 334, 48, 7), (8, 1, 32, 3),
                           (8, 1, 32, 0), (37, 255, 8192, 4096), (2100, 4097, 8192, 4096)):
            run_and_check(ctx, SRC[ch], ctx.src[ch], 7, n, m, N, D)


def test_a_template_past_the_end_of_the_range_takes_the_lowest_candidate(ctx):
    """a range that ends loud, stretched eightfold: the last continuations start behind the range's end, their template is
    all zeros, every score is 0 and the step takes lo"""
    for ch in (1, 2):
        n, N, D = 900, 256, 24
        planes = [p.copy() for p in ctx.src[ch]]
        for p in planes:
            p[5 + n - 200:5 + n] *= np.float32(3.0)
        ctx.clip_upload(50, "f32", RATE, planes)
        for m in (8 * n, 2 * n, 5 * n + 3):
            _, pos, _ = run_and_check(ctx, 50, planes, 5, n, m, N, D)
            c = np.concatenate([[0], pos[:-1] + N // 2])
            past = np.flatnonzero(c >= n)
            assert past.size, m
            for k in past:
                assert pos[k] == max(M.anchor(int(k), n, m, N) - D, 0)


# ---- 2: what the search hears ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_values_that_are_not_finite_and_frames_beside_the_range(ctx, channels):
    """NaN and +-inf inside the range enter as 0.0; loud samples and NaNs in front of and behind the range do not count: the
    result is that of the range alone"""
    planes = source(channels, 3000, seed=0xBE51DE)
    for c, p in enumerate(planes):
        p[:200], p[190:200], p[2700:], p[2710:2720] = 1e30, np.nan, -1e30, np.nan
        at = np.array([200, 205, 500, 1300, 1301, 2699]) - c * np.array([0, 1, 1, 1, 1, 1])
        p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    planes[0].view(np.uint32)[240] = 0xFFC12345                 # a NaN with a payload and a sign
    planes[0][250] = np.float32(-0.0)
    ctx.clip_upload(54, "f32", RATE, planes)
    for first, n in ((200, 2500), (200, 9), (2690, 10)):
        for m, N, D in ((n * 3 // 2, 64, 24), (n // 2 + 1, 32, 40), (n, 256, 96), (2 * n + 3, 256, 96)):
            alone = [p[first:first + n].copy() for p in planes]
            want, want_p, _ = M.stretch_clip(alone, 0, n, m, N, D)
            assert np.all(np.isfinite(np.stack(want)))
            got, pos, _ = run_and_check(ctx, 54, planes, first, n, m, N, D)
            assert first_bad(got, want) is None and np.array_equal(pos, want_p)
    got, _, _ = run_and_check(ctx, 54, planes, 200, 2500, 2500, 64, 24)       # a copy: what is not finite comes back as 0.0
    assert got[0][0] == 0.0 and np.signbit(got[0][50]) and got[0][50] == 0.0


def test_silence_and_opposite_channels_take_the_lowest_candidate(ctx):
    n = 2000
    loud = ctx.src[1][0][:n]
    for planes in ([np.zeros(n, dtype=np.float32)], [loud, -loud], [np.zeros(n, dtype=np.float32)] * 2):
        ctx.clip_upload(55, "f32", RATE, planes)
        for m, N, D in ((3000, 64, 24), (1300, 256, 96), (500, 64, 40)):
            _, pos, info = run_and_check(ctx, 55, planes, 0, n, m, N, D)
            prev, Hs = -(N // 2), N // 2
            for k, pk in enumerate(pos):
                a = M.anchor(k, n, m, N)
                lo, hi = max(a - D, 0), min(a + D, n - 1)
                assert pk == (prev + Hs if lo <= prev + Hs <= hi else lo)
                prev = int(pk)
            assert info["searched_steps"] > 0


def test_exact_ties_go_to_the_lowest_candidate(ctx):
    """a source of period 8: candidates 8 frames apart score EXACTLY the same (the same values in the same order), so away
    from the range's end the winner lies among the first 8 candidates of its span"""
    n = 3000
    pattern = np.array([0.5, 1.0, 0.25, -0.75, -1.0, -0.125, 0.375, 0.0], dtype=np.float32)
    planes = [np.tile(pattern, n // 8 + 1)[:n]]
    ctx.clip_upload(56, "f32", RATE, planes)
    for m, N, D in ((4500, 64, 24), (2000, 64, 24), (6001, 256, 96), (1100, 32, 40)):
        _, pos, info = run_and_check(ctx, 56, planes, 0, n, m, N, D)
        prev, Hs, seen = -(N // 2), N // 2, 0
        for k, pk in enumerate(pos):
            a = M.anchor(k, n, m, N)
            lo, hi = max(a - D, 0), min(a + D, n - 1)
            if not lo <= prev + Hs <= hi and hi + Hs <= n and prev + 2 * Hs <= n and hi - lo >= 16:
                assert pk - lo < 8 and (pk - (prev + Hs)) % 8 == 0, (k, pk, lo)
                seen += 1
            prev = int(pk)
        assert seen > 0


# ---- 3: the seams ----------------------------------------------------------------------------------------------------------------
def test_a_call_across_a_search_launch_and_across_a_band_of_positions():
    """N = 32 and D = 4096: a search launch takes launch_terms / (8193 * 16 + step_terms) steps, a band band_steps of them.  100 steps more
    than a band, stretched eightfold (few steps search: the model stays quick): several search launches per band, two
    bands; p, the counters and the positions cross both seams"""
    L = W.lib()
    B = L.wbx_stretch_band_steps()
    m = 16 * (B + 100) - 5
    n = m // 8 + 1
    per = L.wbx_stretch_launch_steps(n, 32, 4096)
    assert 1 <= per < B and per == L.wbx_stretch_launch_terms() // (8193 * 16 + L.wbx_stretch_step_terms())
    c = W.MixContext(4, block=128)
    planes = source(1, n, seed=0x5EA)
    c.clip_upload(1, "f32", RATE, planes)
    _, pos, info = run_and_check(c, 1, planes, 0, n, m, 32, 4096, dst=2, stats=False)
    assert info["launches"] > 1 and info["launches"] == -(-B // per) + 1 + 2 and info["searched_steps"] > 10
    searched = np.flatnonzero(np.diff(pos) != 16) + 1
    assert np.any(searched >= B) and np.any((searched > per) & (searched < B))
    c.close()


def test_a_band_seam_with_a_search_every_few_steps():
    """stereo, shortened to 2/3 with D = 24: nearly every other step searches, on both sides of the band's seam"""
    B = W.lib().wbx_stretch_band_steps()
    m = 16 * (B + 9) + 3
    n = m * 3 // 2
    c = W.MixContext(4, block=128)
    planes = source(2, n, seed=0x5EB)
    c.clip_upload(1, "f32", RATE, planes)
    _, pos, info = run_and_check(c, 1, planes, 0, n, m, 32, 24, dst=2, stats=False)
    assert info["launches"] == launches_of(n, m, 32, 24) > 4 and info["searched_steps"] > B // 8
    c.close()


def test_the_widest_span_in_lds(ctx):
    """N = 8192, D = 4096 on 20000 frames doubled: step 3 scores 8193 candidates over 4096 terms, three passes"""
    n, m = 20000, 40000
    planes = source(2, n, seed=0x1D5)
    ctx.clip_upload(57, "f32", RATE, planes)
    _, _, info = run_and_check(ctx, 57, planes, 0, n, m, 8192, 4096)
    assert info["candidates"] >= 8193 and info["searched_steps"] >= 1
    ctx.clip_upload(58, "f32", RATE, [planes[1]])
    run_and_check(ctx, 58, [planes[1]], 3, n - 3, 12000, 8192, 4095)


# ---- 4: around the call -----------------------------------------------------------------------------------------------------------
def test_time_of_the_last_stretch_call_and_other_edits_caches():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_stretch_ms(c.h, C.byref(out)) == -4 and out.value == 7.0     # none yet
    planes = source(1, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    assert c.L.wbx_stretch_ms(c.h, None) == -4
    c.clip_limit(1, 3, 0, 5000, 0.5)                            # a limit is no stretch call ...
    assert c.L.wbx_stretch_ms(c.h, C.byref(out)) == -4
    c.clip_stretch(1, 4, 0, 5000, 7500, 256, 96)
    assert 0.0 < c.stretch_ms() < 1000.0
    # a stretch between two limits and between two dynamics calls of one shape leaves their cached ramp and stage valid,
    # and a limit between two stretches of one window leaves the cached window table valid
    gate = DM.table(DM.GATE, -14.0, 3.0, 6.0, -30.0)
    lim_want, _ = LM.limit_clip(planes, 0, 5000, np.float32(0.5), 1.0, 8, 0, 48)
    dyn_want, _ = DM.dynamics_clip(planes, 0, 5000, gate, DM.GATE, A=8, H=0, R=48)
    str_want, _, _ = M.stretch_clip(planes, 0, 5000, 3333, 256, 96)
    c.clip_limit(1, 3, 0, 5000, 0.5, 1.0, 8, 0, 48)
    c.clip_stretch(1, 4, 0, 5000, 3333, 256, 96)
    c.clip_limit(1, 5, 0, 5000, 0.5, 1.0, 8, 0, 48)
    c.clip_dynamics(1, 6, 0, 5000, gate, "gate", lookahead_frames=8, hold_frames=0, release_frames=48)
    c.clip_stretch(1, 7, 0, 5000, 3333, 256, 96)
    c.clip_dynamics(1, 8, 0, 5000, gate, "gate", lookahead_frames=8, hold_frames=0, release_frames=48)
    for clip in (3, 5):
        assert first_bad(download(c, clip, 1, 5000), lim_want) is None
    for clip in (6, 8):
        assert first_bad(download(c, clip, 1, 5000), dyn_want) is None
    for clip in (4, 7):
        assert first_bad(download(c, clip, 1, 3333), str_want) is None
    c.close()


def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    c.clip_stretch(1, 10, 0, 3000, 4000, 64, 24)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        run_and_check(c, 1, planes, first, 3000, 4000, 64, 24, dst=10)
        assert c.pool_stats() == with_one
    run_and_check(c, 1, planes, 0, 3000, 700, 64, 24, dst=10)   # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_stretch(SRC[2], DST, 0, 64, 96, 32, 8)
    kept = bits(np.stack(download(ctx, DST, 2, 96))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    si, st = _ffi.StretchInfo(), _ffi.ClipStats()
    pos = np.full(64, 9, dtype=np.int32)
    S = SRC[2]

    def refused(status, why, src=S, dst=DST, first=0, n=64, m=96, N=32, D=8, cap=None):
        before = ctx.pool_stats()
        si.steps = 777
        got = L.wbx_clip_stretch(ctx.h, src, dst, first, n, m, N, D, None if cap is None else pos.ctypes.data, cap or 0, C.byref(si), C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 96))).tolist() == kept and si.steps == 777
        assert np.all(pos == 9)

    refused(-4, b"unknown source", src=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"no frames", m=0)
    refused(-4, b"past the clip", first=SRC_LEN - 10, n=11, m=11)
    refused(-4, b"past the clip", first=(1 << 64) - 1, n=2, m=2)     # a sum that wraps
    refused(-4, b"may not replace", dst=S)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16, m=(1 << 31) - 17)     # judged on the arithmetic: no clip is that long
    refused(-4, b"2^31 - 16", n=(1 << 30), m=(1 << 31) - 16)
    for N in (0, 24, 36, 8200, 8192 + 8):
        refused(-4, b"window_frames", N=N)
    refused(-4, b"tolerance_frames", D=4097)
    refused(-4, b"positions_cap", cap=5)                        # K = 6
    refused(-3, b"not F32", src=60)                             # (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, b"ratio", m=64 * 8 + 1)
    refused(-3, b"ratio", n=97 * 8, m=96)
    refused(-3, b"ratio", src=60, n=1 << 20, m=1 << 10)          # the sizes are judged before the clip is looked at
    refused(-4, b"window_frames", src=60, N=33)
    refused(-4, b"past the clip", n=1 << 20, m=1 << 20)          # ... the sizes pass, the clip does not
    # what is not refused: the limits themselves, a capacity that is just enough
    got = L.wbx_clip_stretch(ctx.h, S, 62, SRC_LEN - 1, 1, 8, 8192, 4096, pos.ctypes.data, 1, None, None)
    assert got == 0 and pos[0] == 0 and np.all(pos[1:] == 9)
    ctx.clip_stretch(S, 62, 0, 8 * 8, 8, 32, 0)
    assert L.wbx_clip_free(ctx.h, 62) == 0


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 19
    planes = source(2, n)
    c.clip_upload(1, "f32", RATE, planes)                       # 4 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_stretch(1, 10 + len(made), 0, n, 2 * n, 32, 0)   # 8 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    want, _, _ = M.stretch_clip([p[:4096] for p in planes], 0, 4096, 8192, 32, 0)
    got = [c.clip_download(made[-1], k, 2 * n, np.float32)[:8000] for k in range(2)]
    assert first_bad(got, [w[:8000] for w in want]) is None      # (D = 0: a step reads nothing beyond its anchor + N)
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 5: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_stretch_sample_and_stretch_to_tempo_played_and_exported():
    spec = synth.make_session("str2", 3, n_blocks=6, block=128, seed=0x57E2)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    NU = 3000
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)
    new, info = eng.stretch_sample(up, 4000, 256, 96, first_frame=4, n_frames=NU)
    want, _, want_info = M.stretch_clip(planes, 4, NU, 4000, 256, 96)
    assert eng._sample_shape[new] == (4000, 2) and {k: info[k] for k in want_info} == want_info and info["searched_steps"] > 0
    assert first_bad(download(eng.ctx, new, 2, 4000), want) is None
    # a loop recorded at 100 bpm fitted to 120: 5/6 of its length; 40 ms and 10 ms at the sample's rate, on the interface's grid
    t_id, t_info = eng.stretch_to_tempo(up, 100.0, 120.0)
    N, D, m = 8 * int(round(40.0 * rate / 8000.0)), int(round(10.0 * rate / 1000.0)), int(round((NU + 8) * 100.0 / 120.0))
    want_t, _, want_t_info = M.stretch_clip(planes, 0, NU + 8, m, N, D)
    assert eng._sample_shape[t_id] == (m, 2) and t_info["steps"] == want_t_info["steps"] == M.steps(m, N)
    assert first_bad(download(eng.ctx, t_id, 2, m), want_t) is None

    # the stretched sample on a track at speed 1.0, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "stretched", 0.5 * unit, 5.5 * unit, 0.0, new, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want, rate), 1.0, 1.0) == 0
    e.play()
    eng.play()
    eng.render(6)
    mm, _, _ = eng.ctx.fetch()
    heard = False
    for b in range(6):
        om, _ = e.process()
        assert np.array_equal(bits(mm[b]), bits(om)), b
        heard = heard or bool(om.any())
    assert heard
    got, _ = eng.export_sample(new, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want, axis=1).reshape(-1).view(np.uint32))
    with pytest.raises(W.WbxError):
        eng.delete_sample(new)                                  # a clip names it
    eng.delete_sample(t_id)
    # refusals create no sample
    L, new_id = W.lib(), C.c_uint32(12345)
    call = lambda s, n, m, N=64, D=24, ref=C.byref(new_id): L.wbx_engine_stretch_sample(eng.h, s, 0, n, m, N, D, None, ref)
    assert call(9999, 8, 8) == -4
    assert call(t_id, 8, 8) == -4                               # deleted
    assert call(up, NU + 9, NU) == -4
    assert call(up, 0, 8) == -4 and call(up, 8, 0) == -4
    assert call(up, 8, 8, N=36) == -4 and call(up, 8, 8, D=4097) == -4
    assert call(up, 8, 65) == -3 and call(up, 800, 99) == -3
    assert call(up, 8, 8, ref=None) == -4
    assert new_id.value == 12345
    assert call(up, NU + 8, NU) == 0 and new_id.value != 12345
    eng.close()
    e.close()


def test_cpp_adapter_stretches_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::stretch_sample; the result and the
    info equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_stretch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_stretch.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "stretched.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    m = n * 3 // 2
    assert "adapter stretch ok %d" % m in out, out
    g = np.arange(n, dtype=np.uint64)
    ph = g % 50
    tri = np.where(ph < 25, ph, 50 - ph).astype(np.float32) / np.float32(32.0) - np.float32(0.375)
    x = tri + (((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(4096.0)
    want, _, info = M.stretch_clip([x.astype(np.float32)], 0, n, m, 256, 96)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == m and first_bad([got], want) is None
    assert ("steps %d searched %d candidates %d max_shift %d" % (info["steps"], info["searched_steps"], info["candidates"],
                                                                info["max_shift"])) in out and info["searched_steps"] > 0, out


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_stretch_beside_the_audio_thread():
    """The shape of the dynamics test (test_gpu_dynamics.py): a clip far behind the played range names the big source while
    the threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one
    for the pin (-3, asked first) — one thread deletes without pause while the other stretches until a delete has been
    refused for the pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS = 300, 1 << 19, 60.0, 96
    N, D = 1024, 512
    spec = synth.make_session("strthr", 2, n_blocks=NB, block=128, seed=0x57E712)
    planes = source(2, FR, seed=41, period=233.3)

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 44100, planes)
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        return sid

    def run_blocks(eng, sink):
        out = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        for _ in range(NB):
            eng.process(None, out, float(spec.sample_rate))
            sink.append(np.stack(out.channel_buffers).copy())

    alone = []
    ref = build_engine(spec, max_blocks=1)
    with_big(ref)
    run_blocks(ref, alone)
    ref.close()

    eng = build_engine(spec, max_blocks=1)
    big = with_big(eng)
    first, n = 5, FR - 8
    m = n * 3 // 2
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), threading.Event()
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        while not finished.is_set() and time.monotonic() < end:
            st = L.wbx_engine_delete_sample(eng.h, big)
            key_ = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key_] = seen.get(key_, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"], results["info"] = eng.stretch_sample(big, m, N, D, first_frame=first, n_frames=n, channels=2, frames=FR)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (editor, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("stretch calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read a live clip: the result is the model's, bit for bit
    want, _, want_info = M.stretch_clip(planes, first, n, m, N, D)
    assert {k: results["info"][k] for k in want_info} == want_info and want_info["searched_steps"] > 100
    assert first_bad(download(eng.ctx, results["big"], 2, m), want) is None
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
