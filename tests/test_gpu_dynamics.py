"""wbx_clip_dynamics and wbx_engine_dynamics_sample on the device.  Results come back through wbx_clip_download and are
compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/dynamics_model.py, the numpy twin of the
header's text; the statistics are compared field by field, exactly.  Sizes are the limiter's (tests/test_gpu_limit.py):
the smallest at which the kernels can still go wrong, around their shape constants (T, the frames of a workgroup's tile; P,
the ramp terms of a segment; the band of 2^20 output frames) — a lane's 8 frames and the last lane's partial store
(1, 7, 8, 9), T-1, T, T+1, 2T+5; ramps of 1, 2, 7, P-1, P, P+1, 2P+3 terms split several ways between look-ahead, hold
and release — in both senses, with mono and stereo sources keyed by themselves, by a mono key and by a stereo key."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import dynamics_model as M
import limit_model as LM
import loudness_model as LOUD
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
T, P, BAND = M.TILE, M.SEGMENT, M.BAND
FRAMES = [1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 5]
TERMS = [1, 2, 7, P - 1, P, P + 1, 2 * P + 3]
SRC_LEN = 2 * T + 5 + 700
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
KEY = {1: 3, 2: 4}                                              # channels -> clip id of a key
DST = 100
NO_KEY = _ffi.DYN_NO_KEY
bits = BU.bits
COMP = M.table(M.COMPRESS, -12.0, 4.0, 6.0, -24.0)              # works above 0.18: the sources' tall samples and some of the rest
GATE = M.table(M.GATE, -14.0, 3.0, 6.0, -30.0)                  # closes under 0.28: most of a source, not its tall samples
TABLES = {M.COMPRESS: COMP, M.GATE: GATE}


def source(channels, n=SRC_LEN, seed=0xD1A, every=97):
    """noise of +-0.5 around a small offset, every `every`-th sample (the channels at different places) four times as
    large: in both senses some frames are at rest and some are not"""
    rng = np.random.default_rng(seed + channels)
    planes = [(rng.uniform(-0.5, 0.5, n) + 0.0625 * (1 - 2 * k)).astype(np.float32) for k in range(channels)]
    for k, p in enumerate(planes):
        p[11 * k + 3::every] *= np.float32(4.0)
    return planes


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    c.key = {ch: source(ch, SRC_LEN + 40, seed=0x4E1, every=131) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
        c.clip_upload(KEY[ch], "f32", RATE, c.key[ch])
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


def run_and_check(c, clip, planes, first, n, tab, sense, drive=1.0, makeup=1.0, A=72, H=0, R=4800, key_clip=None, key=None,
                  key_first=0, key_gain=1.0, dst=DST, where=None):
    """one call against the model: every output bit, wbx_dynamics_stats and stats_of_result.  Returns (the result's planes,
    the statistics)"""
    ch = len(planes)
    want, want_ds = M.dynamics_clip(planes, first, n, tab, sense, drive, makeup, A, H, R, key, key_first, key_gain)
    ds, st = c.clip_dynamics(clip, dst, first, n, tab, sense, key_clip, key_first, drive, key_gain, makeup, A, H, R, stats_channels=ch)
    got = download(c, dst, ch, n)
    where = where or (ch, first, n, sense, drive, makeup, A, H, R, key_clip, key_first, key_gain)
    assert first_bad(got, want) is None, (where, first_bad(got, want))
    assert ds == want_ds, (where, ds, want_ds)
    check_stats(st, FX.measure(want), n, where)
    return got, ds


# ---- 1: lengths x ramp lengths, both senses, mono and stereo, no key / mono key / stereo key ---------------------------------------
def split(K, i):
    """the i-th way to cut K terms into look-ahead, hold and release"""
    way = i % 4
    if way == 0:
        return 0, 0, K
    if way == 1:
        A = min(K - 1, LM.MAX_LOOKAHEAD)
        return A, 0, K - A
    if way == 2:
        A = min(K // 3, LM.MAX_LOOKAHEAD)
        H = (K - A) // 2
        return A, H, K - A - H
    return 0, K - 1, 1


def shape_of_call(n, K, i):
    """the i-th variation of a case: the split, the sense, the source's channels, the key's (0: none), the range's start
    (inside the clip; on odd i the range ENDS on the clip's last frame), the key's start, drive, key_gain and makeup"""
    A, H, R = split(K, i)
    first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
    assert A + H + R == K and R >= 1 and first >= 0 and first + n <= SRC_LEN
    j = i % 12                                                  # the 12 combinations of sense, source channels and key, in turn
    return dict(A=A, H=H, R=R, sense=(j // 3) % 2, ch=1 + j // 6, key_ch=j % 3, first=first, key_first=(first + 33, first, 7)[(i // 3) % 3],
                drive=(1.0, 1.5, -0.75)[(i // 2) % 3], key_gain=(1.0, -2.0, 0.5)[i % 3], makeup=(1.0, 1.7, 0.5)[(i // 4) % 3])


CASES = [(n, K, ni + ki) for ni, n in enumerate(FRAMES) for ki, K in enumerate(TERMS)]
PER_CASE = (0, 5)                                               # each case runs variations i and i + 5


def test_the_matrix_covers_what_it_claims():
    shapes = [shape_of_call(n, K, i + d) for n, K, i in CASES for d in PER_CASE]
    assert {0, 1, P // 3, P - 1, 4096} <= {s["A"] for s in shapes} and {0, 1, P - 1, P} <= {s["H"] for s in shapes}
    assert {1, 2, 7, P, 2 * P + 3} <= {s["R"] for s in shapes}
    assert {(s["sense"], s["ch"], s["key_ch"]) for s in shapes} == {(a, b, k) for a in (0, 1) for b in (1, 2) for k in (0, 1, 2)}
    assert {(s["ch"], s["first"] + n == SRC_LEN) for n, K, i in CASES for d in PER_CASE for s in [shape_of_call(n, K, i + d)]} == {
        (1, True), (1, False), (2, True), (2, False)}
    assert any(s["key_ch"] and s["key_first"] != s["first"] for s in shapes) and any(0 < s["first"] for s in shapes)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "frames%d-terms%d" % (c[0], c[1]))
def test_dynamics_matrix(ctx, case):
    n, K, i = case
    for d in PER_CASE:
        s = shape_of_call(n, K, i + d)
        kc = s["key_ch"]
        run_and_check(ctx, SRC[s["ch"]], ctx.src[s["ch"]], s["first"], n, TABLES[s["sense"]], s["sense"], s["drive"], s["makeup"], s["A"], s["H"],
                      s["R"], KEY[kc] if kc else None, ctx.key[kc] if kc else None, s["key_first"], s["key_gain"])


# ---- 2: where the bursts stand -----------------------------------------------------------------------------------------------------
def quiet_with_bursts(n, at, channels=1, seed=0x9EA5, level=0.01):
    rng = np.random.default_rng(seed)
    planes = [rng.uniform(-level, level, n).astype(np.float32) for _ in range(channels)]
    for j, f in enumerate(at):
        planes[j % channels][f] = np.float32((0.9, -0.7, 0.5)[j % 3])
    return planes


@pytest.mark.parametrize("sense", [M.COMPRESS, M.GATE])
@pytest.mark.parametrize("channels", [1, 2])
def test_bursts_on_the_ends_on_tile_seams_and_with_a_release_across_a_segment_seam(ctx, channels, sense):
    """bursts on frame 0 and on the last frame, on both sides of both tile seams; the ramp has 16 + 100 + 3000 terms, so every
    burst's release runs from one segment of the walk into the next.  The quiet frames are at rest in both senses"""
    n = 2 * T + 100
    planes = quiet_with_bursts(n, [0, n - 1, T - 1, T, 2 * T - 1, 2 * T], channels)
    tab = TABLES[sense]
    assert M.lookup(tab, np.array([0.01]))[0] == (1.0 if sense == M.COMPRESS else tab.min())
    ctx.clip_upload(50, "f32", RATE, planes)
    _, ds = run_and_check(ctx, 50, planes, 0, n, tab, sense, A=16, H=100, R=3000)
    assert ds["reduced_frames"] > T
    for A, H, R in ((0, 0, 1), (4096, 0, 1), (1, P - 2, 1), (7, 0, P + 9)):
        run_and_check(ctx, 50, planes, 0, n, tab, sense, A=A, H=H, R=R)
    # bursts in curve frames the look-ahead adds: the range starts right behind one and ends right before another
    run_and_check(ctx, 50, planes, 1, n - 2, tab, sense, A=16, H=100, R=3000)


@pytest.mark.parametrize("sense", [M.COMPRESS, M.GATE])
def test_one_burst_alternates_skipped_and_walked_segments(ctx, sense):
    """three tiles, a ramp of 2P + 3 terms and ONE frame that is not at rest: of the segments a tile walks only those whose
    staged span holds the burst can move anything; the others are skipped by the vote"""
    n, K = 3 * T + 11, 2 * P + 3
    tab = TABLES[sense]
    for at in (T + 5, 0, n - 1):
        planes = quiet_with_bursts(n, [at], 2, seed=at)
        ctx.clip_upload(51, "f32", RATE, planes)
        for i in range(3):
            A, H, R = split(K, i)
            _, ds = run_and_check(ctx, 51, planes, 0, n, tab, sense, A=A, H=H, R=R)
            if sense == M.COMPRESS:
                assert ds["min_gain_frame"] == at and 0 < ds["reduced_frames"] <= K + A
            else:
                lo = tab.min()                                  # (the average of A + 1 copies of lo may round beside it)
                assert abs(ds["min_gain"] - lo) <= lo * (A + 2) * 2.0 ** -53 and ds["reduced_frames"] >= n - K - A


@pytest.mark.parametrize("channels", [1, 2])
def test_material_wholly_at_rest_and_material_never_at_rest(ctx, channels):
    """under the compressor's threshold every want is 1.0 and the clip comes back bit for bit; under the gate's floor every
    want is lo and the clip comes back times lo (every segment is skipped in both).  Then material with no frame at rest:
    all above the compressor's knee, all inside the gate's slope"""
    n = 2 * T + 5
    rng = np.random.default_rng(0x9A55 + channels)
    planes = [rng.uniform(-0.01, 0.01, n).astype(np.float32) for _ in range(channels)]
    planes[0][:3] = -0.0, 0.01, 1e-42
    ctx.clip_upload(52, "f32", RATE, planes)
    lo = GATE.min()
    for A, H, R in ((72, 0, 4800), (0, 0, 1), (4096, 9, 7)):
        got, ds = run_and_check(ctx, 52, planes, 0, n, COMP, M.COMPRESS, A=A, H=H, R=R)
        assert first_bad(got, planes) is None and ds == {"min_gain": 1.0, "min_gain_frame": 0, "reduced_frames": 0}
        got, ds = run_and_check(ctx, 52, planes, 0, n, GATE, M.GATE, A=A, H=H, R=R)
        assert ds["min_gain_frame"] == 0 and ds["reduced_frames"] == n and abs(ds["min_gain"] - lo) <= lo * (A + 2) * 2.0 ** -53
    busy = [(np.sign(p) * (0.3 + 30.0 * np.abs(p))).astype(np.float32) for p in planes]   # 0.3 .. 0.6, either sign
    busy[0][0] = 0.3
    ctx.clip_upload(52, "f32", RATE, busy)
    for sense, tab in ((M.COMPRESS, COMP), (M.GATE, M.table(M.GATE, 0.0, 2.0, 0.0, -60.0))):
        rest = 1.0 if sense == M.COMPRESS else tab.min()
        assert np.all(M.gains(busy, tab, sense, 1.0, 0, 0, 1)[2] != rest)
        _, ds = run_and_check(ctx, 52, busy, 0, n, tab, sense, A=40, H=10, R=P + 100)
        assert ds["reduced_frames"] == n


def test_an_event_on_the_band_seam():
    """2^20 + 2053 frames, mono, keyed by a stereo key: two bands.  Bursts on both sides of the seam, a short ramp: the
    second band recomputes the A curve frames in front of it, and the statistics of the two bands are merged"""
    c = W.MixContext(4, block=128)
    n = BAND + 2053
    planes = quiet_with_bursts(n, [BAND - 1, BAND, 17, BAND + 2040, BAND - 9], 1, seed=0xBA4D)
    key = quiet_with_bursts(n + 9, [BAND + 8, BAND + 9, 30, BAND - 3], 2, seed=0xBA4E)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(3, "f32", RATE, key)
    _, ds = run_and_check(c, 1, planes, 0, n, COMP, M.COMPRESS, A=8, H=3, R=40, dst=2)
    assert ds["min_gain_frame"] == BAND - 1 and ds["reduced_frames"] > 100   # 0.9 on the seam's last frame and again 2041 frames on: the first wins
    _, ds = run_and_check(c, 1, planes, 0, n, GATE, M.GATE, makeup=2.0, A=8, H=3, R=40, key_clip=3, key=key, key_first=9, dst=2)
    assert ds["reduced_frames"] > BAND
    c.close()


# ---- 3: the table's edges, inputs that are not finite, hand-drawn tables ------------------------------------------------------------
def test_levels_at_every_table_edge_reached_through_the_drive(ctx):
    """a source of 1.0, the smallest subnormal float, every cell boundary of the octave of 0.25, 256 and 3e38; drives that
    put 1.0 just below and exactly on 2^-40, at the top of a cell (low 46 mantissa bits all ones) and at the top of the
    table's last cell, and 2^32.  A random table, so that a neighbouring entry shows; lo == 0 in the second"""
    rng = np.random.default_rng(0xED6E)
    x = np.concatenate([[1.0, 1e-45, 3e-45, 256.0, 3e38, -3e38, 0.0, 255.99998], 0.25 * (1.0 + np.arange(65) / 64.0),
                        rng.uniform(-1.0, 1.0, 200)]).astype(np.float32)
    top = np.array([(1023 - 3) << 52 | (17 << 46) | ((1 << 46) - 1), (1023 + 7) << 52 | ((1 << 52) - 1)], dtype=np.uint64).view(np.float64)
    n = len(x)
    ctx.clip_upload(53, "f32", RATE, [x])
    tab = rng.uniform(0.0, 1.0, M.TABLE)
    zero = tab.copy()
    zero[rng.integers(0, M.TABLE, 500)] = 0.0
    for drive in (1.0, 2.0 ** 32, -2.0 ** 32, 2.0 ** -40, float(np.nextafter(2.0 ** -40, 0.0)), float(top[0]), float(top[1]), 2.0 ** -8):
        for sense, t in ((M.COMPRESS, tab), (M.GATE, zero), (M.GATE, tab), (M.COMPRESS, zero)):
            run_and_check(ctx, 53, [x], 0, n, t, sense, drive, 1.0, 3, 2, 9)


@pytest.mark.parametrize("channels", [1, 2])
def test_values_that_are_not_finite_and_frames_beside_the_range(ctx, channels):
    """NaN and +-inf inside the range, in the source and in the key, enter as 0.0; loud samples and NaNs in front of and
    behind the range, in both, do not count"""
    planes, key = source(channels, 3000, seed=0xBE51DE), source(3 - channels, 3100, seed=0xBE51DF)
    for q, shift in ((planes, 0), (key, 50)):
        for c, p in enumerate(q):
            p[:200 + shift], p[190 + shift:200 + shift], p[2700 + shift:], p[2710 + shift:2720 + shift] = 1e30, np.nan, -1e30, np.nan
            at = np.array([200, 205, 500, 2047 + 200, 2048 + 200, 2699]) + shift - c * np.array([0, 1, 1, 1, 1, 1])
            p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    planes[0].view(np.uint32)[240] = 0xFFC12345                 # a NaN with a payload and a sign
    ctx.clip_upload(54, "f32", RATE, planes)
    ctx.clip_upload(55, "f32", RATE, key)
    for first, n in ((200, 2500), (200, 1), (2699, 1), (200, 9)):
        for sense in (M.COMPRESS, M.GATE):
            alone = [p[first:first + n].copy() for p in planes]
            want, want_ds = M.dynamics_clip(alone, 0, n, TABLES[sense], sense, -2.0, 1.5, 64, 10, 500)
            assert np.all(np.isfinite(np.stack(want)))
            got, ds = run_and_check(ctx, 54, planes, first, n, TABLES[sense], sense, -2.0, 1.5, 64, 10, 500)
            assert first_bad(got, want) is None and ds == want_ds
            run_and_check(ctx, 54, planes, first, n, TABLES[sense], sense, 1.0, 1.0, 64, 10, 500, key_clip=55, key=key, key_first=first + 50,
                          key_gain=-3.0)


def test_a_hand_drawn_table_that_is_not_monotonic_and_the_makeups_ends(ctx):
    """a table that wobbles (a curve no design gives), in both senses; then samples of 3e38 under a drive of 2^32 with a
    makeup of 2^-32 (the product is back in fp32's range) and of 0.0 (every sample a zero that keeps its sign)"""
    tab = 0.55 + 0.45 * np.sin(0.37 * np.arange(M.TABLE)) * np.cos(0.011 * np.arange(M.TABLE))
    assert M.table_check(tab) > 0.0 and np.any(np.diff(tab) > 0) and np.any(np.diff(tab) < 0)
    for ch in (1, 2):
        for sense in (M.COMPRESS, M.GATE):
            run_and_check(ctx, SRC[ch], ctx.src[ch], 3, SRC_LEN - 3, tab, sense, 0.8, 1.2, 24, 7, 900)
    x = source(1, 600, seed=0x1F)
    x[0][[5, 300]] = 3e38, -3e38
    ctx.clip_upload(56, "f32", RATE, x)
    for makeup in (0.0, 2.0 ** -32):
        got, _ = run_and_check(ctx, 56, x, 0, 600, np.ones(M.TABLE), M.COMPRESS, 2.0 ** 32, makeup, 4, 0, 10)
        assert np.all(np.isfinite(got[0])) and (makeup > 0.0 or (not np.any(got[0]) and np.any(np.signbit(got[0]))))


def test_time_of_the_last_dynamics_call():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_dynamics_ms(c.h, C.byref(out)) == -4 and out.value == 7.0     # none yet
    c.clip_upload(1, "f32", RATE, source(1, 5000))
    assert c.L.wbx_dynamics_ms(c.h, None) == -4
    c.clip_limit(1, 3, 0, 5000, 0.5)                            # a limit is no dynamics call ...
    assert c.L.wbx_dynamics_ms(c.h, C.byref(out)) == -4
    c.clip_dynamics(1, 4, 0, 5000, COMP)
    assert 0.0 < c.dynamics_ms() < 1000.0
    # ... and the two share the ramp and the stage: a limit between two dynamics calls of another shape changes neither
    planes = source(1, 5000)
    want, _ = M.dynamics_clip(planes, 0, 5000, GATE, M.GATE, A=16, H=4, R=300)
    c.clip_dynamics(1, 4, 0, 5000, GATE, "gate", lookahead_frames=16, hold_frames=4, release_frames=300)
    c.clip_limit(1, 3, 0, 5000, 0.5, 1.0, 8, 0, 48)
    lim_want, _ = LM.limit_clip(planes, 0, 5000, np.float32(0.5), 1.0, 8, 0, 48)
    assert first_bad(download(c, 3, 1, 5000), lim_want) is None
    c.clip_dynamics(1, 5, 0, 5000, GATE, "gate", lookahead_frames=16, hold_frames=4, release_frames=300)
    assert first_bad(download(c, 4, 1, 5000), want) is None and first_bad(download(c, 5, 1, 5000), want) is None
    c.close()


# ---- 4: the pool -------------------------------------------------------------------------------------------------------------------
def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    c.clip_dynamics(1, 10, 0, 4000, COMP)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        run_and_check(c, 1, planes, first, 4000, COMP, M.COMPRESS, dst=10)
        assert c.pool_stats() == with_one
    run_and_check(c, 1, planes, 0, 700, GATE, M.GATE, A=0, H=0, R=1, dst=10)   # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_dynamics(SRC[2], DST, 0, 64, COMP, lookahead_frames=8, hold_frames=0, release_frames=48)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    ctx.clip_upload(61, "f32", 44100, [np.zeros(SRC_LEN, dtype=np.float32)])
    ds, st = _ffi.DynamicsStats(), _ffi.ClipStats()
    S, K = SRC[2], KEY[1]
    spoiled = COMP.copy()
    spoiled[1234] = 1.0 + 2.0 ** -52

    def refused(status, why, src=S, key=NO_KEY, dst=DST, first=0, n=64, key_first=0, sense=0, tab=COMP, drive=1.0, key_gain=1.0, makeup=1.0,
                A=8, H=0, R=48):
        before = ctx.pool_stats()
        ds.reduced_frames = 777
        got = L.wbx_clip_dynamics(ctx.h, src, key, dst, first, n, key_first, sense, None if tab is None else tab.ctypes.data, drive, key_gain,
                                  makeup, A, H, R, C.byref(ds), C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept and ds.reduced_frames == 777

    refused(-4, b"unknown source", src=999)
    refused(-4, b"unknown key", key=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"past the clip", first=SRC_LEN - 10, n=11)
    refused(-4, b"past the clip", first=(1 << 64) - 1, n=2)     # a sum that wraps
    refused(-4, b"key's range ends past", key=K, key_first=SRC_LEN + 40 - 10, n=11)
    refused(-4, b"key's range ends past", key=K, key_first=(1 << 64) - 1, n=2)
    refused(-4, b"may not replace", dst=S)
    refused(-4, b"may not replace", key=K, dst=K)
    refused(-4, b"table is NULL", tab=None)
    refused(-4, b"table entry", tab=spoiled)
    for sense in (2, -1):
        refused(-4, b"unknown sense", sense=sense)
    for v in (0.0, -0.0, np.nan, np.inf, -np.inf, 2.0 ** 33, -2.0 ** 32 * (1 + 2.0 ** -52)):
        refused(-4, b"drive", drive=v)
        refused(-4, b"key_gain", key=K, key_gain=v)
    for v in (-1e-300, np.nan, np.inf, -np.inf):
        refused(-4, b"makeup", makeup=v)
    refused(-4, b"lookahead", A=4097)
    refused(-4, b"hold", H=65537)
    refused(-4, b"release", R=0)
    refused(-4, b"release", R=(1 << 20) + 1)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16)                 # judged on the arithmetic: no clip is that long
    refused(-4, b"sample rate differs", key=61)
    refused(-3, b"not F32", src=60)                             # (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, b"not F32", key=60)
    refused(-3, b"2^44", n=(1 << 24) + 1, A=0, H=0, R=1 << 20)
    refused(-4, b"past the clip", n=1 << 24, A=0, H=0, R=1 << 20)               # ... at the cap the sizes pass, the clip does not
    refused(-3, b"2^44", src=60, n=1 << 30, A=4096, H=65536, R=1 << 20)          # the sizes are judged before the clips are looked at
    refused(-4, b"drive", src=60, drive=0.0)
    # what is not refused: the limits themselves, a key_gain nobody looks at, a source that keys itself by name
    ctx.clip_dynamics(S, 62, SRC_LEN - 1, 1, COMP, "gate", None, 0, 2.0 ** 32, 0.0, 0.0, 4096, 65536, 1 << 20)
    ctx.clip_dynamics(S, 62, 0, 9, np.zeros(M.TABLE), "compress", S, 0, -2.0 ** 32, 2.0 ** 32, 3e300, 0, 0, 1)
    assert L.wbx_clip_free(ctx.h, 62) == 0


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    planes = source(2, n)
    c.clip_upload(1, "f32", RATE, planes)                       # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_dynamics(1, 10 + len(made), 0, n, COMP, lookahead_frames=4, hold_frames=0, release_frames=12)   # 8 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    want, _ = M.dynamics_clip([p[:4096] for p in planes], 0, 4096, COMP, M.COMPRESS, A=4, H=0, R=12)
    got = [c.clip_download(made[-1], k, n, np.float32)[:4000] for k in range(2)]
    assert first_bad(got, [w[:4000] for w in want]) is None      # (the model saw 4096 frames: the look-ahead of the last 4 differs)
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 5: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_dynamics_sample_and_its_conveniences_played_exported_and_measured():
    spec = synth.make_session("dyn2", 3, n_blocks=6, block=128, seed=0xD1A2)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    NU = 3 * LOUD.hop_frames(rate)                              # three hops of the loudness meter
    planes = source(2, NU + 8, seed=0x0B)
    voice = quiet_with_bursts(NU + 40, list(range(3000, 5000, 7)) + list(range(9000, 9400)), 1, seed=0x701CE)
    up, vo = eng.add_sample("f32", rate, planes), eng.add_sample("f32", rate, voice)

    # the engine call itself: a range, keyed by the voice from another frame on, with the result's statistics
    new, ds, st = eng.dynamics_sample(up, GATE, "gate", key_sample=vo, key_first=11, drive=1.25, key_gain=-2.0, makeup=0.9, shape=(30, 20, 700),
                                      first_frame=4, n_frames=NU, stats=True)
    want_new, want_ds = M.dynamics_clip(planes, 4, NU, GATE, M.GATE, 1.25, 0.9, 30, 20, 700, voice, 11, -2.0)
    assert eng._sample_shape[new] == (NU, 2) and ds == want_ds and 0 < ds["reduced_frames"] < NU
    assert first_bad(download(eng.ctx, new, 2, NU), want_new) is None
    check_stats(st, FX.measure(want_new), NU, "dynamics_sample's stats")
    # the conveniences: the Python conversions, then the model on what they gave
    A, H, R = W.limit_frames(rate, 5.0, 0.0, 100.0)
    c_id, ds = eng.compress_sample(up, -12.0, 4.0, 6.0, makeup_db=3.0, n_frames=NU)
    want_c, want_ds = M.dynamics_clip(planes, 0, NU, M.table(M.COMPRESS, -12.0, 4.0, 6.0), M.COMPRESS, 1.0, 10.0 ** (3.0 / 20.0), A, H, R)
    assert ds == want_ds and ds["reduced_frames"] > 0 and first_bad(download(eng.ctx, c_id, 2, NU), want_c) is None
    A, H, R = W.limit_frames(rate, 1.0, 20.0, 100.0)
    g_id, ds = eng.gate_sample(vo, -20.0, 10.0, 0.0, -80.0)
    want_g, want_ds = M.dynamics_clip(voice, 0, NU + 40, M.table(M.GATE, -20.0, 10.0, 0.0, -80.0), M.GATE, A=A, H=H, R=R)
    assert ds == want_ds and eng._sample_shape[g_id] == (NU + 40, 1) and first_bad(download(eng.ctx, g_id, 1, NU + 40), want_g) is None
    assert abs(ds["min_gain"] - 1e-4) < 1e-15                   # -80 dB
    A, H, R = W.limit_frames(rate, 10.0, 50.0, 300.0)
    d_id, ds = eng.duck_sample(up, vo, 12.0, -30.0, n_frames=NU)
    want_d, want_ds = M.dynamics_clip(planes, 0, NU, M.table(M.COMPRESS, -30.0, np.inf, 6.0, -12.0), M.COMPRESS, A=A, H=H, R=R, key=voice)
    assert ds == want_ds and first_bad(download(eng.ctx, d_id, 2, NU), want_d) is None
    assert abs(ds["min_gain"] - 10.0 ** (-12.0 / 20.0)) < 1e-12 and 0 < ds["reduced_frames"] < NU   # ducked by 12 dB under the voice, not elsewhere

    # the compressed sample on a track, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "compressed", 0.5 * unit, 5.5 * unit, 0.0, c_id, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want_c, rate), 1.0, 1.0) == 0
    e.play()
    eng.play()
    eng.render(6)
    m, _, _ = eng.ctx.fetch()
    heard = False
    for b in range(6):
        om, _ = e.process()
        assert np.array_equal(bits(m[b]), bits(om)), b
        heard = heard or bool(om.any())
    assert heard
    # exported, and loudness-measured: an ordinary sample
    got, _ = eng.export_sample(c_id, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want_c, axis=1).reshape(-1).view(np.uint32))
    _, E = eng.loudness_sample(c_id, energies=True, rate=rate)
    want_E = LOUD.hop_energies(want_c, 0, NU, rate)
    assert E.shape == want_E.shape == (2, 3) and np.array_equal(E.view(np.uint64), want_E.view(np.uint64))
    with pytest.raises(W.WbxError):
        eng.delete_sample(c_id)                                 # a clip names it
    eng.delete_sample(d_id)
    # refusals create no sample
    L, new_id = W.lib(), C.c_uint32(12345)
    before = eng.ctx.pool_stats()
    call = lambda s, n, key=NO_KEY, sense=0, tab=COMP, drive=1.0, A=8, R=48, ref=C.byref(new_id): L.wbx_engine_dynamics_sample(
        eng.h, s, key, 0, n, 0, sense, None if tab is None else tab.ctypes.data, drive, 1.0, 1.0, A, 0, R, ref, None, None)
    assert call(9999, 8) == -4
    assert call(d_id, 8) == -4                                  # deleted
    assert call(up, 8, key=d_id) == -4 and call(up, 8, key=9999) == -4
    assert call(up, NU + 9) == -4
    assert call(up, NU + 8, key=vo) == 0 and new_id.value != 12345   # (the voice is long enough)
    new_id.value = 12345
    assert call(up, 0) == -4
    assert call(up, 8, sense=2) == -4
    assert call(up, 8, tab=None) == -4
    assert call(up, 8, drive=np.nan) == -4
    assert call(up, 8, A=4097) == -4
    assert call(up, 8, R=0) == -4
    assert call(up, 8, ref=None) == -4
    assert call(up, (1 << 24) + 1, A=0, R=1 << 20) == -3
    assert new_id.value == 12345
    eng.close()
    e.close()
    assert before[0] >= 1


def test_cpp_adapter_compresses_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::dynamics_sample with a designed 4:1
    table; the result and the statistics equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_dynamics")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_dynamics.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "compressed.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    assert "adapter dynamics ok %d" % n in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    want, ds = M.dynamics_clip([x], 0, n, M.table(M.COMPRESS, -12.0, 4.0, 6.0, -40.0), M.COMPRESS, 2.0, 1.5, 48, 10, 480)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None
    assert ("peak %.9g reduced %d min_gain %.17g at %d" % (np.max(np.abs(want[0])), ds["reduced_frames"], ds["min_gain"],
                                                         ds["min_gain_frame"])) in out, out


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_dynamics_beside_the_audio_thread():
    """The shape of the limiter's test (test_gpu_limit.py): clips far behind the played range name the big source and the big
    key while the threads run, so a delete of either can never succeed — between two calls it is refused for the clip (-4),
    inside one for the pin (-3, asked first) — one thread deletes the two in turn without pause while the other runs keyed
    calls until a delete of EACH has been refused for the pin.  Source and key are busy everywhere, so every segment of the
    2^14-term ramp is walked.  The master is what it is without the calls, and the last result equals the model where it
    is compared: the first, a middle and the last tile."""
    NB, FR, WAIT, CALLS = 300, 1 << 20, 60.0, 96
    A, H, R = 64, 0, (1 << 14) - 64
    spec = synth.make_session("dynthr", 2, n_blocks=NB, block=128, seed=0xD1A712)
    rng = np.random.default_rng(41)
    planes = [rng.uniform(-2.0, 2.0, FR).astype(np.float32) for _ in range(2)]
    key = [rng.uniform(-1.0, 1.0, FR).astype(np.float32)]

    def with_big(eng):                                            # the same session in both runs
        ids = [eng.add_sample("f32", 44100, planes), eng.add_sample("f32", 44100, key)]
        for i, sid in enumerate(ids):
            eng.add_audio_clip(eng.tracks[i], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        return ids

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
    big, kid = with_big(eng)
    first, n, key_first = 5, FR - 8, 3
    L = W.lib()
    began, finished = threading.Event(), threading.Event()
    refused = {big: threading.Event(), kid: threading.Event()}
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        turn = 0
        while not finished.is_set() and time.monotonic() < end:
            sid = (big, kid)[turn & 1]
            turn += 1
            st = L.wbx_engine_delete_sample(eng.h, sid)
            key_ = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key_] = seen.get(key_, 0) + 1
            if st == -3:
                refused[sid].set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not (refused[big].is_set() and refused[kid].is_set()):
                results["big"], results["ds"] = eng.dynamics_sample(big, COMP, "compress", key_sample=kid, key_first=key_first, key_gain=2.0,
                                                                    shape=(A, H, R), first_frame=first, n_frames=n, channels=2, frames=FR)
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
    print("dynamics calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused[big].is_set() and refused[kid].is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every call read live clips: the result is the model's, bit for bit.  A window's gains depend on A frames after it
    # and on H + R frames before it: the model gets those and the comparison is made on the tile in the middle
    assert results["ds"]["reduced_frames"] > n // 2
    for at in (0, (n // 2 // T) * T - 9, n - T - 3):
        lo, hi = max(0, at - H - R - A), min(n, at + T + 3 + A)
        want, _ = M.dynamics_clip(planes, first + lo, hi - lo, COMP, M.COMPRESS, A=A, H=H, R=R, key=key, key_first=key_first + lo, key_gain=2.0)
        got = [eng.ctx.clip_download(results["big"], k, n, np.float32)[at:at + T + 3] for k in range(2)]
        assert first_bad(got, [w[at - lo:at - lo + T + 3] for w in want]) is None, at
    # afterwards: no pin is left (the clips are what refuse now), and with the clips gone the deletes succeed
    for i, sid in enumerate((big, kid)):
        assert L.wbx_engine_delete_sample(eng.h, sid) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
        eng.delete_clip(eng.tracks[i], len(eng.clips(eng.tracks[i])) - 1)
        assert L.wbx_engine_delete_sample(eng.h, sid) == 0
    eng.close()
