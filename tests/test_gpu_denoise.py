"""wbx_clip_denoise, wbx_clip_denoise_profile and their engine calls on the device.  Results come back through
wbx_clip_download and are compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/denoise_model.py, the
numpy twin of the header's text; wbx_denoise_stats are compared field by field, exactly, and the profile's sums as uint64
views.  Sizes are the smallest at which the kernels can still go wrong: around one hop (H = W / 4) and one window, a few
hops and a piece, W = 64 (half a wave without a chain of its own) and 256 (two pairs per lane), one W = 2048 case (two pair
tiles, four chunks), and one call of three bands at W = 64."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import denoise_model as M
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 9 * 256 + 37 + 60
SRC = {1: 1, 2: 2}                                              # channels -> clip id
DST = 100


def source(channels, n=SRC_LEN, seed=0xD01):
    rng = np.random.default_rng(seed + channels)
    return [(0.25 * rng.standard_normal(n)).astype(np.float32) for _ in range(channels)]


def random_thr(channels, win, seed=0x7E):
    """thresholds around the power a cell of `source` has (0.0625 / W per bin, doubled inside by the window's sum), so
    that open and closed cells mix and the gains land between floor and 1; another row per channel"""
    B = win // 2 + 1
    return np.random.default_rng(seed + win).uniform(0.0, 0.2 / win, (channels, B)) * (1.0 + np.arange(channels)[:, None])


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


def denoise_and_check(c, clip, planes, first, n, win, S, F, thr, floor, dst=DST, bands=None):
    """one call against the model: every output bit, every field of wbx_denoise_stats, no NaN"""
    ch = len(planes)
    want, want_st = M.denoise_clip(planes, first, n, win, S, F, thr, floor)
    st = c.clip_denoise(clip, dst, first, n, win, thr, floor=floor, smooth_hops=S, smooth_bins=F)
    got = download(c, dst, ch, n)
    where = (ch, first, n, win, S, F, floor)
    assert first_bad(got, want) is None, (where, first_bad(got, want))
    assert st == dict(want_st, bands=M.launches(n, win, ch) if bands is None else bands), (where, st, want_st)
    assert not any(np.isnan(g).any() for g in got), where
    return got, st


# ---- 1: the matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(0, 0), (1, 1), (4, 8)], ids=lambda v: str(v))
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("win", [64, 256])
def test_matrix_of_lengths(ctx, win, ch, S, F):
    H = win // 4
    thr = random_thr(ch, win)
    for k, n in enumerate([1, H - 1, H, H + 1, win - 1, win, win + 1, 5 * H + 3, 9 * win + 37]):
        first = (0, 3, SRC_LEN - n)[k % 3]                         # from the clip's frame 0, inside, up to its last frame
        _, st = denoise_and_check(ctx, SRC[ch], ctx.src[ch], first, n, win, S, F, thr, 0.125)
        assert st["hops"] == -(-n // H) + 3
    assert 0 < st["open_cells"] < st["cells"]                      # the thresholds split the cells of the longest run


def test_nothing_beside_the_range_is_read():
    """a range between neighbours of +-3e38: the same bits as the range alone, the model's"""
    c = W.MixContext(4, block=128)
    for ch in (1, 2):
        inner = source(ch, 700, seed=0x33)
        walled = [np.concatenate([np.full(300, 3e38 * (1 - 2 * (k & 1)), np.float32), p, np.full(300, -3e38, np.float32)]) for k, p in enumerate(inner)]
        c.clip_upload(1, "f32", RATE, walled)
        for win in (64, 256):
            thr = random_thr(ch, win)
            got, _ = denoise_and_check(c, 1, walled, 300, 700, win, 1, 1, thr, 0.1)
            alone, _ = M.denoise_clip(inner, 0, 700, win, 1, 1, thr, 0.1)
            assert first_bad(got, alone) is None
    c.close()


# ---- 2: the values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [64, 256])
def test_values_that_are_not_finite_and_huge(win):
    c = W.MixContext(4, block=128)
    n = 1300
    for ch in (1, 2):
        planes = source(ch, n, seed=0x44)
        p = planes[0]
        p[100], p[400], p[401], p[700] = np.nan, np.inf, -np.inf, -0.0
        p[720:740] = np.float32(-0.0)
        p[900:960] = np.float32(3e38) * np.where(np.arange(60) % 2, np.float32(-1.0), np.float32(1.0))
        p[1000:1010] = np.float32(3e38)
        c.clip_upload(1, "f32", RATE, planes)
        for thr in (np.zeros((ch, win // 2 + 1)), random_thr(ch, win) * 1e70):
            got, _ = denoise_and_check(c, 1, planes, 0, n, win, 1, 2, thr, 0.5)
    c.close()


def test_thresholds_and_floors(ctx):
    ch, n, win = 2, 5 * 64 + 37, 64
    B = win // 2 + 1
    x = [p[:n] for p in ctx.src[ch]]
    peak = max(np.max(np.abs(p)) for p in x)
    # all 0: every cell open, the source comes back (the model's own error is 3.6e-8 of the peak)
    got, st = denoise_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, win, 2, 1, np.zeros((ch, B)), 0.1)
    assert st["open_cells"] == st["cells"]
    assert max(np.max(np.abs(g.astype(np.float64) - p)) for g, p in zip(got, x)) <= 1e-7 * peak
    # all 1e30: every cell at the floor
    got, st = denoise_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, win, 2, 1, np.full((ch, B), 1e30), 0.25)
    assert st["open_cells"] == 0
    assert max(np.max(np.abs(g.astype(np.float64) - 0.25 * p.astype(np.float64))) for g, p in zip(got, x)) <= 5e-8 * peak
    # floor 0 and floor 1, thresholds that differ per channel: one channel all open, the other all closed
    thr = np.stack([np.zeros(B), np.full(B, 1e30)])
    got, st = denoise_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, win, 2, 1, thr, 0.0)
    assert st["open_cells"] * 2 == st["cells"] and np.all(got[1] == 0.0) and np.any(got[0] != 0.0)
    got, _ = denoise_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, win, 2, 1, random_thr(ch, win), 1.0)
    assert max(np.max(np.abs(g.astype(np.float64) - p)) for g, p in zip(got, x)) <= 1e-7 * peak
    denoise_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, win, 2, 1, random_thr(ch, win), 0.0)


def test_window_2048_stereo(ctx):
    n = 3 * 2048 + 517
    planes = source(2, n + 9, seed=0x99)
    ctx.clip_upload(3, "f32", RATE, planes)
    denoise_and_check(ctx, 3, planes, 4, n, 2048, 2, 1, random_thr(2, 2048), 0.1)
    assert ctx.L.wbx_clip_free(ctx.h, 3) == 0


def test_a_call_across_two_band_seams(ctx):
    """three bands at W = 64, stereo: the whole result against the model (which walks its hops in chunks), so every
    seam's blocks, halo hops and counted cells are in the comparison"""
    win, ch = 64, 2
    per = W.denoise_band_hops(win, ch)
    assert per == M.band_hops(win, ch) == (1 << 22) // (win * ch) - 11
    n = (2 * per + 5) * (win // 4) + 3
    assert M.launches(n, win, ch) == 3
    planes = source(ch, n, seed=0x5EA)
    ctx.clip_upload(3, "f32", RATE, planes)
    denoise_and_check(ctx, 3, planes, 0, n, win, 1, 1, random_thr(ch, win), 0.1, bands=3)
    assert ctx.L.wbx_clip_free(ctx.h, 3) == 0


# ---- 3: the profile --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [64, 256])
def test_profile_sums_and_hops(ctx, win):
    H = win // 4
    for ch in (1, 2):
        for k, n in enumerate([win, win + H - 1, win + H, 9 * win + 37]):
            first = (0, 5, SRC_LEN - n)[k % 3]
            want, want_h = M.profile_clip(ctx.src[ch], first, n, win)
            got, got_h = ctx.clip_denoise_profile(SRC[ch], ch, first, n, win)
            assert got_h == want_h == (n - win) // H + 1
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (win, ch, n)
    assert ctx.denoise_ms() > 0.0


def test_profile_of_many_hops_crosses_its_launches(ctx):
    win, ch = 64, 2
    n = ((1 << 22) // (win * ch) + 40) * (win // 4) + win
    planes = source(ch, n, seed=0x77)
    ctx.clip_upload(3, "f32", RATE, planes)
    want, want_h = M.profile_clip(planes, 0, n, win)
    got, got_h = ctx.clip_denoise_profile(3, ch, 0, n, win)
    assert got_h == want_h and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert ctx.L.wbx_clip_free(ctx.h, 3) == 0


# ---- 4: the pool, the refusals ---------------------------------------------------------------------------------------------------
def test_pool_unchanged_but_for_the_result_and_the_timer(ctx):
    n, win = 2051, 256
    thr = random_thr(2, win)
    base = ctx.pool_stats()
    ctx.clip_denoise_profile(SRC[2], 2, 0, n, win)
    assert ctx.pool_stats() == base
    ctx.clip_denoise(SRC[2], 120, 0, n, win, thr)
    with_one = ctx.pool_stats()
    ctx.clip_derive(SRC[2], 121, W.edit_desc(0, n))               # a plain copy of the same size takes the same
    assert [b - a for a, b in zip(with_one, ctx.pool_stats())][2] == [b - a for a, b in zip(base, with_one)][2]
    assert ctx.L.wbx_clip_free(ctx.h, 121) == 0
    for _ in range(3):                                             # a replaced dst takes the old extent
        ctx.clip_denoise(SRC[2], 120, 3, n, win, thr)
        assert ctx.pool_stats() == with_one
    assert ctx.denoise_ms() > 0.0
    assert ctx.L.wbx_clip_free(ctx.h, 120) == 0
    assert ctx.pool_stats() == base


def test_the_timer_needs_a_completed_call():
    c = W.MixContext(4, block=128)
    out = C.c_double(-1.0)
    assert c.L.wbx_denoise_ms(c.h, C.byref(out)) == -4 and out.value == -1.0
    assert b"no denoise call has completed" in c.L.wbx_last_error(c.h)
    assert c.L.wbx_denoise_ms(c.h, None) == -4 and c.L.wbx_denoise_ms(None, C.byref(out)) == -4
    c.close()


def test_every_refusal_leaves_pool_dst_and_outputs_untouched(ctx):
    L = W.lib()
    win = 64
    B = win // 2 + 1
    good = random_thr(2, win)
    ctx.clip_denoise(SRC[2], DST, 0, 64, win, good)
    kept = [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, 64)]
    ctx.clip_upload(5, "i16", RATE, [np.zeros(500, np.int16)] * 2)
    neg, nan, second = good.copy(), good.copy(), good.copy()
    neg[0, 7], nan[0, B - 1], second[1, 3] = -1e-300, np.nan, np.inf
    base = dict(src=SRC[2], dst=DST, first=0, n=64, win=win, S=2, F=1, thr=good, floor=0.1)
    cases = [(dict(n=0), -4, "no frames"), (dict(n=(1 << 31) - 16), -4, "2^31 - 16"), (dict(win=96), -4, "power of two"),
             (dict(win=32), -4, "power of two"), (dict(win=4096), -4, "power of two"), (dict(S=5), -4, "smooth_hops"),
             (dict(F=9), -4, "smooth_bins"), (dict(thr=None), -4, "threshold is NULL"), (dict(thr=neg), -4, "threshold entry"),
             (dict(thr=nan), -4, "threshold entry"), (dict(thr=second), -4, "threshold entry"), (dict(floor=-0.01), -4, "floor"),
             (dict(floor=1.01), -4, "floor"), (dict(floor=np.nan), -4, "floor"),
             (dict(src=999), -4, "unknown source"), (dict(first=SRC_LEN - 63), -4, "range ends past"), (dict(dst=SRC[2]), -4, "replace its source"),
             (dict(src=5), -3, "not F32"), (dict(dst=1 << 24), -4, "clip id"),
             # the order: n, W, S, F, thr, its entries, the floor; the parameters before the clip; the range before the
             # result's place before the storage; the id's bound last
             (dict(n=0, win=96), -4, "no frames"), (dict(win=96, S=5), -4, "power of two"), (dict(S=5, F=9), -4, "smooth_hops"),
             (dict(F=9, thr=None), -4, "smooth_bins"), (dict(thr=None, floor=2.0), -4, "threshold is NULL"), (dict(thr=neg, floor=2.0), -4, "threshold entry"),
             (dict(src=999, floor=2.0), -4, "floor"), (dict(src=999, thr=second), -4, "unknown source"),   # (an unknown clip: the first row alone)
             (dict(src=5, n=501), -4, "range ends past"), (dict(dst=SRC[2], first=SRC_LEN), -4, "range ends past"),
             (dict(src=5, dst=5), -4, "replace its source"), (dict(src=5, dst=1 << 24), -3, "not F32"), (dict(dst=1 << 24, floor=np.nan), -4, "floor")]
    before = ctx.pool_stats()
    for change, status, text in cases:
        a = dict(base, **change)
        ds = _ffi.DenoiseStats()
        ds.hops, ds.cells, ds.open_cells, ds.bands = 9, 8, 7, 6
        t = a["thr"]
        st = L.wbx_clip_denoise(ctx.h, a["src"], a["first"], a["n"], a["win"], a["S"], a["F"], None if t is None else t.ctypes.data,
                                float(a["floor"]), a["dst"], C.byref(ds))
        assert st == status and text in L.wbx_last_error(ctx.h).decode(), (change, st, L.wbx_last_error(ctx.h))
        assert (ds.hops, ds.cells, ds.open_cells, ds.bands) == (9, 8, 7, 6) and ctx.pool_stats() == before, change
    assert [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, 64)] == kept
    # the profile's
    cases = [(dict(n=0), -4, "no frames"), (dict(n=(1 << 31) - 16), -4, "2^31 - 16"), (dict(win=100), -4, "power of two"),
             (dict(n=63), -4, "fewer frames than one window"), (dict(sums=False), -4, "output is NULL"), (dict(hops=False), -4, "output is NULL"),
             (dict(src=999), -4, "unknown source"), (dict(first=SRC_LEN - 63), -4, "range ends past"), (dict(src=5), -3, "not F32"),
             (dict(src=999, n=63), -4, "fewer frames"), (dict(n=0, win=100), -4, "no frames"),
             (dict(win=100, n=63), -4, "power of two"), (dict(src=5, n=501), -4, "range ends past")]
    for change, status, text in cases:
        a = dict(dict(src=SRC[2], first=0, n=64, win=win, sums=True, hops=True), **change)
        sums, hops = np.full(2 * B, 5.5), C.c_uint64(77)
        st = L.wbx_clip_denoise_profile(ctx.h, a["src"], a["first"], a["n"], a["win"], sums.ctypes.data if a["sums"] else None,
                                        C.byref(hops) if a["hops"] else None)
        assert st == status and text in L.wbx_last_error(ctx.h).decode(), (change, st, L.wbx_last_error(ctx.h))
        assert np.all(sums == 5.5) and hops.value == 77 and ctx.pool_stats() == before, change
    assert ctx.L.wbx_clip_free(ctx.h, 5) == 0


# ---- 5: layer 2 ------------------------------------------------------------------------------------------------------------------
def test_engine_entry_points_follow_the_sample_call_protocol():
    """the four points of tests/test_gpu_sample_calls.py for wbx_engine_denoise_sample, and the measurer's for
    wbx_engine_denoise_profile_sample"""
    N, win = 4096, 256
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    L = eng.L
    planes = source(2, N, seed=0x5A3)
    thr = random_thr(2, win)

    def refused(call, status, message=None):
        with pytest.raises(W.WbxError) as err:
            call()
        assert err.value.status == status
        if message is not None:
            assert L.wbx_engine_last_error(eng.h).decode() == message

    # 1: an unknown id
    refused(lambda: eng.denoise_sample(9999, win, thr, first_frame=0, n_frames=N), -4, "denoise_sample: unknown sample")
    refused(lambda: eng.denoise_profile_sample(9999, win, 0, N, channels=2), -4, "denoise_profile_sample: unknown sample")
    # 2: a refusing check leaves no pin
    s = eng.add_sample("f32", RATE, planes)
    refused(lambda: eng.denoise_sample(s, win, thr, first_frame=1, n_frames=N), -4, "clip denoise: the range ends past the clip")
    refused(lambda: eng.denoise_profile_sample(s, win, 0, win - 1), -4, "clip denoise profile: fewer frames than one window")
    eng.delete_sample(s)
    rng16 = np.random.default_rng(0x116)
    s16 = eng.add_sample("i16", RATE, [rng16.integers(-20000, 20000, N).astype(np.int16) for _ in range(2)])
    refused(lambda: eng.denoise_sample(s16, win, thr, first_frame=0, n_frames=N), -3, "clip denoise: the clip's storage format is not F32")
    eng.delete_sample(s16)
    # 3: a success is the pool's next id, registered with n_frames, the source's channels and rate; the profile makes none
    s = eng.add_sample("f32", RATE, planes)
    n = N - 100
    sums, hops = eng.denoise_profile_sample(s, win, 50, n)
    want_sums, want_hops = M.profile_clip(planes, 50, n, win)
    assert hops == want_hops and np.array_equal(sums.view(np.uint64), want_sums.view(np.uint64))
    new, st = eng.denoise_sample(s, win, thr, floor=0.2, smooth_hops=1, smooth_bins=2, first_frame=50, n_frames=n)
    assert new == s + 1
    want, want_st = M.denoise_clip(planes, 50, n, win, 1, 2, thr, 0.2)
    assert first_bad(download(eng.ctx, new, 2, n), want) is None and st == dict(want_st, bands=1)
    eng.measure_sample(new, 0, n, channels=2)
    refused(lambda: eng.measure_sample(new, 0, n + 1, channels=2), -4)
    assert eng._sample_rate.get(new, RATE) == RATE
    up = eng.resample_sample(new, 96000, "fast", 0, n)
    up_id = up[0] if isinstance(up, tuple) else up
    eng.measure_sample(up_id, 0, 2 * n, channels=2)               # registered at the source's rate: 48 kHz -> 96 kHz doubles it
    eng.delete_sample(s)
    # 4: a NULL new_sample
    s2 = eng.add_sample("f32", RATE, planes)
    assert L.wbx_engine_denoise_sample(eng.h, s2, 0, N, win, 2, 1, thr.ctypes.data, 0.1, None, None) == -4
    assert L.wbx_engine_last_error(eng.h).decode() == "denoise_sample: new_sample is NULL"
    eng.delete_sample(s2)
    eng.close()


def test_reduce_noise_sample_builds_the_models_threshold():
    """the profile of a noise stretch of ANOTHER sample, the threshold and the floor the convenience builds, then the call:
    the result is the model's for that threshold and floor, and the noise-only head drops by the floor"""
    win, n = 256, 6000
    rng = np.random.default_rng(0x201)
    noise = [(0.01 * rng.standard_normal(3000)).astype(np.float32)]
    t = np.arange(n, dtype=np.float64)
    x = 0.01 * rng.standard_normal(n)
    x[2000:] += 0.3 * np.sin(2 * np.pi * 0.05 * t[2000:])
    planes = [x.astype(np.float32)]
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    s, ns = eng.add_sample("f32", RATE, planes), eng.add_sample("f32", RATE, noise)
    new, st = eng.reduce_noise_sample(s, 100, 2500, reduction_db=12.0, sensitivity=4.0, window=win, smooth_hops=1, smooth_bins=1,
                                      noise_sample=ns, channels=1, frames=n)
    sums, hops = M.profile_clip(noise, 100, 2500, win)
    thr = M.threshold(sums, hops, 4.0)
    assert np.array_equal(W.denoise_threshold(sums, hops, 4.0).view(np.uint64), thr.view(np.uint64))
    floor = 10.0 ** (-12.0 / 20.0)
    want, want_st = M.denoise_clip(planes, 0, n, win, 1, 1, thr, floor)
    got = download(eng.ctx, new, 1, n)
    assert first_bad(got, want) is None and st == dict(want_st, bands=1)
    head_in, head_out = planes[0][:1500].astype(np.float64), got[0][:1500].astype(np.float64)
    drop = 10.0 * np.log10(np.sum(head_in ** 2) / np.sum(head_out ** 2))
    print("noise-only head drops by %.2f dB (floor 12 dB)" % drop)
    assert 9.0 <= drop <= 12.1
    eng.close()


def test_cpp_adapter_denoises_a_take(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_denoise")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_denoise.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "denoised.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n, win = 5 * 512, 256
    assert "adapter denoise ok %d" % n in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    sums, hops = M.profile_clip([x], 0, 1024, win)
    want, st = M.denoise_clip([x], 0, n, win, 2, 1, M.threshold(sums, hops, 1.0), 0.1)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None
    assert ("hops %d cells %d open %d bands 1" % (st["hops"], st["cells"], st["open_cells"])) in out, out


# ---- 6: beside the renders and the audio thread -------------------------------------------------------------------------------
def test_a_denoise_call_between_two_renders_leaves_the_master_bit_equal():
    spec = synth.make_session("denrender", 2, n_blocks=8, block=128, seed=0xDE01)

    def render(with_call):
        eng = build_engine(spec, max_blocks=1)
        out = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        heard = []
        for b in range(8):
            if with_call and b == 4:
                s = eng.add_sample("f32", RATE, source(2, 3000, seed=0x12))
                eng.denoise_sample(s, 256, random_thr(2, 256), first_frame=0, n_frames=3000)
            eng.process(None, out, float(spec.sample_rate))
            heard.append(np.stack(out.channel_buffers).copy())
        eng.close()
        return heard

    a, b = render(False), render(True)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_denoise_beside_the_audio_thread():
    """The shape of the saturate's test (test_gpu_saturate.py): a clip far behind the played range names the big source
    while the threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside
    one for the pin (-3, asked first) — one thread deletes without pause while the other denoises until a delete has been
    refused for the pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS, win = 300, 1 << 17, 60.0, 96, 1024
    spec = synth.make_session("denthr", 2, n_blocks=NB, block=128, seed=0xDE7712)
    planes = source(2, FR, seed=41)
    thr = random_thr(2, win)

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
                results["big"], results["stats"] = eng.denoise_sample(big, win, thr, first_frame=first, n_frames=n, channels=2, frames=FR)
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
    print("denoise calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    want, want_st = M.denoise_clip(planes, first, n, win, 2, 1, thr, 0.1)
    assert results["stats"] == dict(want_st, bands=1) and first_bad(download(eng.ctx, results["big"], 2, n), want) is None
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
