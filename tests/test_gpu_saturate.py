"""wbx_clip_saturate and wbx_engine_saturate_sample on the device.  Results come back through wbx_clip_download and are
compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/saturate_model.py, the numpy twin of the
header's text — tests/resample_model.py up, the lookup, tests/resample_model.py down —; wbx_saturate_stats are compared
field by field, exactly.  Sizes are the smallest at which the kernels can still go wrong, around the tile
wbx_saturate_launch_shape reports (768 or 1024 output frames per workgroup): a lane's 4 frames and the last lane's partial
store (1, 5), one tile less, exactly and more than a frame, two tiles and a piece (the seams), and one run of 2^18 + 3."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import clipfx_model as FX
import resample_model as RM
import saturate_model as M
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 3000 + 100
SRC = {1: 1, 2: 2}                                              # channels -> clip id
DST = 100
LEGAL = [(os_, q) for os_ in (1, 2, 4, 8) for q in (M.FAST, M.GOOD, M.BEST) if (os_, q) != (8, M.BEST)]


def source(channels, n=SRC_LEN, seed=0x5A7):
    rng = np.random.default_rng(seed + channels)
    return [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(channels)]


def hand_drawn(seed=0x7AB):
    """a RANDOM table: every index matters, an off-by-one cell cannot hide behind a smooth curve"""
    return np.random.default_rng(seed).uniform(-2.0, 2.0, M.TABLE)


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
    c.tabs = {"random": hand_drawn(), "designed": W.saturate_table("tanh", 0.25)}
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
    assert FX.exact_fields_equal(got, want), (where, got, {k: want[k] for k in FX.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if np.isfinite(a):
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


def saturate_and_check(c, clip, planes, first, n, os_, q, tab, drive=1.0, makeup=1.0, dst=DST):
    """one call against the model: every output bit, wbx_saturate_stats, stats_of_result, no NaN and no infinity"""
    ch = len(planes)
    want, want_ss = M.saturate(planes, first, n, os_, q, tab, drive, makeup)
    ss, st = c.clip_saturate(clip, dst, first, n, tab, os=os_, quality=q, drive=drive, makeup=makeup, stats_channels=ch)
    got = download(c, dst, ch, n)
    where = (ch, first, n, os_, q, drive, makeup)
    assert first_bad(got, want) is None, (where, first_bad(got, want))
    assert ss == want_ss, (where, ss, want_ss)
    assert all(np.all(np.isfinite(g)) for g in got), where
    check_stats(st, FX.measure(want), n, where)
    return got, ss


def tile_of(os_, q, ch):
    return W.saturate_launch_shape(os_, q, ch, 1)["tile"]


# ---- 1: the matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("os_,q", LEGAL, ids=lambda v: str(v))
@pytest.mark.parametrize("ch", [1, 2])
def test_matrix_at_tile_plus_3(ctx, os_, q, ch):
    n = tile_of(os_, q, ch) + 3
    i = os_ + q + ch
    first = SRC_LEN - n if i % 2 else 7
    saturate_and_check(ctx, SRC[ch], ctx.src[ch], first, n, os_, q, ctx.tabs["random"], drive=(1.7, -3.0, 9.5)[i % 3], makeup=(0.5, -1.25)[i % 2])
    saturate_and_check(ctx, SRC[ch], ctx.src[ch], first, n, os_, q, ctx.tabs["designed"], drive=2.5, makeup=0.8)


@pytest.mark.parametrize("os_,q", [(1, M.GOOD), (2, M.FAST), (4, M.GOOD), (8, M.GOOD), (4, M.BEST)], ids=lambda v: str(v))
def test_smallest_shapes_seams_and_clip_ends(ctx, os_, q):
    for ch in (1, 2):
        t = tile_of(os_, q, ch)
        for k, n in enumerate([1, 5, t - 1, t, t + 1, 2 * t + 3]):
            first = (0, 3, SRC_LEN - n)[k % 3]                     # from the clip's frame 0, inside, up to its last frame
            saturate_and_check(ctx, SRC[ch], ctx.src[ch], first, n, os_, q, ctx.tabs["random"], drive=4.0, makeup=-0.5)


def test_nothing_beside_the_range_is_read():
    """a range between neighbours of +-3e38: the same bits as the range alone, the model's"""
    c = W.MixContext(4, block=128)
    tab = hand_drawn()
    for ch in (1, 2):
        inner = source(ch, 1500, seed=0x33)
        walled = [np.concatenate([np.full(200, 3e38 * (1 - 2 * (k & 1)), np.float32), p, np.full(200, -3e38, np.float32)]) for k, p in enumerate(inner)]
        c.clip_upload(1, "f32", RATE, walled)
        for os_, q in ((1, M.GOOD), (4, M.GOOD), (8, M.FAST)):
            got, _ = saturate_and_check(c, 1, walled, 200, 1500, os_, q, tab, drive=2.0)
            alone, _ = M.saturate(inner, 0, 1500, os_, q, tab, 2.0, 1.0)
            assert first_bad(got, alone) is None
    c.close()


# ---- 2: the values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("os_,q", [(1, M.GOOD), (2, M.GOOD), (4, M.FAST), (8, M.GOOD)], ids=lambda v: str(v))
def test_values_that_are_not_finite_and_overflow(os_, q):
    c = W.MixContext(4, block=128)
    tab = hand_drawn()
    n = 1300
    for ch in (1, 2):
        planes = source(ch, n, seed=0x44)
        p = planes[0]
        p[100], p[400], p[401], p[700] = np.nan, np.inf, -np.inf, -0.0
        p[900:960] = np.float32(3e38) * np.where(np.arange(60) % 2, np.float32(-1.0), np.float32(1.0))   # the up-sum overflows fp32
        p[1000:1010] = np.float32(3e38)
        c.clip_upload(1, "f32", RATE, planes)
        if os_ > 1:
            u = RM.resample(planes, 0, n, 1, os_, q)
            assert np.isnan(u[0]).sum() >= 2 * RM.QUALITY[q][0] * os_ and np.isinf(u[0]).sum() > 0
        got, ss = saturate_and_check(c, 1, planes, 0, n, os_, q, tab, drive=0.75, makeup=2.0)
    c.close()


def test_drive_makeup_and_bias_corners(ctx):
    ch, n = 2, 1100
    for os_, q in ((1, M.GOOD), (4, M.GOOD)):
        # drive 2^32 over full-scale noise: every sample lies beyond the table
        loud = [np.where(p >= 0, np.float32(1.0), np.float32(-1.0)) * (np.abs(p) + np.float32(0.5)) for p in ctx.src[ch]]
        ctx.clip_upload(3, "f32", RATE, loud)
        _, ss = saturate_and_check(ctx, 3, loud, 5, n, os_, q, ctx.tabs["random"], drive=2.0 ** 32)
        assert ss["beyond"] == ch * n * os_
        # makeup 0 and a negative makeup
        got, _ = saturate_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, os_, q, ctx.tabs["random"], makeup=0.0)
        assert all(np.all(g == 0.0) for g in got)
        saturate_and_check(ctx, SRC[ch], ctx.src[ch], 0, n, os_, q, ctx.tabs["random"], drive=-1.0, makeup=-2.0 ** 32)
        # silence through a biased table: f(0) * makeup inside, the band-limited edge is the model's, not a constant
        ctx.clip_upload(3, "f32", RATE, [np.zeros(SRC_LEN, np.float32)] * ch)
        tab = ctx.tabs["designed"] + 0.125
        got, _ = saturate_and_check(ctx, 3, [np.zeros(SRC_LEN, np.float32)] * ch, 0, n, os_, q, tab, makeup=0.5)
        assert got[0][n // 2] == pytest.approx(tab[8192] * 0.5, rel=1e-3) and (os_ == 1 or got[0][0] != got[0][n // 2])
    assert ctx.L.wbx_clip_free(ctx.h, 3) == 0


def test_one_longer_run(ctx):
    n = (1 << 18) + 3
    planes = source(2, n + 10, seed=0x99)
    ctx.clip_upload(3, "f32", RATE, planes)
    saturate_and_check(ctx, 3, planes, 4, n, 4, M.GOOD, ctx.tabs["random"], drive=3.0, makeup=0.7)
    assert ctx.L.wbx_clip_free(ctx.h, 3) == 0


# ---- 3: the definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("os_,q", [(2, M.FAST), (4, M.FAST), (8, M.FAST), (4, M.BEST)], ids=lambda v: str(v))
def test_the_fused_call_is_the_three_calls_in_a_row_on_the_device(ctx, os_, q):
    n, first, ch = 3000, 9, 2
    tab = ctx.tabs["random"]
    fused = ctx.clip_saturate(SRC[ch], DST, first, n, tab, os=os_, quality=q, drive=2.2, makeup=0.6)
    ctx.clip_resample(SRC[ch], 110, first, n, RATE * os_, q)
    mid = ctx.clip_saturate(110, 111, 0, n * os_, tab, os=1, quality=q, drive=2.2, makeup=0.6)
    ctx.clip_resample(111, 112, 0, n * os_, RATE, q)
    assert first_bad(download(ctx, DST, ch, n), download(ctx, 112, ch, n)) is None and fused == mid
    for k in (110, 111, 112):
        assert ctx.L.wbx_clip_free(ctx.h, k) == 0


# ---- 4: the pool, the refusals ---------------------------------------------------------------------------------------------------
def test_no_intermediate_in_the_pool_and_replace_and_free(ctx):
    n = 2051
    base = ctx.pool_stats()
    ctx.clip_saturate(SRC[2], 120, 0, n, ctx.tabs["random"], os=8, quality=M.GOOD)
    with_one = ctx.pool_stats()
    ctx.clip_derive(SRC[2], 121, W.edit_desc(0, n))               # a plain copy of the same size takes the same
    assert [b - a for a, b in zip(with_one, ctx.pool_stats())][2] == [b - a for a, b in zip(base, with_one)][2]
    assert ctx.L.wbx_clip_free(ctx.h, 121) == 0
    for _ in range(3):                                             # a replaced dst takes the old extent
        ctx.clip_saturate(SRC[2], 120, 3, n, ctx.tabs["designed"], os=4, quality=M.FAST)
        assert ctx.pool_stats() == with_one
    assert ctx.saturate_ms() > 0.0
    assert ctx.L.wbx_clip_free(ctx.h, 120) == 0
    assert ctx.pool_stats() == base


def test_every_refusal_leaves_pool_dst_and_stats_untouched(ctx):
    L = W.lib()
    good = ctx.tabs["random"]
    ctx.clip_saturate(SRC[2], DST, 0, 64, good, os=2, quality=M.FAST)
    kept = [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, 64)]
    ctx.clip_upload(5, "i16", RATE, [np.zeros(500, np.int16)] * 2)
    bad = good.copy()
    bad[77] = np.nan
    base = dict(src=SRC[2], dst=DST, first=0, n=64, os=4, q=M.GOOD, tab=good, drive=1.0, makeup=1.0)
    cases = [(dict(n=0), -4, "no frames"), (dict(os=3), -4, "os is not"), (dict(q=9), -4, "quality"), (dict(tab=None), -4, "table is NULL"),
             (dict(tab=bad), -4, "table entry"), (dict(drive=0.0), -4, "drive"), (dict(makeup=np.inf), -4, "makeup"),
             (dict(n=1 << 29, os=8), -4, "2^31 - 16"), (dict(os=8, q=M.BEST), -3, "512 taps"),
             (dict(src=999), -4, "unknown source"), (dict(first=SRC_LEN - 63), -4, "range ends past"), (dict(dst=SRC[2]), -4, "replace its source"),
             (dict(src=5), -3, "not F32"), (dict(dst=1 << 24), -4, "clip id"),
             # the order: the parameters before the clip, the range before the result's place before the storage
             (dict(src=999, os=3), -4, "os is not"), (dict(src=999, os=8, q=M.BEST), -3, "512 taps"), (dict(src=5, n=501), -4, "range ends past"),
             (dict(dst=SRC[2], first=SRC_LEN), -4, "range ends past"), (dict(src=5, dst=5), -4, "replace its source"), (dict(n=0, tab=None), -4, "no frames"),
             (dict(src=5, dst=1 << 24), -3, "not F32"), (dict(dst=1 << 24, makeup=np.nan), -4, "makeup")]    # the id's bound comes last
    before = ctx.pool_stats()
    for change, status, text in cases:
        a = dict(base, **change)
        ss = _ffi.SaturateStats()
        ss.peak_drive, ss.peak_index, ss.beyond = 9.0, 8, 7
        t = a["tab"]
        st = L.wbx_clip_saturate(ctx.h, a["src"], a["dst"], a["first"], a["n"], a["os"], a["q"], None if t is None else t.ctypes.data,
                                 float(a["drive"]), float(a["makeup"]), C.byref(ss), None)
        assert st == status and text in L.wbx_last_error(ctx.h).decode(), (change, st, L.wbx_last_error(ctx.h))
        assert (ss.peak_drive, ss.peak_index, ss.beyond) == (9.0, 8, 7) and ctx.pool_stats() == before, change
    assert [p.view(np.uint32).tolist() for p in download(ctx, DST, 2, 64)] == kept
    assert ctx.L.wbx_clip_free(ctx.h, 5) == 0


# ---- 5: layer 2 ------------------------------------------------------------------------------------------------------------------
def test_engine_entry_point_follows_the_sample_call_protocol():
    """the four points of tests/test_gpu_sample_calls.py for wbx_engine_saturate_sample"""
    N = 4096
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    L, tab = eng.L, hand_drawn()
    rng = np.random.default_rng(0x5A3)
    planes = [rng.uniform(-0.5, 0.5, N).astype(np.float32) for _ in range(2)]

    def refused(call, status, message=None):
        with pytest.raises(W.WbxError) as err:
            call()
        assert err.value.status == status
        if message is not None:
            assert L.wbx_engine_last_error(eng.h).decode() == message

    # 1: an unknown id
    refused(lambda: eng.saturate_sample(9999, tab, first_frame=0, n_frames=N), -4, "saturate_sample: unknown sample")
    # 2: a refusing check leaves no pin
    s = eng.add_sample("f32", RATE, planes)
    refused(lambda: eng.saturate_sample(s, tab, first_frame=1, n_frames=N), -4, "clip saturate: the range ends past the clip")
    eng.delete_sample(s)
    rng16 = np.random.default_rng(0x116)
    s16 = eng.add_sample("i16", RATE, [rng16.integers(-20000, 20000, N).astype(np.int16) for _ in range(2)])
    refused(lambda: eng.saturate_sample(s16, tab, first_frame=0, n_frames=N), -3, "clip saturate: the clip's storage format is not F32")
    eng.delete_sample(s16)
    # 3: a success is the pool's next id, registered with n_frames, the source's channels and rate
    s = eng.add_sample("f32", RATE, planes)
    n = N - 100
    new, ss, st = eng.saturate_sample(s, tab, os=4, quality="good", drive=3.0, makeup=0.5, first_frame=50, n_frames=n, stats=True)
    assert new == s + 1
    want, want_ss = M.saturate(planes, 50, n, 4, M.GOOD, tab, 3.0, 0.5)
    assert first_bad(download(eng.ctx, new, 2, n), want) is None and ss == want_ss
    check_stats(st, FX.measure(want), n, "engine")
    eng.measure_sample(new, 0, n, channels=2)
    refused(lambda: eng.measure_sample(new, 0, n + 1, channels=2), -4)
    assert eng._sample_rate.get(new, RATE) == RATE
    up = eng.resample_sample(new, 96000, "fast", 0, n)
    up_id = up[0] if isinstance(up, tuple) else up
    assert W.resample_frames(RATE, 96000, n) == 2 * n            # registered at the source's rate: 48 kHz -> 96 kHz doubles it
    eng.measure_sample(up_id, 0, 2 * n, channels=2)
    eng.delete_sample(s)
    # 4: a NULL new_sample
    s2 = eng.add_sample("f32", RATE, planes)
    assert L.wbx_engine_saturate_sample(eng.h, s2, 0, N, 4, 1, tab.ctypes.data, 1.0, 1.0, None, None, None) == -4
    assert L.wbx_engine_last_error(eng.h).decode() == "saturate_sample: new_sample is NULL"
    eng.delete_sample(s2)
    eng.close()


def test_soft_clip_sample_keeps_the_ceiling():
    eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
    eng.add_track("t")
    t = np.arange(20000, dtype=np.float64)
    planes = [(0.9 * np.sin(2 * np.pi * 3500.0 * t / RATE + k)).astype(np.float32) for k in range(2)]
    s = eng.add_sample("f32", RATE, planes)
    ceiling = np.float32(10.0 ** (-3.0 / 20.0))
    free, _ = eng.soft_clip_sample(s, ceiling_db=-3.0, drive_db=18.0, kind="hard", guarantee=False)
    safe, ss = eng.soft_clip_sample(s, ceiling_db=-3.0, drive_db=18.0, kind="hard", guarantee=True)
    peak_free = max(eng.measure_sample(free, channels=2)["peak"])
    peak_safe = max(eng.measure_sample(safe, channels=2)["peak"])
    print("soft clip peaks: free %.6f safe %.6f ceiling %.6f" % (peak_free, peak_safe, ceiling))
    assert peak_free > ceiling                                     # the documented overshoot
    assert peak_safe <= ceiling and ss["peak_drive"] > 1.0
    eng.close()


def test_cpp_adapter_saturates_a_take(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_saturate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_saturate.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "saturated.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    assert "adapter saturate ok %d" % n in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    want, ss = M.saturate([x], 0, n, 4, M.GOOD, M.table(M.CUBIC, 0.25), 3.0, 0.5)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None
    assert ("peak %.9g peak_drive %.17g at %d beyond %d" % (np.max(np.abs(want[0])), ss["peak_drive"], ss["peak_index"], ss["beyond"])) in out, out


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_saturate_beside_the_audio_thread():
    """The shape of the pitch's test (test_gpu_pitch.py): a clip far behind the played range names the big source while the
    threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one for
    the pin (-3, asked first) — one thread deletes without pause while the other saturates until a delete has been refused
    for the pin.  The master is what it is without the calls, and the last result equals the model."""
    NB, FR, WAIT, CALLS = 300, 1 << 19, 60.0, 96
    spec = synth.make_session("satthr", 2, n_blocks=NB, block=128, seed=0x5A7712)
    planes = source(2, FR, seed=41)
    tab = hand_drawn()

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
                results["big"], results["stats"] = eng.saturate_sample(big, tab, os=8, quality="good", drive=2.0, first_frame=first,
                                                                       n_frames=n, channels=2, frames=FR)
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
    print("saturate calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    want, want_ss = M.saturate(planes, first, n, 8, M.GOOD, tab, 2.0, 1.0)
    assert results["stats"] == want_ss and first_bad(download(eng.ctx, results["big"], 2, n), want) is None
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
