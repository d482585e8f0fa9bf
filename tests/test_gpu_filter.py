"""wbx_clip_filter and wbx_engine_filter_sample on the device.  Results come back through wbx_clip_download and are compared
BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/filter_model.py, the numpy twin of the header's text.
Lengths are the smallest at which the kernels can still go wrong: around one chunk of 512 frames (no carry at all, the
first carried state), around the 64 chunks one wave owns, and three waves plus one frame.  The source is uniform noise on a
DC offset and every cascade starts with a 20 Hz high-pass at 192 kHz, so every carried state t_j is far from zero and the
outputs of chunks >= 1 are wrong at once if one element of one t_j is: the states buffer has no hook of its own."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import filter_model as M
import loudness_model as LM
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 192000
LENGTHS = [1, 511, 512, 513, 1024, 32767, 32768, 32769, 66049]
STAGES = [1, 2, 3, 8]
TAILS = [0, 1, 700]
CLIP_LEN = 66049 + 40
SRC = {1: 1, 2: 2}                                              # channels -> clip id
DST = 100
bits = BU.bits
K8 = M.eight_stages(RATE)                                       # stage 0: the 20 Hz high-pass


def source(channels, n=CLIP_LEN, seed=0xF117):
    rng = np.random.default_rng(seed + channels)
    return [(rng.uniform(-0.5, 0.5, n) + 0.25 * (1 - 2 * k)).astype(np.float32) for k in range(channels)]


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


# ---- 1: lengths x channels x stage counts ---------------------------------------------------------------------------------------
def split(total, i):
    """`total` = n + tail: the tails 0, 1 and 700 in turn where they fit; `first` 0, or a few frames in"""
    tail = [t for t in TAILS if t < total][i % len([t for t in TAILS if t < total])]
    return total - tail, tail, (0, 7, 33)[i % 3] if total + 33 <= CLIP_LEN else 0


CASES = [(total, ch, S) + split(total, li + si + ch) for li, total in enumerate(LENGTHS) for ch in (1, 2) for si, S in enumerate(STAGES)]
assert {c[4] for c in CASES} == set(TAILS) and {c[5] for c in CASES} == {0, 7, 33}
assert {(c[0], c[4]) for c in CASES} >= {(513, 1), (1024, 700), (32769, 700), (66049, 0)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_filter_matrix(ctx, case):
    total, ch, S, n, tail, first = case
    k = K8[:S]
    want = M.filter_clip(ctx.src[ch], first, n, tail, k)
    st = ctx.clip_filter(SRC[ch], DST, first, n, k, tail_frames=tail, stats_channels=ch)
    got = download(ctx, DST, ch, total)
    assert first_bad(got, want) is None, first_bad(got, want)
    if total > M.CHUNK:                                         # the carry is no formality here
        assert np.max(np.abs(M.filter_plane(ctx.src[ch][0], first, n, tail, k, states=True)[1][1:])) > 1e-3
    check_stats(st, FX.measure(want), total, "stats_of_result")
    check_stats(ctx.clip_measure(DST, ch, 0, total), FX.measure(want), total, "wbx_clip_measure of the result")


@pytest.mark.parametrize("S", [4, 5, 6, 7])
def test_the_remaining_stage_counts(ctx, S):
    """every compiled instance runs once: stereo and mono, two chunks and a frame"""
    for ch in (1, 2):
        want = M.filter_clip(ctx.src[ch], 3, 1000, 25, K8[:S])
        ctx.clip_filter(SRC[ch], DST, 3, 1000, K8[:S], tail_frames=25)
        assert first_bad(download(ctx, DST, ch, 1025), want) is None, (S, ch)


# ---- 2: what lies beside the range, what is not finite inside it ---------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_frames_beside_the_range_do_not_count(ctx, channels):
    """loud samples and NaNs in front of and behind the range; the range ends on the clip's last frame in the second call"""
    n_clip = 3000
    planes = source(channels, n_clip, seed=0xBE51DE)
    for p in planes:
        p[:200], p[190:200], p[2700:] = 1e30, np.nan, -1e30
        p[2710:2720] = np.nan
    ctx.clip_upload(50, "f32", RATE, planes)
    k = K8[:3]
    for first, n, tail in ((200, 2500, 700), (200, 2500, 0), (200, 1, 0)):
        quiet = [p[first:first + n].copy() for p in planes]
        want = M.filter_clip(quiet, 0, n, tail, k)
        assert np.all(np.isfinite(np.stack(want)))
        ctx.clip_filter(50, DST, first, n, k, tail_frames=tail)
        assert first_bad(download(ctx, DST, channels, n + tail), want) is None, (first, n, tail)
    clean = source(channels, n_clip, seed=0xBE51DE)
    ctx.clip_upload(50, "f32", RATE, clean)
    for first, n, tail in ((n_clip - 1300, 1300, 0), (n_clip - 1300, 1300, 700), (n_clip - 1, 1, 3), (0, n_clip, 1)):
        want = M.filter_clip(clean, first, n, tail, k)
        ctx.clip_filter(50, DST, first, n, k, tail_frames=tail)
        assert first_bad(download(ctx, DST, channels, n + tail), want) is None, ("to the clip's last frame", first, n, tail)


@pytest.mark.parametrize("channels", [1, 2])
def test_samples_that_are_not_finite_enter_as_zero(ctx, channels):
    n = 1600
    planes = source(channels, n, seed=0x0FF)
    zeroed = [p.copy() for p in planes]
    for c, (p, z) in enumerate(zip(planes, zeroed)):
        at = np.array([5, 300, 511, 512, 513, 1100, 1599]) - c
        p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
        z[at] = 0.0
    planes[0].view(np.uint32)[40] = 0xFFC12345                  # a NaN with a payload and a sign
    zeroed[0][40] = 0.0
    ctx.clip_upload(51, "f32", RATE, planes)
    k = K8[:2]
    want = M.filter_clip(planes, 0, n, 10, k)
    assert first_bad(want, M.filter_clip(zeroed, 0, n, 10, k)) is None and np.all(np.isfinite(np.stack(want)))
    ctx.clip_filter(51, DST, 0, n, k, tail_frames=10)
    assert first_bad(download(ctx, DST, channels, n + 10), want) is None


def test_results_that_overflow_fp32(ctx):
    """a huge input through a +12 dB peak: fp64 holds it, fp32 stores +-inf; -0.0 in, +0.0 out (a stage adds to +0.0)"""
    n = 1200
    x = (source(1, n, seed=0xB16)[0].astype(np.float64) * 4e38).astype(np.float32)   # up to 3e38
    x[:3] = -0.0
    ctx.clip_upload(52, "f32", 48000, [x])
    k = np.stack([M.design(48000, "peak", 1000.0, 2.0, 4.0), M.design(48000, "highshelf", 8000.0, 0.7, 4.0)])
    want = M.filter_clip([x], 0, n, 0, k)
    assert np.isinf(want[0]).any() and not np.isnan(want[0]).any() and want[0].view(np.uint32)[0] == 0
    ctx.clip_filter(52, DST, 0, n, k)
    assert first_bad(download(ctx, DST, 1, n), want) is None


def test_phase_times_of_the_last_filter():
    c = W.MixContext(4, block=128)
    out = np.full(3, 7.0)
    assert c.L.wbx_filter_phase_ms(c.h, out.ctypes.data) == -4 and np.all(out == 7.0)     # no filter yet
    c.clip_upload(1, "f32", RATE, source(1, 5000))
    assert c.L.wbx_filter_phase_ms(c.h, None) == -4
    c.clip_filter(1, 2, 0, 5000, K8[:2])
    state, carry, apply = c.filter_phase_ms()
    assert state > 0.0 and carry > 0.0 and apply > 0.0
    c.clip_filter(1, 2, 0, 512, K8[:2])                         # one chunk: nothing is carried
    state, carry, apply = c.filter_phase_ms()
    assert state == 0.0 and carry == 0.0 and apply > 0.0
    c.close()


# ---- 3: the pool -------------------------------------------------------------------------------------------------------------------
def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes = source(2, 5000)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    k = K8[:2]
    c.clip_filter(1, 10, 0, 4000, k, tail_frames=96)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        c.clip_filter(1, 10, first, 4000, k, tail_frames=96)
        assert c.pool_stats() == with_one
        assert first_bad(download(c, 10, 2, 4096), M.filter_clip(planes, first, 4000, 96, k)) is None
    c.clip_filter(1, 10, 0, 700, k)                             # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert first_bad(download(c, 10, 2, 700), M.filter_clip(planes, 0, 700, 0, k)) is None
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    k = np.ascontiguousarray(K8[:2])
    ctx.clip_filter(SRC[2], DST, 0, 64, k)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    st = _ffi.ClipStats()

    def refused(status, src, dst, first, n, tail, coef, stages):
        before = ctx.pool_stats()
        got = L.wbx_clip_filter(ctx.h, src, dst, first, n, tail, coef.ctypes.data if coef is not None else None, stages, C.byref(st))
        assert got == status, (got, status, src, dst, first, n, tail, stages, L.wbx_last_error(ctx.h))
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept

    refused(-4, 999, DST, 0, 64, 0, k, 2)                       # unknown source
    refused(-4, SRC[2], DST, 0, 0, 0, k, 2)                     # no frames
    refused(-4, SRC[2], DST, 0, 0, 64, k, 2)                    # ... even with a tail
    refused(-4, SRC[2], DST, CLIP_LEN - 10, 11, 0, k, 2)        # past the clip
    refused(-4, SRC[2], DST, CLIP_LEN + 1, 1, 0, k, 2)
    refused(-4, DST, DST, 0, 8, 0, k, 2)                        # dst == src
    refused(-4, SRC[2], DST, 0, 64, 0, None, 2)                 # NULL coef
    refused(-4, SRC[2], DST, 0, 64, 0, k, 0)                    # stage counts
    refused(-4, SRC[2], DST, 0, 64, 0, np.tile(k[0], 9), 9)
    for i, v in ((4, 1.0), (3, 2.5), (0, np.nan), (2, np.inf)):  # on the triangle's edge, outside it, not finite
        bad = k.copy()
        bad[1, i] = v
        refused(-4, SRC[2], DST, 0, 64, 0, bad, 2)
    refused(-4, SRC[2], DST, 0, 64, (1 << 31) - 16 - 64, k, 2)  # n + tail == 2^31 - 16
    refused(-4, SRC[2], DST, 0, 64, (1 << 64) - 32, k, 2)       # ... and a sum that wraps
    refused(-3, 60, DST, 0, 64, 0, k, 2)                        # not F32 (a clip of more than 2 channels cannot exist in the pool)


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    planes = source(2, n)
    c.clip_upload(1, "f32", 48000, planes)                      # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_filter(1, 10 + len(made), 0, n, K8[:1], tail_frames=n)       # 16 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 4: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_filter_sample_of_an_upload_a_take_a_bounce_and_a_filter_result():
    spec = synth.make_session("filt2", 3, n_blocks=6, block=128, seed=0xF117E2)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    k = np.stack([M.design(rate, "highpass", 20.0), M.design(rate, "peak", 2500.0, 3.0, 2.0), M.design(rate, "lowshelf", 200.0, 0.7, 0.5)])
    # a bounce of track 1, pre-fader
    lo, hi = BU.bounce_range(spec, 5)
    ids, nb = eng.bounce(lo, hi, [("track", 1, "pre")])
    stem = [np.ascontiguousarray(p) for p in eng.bounce_download(ids[0], nb)]
    assert np.any(np.stack(stem) != 0.0)
    # a take on track 0
    eng.set_audio_channel_config(2, spec.channels, spec.block, rate)
    eng.set_track_input(0, "external_mono", 0, True)
    x = source(1, 5 * spec.block, seed=0x7A4E)[0]
    inp, out = W.AudioBuffer(spec.block, 2), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for b in range(5):
        inp.channel_buffers[0][:] = x[b * spec.block:(b + 1) * spec.block]
        inp.channel_buffers[1][:] = 0.0
        eng.process(inp, out, float(rate))
    frames = eng.record_info(0)["frames"]
    eng.stop_record()
    eng.stop()
    eng.set_playhead_position(0.0)
    take = max(c[5] for c in eng.clips(eng.tracks[0]))
    assert frames == len(x) and first_bad(download(eng.ctx, take, 1, frames), [x]) is None
    # an upload
    NU = 3 * LM.hop_frames(rate)                                # three hops of the loudness meter
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)

    f_up = eng.filter_sample(up, k, tail_frames=300, first_frame=4, n_frames=NU - 300)
    want_up = M.filter_clip(planes, 4, NU - 300, 300, k)
    assert eng._sample_shape[f_up] == (NU, 2)
    assert first_bad(download(eng.ctx, f_up, 2, NU), want_up) is None
    f_take = eng.filter_sample(take, k[:1], tail_frames=0, frames=frames, channels=1)
    assert first_bad(download(eng.ctx, f_take, 1, frames), M.filter_clip([x], 0, frames, 0, k[:1])) is None
    f_stem = eng.filter_sample(ids[0], k, tail_frames=64)
    assert first_bad(download(eng.ctx, f_stem, spec.channels, nb + 64), M.filter_clip(stem, 0, nb, 64, k)) is None
    again = eng.filter_sample(f_up, k[1:], tail_frames=5)       # of an earlier result
    assert first_bad(download(eng.ctx, again, 2, NU + 5), M.filter_clip(want_up, 0, NU, 5, k[1:])) is None

    # the filtered upload on a track, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "filtered", 0.5 * unit, 5.5 * unit, 0.0, f_up, 1.0, 1.0)
    assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, want_up, rate), 1.0, 1.0) == 0
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
    got, _ = eng.export_sample(f_up, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want_up, axis=1).reshape(-1).view(np.uint32))
    _, E = eng.loudness_sample(f_up, energies=True, rate=rate)
    want_E = LM.hop_energies(want_up, 0, NU, rate)
    assert E.shape == want_E.shape == (2, 3) and np.array_equal(E.view(np.uint64), want_E.view(np.uint64))
    with pytest.raises(W.WbxError):
        eng.delete_sample(f_up)                                 # a clip names it
    eng.delete_sample(again)
    # refusals create no sample
    L, new = W.lib(), C.c_uint32(12345)
    before = eng.ctx.pool_stats()
    kk = np.ascontiguousarray(k)
    assert L.wbx_engine_filter_sample(eng.h, 9999, 0, 8, 0, kk.ctypes.data, 3, C.byref(new)) == -4
    assert L.wbx_engine_filter_sample(eng.h, again, 0, 8, 0, kk.ctypes.data, 3, C.byref(new)) == -4        # deleted
    assert L.wbx_engine_filter_sample(eng.h, up, 0, NU + 9, 0, kk.ctypes.data, 3, C.byref(new)) == -4
    assert L.wbx_engine_filter_sample(eng.h, up, 0, 8, 0, None, 3, C.byref(new)) == -4
    assert L.wbx_engine_filter_sample(eng.h, up, 0, 8, 0, kk.ctypes.data, 9, C.byref(new)) == -4
    assert L.wbx_engine_filter_sample(eng.h, up, 0, 8, 0, kk.ctypes.data, 3, None) == -4
    assert new.value == 12345 and eng.ctx.pool_stats() == before
    eng.close()
    e.close()


def test_cpp_adapter_filters_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take, designs a two-stage cascade with wbx_filter_design and
    calls wbx::Engine::filter_sample; the result equals the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_filter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_filter.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "filtered.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n, tail = 5 * 512, 100
    assert "adapter filter ok %d" % (n + tail) in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    k = np.stack([M.design(48000, "highpass", 20.0), M.design(48000, "peak", 1000.0, 8.0, 4.0)])
    want = M.filter_clip([x], 0, n, tail, k)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n + tail and first_bad([got], want) is None


# ---- 5: beside the audio thread -------------------------------------------------------------------------------------------------
def test_filters_beside_the_audio_thread():
    """The shape of the loudness test (test_gpu_loudness.py): a clip far behind the played range names the big sample while
    the threads run, so a delete of it can never succeed — between two filters it is refused for the clip (-4), inside one
    for the pin (-3, asked first) — one thread deletes without pause while the other filters until a refusal for the pin
    has been seen.  The master is what it is without the filters."""
    NB, FR, WAIT, CALLS = 300, 1 << 20, 60.0, 64
    spec = synth.make_session("filtthr", 2, n_blocks=NB, block=128, seed=0xF11712)
    planes = source(2, FR, seed=35)
    k = M.four_stages(44100)

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
    first, n, tail = 5, FR - 8, 100
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), threading.Event()
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        while not finished.is_set() and time.monotonic() < end:
            st = L.wbx_engine_delete_sample(eng.h, big)
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"] = eng.filter_sample(big, k, tail_frames=tail, first_frame=first, n_frames=n, channels=2)
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
    print("filter calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every filter read a live source: the result is the model's, bit for bit
    got = download(eng.ctx, results["big"], 2, n + tail)
    assert first_bad(got, M.filter_clip(planes, first, n, tail, k)) is None
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    new = C.c_uint32(12345)
    kk = np.ascontiguousarray(k)
    assert L.wbx_engine_filter_sample(eng.h, big, 0, 8, 0, kk.ctypes.data, 4, C.byref(new)) == -4 and new.value == 12345
    eng.close()
