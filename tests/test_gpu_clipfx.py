"""wbx_clip_measure / wbx_clip_derive and their engine forms on the device.  Derived clips come back through
wbx_clip_download and are compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/clipfx_model.py; every
statistic but sum / sum_sq is exact; those two are held to the derived bound of any-order fp64 summation.  Shapes are the
smallest at which the kernel can still go wrong: a lane owns 8 frames, a wave 512, a workgroup 2048."""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as M
import oracle_ffi as O
import second_pass as SP
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 9, 511, 513, 1000, 5003]
GAINS = [1.0, -1.0, 0.5, float(np.array([0x3F353BEF], dtype=np.uint32).view(np.float32)[0])]
DST = 100
bits = BU.bits


def clip_id(channels, length):
    return 1 + LENGTHS.index(length) + (len(LENGTHS) if channels == 2 else 0)


def source(channels, length):
    rng = np.random.default_rng(0xC11F + 31 * length + channels)
    return [rng.uniform(-1.4, 1.4, length).astype(np.float32) for _ in range(channels)]


def derive_cases():
    """a sparse draw over the axes of the issue's matrix; the asserts below are the coverage it asks for"""
    rng = np.random.default_rng(0xFADE)
    out = []
    for ch in (1, 2):
        for L in LENGTHS:
            firsts = [0] if L < 9 else [0, 1, 5] + ([11] if L >= 511 else []) + ([2, 4, 6, 7, 8 * 37 + 3] if L >= 1000 else [])
            for first in firsts:
                for rev in (0, 1):
                    rem = L - first
                    n = int(rng.choice(sorted({rem, 1, max(1, rem // 8 * 8), max(1, rem - 3), max(1, rem // 2)})))
                    fades = [(0, 0), (1, 0), (0, 1), (min(9, n), min(9, n)), (n, 0), (0, n), (n, n), (max(1, 2 * n // 3),) * 2]
                    fi, fo = fades[int(rng.integers(len(fades)))]
                    out.append((ch, L, first, n, rev, int(rng.choice(M.MODES_FOR[ch])), int(rng.integers(4)), fi, fo,
                                int(rng.integers(3)), int(rng.integers(3))))
    seen = lambda i: {c[i] for c in out}
    assert seen(1) == set(LENGTHS) and {0, 1, 5} <= seen(2) and seen(6) == {0, 1, 2, 3} and seen(9) == seen(10) == {0, 1, 2}
    assert {(c[4], c[2] % 8) for c in out} == {(r, m) for r in (0, 1) for m in range(8)}
    assert {(c[0], c[5]) for c in out} == {(ch, m) for ch in (1, 2) for m in M.MODES_FOR[ch]}
    assert any(c[3] == 1 for c in out) and any(c[3] % 8 == 0 for c in out) and any(c[3] % 8 for c in out)
    assert {0, 1, 9} <= seen(7) and any(c[7] == c[3] for c in out) and any(c[7] + c[8] > c[3] for c in out)   # n-frame and overlapping fades
    return out


CASES = derive_cases()


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {}
    for ch in (1, 2):
        for L in LENGTHS:
            c.src[(ch, L)] = source(ch, L)
            c.clip_upload(clip_id(ch, L), "f32", 44100, c.src[(ch, L)])
    yield c
    c.close()


def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def check_stats(got, want, n, where):
    assert M.exact_fields_equal(got, want), (where, got, {k: want[k] for k in M.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if math.isfinite(a):
                print(where, k, "error", abs(g - w), "bound", n * 2.0 ** -52 * a)
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


# ---- 1: the parameter matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_derive_matrix(ctx, case):
    ch, L, first, n, rev, mode, g, fi, fo, si, so = case
    want = M.derive(ctx.src[(ch, L)], first, n, bool(rev), mode, GAINS[g], fi, fo, si, so)
    d = W.edit_desc(first, n, bool(rev), mode, GAINS[g], fi, fo, si, so)
    st = ctx.clip_derive(clip_id(ch, L), DST, d, stats_channels=len(want))
    got = download(ctx, DST, len(want), n)
    assert bits(np.stack(got)).tolist() == bits(np.stack(want)).tolist()
    check_stats(st, M.measure(want), n, "stats_of_result")
    check_stats(ctx.clip_measure(DST, len(want), 0, n), M.measure(want), n, "measure of the result")
    src = ctx.src[(ch, L)]
    check_stats(ctx.clip_measure(clip_id(ch, L), ch, first, n), M.measure(src, first, n), n, "measure of the source range")


# ---- 2: every workgroup and wave seam of one pass of the grid (513 workgroups; the second pass is section 2b's) ---------------
@pytest.fixture(scope="module")
def big():
    c = W.MixContext(4, block=128)
    n = SP.CLIPFX_SEAMS_FRAMES
    rng = np.random.default_rng(0x5EA5)
    c.planes = [rng.uniform(-1.1, 1.1, n).astype(np.float32) for _ in range(2)]
    c.clip_upload(1, "f32", 48000, c.planes)
    yield c, n
    c.close()


@pytest.mark.parametrize("rev", [False, True])
def test_workgroup_and_wave_seams(big, rev):
    c, n = big
    fi, fo = 300001, 700003                      # overlapping, ending inside waves
    want = M.derive(c.planes, 0, n, rev, M.KEEP, 0.5, fi, fo, M.SMOOTH, M.SQUARE)
    st = c.clip_derive(1, 2, W.edit_desc(0, n, rev, "keep", 0.5, fi, fo, "smooth", "square"), stats_channels=2)
    got = download(c, 2, 2, n)
    for k in range(2):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, (k, bad[:8], bad.size)
    check_stats(st, M.measure(want), n, "big stats_of_result")
    check_stats(c.clip_measure(1, 2, 5, n - 5), M.measure(c.planes, 5, n - 5), n - 5, "big measure")


# ---- 2b: the second pass of the grid ----------------------------------------------------------------------------------------
# n = one pass of the grid + 1037 frames (tests/second_pass.py, from wbx_clipfx_pass_frames): the first three workgroups run
# the loop a second time, the range ends inside a wave of that pass and its last lane holds 5 frames.  Every frame and every
# statistic is compared, so lane statistics that are reset or mis-merged between the iterations show, as does a skipped tile:
# the pool hands the space of the clip freed last out again (shifted by the few granules of its pseudo-random gap), and that
# clip was filled by a call with another gain and the other direction; no two cases share first_frame, direction and mode.
HUGE_SRC, HUGE_MONO, HUGE_SPOIL, HUGE_DST = 1, 2, 3, 4
HUGE_SLACK = 8                                                  # frames of the source clip behind a range that starts at 0


def huge_material(n):
    """stereo, n + 8 frames.  In the coordinates of the range measured below (first_frame 5), P the frames of one pass:
    channel 0's peak magnitude 3.5 at frame 995 and again, as -3.5, at P + 600: the first is reported, the signed maximum
    lies before P and the minimum behind it; channel 1's peak, -3.25, lies only behind P (its minimum; its maximum 2.0 before);
    NaNs and over-range samples on both sides"""
    P = W.clipfx_pass_frames()
    rng = np.random.default_rng(0x2FA55)
    x = [rng.uniform(-0.9, 0.9, n + HUGE_SLACK).astype(np.float32) for _ in range(2)]
    x[0][[1000, P + 605]] = [3.5, -3.5]
    x[1][[4005, P + 782]] = [2.0, -3.25]
    for k in range(2):
        x[k][[77 + k, 300_000 + k, P + 905 + k, n - 2 - k]] = np.nan
        x[k][[500 + k, P - 3 + k, P + 9 + k, P + 1030 + k]] = [1.5, -1.25, 1.75, -1.5]
    return x


@pytest.fixture(scope="module")
def huge():
    c = W.MixContext(4, block=128)
    n = SP.clipfx_frames()
    assert n > W.clipfx_pass_frames()
    c.planes = huge_material(n)
    c.clip_upload(HUGE_SRC, "f32", 48000, c.planes)
    c.clip_upload(HUGE_MONO, "f32", 48000, c.planes[:1])
    yield c, n
    c.close()


def huge_cases(n, P):
    a, b = (P + 300, 700), (300_001, 1037 + 1500)                # the fade layouts: (fade_in, fade_out)
    return [  # (source channels, first_frame, reversed, mode, fades)
        (2, 0, False, "keep", a), (2, 0, True, "keep", a),      # the fade-in ends inside the second pass, the fade-out lies in it
        (2, 5, False, "keep", b), (2, 3, True, "keep", b),      # the fade-out starts before the seam
        (2, 5, True, "keep", a), (2, 8, True, "keep", b),
        (2, 3, False, "mono_mix", a), (1, 0, True, "dual_mono", b), (2, 8, False, "swap", b)]


@pytest.mark.parametrize("i", range(9))
def test_derive_across_the_second_pass_of_the_grid(huge, i):
    """Reversed at first_frame 0 the range's last lane — it runs in the second pass — has top = 4 < 7 and loads its frames one
    by one, each guarded; at 3 it has top = 7, the first unguarded span, which starts at the clip's frame 0"""
    c, n = huge
    P = W.clipfx_pass_frames()
    cases = huge_cases(n, P)
    assert len(cases) == 9 and {(k[1], k[2]) for k in cases} >= {(f, True) for f in (0, 3, 5, 8)}
    assert [k[2] for k in cases[6:]] == [False, True, False] and n - cases[0][4][0] > 0 and cases[2][4][1] > 1037
    ch, first, rev, mode, (fi, fo) = cases[i]
    src, planes = (HUGE_SRC, c.planes) if ch == 2 else (HUGE_MONO, c.planes[:1])
    want = M.derive(planes, first, n, rev, _ffi.CH_MODE[mode], 0.5, fi, fo, M.SMOOTH, M.SQUARE)
    c.clip_derive(src, HUGE_SPOIL, W.edit_desc(first, n, not rev, mode, -0.25))     # fills the space the result is about to get
    assert c.L.wbx_clip_free(c.h, HUGE_SPOIL) == 0
    st = c.clip_derive(src, HUGE_DST, W.edit_desc(first, n, rev, mode, 0.5, fi, fo, "smooth", "square"), stats_channels=len(want))
    got = download(c, HUGE_DST, len(want), n)
    assert c.L.wbx_clip_free(c.h, HUGE_DST) == 0
    for k in range(len(want)):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, (cases[i], k, bad[:8], bad.size)
    check_stats(st, M.measure(want), n, "second pass stats_of_result")


@pytest.mark.parametrize("channels", [2, 1])
def test_measure_across_the_second_pass_of_the_grid(huge, channels):
    c, n = huge
    P = W.clipfx_pass_frames()
    first, m = 5, n - 5
    assert m > P
    planes = c.planes[:channels]
    want = M.measure(planes, first, m)
    got = c.clip_measure(HUGE_SRC if channels == 2 else HUGE_MONO, channels, first, m)
    # the material is what the docstring of huge_material says it is
    assert want["peak"][0] == 3.5 and want["peak_frame"][0] == 995 and planes[0][first + P + 600] == -3.5
    assert want["min"][0] == -3.5 and want["max"][0] == 3.5
    if channels == 2:
        assert want["peak"][1] == 3.25 and want["peak_frame"][1] == P + 777 and want["min"][1] == -3.25 and want["max"][1] == 2.0
    for p in planes:
        r = p[first:first + m]
        with np.errstate(invalid="ignore"):
            assert np.isnan(r[:P]).any() and np.isnan(r[P:]).any() and (np.abs(r[:P]) > 1).any() and (np.abs(r[P:]) > 1).any()
    check_stats(got, want, m, "second pass measure")
    assert got["peak_frame"][0] == 995


# ---- 3: special values ------------------------------------------------------------------------------------------------------
SPECIALS =np.array([np.inf, -np.inf, np.nan, -0.0, 1e-40, -1.4e-45, 0.0], dtype=np.float32)


@pytest.mark.parametrize("rot", range(len(SPECIALS)))
@pytest.mark.parametrize("channels", [1, 2])
def test_special_values(ctx, channels, rot):
    L = 1000
    planes = [p.copy() for p in source(channels, L)]
    at = [0, 7, 8, L - 1]
    for k, p in enumerate(planes):
        p[at] = np.roll(SPECIALS, rot + 3 * k)[:4]
    if rot % 2:
        planes[0].view(np.uint32)[13] = 0xFFC12345                 # a NaN with a payload and a sign
    ctx.clip_upload(50, "f32", 48000, planes)
    check_stats(ctx.clip_measure(50, channels, 0, L), M.measure(planes), L, "specials")
    for rev in (False, True):
        for mode in M.MODES_FOR[channels]:
            kw = dict(reverse=rev, mode=mode, gain=GAINS[rot % 4], fade_in=9, fade_out=L, shape_in=rot % 3, shape_out=(rot + 1) % 3)
            want = M.derive(planes, 0, L, **kw)
            st = ctx.clip_derive(50, DST, W.edit_desc(0, L, rev, mode, kw["gain"], 9, L, kw["shape_in"], kw["shape_out"]),
                                 stats_channels=len(want))
            got = download(ctx, DST, len(want), L)
            assert bits(np.stack(got)).tolist() == bits(np.stack(want)).tolist(), (rev, mode)
            check_stats(st, M.measure(want), L, "specials derived")


def test_a_peak_attained_twice_reports_its_first_frame(ctx):
    x = source(1, 5003)[0].copy()
    x[[77, 2048 + 5, 4999]] = [-3.5, 3.5, -3.5]
    y = np.zeros(513, dtype=np.float32)
    y[[0, 512]] = [-0.0, 0.0]
    ctx.clip_upload(51, "f32", 48000, [x, x[::-1].copy()])
    st = ctx.clip_measure(51, 2, 0, 5003)
    assert st["peak"] == [3.5, 3.5] and st["peak_frame"] == [77, 3] and st["min"] == [-3.5, -3.5] and st["max"] == [3.5, 3.5]
    st = ctx.clip_measure(51, 2, 78, 4000)
    assert st["peak_frame"] == [2048 + 5 - 78, (5002 - 2053) - 78]
    check_stats(st, M.measure([x, x[::-1]], 78, 4000), 4000, "twice")
    ctx.clip_upload(52, "f32", 48000, [y])
    st = ctx.clip_measure(52, 1, 0, 513)
    assert st["peak"] == [0.0] and st["peak_frame"] == [0]
    assert [np.float32(st[k][0]).tobytes() for k in ("min", "max")] == [np.float32(-0.0).tobytes(), np.float32(0.0).tobytes()]


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    s2, s1 = clip_id(2, 1000), clip_id(1, 1000)
    ctx.clip_derive(s2, DST, W.edit_desc(0, 64))
    ctx.clip_upload(60, "i16", 48000, [np.arange(64, dtype=np.int16)] * 2)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    st = _ffi.ClipStats()

    def refused(status, src, dst, desc):
        before = ctx.pool_stats()
        got = L.wbx_clip_derive(ctx.h, src, dst, C.byref(desc) if desc is not None else None, C.byref(st))
        assert got == status, (got, status, src, dst)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept

    ok = dict(first_frame=0, n_frames=64)
    refused(-4, 999, DST, W.edit_desc(**ok))                                 # unknown source
    refused(-4, s2, DST, W.edit_desc(0, 0))                                  # no frames
    refused(-4, s2, DST, W.edit_desc(990, 11))                               # past the clip
    refused(-4, s2, DST, W.edit_desc(1001, 1))
    refused(-4, DST, DST, W.edit_desc(**ok))                                 # dst == src
    refused(-4, s2, DST, W.edit_desc(**ok, flags=2))                         # unknown flag
    refused(-4, s2, DST, W.edit_desc(**ok, channel_mode=6))
    refused(-4, s2, DST, W.edit_desc(**ok, channel_mode=-1))
    refused(-4, s2, DST, W.edit_desc(**ok, fade_in_shape=3))
    refused(-4, s2, DST, W.edit_desc(**ok, fade_out_shape=-1))
    refused(-4, s2, DST, W.edit_desc(**ok, fade_in=65))                      # a fade longer than the range
    refused(-4, s2, DST, W.edit_desc(**ok, fade_out=65))
    refused(-4, s2, DST, None)                                               # NULL descriptor
    refused(-4, s2, DST, W.edit_desc(**ok, channel_mode="dual_mono"))        # modes that do not fit
    for mode in ("swap", "left", "right", "mono_mix"):
        refused(-4, s1, DST, W.edit_desc(**ok, channel_mode=mode))
    refused(-3, 60, DST, W.edit_desc(**ok))                                  # not F32
    assert L.wbx_clip_measure(ctx.h, 60, 0, 8, C.byref(st)) == -3 and L.wbx_clip_measure(ctx.h, s2, 0, 0, C.byref(st)) == -4
    assert L.wbx_clip_measure(ctx.h, s2, 999, 2, C.byref(st)) == -4 and L.wbx_clip_measure(ctx.h, 999, 0, 8, C.byref(st)) == -4
    assert L.wbx_clip_measure(ctx.h, s2, 0, 8, None) == -4


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    rng = np.random.default_rng(5)
    planes = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(2)]
    c.clip_upload(1, "f32", 48000, planes)           # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_derive(1, 10 + len(made), W.edit_desc(0, n, reverse=True))
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    got = download(c, made[-1], 2, n)
    assert all(np.array_equal(g.view(np.uint32), p[::-1].view(np.uint32)) for g, p in zip(got, planes))
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 5: through the engine -----------------------------------------------------------------------------------------------------
def play_both(eng, e, n_blocks):
    e.play()
    eng.play()
    eng.render(n_blocks)
    m, _, _ = eng.ctx.fetch()
    for b in range(n_blocks):
        om, _ = e.process()
        assert np.array_equal(bits(m[b]), bits(om)), b


def replace_track(eng, e, spec, t, sample, osample, lo, hi):
    while e.clips(t):
        e.delete_clip(t, 0)
    while eng.clips(eng.tracks[t]):
        eng.delete_clip(eng.tracks[t], 0)
    assert e.add_audio_clip(t, lo, hi, 0.0, osample, 1.0, 1.0) == 0
    eng.add_audio_clip(eng.tracks[t], "edited", lo, hi, 0.0, sample, 1.0, 1.0)


def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_a_take_normalized_trimmed_and_faded_plays_as_the_models_clip():
    spec = synth.make_session("fxtake", 3, n_blocks=6, block=128, seed=0xF17A4E)
    eng = build_engine(spec, max_blocks=8)
    eng.set_audio_channel_config(1, spec.channels, spec.block, spec.sample_rate)
    eng.set_track_input(1, "external_mono", 0, True)
    x = np.random.default_rng(17).uniform(-0.3, 0.3, 3 * spec.block).astype(np.float32)
    inp, out = W.AudioBuffer(spec.block, 1), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for b in range(3):
        inp.channel_buffers[0][:] = x[b * spec.block:(b + 1) * spec.block]
        eng.process(inp, out, float(spec.sample_rate))
    frames = eng.record_info(1)["frames"]
    eng.stop_record()
    eng.stop()
    eng.set_playhead_position(0.0)
    assert frames == len(x)
    take = max(c[5] for c in eng.clips(eng.tracks[1]))
    st = eng.measure_sample(take, channels=1, frames=frames)
    want_st = M.measure([x])
    check_stats(st, want_st, frames, "take")
    loud, gain = eng.normalize_sample(take, 0.5, channels=1, frames=frames)
    assert np.float32(gain) == M.normalize_gain(0.5, want_st["peak"][0])
    normal = M.derive([x], 0, frames, gain=np.float32(gain))
    assert abs(float(M.measure(normal)["peak"][0]) - 0.5) <= float(np.spacing(np.float32(0.5)))
    d = dict(first=40, n=300, reverse=False, mode=M.DUAL_MONO, gain=1.0, fade_in=64, fade_out=200, shape_in=M.SMOOTH, shape_out=M.SQUARE)
    model = M.derive(normal, **d)
    edited = eng.derive_sample(loud, W.edit_desc(40, 300, False, "dual_mono", 1.0, 64, 200, "smooth", "square"))
    assert bits(np.stack(download(eng.ctx, edited, 2, 300))).tolist() == bits(np.stack(model)).tolist()
    # the session the oracle plays: the same tracks, track 2 holding the MODEL's clip uploaded from the host
    e = O.build_oracle_engine(spec)
    while eng.clips(eng.tracks[1]):
        eng.delete_clip(eng.tracks[1], 0)
    while e.clips(1):
        e.delete_clip(1, 0)
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    replace_track(eng, e, spec, 2, edited, oracle_sample(e, model, spec.sample_rate), 0.5 * unit, 4.5 * unit)
    play_both(eng, e, 6)
    # the new samples are ordinary ones: exportable, deletable once no clip names them
    got, _ = eng.export_sample(edited, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(model, axis=1).reshape(-1).view(np.uint32))
    with pytest.raises(W.WbxError):
        eng.delete_sample(edited)
    eng.delete_sample(loud)
    with pytest.raises(W.WbxError) as ex:
        eng.normalize_sample(edited, 0.5, first_frame=0, n_frames=1)    # the fade-in's first frame: silent
    assert ex.value.status == -4
    eng.close()
    e.close()


def test_a_pre_fader_bounce_put_back_as_one_derived_clip():
    spec = synth.make_session("fxfreeze", 6, src_rate=44100, seek=True, n_blocks=10, seed=0xF1B0C5)
    t = 3
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    lo, hi = 0.0, 10 * unit
    e = O.build_oracle_engine(spec)
    tw = O.build_oracle_engine(BU.unity_twin(spec))
    n, _, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    _, pre, _, _ = BU.oracle_sequence(tw, spec, lo, hi)
    eng = build_engine(spec, max_blocks=8, group_size=spec.n_tracks)
    (stem,), frames = eng.bounce(lo, hi, [("track", t, "pre")])
    first, m = 13, n - 13 - 29
    model = M.derive([np.ascontiguousarray(pre[t][c]) for c in range(spec.channels)], first, m, True, M.SWAP, -1.0, 500, m, M.LINEAR, M.SMOOTH)
    edited = eng.derive_sample(stem, W.edit_desc(first, m, True, "swap", -1.0, 500, m, "linear", "smooth"))
    assert bits(np.stack(download(eng.ctx, edited, 2, m))).tolist() == bits(np.stack(model)).tolist()
    replace_track(eng, e, spec, t, edited, oracle_sample(e, model, spec.sample_rate), lo, hi)
    play_both(eng, e, 8)
    eng.close()
    e.close()
    tw.close()


def test_the_padding_behind_a_derived_clip_is_zero():
    """the extent of a freed clip of ones is handed to the result (first fit); played at 44.1 kHz in a 48 kHz session the
    interpolation window reads past the clip's last frame, into the padding: the render equals the oracle's, whose sample
    has 16 zero frames there"""
    spec = synth.make_session("fxpad", 2, n_blocks=4, block=128, seed=0xF1FAD)
    eng = build_engine(spec, max_blocks=4)
    e = O.build_oracle_engine(spec)
    n = 331
    rng = np.random.default_rng(23)
    planes = [rng.uniform(-0.9, 0.9, n + 40).astype(np.float32) for _ in range(2)]
    src = eng.add_sample("f32", 44100, planes)
    junk = eng.add_sample("f32", 44100, [np.full(n + 16, 1.0, dtype=np.float32)] * 2)
    live = eng.ctx.pool_stats()[2]
    eng.delete_sample(junk)
    edited = eng.derive_sample(src, W.edit_desc(3, n, True, "keep", 1.0))
    assert eng.ctx.pool_stats()[2] == live                      # the hole was reused
    model = M.derive(planes, 3, n, True)
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    replace_track(eng, e, spec, 1, edited, oracle_sample(e, model, 44100), 0.0, 4 * unit)
    play_both(eng, e, 4)
    eng.close()
    e.close()


def test_mipmaps_of_a_derived_sample():
    spec = synth.make_session("fxmip", 2, n_blocks=2, block=128, seed=0xF1319)
    eng = build_engine(spec, max_blocks=2)
    planes = source(2, 5003)
    src = eng.add_sample("f32", 48000, planes)
    sid = eng.derive_sample(src, W.edit_desc(2, 5000, True, "mono_mix", 0.5, 1000, 1000, "smooth", "smooth"))
    model = M.derive(planes, 2, 5000, True, M.MONO_MIX, 0.5, 1000, 1000, M.SMOOTH, M.SMOOTH)
    eng.ctx.build_mipmaps(sid, 1)
    levels = eng.L.wbx_mip_levels(5000)
    assert levels >= 2
    for lv in range(levels):
        mip = eng.ctx.fetch_mipmap(sid, lv, 1, 5000, 1)
        assert np.array_equal(mip[0], O.oracle_mip("f32", model[0], lv, 1)), lv
    eng.close()


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_edits_beside_the_audio_thread():
    """An edit shows nothing on the host while it runs, so a delete cannot be AIMED into one.  Instead a clip far behind the
    played range names the big sample for as long as the threads run: a delete of it can never succeed there, whenever it
    lands — between two edits it is refused for the clip (-4), inside one for the pin (-3, the pin is asked first) — so one
    thread deletes without pause while the other normalizes (measure and derive under ONE pin) until a refusal for the pin
    has been seen.  Afterwards, the clip gone, the delete succeeds."""
    NB, FR, WAIT, CALLS = 300, 1 << 21, 60.0, 64
    spec = synth.make_session("fxthr", 2, n_blocks=NB, block=128, seed=0xF17812)
    rng = np.random.default_rng(29)
    planes = [rng.uniform(-1.0, 1.0, FR).astype(np.float32) for _ in range(2)]

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 48000, planes)
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
    playing = sorted({c[5] for t in eng.tracks for c in eng.clips(t)})[:2]      # samples the session is playing
    shapes = {s: (spec.samples[s].frames, spec.samples[s].channels) for s in playing}
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
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            for s in playing:
                fr, ch = shapes[s]
                results[("st", s)] = eng.measure_sample(s, channels=ch, frames=fr)
                results[("id", s)] = eng.derive_sample(s, W.edit_desc(1, min(fr - 1, 4099), True, "keep", 0.5, 9, 9), channels=ch)
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"] = eng.normalize_sample(big, 0.5, first_frame=first, n_frames=n, channels=2, frames=FR)
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
    # every delete beside the edits was refused — for the clip, or, inside an edit, for the pin, and that one was seen
    print("normalize calls", results["calls"], "deletes", {k: v for k, v in seen.items()})
    pinned = [k for k in seen if k[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every edit read a live source: the results are the model's, bit for bit
    sid, gain = results["big"]
    peak = max(float(np.abs(p[first:first + n]).max()) for p in planes)
    assert np.float32(gain) == M.normalize_gain(0.5, np.float32(peak))
    want = M.derive(planes, first, n, gain=np.float32(gain))
    got = download(eng.ctx, sid, 2, n)
    assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))
    for s in playing:
        fr, ch = shapes[s]
        src = download(eng.ctx, s, ch, fr)
        m = min(fr - 1, 4099)
        assert bits(np.stack(download(eng.ctx, results[("id", s)], ch, m))).tolist() == \
            bits(np.stack(M.derive(src, 1, m, True, M.KEEP, 0.5, 9, 9))).tolist()
        check_stats(results[("st", s)], M.measure(src), fr, "playing sample")
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    with pytest.raises(W.WbxError) as ex:
        eng.measure_sample(big, channels=2, frames=FR)
    assert ex.value.status == -4
    eng.close()


# ---- 7: an export and edits side by side ----------------------------------------------------------------------------------------
def test_an_export_and_edits_run_side_by_side():
    """wbx_engine_export_sample works on the export stream under export_mu, derive and resample on the edit stream under
    fx_mu: one thread exports a sample (17 chunks of 4096 frames) while a second derives and then resamples the same sample
    and the main thread renders a track that plays it.  Every call succeeds, and the exported bytes, both new samples and
    the rendered blocks are, bit for bit, what the same calls give one after another on a fresh engine."""
    FR, F, NB = (1 << 16) + 5, 128, 8
    rng = np.random.default_rng(0x51DE)
    planes = [rng.uniform(-1.3, 1.3, FR).astype(np.float32) for _ in range(2)]
    desc = W.edit_desc(0, FR, True, "keep", 0.5, 100, 0)
    n_rs = W.resample_frames(48000, 44100, FR)

    def session():
        eng = W.Engine(1, buffer_size=F, sample_rate=48000, max_blocks=1)
        sid = eng.add_sample("f32", 48000, planes)
        eng.add_audio_clip(eng.add_track("t"), "clip", 0.0, 4.0, 0.0, sid)
        eng.ctx.set_export_chunk(4096)
        eng.play()
        return eng, sid

    def export(eng, sid, r):
        r["bytes"], r["stats"] = eng.export_sample(sid, "i16", clamp=True)

    def edit(eng, sid, r):
        r["derived"] = eng.derive_sample(sid, desc)
        r["resampled"] = eng.resample_sample(sid, 44100, "fast")

    def render(eng, r):
        out = W.AudioBuffer(F, 2)
        r["blocks"] = []
        for _ in range(NB):
            eng.process(None, out, 48000.0)
            r["blocks"].append(np.stack(out.channel_buffers).copy())

    def audio_of(eng, r):
        r["derived_audio"] = np.stack(download(eng.ctx, r["derived"], 2, FR))
        r["resampled_audio"] = np.stack(download(eng.ctx, r["resampled"], 2, n_rs))

    want = {}
    eng, sid = session()
    export(eng, sid, want)
    edit(eng, sid, want)
    render(eng, want)
    audio_of(eng, want)
    eng.close()

    got, errors = {}, []
    eng, sid = session()
    start = threading.Barrier(3)

    def beside(fn):
        def run():
            try:
                start.wait()
                fn(eng, sid, got)
            except Exception as ex:   # a status that is not WBX_OK raises WbxError
                errors.append(ex)
        return threading.Thread(target=run)

    threads = [beside(export), beside(edit)]
    for th in threads:
        th.start()
    start.wait()
    render(eng, got)
    for th in threads:
        th.join()
    assert not errors, errors
    audio_of(eng, got)
    eng.close()
    assert got["bytes"].size == 2 * FR and np.array_equal(got["bytes"], want["bytes"]) and got["stats"] == want["stats"]
    assert (got["derived"], got["resampled"]) == (want["derived"], want["resampled"])
    for k in ("derived_audio", "resampled_audio"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k
    assert any(b.any() for b in want["blocks"]) and len(got["blocks"]) == NB
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got["blocks"], want["blocks"]))
