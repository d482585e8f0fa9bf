"""wbx_clip_convolve and wbx_engine_convolve_sample on the device.  Results come back through wbx_clip_download and are
compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/convolve_model.py, the numpy twin of the
header's text.  Sizes are the smallest at which the kernel can still go wrong, around its two shape constants (T, the
output frames of a workgroup's tile; P, the taps of a segment): a lane's 8 frames and the last lane's partial store
(1, 7, 8, 9), one tile less, exactly and more than a frame (T-1, T, T+1), two tiles and a piece (2T+5); a response of
1, 2, 7 taps (less than one block of 8), of one segment less, exactly and more than a tap (P-1, P, P+1) and of two
segments and a piece (2P+3).  Every case is a few thousand frames by a few thousand taps."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import convolve_model as M
import loudness_model as LM
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
T, P = W.lib().wbx_convolve_tile_frames(), W.lib().wbx_convolve_segment_taps()
assert (T, P) == (M.TILE, M.SEGMENT)
OUTS = [1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 5]
TAPS = [1, 2, 7, P - 1, P, P + 1, 2 * P + 3]
PAIRS = [(1, 1), (2, 1), (2, 2), (1, 2)]                        # (source channels, response channels)
SRC_LEN, IR_LEN = 2 * T + 5 + P + 2 + 700, 2 * P + 3 + 9
SRC = {1: 1, 2: 2}                                              # channels -> clip id
IR = {1: 3, 2: 4}
DST = 100
bits = BU.bits


def source(channels, n=SRC_LEN, seed=0xC0417):
    rng = np.random.default_rng(seed + channels)
    return [(rng.uniform(-0.5, 0.5, n) + 0.125 * (1 - 2 * k)).astype(np.float32) for k in range(channels)]


def response(channels, n=IR_LEN, seed=0x1E5):
    """decaying noise, the two channels different"""
    rng = np.random.default_rng(seed + channels)
    return [(rng.uniform(-1.0, 1.0, n) * np.exp(-np.arange(n) * (3.0 + k) / n)).astype(np.float32) for k in range(channels)]


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    c.ir = {ch: response(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
        c.clip_upload(IR[ch], "f32", RATE, c.ir[ch])
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


# ---- 1: output lengths x response lengths, the four channel pairings, three out_firsts ------------------------------------------
def shape_of_call(O_, L, i):
    """the i-th variation of a case: out_first 0, 1 or (L - 1) / 2; the window ends 0, 3 or 600 frames before the full
    result's last frame; the ranges start inside their clips, and on odd i END on their clips' last frames"""
    out_first = (0, 1, (L - 1) // 2)[i % 3]
    n = max(1, O_ + out_first - L + 1 + (0, 3, 600)[(i // 3 + i) % 3])
    while out_first + O_ > n + L - 1:
        n += 1
    first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
    ir_first = IR_LEN - L if i % 2 else (0, 9, 4)[i % 3]
    assert first >= 0 and first + n <= SRC_LEN and ir_first >= 0 and ir_first + L <= IR_LEN
    return out_first, n, first, ir_first


CASES = [(O_, L, oi + li) for oi, O_ in enumerate(OUTS) for li, L in enumerate(TAPS)]


def test_the_matrix_covers_what_it_claims():
    seen = {(pi, shape_of_call(O_, L, i + pi)[0] == (L - 1) // 2, (i + pi) % 2) for O_, L, i in CASES for pi in range(4)}
    assert len(seen) == 16                                      # every pairing with and without the delay dropped, both range ends
    assert {shape_of_call(O_, L, i + pi)[0] for O_, L, i in CASES for pi in range(4)} >= {0, 1, P // 2, P + 1}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "out%d-taps%d" % (c[0], c[1]))
def test_convolve_matrix(ctx, case):
    O_, L, i = case
    for pi, (cs, ci) in enumerate(PAIRS):
        out_first, n, first, ir_first = shape_of_call(O_, L, i + pi)
        ch = max(cs, ci)
        want = M.convolve_clip(ctx.src[cs], first, n, ctx.ir[ci], ir_first, L, out_first, O_)
        st = ctx.clip_convolve(SRC[cs], IR[ci], DST, first, n, ir_first, L, out_first, O_, stats_channels=ch)
        got = download(ctx, DST, ch, O_)
        assert first_bad(got, want) is None, ((cs, ci), out_first, n, first, ir_first, first_bad(got, want))
        check_stats(st, FX.measure(want), O_, "stats_of_result")


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d" % p)
def test_same_length_and_full_ring_out_windows(ctx, pair):
    cs, ci = pair
    ch = max(cs, ci)
    for n, L in ((T + 3, 300), (2 * T, P + 9), (5, 900), (3000, 1)):
        for out_first, O_ in ((0, n), (0, n + L - 1), ((L - 1) // 2, n), (n + L - 2, 1)):
            want = M.convolve_clip(ctx.src[cs], 7, n, ctx.ir[ci], 2, L, out_first, O_)
            ctx.clip_convolve(SRC[cs], IR[ci], DST, 7, n, 2, L, out_first, O_)
            assert first_bad(download(ctx, DST, ch, O_), want) is None, (n, L, out_first, O_)
        ctx.clip_convolve(SRC[cs], IR[ci], DST, 7, n, 2, L)     # the default window: the whole ring-out
        assert first_bad(download(ctx, DST, ch, n + L - 1), M.convolve_clip(ctx.src[cs], 7, n, ctx.ir[ci], 2, L)) is None


# ---- 2: what lies beside the ranges, what is not finite inside them, gains, overflow ------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d" % p)
def test_frames_beside_the_ranges_do_not_count(ctx, pair):
    """loud samples and NaNs in front of and behind BOTH ranges: the result is that of the quiet ranges alone"""
    cs, ci = pair
    planes, taps = source(cs, 3000, seed=0xBE51DE), response(ci, 2600, seed=0xBE51)
    for p in planes:
        p[:200], p[190:200], p[2700:], p[2710:2720] = 1e30, np.nan, -1e30, np.nan
    for h in taps:
        h[:100], h[95:100], h[2500:], h[2500:2510] = -1e30, np.nan, 1e30, np.inf
    ctx.clip_upload(50, "f32", RATE, planes)
    ctx.clip_upload(51, "f32", RATE, taps)
    for (first, n), (ir_first, L) in (((200, 2500), (100, 2400)), ((200, 1), (100, 2400)), ((200, 2500), (100, 1)), ((200, 9), (100, 7))):
        quiet_x = [p[first:first + n].copy() for p in planes]
        quiet_h = [h[ir_first:ir_first + L].copy() for h in taps]
        want = M.convolve_clip(quiet_x, 0, n, quiet_h, 0, L)
        assert np.all(np.isfinite(np.stack(want))) and np.max(np.abs(np.stack(want))) < 1e6
        ctx.clip_convolve(50, 51, DST, first, n, ir_first, L)
        assert first_bad(download(ctx, DST, max(cs, ci), n + L - 1), want) is None, (first, n, ir_first, L)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d" % p)
def test_values_that_are_not_finite_enter_as_zero(ctx, pair):
    cs, ci = pair
    n, L = T + 600, P + 40
    planes, taps = source(cs, n, seed=0x0FF), response(ci, L, seed=0x0FE)
    zx, zh = [p.copy() for p in planes], [h.copy() for h in taps]
    for c, (p, z) in enumerate(zip(planes, zx)):
        at = np.array([0, 5, 300, T - 1, T, T + 1, n - 1]) - (c if c else 0) * np.array([0, 1, 1, 1, 1, 1, 1])
        p[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan]
        z[at] = 0.0
    for c, (h, z) in enumerate(zip(taps, zh)):
        at = np.array([0, 3, 8, P - 1, P, P + 1, L - 1]) - (c if c else 0) * np.array([0, 1, 1, 1, 1, 1, 1])
        h[at] = [np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan, -np.inf]
        z[at] = 0.0
    planes[0].view(np.uint32)[40] = 0xFFC12345                  # a NaN with a payload and a sign
    zx[0][40] = 0.0
    ctx.clip_upload(52, "f32", RATE, planes)
    ctx.clip_upload(53, "f32", RATE, taps)
    want = M.convolve_clip(planes, 0, n, taps, 0, L)
    assert first_bad(want, M.convolve_clip(zx, 0, n, zh, 0, L)) is None and np.all(np.isfinite(np.stack(want)))
    ctx.clip_convolve(52, 53, DST, 0, n, 0, L)
    assert first_bad(download(ctx, DST, max(cs, ci), n + L - 1), want) is None


@pytest.mark.parametrize("gain", [1.0, 0.5, -2.0, 0.0])
def test_gains(ctx, gain):
    """one multiplication after the sum, one rounding; a gain of 0 leaves zeros that carry acc's sign"""
    n, L = T + 11, 700
    want = M.convolve_clip(ctx.src[2], 3, n, ctx.ir[2], 0, L, gain=gain)
    ctx.clip_convolve(SRC[2], IR[2], DST, 3, n, 0, L, gain=gain)
    assert first_bad(download(ctx, DST, 2, n + L - 1), want) is None
    if gain == 0.0:
        assert not np.any(np.stack(want)) and np.any(np.signbit(np.stack(want))) and not np.all(np.signbit(np.stack(want)))


def test_a_result_that_overflows_fp32(ctx):
    """fp64 holds the sum, fp32 stores +-inf; -0.0 in, +0.0 out (the sum starts at +0.0)"""
    n, L = 1200, 300
    x = (source(1, n, seed=0xB16)[0].astype(np.float64) * 5e38).astype(np.float32)   # up to 3.1e38
    x[:3] = -0.0
    h = np.full(L, 4.0, dtype=np.float32)
    h[::2] = -4.0
    ctx.clip_upload(54, "f32", RATE, [x])
    ctx.clip_upload(55, "f32", RATE, [h])
    want = M.convolve_clip([x], 0, n, [h], 0, L)
    assert np.isinf(want[0]).any() and not np.isnan(want[0]).any() and want[0].view(np.uint32)[0] == 0
    ctx.clip_convolve(54, 55, DST, 0, n, 0, L)
    assert first_bad(download(ctx, DST, 1, n + L - 1), want) is None
    want = M.convolve_clip([x], 0, n, [h], 0, L, gain=1e-4)     # ... and a gain that brings it back: no overflow before it
    assert np.all(np.isfinite(want[0]))
    ctx.clip_convolve(54, 55, DST, 0, n, 0, L, gain=1e-4)
    assert first_bad(download(ctx, DST, 1, n + L - 1), want) is None


@pytest.mark.parametrize("channels", [1, 2])
def test_the_response_may_be_the_source_itself(ctx, channels):
    n, L = T + 70, P + 5
    want = M.convolve_clip(ctx.src[channels], 10, n, ctx.src[channels], 3, L)
    ctx.clip_convolve(SRC[channels], SRC[channels], DST, 10, n, 3, L)
    assert first_bad(download(ctx, DST, channels, n + L - 1), want) is None


@pytest.mark.parametrize("channels", [1, 2])
def test_a_unit_impulse_returns_the_source_exactly(ctx, channels):
    """(the source holds no -0.0, which would come back as +0.0: the sum starts at +0.0)"""
    n = 2 * T + 5
    for delay, L in ((0, 1), (0, P + 3), (5, 6), (P, P + 1)):
        h = np.zeros(L, dtype=np.float32)
        h[delay] = 1.0
        ctx.clip_upload(56, "f32", RATE, [h])
        ctx.clip_convolve(SRC[channels], 56, DST, 9, n, 0, L, delay, n)
        assert first_bad(download(ctx, DST, channels, n), [p[9:9 + n] for p in ctx.src[channels]]) is None, (delay, L)


def test_time_of_the_last_convolution():
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_convolve_ms(c.h, C.byref(out)) == -4 and out.value == 7.0     # none yet
    c.clip_upload(1, "f32", RATE, source(1, 5000))
    c.clip_upload(2, "f32", RATE, response(1, 300))
    assert c.L.wbx_convolve_ms(c.h, None) == -4
    c.clip_convolve(1, 2, 3, 0, 5000, 0, 300)
    assert 0.0 < c.convolve_ms() < 1000.0
    c.close()


# ---- 3: the pool -------------------------------------------------------------------------------------------------------------------
def test_a_replaced_dst_takes_the_old_extents_place_and_a_delete_restores_the_pool():
    c = W.MixContext(4, block=128)
    planes, taps = source(2, 5000), response(1, 97)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_upload(3, "f32", RATE, taps)
    c.clip_upload(2, "f32", RATE, [np.ones(4000, dtype=np.float32)] * 2)        # a neighbour behind what comes next
    base = c.pool_stats()
    c.clip_convolve(1, 3, 10, 0, 4000, 0, 97)
    with_one = c.pool_stats()
    assert with_one[0] == base[0] and with_one[1] == base[1] and with_one[2] > base[2]
    for first in (5, 900):                                      # replaced by results of the same length: the same figures
        c.clip_convolve(1, 3, 10, first, 4000, 0, 97)
        assert c.pool_stats() == with_one
        assert first_bad(download(c, 10, 2, 4096), M.convolve_clip(planes, first, 4000, taps, 0, 97)) is None
    c.clip_convolve(1, 3, 10, 0, 700, 0, 1)                     # ... by a shorter one: nothing more is reserved or live
    assert c.pool_stats()[:2] == with_one[:2] and c.pool_stats()[2] <= with_one[2]
    assert first_bad(download(c, 10, 2, 700), M.convolve_clip(planes, 0, 700, taps, 0, 1)) is None
    assert all(np.all(p == 1.0) for p in download(c, 2, 2, 4000))
    assert c.L.wbx_clip_free(c.h, 10) == 0
    assert c.pool_stats() == base
    c.close()


def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    ctx.clip_convolve(SRC[2], IR[1], DST, 0, 64, 0, 8, 0, 64)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    ctx.clip_upload(60, "i16", RATE, [np.arange(64, dtype=np.int16)] * 2)
    ctx.clip_upload(61, "f32", 44100, response(1, 64))
    st = _ffi.ClipStats()
    S, R = SRC[2], IR[1]

    def refused(status, why, src=S, ir=R, dst=DST, first=0, n=64, ir_first=0, taps=8, out_first=0, out=64, gain=1.0):
        before = ctx.pool_stats()
        got = L.wbx_clip_convolve(ctx.h, src, ir, dst, first, n, ir_first, taps, out_first, out, gain, C.byref(st))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept

    refused(-4, b"unknown source", src=999)
    refused(-4, b"unknown response", ir=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"no frames", taps=0)
    refused(-4, b"no frames", out=0)
    refused(-4, b"source's range", first=SRC_LEN - 10, n=11, out=11)
    refused(-4, b"source's range", first=SRC_LEN + 1, n=1, out=1)
    refused(-4, b"response's range", ir_first=IR_LEN - 7, taps=8)
    refused(-4, b"response's range", ir_first=IR_LEN + 1, taps=1)
    refused(-4, b"past the full result", out=72)                # 64 + 8 - 1 = 71 frames exist
    refused(-4, b"past the full result", out_first=8, out=64)
    refused(-4, b"past the full result", out_first=71, out=1)
    refused(-4, b"past the full result", out_first=(1 << 64) - 1, out=2)        # a sum that wraps
    refused(-4, b"may not replace", dst=S)
    refused(-4, b"may not replace", dst=R)
    refused(-4, b"may not replace", src=S, ir=S, dst=S)
    for g in (np.nan, np.inf, -np.inf):
        refused(-4, b"gain", gain=g)
    refused(-4, b"2^31 - 16", n=1 << 31, taps=1, out=(1 << 31) - 16)             # judged on the arithmetic: no clip is that long
    refused(-4, b"rates differ", ir=61)
    refused(-3, b"not F32", src=60)                             # (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, b"not F32", ir=60)
    refused(-3, b"2^20", n=1 << 22, taps=(1 << 20) + 1, out=64)
    refused(-3, b"2^46", n=1 << 30, taps=1 << 20, out=(1 << 25) + 1)             # stereo: 2^25 frames x 2^20 taps x 2 is the cap
    refused(-4, b"source's range", n=1 << 30, taps=1 << 20, out=1 << 25)         # ... at the cap the sizes pass, the clips do not
    refused(-3, b"2^46", src=SRC[1], n=1 << 30, taps=1 << 20, out=(1 << 26) + 1)  # mono: 2^26 frames
    refused(-4, b"source's range", src=SRC[1], n=1 << 30, taps=1 << 20, out=1 << 26)
    refused(-3, b"2^46", src=SRC[1], ir=IR[2], n=1 << 30, taps=1 << 20, out=(1 << 25) + 1)   # the RESULT's channels count
    # what is not refused: the window's last frame, the response being the source
    ctx.clip_convolve(S, R, 62, 0, 64, 0, 8, 70, 1)
    ctx.clip_convolve(S, S, 62, 0, 64, 0, 8)
    assert L.wbx_clip_free(ctx.h, 62) == 0


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    planes = source(2, n)
    c.clip_upload(1, "f32", RATE, planes)                       # 8 MiB in the first slab (64 MiB)
    c.clip_upload(2, "f32", RATE, response(1, 8))
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_convolve(1, 2, 10 + len(made), 0, n, 0, 8)   # 8 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    want = M.convolve_clip([p[:4096] for p in planes], 0, 4096, response(1, 8), 0, 8, 0, 4096)
    assert first_bad([c.clip_download(made[-1], k, n + 7, np.float32)[:4096] for k in range(2)], want) is None
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 4: through the engine -----------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_convolve_sample_of_an_upload_a_take_a_bounce_and_an_earlier_result():
    spec = synth.make_session("conv2", 3, n_blocks=6, block=128, seed=0xC0412)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
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
    # an upload, a stereo room and a designed low-pass
    NU = 3 * LM.hop_frames(rate)                                # three hops of the loudness meter
    planes = source(2, NU + 8, seed=0x0B)
    up = eng.add_sample("f32", rate, planes)
    room_planes = response(2, 900, seed=0x400)
    room = eng.add_sample("f32", rate, room_planes)
    taps = W.fir_design(rate, "lowpass", 6000.0)
    assert taps.shape == (255,) and np.array_equal(taps.view(np.uint32), M.fir_design(rate, "lowpass", 6000.0).view(np.uint32))
    fir = eng.add_fir(rate, taps)
    assert eng._sample_shape[fir] == (255, 1)

    # the low-pass on the upload, its delay dropped: as long as the range
    c_up, st = eng.convolve_sample(up, fir, out_first=127, out_frames=NU, first_frame=4, n_frames=NU, stats=True)
    want_up = M.convolve_clip(planes, 4, NU, [taps], 0, 255, 127, NU)
    assert eng._sample_shape[c_up] == (NU, 2)
    assert first_bad(download(eng.ctx, c_up, 2, NU), want_up) is None
    check_stats(st, FX.measure(want_up), NU, "convolve_sample's stats")
    # the room on the mono take: a stereo result, the full ring-out, -6 dB
    c_take = eng.convolve_sample(take, room, gain_db=-6.0, frames=frames, channels=1)
    assert eng._sample_shape[c_take] == (frames + 899, 2)
    want_take = M.convolve_clip([x], 0, frames, room_planes, 0, 900, gain=10.0 ** (-6.0 / 20.0))
    assert first_bad(download(eng.ctx, c_take, 2, frames + 899), want_take) is None
    # the room on the bounce, a window of it
    c_stem = eng.convolve_sample(ids[0], room, out_first=50, out_frames=nb, ir_first=10, ir_frames=800)
    assert first_bad(download(eng.ctx, c_stem, spec.channels, nb), M.convolve_clip(stem, 0, nb, room_planes, 10, 800, 50, nb)) is None
    # of an earlier result, which is also its own response
    again = eng.convolve_sample(c_up, c_up, n_frames=600, ir_frames=300)
    assert first_bad(download(eng.ctx, again, 2, 899), M.convolve_clip(want_up, 0, 600, want_up, 0, 300)) is None

    # the low-passed upload on a track, against the oracle playing the MODEL's clip
    unit = BU.block_beats(spec.block, rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    for t in range(3):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
        while e.clips(t):
            e.delete_clip(t, 0)
    eng.add_audio_clip(eng.tracks[2], "lowpassed", 0.5 * unit, 5.5 * unit, 0.0, c_up, 1.0, 1.0)
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
    got, _ = eng.export_sample(c_up, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want_up, axis=1).reshape(-1).view(np.uint32))
    _, E = eng.loudness_sample(c_up, energies=True, rate=rate)
    want_E = LM.hop_energies(want_up, 0, NU, rate)
    assert E.shape == want_E.shape == (2, 3) and np.array_equal(E.view(np.uint64), want_E.view(np.uint64))
    with pytest.raises(W.WbxError):
        eng.delete_sample(c_up)                                 # a clip names it
    eng.delete_sample(again)
    # refusals create no sample
    L, new = W.lib(), C.c_uint32(12345)
    before = eng.ctx.pool_stats()
    call = lambda s, r, n, taps, out, gain=1.0, ref=C.byref(new): L.wbx_engine_convolve_sample(eng.h, s, r, 0, n, 0, taps, 0, out, gain, ref, None)
    assert call(9999, fir, 8, 8, 8) == -4
    assert call(up, 9999, 8, 8, 8) == -4
    assert call(again, fir, 8, 8, 8) == -4                      # deleted
    assert call(up, again, 8, 8, 8) == -4
    assert call(up, fir, NU + 9, 8, 8) == -4
    assert call(up, fir, 8, 256, 8) == -4
    assert call(up, fir, 8, 8, 16) == -4
    assert call(up, fir, 8, 8, 8, gain=np.nan) == -4
    assert call(up, fir, 8, 8, 8, ref=None) == -4
    assert call(up, fir, 1 << 30, 1 << 20, (1 << 25) + 1) == -3
    assert new.value == 12345 and eng.ctx.pool_stats() == before
    eng.close()
    e.close()


def test_cpp_adapter_convolves_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take, designs a band-stop with wbx_fir_design, uploads it and
    calls wbx::Engine::convolve_sample with the delay dropped and a gain of 0.5; the result equals the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_convolve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_convolve.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "convolved.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    assert "adapter convolve ok %d" % n in out, out
    idx = np.arange(n, dtype=np.uint64)
    x = (((idx * 2654435761) & 0xFFFFFFFF) & 0xFFFF).astype(np.float32) / np.float32(65536.0) - np.float32(0.25)
    h = M.fir_design(48000, "bandstop", 3000.0, 9000.0, 255, 8.6)
    want = M.convolve_clip([x], 0, n, [h], 0, 255, 127, n, gain=0.5)
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == n and first_bad([got], want) is None
    assert ("peak %.9g" % np.max(np.abs(want[0]))) in out, out


# ---- 5: beside the audio thread -------------------------------------------------------------------------------------------------
def test_convolutions_beside_the_audio_thread():
    """The shape of the filter's test (test_gpu_filter.py): clips far behind the played range name the big sample AND the
    response while the threads run, so a delete of either can never succeed — between two convolutions it is refused for
    the clip (-4), inside one for the pin (-3, asked first) — one thread deletes the response and the source in turn without
    pause while the other convolves until BOTH have been refused for the pin.  The master is what it is without the
    convolutions, and the last result equals the model where it is compared: the first, a middle and the last tile."""
    NB, FR, TAPS_, WAIT, CALLS = 300, 1 << 20, 1 << 14, 60.0, 64
    spec = synth.make_session("convthr", 2, n_blocks=NB, block=128, seed=0xC04712)
    planes, taps = source(2, FR, seed=35), response(1, TAPS_, seed=36)

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 44100, planes)
        rid = eng.add_sample("f32", 44100, taps)
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        eng.add_audio_clip(eng.tracks[1], "far too", 1000.0, 1001.0, 0.0, rid, 1.0, 1.0)
        return sid, rid

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
    big, room = with_big(eng)
    first, n = 5, FR - 8
    L = W.lib()
    began, finished = threading.Event(), threading.Event()
    refused = {big: threading.Event(), room: threading.Event()}
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        turn = 0
        while not finished.is_set() and time.monotonic() < end:
            which = (room, big)[turn & 1]
            turn += 1
            st = L.wbx_engine_delete_sample(eng.h, which)
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            if st == -3:
                refused[which].set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not (refused[big].is_set() and refused[room].is_set()):
                results["big"] = eng.convolve_sample(big, room, first_frame=first, n_frames=n, channels=2, frames=FR,
                                                     ir_channels=1, ir_length=TAPS_)
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
    print("convolve calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused[big].is_set() and refused[room].is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every convolution read live clips: the result is the model's, bit for bit
    total = n + TAPS_ - 1
    for at in (0, (total // 2 // T) * T - 9, total - T - 3):
        want = M.convolve_clip(planes, first, n, taps, 0, TAPS_, at, T + 3)
        got = [eng.ctx.clip_download(results["big"], k, total, np.float32)[at:at + T + 3] for k in range(2)]
        assert first_bad(got, want) is None, at
    # afterwards: no pin is left (the clips are what refuses now), and with the clips gone the deletes succeed
    for sid, t in ((big, 0), (room, 1)):
        assert L.wbx_engine_delete_sample(eng.h, sid) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
        eng.delete_clip(eng.tracks[t], len(eng.clips(eng.tracks[t])) - 1)
        assert L.wbx_engine_delete_sample(eng.h, sid) == 0
    new = C.c_uint32(12345)
    assert L.wbx_engine_convolve_sample(eng.h, big, room, 0, 8, 0, 8, 0, 8, 1.0, C.byref(new), None) == -4 and new.value == 12345
    eng.close()
