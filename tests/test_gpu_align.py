"""wbx_clip_align and wbx_engine_align_samples on the device.  info — and the curve where asked — are compared BIT FOR BIT
(uint64 views: -0.0 shows) with tests/align_model.py, the numpy twin of the header's text.  Shapes are the smallest that reach
their hazard: a last lane with unused lags (one chunk, one wave, 17 lags), a last chunk of 8 terms with lags across a wave's
512 (two chunks), two blocks of 4096 lags (three chunks), and — from the library's getters, tests/align_shapes.py — the
smallest template and lag count that cut a call into two bands.  B's range lies between neighbours of 3e38 in its clip, and
the clips hold NaN, both infinities and -0.0."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import align_model as M
import align_shapes
import bounce_util as BU
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
BIG = np.float32(3e38)
# name -> (n, lag_min, lag_max)
SHAPES = {"one wave": (64, -8, 8), "short last chunk": (2048 + 8, -5, 600), "two lag blocks": (3 * 2048, -2050, 2050)}


def noise(n, seed, specials=True):
    """seeded noise with a NaN, both infinities, -0.0 and a huge sample sprinkled in"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    if specials and n >= 40:
        at = rng.choice(n, 10, replace=False)
        v[at[:2]], v[at[2:4]], v[at[4:6]], v[at[6:8]], v[at[8:]] = np.nan, np.inf, -np.inf, np.float32(-0.0), np.float32(1e30)
    return v


def between_neighbours(planes, front, back):
    """the planes as a range of a longer clip whose other frames are 3e38"""
    return [np.concatenate([np.full(front, BIG), p, np.full(back, BIG)]).astype(np.float32) for p in planes]


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.next_id = 0
    yield c
    c.close()


def upload(c, planes, rate=RATE, fmt="f32"):
    c.next_id += 1
    c.clip_upload(c.next_id, fmt, rate, planes)
    return c.next_id


def bits(v):
    return np.float64(v).view(np.uint64)


def same_info(got, want):
    """None, or the first field that differs (floats in a bit)"""
    for k in M.INFO_FIELDS:
        if k in want and (bits(got[k]) != bits(want[k]) if isinstance(want[k], float) else got[k] != want[k]):
            return k, got[k], want[k]
    return None


def same_curve(got, want):
    """None, or the first lag index that differs in a bit"""
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.flatnonzero((got["r"].view(np.uint64) != want["r"].view(np.uint64)) | (got["energy"].view(np.uint64) != want["energy"].view(np.uint64)))
    return (int(bad[0]), got[bad[0]], want[bad[0]], len(bad)) if bad.size else None


def run_and_check(c, a_planes, a_first, n, b_planes, b_first, m, lo, hi, flags=0, ids=None):
    """uploads the two clips (or takes `ids`), aligns them with and without a curve, and holds both against the model"""
    ra, rb = ids if ids else (upload(c, a_planes), upload(c, b_planes))
    want, want_curve = M.align_clips(a_planes, a_first, n, b_planes, b_first, m, lo, hi, flags)
    info, curve = c.clip_align(ra, a_first, n, rb, b_first, m, lo, hi, either_polarity=flags, curve=True)
    where = (len(a_planes), len(b_planes), a_first, n, b_first, m, lo, hi, flags)
    assert same_curve(curve, want_curve) is None, (where, same_curve(curve, want_curve))
    assert same_info(info, want) is None, (where, same_info(info, want), info, want)
    assert info["launches"] == W.lib().wbx_align_launches(n, hi - lo + 1)
    alone, none = c.clip_align(ra, a_first, n, rb, b_first, m, lo, hi, either_polarity=flags)
    assert none is None and same_info(alone, info) is None and alone == info      # curve_out NULL: the same info
    return info, curve


# ---- 1: the shapes ---------------------------------------------------------------------------------------------------------------
def test_unused_lags_of_the_last_lane_are_neither_stored_nor_picked(ctx):
    """n = 64, lags -8 .. 8: the third lane owns lags 8 .. 15 and only the first counts.  B is loud where lags 9 .. 15 alone
    reach (their scores would win), and a curve buffer of 32 records keeps what lies behind the 17"""
    n, lo, hi = SHAPES["one wave"]
    a = [noise(n, 1, specials=False)]
    a[0][57:] *= np.float32(10.0)
    b = noise(n + 16, 2, specials=False)
    b[n + hi:] = np.concatenate([a[0][57:] * np.float32(1e6), [np.float32(0.0)]])   # frames 72 .. 79, which only a lag above 8
                                                                  # multiplies, hold the template's tail as lag 15 meets it
    info, curve = run_and_check(ctx, a, 0, n, [b], 0, len(b), lo, hi)
    assert lo <= info["lag"] <= hi and info["lags"] == 17 and info["chunks"] == 1 and info["terms"] == 17 * 64
    # the same call through the C interface with room for 32 records
    ra, rb = upload(ctx, a), upload(ctx, [b])
    pts = np.zeros(32, dtype=M.CURVE_DTYPE)
    pts["r"], pts["energy"] = 9.0, 7.0
    ai = _ffi.AlignInfo()
    assert W.lib().wbx_clip_align(ctx.h, ra, 0, n, rb, 0, len(b), lo, hi, 0, C.byref(ai), pts.ctypes.data, 32) == 0
    assert same_curve(pts[:17], curve) is None and np.all(pts["r"][17:] == 9.0) and np.all(pts["energy"][17:] == 7.0)
    assert ai.lag == info["lag"]
    # ... and it WOULD win: with lag_max 15 the loud frames are picked
    far, _ = ctx.clip_align(ra, 0, n, rb, 0, len(b), lo, 15)
    assert far["lag"] == 15


@pytest.mark.parametrize("b_first", [0, 40])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_with_ranges_reaching_in_front_of_and_past_b(ctx, name, b_first):
    """a stereo reference against a mono clip whose range is shorter than n + lag_max and is reached in front of by the
    negative lags; around the range the clip holds 3e38, which the curve would show"""
    n, lo, hi = SHAPES[name]
    m = n + hi - 37
    a = between_neighbours([noise(n, 10), noise(n, 11)], 24, 8)
    b = between_neighbours([noise(m, 12 + b_first)], b_first, 56)
    info, curve = run_and_check(ctx, a, 24, n, b, b_first, m, lo, hi)
    assert np.all(np.isfinite(curve["r"])) and np.all(curve["energy"] < 1e70) and info["chunks"] == -(-n // 2048)


@pytest.mark.parametrize("cha,chb", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("name", ["one wave", "short last chunk"])
def test_channel_counts_may_differ(ctx, name, cha, chb):
    n, lo, hi = SHAPES[name]
    m = n + hi + 9
    a = [noise(n + 3, 20 + k) for k in range(cha)]
    b = between_neighbours([noise(m, 30 + k) for k in range(chb)], 16, 16)
    run_and_check(ctx, a, 3, n, b, 16, m, lo, hi, flags=cha & 1)


def test_the_band_seam(ctx):
    """the smallest template and lag count that make two bands: the curve at the first and last lags, at both sides of every
    4096-lag block boundary and at 256 seeded lags; info by the model's pick over the device's own curve; the launches"""
    L = W.lib()
    n, lags, per = align_shapes.band_seam_case()
    assert L.wbx_align_chunks(n) == per + 1 and L.wbx_align_launches(n, lags) == 6
    lo = -(lags // 2)
    hi = lo + lags - 1
    m = n + hi - 1000
    a, b = [noise(n, 40)], [noise(m, 41), noise(m, 42)]
    ra, rb = upload(ctx, a), upload(ctx, b)
    info, curve = ctx.clip_align(ra, 0, n, rb, 0, m, lo, hi, curve=True)
    rng = np.random.default_rng(0x5EA)
    at = {0, 1, lags - 2, lags - 1} | {q + d for q in range(4096, lags, 4096) for d in (-1, 0)} | {int(v) for v in rng.integers(0, lags, 256)}
    at = sorted(at)
    _, want = M.align_clips(a, 0, n, b, 0, m, lo, hi, only=[lo + q for q in at])
    assert same_curve(np.ascontiguousarray(curve[at]), want) is None, same_curve(np.ascontiguousarray(curve[at]), want)
    picked = M.pick(curve["r"], curve["energy"], lo, M.ref_energy(M.detector_of(a, 0, n)))
    picked.update(lags=lags, chunks=per + 1, terms=lags * n, launches=int(L.wbx_align_launches(n, lags)))
    assert same_info(info, picked) is None, (same_info(info, picked), info, picked)
    again, none = ctx.clip_align(ra, 0, n, rb, 0, m, lo, hi, either_polarity=True)
    either = M.pick(curve["r"], curve["energy"], lo, picked["ref_energy"], M.EITHER)
    assert none is None and same_info(again, either) is None


# ---- 2: behaviours -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one wave", "short last chunk"])
def test_a_clip_against_itself_has_lag_zero(ctx, name):
    n, lo, hi = SHAPES[name]
    x = [noise(n + hi + 20, 50), noise(n + hi + 20, 51)]
    s = upload(ctx, x)
    info, _ = run_and_check(ctx, x, 0, n, x, 0, len(x[0]), lo, hi, ids=(s, s))
    assert info["lag"] == 0 and info["inverted"] == 0 and abs(info["confidence"] - 1.0) < 1e-15 and info["r"] == info["energy"] == info["ref_energy"]


@pytest.mark.parametrize("name", ["one wave", "short last chunk"])
def test_silence_in_either_clip_picks_lag_min(ctx, name):
    n, lo, hi = SHAPES[name]
    m = n + hi
    for a, b in (([np.zeros(n, np.float32)], [noise(m, 60)]), ([noise(n, 61)], [np.zeros(m, np.float32)] * 2),
                 ([np.full(n, np.nan, np.float32)], [noise(m, 62)])):
        info, curve = run_and_check(ctx, a, 0, n, b, 0, m, lo, hi)
        assert info["lag"] == lo and info["score"] == 0.0 and info["confidence"] == 0.0 and info["offset"] == 0.0 and info["inverted"] == 0
        assert np.all(curve["r"] == 0.0)


def test_of_two_equal_best_lags_the_lowest_wins(ctx):
    """an integer-valued signal of period 16: lags 16 and 32 see the same products, exactly"""
    period = np.array([3, -5, 1, 7, -2, 0, 4, -6, 2, 5, -1, -7, 6, -3, 1, -4], dtype=np.float32)
    a, b = [np.tile(period, 4)], [np.tile(period, 7)]
    info, curve = run_and_check(ctx, a, 0, 64, b, 0, 112, 3, 40)
    assert info["lag"] == 16 and curve[13].tobytes() == curve[29].tobytes() and info["confidence"] == 1.0
    info, _ = run_and_check(ctx, a, 0, 64, b, 0, 112, 17, 40)
    assert info["lag"] == 32


@pytest.mark.parametrize("name", ["one wave", "short last chunk"])
def test_both_polarity_modes_on_an_inverted_copy(ctx, name):
    n, lo, hi = SHAPES[name]
    x = noise(n + hi + 8, 70, specials=False)
    a, b = [x[5:5 + n].copy()], [-x]
    either, _ = run_and_check(ctx, a, 0, n, b, 0, len(x), lo, hi, flags=M.EITHER)
    assert either["lag"] == 5 and either["inverted"] == 1 and either["r"] < 0.0 and abs(either["confidence"] - 1.0) < 1e-15
    plain, _ = run_and_check(ctx, a, 0, n, b, 0, len(x), lo, hi)
    assert plain["lag"] != 5 and plain["confidence"] < 0.5


def test_every_refusal_leaves_the_outputs_alone(ctx):
    L = W.lib()
    a, b = upload(ctx, [noise(5000, 80)] * 2), upload(ctx, [noise(6000, 81)])
    i16 = upload(ctx, [np.arange(6000, dtype=np.int16)], fmt="i16")
    other_rate = upload(ctx, [noise(6000, 82)], rate=44100)
    pts = np.zeros(512, dtype=M.CURVE_DTYPE)
    pts["r"] = 9.0
    ai = _ffi.AlignInfo()

    def refused(status, why, ref=a, a_first=0, n=4096, clip=b, b_first=0, m=6000, lo=-100, hi=100, flags=0, info=True, curve=True, cap=512):
        before = ctx.pool_stats()
        ai.lag, ai.lags = -77, 777
        got = L.wbx_clip_align(ctx.h, ref, a_first, n, clip, b_first, m, lo, hi, flags, C.byref(ai) if info else None,
                               pts.ctypes.data if curve else None, cap)
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert got == M.check(n, m, lo, hi, flags, info, curve, cap) or b"clip" in msg[12:] or b"rates" in msg
        assert ctx.pool_stats() == before and ai.lag == -77 and ai.lags == 777 and np.all(pts["r"] == 9.0) and np.all(pts["energy"] == 0.0)

    refused(-4, b"unknown reference clip", ref=999)
    refused(-4, b"unknown clip", clip=999)
    for bad in (0, 56, 4100, (1 << 24) + 8):
        refused(-4, b"n_frames", n=bad)
    for bad in (0, (1 << 31) - 16):
        refused(-4, b"m_frames", m=bad)
    refused(-4, b"lag_min outside", lo=-(1 << 24) - 1)
    refused(-4, b"lag_max outside", hi=(1 << 24) + 1)
    refused(-4, b"above lag_max", lo=5, hi=4)
    refused(-4, b"flag bits", flags=2)
    refused(-4, b"both NULL", info=False, curve=False)
    refused(-4, b"curve_cap", cap=200)
    refused(-3, b"2^17 lags", lo=0, hi=1 << 17, curve=False)
    refused(-4, b"curve_cap", lo=0, hi=1 << 17)                    # the capacity is asked first
    refused(-3, b"reference clip's storage format", ref=i16)
    refused(-3, b"clip's storage format is not F32", clip=i16)
    refused(-4, b"n_frames", ref=i16, n=4100)                      # the sizes are judged before the clips are looked at
    refused(-3, b"sample rates differ", clip=other_rate)
    refused(-4, b"reference's range ends past", a_first=5000 - 4095)
    refused(-4, b"reference's range ends past", a_first=(1 << 64) - 1)     # a sum that wraps
    refused(-4, b"range ends past the clip", b_first=1)
    refused(-3, b"sample rates differ", clip=other_rate, b_first=1)        # the rates are judged before the ranges
    # Python's wrapper asks wbx_align_check before it allocates the curve
    with pytest.raises(W.WbxError) as err:
        ctx.clip_align(a, 0, 4096, b, 0, 6000, -(1 << 24), 1 << 24, curve=True)
    assert err.value.status == -3
    # what is not refused: a curve without info, a capacity that is just enough
    assert L.wbx_clip_align(ctx.h, a, 0, 4096, b, 0, 6000, -100, 100, 0, None, pts.ctypes.data, 201) == 0
    assert np.all(pts["r"][:201] != 9.0) and np.all(pts["r"][201:] == 9.0)
    assert ctx.align_ms() > 0.0


# ---- 3: through the engine, the adapter, Python's conveniences ------------------------------------------------------------------
def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def test_align_samples_and_aligned_sample():
    """wbx_engine_align_samples equals the model; aligned_sample of a late, inverted copy and of an early one equals the
    reference sample for sample over their common range"""
    spec = synth.make_session("aln", 2, n_blocks=2, block=128, seed=0xA11)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=2)
    n = 6000
    x = noise(n, 90, specials=False)
    late = np.concatenate([np.zeros(137, np.float32), -x])[:n]
    early = x[50:].copy()
    ref, s_late, s_early = eng.add_sample("f32", rate, [x, x]), eng.add_sample("f32", rate, [late]), eng.add_sample("f32", rate, [early])
    info, curve = eng.align_samples(ref, s_late, -300, 300, either_polarity=True, curve=True)
    want, want_curve = M.align_clips([x, x], 0, n, [late], 0, n, -300, 300, M.EITHER)
    assert same_info(info, want) is None and same_curve(curve, want_curve) is None
    assert info["lag"] == 137 and info["inverted"] == 1
    odd, _ = eng.align_samples(ref, s_late, -300, 300, a_first=3, either_polarity=True)  # 5997 frames behind frame 3: 5992 are used
    assert odd["terms"] == 601 * 5992 and odd["lag"] == 140
    new, got = eng.aligned_sample(ref, s_late, 300)
    assert got == info and eng._sample_shape[new] == (n - 137, 1)
    assert np.array_equal(download(eng.ctx, new, 1, n - 137)[0], x[:n - 137])
    new, got = eng.aligned_sample(ref, s_early, 300)
    assert got["lag"] == -50 and got["inverted"] == 0 and eng._sample_shape[new] == (n, 1)
    moved = download(eng.ctx, new, 1, n)[0]
    assert np.all(moved[:50] == 0.0) and np.array_equal(moved[50:], x[50:])
    with pytest.raises(W.WbxError) as err:
        eng.align_samples(ref, 9999, -300, 300, m_frames=n)
    assert err.value.status == -4
    eng.close()


def test_measure_latency_of_a_bounce_played_through_a_take():
    """a bounced stem's mid goes out and comes back 75 frames later into a mono take: measure_latency finds the 75"""
    spec = synth.make_session("alnlat", 3, n_blocks=6, block=128, seed=0xA117E)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=8)
    lo, hi = BU.bounce_range(spec, 5)
    ids, nb = eng.bounce(lo, hi, [("track", 1, "pre")])
    stem = [np.ascontiguousarray(p) for p in eng.bounce_download(ids[0], nb)]
    assert np.any(np.stack(stem) != 0.0) and len(stem) == 2
    mid = (0.5 * (stem[0].astype(np.float64) + stem[1].astype(np.float64))).astype(np.float32)
    blocks = -(-(nb + 75) // spec.block)
    wire = np.concatenate([np.zeros(75, np.float32), mid, np.zeros(blocks * spec.block - nb - 75, np.float32)])
    eng.set_audio_channel_config(2, spec.channels, spec.block, rate)
    eng.set_track_input(0, "external_mono", 0, True)
    inp, out = W.AudioBuffer(spec.block, 2), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for k in range(blocks):
        inp.channel_buffers[0][:] = wire[k * spec.block:(k + 1) * spec.block]
        inp.channel_buffers[1][:] = 0.0
        eng.process(inp, out, float(rate))
    frames = eng.record_info(0)["frames"]
    eng.stop_record()
    eng.stop()
    take = max(c[5] for c in eng.clips(eng.tracks[0]))
    assert frames == len(wire)
    assert eng.measure_latency(ids[0], take, 128, played_frames=nb, recorded_frames=frames) == 75
    info, _ = eng.align_samples(ids[0], take, 0, 128, ref_frames=nb, frames=frames)
    want, _ = M.align_clips(stem, 0, nb & ~7, [wire], 0, frames, 0, 128)
    assert same_info(info, want) is None and abs(info["confidence"] - 1.0) < 1e-15
    eng.close()


def test_cpp_adapter_aligns_a_take_with_itself(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::align_samples; info and the curve
    equal the model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_align")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_align.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "align.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    m = 5 * 512
    g = np.arange(m, dtype=np.uint64)
    x = ((((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(256.0) - np.float32(0.5)).astype(np.float32)
    want, want_curve = M.align_clips([x], 256, 1024, [x], 0, m, -300, 300)
    raw = open(dump, "rb").read()
    ai = _ffi.AlignInfo.from_buffer_copy(raw[:80])
    got = {k: getattr(ai, k) for k in M.INFO_FIELDS}
    curve = np.frombuffer(raw[80:], dtype=M.CURVE_DTYPE)
    assert "adapter align ok lag 256" in out, out
    assert same_info(got, want) is None and same_curve(curve, want_curve) is None and want["lag"] == 256


# ---- 4: beside the audio thread -------------------------------------------------------------------------------------------------
def test_align_beside_the_audio_thread():
    """The shape of the spectrum call's test (test_gpu_spectrum.py): clips far behind the played range name the reference
    sample AND the sample to be aligned while the threads run, so a delete of either can never succeed — between two calls it
    is refused for the clip (-4), inside one for the pin (-3, asked first) — one thread deletes the two in turn without pause
    while the other aligns until deletes of both have been refused for the pin: a sample deleted during the call survives it.
    The master is what it is without the calls, and the last curve equals the model's at sampled lags."""
    NB, FR, WAIT, CALLS = 200, 1 << 21, 60.0, 96
    n, lo, hi = 1 << 20, -(1 << 14), (1 << 14) - 1
    spec = synth.make_session("alnthr", 2, n_blocks=NB, block=128, seed=0xA17712)
    pa, pb = [noise(FR, 95), noise(FR, 96)], [noise(FR, 97)]

    def with_big(eng):                                            # the same session in both runs
        sa, sb = eng.add_sample("f32", 44100, pa), eng.add_sample("f32", 44100, pb)
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sa, 1.0, 1.0)
        eng.add_audio_clip(eng.tracks[1], "far too", 1000.0, 1001.0, 0.0, sb, 1.0, 1.0)
        return sa, sb

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
    sa, sb = with_big(eng)
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), {sa: threading.Event(), sb: threading.Event()}
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        turn = 0
        while not finished.is_set() and time.monotonic() < end:
            which = (sa, sb)[turn % 2]
            turn += 1
            st = L.wbx_engine_delete_sample(eng.h, which)
            key_ = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key_] = seen.get(key_, 0) + 1
            if st == -3:
                refused[which].set()

    def aligner():
        try:
            began.set()
            while results["calls"] < CALLS and not (refused[sa].is_set() and refused[sb].is_set()):
                results["info"], results["curve"] = eng.align_samples(sa, sb, lo, hi, n_frames=n, a_first=70000, b_first=5, m_frames=FR - 8,
                                                                      curve=True)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (aligner, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("align calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused[sa].is_set() and refused[sb].is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read live clips: the curve is the model's, bit for bit (lags are independent: a sample of them)
    lags = hi - lo + 1
    some = sorted({0, 1, 4095, 4096, lags // 3, lags // 2, lags - 2, lags - 1})
    _, want = M.align_clips(pa, 70000, n, pb, 5, FR - 8, lo, hi, only=[lo + q for q in some])
    assert results["info"]["lags"] == lags and results["info"]["launches"] == L.wbx_align_launches(n, lags) == 2 * 4 + 2
    assert same_curve(np.ascontiguousarray(results["curve"][some]), want) is None
    picked = M.pick(results["curve"]["r"], results["curve"]["energy"], lo, M.ref_energy(M.detector_of(pa, 70000, n)))
    assert same_info(results["info"], picked) is None
    # afterwards: no pin is left (the clips are what refuses now), and with the clips gone the deletes succeed
    for which, track in ((sa, 0), (sb, 1)):
        assert L.wbx_engine_delete_sample(eng.h, which) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
        eng.delete_clip(eng.tracks[track], len(eng.clips(eng.tracks[track])) - 1)
        assert L.wbx_engine_delete_sample(eng.h, which) == 0
    eng.close()
