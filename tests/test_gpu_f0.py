"""wbx_clip_f0 and wbx_engine_f0_sample on the device.  The records are compared BIT FOR BIT with tests/f0_model.py: period, dip
and energy as their 64-bit patterns, lag, voiced and the info exactly.  Sizes are the smallest at which the kernel can still
go wrong: windows of 64, 72 and 256 frames; lag bounds that fill a fraction of one wave, cross a wave's 512 lags and meet every
number of waves per hop (1, 2, 4, 8); hop lengths that make hops share a staged span (1, 7, 64, 1000) and that leave gaps
between the hops; 0, 1, 2, 8, 9 and 17 hops with ragged ends.  In that matrix every workgroup has its full 512 lanes; hop lengths
of 2000 to 14 000 frames, whose shared span does not fit the budget so that a workgroup takes 4, 2 or 1 hops and has 256, 128 or
64 lanes, have a test of their own — and, once each, the largest span (W = 8192, tau_max = 4095) and a call across a launch
bound that ends in a launch and a workgroup that are not full."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import f0_model as M
import pitch_model as PM
import resample_model as RS
import stretch_model as ST
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 24000
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
TAU_MAX = [8, 15, 63, 511, 512, 513, 1023, 1024, 2047, 4095]
HOP_COUNTS = [0, 1, 2, 8, 9, 17]


def source(channels, n=SRC_LEN, seed=0xF0):
    """two tones per channel (the channels at different periods), switching pitch mid-range, and a little seeded noise"""
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n, dtype=np.float64)
    out = []
    for c in range(channels):
        p1 = np.where(i < n // 2, 41.7 + 9 * c, 67.3 + 5 * c)
        v = 0.6 * np.sin(2 * np.pi * i / p1) + 0.25 * np.sin(2 * np.pi * i / (13.1 + c)) + 0.02 * rng.standard_normal(n)
        out.append(v.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
    yield c
    c.close()


def same(got, want):
    """None, or the first record that differs in a bit"""
    assert got.dtype == want.dtype == M.DTYPE and W.F0_DTYPE == M.DTYPE
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint64).reshape(-1, 4) != want.view(np.uint64).reshape(-1, 4))
    if bad.size:
        h = int(bad[0]) // 4
        return (h, got[h], want[h], int(bad.size))
    return None


def launches_of(hops, Wn, tau_max):
    return M.launches(hops, Wn, tau_max, int(W.lib().wbx_f0_launch_terms()))


def run_and_check(c, clip, planes, first, n, Wn, H, tau_min, tau_max, thr=0.15):
    want, want_info = M.f0_clip(planes, first, n, Wn, H, tau_min, tau_max, thr)
    got, info = c.clip_f0(clip, first, n, Wn, H, tau_min, tau_max, thr)
    where = (len(planes), first, n, Wn, H, tau_min, tau_max, thr)
    assert same(got, want) is None, (where, same(got, want))
    assert info == dict(want_info, launches=launches_of(want_info["hops"], Wn, tau_max)), (where, info, want_info)
    return got, info


def length_for(hops, Wn, H, tau_max, ragged):
    """a range of exactly `hops` complete frames, with up to H - 1 frames behind the last one"""
    if hops == 0:
        return Wn + tau_max - 1
    return Wn + tau_max + (hops - 1) * H + (ragged % H)


# ---- 1: the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau_max", TAU_MAX)
@pytest.mark.parametrize("channels", [1, 2])
def test_f0_matrix(ctx, channels, tau_max):
    """every window and hop length at one lag bound; tau_min, the number of hops, the ragged end and the range's place take
    turns.  The range starts inside the clip and, at the odd places, ends on its last frame"""
    seen_hops, voiced = set(), 0
    cases = [(Wn, H) for Wn in (64, 72, 256) for H in (1, 7, 64, 1000, None)]
    for i, (Wn, H) in enumerate(cases):
        H = Wn + tau_max + 5 if H is None else H
        k = (i + TAU_MAX.index(tau_max)) % len(HOP_COUNTS)
        hops = HOP_COUNTS[k]
        n = length_for(hops, Wn, H, tau_max, 3 * i + 1)
        if n > SRC_LEN - 7:                                     # (17 hops that do not overlap, under the widest lag bound)
            hops = (SRC_LEN - 7 - Wn - tau_max) // H + 1
            n = length_for(hops, Wn, H, tau_max, 0)
        tau_min = 2 if i % 2 else tau_max - 1
        first = SRC_LEN - n if i % 2 else (5, 0, 64)[i % 3]
        thr = (0.15, 0.4, 1.0)[i % 3]
        got, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, Wn, H, tau_min, tau_max, thr)
        assert info["hops"] == hops == len(got)
        seen_hops.add(hops)
        voiced += info["voiced_hops"]
    assert len(seen_hops) >= 5 and (voiced > 0 or tau_max < 63)


@pytest.mark.parametrize("hops", HOP_COUNTS)
def test_hop_counts_at_the_clips_first_and_last_frame(ctx, hops):
    """every number of hops at a lag bound that takes two waves per hop, the range at the clip's first frame and ending on
    its last, with a ragged end"""
    for first_of in (lambda n: 0, lambda n: SRC_LEN - n):
        for Wn, H, tau_max in ((64, 7, 600), (256, 64, 63), (72, 1000, 1023)):
            n = length_for(hops, Wn, H, tau_max, 5)
            got, _ = run_and_check(ctx, SRC[2], ctx.src[2], first_of(n), n, Wn, H, 20, tau_max)
            assert len(got) == hops


def shape_of(Wn, H, tau_max):
    """wbx_f0.h's f0_shape: (G, F) — waves per hop, hops per workgroup"""
    waves, G = -(-(tau_max + 1) // 512), 1
    while G < waves:
        G *= 2
    F = 8 // G
    while F > 1 and (F - 1) * H + Wn + 512 * G + 16 > 14336:
        F //= 2
    return G, F


# (W, tau_max, H, hops) -> the (G, F) it must reach: fewer hops per workgroup than 8 / G, and a last workgroup that is not full
HALVED = [((256, 511, 2000, 9), (1, 4)), ((256, 511, 2001, 7), (1, 4)), ((256, 511, 5000, 5), (1, 2)), ((72, 63, 5001, 3), (1, 2)),
          ((256, 511, 13600, 3), (1, 1)), ((64, 8, 13999, 2), (1, 1)), ((256, 1023, 5000, 5), (2, 2)), ((256, 1023, 4999, 3), (2, 2)),
          ((256, 1023, 14000, 3), (2, 1)), ((256, 1500, 13000, 3), (4, 1)), ((72, 2047, 13001, 3), (4, 1)),
          ((8192, 511, 2000, 5), (1, 2)), ((8192, 1023, 4000, 3), (2, 2)), ((8192, 1023, 6000, 3), (2, 1))]


@pytest.mark.parametrize("channels", [1, 2])
def test_hops_per_workgroup_halved(channels):
    """hop lengths whose shared span does not fit the budget: a workgroup takes 4, 2 or 1 hops (256, 128 or 64 lanes at one
    wave per hop; 256 at two and four waves per hop), with hop lengths that are and are not a multiple of 4 and a number of
    hops that leaves the last workgroup short"""
    c = W.MixContext(4, block=128)
    n_all = 48000
    planes = source(channels, n_all, seed=0x4A1)
    c.clip_upload(1, "f32", RATE, planes)
    seen = set()
    for i, ((Wn, tau_max, H, hops), want_shape) in enumerate(HALVED):
        G, F = shape_of(Wn, H, tau_max)
        assert (G, F) == want_shape and F < 8 // G, (Wn, tau_max, H, G, F)
        assert hops % F or F == 1
        n = length_for(hops, Wn, H, tau_max, 3 * i + 1)
        assert n <= n_all
        first = n_all - n if i % 2 else 3
        got, info = run_and_check(c, 1, planes, first, n, Wn, H, (2, 7, tau_max - 1)[i % 3], tau_max, (0.15, 0.5)[i % 2])
        assert info["hops"] == hops and info["launches"] == 1
        seen.add((G, F, H % 4 == 0))
    assert {(1, 4, True), (1, 4, False), (1, 2, True), (1, 2, False), (1, 1, True), (1, 1, False), (2, 2, True), (2, 2, False),
            (2, 1, True), (4, 1, True), (4, 1, False)} <= seen
    c.close()


# ---- 2: the material ----------------------------------------------------------------------------------------------------------
def test_noise_silence_tiny_and_huge_samples():
    """noise and silence (unvoiced), a tone 2^-100 in size (voiced: nothing underflows), full-scale +-3.4e38 samples (nothing
    overflows), each mono and stereo"""
    c = W.MixContext(4, block=128)
    n = 3000
    rng = np.random.default_rng(0xF011)
    i = np.arange(n, dtype=np.float64)
    tone = np.sin(2 * np.pi * i / 57.3)
    big = np.float32(3.4e38)
    material = {
        "noise": [rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)],
        "silence": [np.zeros(n, dtype=np.float32)] * 2,
        "tiny": [(tone * 2.0 ** -100).astype(np.float32), (np.roll(tone, 3) * 2.0 ** -100).astype(np.float32)],
        "huge": [np.where(tone >= 0, big, -big).astype(np.float32), np.where(np.roll(tone, 5) >= 0, big, -big).astype(np.float32)],
        "huge-noise": [(big * np.sign(rng.standard_normal(n))).astype(np.float32), np.full(n, big, dtype=np.float32)],
    }
    for k, (name, planes) in enumerate(material.items()):
        for ch in (1, 2):
            clip = 10 + 2 * k + ch
            c.clip_upload(clip, "f32", RATE, planes[:ch])
            for Wn, H, tau_max in ((256, 64, 511), (64, 7, 1023)):
                got, info = run_and_check(c, clip, planes[:ch], 0, n, Wn, H, 8, tau_max)
                assert np.all(np.isfinite(got["period"])) and np.all(np.isfinite(got["dip"])) and np.all(np.isfinite(got["energy"]))
                if name in ("noise", "silence"):
                    assert info["voiced_hops"] == 0, name
                if name == "silence":
                    assert np.all(got["lag"] == 8) and np.all(got["period"] == 8.0) and np.all(got["dip"] == 1.0) and np.all(got["energy"] == 0.0)
                if name == "tiny":
                    assert info["voiced_hops"] == info["hops"] and np.all(got["energy"] > 0.0), name
    c.close()


def test_non_finite_samples_inside_and_loud_neighbours_outside():
    """NaN and +-inf inside the range enter as 0.0; NaNs and loud samples beside the range — in the clip and in the pool's
    neighbouring clips — have no influence: the records equal those of the same range in a clip of its own"""
    c = W.MixContext(4, block=128)
    n_all, first, n = 5000, 700, 3001
    quiet = source(2, n_all, seed=0x51)
    for p in quiet:
        p[[first, first + 1, first + 999, first + n - 1]] = [np.nan, np.inf, -np.inf, np.nan]
    loud = [p.copy() for p in quiet]
    for p in loud:
        p[:first] = np.float32(3e38)
        p[first - 1] = np.nan
        p[first + n:] = np.nan
        p[first + n + 1::2] = np.float32(-3e38)
    hot = [np.full(4096, np.nan, dtype=np.float32), np.full(4096, 3e38, dtype=np.float32)]
    c.clip_upload(1, "f32", RATE, hot)                          # neighbours in the pool on both sides
    c.clip_upload(2, "f32", RATE, loud)
    c.clip_upload(3, "f32", RATE, hot)
    c.clip_upload(4, "f32", RATE, [p[first:first + n] for p in quiet])
    for ch_clip, planes, at in ((2, loud, first), (4, [p[first:first + n] for p in quiet], 0)):
        for Wn, H, tau_max in ((256, 64, 600), (72, 7, 63), (64, 1000, 2100)):
            got, _ = run_and_check(c, ch_clip, planes, at, n, Wn, H, 9, tau_max)
            alone, _ = M.f0_clip([p[first:first + n] for p in quiet], 0, n, Wn, H, 9, tau_max, 0.15)
            assert same(got, alone) is None
    c.close()


# ---- 3: the largest span, a launch's seam ---------------------------------------------------------------------------------------
def test_the_largest_window_and_lag_bound(ctx):
    """W = 8192, tau_max = 4095: 12 288 staged words and 8 waves per hop; 3 hops, H = 1000"""
    n = 8192 + 4095 + 2 * 1000 + 17
    got, info = run_and_check(ctx, SRC[2], ctx.src[2], 3, n, 8192, 1000, 30, 4095)
    assert info["hops"] == 3 and info["launches"] == 1


def test_a_call_across_launch_bounds():
    """a range of more hops than two launches take, at H = 1 and the smallest window and lag bound (of at most four waves
    per hop) at which a call of at most 2^20 hops holds them (read from the getters): two full launches and a third of 11
    hops, which is no multiple of the hops a workgroup takes.  The model is evaluated for the hops either side of every
    seam, for the first and for the last hops — hops are independent"""
    L = W.lib()
    H = 1
    for Wn, tau_max in ((64, 8), (64, 63), (64, 511), (72, 1023), (256, 1023), (2048, 1023), (8192, 1023), (8192, 4095)):
        per = L.wbx_f0_launch_hops(Wn, tau_max)
        assert per == M.launch_hops(Wn, tau_max, L.wbx_f0_launch_terms()) and per >= 1
        if 2 * per + 11 <= 1 << 20:
            break
    assert 2 * per + 11 <= 1 << 20, "no shape whose launches a call of 2^20 hops can cross"
    hops = 2 * per + 11                                         # the third launch has 11 hops: its last workgroup is not full
    G, F = shape_of(Wn, H, tau_max)
    assert F > 1 and 11 % F and per % F == 0
    n = Wn + tau_max + (hops - 1) * H
    c = W.MixContext(4, block=128)
    planes = source(1, n + 5, seed=0x5EA)
    c.clip_upload(1, "f32", RATE, planes)
    got, info = c.clip_f0(1, 2, n, Wn, H, 2, tau_max, 0.3)
    seams = sorted({h for s in range(per, hops, per) for h in (s - 2, s - 1, s, s + 1)} | {0, 1} | set(range(hops - 11, hops)))
    want, want_info = M.f0_clip(planes, 2, n, Wn, H, 2, tau_max, 0.3, only=seams)
    assert info["hops"] == hops == want_info["hops"] == len(got) and info["terms"] == want_info["terms"]
    assert info["launches"] == -(-hops // per) == 3
    assert same(np.ascontiguousarray(got[seams]), want) is None
    assert info["voiced_hops"] == int(got["voiced"].sum())
    c.close()


# ---- 4: refusals, the pool, the timer ---------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_pool_and_frames_out_alone(ctx):
    L = W.lib()
    ctx.clip_upload(60, "i16", RATE, [np.arange(4000, dtype=np.int16)] * 2)
    S = SRC[2]
    rec = np.zeros(64, dtype=M.DTYPE)
    rec["lag"] = 9
    fi = _ffi.F0Info()

    def refused(status, why, clip=S, first=0, n=2000, Wn=256, H=64, tau_min=8, tau_max=511, thr=0.15, cap=64, out=True):
        before = ctx.pool_stats()
        fi.hops = 777
        got = L.wbx_clip_f0(ctx.h, clip, first, n, Wn, H, tau_min, tau_max, thr, rec.ctypes.data if out else None, cap, C.byref(fi))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert got == M.check(n, Wn, H, tau_min, tau_max, thr, out, cap) or b"clip" in msg[8:]
        assert ctx.pool_stats() == before and fi.hops == 777 and np.all(rec["lag"] == 9) and not rec["period"].any()

    refused(-4, b"unknown clip", clip=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16)
    for Wn in (0, 56, 68, 8200, 8192 + 8):
        refused(-4, b"window_frames", Wn=Wn)
    for tau_max in (7, 4096):
        refused(-4, b"tau_max", tau_max=tau_max)
    for tau_min in (0, 1, 511, 600):
        refused(-4, b"tau_min", tau_min=tau_min)
    for H in (0, (1 << 20) + 1):
        refused(-4, b"hop_frames", H=H)
    for thr in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        refused(-4, b"threshold", thr=thr)
    refused(-4, b"frames_out is NULL", out=False)
    refused(-4, b"frames_cap", cap=19)                          # (2000 - 767) // 64 + 1 = 20 hops: short by one
    refused(-3, b"2^20 hops", n=64 + 8 + (1 << 20), Wn=64, H=1, tau_min=2, tau_max=8, cap=(1 << 20) + 1)   # max + 1 hops
    refused(-4, b"frames_cap", n=64 + 8 + (1 << 20), Wn=64, H=1, tau_min=2, tau_max=8, cap=1 << 20)      # ... asked first
    refused(-3, b"not F32", clip=60)
    refused(-4, b"window_frames", clip=60, Wn=68)               # the sizes are judged before the clip is looked at
    refused(-4, b"past the clip", first=SRC_LEN - 1999)
    refused(-4, b"past the clip", first=(1 << 64) - 1, n=2000)  # a sum that wraps
    refused(-4, b"past the clip", n=64 + 8 + (1 << 20) - 1, Wn=64, H=1, tau_min=2, tau_max=8, cap=1 << 20)   # max hops pass, the clip does not
    # Python's wrapper asks wbx_f0_check before it allocates the records: 2^31 hops are refused without 64 GB
    with pytest.raises(W.WbxError) as err:
        ctx.clip_f0(S, 0, (1 << 31) - 17, 64, 1, 2, 8)
    assert err.value.status == -3
    # what is not refused: no hops and no buffer, a capacity that is just enough
    assert L.wbx_clip_f0(ctx.h, S, 0, 766, 256, 64, 8, 511, 0.15, None, 0, C.byref(fi)) == 0
    assert (fi.hops, fi.voiced_hops, fi.terms, fi.launches) == (0, 0, 0, 0)
    assert L.wbx_clip_f0(ctx.h, S, 0, 2000, 256, 64, 8, 511, 1.0, rec.ctypes.data, 20, None) == 0
    assert np.all(rec["lag"][:20] != 9) and np.all(rec["lag"][20:] == 9)


def test_the_pool_is_unchanged_and_the_timers_keep_apart():
    """a call allocates nothing in the pool; wbx_f0_ms works; a call between a stretch and a pitch call leaves their
    results and their timers undisturbed"""
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_f0_ms(c.h, C.byref(out)) == -4 and out.value == 7.0          # none yet
    assert c.L.wbx_f0_ms(c.h, None) == -4 and c.L.wbx_f0_ms(None, C.byref(out)) == -4
    planes = source(1, 5000, seed=3)
    c.clip_upload(1, "f32", RATE, planes)
    c.clip_stretch(1, 3, 0, 5000, 7500, 256, 96)
    assert c.L.wbx_f0_ms(c.h, C.byref(out)) == -4                                # a stretch is no f0 call
    stretch_ms = c.stretch_ms()
    base = c.pool_stats()
    run_and_check(c, 1, planes, 0, 5000, 256, 64, 8, 600)
    assert c.pool_stats() == base
    f0_ms = c.f0_ms()
    assert 0.0 < f0_ms < 1000.0 and c.stretch_ms() == stretch_ms
    pit_want, _, _ = PM.pitch_clip(planes, 0, 5000, 5000, 3, 2, RS.GOOD, 64, 24)
    str_want, _, _ = ST.stretch_clip(planes, 0, 5000, 3333, 256, 96)
    c.clip_stretch(1, 5, 0, 5000, 3333, 256, 96)
    stretch_ms = c.stretch_ms()
    run_and_check(c, 1, planes, 5, 4000, 72, 7, 2, 15)
    c.clip_pitch(1, 7, 0, 5000, 5000, 3, 2, "good", 64, 24)
    pitch_ms = c.pitch_ms()
    base = c.pool_stats()
    run_and_check(c, 7, pit_want, 0, 5000, 64, 1000, 8, 1023)                    # ... of the pitch call's own result
    assert c.pool_stats() == base and c.stretch_ms() == stretch_ms and c.pitch_ms() == pitch_ms and c.f0_ms() != f0_ms
    for clip, n, want in ((5, 3333, str_want), (7, 5000, pit_want)):
        got = c.clip_download(clip, 0, n, np.float32)
        assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))
    c.close()


# ---- 5: through the engine, the adapter, Python's conveniences ----------------------------------------------------------------------
def harmonic_tone(hz, n, rate, harmonics=8):
    i = np.arange(n, dtype=np.float64)
    return (0.3 * sum(np.sin(2 * np.pi * hz * k * i / rate + k) / k for k in range(1, harmonics + 1))).astype(np.float32)


def test_f0_sample_detect_note_and_tune_sample():
    """wbx_engine_f0_sample equals the model; tune_sample on a 452 Hz 8-harmonic tone (46.6 cents above A4) yields a sample
    whose detect_note_sample lies within 1 cent of 440 Hz: pitch_ratio's documented 0.4 cent plus the 0.18 cent measured
    for the tracker on tones.  The model alone stays inside that for this input (tests/test_f0_host.py checks the tracker's
    part on 452 Hz itself)"""
    spec = synth.make_session("f0e", 2, n_blocks=2, block=128, seed=0xF0E)
    rate = spec.sample_rate
    eng = build_engine(spec, max_blocks=2)
    n = 24000
    tone = harmonic_tone(452.0, n, rate)
    planes = [tone, np.roll(tone, 1)]
    s = eng.add_sample("f32", rate, planes)
    rec, info = eng.f0_sample(s, 1024, 256, 24, 1024, 0.15, first_frame=7, n_frames=n - 9)
    want, want_info = M.f0_clip(planes, 7, n - 9, 1024, 256, 24, 1024, 0.15)
    assert same(rec, want) is None and {k: info[k] for k in want_info} == want_info and info["voiced_hops"] == info["hops"] > 80
    note = eng.detect_note_sample(s)
    print("detected", note)
    assert note["midi"] == 69 and abs(note["cents"] - 1200.0 * np.log2(452.0 / 440.0)) < 0.2 and note["voiced"] == 1.0
    assert abs(1200.0 * np.log2(note["hz"] / 452.0)) < 0.2
    new, pinfo, seen = eng.tune_sample(s)
    assert seen == note and eng._sample_shape[new] == (n, 2)
    tuned = eng.detect_note_sample(new)
    off = 1200.0 * np.log2(tuned["hz"] / 440.0)
    print("tuned", tuned, "cents off 440 Hz: %.4f" % off, "ratio %d/%d" % (pinfo["M"], pinfo["L"]))
    assert abs(off) <= 1.0 and tuned["midi"] == 69
    up, _, _ = eng.tune_sample(s, to_midi=71)
    assert abs(1200.0 * np.log2(eng.detect_note_sample(up)["hz"] / (440.0 * 2.0 ** (2.0 / 12.0)))) <= 1.0
    # no voiced hop: nothing to tune; already in tune: a ratio of 1
    quiet = eng.add_sample("f32", rate, [np.zeros(6000, dtype=np.float32)])
    assert eng.detect_note_sample(quiet)["hz"] is None and eng.detect_note_sample(quiet)["voiced"] == 0.0
    with pytest.raises(ValueError):
        eng.tune_sample(quiet)
    with pytest.raises(ValueError):
        eng.tune_sample(eng.add_sample("f32", rate, [harmonic_tone(440.0, 12000, rate)]))
    # refusals through layer 2
    L, fi = W.lib(), _ffi.F0Info()
    buf = np.zeros(128, dtype=M.DTYPE)
    call = lambda smp, nn, Wn=1024, out=buf.ctypes.data, cap=128: L.wbx_engine_f0_sample(eng.h, smp, 0, nn, Wn, 256, 24, 1024, 0.15, out, cap,
                                                                                     C.byref(fi))
    assert call(9999, 4000) == -4 and call(s, n + 1) == -4 and call(s, 0) == -4 and call(s, 4000, Wn=1004) == -4
    assert call(s, 4000, out=None) == -4 and call(s, 4000, cap=7) == -4 and not buf["period"].any()
    assert call(s, 4000, cap=8) == 0 and fi.hops == 8 and buf["period"][:8].all() and not buf["period"][8:].any()
    assert L.wbx_engine_f0_sample(None, s, 0, 4000, 1024, 256, 24, 1024, 0.15, buf.ctypes.data, 128, None) == -4
    eng.close()


def test_cpp_adapter_tracks_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::f0_sample; the records equal the
    model's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_f0")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_f0.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "f0.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n = 5 * 512
    g = np.arange(n, dtype=np.uint64)
    ph = g % 50
    tri = np.where(ph < 25, ph, 50 - ph).astype(np.float32) / np.float32(32.0) - np.float32(0.375)
    x = (tri + (((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(4096.0)).astype(np.float32)
    want, info = M.f0_clip([x], 0, n, 256, 64, 8, 255, 0.2)
    got = np.fromfile(dump, dtype=M.DTYPE)
    assert "adapter f0 ok %d hops %d voiced" % (info["hops"], info["voiced_hops"]) in out, out
    assert same(got, want) is None and info["voiced_hops"] > 0
    assert np.all(np.abs(got["period"][got["voiced"] != 0] - 50.0) < 0.5)


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_f0_beside_the_audio_thread():
    """The shape of the pitch call's test (test_gpu_pitch.py): a clip far behind the played range names the big sample while
    the threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one
    for the pin (-3, asked first) — one thread deletes without pause while the other tracks until a delete has been refused
    for the pin.  The master is what it is without the calls, and the last records equal the model's at sampled hops."""
    NB, FR, WAIT, CALLS = 300, 1 << 21, 60.0, 96
    Wn, H, tau_min, tau_max = 2048, 64, 24, 1023
    spec = synth.make_session("f0thr", 2, n_blocks=NB, block=128, seed=0xF07712)
    planes = source(2, FR, seed=41)

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

    def tracker():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["rec"], results["info"] = eng.f0_sample(big, Wn, H, tau_min, tau_max, 0.15, first_frame=first, n_frames=n,
                                                                channels=2, frames=FR)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (tracker, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("f0 calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read a live clip: the records are the model's, bit for bit (hops are independent: a sample of them)
    hops = M.hops(n, Wn, H, tau_max)
    some = sorted({0, 1, 7, 8, hops // 3, hops // 2, hops - 9, hops - 2, hops - 1})
    want, want_info = M.f0_clip(planes, first, n, Wn, H, tau_min, tau_max, 0.15, only=some)
    assert results["info"]["hops"] == hops == want_info["hops"] and results["info"]["terms"] == want_info["terms"]
    assert same(np.ascontiguousarray(results["rec"][some]), want) is None
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
