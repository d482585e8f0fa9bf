"""wbx_clip_onsets, wbx_clip_tempo and their engine twins on the device.  The records are compared BIT FOR BIT with
tests/onset_model.py — energy, edge_energy and novelty as their 64-bit patterns, onset and the info exactly — and the tempo
records with tests/f0_model.py's track over the model's novelty.  Sizes are the smallest at which the kernels can still go
wrong: hop lengths of 64, 128 and 256 frames (a lane reads its run of 1, 2 or 4 frames directly, as one load where the range
starts on that many bytes and word by word where it does not), 192 and 320 (the LDS chunk with an odd run of 3 and 5), 1024
(a run of 16), 2112 (two chunks, the second a single column), 4160 (three, the last a single column) and 16384 (eight
chunks); 0 to 70 hops with ragged tails that must not be read; more hops than one pass of the grid takes."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import f0_model as F0
import onset_model as M
import stretch_model as ST
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
HOPS = [64, 128, 192, 256, 320, 1024, 2112, 4160, 16384]
HOP_COUNTS = [0, 1, 2, 3, 4, 5, 9, 63, 64, 65, 70]
SRC_LEN = 8200 * 320                                            # more hops than the grid takes at once, at the LDS instance's H = 320
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
PICK = dict(floor_power=1e-9, threshold=0.3, delta=0.1, w=3, a=8)
TEMPO_BOUND = 2 * 0.00203                                       # tests/test_onsets_host.py's: twice the model's worst error


def source(channels, n=SRC_LEN, seed=0x0A5E7):
    """noise bursts of several lengths and levels over a tone and a noise floor, the channels different"""
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n, dtype=np.float64)
    out = []
    for c in range(channels):
        env = np.full(n, 0.01)
        for period, width, level in ((1531 + 97 * c, 200, 0.5), (40009, 3000, 0.9), (333333, 20000, 0.3)):
            env = np.where((i + 17 * c) % period < width, level, env)
        v = env * rng.standard_normal(n) + 0.05 * np.sin(2 * np.pi * i / (91.3 + c))
        out.append(v.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
        for p in c.src[ch]:
            p.setflags(write=False)
    yield c
    c.close()


def same(got, want, dtype=M.DTYPE):
    """None, or the first record that differs in a bit"""
    assert got.dtype == want.dtype == dtype
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint64).reshape(-1, 4) != want.view(np.uint64).reshape(-1, 4))
    if bad.size:
        h = int(bad[0]) // 4
        return (h, got[h], want[h], int(bad.size))
    return None


def run_and_check(c, clip, planes, first, n, H, **pick):
    pick = dict(PICK, **pick)
    want, want_info = M.onsets_clip(planes, first, n, H, **pick)
    got, info = c.clip_onsets(clip, first, n, H, **pick)
    where = (len(planes), first, n, H, pick)
    assert same(got, want) is None, (where, same(got, want))
    assert info == want_info, (where, info, want_info)
    return got, info


def tempo_and_check(c, clip, planes, first, n, H, Wn, step, lo, hi, thr=0.5, floor_power=1e-9):
    want, want_info = M.tempo_clip(planes, first, n, H, floor_power, Wn, step, lo, hi, thr)
    got, info = c.clip_tempo(clip, first, n, H, floor_power, Wn, step, lo, hi, thr)
    where = (len(planes), first, n, H, Wn, step, lo, hi, thr)
    assert same(got, want, F0.DTYPE) is None, (where, same(got, want, F0.DTYPE))
    assert {k: info[k] for k in want_info} == want_info and info["launches"] == (1 if want_info["hops"] else 0), (where, info, want_info)
    return got, info


# ---- 1: the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HOPS)
@pytest.mark.parametrize("channels", [1, 2])
def test_onset_matrix(ctx, channels, H):
    """every number of hops at one hop length; the ragged tail and the range's place — on and off 16, 8 and 4 bytes — take
    turns.  At the odd turns the range ends on the clip's last frame"""
    onsets = 0
    for i, hops in enumerate(HOP_COUNTS):
        n = hops * H + (0, 1, H - 1, H // 2 + 3)[i % 4]
        first = SRC_LEN - n if i % 2 else (0, 5, 4, 2, 8, 1)[(i // 2) % 6]
        if n == 0:
            n = 1                                               # (no frames is a refusal; one frame is no hop)
        got, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, H)
        assert info["hops"] == hops == len(got)
        onsets += info["onsets"]
    assert onsets > 0


@pytest.mark.parametrize("channels", [1, 2])
def test_more_hops_than_one_pass_of_the_grid(ctx, channels):
    """the grid has at most 2048 workgroups of 4 waves: 8192 hops in flight, four times that where a wave asks for four hops
    at once.  9000 and 8192 + 5 hops through the LDS chunk; 40 000, 32 768 + 3 and 17 000 hops read directly (the last leaves
    waves with one, two and three of their four hops)"""
    planes = ctx.src[channels]
    for H, hops, first in ((192, 9000, 3), (320, 8197, 0), (64, 40000, 0), (64, 32771, 1), (128, 17000, 6), (256, 8200, 4)):
        n = hops * H + 7
        assert first + n <= SRC_LEN
        got, info = run_and_check(ctx, SRC[channels], planes, first, n, H)
        assert info["hops"] == hops and info["onsets"] > 0


# ---- 2: what is never read, the material ------------------------------------------------------------------------------------------
def test_frames_beside_the_range_are_never_read():
    """first_frame > 0 with a sample of 3.4e38 and a NaN immediately before and after the range, and hot neighbours in the
    pool: the records equal those of the same frames in a clip of their own, which pins d[-1] = 0 and the unread tail"""
    c = W.MixContext(4, block=128)
    n_all = 40000
    quiet = source(2, n_all, seed=0x51)
    hot = [np.full(4096, np.nan, dtype=np.float32), np.full(4096, 3.4e38, dtype=np.float32)]
    c.clip_upload(1, "f32", RATE, hot)                          # neighbours in the pool on both sides
    slot = 2
    for first, n in ((700, 30001), (701, 30333), (4, 32 * 320 + 319), (8, 2 * 16384 + 100)):
        for before, after in ((3.4e38, np.nan), (np.nan, -3.4e38)):
            loud = [p.copy() for p in quiet]
            for p in loud:
                p[:first] = np.float32(before)
                p[first - 1] = np.float32(before)
                p[first - 2] = np.float32(after)
                p[first + n:] = np.float32(after)
                p[first + n + 1::2] = np.float32(before)
            c.clip_upload(slot, "f32", RATE, loud)
            c.clip_upload(slot + 1, "f32", RATE, hot)
            c.clip_upload(slot + 2, "f32", RATE, [p[first:first + n] for p in quiet])
            for H in (64, 128, 256, 192, 320, 1024, 2112, 16384):
                got, _ = run_and_check(c, slot, loud, first, n, H)
                alone, _ = run_and_check(c, slot + 2, [p[first:first + n] for p in quiet], 0, n, H)
                assert same(got, alone) is None and len(got) == n // H
            slot += 3
    c.close()


def test_non_finite_huge_tiny_and_silent_material():
    """NaN and +-inf inside the range enter as 0.0; +-3.4e38 alternating keeps B finite; a tone of 2^-100 and silence"""
    c = W.MixContext(4, block=128)
    n = 20000
    rng = np.random.default_rng(0x0A5E)
    i = np.arange(n, dtype=np.float64)
    tone = np.sin(2 * np.pi * i / 57.3)
    big = np.float32(3.4e38)
    holes = source(2, n, seed=9)
    for p in holes:
        p[[0, 1, 63, 64, 999, 5000, 5001, n - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan]
        p[7000:7300] = np.nan
    alternating = np.where(np.arange(n) % 2 == 0, big, -big).astype(np.float32)
    material = {
        "holes": holes,
        "alternating": [alternating, alternating.copy()],
        "huge-noise": [(big * np.sign(rng.standard_normal(n))).astype(np.float32), np.full(n, big, dtype=np.float32)],
        "tiny": [(tone * 2.0 ** -100).astype(np.float32), (np.roll(tone, 3) * 2.0 ** -100).astype(np.float32)],
        "silence": [np.zeros(n, dtype=np.float32)] * 2,
    }
    for k, (name, planes) in enumerate(material.items()):
        for ch in (1, 2):
            clip = 10 + 2 * k + ch
            c.clip_upload(clip, "f32", RATE, planes[:ch])
            for H, first in ((64, 0), (256, 3), (320, 0), (1024, 1), (2112, 0)):
                got, info = run_and_check(c, clip, planes[:ch], first, n - first, H, floor_power=(1e-9, 1e-30, 1.0)[k % 3])
                assert np.all(np.isfinite(got["energy"])) and np.all(np.isfinite(got["edge_energy"])) and np.all(np.isfinite(got["novelty"]))
                assert np.all(got["novelty"] >= 0.0) and np.all(got["novelty"] <= 2.0)   # (2.0: both rises round to 1.0 over a vanishing floor)
                if name == "silence":
                    assert not got["novelty"].any() and not got["energy"].any() and info["onsets"] == 0
                if name == "alternating":
                    assert np.all(got["edge_energy"] > 1e77)
                if name == "tiny":
                    assert np.all(got["energy"] > 0.0) and np.all(got["energy"] < 1e-55)
    c.close()


def test_the_boundaries_of_the_pick(ctx):
    n, first = 200 * 256 + 9, 5
    for pick in (dict(threshold=2.0), dict(threshold=5e-324, delta=0.0), dict(delta=2.0), dict(delta=0.0, w=0, a=0), dict(w=64, a=256),
                 dict(w=0, a=256), dict(w=64, a=0), dict(threshold=0.05, delta=0.0, w=1, a=1), dict(floor_power=1.0), dict(floor_power=1e-30)):
        run_and_check(ctx, SRC[2], ctx.src[2], first, n, 256, **pick)
    got, info = run_and_check(ctx, SRC[1], ctx.src[1], first, n, 256, threshold=5e-324, delta=0.0, w=0, a=0)
    assert info["onsets"] == int((got["novelty"] > 0).sum()) > 20   # every hop that rises at all


# ---- 3: the tempo -------------------------------------------------------------------------------------------------------------
# (H, W, step, lag_min, lag_max): one, two, four and eight waves per tracked hop (f0_shape's G)
TEMPO_SHAPES = [(64, 64, 8, 8, 63), (64, 256, 64, 20, 600), (64, 72, 7, 9, 1100), (64, 64, 1000, 30, 2100)]


@pytest.mark.parametrize("shape", TEMPO_SHAPES)
def test_tempo_equals_the_track_of_the_models_novelty(ctx, shape):
    """hop counts just below window_hops + lag_max (no record), at it (one) and three steps and a ragged rest beyond, mono
    and stereo, the range on and off 4 bytes"""
    H, Wn, step, lo, hi = shape
    for k, hops in enumerate((Wn + hi - 1, Wn + hi, Wn + hi + 3 * step + (step // 2))):
        for ch in (1, 2):
            n, first = hops * H + 13 * k, (0, 3)[(k + ch) % 2]
            got, info = tempo_and_check(ctx, SRC[ch], ctx.src[ch], first, n, H, Wn, step, lo, hi, thr=(0.5, 0.15, 1.0)[k])
            assert info["hops"] == len(got) == (0, 1, 4)[k]
    got, info = ctx.clip_tempo(SRC[1], 0, H - 1, H, 1e-9, Wn, step, lo, hi, 0.5)    # no onset hop at all
    assert len(got) == 0 and info["hops"] == 0 and info["launches"] == 0


def test_a_tempo_call_between_an_f0_and_a_stretch_call_disturbs_neither():
    c = W.MixContext(4, block=128)
    planes = source(1, 70000, seed=3)
    c.clip_upload(1, "f32", RATE, planes)
    f0_before, _ = c.clip_f0(1, 0, 5000, 256, 64, 8, 600)
    c.clip_stretch(1, 3, 0, 5000, 7500, 256, 96)
    stretched = c.clip_download(3, 0, 7500, np.float32)
    stretch_ms = c.stretch_ms()
    out = C.c_double(7.0)
    assert c.L.wbx_onset_ms(c.h, C.byref(out)) == -4 and out.value == 7.0          # none yet: f0 and stretch are no onset calls
    base = c.pool_stats()
    tempo_and_check(c, 1, planes, 2, 64 * 900, 64, 256, 64, 20, 600)
    assert c.pool_stats() == base and 0.0 < c.onsets_ms() < 1000.0 and 0.0 < c.f0_ms() < 1000.0 and c.stretch_ms() == stretch_ms
    run_and_check(c, 1, planes, 0, 70000, 320)
    assert c.pool_stats() == base
    f0_after, _ = c.clip_f0(1, 0, 5000, 256, 64, 8, 600)
    assert same(f0_after, f0_before, F0.DTYPE) is None
    want, _, _ = ST.stretch_clip(planes, 0, 5000, 7500, 256, 96)
    c.clip_stretch(1, 5, 0, 5000, 7500, 256, 96)
    for clip in (3, 5):
        got = c.clip_download(clip, 0, 7500, np.float32)
        assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got.view(np.uint32), stretched.view(np.uint32))
    c.close()


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_pool_and_the_outputs_alone(ctx):
    L = W.lib()
    ctx.clip_upload(60, "i16", RATE, [np.arange(4000, dtype=np.int16)] * 2)
    S = SRC[2]
    rec = np.zeros(64, dtype=M.DTYPE)
    rec["onset"] = 9
    trk = np.zeros(64, dtype=F0.DTYPE)
    trk["lag"] = 9
    oi, fi = _ffi.OnsetInfo(), _ffi.F0Info()
    NAN = float("nan")

    def refused(status, why, clip=S, first=0, n=4000, H=256, fl=1e-9, thr=0.3, delta=0.1, w=3, a=8, cap=64, out=True):
        before = ctx.pool_stats()
        oi.hops = 777
        got = L.wbx_clip_onsets(ctx.h, clip, first, n, H, fl, thr, delta, w, a, rec.ctypes.data if out else None, cap, C.byref(oi))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert got == M.check(n, H, fl, thr, delta, w, a, out, cap) or b"clip" in msg[13:]
        assert ctx.pool_stats() == before and oi.hops == 777 and np.all(rec["onset"] == 9) and not rec["novelty"].any()

    def tempo_refused(status, why, clip=S, first=0, n=64 * 400, H=64, fl=1e-9, Wn=64, step=8, lo=8, hi=63, thr=0.5, cap=64, out=True):
        before = ctx.pool_stats()
        fi.hops = 777
        got = L.wbx_clip_tempo(ctx.h, clip, first, n, H, fl, Wn, step, lo, hi, thr, trk.ctypes.data if out else None, cap, C.byref(fi))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert got == M.tempo_check(n, H, fl, Wn, step, lo, hi, thr, out, cap) or b"clip" in msg[11:]
        assert ctx.pool_stats() == before and fi.hops == 777 and np.all(trk["lag"] == 9) and not trk["period"].any()

    refused(-4, b"unknown clip", clip=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16)
    for H in (0, 32, 65, 96, 16448):
        refused(-4, b"hop_frames", H=H)
    for fl in (0.0, 0.9e-30, 1.0000001, -1.0, NAN, float("inf")):
        refused(-4, b"floor_power", fl=fl)
    for thr in (0.0, -0.1, 2.0000001, NAN, float("inf")):
        refused(-4, b"threshold", thr=thr)
    for delta in (-1e-300, 2.0000001, NAN):
        refused(-4, b"delta", delta=delta)
    refused(-4, b"w above", w=65)
    refused(-4, b"a above", a=257)
    refused(-4, b"frames_out is NULL", out=False)
    refused(-4, b"frames_cap", cap=14)                          # 4000 // 256 = 15 hops: short by one
    refused(-3, b"2^20 hops", n=(64 << 20) + 64, H=64, cap=(1 << 20) + 1)   # max + 1 hops
    refused(-4, b"frames_cap", n=(64 << 20) + 64, H=64, cap=1 << 20)        # ... asked first
    refused(-3, b"not F32", clip=60)
    refused(-4, b"hop_frames", clip=60, H=100)                  # the sizes are judged before the clip is looked at
    refused(-4, b"past the clip", first=SRC_LEN - 3999)
    refused(-4, b"past the clip", first=(1 << 64) - 1)          # a sum that wraps
    refused(-4, b"past the clip", n=64 << 20, H=64, cap=1 << 20)   # max hops pass, the clip does not

    tempo_refused(-4, b"unknown clip", clip=999)
    tempo_refused(-4, b"no frames", n=0)
    tempo_refused(-4, b"2^31 - 16", n=(1 << 31) - 16)
    tempo_refused(-4, b"hop_frames", H=100)
    tempo_refused(-4, b"floor_power", fl=NAN)
    tempo_refused(-3, b"2^20 hops", n=(64 << 20) + 64, cap=1 << 21)
    tempo_refused(-3, b"2^20 hops", n=(64 << 20) + 64, Wn=68, cap=1 << 21)   # the onset arguments first
    tempo_refused(-4, b"window_frames", Wn=68)
    tempo_refused(-4, b"window_frames", Wn=68, n=63)            # no onset hop: the track's shape is judged all the same
    tempo_refused(-4, b"tau_max", hi=4096)
    tempo_refused(-4, b"tau_min", lo=63)
    tempo_refused(-4, b"hop_frames", step=0)
    for thr in (0.0, 1.0000001, NAN):
        tempo_refused(-4, b"threshold", thr=thr)
    tempo_refused(-4, b"frames_out is NULL", out=False)
    tempo_refused(-4, b"frames_cap", cap=34)                    # (400 - 127) // 8 + 1 = 35 windows: short by one
    tempo_refused(-3, b"not F32", clip=60)
    tempo_refused(-4, b"window_frames", clip=60, Wn=68)
    tempo_refused(-4, b"past the clip", first=SRC_LEN - 64 * 400 + 1)
    # Python's wrapper asks wbx_onset_check before it allocates the records
    with pytest.raises(W.WbxError) as err:
        ctx.clip_onsets(S, 0, (1 << 31) - 17, 64)
    assert err.value.status == -3
    # what is not refused: no hops and no buffer, a capacity that is just enough
    assert L.wbx_clip_onsets(ctx.h, S, 0, 255, 256, 1e-9, 0.3, 0.1, 3, 8, None, 0, C.byref(oi)) == 0
    assert (oi.hops, oi.onsets, oi.launches) == (0, 0, 0)
    assert L.wbx_clip_onsets(ctx.h, S, 0, 4000, 256, 1e-9, 0.3, 0.1, 3, 8, rec.ctypes.data, 15, None) == 0
    assert np.all(rec["onset"][:15] != 9) and np.all(rec["onset"][15:] == 9)
    assert L.wbx_clip_tempo(ctx.h, S, 0, 64 * 126, 64, 1e-9, 64, 8, 8, 63, 0.5, None, 0, C.byref(fi)) == 0 and fi.hops == 0
    assert L.wbx_clip_tempo(ctx.h, S, 0, 64 * 400, 64, 1e-9, 64, 8, 8, 63, 0.5, trk.ctypes.data, 35, None) == 0
    assert trk["period"][:35].all() and not trk["period"][35:].any() and np.all(trk["lag"][35:] == 9)


# ---- 5: through the engine, the adapter, Python's conveniences ----------------------------------------------------------------------
def test_engine_calls_detect_fit_and_slice():
    """wbx_engine_onsets_sample and wbx_engine_tempo_sample equal the model; detect_tempo_sample finds the 120 bpm loop within
    the host test's bound; fit_sample_to_tempo's result has round(n * detected / target) frames; slice_sample's pieces
    concatenate to the range from the first onset on"""
    spec = synth.make_session("onse", 2, n_blocks=2, block=128, seed=0x0A5E)
    rate = spec.sample_rate
    assert rate == RATE
    eng = build_engine(spec, max_blocks=2)
    x, at = M.drum_loop(120, rate)
    n = len(x)
    planes = [x, np.roll(x, 1)]
    s = eng.add_sample("f32", rate, planes)
    rec, info = eng.onsets_sample(s, first_frame=7, n_frames=n - 9)
    want, want_info = M.onsets_clip(planes, 7, n - 9)
    assert same(rec, want) is None and info == want_info and info["onsets"] > 50
    trk, tinfo = eng.tempo_sample(s, first_frame=7, n_frames=n - 9)
    twant, twant_info = M.tempo_clip(planes, 7, n - 9, 256, 1e-9, 1024, 64, 56, 188, 0.5)
    assert same(trk, twant, F0.DTYPE) is None and {k: tinfo[k] for k in twant_info} == twant_info and tinfo["voiced_hops"] == tinfo["hops"] > 20
    tempo = eng.detect_tempo_sample(s)
    print("detected", tempo)
    assert tempo["voiced"] == 1.0 and abs(tempo["bpm"] / 120.0 - 1.0) <= TEMPO_BOUND
    new, sinfo, seen = eng.fit_sample_to_tempo(s, 100.0)
    assert seen == tempo and eng._sample_shape[new] == (int(round(n * tempo["bpm"] / 100.0)), 2)
    ids, pieces = eng.slice_sample(s)
    found = np.flatnonzero(M.onsets_clip(planes, 0, n)[0]["onset"])
    assert len(ids) == len(found) > 50 and pieces[0][0] == int(found[0]) * 256 and sum(m for _, m in pieces) == n - pieces[0][0]
    joined = np.concatenate([eng.export_sample(i, "f32", clamp=False)[0] for i in ids])
    assert np.array_equal(joined.view(np.uint32), np.stack(planes, axis=1)[pieces[0][0]:].reshape(-1).view(np.uint32))
    # no voiced window: nothing to fit; no onset: no piece
    quiet = eng.add_sample("f32", rate, [np.zeros(400000, dtype=np.float32)])
    assert eng.detect_tempo_sample(quiet)["bpm"] is None and eng.detect_tempo_sample(quiet)["voiced"] == 0.0
    with pytest.raises(ValueError):
        eng.fit_sample_to_tempo(quiet, 100.0)
    assert eng.slice_sample(quiet) == ([], [])
    # refusals through layer 2
    L, oi, fi = W.lib(), _ffi.OnsetInfo(), _ffi.F0Info()
    buf = np.zeros(128, dtype=M.DTYPE)
    call = lambda smp, nn, H=256, out=buf.ctypes.data, cap=128: L.wbx_engine_onsets_sample(eng.h, smp, 0, nn, H, 1e-9, 0.3, 0.1, 3, 8, out, cap,
                                                                                       C.byref(oi))
    assert call(9999, 4000) == -4 and call(s, n + 1) == -4 and call(s, 0) == -4 and call(s, 4000, H=100) == -4
    assert call(s, 4000, out=None) == -4 and call(s, 4000, cap=14) == -4 and not buf["energy"].any()
    assert call(s, 4000, cap=15) == 0 and oi.hops == 15 and buf["energy"][:15].all() and not buf["energy"][15:].any()
    tbuf = np.zeros(8, dtype=F0.DTYPE)
    tcall = lambda smp, nn, Wn=64, cap=8: L.wbx_engine_tempo_sample(eng.h, smp, 0, nn, 64, 1e-9, Wn, 8, 8, 63, 0.5, tbuf.ctypes.data, cap, C.byref(fi))
    assert tcall(9999, 64 * 140) == -4 and tcall(s, n + 1) == -4 and tcall(s, 64 * 140, Wn=68) == -4 and tcall(s, 64 * 140, cap=1) == -4
    assert not tbuf["period"].any() and tcall(s, 64 * 140, cap=2) == 0 and fi.hops == 2 and tbuf["period"][:2].all()
    eng.close()


def test_cpp_adapter_finds_a_takes_onsets_and_tempo(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take and calls wbx::Engine::onsets_sample and tempo_sample; the
    records equal the model's, and the bursts every 2048 frames come out as a period of 32 hops of 64"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_onsets")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_onsets.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dumps = [str(tmp_path / "onsets.bin"), str(tmp_path / "tempo.bin")]
    out = subprocess.check_output([exe] + dumps, timeout=120).decode()
    n = 40 * 512
    g = np.arange(n, dtype=np.uint64)
    x = ((((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(256.0) - np.float32(0.5)) \
        * np.where(g % 2048 < 256, np.float32(1.0), np.float32(0.015625))
    x = x.astype(np.float32)
    want, info = M.onsets_clip([x], 0, n, 64)
    twant, tinfo = M.tempo_clip([x], 0, n, 64, 1e-9, 64, 8, 8, 63, 0.5)
    assert "adapter onsets ok %d hops %d onsets %d windows %d voiced" % (info["hops"], info["onsets"], tinfo["hops"], tinfo["voiced_hops"]) in out, out
    assert same(np.fromfile(dumps[0], dtype=M.DTYPE), want) is None and same(np.fromfile(dumps[1], dtype=F0.DTYPE), twant, F0.DTYPE) is None
    assert list(np.flatnonzero(want["onset"])) == list(range(0, n // 64, 32))
    assert tinfo["voiced_hops"] == tinfo["hops"] == 25 and np.all(np.abs(twant["period"] - 32.0) < 0.5)


# ---- 6: beside the audio thread -------------------------------------------------------------------------------------------------
def test_onsets_and_tempo_beside_the_audio_thread():
    """The shape of the f0 call's test (test_gpu_f0.py): a clip far behind the played range names the big sample while the
    threads run, so a delete of it can never succeed — between two calls it is refused for the clip (-4), inside one for
    the pin (-3, asked first) — one thread deletes without pause while the other measures, onsets and tempo in turn, until a
    delete has been refused for the pin.  The master is what it is without the calls, and the last records equal the
    model's."""
    NB, FR, WAIT, CALLS = 300, 1 << 21, 60.0, 400
    H = 64
    spec = synth.make_session("onsthr", 2, n_blocks=NB, block=128, seed=0x0A5E12)
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

    def measurer():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["rec"], results["info"] = eng.onsets_sample(big, H, w=64, a=256, first_frame=first, n_frames=n, channels=2, frames=FR)
                results["trk"], results["tinfo"] = eng.tempo_sample(big, H, 1e-9, 1024, 512, 30, 700, first_frame=first, n_frames=n,
                                                                    channels=2, frames=FR)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (measurer, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused.is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read a live clip: the records are the model's, bit for bit
    want, want_info = M.onsets_clip(planes, first, n, H, w=64, a=256)
    assert same(results["rec"], want) is None and results["info"] == want_info
    windows = F0.hops(n // H, 1024, 512, 700)
    some = [0, 1, 7, 30, windows - 2, windows - 1]
    twant, twant_info = M.tempo_clip(planes, first, n, H, 1e-9, 1024, 512, 30, 700, 0.5, only=some)
    assert results["tinfo"]["hops"] == twant_info["hops"] == windows > 50 and same(np.ascontiguousarray(results["trk"][some]), twant, F0.DTYPE) is None
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    eng.close()
