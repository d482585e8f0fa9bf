"""wbx_clip_spectrum and wbx_engine_spectrum_sample on the device.  Every cell is compared as its 32-bit pattern with
tests/spectrum_model.py, and the info exactly.  Sizes are the smallest at which the kernel can still go wrong: windows of 32,
36 and 256 frames (one chunk each); 1, 2, 7, 64, 65 and 130 bins — below, at and across the 64 lanes of a wave and its 128
bins, on and off a lane's pair of bins; hop lengths that make the hops of a workgroup share their staged words (1, 7, 64), that
are no multiple of 4 (the word-by-word instance) and that leave gaps between the windows (1000, W + 5); 0, 1, 2, 8, 9 and 17
hops with ragged ends, so that a workgroup's 16 or 32 hops and a lane's 4 or 8 end early; the three channel modes on a mono and on a
stereo source with non-finite samples in it.  Once each: the largest span (W = 8192, B = 256: 16 chunks), windows of 516 to
1100 frames (a last chunk that is not full) with hop lengths of 2000 to 14 000 frames and 256 to 1024 bins (8 and 4 hops per
workgroup), and a call across a launch bound."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import spectrum_model as M
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RATE = 48000
SRC_LEN = 20000
SRC = {1: 1, 2: 2}                                              # channels -> clip id of a source
BINS = [1, 2, 7, 64, 65, 130]
HOP_COUNTS = [0, 1, 2, 8, 9, 17]
KINDS = ["rect", "hann", "kaiser"]


def source(channels, n=SRC_LEN, seed=0x5BEC):
    """two tones per channel (the channels differ) and seeded noise, with a NaN, both infinities and a huge sample in each"""
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n, dtype=np.float64)
    out = []
    for c in range(channels):
        v = 0.5 * np.sin(2 * np.pi * i / (23.7 + 9 * c)) + 0.25 * np.sin(2 * np.pi * i / (5.1 + c)) + 0.05 * rng.standard_normal(n)
        v = v.astype(np.float32)
        at = rng.integers(0, n, 12)
        v[at[:3]], v[at[3:6]], v[at[6:9]], v[at[9:]] = np.nan, np.inf, -np.inf, np.float32(3e38)
        v[[0, 1, n - 1]] = [np.nan, 0.75, np.inf]                # ... at the clip's first and last frame
        out.append(v)
    return out


def design(Wn, B, seed, kind="hann", lengths=False):
    """a basis of B frequencies: 0, 0.5 and seeded ones, some with windows of their own"""
    rng = np.random.default_rng(seed)
    f = np.concatenate([[0.0, 0.5], rng.random(B)])[:B] * np.where(np.arange(B) < 2, 1.0, 0.5)
    ln = np.concatenate([[4, Wn], rng.integers(4, Wn + 1, B)])[:B].astype(np.uint32) if lengths else None
    return W.spectrum_basis(Wn, f, ln, kind, 7.0)


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {ch: source(ch) for ch in (1, 2)}
    for ch in (1, 2):
        c.clip_upload(SRC[ch], "f32", RATE, c.src[ch])
    c.next_id = 100
    yield c
    c.close()


def upload_basis(c, words):
    c.next_id += 1
    c.clip_upload(c.next_id, "f32", RATE, [words])
    return c.next_id


def same(got, want):
    """None, or the first cell that differs in a bit"""
    assert got.dtype == want.dtype == np.float32
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        h, b = (int(v) for v in bad[0])
        return (h, b, got[h, b], want[h, b], len(bad))
    return None


def launches_of(hops, Wn, B):
    return M.launches(hops, Wn, B, int(W.lib().wbx_spectrum_launch_terms()))


def run_and_check(c, clip, planes, first, n, channel, basis_clip, words, Wn, B, H):
    want, want_info = M.spectrum_clip(planes, first, n, channel, words, Wn, B, H)
    got, info = c.clip_spectrum(clip, first, n, basis_clip, Wn, B, H, channel=channel)
    where = (len(planes), first, n, channel, Wn, B, H)
    assert same(got, want) is None, (where, same(got, want))
    assert info == dict(want_info, launches=launches_of(want_info["hops"], Wn, B)), (where, info, want_info)
    return got, info


def length_for(hops, Wn, H, ragged):
    """a range of exactly `hops` complete frames, with up to H - 1 frames behind the last one"""
    return Wn - 1 if hops == 0 else Wn + (hops - 1) * H + (ragged % H)


# ---- 1: the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("channels", [1, 2])
def test_spectrum_matrix(ctx, channels, B):
    """every window and hop length at one bin count; the number of hops, the ragged end, the channel mode, the window kind and
    the range's place take turns.  The range starts at the clip's first frame or inside it and, at the odd places, ends on its
    last"""
    seen_hops, seen_ch = set(), set()
    cases = [(Wn, H) for Wn in (32, 36, 256) for H in (1, 7, 64, 1000, None)]
    for i, (Wn, H) in enumerate(cases):
        H = Wn + 5 if H is None else H
        k = (i + BINS.index(B)) % len(HOP_COUNTS)
        hops = HOP_COUNTS[k]
        n = length_for(hops, Wn, H, 3 * i + 1)
        assert n <= SRC_LEN
        first = SRC_LEN - n if i % 2 else (0, 5, 64)[i % 3]
        channel = ((0, M.MID) if channels == 1 else (0, 1, M.MID))[(i + B) % (channels + 1)]
        words = design(Wn, B, 1000 * B + i, KINDS[i % 3], lengths=i % 2 == 0)
        got, info = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, channel, upload_basis(ctx, words), words, Wn, B, H)
        assert info["hops"] == hops == len(got) and got.shape == (hops, B)
        seen_hops.add(hops)
        seen_ch.add(channel)
    assert len(seen_hops) >= 5 and len(seen_ch) == channels + 1


@pytest.mark.parametrize("hops", HOP_COUNTS)
def test_hop_counts_and_channels_at_the_clips_first_and_last_frame(ctx, hops):
    """every number of hops in every channel mode of both sources, the range at the clip's first frame and ending on its
    last — where the NaN and the infinity lie — with a ragged end"""
    for j, (Wn, B, H) in enumerate(((32, 7, 7), (256, 65, 64), (36, 130, 1000))):
        words = design(Wn, B, 77 + j)
        basis = upload_basis(ctx, words)
        for channels in (1, 2):
            for channel in ((0, M.MID) if channels == 1 else (0, 1, M.MID)):
                n = length_for(hops, Wn, H, 5)
                for first in (0, SRC_LEN - n):
                    got, _ = run_and_check(ctx, SRC[channels], ctx.src[channels], first, n, channel, basis, words, Wn, B, H)
                    assert len(got) == hops


def test_mid_of_mono_is_the_sample_and_of_stereo_the_rounded_mean(ctx):
    words = design(36, 7, 5)
    basis = upload_basis(ctx, words)
    mono0, _ = ctx.clip_spectrum(SRC[1], 3, 900, basis, 36, 7, 7, channel=0)
    monom, _ = ctx.clip_spectrum(SRC[1], 3, 900, basis, 36, 7, 7, channel="mid")
    assert same(mono0, monom) is None
    l, r = (M.ST.inputs([p])[0] for p in ctx.src[2])
    mid = (0.5 * (l + r)).astype(np.float32)
    want = M.power(mid.astype(np.float64)[3:903], words, 36, 7, 7)
    got, _ = ctx.clip_spectrum(SRC[2], 3, 900, basis, 36, 7, 7)
    assert same(got, want) is None and same(got, mono0) is not None


# ---- 2: chunks, large hops, the largest span, a launch's seam ---------------------------------------------------------------------
# (W, B, H, hops): windows of more than one chunk with a last chunk that is not full, hop lengths of 2000 to 14 000 frames (a
# workgroup's hops share no words, and none are dropped: the kernel stages chunk by chunk), bin counts
# that put 2 and 4 waves side by side (8 and 4 hops per workgroup) with a last tile of bins that is not full
LARGE = [(516, 256, 2000, 9), (1100, 300, 2001, 5), (1024, 513, 5000, 5), (640, 1024, 13999, 3), (2048, 600, 14000, 2), (516, 130, 515, 9),
         (1028, 64, 513, 17), (600, 7, 512, 33)]


@pytest.mark.parametrize("channels", [1, 2])
def test_windows_of_several_chunks_large_hops_and_many_bins(channels):
    c = W.MixContext(4, block=128)
    n_all = 48000
    planes = source(channels, n_all, seed=0x4A1)
    c.clip_upload(1, "f32", RATE, planes)
    c.next_id = 10
    for i, (Wn, B, H, hops) in enumerate(LARGE):
        n = length_for(hops, Wn, H, 3 * i + 1)
        assert n <= n_all
        first = n_all - n if i % 2 else 3
        words = design(Wn, B, 31 * i, KINDS[i % 3], lengths=i % 2 == 1)
        channel = (0, M.MID)[i % 2] if channels == 1 else (M.MID, 1, 0)[i % 3]
        got, info = run_and_check(c, 1, planes, first, n, channel, upload_basis(c, words), words, Wn, B, H)
        assert info["hops"] == hops and info["launches"] == 1
    c.close()


def test_the_largest_window(ctx):
    """W = 8192, B = 256: 16 chunks of 512 terms and the largest basis (16 MB); 3 hops, H = 1000"""
    words = design(8192, 256, 9, "hann", lengths=True)
    n = 8192 + 2 * 1000 + 17
    got, info = run_and_check(ctx, SRC[2], ctx.src[2], 3, n, M.MID, upload_basis(ctx, words), words, 8192, 256, 1000)
    assert info["hops"] == 3 and info["launches"] == 1


def tile_hops(B):
    """wbx_spectrum.h's spectrum_shape: the hops a workgroup takes — 32 with at most 64 bins (a lane owns 8 hops of one
    bin), else 16 / G with G = 1, 2 or 4 waves over the bins"""
    if B <= 64:
        return 32
    G = 1
    while G < -(-B // 128) and G < 4:
        G *= 2
    return 16 // G


def test_a_call_across_launch_bounds():
    """a range of more hops than two launches take, at H = 1 and the smallest window and bin count at which a call of at most
    2^20 hops and 2^25 cells holds them (read from the getters): two full launches and a third of 11 hops, which is no multiple
    of the hops a workgroup takes.  The model is evaluated for the first and last hop of every launch and of every tile of
    hops next to a bound, for the call's first and last hops and for seeded ones — hops are independent"""
    L = W.lib()
    H, found = 1, None
    for Wn in (32, 36, 256, 1024, 8192):
        for B in (1, 2, 7, 64, 65, 130, 256, 512, 1024):
            per = L.wbx_spectrum_launch_hops(Wn, B)
            assert per == M.launch_hops(Wn, B, L.wbx_spectrum_launch_terms())
            if per and 2 * per + 11 <= 1 << 20 and (2 * per + 11) * B <= 1 << 25 and (found is None or Wn * B * per < found[3]):
                found = (Wn, B, per, Wn * B * per)
    assert found, "no shape whose launches a call can cross"
    Wn, B, per, _ = found
    hops = 2 * per + 11
    F = tile_hops(B)
    assert per % F == 0 and 11 % F
    n = Wn + (hops - 1) * H
    c = W.MixContext(4, block=128)
    planes = source(1, n + 5, seed=0x5EA)
    c.clip_upload(1, "f32", RATE, planes)
    words = design(Wn, B, 3)
    c.clip_upload(2, "f32", RATE, [words])
    got, info = c.clip_spectrum(1, 2, n, 2, Wn, B, H, channel=0)
    rng = np.random.default_rng(4)
    seams = {h for s in range(per, hops, per) for h in (s - F, s - 1, s, min(s + F, hops) - 1)} | {0, F - 1} | set(range(hops - 11, hops))
    seams |= {per - 1, per, 2 * per - 1, 2 * per} | {int(v) for v in rng.integers(0, hops, 48)}
    seams = sorted(seams)
    assert len(seams) >= 64
    want, want_info = M.spectrum_clip(planes, 2, n, 0, words, Wn, B, H, only=seams)
    assert info == dict(want_info, launches=3) and got.shape == (hops, B)
    assert same(np.ascontiguousarray(got[seams]), want) is None
    c.close()


# ---- 3: refusals, the pool, the timer ---------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_pool_and_power_out_alone(ctx):
    L = W.lib()
    ctx.clip_upload(60, "i16", RATE, [np.arange(4000, dtype=np.int16)] * 2)
    S, Wn, B, H = SRC[2], 256, 8, 64
    words = design(Wn, B, 1)
    good = upload_basis(ctx, words)
    short = upload_basis(ctx, words[:-1])
    longer = upload_basis(ctx, np.concatenate([words, [np.float32(0)]]))
    stereo = ctx.next_id = ctx.next_id + 1
    ctx.clip_upload(stereo, "f32", RATE, [words[:2 * Wn * B // 2], words[2 * Wn * B // 2:]])
    stereo_full = ctx.next_id = ctx.next_id + 1
    ctx.clip_upload(stereo_full, "f32", RATE, [words, words])
    i16 = ctx.next_id = ctx.next_id + 1
    ctx.clip_upload(i16, "i16", RATE, [np.zeros(2 * Wn * B, dtype=np.int16)])
    cells = np.full(1024, 9.0, dtype=np.float32)
    si = _ffi.SpectrumInfo()

    def refused(status, why, clip=S, first=0, n=2000, channel=M.MID, basis=good, Wn=Wn, B=B, H=H, cap=1024, out=True):
        before = ctx.pool_stats()
        si.hops = 777
        got = L.wbx_clip_spectrum(ctx.h, clip, first, n, channel, basis, Wn, B, H, cells.ctypes.data if out else None, cap, C.byref(si))
        msg = bytes(L.wbx_last_error(ctx.h))
        assert got == status and why in msg, (got, status, why, msg)
        assert got == M.check(n, channel, Wn, B, H, out, cap) or b"clip" in msg[14:] or b"channel 1" in msg
        assert ctx.pool_stats() == before and si.hops == 777 and np.all(cells == 9.0)

    refused(-4, b"unknown clip", clip=999)
    refused(-4, b"no frames", n=0)
    refused(-4, b"2^31 - 16", n=(1 << 31) - 16)
    for ch in (3, 7, 0xFFFFFFFF):
        refused(-4, b"channel is not", channel=ch)
    for bad in (0, 28, 34, 8196):
        refused(-4, b"window_frames", Wn=bad)
    for bad in (0, 1025):
        refused(-4, b"n_bins", B=bad)
    refused(-4, b"above 2^21", Wn=8192, B=257)
    for bad in (0, 65537):
        refused(-4, b"hop_frames", H=bad)
    refused(-4, b"power_out is NULL", out=False)
    refused(-4, b"cells_cap", cap=28 * 8 - 1)                   # (2000 - 256) // 64 + 1 = 28 hops of 8 bins: one cell short
    refused(-3, b"2^20 hops", n=32 + (1 << 20), Wn=32, B=1, H=1, cap=(1 << 20) + 1)                # 2^20 + 1 hops
    refused(-4, b"cells_cap", n=32 + (1 << 20), Wn=32, B=1, H=1, cap=1 << 20)                      # ... the capacity is asked first
    refused(-3, b"2^25 cells", n=32 + (1 << 19), Wn=32, B=64, H=1, cap=1 << 26)
    refused(-3, b"not F32", clip=60)
    refused(-4, b"window_frames", clip=60, Wn=34)               # the sizes are judged before the clips are looked at
    refused(-4, b"channel 1 of a mono", clip=SRC[1], channel=1)
    refused(-4, b"past the clip", first=SRC_LEN - 1999)
    refused(-4, b"past the clip", first=(1 << 64) - 1)          # a sum that wraps
    refused(-4, b"unknown basis", basis=9999)
    refused(-3, b"basis clip's storage format", basis=i16)
    refused(-3, b"basis clip is not mono", basis=stereo)
    refused(-3, b"basis clip is not mono", basis=stereo_full)
    refused(-4, b"does not have", basis=short)
    refused(-4, b"does not have", basis=longer)
    refused(-4, b"does not have", basis=good, B=4)              # the right words for another shape
    refused(-4, b"does not have", basis=SRC[1])                 # a clip that is no basis
    refused(-4, b"past the clip", basis=9999, first=SRC_LEN)    # the source is judged before the basis
    # Python's wrapper asks wbx_spectrum_check before it allocates the cells
    with pytest.raises(W.WbxError) as err:
        ctx.clip_spectrum(S, 0, (1 << 31) - 17, good, 32, 1024, 1)
    assert err.value.status == -3
    # what is not refused: no hops and no buffer, a capacity that is just enough
    assert L.wbx_clip_spectrum(ctx.h, S, 0, 255, M.MID, good, Wn, B, H, None, 0, C.byref(si)) == 0
    assert (si.hops, si.bins, si.launches) == (0, 8, 0)
    assert L.wbx_clip_spectrum(ctx.h, S, 0, 2000, M.MID, good, Wn, B, H, cells.ctypes.data, 28 * 8, None) == 0
    assert np.all(cells[:28 * 8] != 9.0) and np.all(cells[28 * 8:] == 9.0)


def test_a_non_finite_basis_row_stays_in_its_bin_and_loud_neighbours_stay_outside(ctx):
    """rows 2 and 4 of a basis hold a NaN and an infinity: their bins are not finite, every other cell is the model's of the
    clean basis; the source's range lies between NaNs and huge samples (tests/test_gpu_f0.py's neighbours) that are never read"""
    Wn, B, H = 36, 7, 7
    words = design(Wn, B, 2)
    bad = words.copy().reshape(Wn, B, 2)
    bad[3, 2, 0], bad[9, 4, 1] = np.nan, np.inf
    clean, hurt = upload_basis(ctx, words), upload_basis(ctx, bad.reshape(-1))
    planes = ctx.src[2]
    want, _ = M.spectrum_clip(planes, 40, 1000, M.MID, words, Wn, B, H)
    got, _ = ctx.clip_spectrum(SRC[2], 40, 1000, hurt, Wn, B, H)
    ok = [0, 1, 3, 5, 6]
    assert same(np.ascontiguousarray(got[:, ok]), np.ascontiguousarray(want[:, ok])) is None and not np.isfinite(got[:, [2, 4]]).any()
    assert same(ctx.clip_spectrum(SRC[2], 40, 1000, clean, Wn, B, H)[0], want) is None
    loud = [p.copy() for p in planes]
    for p in loud:
        p[:40], p[39], p[1040:] = np.float32(3e38), np.nan, np.nan
    ctx.next_id += 1
    ctx.clip_upload(ctx.next_id, "f32", RATE, loud)
    assert same(ctx.clip_spectrum(ctx.next_id, 40, 1000, clean, Wn, B, H)[0], want) is None


def test_the_pool_is_unchanged_and_the_timers_keep_apart():
    """a call allocates nothing in the pool; wbx_spectrum_ms works and is the spectrum calls' alone"""
    c = W.MixContext(4, block=128)
    out = C.c_double(7.0)
    assert c.L.wbx_spectrum_ms(c.h, C.byref(out)) == -4 and out.value == 7.0     # none yet
    assert c.L.wbx_spectrum_ms(c.h, None) == -4 and c.L.wbx_spectrum_ms(None, C.byref(out)) == -4
    planes = source(1, 5000, seed=3)
    c.clip_upload(1, "f32", RATE, planes)
    words = design(256, 65, 4)
    c.clip_upload(2, "f32", RATE, [words])
    c.clip_f0(1, 0, 5000, 256, 64, 8, 600)
    assert c.L.wbx_spectrum_ms(c.h, C.byref(out)) == -4                          # an f0 call is no spectrum call
    f0_ms = c.f0_ms()
    base = c.pool_stats()
    c.next_id = 2
    run_and_check(c, 1, planes, 0, 5000, 0, 2, words, 256, 65, 64)
    assert c.pool_stats() == base
    ms = c.spectrum_ms()
    assert 0.0 < ms < 1000.0 and c.f0_ms() == f0_ms
    run_and_check(c, 1, planes, 5, 255, 0, 2, words, 256, 65, 64)                # no hops: no launch, a time of 0
    assert c.spectrum_ms() == 0.0 and c.pool_stats() == base
    c.close()


# ---- 4: through the engine, the adapter, Python's conveniences ----------------------------------------------------------------------
def test_spectrum_sample_spectrogram_and_chroma():
    """wbx_engine_spectrum_sample equals the model; spectrogram_sample and chroma_sample equal the model for the basis they
    design and leave the pool as they found it; an A major triad's chroma has A, C# and E on top; a spectrum call between two
    renders leaves the master bit-equal"""
    spec = synth.make_session("spece", 2, n_blocks=4, block=128, seed=0x5BE)
    rate = spec.sample_rate
    quiet = build_engine(spec, max_blocks=2)
    quiet.play()
    masters = []
    for _ in range(2):
        quiet.render(2)
        masters.append(quiet.ctx.fetch()[0].copy())
    quiet.close()
    eng = build_engine(spec, max_blocks=2)
    eng.play()
    eng.render(2)
    first_master = eng.ctx.fetch()[0].copy()
    n = 24000
    i = np.arange(n, dtype=np.float64)
    triad = sum(0.3 * np.sin(2 * np.pi * 440.0 * 2.0 ** (k / 12.0) * i / rate + 0.1 * k) for k in (-12, -8, -5)).astype(np.float32)
    planes = [triad, np.roll(triad, 7)]
    s = eng.add_sample("f32", rate, planes)
    freqs = np.linspace(0.0, 0.5, 65)
    words = W.spectrum_basis(256, freqs, None, "kaiser", 9.0)
    basis = eng.add_spectrum_basis(256, freqs, None, "kaiser", 9.0)
    assert eng._sample_shape[basis] == (2 * 65 * 256, 1)
    for channel in (0, 1, "mid"):
        got, info = eng.spectrum_sample(s, basis, 256, 65, 64, channel=channel, first_frame=7, n_frames=n - 9)
        want, want_info = M.spectrum_clip(planes, 7, n - 9, M.MID if channel == "mid" else channel, words, 256, 65, 64)
        assert same(got, want) is None and info == dict(want_info, launches=1) and info["hops"] > 300
    eng.render(2)
    assert np.array_equal(first_master.view(np.uint32), masters[0].view(np.uint32))
    assert np.array_equal(eng.ctx.fetch()[0].view(np.uint32), masters[1].view(np.uint32))      # the call between the renders changed nothing
    # the conveniences: the basis they design is the model's, and it is gone afterwards
    base, ids = eng.ctx.pool_stats(), len(eng._sample_shape)
    for constant_q in (False, True):
        got, f, info = eng.spectrogram_sample(s, 55.0 / rate, 12.0, 72, 4096, 1024, constant_q=constant_q)
        wf, clamped = M.log_freqs(55.0 / rate, 12.0, 72)
        assert np.array_equal(f.view(np.uint64), wf.view(np.uint64)) and clamped == 0
        lengths = M.constant_q_lengths(wf, 4096, 4096 * wf[0]) if constant_q else None
        assert lengths is None or (lengths[0] == 4096 and lengths[-1] < 128)
        want, want_info = M.spectrum_clip(planes, 0, n, M.MID, M.basis(4096, 72, wf, lengths, M.HANN), 4096, 72, 1024)
        assert same(got, want) is None and info == dict(want_info, launches=1)
        assert eng.ctx.pool_stats() == base and len(eng._sample_shape) == ids
    c1 = 440.0 * 2.0 ** (-45.0 / 12.0) / rate
    chroma, info = eng.chroma_sample(s, c1, octaves=5, window=8192, hop=2048, cycles=8192 * c1 * 8.0)
    wf, _ = M.log_freqs(c1, 12.0, 60)
    lengths = M.constant_q_lengths(wf, 8192, 8192 * c1 * 8.0)
    cells, _ = M.spectrum_clip(planes, 0, n, M.MID, M.basis(8192, 60, wf, lengths, M.HANN), 8192, 60, 2048)
    want = M.chroma_fold(cells, 5)
    assert chroma.dtype == np.float64 and np.array_equal(chroma.view(np.uint64), want.view(np.uint64)) and info["hops"] == len(chroma) == 8
    for row in chroma:
        assert set(np.argsort(row)[-3:]) == {9, 1, 4}, row
    assert eng.ctx.pool_stats() == base
    # refusals through layer 2: pool and outputs untouched
    L, si = W.lib(), _ffi.SpectrumInfo()
    si.hops = 777
    buf = np.full(4096, 9.0, dtype=np.float32)
    i16 = eng.add_sample("i16", rate, [np.zeros(2 * 65 * 256, dtype=np.int16)])
    two = eng.add_sample("f32", rate, [words, words])
    short = eng.add_sample("f32", rate, [words[:-1]])
    base = eng.ctx.pool_stats()
    call = lambda smp=s, nn=1000, b=basis, Wn=256, B=65, H=64, out=buf.ctypes.data, cap=4096: L.wbx_engine_spectrum_sample(
        eng.h, smp, 0, nn, 2, b, Wn, B, H, out, cap, C.byref(si))
    assert call(smp=9999) == -4 and call(nn=n + 1) == -4 and call(nn=0) == -4 and call(Wn=258) == -4 and call(b=9999) == -4
    assert call(b=short) == -4 and call(b=i16) == -3 and call(b=two) == -3 and call(B=64) == -4
    assert call(out=None) == -4 and call(cap=12 * 65 - 1) == -4                 # (1000 - 256) // 64 + 1 = 12 hops: one cell short
    assert call(nn=32 + (1 << 20), Wn=32, B=1, H=1, b=short, cap=1 << 21) == -3     # 2^20 + 1 hops, refused before the clips are looked at
    assert np.all(buf == 9.0) and si.hops == 777 and eng.ctx.pool_stats() == base
    assert call(cap=12 * 65) == 0 and si.hops == 12 and si.bins == 65 and np.all(buf[:12 * 65] != 9.0) and np.all(buf[12 * 65:] == 9.0)
    assert L.wbx_engine_spectrum_sample(None, s, 0, 1000, 2, basis, 256, 65, 64, buf.ctypes.data, 4096, None) == -4
    eng.close()


def test_cpp_adapter_looks_at_a_take(tmp_path):
    """a C++ host on include/wbx_adapter.hpp records a mono take, designs and uploads a basis and calls
    wbx::Engine::spectrum_sample; the basis words and the cells equal the model's, and the take's period of 50 frames shows"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_spectrum")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_spectrum.cpp"),
                           "-I" + os.path.join(root, "include"), "-L" + os.path.join(root, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "spectrum.bin")
    out = subprocess.check_output([exe, dump], timeout=120).decode()
    n, Wn, B, H = 5 * 512, 256, 24, 64
    g = np.arange(n, dtype=np.uint64)
    ph = g % 50
    tri = np.where(ph < 25, ph, 50 - ph).astype(np.float32) / np.float32(32.0) - np.float32(0.375)
    x = (tri + (((g * 2654435761) & 0xFFFFFFFF) >> 24).astype(np.float32) / np.float32(4096.0)).astype(np.float32)
    freqs, clamped = M.log_freqs(0.01, 12.0, B)
    words = M.basis(Wn, B, freqs, None, M.HANN)
    want, info = M.spectrum_clip([x], 0, n, M.MID, words, Wn, B, H)
    got = np.fromfile(dump, dtype=np.float32)
    assert "adapter spectrum ok %d hops %d bins" % (info["hops"], B) in out, out
    assert np.array_equal(got[:words.size].view(np.uint32), words.view(np.uint32))
    assert same(got[words.size:].reshape(info["hops"], B), want) is None
    assert np.all(np.argmax(want, axis=1) == 12) and abs(freqs[12] - 0.02) < 1e-15      # 1 / 50 cycles per frame: an octave above 0.01


# ---- 5: beside the audio thread -------------------------------------------------------------------------------------------------
def test_spectrum_beside_the_audio_thread():
    """The shape of the f0 call's test (test_gpu_f0.py): clips far behind the played range name the big sample AND the basis
    sample while the threads run, so a delete of either can never succeed — between two calls it is refused for the clip (-4),
    inside one for the pin (-3, asked first) — one thread deletes the two in turn without pause while the other measures
    until deletes of both have been refused for the pin.  The master is what it is without the calls, and the last cells
    equal the model's at sampled hops."""
    NB, FR, WAIT, CALLS = 300, 1 << 21, 60.0, 96
    Wn, B, H = 2048, 256, 64
    spec = synth.make_session("specthr", 2, n_blocks=NB, block=128, seed=0x5BE712)
    planes = source(2, FR, seed=41)
    freqs, _ = M.log_freqs(0.0005, 32.0, B)
    words = M.basis(Wn, B, freqs, None, M.HANN)

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 44100, planes)
        bid = eng.add_sample("f32", 44100, [words])
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        eng.add_audio_clip(eng.tracks[1], "far basis", 1000.0, 1001.0, 0.0, bid, 1.0, 1.0)
        return sid, bid

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
    big, basis = with_big(eng)
    first, n = 5, FR - 8
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), {big: threading.Event(), basis: threading.Event()}
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        turn = 0
        while not finished.is_set() and time.monotonic() < end:
            which = (big, basis)[turn % 2]
            turn += 1
            st = L.wbx_engine_delete_sample(eng.h, which)
            key_ = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key_] = seen.get(key_, 0) + 1
            if st == -3:
                refused[which].set()

    def measurer():
        try:
            began.set()
            while results["calls"] < CALLS and not (refused[big].is_set() and refused[basis].is_set()):
                results["cells"], results["info"] = eng.spectrum_sample(big, basis, Wn, B, H, first_frame=first, n_frames=n, channels=2,
                                                                        frames=FR)
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
    print("spectrum calls", results["calls"], "deletes", {k_: v for k_, v in seen.items()})
    assert refused[big].is_set() and refused[basis].is_set(), seen
    pinned = [k_ for k_ in seen if k_[0] == -3]
    assert pinned and all(b"being edited" in msg for _, msg in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in msg) for st, msg in seen), seen
    # every call read live clips: the cells are the model's, bit for bit (hops are independent: a sample of them)
    hops = M.hops(n, Wn, H)
    some = sorted({0, 1, 15, 16, hops // 3, hops // 2, hops - 17, hops - 2, hops - 1})
    want, want_info = M.spectrum_clip(planes, first, n, M.MID, words, Wn, B, H, only=some)
    assert results["info"]["hops"] == hops == want_info["hops"] and results["info"]["launches"] == launches_of(hops, Wn, B)
    assert same(np.ascontiguousarray(results["cells"][some]), want) is None
    # afterwards: no pin is left (the clips are what refuses now), and with the clips gone the deletes succeed
    for which, track in ((big, 0), (basis, 1)):
        assert L.wbx_engine_delete_sample(eng.h, which) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
        eng.delete_clip(eng.tracks[track], len(eng.clips(eng.tracks[track])) - 1)
        assert L.wbx_engine_delete_sample(eng.h, which) == 0
    eng.close()
