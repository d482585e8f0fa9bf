"""Renders far into long clips, bit for bit: clips of 2^31-17 frames — the longest the ABI accepts — made on the device
(wbx_clip_synth), tracks reading them around 2^24, 2^30, classify's hot-path bound 2147483000 and the clip's last frames at
every speed the mix kernel streams, cut clips near the bound, and slow clips whose tail quotient passes 2^32 mid-render.
The oracle reads sparse host arrays filled where the session reads (tests/sparse_clip.py): a kernel that read any other
frame would see the hash value where the oracle sees 0.  Each test names the row kinds its whole-block rows reached: those
come from the product's sequencer source on the CPU (tests/host_sim.py) — the device does not report them — whose
stream calls the device's are asserted equal to, and classify(), which names a whole-block row, is the same host/device code.
The kinds of partial rows (cut clips) depend on the mix family's mask level and are not asserted; their audio is."""
import gc

import numpy as np
import pytest

import grouped_order as GO
import long_sessions as LS
import oracle_ffi as O
import whitebox_amd as W
from sparse_clip import CAP
from whitebox_amd.engine import AudioBuffer, build_engine

pytestmark = pytest.mark.gpu


def plan_rows(plan):
    return [(b, t, bo, ns, O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (b, t, bo, ns, na, smp, off, spd, g, fl) in plan]


def oracle_run(spec, n_blocks, data):
    """master [K][C][F], peaks [K][T][C], tracks [K][T][C][F], stream-call log and transport of the oracle"""
    e = O.build_oracle_engine(spec, sample_data=data)
    e.enable_seglog()
    e.play()
    ms, pks, ts, rows, trs = [], [], [], [], []
    for b in range(n_blocks):
        m, _, t = e.process_tracks()
        ms.append(m)
        ts.append(t)
        pks.append(e.peaks())
        rows += [(b, t_, ds, min(ln, 0xFFFF), O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
                 for (t_, ds, ln, off, spd, g, smp) in e.seglog()]
        trs.append((O.f64_bits(e.playhead), O.f64_bits(e.sample_position)))
    e.close()
    return np.stack(ms), np.stack(pks), np.stack(ts), rows, trs


def check(spec, n_blocks, callback=False, segments=False):
    """one render of the session on the device — a batch of n_blocks, or the one-block callback n_blocks times — against
    the oracle: stream-call log, transport, per-track peaks, and the master bit for bit against the grouped-order model.
    segments: the batch must have been planned by the segmented planner"""
    data = LS.oracle_data(spec, n_blocks)
    om, opk, otr, orows, otrans = oracle_run(spec, n_blocks, data)
    eng = build_engine(spec, max_blocks=1 if callback else n_blocks, device_synth=True)
    try:
        eng.play()
        if not callback:
            eng.render(n_blocks)
            m, pk, _ = eng.ctx.fetch(peaks=True)
            assert plan_rows(eng.fetch_plan()) == orows
            ph, sp, _ = eng.transport()
            assert (O.f64_bits(ph), O.f64_bits(sp)) == otrans[-1]
            assert np.array_equal(pk, opk[..., :spec.channels])
            groups = GO.render_partition(spec, eng.ctx.render_order(n_blocks), 0, n_blocks)
            em, _ = GO.grouped_sum(otr, groups, 0)
            GO.assert_model(m, em, None, None, what=(spec.name, "batch"))
            if segments:
                assert eng.sequencer_stats()[0] >= 1, eng.sequencer_stats()
        else:
            out = AudioBuffer(spec.block, spec.channels)
            for b in range(n_blocks):
                eng.process(None, out, float(spec.sample_rate))
                groups = GO.render_partition(spec, eng.ctx.render_order(1), 0, 1)
                got = np.stack([out.get_write_pointer(c) for c in range(spec.channels)])
                assert plan_rows(eng.fetch_plan()) == [(0,) + r[1:] for r in orows if r[0] == b], b
                ph, sp, _ = eng.transport()
                assert (O.f64_bits(ph), O.f64_bits(sp)) == otrans[b], b
                em, _ = GO.grouped_sum(otr[b:b + 1], groups, 0)
                GO.assert_model(got[None], em, None, None, what=(spec.name, "callback", b))
                _, pk, _ = eng.ctx.fetch(peaks=True)
                assert np.array_equal(pk[0], opk[b][:, :spec.channels]), b
    finally:
        eng.close()
        del data
        gc.collect()


def kinds_reached(spec, n_blocks, want_above_2_30):
    """the kinds of whole-block rows at source positions >= 2^30, as the sequencer source plans them (see the module's note)"""
    top, per_track = LS.row_kinds_by_position(spec, n_blocks)
    above = {k for k, pos in top.items() if pos >= 2**30}
    assert set(want_above_2_30) <= above, (sorted(above), want_above_2_30)
    return per_track


def assert_handover(per_track, tracks, speeds):
    """tracks that start below 2147483000 and end above it: hot kind first, KIND_GENERIC after — in the same render"""
    for sp in speeds:
        t = next(i for i, tr in enumerate(tracks) if tr[0] == sp)       # the first track of a speed crosses the bound
        seq = [k for k in per_track[t] if k is not None]
        assert seq[0] != "GENERIC" and seq[-1] == "GENERIC", (sp, seq)


F32_SPEEDS = (1.0, 44100 / 48000, 1.088, 2.0, 3.7, 4096.0, 4097.0)


@pytest.mark.parametrize("mode", ["batch512", "batch4096", "segments", "callback", "no_masked_rows"])
def test_f32_clip_of_2_31_minus_17_frames(monkeypatch, mode):
    """fp32 mono, 2^31-17 frames (8 GiB on the device).  Kinds above 2^30: KIND_UNITY, KIND_WINDOW (44.1 -> 48 kHz),
    KIND_STRIDE (1.088, 2.0, 3.7, 4096), KIND_GENERIC (4097 and past the bound); every speed's first track hands over
    from the hot kernel to gen_kernel at 2147483000 within the render.  Paths: batch renders of 512- and 4096-frame blocks,
    the segmented planner (WBX_PLAN_SEG=2), the one-block callback, boundary rows through the pre-render pass
    (WBX_MASKED_ROWS=0)"""
    F = 4096 if mode == "batch4096" else 512
    n_blocks = 6
    speeds = F32_SPEEDS if F == 512 else F32_SPEEDS[:5]
    if mode == "segments":
        monkeypatch.setenv("WBX_PLAN_SEG", "2")
    if mode == "no_masked_rows":
        monkeypatch.setenv("WBX_MASKED_ROWS", "0")
    tracks = LS.landmark_tracks(F, CAP, speeds, n_blocks, fast_above=8.0)
    spec = LS.session(f"lp_f32_{mode}", "f32", CAP, tracks, block=F)
    per_track = kinds_reached(spec, n_blocks, {"UNITY", "WINDOW", "STRIDE", "GENERIC"})
    assert_handover(per_track, tracks, speeds[:-1])
    check(spec, n_blocks, callback=mode == "callback", segments=mode == "segments")


def test_i16_clip_of_2_31_minus_17_frames():
    """16-bit mono, 2^31-17 frames (4 GiB), 4096-frame blocks.  Kinds above 2^30: KIND_UNITY_I16, KIND_WINDOW_I16, KIND_STRIDE,
    KIND_GENERIC; handover at 2147483000"""
    F, n_blocks = 4096, 4
    speeds = (1.0, 44100 / 48000, 1.088, 2.0)
    tracks = LS.landmark_tracks(F, CAP, speeds, n_blocks)
    spec = LS.session("lp_i16", "i16", CAP, tracks, block=F)
    per_track = kinds_reached(spec, n_blocks, {"UNITY_I16", "WINDOW_I16", "STRIDE", "GENERIC"})
    assert_handover(per_track, tracks, speeds)
    check(spec, n_blocks)


@pytest.mark.parametrize("fmt", ["i32", "i24"])
def test_i32_clip_of_2_31_minus_17_frames(fmt):
    """24/32-bit mono in 4-byte containers, 2^31-17 frames (8 GiB).  Kinds above 2^30: KIND_UNITY_I32, KIND_WINDOW,
    KIND_STRIDE, KIND_GENERIC; handover at 2147483000"""
    F, n_blocks = 512, 6
    speeds = (1.0, 48000 / 44100 * 0.5, 3.7)
    tracks = LS.landmark_tracks(F, CAP, speeds, n_blocks)
    spec = LS.session(f"lp_{fmt}", fmt, CAP, tracks, block=F)
    per_track = kinds_reached(spec, n_blocks, {"UNITY_I32", "WINDOW", "STRIDE", "GENERIC"})
    assert_handover(per_track, tracks, speeds)
    check(spec, n_blocks)


def test_i16_stereo_clip_of_2_30_frames():
    """16-bit stereo, 2^30+2^20+5 frames (4 GiB): tracks through 2^30 and to the clip's last frame, unity and resampled"""
    F, n_blocks, count = 512, 6, 2**30 + 2**20 + 5
    speeds = (1.0, 44100 / 48000, 2.0)
    tracks = LS.landmark_tracks(F, count, speeds, n_blocks)
    spec = LS.session("lp_i16s", "i16", count, tracks, channels=2, block=F)
    kinds_reached(spec, n_blocks, {"UNITY_I16", "WINDOW_I16", "STRIDE"})
    check(spec, n_blocks)


@pytest.mark.parametrize("callback", [False, True])
def test_tail_quotient_crossing_2_32(callback):
    """slow fp32 clips whose tail quotient ceil((count - offset) / speed) passes k * 2^32 at frames 0, 1, F/2 and F-1 of a
    block: the reference plays that block short or silent (sampler.cpp:104), and so must the device"""
    F, n_blocks = 512, 6
    tracks = []
    for count, speed, k in ((5_000_000, 1e-3, 1), (CAP, 2e-5, 24)):
        for r in (0, 1, F // 2, F - 1):
            sp, off, _b = LS.crossing_track(count, speed, k, r, F, n_blocks)
            tracks.append((sp, off, 0.0, 1e12))
    # (one clip per session: the 5 M-frame crossings read the same 2^31-17-frame clip, whose quotient is then different)
    spec = LS.session("q32", "f32", CAP, tracks[4:], block=F)
    check(spec, n_blocks, callback=callback)
    spec = LS.session("q32s", "f32", 5_000_000, tracks[:4], block=F)
    check(spec, n_blocks, callback=callback)


def test_clip_length_cap_at_every_entry_point():
    """2^31-16 frames is refused with WBX_ERR_UNSUPPORTED by planar upload, synth, interleaved host and device ingest — the
    check comes before any read, so a small buffer stands in.  Synth and device ingest accept 2^31-17 frames, and the
    ingested clip reads back right at its last frames"""
    import ctypes as C
    import torch
    from whitebox_amd import _ffi
    over = CAP + 1
    ctx = W.MixContext(4)
    try:
        small = np.zeros(64, np.int16)
        dev = torch.zeros(64, dtype=torch.int16, device="cuda")
        ptrs = (C.c_void_p * 1)(small.ctypes.data)
        L = ctx.L
        assert L.wbx_clip_upload(ctx.h, 0, _ffi.FMT["i16"], 1, 48000, over, ptrs) == -3
        assert L.wbx_clip_synth(ctx.h, 0, _ffi.FMT["i16"], 1, 48000, over, 1, 0, np.float32(1.0)) == -3
        assert L.wbx_clip_upload_interleaved(ctx.h, 0, _ffi.FMT["i16"], 1, 48000, over, small.ctypes.data) == -3
        assert L.wbx_clip_ingest_device(ctx.h, 0, _ffi.FMT["i16"], 1, 48000, over, dev.data_ptr()) == -3
        # acceptance: device-source ingest of 2^31-17 16-bit frames (4 GiB), distinct values in the last 4096; read back on the
        # device through the level-0 mip-map (pairs of 2 samples; 16-bit quality keeps an i16 value), no 4 GiB download
        from test_gpu_media import device_level
        src = torch.zeros(CAP, dtype=torch.int16, device="cuda")
        tail = np.arange(-2048, 2048, dtype=np.int16) * 7
        src[-4096:] = torch.from_numpy(tail).to("cuda")
        torch.cuda.synchronize()                              # (torch's stream is not the library's: the source must be written)
        ctx.clip_ingest_device(0, "i16", 1, 48000, CAP, src.data_ptr())
        torch.cuda.synchronize()
        del src
        torch.cuda.empty_cache()
        ctx.build_mipmaps(0, 1)
        torch.cuda.synchronize()
        lv0, n = device_level(ctx, 0, 0, np.int16)
        a = CAP - 8193                                        # (even: a pair boundary) 4097 zero frames, then the tail
        exp = O.oracle_mip("i16", np.concatenate([np.zeros(CAP - 4096 - a, np.int16), tail]), 0, 1)
        got = lv0[a:].cpu().numpy()
        bad = np.flatnonzero(got != exp)
        assert a + len(exp) == n and not bad.size, (n, bad.size, bad[:6].tolist(), got[bad[:6]].tolist(), exp[bad[:6]].tolist())
        del lv0
        # ... and the synth entry point accepts the same length; its last frames play in the long-position tests above
        ctx.clip_synth(1, "i16", 1, 48000, CAP, LS.SEED, 1, 1.0)
    finally:
        ctx.close()
        gc.collect()
        torch.cuda.empty_cache()
