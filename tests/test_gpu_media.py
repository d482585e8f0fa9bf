"""GPU parity tests for the two rows next to the mix path, through the C ABI:
  * clip ingest: interleaved decoder frames -> planar clip storage (deinterleave_samples, dsp/sample.cpp:29-43)
  * waveform mip-maps (summarize_for_mipmaps_impl / WaveformVisual::create, gfx/waveform_visual.cpp:9-246)
Byte / integer work: everything is compared bit-for-bit with the oracle's restatement."""
import numpy as np
import pytest

import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

DT = {"i16": np.int16, "i32": np.int32, "f32": np.float32}


def make_pcm(fmt, frames, ch, seed):
    rng = np.random.default_rng(seed)
    if fmt == "i16":
        return rng.integers(-32768, 32768, (frames, ch)).astype(np.int16)
    if fmt == "i32":
        return rng.integers(-2**31, 2**31, (frames, ch)).astype(np.int32)
    return (rng.standard_normal((frames, ch)) * 0.4).astype(np.float32)


@pytest.mark.parametrize("fmt", ["i16", "i32", "f32"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("frames", [1, 3, 1024, 2501, 70001])
def test_ingest_matches_oracle(fmt, ch, frames):
    a = make_pcm(fmt, frames, ch, frames * 3 + ch)
    exp = O.oracle_deinterleave(a)
    ctx = W.MixContext(4)
    ctx.clip_upload_interleaved(0, fmt, 48000, a)
    for c in range(ch):
        got = ctx.clip_download(0, c, frames, DT[fmt])
        assert np.array_equal(got.view(np.uint8), exp[c].view(np.uint8))
    ctx.close()


def test_ingest_multi_chunk_and_device_source():
    """longer than one 4 Mi-frame staging chunk (both staging buffers in play), and the device-source entry point"""
    torch = pytest.importorskip("torch")
    frames, ch = (4 << 20) * 2 + 12345, 2
    a = make_pcm("i16", frames, ch, 99)
    ctx = W.MixContext(4)
    ctx.clip_upload_interleaved(0, "i16", 44100, a)
    for c in range(ch):
        assert np.array_equal(ctx.clip_download(0, c, frames, np.int16), a[:, c])
    d = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    ctx.clip_ingest_device(1, "i16", ch, 44100, frames, d.data_ptr())
    for c in range(ch):
        assert np.array_equal(ctx.clip_download(1, c, frames, np.int16), a[:, c])
    # a misaligned device pointer is refused, not mis-read
    with pytest.raises(W.WbxError):
        ctx.clip_ingest_device(2, "i16", ch, 44100, frames - 8, d.data_ptr() + 4)
    ctx.close()


def test_ingested_clip_plays_like_planar_upload():
    """the whole path: an engine fed through add_sample_interleaved renders the same bits as through add_sample"""
    spec = synth.make_session("ing", 24, seek=True, src_rate=44100, n_blocks=6, seed=0x1A)
    outs = []
    for mode in ("planar", "interleaved"):
        eng = build_engine(spec, max_blocks=6, device_synth=False, interleaved_ingest=(mode == "interleaved"))
        eng.play()
        eng.render(6)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        outs.append((m.copy(), pk.copy()))
        eng.close()
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


def special_values(fmt, data):
    if fmt == "f32":
        data[5] = 1.0
        data[9] = -1.0
        data[11] = 2.5      # beyond [-1, 1]: (T)conv wraps like the reference's x86 build
        data[12] = -3.0
        data[20] = np.nan
        data[21] = np.inf
    return data


@pytest.mark.parametrize("fmt", ["i16", "i32", "f32"])
@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("frames", [65, 83, 2048, 2049, 8195, 100003])
def test_mipmaps_match_oracle(fmt, quality, frames):
    a = make_pcm(fmt, frames, 2, frames + quality)
    a[:, 0] = special_values(fmt, a[:, 0].copy())
    ctx = W.MixContext(4)
    ctx.clip_upload_interleaved(0, fmt, 48000, a)
    ctx.build_mipmaps(0, quality)
    levels = ctx.L.wbx_mip_levels(frames)
    assert levels == O.oracle_mip_levels(frames)
    for lvl in range(levels):
        got = ctx.fetch_mipmap(0, lvl, 2, frames, quality)
        for c in range(2):
            exp = O.oracle_mip(fmt, np.ascontiguousarray(a[:, c]), lvl, quality)
            assert got.shape[1] == len(exp)
            assert np.array_equal(got[c], exp), (fmt, quality, frames, lvl, c, np.flatnonzero(got[c] != exp)[:8])
    ctx.close()


def test_mipmaps_plateaus_and_order():
    """equal runs (first occurrence wins) and min/max order inside a pair, at every level"""
    frames = 40000
    rng = np.random.default_rng(5)
    data = np.repeat(rng.integers(-5, 6, frames // 16 + 1), 16)[:frames].astype(np.int16) * 3000
    ctx = W.MixContext(4)
    ctx.clip_upload_interleaved(0, "i16", 48000, data.reshape(-1, 1))
    for quality in (0, 1):
        ctx.build_mipmaps(0, quality)
        for lvl in range(O.oracle_mip_levels(frames)):
            got = ctx.fetch_mipmap(0, lvl, 1, frames, quality)[0]
            assert np.array_equal(got, O.oracle_mip("i16", data, lvl, quality)), (quality, lvl)
    ctx.close()


def test_mipmaps_full_size_clip():
    """a clip of the bench session's size (5.5 M frames, 9 levels): every level against the oracle, plus the
    size-independent property that a level's pair is the ordered merge of the four pairs below it"""
    frames = 5_500_003
    a = make_pcm("f32", frames, 1, 1234)
    ctx = W.MixContext(4)
    ctx.clip_upload_interleaved(0, "f32", 44100, a)
    ctx.build_mipmaps(0, 1)
    levels = ctx.L.wbx_mip_levels(frames)
    assert levels == 9
    prev = None
    for lvl in range(levels):
        got = ctx.fetch_mipmap(0, lvl, 1, frames, 1)[0]
        assert np.array_equal(got, O.oracle_mip("f32", np.ascontiguousarray(a[:, 0]), lvl, 1)), lvl
        if prev is not None:
            n = min(len(got) // 2, len(prev) // 8)       # pairs fully covered by stored pairs of the level below
            lo = prev[:n * 8].reshape(n, 8)
            assert np.array_equal(got[:2 * n].reshape(n, 2).min(axis=1), lo.min(axis=1))
            assert np.array_equal(got[:2 * n].reshape(n, 2).max(axis=1), lo.max(axis=1))
        prev = got
    ctx.close()


def test_mipmaps_reject_unsupported():
    ctx = W.MixContext(4)
    ctx.clip_upload(0, "i24", 48000, [np.zeros(100, np.int32)])
    with pytest.raises(W.WbxError):
        ctx.build_mipmaps(0, 0)       # the reference's switch has no 24-bit case
    with pytest.raises(W.WbxError):
        ctx.fetch_mipmap(0, 0, 1, 100, 0)
    ctx.close()


def test_mipmaps_match_the_reference_fixture():
    """the device's mip levels against tests/golden/mip.npz — outputs of the reference's own summarize_for_mipmaps_impl
    (oracle/gen_golden.py; every storage format, both qualities, every level, values beyond [-1, 1], ±Inf, NaN)"""
    from test_oracle_golden import mip_golden_cases
    n = 0
    for name, fmt, data, want in mip_golden_cases():
        ctx = W.MixContext(2)
        ctx.clip_upload_interleaved(0, fmt, 48000, np.ascontiguousarray(data.reshape(-1, 1)))
        for q in (0, 1):
            ctx.build_mipmaps(0, q)
            for lvl in range(ctx.L.wbx_mip_levels(len(data))):
                got = ctx.fetch_mipmap(0, lvl, 1, len(data), q)[0]
                assert np.array_equal(got, want[(q, lvl)]), (name, q, lvl, np.flatnonzero(got != want[(q, lvl)])[:8])
                n += 1
        ctx.close()
    assert n == 82


def test_ingest_matches_the_reference_fixture():
    """the device's planar clip storage against tests/golden/ingest.npz — outputs of the reference's own
    deinterleave_samples<T> under load_file's loop (oracle/gen_golden.py ingest); clips of more than two channels are refused
    (the path's AudioBuffer is mono / stereo), never mis-read"""
    from test_oracle_golden import ingest_golden_cases
    n = 0
    for name, a, want in ingest_golden_cases():
        frames, ch = a.shape
        fmt = name.split("_")[0]
        ctx = W.MixContext(2)
        if ch > 2:
            with pytest.raises(W.WbxError):
                ctx.clip_upload_interleaved(0, fmt, 48000, a)
            ctx.close()
            continue
        ctx.clip_upload_interleaved(0, fmt, 48000, a)
        for c in range(ch):
            got = ctx.clip_download(0, c, frames, DT[fmt])
            assert np.array_equal(got.view(np.uint8), want[c, :frames].view(np.uint8)), (name, c)
        ctx.close()
        n += 1
    assert n == 36


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_mipmaps_above_level_9(fmt):
    """a 2^28+3-frame mono clip: 11 levels, both qualities, every level against the oracle — f32 salted with NaN, ±Inf and
    values beyond [-1, 1] near its start, middle and end"""
    frames = 2**28 + 3
    a = make_pcm(fmt, frames, 1, 28 + len(fmt))
    if fmt == "f32":
        for at in (0, frames // 2, frames - 64):
            a[at:at + 64, 0] = special_values(fmt, a[at:at + 64, 0].copy())[:64]
            a[at + 30, 0] = -np.inf
    ctx = W.MixContext(4)
    try:
        ctx.clip_upload_interleaved(0, fmt, 48000, a)
        col = np.ascontiguousarray(a[:, 0])
        del a
        levels = ctx.L.wbx_mip_levels(frames)
        assert levels == O.oracle_mip_levels(frames) == 11
        for quality in (0, 1):
            ctx.build_mipmaps(0, quality)
            for lvl in range(levels):
                got = ctx.fetch_mipmap(0, lvl, 1, frames, quality)[0]
                exp = O.oracle_mip(fmt, col, lvl, quality)
                assert np.array_equal(got, exp), (fmt, quality, lvl, np.flatnonzero(got != exp)[:8])
    finally:
        ctx.close()


class _DeviceArray:
    """a device allocation of the library's, seen by torch (__cuda_array_interface__) so that a slice of it can be copied"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def device_level(ctx, clip, level, dtype):
    """(torch view of mip-map level `level` on the device, element count): slices of a level without fetching all of it"""
    import ctypes as C
    import torch
    p, n = C.c_void_p(), C.c_uint64()
    assert ctx.L.wbx_clip_mipmap_device(ctx.h, clip, level, C.byref(p), C.byref(n)) == 0
    return torch.as_tensor(_DeviceArray(p.value, n.value, np.dtype(dtype).str), device="cuda"), n.value


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_mipmaps_of_the_longest_clip(fmt):
    """a 2^31-17-frame mono clip (the longest the ABI accepts; made on the device): 13 levels, both qualities.  Too long for a
    host oracle of every level: per level the pairs of the first 2^20 samples and of the last 2^20 (each stretch widened to a
    whole chunk of the level, and the last one started on a chunk boundary so the chunks line up) against oracle_mip, every
    level's length, and the ordered-merge property between levels 2..12 — a pair is the ordered merge of the four below it"""
    import torch
    from sparse_clip import CAP
    seed, key, amp = 0x313, 2, 0.9
    A = ((CAP - 2**20) >> 25) << 25                      # a chunk boundary of level 12 (2^25 samples a pair)
    gen = synth.clip_channel if fmt == "f32" else synth.clip_channel_i16
    kw = {"amp": amp} if fmt == "f32" else {}
    head = gen(seed, key, 0, 2**25, first=0, **kw)
    tail = gen(seed, key, 0, CAP - A, first=A, **kw)
    ctx = W.MixContext(4)
    try:
        ctx.clip_synth(0, fmt, 1, 48000, CAP, seed, key, amp)
        levels = ctx.L.wbx_mip_levels(CAP)
        assert levels == O.oracle_mip_levels(CAP) == 13
        for quality in (0, 1):
            dt = np.int16 if quality else np.int8
            ctx.build_mipmaps(0, quality)
            torch.cuda.synchronize()
            prev = None
            for lvl in range(levels):
                dev, n = device_level(ctx, 0, lvl, dt)
                assert n == O.lib().wbo_mip_data_count(CAP, lvl)
                chunk = 2 << (2 * lvl)                   # samples a pair of this level summarises
                h = max(2**20, chunk)
                a = ((CAP - 2**20) // chunk) * chunk
                eh = O.oracle_mip(fmt, head[:h], lvl, quality)
                et = O.oracle_mip(fmt, tail[a - A:], lvl, quality)
                off = a >> (2 * lvl)
                assert off + len(et) == n
                assert np.array_equal(dev[:len(eh)].cpu().numpy(), eh), (fmt, quality, lvl, "head")
                assert np.array_equal(dev[off:].cpu().numpy(), et), (fmt, quality, lvl, "tail")
                if lvl >= 2:
                    got = dev.cpu().numpy()
                    if prev is not None:
                        k = min(len(got) // 2, len(prev) // 8)
                        lo = prev[:k * 8].reshape(k, 8)
                        assert np.array_equal(got[:2 * k].reshape(k, 2).min(axis=1), lo.min(axis=1)), (fmt, quality, lvl)
                        assert np.array_equal(got[:2 * k].reshape(k, 2).max(axis=1), lo.max(axis=1)), (fmt, quality, lvl)
                    prev = got
                del dev
    finally:
        ctx.close()
        torch.cuda.empty_cache()
