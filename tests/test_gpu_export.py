"""wbx_clip_export / wbx_engine_export_sample on the device: a frame range of a resident F32 clip as interleaved samples of
a device format, bit for bit (byte views, no tolerance) against the oracle's wbo_f32_to_interleaved_{i16,i24_x8,i32,f32}
(tests/test_oracle_vs_ref.py holds those to the reference's own translation unit) run on the source range — after a numpy
restatement of the compare-clamp  x > 1 ? 1 : (x < -1 ? -1 : x)  when WBX_EXPORT_CLAMP is set.  Packed 24-bit is true
interleave: the low three bytes of the i24_x8 words at (i*C + c)*3.  peak / over / nans are order-independent, hence exact:
checked against numpy."""
import ctypes as C
import threading
import wave

import numpy as np
import pytest

import bounce_util as BU
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth, wav
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

FORMATS = ["i16", "i24", "i24_x8", "i32", "f32"]
ELEM = {"i16": np.int16, "i24": np.uint8, "i24_x8": np.int32, "i32": np.int32, "f32": np.float32}
N = 1000


def clamp_np(x):
    """engine.cpp:1627-1636 as a compare-select: NaN passes"""
    x = np.asarray(x, dtype=np.float32)
    return np.where(x > np.float32(1.0), np.float32(1.0), np.where(x < np.float32(-1.0), np.float32(-1.0), x)).astype(np.float32)


def expected_bytes(planes, fmt, clamp):
    """planes: [C] float32 arrays of the range -> the bytes the export must leave"""
    src = [np.ascontiguousarray(clamp_np(p) if clamp else p, dtype=np.float32) for p in planes]
    n, ch = len(src[0]), len(src)
    name = "i24_x8" if fmt == "i24" else fmt
    a = np.zeros(n * ch, dtype=ELEM[name])
    getattr(O.lib(), "wbo_f32_to_interleaved_" + name)(a.ctypes.data, O.planar_ptrs(src), 0, n, ch)
    if fmt == "i24":
        return np.ascontiguousarray(a.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    return a.view(np.uint8)


def expected_stats(planes):
    peak, over, nans = [], [], []
    for p in planes:
        p = np.asarray(p, dtype=np.float32)
        nan = np.isnan(p)
        a = np.abs(p[~nan])
        peak.append(float(a.max()) if a.size else 0.0)
        with np.errstate(invalid="ignore"):
            over.append(int(np.count_nonzero((p > 1.0) | (p < -1.0))))
        nans.append(int(np.count_nonzero(nan)))
    return {"peak": peak, "over": over, "nans": nans}


def special_values():
    f = np.float32
    one_up = np.nextafter(f(1.0), f(2.0))
    v = [0.0, -0.0, 1.0, -1.0, one_up, -one_up, 1.5, -1.5, 3.0e9, -3.0e9, np.inf, -np.inf, np.nan,
         1e-40, -1e-40, 1.4e-45, -1.4e-45, np.nextafter(f(1.0), f(0.0)), -np.nextafter(f(1.0), f(0.0)), 0.5, -0.5]
    for scale in (32767.0, 32768.0, 8388607.0, 8388608.0, 2147483647.0):
        for k in (0, 1, 2, 100, 12345, 32766):
            for num in (k + 0.5, k + 1.0, k + 0.999999):
                x = f(num / scale)
                for y in (np.nextafter(x, f(0.0)), x, np.nextafter(x, f(2.0))):
                    v += [y, -y]
    return np.array(v, dtype=np.float32)


def make_planes(channels, n=N, seed=0xE8907):
    rng = np.random.default_rng(seed)
    sp = special_values()
    assert len(sp) < n
    out = []
    for c in range(channels):
        x = np.concatenate([sp, rng.uniform(-1.2, 1.2, n - len(sp)).astype(np.float32)])
        out.append(np.ascontiguousarray(rng.permutation(x)))
    return out


@pytest.fixture(scope="module")
def ctx():
    """one context with the 1000-frame clips every layer-1 test reads: clip 1 mono, clip 2 stereo (F32), clip 3 stereo I16"""
    c = W.MixContext(4, block=128)
    planes = {1: make_planes(1), 2: make_planes(2)}
    for ch, p in planes.items():
        c.clip_upload(ch, "f32", 48000, p)
    c.clip_upload(3, "i16", 48000, [np.arange(N, dtype=np.int16), np.arange(N, dtype=np.int16)])
    c.planes = planes
    yield c
    c.close()


def same_stats(got, want):
    return got["over"] == want["over"] and got["nans"] == want["nans"] and \
        [np.float32(x).tobytes() for x in got["peak"]] == [np.float32(x).tobytes() for x in want["peak"]]


# ---- 1: values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("channels", [1, 2])
def test_values(ctx, channels, fmt, clamp):
    planes = ctx.planes[channels]
    got, st = ctx.clip_export(channels, fmt, channels, 0, N, clamp=bool(clamp))
    want = expected_bytes(planes, fmt, clamp)
    bad = np.flatnonzero(got.view(np.uint8) != want)
    assert bad.size == 0, (fmt, clamp, bad[:8], got.view(np.uint8)[bad[:8]], want[bad[:8]])
    ws = expected_stats(planes)
    print("stats", channels, fmt, clamp, st, ws)
    assert same_stats(st, ws), (st, ws)
    assert all(o > 0 for o in ws["over"]) and all(n > 0 for n in ws["nans"]) and all(np.isinf(p) for p in ws["peak"])


def test_the_wrap_and_the_clamp_are_the_oracles():
    """1.5 as 16-bit wraps to -16386 without the clamp (the x86 conversion) and is 32767 with it; a finite peak and an
    all-NaN channel (peak 0)"""
    c = W.MixContext(4, block=128)
    x = np.array([1.5, -1.5, 0.25, np.nan] * 4, dtype=np.float32)
    y = np.full(16, np.nan, dtype=np.float32)
    c.clip_upload(0, "f32", 48000, [x, y])
    raw, st = c.clip_export(0, "i16", 2, 0, 16, clamp=False)
    assert raw.reshape(-1, 2)[:4, 0].tolist() == [-16386, 16384, 8191, 0] and not raw.reshape(-1, 2)[:, 1].any()
    cl, st2 = c.clip_export(0, "i16", 2, 0, 16, clamp=True)
    assert cl.reshape(-1, 2)[:4, 0].tolist() == [32767, -32768, 8191, 0]
    assert st == st2 == {"peak": [1.5, 0.0], "over": [8, 0], "nans": [4, 16]}
    c.close()


def test_export_into_pinned_memory(ctx):
    """dst from wbx_host_alloc: the copy engine writes it directly (no host copy out of the staging slot)"""
    L = W.lib()
    for fmt in ("i16", "i24"):
        nbytes = L.wbx_export_bytes(_ffi.OUT_FMT[fmt], 2, N - 3)
        p = C.c_void_p()
        assert L.wbx_host_alloc(nbytes, C.byref(p)) == 0
        buf = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))
        buf[:] = 0xA5
        ctx.set_export_chunk(64)
        _, st = ctx.clip_export(2, fmt, 2, 3, N - 3, out=buf)
        ctx.set_export_chunk(0)
        planes = [q[3:] for q in ctx.planes[2]]
        assert np.array_equal(buf, expected_bytes(planes, fmt, True)) and same_stats(st, expected_stats(planes))
        del buf
        assert L.wbx_host_free(p) == 0


# ---- 2: ranges ------------------------------------------------------------------------------------------------------------
RANGES = [(f, n) for f in (0, 1, 2, 3, 5, 997) for n in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, None) if f + (n or 1) <= N]


@pytest.mark.parametrize("fmt", ["i16", "i24"])
@pytest.mark.parametrize("channels", [1, 2])
def test_ranges_with_guard_bytes(ctx, channels, fmt):
    L = W.lib()
    assert len(RANGES) == 6 * 12 - 8          # first_frame 997: only 1, 2, 3 and "to the end" fit
    for first, n in RANGES:
        n = N - first if n is None else n
        nbytes = L.wbx_export_bytes(_ffi.OUT_FMT[fmt], channels, n)
        buf = np.full(nbytes + 128, 0xA5, dtype=np.uint8)
        _, st = ctx.clip_export(channels, fmt, channels, first, n, out=buf[64:64 + nbytes])
        planes = [p[first:first + n] for p in ctx.planes[channels]]
        assert np.array_equal(buf[64:64 + nbytes], expected_bytes(planes, fmt, True)), (first, n)
        assert np.all(buf[:64] == 0xA5) and np.all(buf[64 + nbytes:] == 0xA5), (first, n)
        assert same_stats(st, expected_stats(planes)), (first, n, st)


# ---- 3: chunk seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("channels", [1, 2])
def test_chunk_seams(ctx, channels, fmt):
    for first in (0, 3):
        n = N - first
        planes = [p[first:] for p in ctx.planes[channels]]
        want, ws = expected_bytes(planes, fmt, True), expected_stats(planes)
        base, bst = ctx.clip_export(channels, fmt, channels, first, n)
        assert np.array_equal(base.view(np.uint8), want) and same_stats(bst, ws)
        try:
            for chunk in (64, 8):
                ctx.set_export_chunk(chunk)
                got, st = ctx.clip_export(channels, fmt, channels, first, n)
                assert np.array_equal(got.view(np.uint8), want), (chunk, first)
                assert same_stats(st, ws), (chunk, first, st, ws)
        finally:
            ctx.set_export_chunk(0)


# ---- 4: split calls -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("channels", [1, 2])
def test_split_calls_equal_one_call(ctx, channels, fmt):
    whole, ws = ctx.clip_export(channels, fmt, channels, 0, N)
    parts, over, nans, peak = [], [0] * channels, [0] * channels, [0.0] * channels
    at = 0
    for n in (333, 333, 334):
        got, st = ctx.clip_export(channels, fmt, channels, at, n)
        parts.append(got.view(np.uint8))
        for c in range(channels):
            over[c] += st["over"][c]
            nans[c] += st["nans"][c]
            peak[c] = max(peak[c], st["peak"][c])
        at += n
    assert np.array_equal(np.concatenate(parts), whole.view(np.uint8))
    assert same_stats({"peak": peak, "over": over, "nans": nans}, ws)


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_untouched(ctx):
    L = W.lib()
    buf = np.full(8192, 0xA5, dtype=np.uint8)
    st = _ffi.ExportStats()
    I16, CL = _ffi.OUT_FMT["i16"], _ffi.EXPORT_CLAMP

    def call(clip, first, n, fmt, flags, dst=buf.ctypes.data):
        return L.wbx_clip_export(ctx.h, clip, first, n, fmt, flags, dst, C.byref(st))

    assert call(7, 0, 8, I16, CL) == -4                     # never uploaded
    assert call(1 << 30, 0, 8, I16, CL) == -4               # out of the table
    assert call(2, 0, 0, I16, CL) == -4                     # no frames
    assert call(2, N - 7, 8, I16, CL) == -4                 # ends past the clip
    assert call(2, N + 1, 1, I16, CL) == -4
    assert call(2, 1, (1 << 64) - 1, I16, CL) == -4         # first + n wraps
    assert call(2, 0, 8, I16, CL, None) == -4               # null dst
    assert call(2, 0, 8, I16, 2) == -4 and call(2, 0, 8, I16, 3) == -4 and call(2, 0, 8, I16, 1 << 31) == -4
    for fmt in (0, 1, 4, 8, 10, -1):
        assert call(2, 0, 8, fmt, CL) == -3                 # unknown output format
    assert call(3, 0, 8, I16, CL) == -3                     # an I16-format clip
    assert b"F32" in L.wbx_last_error(ctx.h)
    for bad in (4, 7, 12, 100, (1 << 24) + 8):
        assert L.wbx_set_export_chunk(ctx.h, bad) == -4
    assert np.all(buf == 0xA5)
    assert call(2, N - 8, 8, I16, CL) == 0 and not np.all(buf[:32] == 0xA5) and np.all(buf[32:] == 0xA5)


# ---- 6: through the engine ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hot():
    """2 tracks, F = 128, track 0 at +14 dB: post-fader beyond 1.0; the master and track 0 bounced over a range that is not
    a whole number of blocks"""
    spec = synth.make_session("exphot", 2, n_blocks=6, block=128, amp=0.6, seed=0xE4907)
    spec.volumes_db[0] = 14.0
    lo, hi = BU.bounce_range(spec, 6)
    eng = build_engine(spec, max_blocks=8)
    ids, n = eng.bounce(lo, hi, [("master",), ("track", 0, "post")])
    assert n % spec.block
    yield spec, eng, ids, n, lo
    eng.close()


def test_engine_master_export_equals_the_live_interleaved_blocks(hot):
    spec, eng, ids, n, lo = hot
    live = build_engine(spec, max_blocks=8)
    live.set_playhead_position(lo)
    live.play()
    blocks = [live.process_interleaved("i16") for _ in range(-(-n // spec.block))]
    live.close()
    want = np.concatenate(blocks)[:n * spec.channels]
    for clamp in (True, False):   # the master is clamped already
        got, st = eng.export_sample(ids[0], "i16", clamp=clamp)
        assert got.dtype == np.int16 and np.array_equal(got, want)
        assert st["over"] == [0, 0] and st["nans"] == [0, 0]


def test_engine_stem_export_clamps_and_counts(hot):
    spec, eng, ids, n, lo = hot
    stem = eng.bounce_download(ids[1], n)
    planes = [np.ascontiguousarray(stem[c]) for c in range(spec.channels)]
    ws = expected_stats(planes)
    assert all(o > 0 for o in ws["over"]) and max(ws["peak"]) > 1.0
    got, st = eng.export_sample(ids[1], "i16", clamp=True)
    assert np.array_equal(got.view(np.uint8), expected_bytes(planes, "i16", True)) and same_stats(st, ws)
    raw, st = eng.export_sample(ids[1], "i16", clamp=False)
    want = expected_bytes(planes, "i16", False)
    assert np.array_equal(raw.view(np.uint8), want) and same_stats(st, ws)
    il = np.stack(planes, axis=1).reshape(-1)
    wrapped = (il > 1.001) & (il < 1.9)
    assert wrapped.any() and np.all(raw[wrapped] < 0) and np.all(got[wrapped] == 32767)   # the wrap the oracle shows
    # a partial range through the engine, packed 24-bit
    p24, _ = eng.export_sample(ids[1], "i24", first_frame=5, n_frames=301)
    assert np.array_equal(p24, expected_bytes([p[5:306] for p in planes], "i24", True))


def test_engine_refusals(hot):
    spec, eng, ids, n, lo = hot
    L = W.lib()
    buf = np.full(4096, 0xA5, dtype=np.uint8)
    st = _ffi.ExportStats()
    call = lambda s, first, cnt, fmt, flags, dst: L.wbx_engine_export_sample(eng.h, s, first, cnt, fmt, flags, dst, C.byref(st))
    d = buf.ctypes.data
    assert call(999, 0, 8, 3, 1, d) == -4 and b"sample" in L.wbx_engine_last_error(eng.h)
    assert call(ids[0], 0, 0, 3, 1, d) == -4 and call(ids[0], n - 1, 2, 3, 1, d) == -4 and call(ids[0], 0, 8, 3, 1, None) == -4
    assert call(ids[0], 0, 8, 3, 4, d) == -4 and call(ids[0], 0, 8, 4, 1, d) == -3
    i16 = eng.add_sample("i16", 48000, [np.arange(64, dtype=np.int16)] * 2)
    assert call(i16, 0, 8, 3, 1, d) == -3
    assert np.all(buf == 0xA5)
    eng.delete_sample(i16)


# ---- 7: a take ------------------------------------------------------------------------------------------------------------
def test_a_take_exports_bit_equal_to_its_input():
    spec = synth.make_session("exptake", 2, n_blocks=4, block=128, seed=0xE7A4E)
    eng = build_engine(spec, max_blocks=1)
    eng.set_audio_channel_config(1, spec.channels, spec.block, spec.sample_rate)
    eng.set_track_input(1, "external_mono", 0, True)
    rng = np.random.default_rng(7)
    x = rng.uniform(-2.5, 2.5, 3 * spec.block).astype(np.float32)
    x[[5, 200, 383]] = [3.25, -7.5, 1.0]
    inp, out = W.AudioBuffer(spec.block, 1), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for b in range(3):
        inp.channel_buffers[0][:] = x[b * spec.block:(b + 1) * spec.block]
        eng.process(inp, out, float(spec.sample_rate))
    frames = eng.record_info(1)["frames"]
    eng.stop_record()
    assert frames == 3 * spec.block
    sid = max(c[5] for c in eng.clips(eng.tracks[1]))
    got, st = eng.export_sample(sid, "f32", clamp=False, channels=1, frames=frames)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x.view(np.uint32))
    assert same_stats(st, expected_stats([x])) and st["peak"] == [7.5]
    eng.close()


# ---- 8: while the audio thread runs ------------------------------------------------------------------------------------------
def test_export_while_the_audio_thread_processes():
    NB, FR = 200, 1 << 16
    spec = synth.make_session("expthr", 2, n_blocks=NB, block=128, seed=0xE7812)

    def run_blocks(eng, sink):
        out = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        for _ in range(NB):
            eng.process(None, out, float(spec.sample_rate))
            sink.append(np.stack(out.channel_buffers).copy())

    alone = []
    ref = build_engine(spec, max_blocks=1)
    run_blocks(ref, alone)
    ref.close()

    eng = build_engine(spec, max_blocks=1)
    rng = np.random.default_rng(11)
    planes = [rng.uniform(-1.3, 1.3, FR).astype(np.float32) for _ in range(2)]
    sid = eng.add_sample("f32", 48000, planes)
    eng.ctx.set_export_chunk(4096)
    want = expected_bytes(planes, "i16", True)
    dst = np.full(want.size, 0xA5, dtype=np.uint8)
    assert not np.all(want[-64:] == 0xA5) and not np.all(want[:64] == 0xA5)
    L = W.lib()
    began, finished = threading.Event(), threading.Event()
    heard, attempts = [], []

    def deleter():
        began.wait()
        while np.all(dst[:64] == 0xA5) and not finished.is_set():   # the export has begun: its first chunk is in dst
            pass
        while True:
            st = L.wbx_engine_delete_sample(eng.h, sid)
            tail_written = not np.all(dst[-64:] == 0xA5)      # read AFTER the call returned
            attempts.append((st, tail_written, L.wbx_engine_last_error(eng.h) if st else b""))
            if st == 0:
                return
            finished.wait()

    audio = threading.Thread(target=run_blocks, args=(eng, heard))
    third = threading.Thread(target=deleter)
    audio.start()
    third.start()
    began.set()
    got, st = eng.export_sample(sid, "i16", out=dst)
    finished.set()
    third.join()
    audio.join()
    assert np.array_equal(dst, want) and same_stats(st, expected_stats(planes))
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    # a delete never succeeds mid-export: a successful one found the export's last chunk already in dst; a refused one
    # says why, and the delete after the export is the one that succeeds
    assert 1 <= len(attempts) <= 2 and attempts[-1][0] == 0 and attempts[-1][1], attempts
    for stt, _, msg in attempts[:-1]:
        assert stt == -3 and b"being exported" in msg, attempts
    with pytest.raises(W.WbxError) as ex:
        eng.export_sample(sid, "i16", n_frames=8)
    assert ex.value.status == -4
    eng.close()


# ---- 9: WAV round trip -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 24])
def test_wav_round_trip(hot, tmp_path, bits):
    spec, eng, ids, n, lo = hot
    path = str(tmp_path / f"master{bits}.wav")
    total = wav.write_sample(eng, ids[0], path, bits=bits, piece_frames=200)     # several bounded calls
    master = eng.bounce_download(ids[0], n)
    planes = [np.ascontiguousarray(master[c]) for c in range(spec.channels)]
    with wave.open(path, "rb") as r:
        assert (r.getnchannels(), r.getsampwidth(), r.getframerate(), r.getnframes()) == (spec.channels, bits // 8, spec.sample_rate, n)
        data = r.readframes(n)
    assert data == expected_bytes(planes, "i16" if bits == 16 else "i24", True).tobytes()
    assert same_stats(total, expected_stats(planes))
