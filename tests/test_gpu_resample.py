"""wbx_clip_resample and wbx_engine_resample_sample on the device.  Results come back through wbx_clip_download and are
compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/resample_model.py, the numpy twin of the header's
text.  Shapes are the smallest at which the kernel can still go wrong: range lengths around the filter's half width H and
its T taps (every tap of some output masked at one end, at both, at neither), around the 512 frames of half a tile, more
than one tile; ranges that start at the clip's frame 0 and ranges that end at its last frame, inside a clip whose frames
beside the range are NOT zero."""
import ctypes as C
import math
import struct
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import oracle_ffi as O
import resample_model as M
import second_pass as SP
import whitebox_amd as W
from whitebox_amd import _ffi, synth, wav
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (48000, 44100), (96000, 48000), (48000, 96000), (48000, 32000), (8000, 44100)]
QUALITIES = (M.FAST, M.GOOD, M.BEST)
FIRSTS = [0, 1, 5, 8 * 37 + 3]
CLIP_LEN = 6000
DST = 100
bits = BU.bits
_tab = {}


def table(rs, rd, q):
    if (rs, rd, q) not in _tab:
        _tab[(rs, rd, q)] = M.table(rs, rd, q)
    return _tab[(rs, rd, q)]


def model(planes, first, n, rs, rd, q, window=None):
    return M.resample(planes, first, n, rs, rd, q, window=window, tab=table(rs, rd, q))


def lengths(rs, rd, q):
    p = M.plan(rs, rd, q)
    return [1, 2, p["H"] - 1, p["H"], p["T"] - 1, p["T"], p["T"] + 1, 511, 513, 5003]


def clip_id(channels, rate):
    return 1 + sorted({p[0] for p in PAIRS}).index(rate) * 2 + (channels - 1)


def source(channels, rate):
    rng = np.random.default_rng(0x5AC + 7 * rate + channels)
    return [rng.uniform(-1.2, 1.2, CLIP_LEN).astype(np.float32) for _ in range(channels)]


def matrix_cases():
    """a sparse draw over the axes of the matrix; the asserts below are the coverage asked for"""
    rng = np.random.default_rng(0x5EC0DE)
    out = []
    for pair in PAIRS:
        for q in QUALITIES:
            for li in range(10):
                n = lengths(*pair, q)[li]
                at_end = bool(rng.integers(4) == 0)
                first = CLIP_LEN - n if at_end else FIRSTS[int(rng.integers(4))]
                out.append((pair[0], pair[1], q, int(rng.integers(1, 3)), li, n, first))
    seen = lambda i: {c[i] for c in out}
    assert {(c[0], c[1]) for c in out} == set(PAIRS) and seen(2) == set(QUALITIES) and seen(3) == {1, 2} and seen(4) == set(range(10))
    assert set(FIRSTS) <= seen(6) and {(c[2], c[0] < c[1]) for c in out} == {(q, up) for q in QUALITIES for up in (False, True)}
    assert {(c[2], c[3]) for c in out} == {(q, ch) for q in QUALITIES for ch in (1, 2)}
    assert any(c[6] == 0 for c in out) and any(c[6] + c[5] == CLIP_LEN for c in out) and all(c[6] + c[5] <= CLIP_LEN for c in out)
    assert {c[3] for c in out if c[6] == 0} == {1, 2} == {c[3] for c in out if c[6] + c[5] == CLIP_LEN}
    return out


CASES = matrix_cases()


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {}
    for rate in sorted({p[0] for p in PAIRS}):
        for ch in (1, 2):
            c.src[(ch, rate)] = source(ch, rate)
            c.clip_upload(clip_id(ch, rate), "f32", rate, c.src[(ch, rate)])
    yield c
    c.close()


def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def mismatches(got, want):
    return [int(np.count_nonzero(g.view(np.uint32) != w.view(np.uint32))) for g, w in zip(got, want)]


def check_stats(got, want, n, where):
    """wbx_clip_measure's rules: every field but sum / sum_sq exact, those two within any-order fp64 summation's bound"""
    assert FX.exact_fields_equal(got, want), (where, got, {k: want[k] for k in FX.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if math.isfinite(a):
                print(where, k, "error", abs(g - w), "bound", n * 2.0 ** -52 * a)
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


# ---- 1: the matrix --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_resample_matrix(ctx, case):
    rs, rd, q, ch, _, n, first = case
    want = model(ctx.src[(ch, rs)], first, n, rs, rd, q)
    n_out = W.resample_frames(rs, rd, n)
    assert n_out == len(want[0]) == -(-n * rd // rs)
    st = ctx.clip_resample(clip_id(ch, rs), DST, first, n, rd, q, stats_channels=ch)
    got = download(ctx, DST, ch, n_out)
    assert bits(np.stack(got)).tolist() == bits(np.stack(want)).tolist()
    check_stats(st, FX.measure(want), n_out, "stats_of_result")


# ---- 2: every tile seam of one pass of the grid (some 280 tiles, each with a workgroup of its own; the second pass is section 3b's)
@pytest.fixture(scope="module")
def big():
    c = W.MixContext(4, block=128)
    n = SP.RESAMPLE_SEAMS_FRAMES
    rng = np.random.default_rng(0x5EA6)
    c.planes = [rng.uniform(-1.1, 1.1, n).astype(np.float32) for _ in range(2)]
    c.clip_upload(1, "f32", 44100, c.planes)
    c.clip_upload(2, "f32", 48000, c.planes)
    yield c, n
    c.close()


@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100)], ids=lambda p: "%d-%d" % p)
def test_tile_seams(big, pair):
    """the whole result of some 280 tiles, both directions of 44100 <-> 48000: every seam between two tiles.  No workgroup takes
    a second tile here (tests/test_second_pass_host.py holds that against the launch's own shape)"""
    c, n = big
    rs, rd = pair
    want = model(c.planes, 0, n, rs, rd, M.GOOD)
    n_out = len(want[0])
    st = c.clip_resample(1 if rs == 44100 else 2, 3, 0, n, rd, "good", stats_channels=2)
    got = download(c, 3, 2, n_out)
    for k in range(2):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, (k, bad[:8], bad.size)
    check_stats(st, FX.measure(want), n_out, "seams stats_of_result")
    check_stats(st, FX.measure(got), n_out, "seams stats against the download")
    check_stats(c.clip_measure(3, 2, 0, n_out), FX.measure(want), n_out, "seams wbx_clip_measure")


# ---- 3: positions past 2^32 -----------------------------------------------------------------------------------------------------
SynthPlane = SP.SynthPlane


def test_positions_past_2_to_the_32():
    """192000 -> 44100 at FAST: M = 640, so j * M passes 2^32 at output frame 6 710 887 (a 32-bit product would wrap there)"""
    rs, rd, q = 192000, 44100, M.FAST
    n = 29_300_000                                              # 117 MB of mono fp32
    n_out = W.resample_frames(rs, rd, n)
    cross = (1 << 32) // 640
    assert n_out > cross + 4096 + 2048 and (n_out - 1) * 640 > 1 << 32
    c = W.MixContext(4, block=128)
    seed, track, amp = 0xB16_5EED, 3, 0.75
    c.clip_synth(1, "f32", 1, rs, n, seed, track, amp)
    c.clip_resample(1, 2, 0, n, rd, q)
    got = c.clip_download(2, 0, n_out, np.float32)
    plane = SynthPlane(seed, track, 0, n, amp)
    for j0, j1 in ((cross - 2048, cross + 2048), (n_out - 4096, n_out), (0, 4096)):
        want = model([plane], 0, n, rs, rd, q, window=(j0, j1))[0]
        bad = np.flatnonzero(got[j0:j1].view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (j0, bad[:8], bad.size)
    c.close()


# ---- 3b: the second pass of the grid ----------------------------------------------------------------------------------------
def export_window(c, clip, channels, j0, j1):
    """frames [j0, j1) of a resident clip as [channels] float32 planes, through wbx_clip_export (unclamped f32: the stored bits)"""
    out, _ = c.clip_export(clip, "f32", channels, j0, j1 - j0, clamp=False)
    return [np.ascontiguousarray(out.reshape(-1, channels)[:, k]) for k in range(channels)]


@pytest.mark.parametrize("rs,rd,q,channels", [(8000, 192000, "good", 1), (22050, 192000, "fast", 2)], ids=["24-1-good-mono", "1280-147-fast-stereo"])
def test_tiles_past_the_grid_cap(rs, rd, q, channels):
    """Upsampling, so that the tile is 1024 outputs and the source stays small: n_out has G + 3 tiles, G the grid's cap
    (tests/second_pass.py, from wbx_resample_launch_shape), so workgroups 0, 1 and 2 take a second tile.  L = 24 and L = 1280
    are the two ends of the table; the stereo result ends inside a 16-byte word (every result of 24 : 1 is a multiple of 24
    frames long).  Compared bit for bit: the first three tiles — the same workgroups' first pass —, the frames around tile G's
    first, and everything from tile G - 2 to the end: the whole second pass and the last lane's partial store.  A conversion of
    the same range at another quality is made and freed first: the memory the result then gets held other frames, so a
    skipped tile shows."""
    n, n_out, sh, G = SP.resample_case(rs, rd, q)
    tile = sh["tile"]
    assert sh["n_tiles"] == G + 3 > sh["grid"] == G and (channels == 1 or n_out % 4)
    qi = _ffi.SRC_QUALITY[q]
    c = W.MixContext(4, block=128)
    seed, track, amp = 0x2D_9A55 + channels, 5, 0.75
    c.clip_synth(1, "f32", channels, rs, n, seed, track, amp)
    planes = [SynthPlane(seed, track, k, n, amp) for k in range(channels)]
    c.clip_resample(1, 2, 0, n, rd, "best")                     # fills the memory the result is about to get
    assert c.L.wbx_clip_free(c.h, 2) == 0
    st = c.clip_resample(1, 3, 0, n, rd, q, stats_channels=channels if channels == 2 else 0)
    for j0, j1 in ((0, 3 * tile), (G * tile - 2048, G * tile + 2048), ((G - 2) * tile, n_out)):
        want = model(planes, 0, n, rs, rd, qi, window=(j0, j1))
        got = export_window(c, 3, channels, j0, j1)
        for k in range(channels):
            bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
            assert bad.size == 0 and got[k].size == j1 - j0, (j0, k, bad[:8], bad.size)
    if st is not None:                                          # stats_of_result is wbx_clip_measure of the result (pinned by test_gpu_clipfx.py)
        again = c.clip_measure(3, channels, 0, n_out)
        assert FX.exact_fields_equal(st, again) and all(p > 0 for p in st["peak"]), (st, again)
        # two any-order fp64 sums of the same terms: each within check_stats' n * 2^-52 * (sum of magnitudes) of the exact
        # sum, so within twice that of each other; the magnitudes of sum's terms add up to at most sqrt(n * sum_sq)
        for k in range(channels):
            mags = {"sum": math.sqrt(n_out * again["sum_sq"][k]) * (1 + 2.0 ** -40), "sum_sq": again["sum_sq"][k]}
            for f in ("sum", "sum_sq"):
                assert abs(st[f][k] - again[f][k]) <= 2 * n_out * 2.0 ** -52 * mags[f], (f, k, st[f][k], again[f][k])
    c.close()


# ---- 4: special values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100)], ids=lambda p: "%d-%d" % p)
def test_special_values(ctx, pair, channels):
    rs, rd = pair
    n = 1700
    rng = np.random.default_rng(0x5bec + channels)
    planes = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(channels)]
    for k, p in enumerate(planes):
        o = 3 * k
        p[100 + o] = np.nan
        p[300 + o], p[500 + o] = np.inf, -np.inf                # each alone: more than T frames apart
        p[700 + o] = -0.0
        p[800 + o] = 1e-40
        p[900 + o:902 + o] = 3e38                               # neighbours whose weighted sum overflows fp32
        p[1000 + o:1002 + o] = -3e38
        p[1200 + o], p[1210 + o] = np.inf, -np.inf              # inside one window: inf - inf
        p[1400 + o:1500 + o] = 1e-40                            # a stretch of denormals: denormal results
        p[1600:] = 0.0
        p[1650 + o] = -0.0
    planes[0].view(np.uint32)[110] = 0xFFC12345                 # a NaN with a payload and a sign
    ctx.clip_upload(50, "f32", rs, planes)
    want = model(planes, 0, n, rs, rd, M.GOOD)
    n_out = len(want[0])
    st = ctx.clip_resample(50, DST, 0, n, rd, "good", stats_channels=channels)
    got = download(ctx, DST, channels, n_out)
    assert bits(np.stack(got)).tolist() == bits(np.stack(want)).tolist()
    w = np.stack(want)
    nan = np.isnan(w)
    assert nan.any() and np.all(w.view(np.uint32)[nan] == 0x7FC00000) and np.isinf(w).any()
    assert np.any((w != 0) & (np.abs(w) < 1e-38)), "no denormal result: the case checks nothing about them"
    check_stats(st, FX.measure(want), n_out, "specials stats_of_result")


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    s2, s1 = clip_id(2, 44100), clip_id(1, 48000)
    ctx.clip_resample(s2, DST, 0, 64, 48000, "fast")
    kept_n = W.resample_frames(44100, 48000, 64)
    ctx.clip_upload(60, "i16", 44100, [np.arange(64, dtype=np.int16)] * 2)
    ctx.clip_upload(61, "f32", 11025, [np.ones(64, dtype=np.float32)])
    ctx.clip_upload(62, "f32", 192000, [np.ones(64, dtype=np.float32)])
    ctx.clip_synth(63, "f32", 1, 150, 1_700_000, 7, 0, 0.5)     # 150 -> 192000 Hz: L = 1280, M = 1: n_out = 2.18e9
    kept = bits(np.stack(download(ctx, DST, 2, kept_n))).tolist()
    st = _ffi.ClipStats()

    def refused(status, src, dst, first, n, rate, q):
        before = ctx.pool_stats()
        got = L.wbx_clip_resample(ctx.h, src, dst, first, n, rate, q, C.byref(st))
        assert got == status, (got, status, src, dst, first, n, rate, q, L.wbx_last_error(ctx.h))
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, kept_n))).tolist() == kept

    refused(-4, 999, DST, 0, 64, 48000, 1)                      # unknown source
    refused(-4, s2, DST, 0, 0, 48000, 1)                        # no frames
    refused(-4, s2, DST, CLIP_LEN - 10, 11, 48000, 1)           # past the clip
    refused(-4, s2, DST, CLIP_LEN + 1, 1, 48000, 1)
    refused(-4, DST, DST, 0, 8, 44100, 1)                       # dst == src
    refused(-4, s2, DST, 0, 64, 48000, 3)                       # unknown quality
    refused(-4, s2, DST, 0, 64, 48000, -1)
    refused(-4, s2, DST, 0, 64, 0, 1)                           # dst_rate 0
    refused(-4, s2, DST, 0, 64, 44100, 1)                       # the source's own rate
    refused(-4, 63, DST, 0, 1_700_000, 192000, 0)               # n_out >= 2^31 - 16
    assert W.resample_frames(150, 192000, 1_700_000) == 0 and W.resample_frames(150, 192000, 1_600_000) == 2_048_000_000
    refused(-3, 60, DST, 0, 64, 48000, 1)                       # not F32 (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, 61, DST, 0, 64, 192000, 1)                      # L = 2560
    refused(-3, 62, DST, 0, 64, 32000, 2)                       # T = 576
    ctx.clip_resample(62, DST + 1, 0, 64, 32000, "good")        # ... and GOOD (T = 288) is accepted
    assert bits(download(ctx, DST + 1, 1, 11)[0]).tolist() == bits(model([np.ones(64, dtype=np.float32)], 0, 64, 192000, 32000, M.GOOD)[0]).tolist()
    assert ctx.L.wbx_clip_free(ctx.h, DST + 1) == 0
    assert s1 != s2


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    rng = np.random.default_rng(5)
    planes = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(2)]
    c.clip_upload(1, "f32", 48000, planes)                      # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_resample(1, 10 + len(made), 0, n, 96000, "fast")     # 16 MiB each
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            assert c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    want = model(planes, 0, n, 48000, 96000, M.FAST, window=(2 * n - 4096, 2 * n))
    got = download(c, made[-1], 2, 2 * n)
    assert mismatches([g[-4096:] for g in got], want) == [0, 0]
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.pool_limit(0)
    c.close()


# ---- 6: through the engine ------------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def replace_track(eng, e, t, sample, osample, lo, hi):
    while e.clips(t):
        e.delete_clip(t, 0)
    while eng.clips(eng.tracks[t]):
        eng.delete_clip(eng.tracks[t], 0)
    assert e.add_audio_clip(t, lo, hi, 0.0, osample, 1.0, 1.0) == 0
    eng.add_audio_clip(eng.tracks[t], "conformed", lo, hi, 0.0, sample, 1.0, 1.0)


@pytest.mark.parametrize("callback", [False, True], ids=["batch", "callback"])
def test_a_file_conformed_to_the_session_rate_plays_as_the_models_clip(callback, tmp_path):
    NB, t = 6, 1
    spec = synth.make_session("rsconform", 3, n_blocks=NB, block=128, seed=0x5AC0F0)
    eng = build_engine(spec, max_blocks=1 if callback else 8)
    e = O.build_oracle_engine(spec)
    rng = np.random.default_rng(41)
    n = 2000
    planes = [rng.uniform(-0.4, 0.4, n).astype(np.float32) for _ in range(2)]
    src = eng.add_sample("f32", 44100, planes)
    new = eng.resample_sample(src, spec.sample_rate, "good", src_rate=44100)
    want = model(planes, 0, n, 44100, spec.sample_rate, M.GOOD)
    n_out = len(want[0])
    assert eng._sample_shape[new] == (n_out, 2)
    assert bits(np.stack(download(eng.ctx, new, 2, n_out))).tolist() == bits(np.stack(want)).tolist()
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    replace_track(eng, e, t, new, oracle_sample(e, want, spec.sample_rate), 0.5 * unit, 4.5 * unit)
    e.play()
    eng.play()
    if callback:
        out = W.AudioBuffer(spec.block, spec.channels)
        rows = []
        for b in range(NB):
            eng.process(None, out, float(spec.sample_rate))
            om, _ = e.process()
            assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), b
            rows += [r for r in eng.fetch_plan() if r[1] == t]
        assert len(rows) >= 4 and all(r[5] == new and r[7] == 1.0 for r in rows), rows
    else:
        eng.render(NB)
        m, _, _ = eng.ctx.fetch()
        for b in range(NB):
            om, _ = e.process()
            assert np.array_equal(bits(m[b]), bits(om)), b
        rows = [r for r in eng.fetch_plan() if r[1] == t]
        assert len(rows) >= 4 and all(r[5] == new and r[7] == 1.0 for r in rows), rows     # the unity row mode: speed exactly 1
    # the new sample is an ordinary one, registered at the session's rate: exportable, deletable once no clip names it
    got, _ = eng.export_sample(new, "f32", clamp=False)
    assert np.array_equal(got.view(np.uint32), np.stack(want, axis=1).reshape(-1).view(np.uint32))
    with pytest.raises(W.WbxError):
        eng.delete_sample(new)
    with pytest.raises(W.WbxError) as ex:
        eng.resample_sample(new, spec.sample_rate, "good")      # it HAS the session's rate now
    assert ex.value.status == -4
    back = eng.resample_sample(new, 44100, "best", src_rate=spec.sample_rate)
    assert bits(np.stack(download(eng.ctx, back, 2, W.resample_frames(48000, 44100, n_out)))).tolist() == \
        bits(np.stack(model(want, 0, n_out, 48000, 44100, M.BEST))).tolist()
    # ... and leaves as a file at ITS rate, not the session's
    path = str(tmp_path / "back.wav")
    wav.write_sample(eng, back, path, bits=32, float32=True)
    head = open(path, "rb").read(28)
    assert struct.unpack("<I", head[24:28])[0] == 44100
    wav.write_sample(eng, new, path, bits=16)
    assert struct.unpack("<I", open(path, "rb").read(28)[24:28])[0] == spec.sample_rate
    eng.delete_sample(src)
    eng.close()
    e.close()


# ---- 7: beside the audio thread -------------------------------------------------------------------------------------------------
def test_conversions_beside_the_audio_thread():
    """The shape of the edits' test (test_gpu_clipfx.py): a clip far behind the played range names the big sample while the
    threads run, so a delete of it can never succeed — between two conversions it is refused for the clip (-4), inside one
    for the pin (-3, asked first) — one thread deletes without pause while the other converts until a refusal for the pin
    has been seen.  The master is what it is without the conversions."""
    NB, FR, WAIT, CALLS = 300, 1 << 20, 60.0, 64
    spec = synth.make_session("rsthr", 2, n_blocks=NB, block=128, seed=0x5A7812)
    rng = np.random.default_rng(31)
    planes = [rng.uniform(-1.0, 1.0, FR).astype(np.float32) for _ in range(2)]

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
    playing = sorted({c[5] for t in eng.tracks for c in eng.clips(t)})[:2]      # samples the session is playing (48 kHz)
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
                results[("id", s)] = eng.resample_sample(s, 44100, "fast", first_frame=1, n_frames=min(fr - 1, 4099), channels=ch)
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"] = eng.resample_sample(big, 48000, "good", first_frame=first, n_frames=n, channels=2)
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
    print("resample calls", results["calls"], "deletes", {k: v for k, v in seen.items()})
    pinned = [k for k in seen if k[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every conversion read a live source: the results are the model's, bit for bit
    n_out = W.resample_frames(44100, 48000, n)
    got = download(eng.ctx, results["big"], 2, n_out)
    assert mismatches(got, model(planes, first, n, 44100, 48000, M.GOOD)) == [0, 0]
    for s in playing:
        fr, ch = shapes[s]
        src = download(eng.ctx, s, ch, fr)
        m = min(fr - 1, 4099)
        assert bits(np.stack(download(eng.ctx, results[("id", s)], ch, W.resample_frames(48000, 44100, m)))).tolist() == \
            bits(np.stack(model(src, 1, m, 48000, 44100, M.FAST))).tolist()
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    new = C.c_uint32(12345)
    assert L.wbx_engine_resample_sample(eng.h, big, 0, 8, 48000, 1, C.byref(new)) == -4 and new.value == 12345
    eng.close()
