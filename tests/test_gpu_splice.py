"""wbx_clip_splice and wbx_engine_splice_samples on the device.  Spliced clips come back through wbx_clip_download and are
compared BIT FOR BIT (uint32 views: -0.0 and NaN payloads show) with tests/splice_model.py; statistics as in
tests/test_gpu_clipfx.py.  Shapes are the smallest at which the kernel can still go wrong: a lane owns 8 output frames, a
wave one tile of 512, a workgroup 4 tiles; the usual result has 2573 frames — two workgroups and a ragged last lane."""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as M
import oracle_ffi as O
import splice_model as S
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

N = 2573
DST, TMP = 100, 101
P = S.Part
bits = BU.bits
GAINS = [1.0, -1.0, 0.5, float(np.array([0x3F353BEF], dtype=np.uint32).view(np.float32)[0])]
SRC_SHAPES = {1: (1, 3000), 2: (2, 3000), 3: (1, 1000), 4: (2, 2000)}     # clip id -> (channels, frames), all at 48 kHz


def source(clip):
    ch, n = SRC_SHAPES[clip]
    rng = np.random.default_rng(0x5B11CE + clip)
    planes = [rng.uniform(-1.4, 1.4, n).astype(np.float32) for _ in range(ch)]
    for p in planes:
        p[[0, 5, n - 1]] = [-0.0, 0.0, -0.0]
    return planes


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {}
    for clip in SRC_SHAPES:                                   # clip 1 is the first clip of the fresh context's first slab
        c.src[clip] = source(clip)
        c.clip_upload(clip, "f32", 48000, c.src[clip])
    yield c
    c.close()


def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def check_stats(got, want, n, where):
    assert M.exact_fields_equal(got, want), (where, got, {k: want[k] for k in M.EXACT})
    for k, mag in (("sum", "abs_sum"), ("sum_sq", "abs_sum_sq")):
        for g, w, a in zip(got[k], want[k], want[mag]):
            if math.isfinite(a):
                assert abs(g - w) <= n * 2.0 ** -52 * a, (where, k, g, w)


def same_bits(got, want, where=""):
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(bits(g) != bits(w))
        assert bad.size == 0, (where, c, bad[:8].tolist(), bad.size, g[bad[:4]].tolist(), w[bad[:4]].tolist())
    assert len(got) == len(want)


def run(c, channels, n_frames, parts, stats=True, dst=DST, where=""):
    """the splice on the device against the model; -> the model's planes"""
    want = S.splice(c.src, channels, n_frames, parts)
    st = c.clip_splice(dst, channels, n_frames, [S.to_ffi(W, p) for p in parts], stats=stats)
    same_bits(download(c, dst, channels, n_frames), want, where)
    if stats:
        check_stats(st, M.measure(want), n_frames, where)
    return want


def modes_into(src_channels, channels):
    return [m for m in M.MODES_FOR[src_channels] if M.out_channels(src_channels, m) == channels]


# ---- 1: one part is wbx_clip_derive -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("clip,mode", [(c, m) for c in (1, 2) for m in M.MODES_FOR[SRC_SHAPES[c][0]]])
def test_one_part_equals_clip_derive(ctx, clip, mode, reverse):
    first, fi, fo = 0, 300, 700                               # (frames 0 and 5 are -0.0 / +0.0: kept by gain 1, swapped by -1)
    for gain in (1.0, -1.0):
        ctx.clip_derive(clip, TMP, W.edit_desc(first, N, reverse, mode, gain, fi, fo, "smooth", "square"))
        ch = M.out_channels(SRC_SHAPES[clip][0], mode)
        derived = download(ctx, TMP, ch, N)
        want = run(ctx, ch, N, [P(clip, first, N, 0, reverse, mode, gain, fi, fo, M.SMOOTH, M.SQUARE)], where=(clip, mode, reverse, gain))
        same_bits(derived, want, "derive")
        assert np.any(bits(np.stack(want)) == 0x80000000)     # a -0.0 survived


# ---- 2: the matrix ----------------------------------------------------------------------------------------------------------------
def matrix_cases():
    rng = np.random.default_rng(0xC0FADE)
    out = []
    for k in range(16):
        channels = 1 + k % 2
        parts = []
        for i in range(int(rng.integers(3, 6))):
            clip = int(rng.integers(1, 5)) if i else 1 + (k // 2) % 4
            sc, frames = SRC_SHAPES[clip]
            n = int(rng.integers(1, min(frames, N) + 1))
            first = int(rng.integers(0, frames - n + 1))
            at = int(rng.integers(0, N - n + 1))
            if i == 0 and n > 9:                              # at % 8 != 0 and first_frame % 4 != 0 in every case
                n -= 8
                first, at = first | 1, at | 1
            fi, fo = (int(rng.integers(0, n + 1)) for _ in range(2))
            parts.append(P(clip, first, n, at, bool(rng.integers(2)), int(rng.choice(modes_into(sc, channels))), GAINS[int(rng.integers(4))],
                           fi, fo, int(rng.integers(3)), int(rng.integers(3))))
        out.append((channels, parts))
    flat = [(ch, p) for ch, parts in out for p in parts]
    assert {(SRC_SHAPES[p.src][0], ch) for ch, p in flat} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {p.mode for _, p in flat} == set(range(6)) and {p.shape_in for _, p in flat} == {p.shape_out for _, p in flat} == {0, 1, 2}
    assert all(any(p.at % 8 and p.first % 4 for p in parts) for _, parts in out)
    assert {p.reverse for _, p in flat} == {False, True}
    return out


@pytest.mark.parametrize("case", list(enumerate(matrix_cases())), ids=lambda c: "m%d" % c[0])
def test_matrix(ctx, case):
    k, (channels, parts) = case
    run(ctx, channels, N, parts, where=("matrix", k))


# ---- 3: seams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [7, 8, 9, 511, 512, 513])
@pytest.mark.parametrize("reverse", [False, True])
def test_parts_that_start_and_end_at_lane_and_tile_edges(ctx, edge, reverse):
    run(ctx, 2, N, [P(2, 3, edge, 0, reverse, M.KEEP, 0.5), P(4, 1, 600, edge, reverse, M.SWAP, 1.0, 9, 9)], where=("abut", edge))
    run(ctx, 2, N, [P(2, 0, N, 0), P(4, 5, edge, 1024 - edge, reverse), P(1, 2, 777, edge, reverse, M.DUAL_MONO, -1.0, 5, 0)],
        where=("over", edge))
    run(ctx, 1, N, [P(2, 9, 900, edge, reverse, M.MONO_MIX), P(3, 0, 1000 - edge, N - (1000 - edge), reverse)], where=("mono", edge))


def test_a_one_frame_part_alone_and_over_another(ctx):
    for at in (0, 7, 8, 511, 512, N - 1):
        run(ctx, 1, N, [P(1, 17, 1, at, gain=-1.0)], where=("alone", at))
        run(ctx, 2, N, [P(2, 100, 2000, 300), P(4, 1999, 1, max(at, 300), True, fade_in=0)], where=("over", at))


def test_parts_at_the_ends_of_their_clips():
    """a fresh context: clip 1 is the first clip of its first slab, nothing readable lies in front of its frame 0"""
    c = W.MixContext(4, block=128)
    c.src = {1: source(1), 2: source(2)}
    c.clip_upload(1, "f32", 48000, c.src[1])
    c.clip_upload(2, "f32", 48000, c.src[2])
    for reverse in (False, True):
        run(c, 1, N, [P(1, 0, 1000, 3, reverse), P(1, 0, 5, 1500, reverse), P(1, 0, 13, 2001, reverse)], where=("frame 0", reverse))
        for first in range(7):                                # reversed with first_frame < 7: the mirrored words would start before the range
            run(c, 1, N, [P(1, first, 8 + first, 40 + first, reverse, fade_in=3)], stats=False, where=("first", first, reverse))
        run(c, 2, N, [P(2, 3000 - 1100, 1100, 1, reverse), P(2, 3000 - 9, 9, 2564, reverse), P(1, 3000 - 512, 512, 1024, reverse, M.DUAL_MONO)],
            where=("last frame", reverse))
    c.close()


@pytest.mark.parametrize("shape", [M.LINEAR, M.SQUARE, M.SMOOTH])
def test_fades_that_end_on_tile_edges(ctx, shape):
    # the fade-in's last frame is output frame 511 / 1023, the fade-out's first one is output frame 1024 / 512
    run(ctx, 2, N, [P(2, 1, 1500, 12, False, M.KEEP, 1.0, 500, 1500 - (1024 - 12), shape, shape)], where="forward")
    run(ctx, 1, N, [P(1, 2, 2000, 0, True, M.KEEP, 0.5, 1024, 2000 - 512, shape, shape)], where="reversed")
    run(ctx, 1, N, [P(3, 0, 512, 512, False, M.KEEP, 1.0, 512, 512, shape, shape)], where="one tile, both fades whole")


# ---- 4: depth and order -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3, 9])
def test_depth_with_order_sensitive_values(ctx, depth):
    """the same frames covered `depth` times by values whose sum depends on the order: gains 1e8, 1, -1e8, ..."""
    big = float(np.float32(1e8))
    gains = [big, 1.0, -big, 3.0, -big, big, 0.25, -1.0, big][:depth]
    parts = [P(1 + i % 2 * 1, 11 + i, 1800, 400, bool(i % 2), M.KEEP if i % 2 == 0 else M.LEFT, g) for i, g in enumerate(gains)]
    want = run(ctx, 1, N, parts, where=("depth", depth))
    if depth >= 3:
        other = S.splice(ctx.src, 1, N, parts[::-1])
        assert np.any(bits(other[0]) != bits(want[0]))
        run(ctx, 1, N, parts[::-1], where=("depth reversed", depth))


def test_a_loop_of_forty_parts_with_crossfades(ctx):
    n, step = 80, 64                                          # 16-frame crossfades
    parts = [P(3, 100, n, i * step, False, M.KEEP, 1.0, 16 if i else 0, 16 if i < 39 else 0, M.SMOOTH, M.SMOOTH) for i in range(40)]
    run(ctx, 1, 39 * step + n, parts, where="loop")


def test_gaps_are_zero_where_the_result_replaces_a_clip_of_ones(ctx):
    ones = [np.full(N, 1.0, dtype=np.float32)] * 2
    live = None
    for _ in range(2):                                        # the second time the result replaces the first result's extent
        ctx.clip_upload(DST, "f32", 48000, ones)
        live = ctx.pool_stats()[2] if live is None else live
        want = run(ctx, 2, N, [P(2, 0, 100, 9), P(4, 0, 300, 1000, True), P(1, 7, 3, N - 3, False, M.DUAL_MONO)], where="gaps")
        assert ctx.pool_stats()[2] == live
    covered = np.zeros(N, dtype=bool)
    for lo, n in ((9, 100), (1000, 300), (N - 3, 3)):
        covered[lo:lo + n] = True
    got = download(ctx, DST, 2, N)
    assert all(not bits(g)[~covered].any() for g in got) and all(not bits(w)[~covered].any() for w in want)


def test_inf_and_nan_sources_give_the_canonical_nan(ctx):
    x = source(3)[0]
    x[[10, 11, 12, 13]] = [np.inf, -np.inf, np.nan, np.inf]
    x.view(np.uint32)[14] = 0xFFC12345                         # a NaN with a payload and a sign
    ctx.src[50] = [x]
    ctx.clip_upload(50, "f32", 48000, [x])
    want = run(ctx, 1, N, [P(50, 0, 1000, 0), P(50, 0, 1000, 0, gain=-1.0), P(50, 0, 1000, 1200, gain=0.0), P(50, 1, 999, 1200)], where="specials")
    b = bits(want[0])
    assert b[[10, 11, 12, 13, 14]].tolist() == [0x7FC00000] * 5 and b[[1210, 1211, 1212, 1213]].tolist() == [0x7FC00000] * 4


# ---- 5: one launch for any length -----------------------------------------------------------------------------------------------------
def test_grid_stride():
    """mono, 3 parts, just above 4096 workgroups x 4 tiles: the first workgroups take a second tile"""
    n = 4096 * 2048 + 1037
    c = W.MixContext(4, block=128)
    rng = np.random.default_rng(0x6121D)
    c.src = {1: [rng.uniform(-1.1, 1.1, n).astype(np.float32)]}
    c.clip_upload(1, "f32", 48000, c.src[1])
    parts = [P(1, 0, n, 0, False, M.KEEP, 0.5, 300001, 0, M.SMOOTH), P(1, 5, 2001, 4096 * 2048 - 1500, True, M.KEEP, -1.0, 7, 9),
             P(1, 123, 1000, n - 1000, False, M.KEEP, 1.0, 0, 1000, M.LINEAR, M.SQUARE)]
    run(c, 1, n, parts, where="grid stride")
    c.close()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_pool_and_dst_alone(ctx):
    L = W.lib()
    sp = W.splice_part
    ctx.clip_splice(DST, 2, 64, [sp(2, 0, 64)])
    ctx.clip_upload(60, "i16", 48000, [np.arange(64, dtype=np.int16)] * 2)
    ctx.clip_upload(61, "f32", 44100, [np.ones(64, dtype=np.float32)] * 2)
    kept = bits(np.stack(download(ctx, DST, 2, 64))).tolist()
    st = _ffi.ClipStats()

    def refused(status, parts, channels=2, n_frames=64, dst=DST, n_parts=None):
        before = ctx.pool_stats()
        arr = (_ffi.SplicePart * len(parts))(*parts) if parts else None
        got = L.wbx_clip_splice(ctx.h, dst, channels, n_frames, arr, len(parts) if n_parts is None else n_parts, C.byref(st))
        assert got == status, (got, status, L.wbx_last_error(ctx.h))
        assert ctx.pool_stats() == before and bits(np.stack(download(ctx, DST, 2, 64))).tolist() == kept

    ok = dict(src_clip=2, first_frame=0, n_frames=64)
    refused(-4, [], n_parts=1)                                                # parts NULL
    refused(-4, [sp(**ok)], n_parts=0)                                        # no parts
    refused(-4, [sp(**ok)], n_frames=0)
    refused(-4, [sp(**ok)], n_frames=(1 << 31) - 16)
    refused(-4, [sp(**ok)], channels=0)
    refused(-4, [sp(**ok)], channels=3)
    refused(-4, [sp(999, 0, 64)])                                             # unknown source
    refused(-4, [sp(**ok), sp(DST, 0, 64)])                                   # dst is a part's source
    refused(-4, [sp(2, 0, 0)])                                                # a part with no frames
    refused(-4, [sp(2, 2990, 11)])                                            # past its clip
    refused(-4, [sp(2, 3001, 1)])
    refused(-4, [sp(2, 0, 64, at=1)])                                         # past the result
    refused(-4, [sp(2, 0, 65)])
    refused(-4, [sp(**ok, flags=2)])
    refused(-4, [sp(**ok, channel_mode=6)])
    refused(-4, [sp(**ok, channel_mode=-1)])
    refused(-4, [sp(**ok, fade_in_shape=3)])
    refused(-4, [sp(**ok, fade_out_shape=-1)])
    refused(-4, [sp(**ok, fade_in=65)])
    refused(-4, [sp(**ok, fade_out=65)])
    refused(-4, [sp(**ok, channel_mode="dual_mono")])                         # modes that do not fit the source
    for mode in ("swap", "left", "right", "mono_mix"):
        refused(-4, [sp(1, 0, 64, channel_mode=mode)], channels=1)
    refused(-4, [sp(**ok)], channels=1)                                       # modes that do not yield `channels`
    refused(-4, [sp(1, 0, 64)])
    refused(-4, [sp(**ok, channel_mode="mono_mix")])
    refused(-4, [sp(**ok), sp(61, 0, 64)])                                    # the rates differ
    refused(-3, [sp(60, 0, 64)])                                              # not F32
    refused(-3, [sp(2, 0, 1)] * 65537)                                        # too many parts
    # a tile table of more than 2^24 entries: 65536 parts that touch 257 tiles each (one frame fewer and they would pass)
    wide = 256 * 512 + 1
    ctx.clip_upload(62, "f32", 48000, [np.zeros(wide, dtype=np.float32)])
    refused(-3, [sp(62, 0, wide)] * 65536, channels=1, n_frames=1 << 18)
    assert b"2^24 entries" in L.wbx_last_error(ctx.h)
    L.wbx_clip_splice(ctx.h, DST, 2, 64, (_ffi.SplicePart * 2)(sp(**ok), sp(61, 0, 64)), 2, None)
    assert b"wbx_clip_resample" in L.wbx_last_error(ctx.h)


def test_the_engine_refuses_a_table_too_long_and_leaves_no_pin():
    """wbx_engine_splice_samples meets that refusal AFTER it has pinned its sources and left the editor lock (the table is
    sized without it): nothing is allocated or registered, and the pin is gone — the source can be deleted at once"""
    eng = W.Engine(1, buffer_size=128, sample_rate=48000, max_blocks=1)
    wide = 256 * 512 + 1
    src = eng.add_sample("f32", 48000, [np.zeros(wide, dtype=np.float32)])
    before, n_ids = eng.ctx.pool_stats(), src + 1
    with pytest.raises(W.WbxError) as ex:
        eng.splice_samples(1, 1 << 18, [W.splice_part(src, 0, wide)] * 65536)
    assert ex.value.status == -3 and "2^24 entries" in str(ex.value)
    assert eng.ctx.pool_stats() == before
    ok = eng.splice_samples(1, 1 << 18, [W.splice_part(src, 0, wide - 1)] * 2)     # the next id: the refusal registered nothing
    assert ok == n_ids
    eng.delete_sample(ok)
    eng.delete_sample(src)                                                         # no pin was left
    eng.close()


def test_the_pool_limit_refuses_and_nothing_leaks():
    c = W.MixContext(4, block=128)
    n = 1 << 20
    c.src = {1: [np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32) for _ in range(2)]}
    c.clip_upload(1, "f32", 48000, c.src[1])          # 8 MiB in the first slab (64 MiB)
    slabs, reserved, live = c.pool_stats()
    c.pool_limit(reserved)
    made = []
    while True:
        before = c.pool_stats()
        try:
            c.clip_splice(10 + len(made), 2, n, [W.splice_part(1, 0, n, reverse=True)])
        except W.WbxError as ex:
            assert ex.status == BU.OOM and c.pool_stats() == before
            break
        made.append(10 + len(made))
        assert len(made) < 64
    assert len(made) >= 2, "the slab has room for a few results"
    for i in made:
        assert c.L.wbx_clip_free(c.h, i) == 0
    assert c.pool_stats() == (slabs, reserved, live)
    c.close()


# ---- 7: through the engine ------------------------------------------------------------------------------------------------------------
def oracle_sample(e, planes, rate):
    n = len(planes[0])
    return e.add_sample("f32", len(planes), rate, n, [np.concatenate([p, np.zeros(16, np.float32)]) for p in planes])


def test_two_takes_crossfaded_play_as_the_models_clip():
    """two mono takes recorded side by side, comped into one stereo sample by splice_samples — the first take fading out
    while the second fades in — placed on a track and rendered, in one batch and block by block through process(), against
    the oracle playing the MODEL's clip"""
    spec = synth.make_session("spltake", 3, n_blocks=6, block=128, seed=0x5B17A4E)
    eng = build_engine(spec, max_blocks=8)
    eng.set_audio_channel_config(2, spec.channels, spec.block, spec.sample_rate)
    eng.set_track_input(0, "external_mono", 0, True)
    eng.set_track_input(1, "external_mono", 1, True)
    rng = np.random.default_rng(19)
    x = [rng.uniform(-0.3, 0.3, 3 * spec.block).astype(np.float32) for _ in range(2)]
    inp, out = W.AudioBuffer(spec.block, 2), W.AudioBuffer(spec.block, spec.channels)
    eng.record()
    for b in range(3):
        for k in range(2):
            inp.channel_buffers[k][:] = x[k][b * spec.block:(b + 1) * spec.block]
        eng.process(inp, out, float(spec.sample_rate))
    frames = eng.record_info(0)["frames"]
    eng.stop_record()
    eng.stop()
    eng.set_playhead_position(0.0)
    assert frames == len(x[0]) == eng.record_info(1)["frames"]
    takes = [max(c[5] for c in eng.clips(eng.tracks[t])) for t in (0, 1)]
    for t in (0, 1):
        same_bits(download(eng.ctx, takes[t], 1, frames), [x[t]], ("take", t))
    overlap, n = 100, 2 * frames - 100
    parts = [P(takes[0], 0, frames, 0, False, M.DUAL_MONO, 1.0, 0, overlap, M.LINEAR, M.SMOOTH),
             P(takes[1], 0, frames, frames - overlap, False, M.DUAL_MONO, 1.0, overlap, 0, M.SMOOTH, M.LINEAR)]
    model = S.splice({takes[0]: [x[0]], takes[1]: [x[1]]}, 2, n, parts)
    comp = eng.splice_samples(2, n, [S.to_ffi(W, p) for p in parts])
    same_bits(download(eng.ctx, comp, 2, n), model, "comp")
    # the conveniences build part lists: a mono crossfade of the two takes, and a join of three samples
    mono = eng.crossfade_samples(takes[0], takes[1], overlap, "smooth", frames=[frames, frames], channels=1)
    want = S.splice({0: [x[0]], 1: [x[1]]}, 1, n, [P(0, 0, frames, 0, fade_out=overlap, shape_out=M.SMOOTH),
                                                  P(1, 0, frames, frames - overlap, fade_in=overlap, shape_in=M.SMOOTH)])
    same_bits(download(eng.ctx, mono, 1, n), want, "crossfade_samples")
    joined = eng.join_samples([takes[1], mono, takes[0]], frames=[frames, n, frames], channels=1)
    same_bits(download(eng.ctx, joined, 1, 2 * frames + n), [np.concatenate([x[1], want[0], x[0]])], "join_samples")
    # the session both oracles play: tracks 0 and 1 empty, track 2 holding the MODEL's clip uploaded from the host
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    oracles = [O.build_oracle_engine(spec) for _ in range(2)]
    for t in (0, 1):
        while eng.clips(eng.tracks[t]):
            eng.delete_clip(eng.tracks[t], 0)
    while eng.clips(eng.tracks[2]):
        eng.delete_clip(eng.tracks[2], 0)
    eng.add_audio_clip(eng.tracks[2], "comp", 0.5 * unit, 5.5 * unit, 0.0, comp, 1.0, 1.0)
    for e in oracles:
        for t in (0, 1, 2):
            while e.clips(t):
                e.delete_clip(t, 0)
        assert e.add_audio_clip(2, 0.5 * unit, 5.5 * unit, 0.0, oracle_sample(e, model, spec.sample_rate), 1.0, 1.0) == 0
    batch, callback = oracles
    batch.play()
    eng.play()
    eng.render(6)
    m, _, _ = eng.ctx.fetch()
    heard = False
    for b in range(6):
        om, _ = batch.process()
        assert np.array_equal(bits(m[b]), bits(om)), ("batch", b)
        heard = heard or bool(om.any())
    assert heard
    eng.stop()
    eng.set_playhead_position(0.0)
    callback.play()
    eng.play()
    for b in range(6):
        om, _ = callback.process()
        eng.process(None, out, float(spec.sample_rate))
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), ("callback", b)
    # the new samples are ordinary ones: deletable once no clip names them
    with pytest.raises(W.WbxError):
        eng.delete_sample(comp)
    eng.delete_sample(mono)
    eng.delete_sample(joined)
    with pytest.raises(W.WbxError) as ex:
        eng.splice_samples(2, n, [S.to_ffi(W, parts[0]), S.to_ffi(W, parts[1]._replace(src=mono))])    # a deleted source
    assert ex.value.status == -4
    eng.close()
    for e in oracles:
        e.close()


def test_deletes_of_both_sources_beside_a_running_splice():
    """A splice shows nothing on the host while it runs, so a delete cannot be AIMED into one (tests/test_gpu_clipfx.py).
    Clips far behind the played range name both big samples for as long as the threads run: a delete of either can never
    succeed there — between two splices it is refused for the clip (-4), inside one for the pin (-3, asked first).  One
    thread deletes the two in turn without pause while another crossfades them until a refusal for the pin has been seen
    for EACH.  The splices start only once the deleter is seen spinning and go on for as long as it takes, up to SEEK
    seconds — no count of calls bounds them: to fail with no bug present a thread that does nothing but delete would have
    to miss every one of thousands of splices.  Afterwards, the clips gone, both deletes succeed."""
    NB, FR, WAIT, SEEK = 200, 1 << 21, 60.0, 20.0
    spec = synth.make_session("splthr", 2, n_blocks=NB, block=128, seed=0x5B17812)
    rng = np.random.default_rng(31)
    planes = [[rng.uniform(-1.0, 1.0, FR).astype(np.float32) for _ in range(2)] for _ in range(2)]

    def with_big(eng):                                            # the same session in both runs
        ids = [eng.add_sample("f32", 48000, p) for p in planes]
        for k, sid in enumerate(ids):
            eng.add_audio_clip(eng.tracks[0], "far", 1000.0 + 2 * k, 1001.0 + 2 * k, 0.0, sid, 1.0, 1.0)
        return ids

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
    L = W.lib()
    overlap = 4096
    began, spinning, finished = threading.Event(), threading.Event(), threading.Event()
    pinned = {s: threading.Event() for s in big}
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        k = 0
        while not finished.is_set() and time.monotonic() < end:
            s = big[k % 2]
            k += 1
            st = L.wbx_engine_delete_sample(eng.h, s)
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            spinning.set()
            if st == -3:
                pinned[s].set()

    def editor():
        try:
            began.set()
            spinning.wait(WAIT)
            end = time.monotonic() + SEEK
            while time.monotonic() < end and not all(ev.is_set() for ev in pinned.values()):
                if "id" in results:
                    eng.delete_sample(results["id"])             # (keeps the pool at one result)
                results["id"] = eng.crossfade_samples(big[0], big[1], overlap, "square")
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
    print("splice calls", results["calls"], "deletes", seen)
    assert all(ev.is_set() for ev in pinned.values()), seen
    assert all((st == -3 and b"being edited" in m) or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every splice read live sources: the last result is the model's, bit for bit
    n = 2 * FR - overlap
    want = S.splice({0: planes[0], 1: planes[1]}, 2, n, [P(0, 0, FR, 0, fade_out=overlap, shape_out=M.SQUARE),
                                                        P(1, 0, FR, FR - overlap, fade_in=overlap, shape_in=M.SQUARE)])
    same_bits(download(eng.ctx, results["id"], 2, n), want, "beside")
    # afterwards: no pin is left (the clips are what refuses now), and with the clips gone both deletes succeed
    for s in big:
        assert L.wbx_engine_delete_sample(eng.h, s) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    for _ in big:
        eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    for s in big:
        assert L.wbx_engine_delete_sample(eng.h, s) == 0
    eng.close()
