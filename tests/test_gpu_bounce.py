"""wbx_engine_bounce on the device: tracks (post- and pre-fader), buses and the master kept as clip-pool samples, held
bit for bit (uint32 views, no tolerance) to the oracle running the bounce's defining sequence
    set_playhead_position(min), play(), K blocks, stop(), set_playhead_position(the playhead before)
with wbo_engine_process_tracks, trimmed to n_frames.

Sessions bounced whole (bounce_util.drawn_sessions()): 10 random_session + 12 random_masked_session draws, c1 / c2 / c3 / c3
cut into clips / the seek session — 27.  None of the generators redirects the master, so bounce refuses none of them:
counted on the CPU by tests/test_bounce_model.py::test_no_drawn_session_is_refused (0 of 27, 0 %).
Every mix instance the library compiles (tests/instance_census.py: every family, row mode, block shape and the packed
instances) has a case of its own that asserts WHICH instance the bounce's pass launched (wbx_kernel_name):
test_every_mix_instance_bounces_exactly, 41 entries; the callback_kernel instances cannot be launched by a bounce."""
import ctypes as C
import re

import numpy as np
import pytest

import bounce_util as BU
import fuzz_util as FZ
import instance_census as IC
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

bits = BU.bits
SESSIONS = BU.drawn_sessions()


def fetch(eng, ids, n):
    return [eng.bounce_download(i, n) for i in ids]


def first_diff(a, b):
    d = np.argwhere(bits(a) != bits(b))
    return None if len(d) == 0 else (tuple(int(x) for x in d[0]), float(np.asarray(a)[tuple(d[0])]), float(np.asarray(b)[tuple(d[0])]), len(d))


# ---- 1 + 2: stems = the oracle's track_out, both taps --------------------------------------------------------------------
@pytest.mark.parametrize("name,spec,n_blocks", SESSIONS, ids=[s[0] for s in SESSIONS])
def test_stems_equal_the_oracles_track_buffers(name, spec, n_blocks):
    """every track of the session, post-fader (= track_out) and pre-fader (= track_out of the twin with every fader at
    unity), in ONE call of 2 N sources; the range starts and ends inside blocks; max_blocks 8, so longer ranges take
    several passes"""
    lo, hi = BU.bounce_range(spec, n_blocks)
    e = O.build_oracle_engine(spec)
    n, want_post, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    tw = O.build_oracle_engine(BU.unity_twin(spec))
    _, want_pre, _, _ = BU.oracle_sequence(tw, spec, lo, hi)
    eng = build_engine(spec, max_blocks=8)
    ids, frames = eng.bounce(lo, hi, BU.all_stems(spec))
    assert frames == n and len(ids) == 2 * spec.n_tracks and len(set(ids)) == len(ids)
    N = spec.n_tracks
    for t in range(N):
        got = eng.bounce_download(ids[t], n)
        assert got.shape == want_post[t].shape
        assert np.array_equal(bits(got), bits(want_post[t])), (name, "post", t, first_diff(got, want_post[t]))
        got = eng.bounce_download(ids[N + t], n)
        assert np.array_equal(bits(got), bits(want_pre[t])), (name, "pre", t, first_diff(got, want_pre[t]))
    assert eng.transport() == (e.playhead, e.sample_position, False)
    eng.close()
    e.close()
    tw.close()


CENSUS = BU.census_entries()


@pytest.mark.parametrize("entry", CENSUS, ids=[re.sub(r"[^0-9A-Za-z]+", "_", e.name.removeprefix("wbx::")).strip("_") for e in CENSUS])
def test_every_mix_instance_bounces_exactly(entry, monkeypatch):
    """The census entry's session (finite audio), its switches set before the engine is built, the entry's group size, and
    max_blocks = the entry's K: a bounce of K blocks (the last one cut) is ONE pass, and the instance that pass launched is
    the entry's.  Every track's stem, both taps, equals the oracle.  Then the same range from inside the first block with
    max_blocks 3 (several passes), and — entries that render into interleaved device formats — with such a master format set.
    The 2048-block entry (chained long render) keeps 9 of its 131 tracks: 2 GiB of stems otherwise."""
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    K = entry.n_blocks
    spec = IC.build_spec(entry, salt=False)
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    tracks = list(range(spec.n_tracks)) if K <= 16 else [0, 1, 2, 3, 4, 5, 64, 127, 130]
    srcs = [("track", t, "post") for t in tracks] + [("track", t, "pre") for t in tracks]
    runs = [(0.0, (K - 0.45) * unit, K, None)]
    if K <= 16:
        runs.append((0.37 * unit, (K - 0.45) * unit, 3, None))
        runs += [(0.0, (K - 0.45) * unit, K, fmt) for fmt in entry.master_formats[:2]]
    for lo, hi, mb, fmt in runs:
        n, post, pre = BU.oracle_stems(spec, lo, hi, None if K <= 16 else tracks)
        eng = build_engine(spec, max_blocks=mb, group_size=entry.group_size)
        if fmt:
            eng.ctx.set_master_format(fmt)
        ids, frames = eng.bounce(lo, hi, srcs)
        assert frames == n and -(-n // spec.block) == K
        if mb == K:
            assert eng.ctx.kernel_name() == BU.census_mix_name(entry), (eng.ctx.kernel_name(), mb, fmt)
        for i, t in enumerate(tracks):
            got = eng.bounce_download(ids[i], n)
            assert np.array_equal(bits(got), bits(post[i])), (entry.name, mb, fmt, "post", t, first_diff(got, post[i]))
            got = eng.bounce_download(ids[len(tracks) + i], n)
            assert np.array_equal(bits(got), bits(pre[i])), (entry.name, mb, fmt, "pre", t, first_diff(got, pre[i]))
        eng.close()


def test_a_muted_tracks_post_fader_stem_is_the_oracles_signed_zeros():
    spec = synth.make_session("muted", 6, n_blocks=4, seed=0xB0C1)
    spec.mutes[2] = True
    lo, hi = BU.bounce_range(spec, 4)
    e = O.build_oracle_engine(spec)
    n, want, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    eng = build_engine(spec, max_blocks=8)
    ids, _ = eng.bounce(lo, hi, [("track", 2, "post"), ("track", 2, "pre"), ("track", 2, "post")])
    post, pre, again = fetch(eng, ids, n)
    assert np.array_equal(bits(post), bits(want[2])) and np.array_equal(bits(again), bits(post))
    assert set(np.unique(bits(post)).tolist()) == {0x00000000, 0x80000000}       # 0.0f * x: the sign of x survives
    assert np.array_equal(bits(post) == 0x80000000, pre < 0)
    assert np.abs(pre).max() > 0
    eng.close()
    e.close()


def test_ranges_inside_a_clip_across_silence_and_shorter_than_a_block():
    """one clip per track with a gap in the middle of the session: ranges that start inside a clip, end inside a clip, span
    the silence between two clips, lie wholly in silence, and are shorter than one block"""
    spec = synth.make_session("gaps", 5, n_blocks=24, seed=0xB0C2, src_rate=44100)
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    spec.clips = []
    for t in range(5):
        spec.clips.append(synth.ClipSpec(t, 0.0, (6.3 + t) * unit, start_offset=float(3 * t)))
        spec.clips.append(synth.ClipSpec(t, (12.6 + t) * unit, 23.0 * unit, start_offset=100.0, gain=0.5))
    eng = build_engine(spec, max_blocks=8)
    e = O.build_oracle_engine(spec)
    for lo, hi in [(2.2 * unit, 5.9 * unit), (5.5 * unit, 14.1 * unit), (11.0 * unit, 12.0 * unit), (3.1 * unit, 3.6 * unit),
                   (0.0, 23.5 * unit), (13.0 * unit, 13.0 * unit + 1.5 / 24000.0)]:
        n, want, _, _ = BU.oracle_sequence(e, spec, lo, hi)
        ids, frames = eng.bounce(lo, hi, [("track", t) for t in range(5)])
        assert frames == n
        for t, got in enumerate(fetch(eng, ids, n)):
            assert np.array_equal(bits(got), bits(want[t])), (lo / unit, hi / unit, t, first_diff(got, want[t]))
        for i in ids:
            eng.delete_sample(i)
    eng.close()
    e.close()


# ---- 3: buses and the master ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bus_and_master_sources_equal_wbx_fetch_and_the_oracle(seed):
    spec = synth.make_session("buses", 45, n_blocks=10, n_buses=3, seed=0xB0C3 + seed, src_rate=44100 if seed else 48000)
    spec.track_bus = [t % 4 - 1 for t in range(45)]            # direct tracks between the bus members
    lo, hi = BU.bounce_range(spec, 10)
    e = O.build_oracle_engine(spec)
    n, _, om, ob = BU.oracle_sequence(e, spec, lo, hi)
    K = -(-n // spec.block)
    twin = build_engine(spec, max_blocks=16, group_size=spec.n_tracks)
    twin.set_playhead_position(lo)
    twin.play()
    twin.render(K)
    m, _, b = twin.ctx.fetch(buses=True)                       # [K][C][F], [K][NB][C][F]
    tm = m.transpose(1, 0, 2).reshape(spec.channels, -1)[:, :n]
    tb = b.transpose(1, 2, 0, 3).reshape(3, spec.channels, -1)[:, :, :n]
    eng = build_engine(spec, max_blocks=4, group_size=spec.n_tracks)
    srcs = [("bus", 2), ("master",), ("bus", 0), ("track", 7, "pre"), ("bus", 1), ("master",)]
    ids, frames = eng.bounce(lo, hi, srcs)
    assert frames == n
    got = fetch(eng, ids, n)
    for g, u in ((got[0], 2), (got[2], 0), (got[4], 1)):
        assert np.array_equal(bits(g), bits(tb[u])) and np.array_equal(bits(g), bits(ob[u])), u
    for g in (got[1], got[5]):
        assert np.array_equal(bits(g), bits(tm)) and np.array_equal(bits(g), bits(om))
    for x in (eng, twin, e):
        x.close()


# ---- 4: pass independence ------------------------------------------------------------------------------------------------
def test_the_samples_do_not_depend_on_where_the_passes_are_cut():
    spec, _ = FZ.random_session(3)
    k = 11
    lo, hi = BU.bounce_range(spec, k)
    srcs = BU.all_stems(spec) + [("master",)] + [("bus", u) for u in range(spec.n_buses)]
    ref = None
    for mb in (1, 3, 8, 64):
        eng = build_engine(spec, max_blocks=mb, group_size=spec.n_tracks)
        ids, n = eng.bounce(lo, hi, srcs)
        assert -(-n // spec.block) == k
        got = np.stack(fetch(eng, ids, n))
        if ref is None:
            ref = got
        assert np.array_equal(bits(got), bits(ref)), (mb, first_diff(got, ref))
        eng.close()


# ---- 5: freeze ---------------------------------------------------------------------------------------------------------
def test_freeze_round_trip():
    """bounce track t pre-fader, delete its clips, put the stem back as ONE clip over the range: the following playback's
    master equals the oracle's, given the oracle's own stem through add_sample + the same clip"""
    spec = synth.make_session("freeze", 12, src_rate=44100, seek=True, n_blocks=10, seed=0xB0C5)
    t = 4
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    lo, hi = 0.0, 10 * unit
    e = O.build_oracle_engine(spec)
    tw = O.build_oracle_engine(BU.unity_twin(spec))
    n, _, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    _, pre, _, _ = BU.oracle_sequence(tw, spec, lo, hi)
    eng = build_engine(spec, max_blocks=8, group_size=spec.n_tracks)
    (stem,), frames = eng.bounce(lo, hi, [("track", t, "pre")])
    assert np.array_equal(bits(eng.bounce_download(stem, n)), bits(pre[t]))
    data = [np.concatenate([pre[t][c], np.zeros(16, np.float32)]) for c in range(spec.channels)]
    osmp = e.add_sample("f32", spec.channels, spec.sample_rate, n, data)
    while e.clips(t):
        e.delete_clip(t, 0)
        eng.delete_clip(eng.tracks[t], 0)
    assert e.add_audio_clip(t, lo, hi, 0.0, osmp, 1.0, 1.0) == 0
    eng.add_audio_clip(eng.tracks[t], "frozen", lo, hi, 0.0, stem, 1.0, 1.0)
    with pytest.raises(W.WbxError):
        eng.delete_sample(stem)                        # a clip names it: refused as for any sample
    e.play()
    eng.play()
    eng.render(8)
    m, _, _ = eng.ctx.fetch()
    for b in range(8):
        om, _ = e.process()
        assert np.array_equal(bits(m[b]), bits(om)), b
    eng.close()
    e.close()
    tw.close()


# ---- 6: the state afterwards -------------------------------------------------------------------------------------------
def test_transport_and_the_following_playback_are_the_defining_sequences():
    """after a bounce: the transport is what the sequence leaves through the existing calls (a twin engine runs it block by
    block) and what the oracle holds; play() + 8 blocks afterwards equal the oracle continuing from the same sequence"""
    spec, k = FZ.random_session(5)
    lo, hi = BU.bounce_range(spec, k)
    g = max(1, spec.n_tracks)
    e = O.build_oracle_engine(spec)
    e.set_playhead(1.25)
    n, _, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    eng = build_engine(spec, max_blocks=3, group_size=g)
    eng.set_playhead_position(1.25)
    eng.bounce(lo, hi, [("track", 0), ("master",)])
    twin = build_engine(spec, max_blocks=1, group_size=g)
    out = W.AudioBuffer(spec.block, spec.channels)
    twin.set_playhead_position(1.25)
    twin.set_playhead_position(lo)
    twin.play()
    for _ in range(-(-n // spec.block)):
        twin.process(None, out, float(spec.sample_rate))
    twin.stop()
    twin.set_playhead_position(1.25)
    assert eng.transport() == twin.transport() == (1.25, e.sample_position, False)
    e.play()
    eng.play()
    twin.play()
    for r in (3, 3, 2):
        eng.render(r)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        for b in range(r):
            om, _ = e.process()
            twin.process(None, out, float(spec.sample_rate))
            assert np.array_equal(bits(m[b]), bits(om)), (r, b)
            assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), (r, b)
            assert np.array_equal(pk[b], e.peaks()[:, :spec.channels]), (r, b)
    assert eng.transport() == twin.transport() == (e.playhead, e.sample_position, True)
    for x in (eng, twin, e):
        x.close()


@pytest.mark.parametrize("seed", [2024, 11])
def test_a_bounce_in_the_middle_of_an_edit_script_leaves_later_blocks_unchanged(seed):
    """the random edit scripts of the parity tests; at steps 7 and 15 both sides stop, run the bounce (the oracle its
    defining sequence) over a range around the playhead, and play on — every block before and after is compared"""
    spec = FZ.edit_session_spec(seed)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=4, group_size=spec.n_tracks)
    out = W.AudioBuffer(spec.block, spec.channels)
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)

    def on_block(step, op):
        if step in (7, 15):
            e.stop()
            eng.stop()
            lo, hi = max(0.0, e.playhead - 2.3 * unit), e.playhead + 6.6 * unit
            n, want, om, _ = BU.oracle_sequence(e, spec, lo, hi)
            ids, frames = eng.bounce(lo, hi, [("track", t) for t in range(spec.n_tracks)] + [("master",)])
            assert frames == n
            got = fetch(eng, ids, n)
            for t in range(spec.n_tracks):
                assert np.array_equal(bits(got[t]), bits(want[t])), (seed, step, t, first_diff(got[t], want[t]))
            assert np.array_equal(bits(got[-1]), bits(om)), (seed, step)
            e.play()
            eng.play()
        om, _ = e.process()
        eng.process(None, out, float(spec.sample_rate))
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), (seed, step, op)
        assert eng.transport()[:2] == (e.playhead, e.sample_position)

    FZ.run_edit_script(seed, spec, e, eng, on_block, sounding_bias=False)
    eng.close()
    e.close()


def test_a_bounces_blocks_count_into_the_levels():
    spec = synth.make_session("levels", 9, n_blocks=6, seed=0xB0C6)
    lo, hi = BU.bounce_range(spec, 6)
    e = O.build_oracle_engine(spec)
    n = BU.bounce_frames(lo, hi, spec.sample_rate, spec.bpm)
    e.set_playhead(lo)
    e.play()
    want = np.zeros((9, 2), np.float32)
    for _ in range(-(-n // spec.block)):
        e.process()
        want = np.maximum(want, e.peaks())
    eng = build_engine(spec, max_blocks=4)
    eng.bounce(lo, hi, [("track", 3)])
    assert np.array_equal(eng.levels(), want)
    eng.close()
    e.close()


# ---- 7: refusals and the pool --------------------------------------------------------------------------------------------
def test_every_refusal_leaves_pool_and_transport_alone():
    spec = synth.make_session("refuse", 4, n_blocks=4, n_buses=2, seed=0xB0C7)
    eng = build_engine(spec, max_blocks=4)
    L, h = eng.L, eng.h
    eng.set_playhead_position(0.5)
    eng.render(1)                                              # (everything a first render allocates is there)
    eng.ctx.sync()
    unit = BU.block_beats(spec.block, spec.sample_rate, spec.bpm)

    def refused(status, lo, hi, srcs, n_src=None):
        before = (eng.ctx.pool_stats(), eng.transport())
        arr = (_ffi.BounceSource * max(1, len(srcs)))(*[_ffi.BounceSource(*s, 0) for s in srcs])
        ids = (C.c_uint32 * 8)(*([0xDEAD] * 8))
        fr = C.c_uint64(77)
        st = L.wbx_engine_bounce(h, lo, hi, arr, len(srcs) if n_src is None else n_src, ids, C.byref(fr))
        assert st == status, (st, status, srcs)
        assert (eng.ctx.pool_stats(), eng.transport()) == before
        assert list(ids) == [0xDEAD] * 8 and fr.value == 77

    T, B, M = BU.TRACK, BU.BUS, BU.MASTER
    refused(BU.INVALID, 0.0, 2 * unit, [(T, 0, 0)], n_src=0)
    refused(BU.INVALID, 1.0, 1.0, [(T, 0, 0)])
    refused(BU.INVALID, 2.0, 1.0, [(T, 0, 0)])
    refused(BU.INVALID, 1.0, 1.0 + 1e-9, [(T, 0, 0)])          # not one frame
    refused(BU.INVALID, 0.0, 2 * unit, [(T, 0, 0), (T, 4, 0)])
    refused(BU.INVALID, 0.0, 2 * unit, [(B, 2, 0)])
    refused(BU.INVALID, 0.0, 2 * unit, [(B, 0, 1)])            # a tap on a bus
    refused(BU.INVALID, 0.0, 2 * unit, [(M, 0, 1)])
    refused(BU.INVALID, 0.0, 2 * unit, [(3, 0, 0)])
    refused(BU.INVALID, 0.0, 2 * unit, [(T, 0, 2)])
    eng.play()
    refused(BU.UNSUPPORTED, 0.0, 2 * unit, [(T, 0, 0)])       # playing
    eng.stop()
    eng.set_track_input(0, "external_mono", 0, True)
    assert L.wbx_engine_set_input_channels(h, 1) == 0
    eng.record()
    refused(BU.UNSUPPORTED, 0.0, 2 * unit, [(T, 0, 0)])       # recording
    eng.stop()
    p = C.c_void_p()
    assert L.wbx_host_alloc(4 * spec.block * spec.channels * 4, C.byref(p)) == 0
    eng.ctx.set_master_target(p.value)
    refused(BU.UNSUPPORTED, 0.0, 2 * unit, [(T, 0, 0)])       # a redirected master
    eng.ctx.set_master_target(None)
    eng.ctx.set_master_init(p.value)
    refused(BU.UNSUPPORTED, 0.0, 2 * unit, [(T, 0, 0)])       # a running master to continue
    eng.ctx.set_master_init(None)
    assert L.wbx_host_free(p) == 0
    eng.ctx.set_master_format("i16")
    refused(BU.UNSUPPORTED, 0.0, 2 * unit, [(T, 0, 0), (M, 0, 0)])   # the master as a source while it leaves as 16-bit samples
    ids, n = eng.bounce(0.0, 2 * unit, [("track", 1), ("bus", 0)])   # ... tracks and buses are not the master: bounced
    assert n == 2 * spec.block
    eng.ctx.set_master_format(None)
    ids, n = eng.bounce(0.0, 2 * unit, [("track", 0)])         # ... and it still bounces
    assert n == 2 * spec.block
    eng.close()


def test_a_pool_that_cannot_hold_every_stem_gives_back_what_it_took():
    spec = synth.make_session("small_pool", 6, n_blocks=40, seed=0xB0C8)
    lo, hi = 0.0, 40 * BU.block_beats(spec.block, spec.sample_rate, spec.bpm)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=8, group_size=6)
    eng.render(1)
    eng.ctx.sync()
    slabs, reserved, live = eng.ctx.pool_stats()
    # each stem is 40 * 512 * 4 B * 2 channels = 160 KiB, 192 KiB of pool with its granule rounding: room for a few, not six
    eng.ctx.pool_limit(reserved)
    fit = 0
    ids = []
    while True:
        try:
            i, n = eng.bounce(lo, hi, [("track", 0)])
        except W.WbxError as ex:
            assert ex.status == BU.OOM
            break
        ids += i
        fit += 1
        assert fit < 1000
    assert fit >= 2, "the slab has room for a few stems"
    for i in ids[1:]:
        eng.delete_sample(i)
    before, tr = eng.ctx.pool_stats(), eng.transport()
    with pytest.raises(W.WbxError) as ei:
        eng.bounce(lo, hi, [("track", t) for t in range(6)] * 80)      # 480 stems, 90 MiB: more than the 64-MiB slab holds
    assert ei.value.status == BU.OOM
    assert eng.ctx.pool_stats() == before and eng.transport() == tr
    n, want, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    assert np.array_equal(bits(eng.bounce_download(ids[0], n)), bits(want[0]))
    eng.ctx.pool_limit(0)
    got, _ = eng.bounce(lo, hi, [("track", 5)])
    assert np.array_equal(bits(eng.bounce_download(got[0], n)), bits(want[5]))
    e.play()
    eng.play()
    eng.render(8)
    m, _, _ = eng.ctx.fetch()
    for b in range(8):
        om, _ = e.process()
        assert np.array_equal(bits(m[b]), bits(om)), b
    eng.close()
    e.close()


# ---- 8: an ordinary sample ------------------------------------------------------------------------------------------------
def test_a_bounced_sample_is_an_ordinary_sample():
    spec = synth.make_session("ordinary", 3, n_blocks=20, seed=0xB0C9)
    lo, hi = BU.bounce_range(spec, 20)
    eng = build_engine(spec, max_blocks=8)
    (sid,), n = eng.bounce(lo, hi, [("master",)])
    audio = eng.bounce_download(sid, n)
    eng.ctx.build_mipmaps(sid, 1)
    levels = eng.L.wbx_mip_levels(n)
    assert levels >= 1
    for lv in range(levels):
        mip = eng.ctx.fetch_mipmap(sid, lv, spec.channels, n, 1)
        for c in range(spec.channels):
            assert np.array_equal(mip[c], O.oracle_mip("f32", audio[c], lv, 1)), (lv, c)
    eng.add_audio_clip(eng.tracks[0], "bounced", 40.0, 41.0, 0.0, sid)
    with pytest.raises(W.WbxError):
        eng.delete_sample(sid)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    live = eng.ctx.pool_stats()[2]
    eng.delete_sample(sid)
    assert eng.ctx.pool_stats()[2] < live
    with pytest.raises(W.WbxError):
        eng.delete_sample(sid)
    eng.close()
