"""GPU parity tests: the HIP path (libwbx.so through the C ABI) against the committed golden vectors
and against the CPU oracle on the same seeded inputs.  Run on a real MI355X:  pytest -m gpu

Bars (BASELINE.json north_star): output within 1e-6 RMS per sample of the CPU reference (fp32); seek /
sample-index math bit-exact.  What is actually asserted is tighter wherever the design allows it:
  * every per-track value is computed with the reference's roundings, so per-track peaks are EQUAL;
  * the master is BIT-EXACT whenever the summation order equals the reference's (group_size >= N, or
    the bus layout of config 4), and within 1e-6 RMS otherwise (grouped order);
  * the device sequencer's plan (buffer offsets, lengths, sample offsets as bit patterns) is EQUAL
    to the oracle's Sampler::stream call log.
"""
import dataclasses
import os
import re

import numpy as np
import pytest

import fuzz_util as FZ
import golden_util as G
import grouped_order as GO
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-6     # north_star: "within 1e-6 RMS per sample (fp32)"


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def instance_id(name):
    """a kernel instance's C++ name as a test id: "wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>" -> "mix_kernel_2_true_4_0_1_1_1_256"
    (the name itself holds "::", the separator of pytest's node ids)"""
    return re.sub(r"[^0-9A-Za-z]+", "_", name.removeprefix("wbx::")).strip("_")


def plan_rows(plan):
    """(block, track, buffer_offset, num_samples, offset_bits, speed_bits, gain_bits, sample)"""
    return [(b, t, bo, ns, O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (b, t, bo, ns, na, smp, off, spd, g, fl) in plan]


def oracle_rows(e, block):
    return [(block, t, ds, min(ln, 0xFFFF), O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (t, ds, ln, off, spd, g, smp) in e.seglog()]


def run_oracle(spec, n_blocks, want_buses=False):
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    e.play()
    masters, peaks, buses, rows = [], [], [], []
    for b in range(n_blocks):
        m, bu = e.process(want_buses=want_buses)
        masters.append(m)
        peaks.append(e.peaks())
        rows += oracle_rows(e, b)
        if bu is not None:
            buses.append(bu)
    tr = (e.playhead, e.sample_position)
    e.close()
    return np.stack(masters), np.stack(peaks), (np.stack(buses) if buses else None), rows, tr


# ---------------------------------------------------------------------------------------------------
# golden vectors (outputs of the reference's own translation units)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.session_names())
def test_golden_sessions_block_by_block(name):
    """Engine::process one block at a time.  All fixtures have <= 64 tracks per group, so the summation
    order IS the reference's: master, bus sums and peaks must match the golden bits."""
    spec, n_blocks, g = G.load_session(name)
    eng = build_engine(spec, max_blocks=1)
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    for b in range(n_blocks):
        eng.process(None, out, float(spec.sample_rate))
        m = np.stack(out.channel_buffers)
        assert np.array_equal(bits(m), bits(g["master"][b])), (name, b, rms(m, g["master"][b]))
        _, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
        assert np.array_equal(pk[0], g["peaks"][b]), (name, b)
        if spec.n_buses:
            assert np.array_equal(bits(bus[0]), bits(g["buses"][b]))
        rows = [r[1:] for r in plan_rows(eng.fetch_plan())]
        gold = [(t, ds, min(ln, 0xFFFF), ob, sb, gb, smp) for (t, ds, ln, ob, sb, gb, smp, _e) in G.golden_segments(g, b)]
        assert rows == gold, (name, b)
    eng.close()


@pytest.mark.parametrize("name", ["c2", "c3", "c4", "seek", "seek441", "i24_441"])
def test_golden_sessions_batched(name):
    """The same sessions rendered as ONE K-block device pass (sequencer on the device for all K blocks)."""
    spec, n_blocks, g = G.load_session(name)
    eng = build_engine(spec, max_blocks=n_blocks)
    eng.play()
    eng.render(n_blocks)
    m, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
    assert np.array_equal(bits(m), bits(g["master"]))
    assert np.array_equal(pk, g["peaks"])
    if spec.n_buses:
        assert np.array_equal(bits(bus), bits(g["buses"]))
    eng.close()


# ---------------------------------------------------------------------------------------------------
# oracle on the same seeded inputs — BASELINE.json configs
# ---------------------------------------------------------------------------------------------------
def check_against_oracle(spec, n_blocks, group_size=0, expect_exact=False, device_synth=False):
    om, opk, obus, orows, otr = run_oracle(spec, n_blocks, want_buses=bool(spec.n_buses))
    eng = build_engine(spec, max_blocks=n_blocks, group_size=group_size, device_synth=device_synth)
    eng.play()
    eng.render(n_blocks)
    m, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
    # seek / sample-index math: bit-exact
    assert plan_rows(eng.fetch_plan()) == orows
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(otr[0]), O.f64_bits(otr[1]))
    # per-track values carry the reference's roundings -> peaks equal
    assert np.array_equal(pk, opk[..., :spec.channels])
    r = rms(m, om)
    if expect_exact:
        assert np.array_equal(bits(m), bits(om)), r
        if bus is not None:
            assert np.array_equal(bits(bus), bits(obus))
    else:
        assert r <= RMS_TOL, r
    check_grouped_order(eng, spec, n_blocks, group_size, m, bus)
    eng.close()
    return r


def check_grouped_order(eng, spec, n_blocks, group_size, m, bus):
    """the render's master and bus sums, bit for bit, against tests/grouped_order.py's model of the order the render took
    (wbx_render_order: the reference's, or groups of G) over the oracle's track buffers"""
    order = eng.ctx.render_order(n_blocks)
    groups = GO.render_partition(spec, order, group_size, n_blocks)
    _, _, tracks = GO.oracle_tracks(spec, n_blocks)
    em, ebus = GO.grouped_sum(tracks, groups, spec.n_buses)
    GO.assert_model(m, em, bus, ebus if spec.n_buses else None, what=(spec.name, order))


def test_config1_8_mono_unity():
    spec = synth.make_session("c1", 8, clip_channels=1, n_blocks=8, unity_gain=True, seed=0x5EED0001)
    check_against_oracle(spec, 8, expect_exact=True)


def test_config2_256_stereo_gain_pan():
    spec = synth.make_session("c2", 256, n_blocks=8, seed=0x5EED0002)
    r = check_against_oracle(spec, 8)
    assert r <= RMS_TOL


def test_config2_exact_order_mode():
    """group_size >= N reproduces the reference's strictly sequential sum: bit-exact master."""
    spec = synth.make_session("c2", 256, n_blocks=4, seed=0x5EED0002)
    check_against_oracle(spec, 4, group_size=256, expect_exact=True)


def test_config3_4096_resample():
    """BASELINE config 3 at full size: 4096 stereo tracks, gain+pan, linear 44.1k -> 48k."""
    spec = synth.make_session("c3", 4096, src_rate=44100, n_blocks=4, seed=0x5EED0003)
    r = check_against_oracle(spec, 4)
    print("config3 rms vs oracle:", r)


def test_config3_exact_order_mode():
    spec = synth.make_session("c3", 1024, src_rate=44100, n_blocks=2, seed=0x5EED0003)
    check_against_oracle(spec, 2, group_size=1024, expect_exact=True)


@pytest.mark.parametrize("chain", ["1", "0"])
def test_config3_4096_whole_list_walk_is_bit_exact(monkeypatch, chain):
    """BASELINE config 3 at full width in the reference's own summation order, both ways the library has it: chained
    128-track pieces (each workgroup continues the running sum of the piece before it: what renders of >= 1024 blocks
    take) and, WBX_CHAIN=0, one workgroup walking all 4096 tracks of its block (32 staged chunks).  WBX_EXACT_MIN_BLOCKS
    lowers the threshold so that the oracle only has to render 4 blocks.  Master, peaks, stream-call log and transport bit
    for bit."""
    monkeypatch.setenv("WBX_EXACT_MIN_BLOCKS", "4")
    monkeypatch.setenv("WBX_CHAIN", chain)
    spec = synth.make_session("c3", 4096, src_rate=44100, n_blocks=4, seed=0x5EED0003)
    check_against_oracle(spec, 4, expect_exact=True)
    spec = synth.make_session("c3s", 4096, src_rate=44100, seek=True, n_blocks=5, seed=0x5EED0013)   # clip boundaries in the walk
    check_against_oracle(spec, 5, expect_exact=True)


def test_render_of_1024_blocks_takes_the_reference_order(monkeypatch):
    """The default for a long render, at BASELINE config 3's full size and a benchmark-sized render: wbx_render_order
    reports the reference's order (32 chained pieces of 128 tracks; WBX_CHAIN=0: one walk of 4096 tracks per workgroup),
    the head of the render — the first 4 blocks — is bit-identical to the oracle (the bench's own --verify does the same
    after its timed loop), and the two ways of adding in that order agree on every one of the 1024 blocks."""
    K, N = 1024, 4096
    long_spec = synth.make_session("c3", N, src_rate=44100, n_blocks=K, seed=0x5EED0003)
    om, opk, _, _, _ = run_oracle(synth.make_session("c3", N, src_rate=44100, n_blocks=4, seed=0x5EED0003), 4)
    got = {}
    for chain in ("1", "0"):
        monkeypatch.setenv("WBX_CHAIN", chain)
        eng = build_engine(long_spec, max_blocks=K, device_synth=True)
        eng.play()
        eng.render(K)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        assert eng.ctx.render_order(K) == ((32, 128, True) if chain == "1" else (1, N, True)) and eng.ctx.render_order(256)[2] is False
        assert eng.ctx.kernel_name() == ("wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>" if chain == "1"
                                         else "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 128>")
        assert np.array_equal(bits(m[:4]), bits(om)) and np.array_equal(pk[:4], opk[..., :2])
        assert np.abs(m[4:]).max() > 0.05 and np.isfinite(m).all()
        got[chain] = (m, pk)
        eng.close()
    assert np.array_equal(bits(got["1"][0]), bits(got["0"][0])) and np.array_equal(got["1"][1], got["0"][1])


# ---------------------------------------------------------------------------------------------------
# the 1e-6 RMS gate where it is tight: sessions at mix-bus level (tools/level_probe.py, profiles/r03_level_probe.txt)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,mult", [("c3", dict(src_rate=44100), 1.0), ("c3", dict(src_rate=44100), 2.0),
                                          ("c4", dict(n_buses=64), 1.0), ("c4", dict(n_buses=64), 2.0)])
def test_grouped_order_at_mix_bus_levels(name, kw, mult):
    """Short renders add 128-track groups in order and then the group sums.  The association error scales with the level
    of the running sum: the synthetic default amp = 0.25/sqrt(N) (master peak 0.4) is a friendly level.  Here the master
    runs around full scale (amp = 1/sqrt(N): rms 0.44, 3 % of the samples on the clamp) and far beyond (2/sqrt(N): a
    quarter of them clamped) — N = 4096 stays inside north_star's 1e-6 RMS either way (measured 4.9e-7 / 7.0e-7); config
    4's bus layout (64-track buses = one group each) is the reference's order and stays bit-exact."""
    N, K = 4096, 4
    spec = synth.make_session(name, N, n_blocks=K, seed=0x5EED0003, amp=float(np.float32(mult / np.sqrt(N))), **kw)
    om, opk, _, _, _ = run_oracle(spec, K)
    eng = build_engine(spec, max_blocks=K)
    eng.play()
    eng.render(K)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    groups = GO.render_partition(spec, eng.ctx.render_order(K), 0, K)
    eng.close()
    assert np.array_equal(pk, opk[..., :2])
    d = m.astype(np.float64) - om.astype(np.float64)
    r, mx = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"{name} amp={mult}/sqrt(N): master rms {np.sqrt(np.mean(om.astype(np.float64) ** 2)):.3f}, "
          f"clamped {np.mean(np.abs(om) >= 1.0):.3f}, rms vs oracle {r:.3e}, max abs {mx:.3e}")
    if name == "c4":
        assert np.array_equal(bits(m), bits(om))
    else:
        assert r <= RMS_TOL, r
    _, _, tracks = GO.oracle_tracks(spec, K)      # ... and exactly the order the render took (c3: 32 groups of 128 tracks)
    assert len(groups) == (32 if name == "c3" else 64)
    em, _ = GO.grouped_sum(tracks, groups, spec.n_buses)
    GO.assert_model(m, em, what=(name, mult))


@pytest.mark.parametrize("mult", [0.25, 1.0])
def test_config5_chain_of_8_engines_is_bit_exact(mult):
    """BASELINE config 5 in the reference's order ACROSS the shards: engine g continues the running, un-clamped master of
    engine g-1 (wbx_set_master_init — what WBX_DIST_CHAIN does between GPUs with ncclSend / ncclRecv), every shard walks
    its 4096 tracks in one workgroup per block, the last engine clamps.  Bit-identical to the single-engine oracle over
    all 32768 tracks — also at mix-bus level (amp = 1/sqrt(N)), where adding shard SUMS leaves the 1e-6 RMS budget
    (1.5e-6: profiles/r03_level_probe.txt)."""
    from test_dist_gloo import _shard_spec
    from whitebox_amd.dist import PinnedBuffer, shard_tracks
    n_tracks, world, K = 32768, 8, 2
    spec = synth.make_session("c5", n_tracks, n_blocks=K, seed=0x5EED0006, amp=float(np.float32(mult / np.sqrt(n_tracks))))
    om, opk, _, _, _ = run_oracle(spec, K)
    running = PinnedBuffer(K * 2 * 512)
    shard_sums = np.zeros_like(om)
    for rank in range(world):
        first, count = shard_tracks(n_tracks, world, rank)
        eng = build_engine(_shard_spec(spec, first, count), max_blocks=K, group_size=count)
        eng.ctx.set_clamp(rank == world - 1)                   # engine.cpp:1627-1636 follows the LAST addition
        eng.ctx.set_master_target(running.ptr)
        eng.ctx.set_master_init(running.ptr if rank else None)
        eng.play()
        eng.render(K)
        _, pk, _ = eng.ctx.fetch(peaks=True)
        assert np.array_equal(pk, opk[:, first:first + count, :2])
        eng.close()
    got = running.array.reshape(K, 2, 512).copy()
    running.close()
    assert np.array_equal(bits(got), bits(om)), rms(got, om)


def test_master_init_continues_a_running_sum():
    """wbx_set_master_init on a small session split 23 + 17 + 9 tracks over three engines, clip boundaries inside the
    blocks, block by block (Engine::process) and as one render; sub-buses refuse."""
    from test_dist_gloo import _shard_spec
    from whitebox_amd.dist import PinnedBuffer
    K = 5
    spec = synth.make_session("split", 49, seek=True, src_rate=44100, n_blocks=K, seed=0x51C, amp=0.3)
    om, _, _, _, _ = run_oracle(spec, K)
    running = PinnedBuffer(K * 2 * 512)
    first = 0
    for i, count in enumerate((23, 17, 9)):
        eng = build_engine(_shard_spec(spec, first, count), max_blocks=K, group_size=count)
        eng.ctx.set_clamp(i == 2)
        eng.ctx.set_master_target(running.ptr)
        eng.ctx.set_master_init(running.ptr if i else None)
        eng.play()
        eng.render(K)
        eng.ctx.sync()
        eng.close()
        first += count
    assert np.array_equal(bits(running.array.reshape(K, 2, 512)), bits(om))
    assert (np.abs(om) == 1.0).any()                          # the session really clamps, and only after the last shard
    eng = build_engine(synth.make_session("b", 8, n_buses=2, n_blocks=1), max_blocks=1)
    eng.ctx.set_master_init(running.ptr)
    eng.play()
    with pytest.raises(W.WbxError):
        eng.render(1)
    eng.close()
    running.close()


def test_levels_of_tracks_added_since_the_last_render_read_zero():
    """wbx_engine_levels for more tracks than have been through a render (a track was just added, the audio callback is
    not running): zeros for those, no error — the UI's per-frame meter read must not fail."""
    spec = synth.make_session("lv", 6, n_blocks=5, seed=0x1E7)
    eng = build_engine(spec, max_blocks=2, spare_tracks=2)
    assert not eng.levels().any()                              # nothing rendered yet
    eng.play()
    eng.render(2)
    eng.add_track("late")
    eng.add_track("later")
    lv = eng.levels()
    assert lv.shape == (8, 2) and (lv[:6] > 0).all() and not lv[6:].any()
    assert not eng.levels().any()                              # read and reset (VUMeter::update, vu_meter.h:33)
    eng.render(2)                                              # the new tracks get their (cleared) device state: no stall, no error
    assert (eng.levels()[:6] > 0).all()
    eng.close()


def test_clip_storage_reuses_the_extent_of_a_replaced_clip():
    """Replacing a clip again and again beside a long-lived one stays inside the slab (first fit over the released
    extents): the pool does not grow."""
    ctx = W.MixContext(8, max_blocks=1)
    rng = np.random.default_rng(11)
    keep = [rng.standard_normal(1_000_000).astype(np.float32)]
    ctx.clip_upload(0, "f32", 48000, keep)

    def stats():
        import ctypes as CT
        n, res, live = CT.c_uint32(), CT.c_uint64(), CT.c_uint64()
        assert ctx.L.wbx_clip_pool_stats(ctx.h, CT.byref(n), CT.byref(res), CT.byref(live)) == 0
        return n.value, res.value, live.value
    for i in range(40):                                        # 40 x 16 MB through a 64-MiB slab
        data = [rng.standard_normal(4_000_000 - 1000 * i).astype(np.float32)]
        ctx.clip_upload(1, "f32", 48000, data)
        assert np.array_equal(ctx.clip_download(1, 0, len(data[0]), np.float32), data[0])
    n, res, live = stats()
    assert n == 1 and res == 64 << 20 and live < 24 << 20
    assert np.array_equal(ctx.clip_download(0, 0, len(keep[0]), np.float32), keep[0])
    ctx.close()


def test_config4_4096_into_64_buses():
    """BASELINE config 4 at full size: bus = track/64, group_size 64 -> every bus is summed in the
    oracle's order and the master in bus order: bit-exact, bus sums included."""
    spec = synth.make_session("c4", 4096, n_buses=64, n_blocks=4, seed=0x5EED0004)
    check_against_oracle(spec, 4, expect_exact=True)


def test_seek_variants_full_width():
    for rate in (48000, 44100):
        spec = synth.make_session("seek", 512, seek=True, src_rate=rate, n_blocks=8, seed=0x5EED0005)
        check_against_oracle(spec, 8)


def test_device_synth_equals_host_upload():
    spec = synth.make_session("c2", 128, n_blocks=3, seed=0x5EED0002)
    check_against_oracle(spec, 3, device_synth=True)
    spec = synth.make_session("i16", 16, fmt="i16", n_blocks=3, seed=0x5EED0008)
    check_against_oracle(spec, 3, device_synth=True, expect_exact=True)


# ---------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------
def test_empty_and_ragged():
    """Tracks without clips, a muted track, N not a multiple of the group size, clips that end
    (tail + finished sampler), silence after the last clip."""
    spec = synth.make_session("ragged", 70, n_blocks=3, seed=0x77)
    spec.clips = [c for c in spec.clips if c.track % 5 != 0]          # every 5th track is empty
    for c in spec.clips:                                               # short clips: end inside block 2
        c.max_beat = (2 * 512 + 100 + c.track) / 24000.0
    spec.mutes[3] = True
    for s in spec.samples:
        s.frames = 900 + 7 * s.seed_track                              # sample shorter than the clip: tail path
    check_against_oracle(spec, 6, group_size=16)


def test_not_playing_is_silent_and_transport_frozen():
    spec = synth.make_session("idle", 8, n_blocks=2)
    eng = build_engine(spec, max_blocks=2)
    eng.render(2)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    assert not m.any() and not pk.any()
    assert eng.transport() == (0.0, 0.0, False)
    eng.close()


def test_stop_then_play_again_matches_oracle():
    spec = synth.make_session("replay", 12, n_blocks=6, seed=0x99)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=1)
    out = W.AudioBuffer(spec.block, spec.channels)
    for phase in range(2):
        e.play()
        eng.play()
        for _ in range(3):
            om, _ = e.process()
            eng.process(None, out, 48000.0)
            assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om))
        e.stop()
        eng.stop()
    e.close()
    eng.close()


def test_parameter_changes_are_block_rate():
    spec = synth.make_session("params", 6, n_blocks=6, seed=0x31)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=1)
    e.play()
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    for b in range(5):
        if b == 2:
            e.set_volume(1, -20.0); eng.tracks[1].set_volume(-20.0)
            e.set_pan(2, -0.75); eng.tracks[2].set_pan(-0.75)
        if b == 3:
            e.set_mute(0, True); eng.tracks[0].set_mute(True)
            e.set_volume(4, -80.0); eng.tracks[4].set_volume(-80.0)     # <= -72 dB -> exactly 0
        om, _ = e.process()
        eng.process(None, out, 48000.0)
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), b
    e.close()
    eng.close()


@pytest.mark.parametrize("block,channels", [(128, 2), (256, 2), (1024, 2), (2048, 2), (512, 1), (96, 2), (256, 1), (64, 2), (4096, 2),
                                            (32768, 2), (4, 2)])
def test_other_block_sizes_and_mono_out(block, channels):
    spec = synth.make_session("blk", 40, n_blocks=3, block=block, seed=0x42, src_rate=44100)
    spec.channels = channels
    check_against_oracle(spec, 3, group_size=8)


@pytest.mark.parametrize("block,channels,n_blocks", [(256, 2, 7), (256, 2, 8), (512, 1, 5), (256, 1, 6), (256, 1, 9),
                                                     (128, 2, 5), (128, 2, 8), (128, 2, 11)])
@pytest.mark.parametrize("kind", ["resampled", "buses_i16", "downsampled"])
def test_short_blocks_several_per_workgroup(block, channels, n_blocks, kind):
    """256-frame blocks (and mono 512 / 256): the mix kernel renders 2 or 4 consecutive blocks per workgroup;
    128-frame stereo blocks: one block per wave with a channel in each half-wave.  Block counts that are not
    a multiple leave the last workgroup with empty sub-blocks.  Clip boundaries inside blocks, bus
    routing, 16-bit clips and per-frame-tap rows go through the same instances."""
    if kind == "resampled":
        spec = synth.make_session("sb", 300, seek=True, n_blocks=n_blocks, block=block, seed=0x5B0, src_rate=44100)
    elif kind == "buses_i16":
        spec = synth.make_session("sb", 192, seek=True, n_blocks=n_blocks, block=block, seed=0x5B1, n_buses=6, fmt="i16")
        for i, smp in enumerate(spec.samples):
            if i % 3 == 0:
                smp.rate = 44100
        for t in range(spec.n_tracks):
            spec.volumes_db[t] = -40.0
    else:
        spec = synth.make_session("sb", 150, seek=True, n_blocks=n_blocks, block=block, seed=0x5B2, src_rate=96000)
    spec.channels = channels
    check_against_oracle(spec, n_blocks)
    check_against_oracle(spec, n_blocks, group_size=512, expect_exact=(kind != "buses_i16"))


def test_speed_variants_and_formats():
    """Time-stretched clips (speed != 1 at equal rates), speed > 1, near-unity speed, all PCM formats."""
    spec = synth.make_session("speeds", 24, n_blocks=4, seed=0x55)
    speeds = [0.5, 1.75, 0.999999, 1.0000001, 0.25, 2.5]
    fmts = ["f32", "i16", "i24", "i32"]
    for i, c in enumerate(spec.clips):
        c.speed = speeds[i % len(speeds)]
    for i, s in enumerate(spec.samples):
        s.fmt = fmts[(i // 6) % 4]
        s.amp = 0.05 if s.fmt == "f32" else 1.0
        s.frames = 6000
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -30.0
    check_against_oracle(spec, 4, expect_exact=True)


@pytest.mark.parametrize("src_rate,sample_rate", [(48000, 44100), (96000, 48000), (88200, 48000), (192000, 44100)])
def test_downsampled_clips_hot_loop(src_rate, sample_rate):
    """Clips recorded at a higher rate than the session (playback speed > 1): whole-block rows are streamed
    by the mix kernel with per-frame taps; clip boundaries inside blocks stay on the pre-render pass."""
    spec = synth.make_session("down", 200, seek=True, n_blocks=6, seed=0xD0 + src_rate // 1000, src_rate=src_rate,
                              sample_rate=sample_rate)
    check_against_oracle(spec, 6)                                     # grouped order
    check_against_oracle(spec, 6, group_size=200, expect_exact=True)  # reference order: bit-exact
    # among unity, up-sampled and 16-bit tracks in the same group
    spec = synth.make_session("downmix", 96, n_blocks=5, seed=0xD7, src_rate=src_rate, sample_rate=sample_rate)
    for i, smp in enumerate(spec.samples):
        if i % 4 == 1:
            smp.rate = sample_rate
        elif i % 4 == 2:
            smp.rate = sample_rate * 3 // 4
        elif i % 8 == 3:
            smp.fmt, smp.rate, smp.amp = "i16", sample_rate, 1.0
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -36.0
    check_against_oracle(spec, 5, group_size=96, expect_exact=True)
    check_against_oracle(spec, 5, group_size=12, expect_exact=False)


@pytest.mark.parametrize("fmt", ["i16", "i24", "i32"])
@pytest.mark.parametrize("src_rate", [44100, 96000])
def test_resampled_integer_pcm_hot_loop(fmt, src_rate):
    """Integer PCM clips at a rate other than the session's (the usual 16-bit 44.1 kHz file in a 48 kHz
    session): whole-block rows are read by the mix kernel with per-frame taps and the linear path's
    normalisers (sampler.cpp:9-14,34-59); also next to unity rows of the same format."""
    spec = synth.make_session("pcmr_" + fmt, 192, fmt=fmt, seek=True, n_blocks=5, seed=0xA26, src_rate=src_rate)
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -40.0 + (t % 5)
    for i, smp in enumerate(spec.samples):
        if i % 3 == 2:
            smp.rate = 48000
    check_against_oracle(spec, 5)
    check_against_oracle(spec, 5, group_size=192, expect_exact=True)
    # time-stretched on top (speeds below 0.75 take the general tap selection of the windowed 16-bit read,
    # speeds above 0.999 the per-frame taps)
    stretch = [0.5, 0.31, 0.76, 0.999, 1.0, 0.9990001, 0.05, 1.3]
    for c in spec.clips:   # groups of 8 in the first half of the tracks hold no per-frame-tap row
        k = stretch[c.track % 8]
        c.speed = 0.6 if (k > 0.999 and c.track < 96) else k
    for smp in spec.samples:
        smp.frames = int(smp.frames * 1.5) + 64
    check_against_oracle(spec, 5, group_size=8, expect_exact=False)
    check_against_oracle(spec, 5, group_size=192, expect_exact=True)


@pytest.mark.parametrize("block,channels", [(256, 2), (128, 2), (256, 1), (512, 1)])
def test_callback_mode_short_blocks(block, channels):
    """Engine::process one block per call (the audio callback) at the block sizes that pack several blocks into
    a workgroup in batch mode: here every workgroup has one valid sub-block and empty ones beside it."""
    n_blocks = 7
    spec = synth.make_session("cb", 150, seek=True, n_blocks=n_blocks, block=block, seed=0xCB0 + block, src_rate=44100)
    spec.channels = channels
    om, opk, _, orows, otr = run_oracle(spec, n_blocks)
    eng = build_engine(spec, max_blocks=1, group_size=150)
    eng.play()
    out = W.AudioBuffer(block, channels)
    for b in range(n_blocks):
        eng.process(None, out, float(spec.sample_rate))
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om[b])), b
        _, pk, _ = eng.ctx.fetch(peaks=True)
        assert np.array_equal(pk[0], opk[b][..., :channels]), b
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(otr[0]), O.f64_bits(otr[1]))
    eng.close()


@pytest.mark.parametrize("clip_blocks,block", [(1.3, 512), (0.7, 512), (2.45, 256), (0.4, 128), (3.1, 96)])
def test_sessions_cut_into_many_clips(clip_blocks, block):
    """Every track is a chain of back-to-back clips a fraction of a block to a few blocks long, staggered per
    track, alternating samples (rates 48 k / 44.1 k / 96 k), stretch factors, gains and fractional start
    offsets: most track-blocks hold one or two clip boundaries and go through the pre-render pass (two-segment
    fast path, three and more segments, unity reads at fractional positions)."""
    n_tracks, n_blocks = 96, 9
    beat_frames = 48000 * 60.0 / 120.0
    total = (n_blocks + 1) * block
    samples, clips, vols, pans = [], [], [], []
    rates = [48000, 44100, 96000]
    for t in range(n_tracks):
        for r in range(3):
            samples.append(synth.SampleSpec(seed_track=3 * t + r, channels=1 + (t + r) % 2, rate=rates[(t + r) % 3],
                                            frames=int(total * 2.2) + 400, fmt="f32", amp=0.02))
        v, p = synth.track_params(0xC11, t)
        vols.append(float(v))
        pans.append(float(p))
        L = clip_blocks * block
        pos = -((t * 37) % 101) / 101.0 * L
        k = 0
        while pos < total:
            a, b = max(pos, 0.0), pos + L
            stretch = [1.0, 1.0, 0.5, 1.25][(t + k) % 4]
            clips.append(synth.ClipSpec(t, a / beat_frames, b / beat_frames, start_offset=a * 0.8 + 0.37 * (k % 3),
                                        speed=stretch, gain=[1.0, 0.5, 1.7][k % 3], sample=3 * t + k % 3))
            pos = b
            k += 1
    spec = synth.SessionSpec(name="cut", n_tracks=n_tracks, seed=0xC11, samples=samples, clips=clips, volumes_db=vols,
                             pans=pans, mutes=[False] * n_tracks, block=block)
    check_against_oracle(spec, n_blocks, group_size=n_tracks, expect_exact=True)
    check_against_oracle(spec, n_blocks, group_size=16)


class _SpecialValuesSpec(synth.SessionSpec):
    """fp32 clips salted with denormals, signed zeros, huge values, infinities and NaNs."""
    SALTS = {"denormals_and_zeros": [1e-40, -1e-45, -0.0, 0.0, 1.17549435e-38, -1e-39],
             "huge": [3e38, -3e38, 1e-40, -0.0, 2.5e37],
             "nonfinite": [np.inf, -np.inf, np.nan, 3e38, -0.0, 1e-40]}

    def sample_data(self, i):
        out = super().sample_data(i)
        if self.samples[i].fmt != "f32":
            return out
        specials = np.array(self.SALTS[self.salt], np.float32)
        for c, a in enumerate(out):
            n = len(a) - 16
            idx = (np.arange(0, n, 37) + 5 * i + c) % max(n, 1)
            a[idx] = specials[(np.arange(len(idx)) + i) % len(specials)]
        return out


def _boundary_session(n_tracks, n_blocks, block, clip_blocks, channels=2, gaps=True, salt=None):
    """fp32 tracks at 48 and 44.1 kHz cut into clips (touching, or with gaps so that single starts / ends occur), stretch
    speeds on the window path: every clip boundary lies inside a block."""
    beat_frames = 48000 * 60.0 / 120.0
    total = (n_blocks + 1) * block
    samples, clips, vols, pans = [], [], [], []
    for t in range(n_tracks):
        for r in range(2):
            samples.append(synth.SampleSpec(seed_track=2 * t + r, channels=1 + (t + r) % 2, rate=[48000, 44100][(t + r) % 2],
                                            frames=int(total * 1.3) + 400, fmt="f32", amp=0.02))
        v, p = synth.track_params(0xB0D, t)
        vols.append(float(v))
        pans.append(float(p))
        L = clip_blocks * block
        pos = -((t * 37) % 101) / 101.0 * L
        k = 0
        while pos < total:
            a, b = max(pos, 0.0), pos + L * (0.6 if (gaps and (t + k) % 3 == 0) else 1.0)
            stretch = [1.0, 1.0, 0.5, 0.8][(t + k) % 4]
            if b > a:
                clips.append(synth.ClipSpec(t, a / beat_frames, b / beat_frames, start_offset=a * 0.8 + 0.37 * (k % 3),
                                            speed=stretch, gain=[1.0, 0.5, 1.7][k % 3], sample=2 * t + k % 2))
            pos += L
            k += 1
    cls = _SpecialValuesSpec if salt else synth.SessionSpec
    spec = cls(name="bound", n_tracks=n_tracks, seed=0xB0D, samples=samples, clips=clips, volumes_db=vols,
               pans=pans, mutes=[False] * n_tracks, block=block, channels=channels)
    if salt:
        spec.salt = salt
    return spec


@pytest.mark.parametrize("fmts,rates", [(("i24",), (44100, 48000)), (("i16", "i24"), (44100, 48000)), (("f32", "i32"), (96000, 44100)),
                                        (("i16", "i24", "f32"), (44100, 96000, 48000))])
def test_clip_boundaries_in_the_hot_loop_every_format(fmts, rates):
    """... and for the sessions the everything family serves: resampled 24 / 32-bit PCM, 16-bit resampled beside other
    formats, 96 kHz clips (per-frame taps) — no pre-render queue entry for a block with one or two stream calls."""
    n_blocks = 9
    spec = _boundary_session(40, n_blocks, 512, 1.3)
    for i, smp in enumerate(spec.samples):
        smp.fmt = fmts[i % len(fmts)]
        smp.rate = rates[(i // 2) % len(rates)]
        smp.amp = 0.02 if smp.fmt == "f32" else 1.0
        smp.frames = int(smp.frames * 2.2)
    spec.volumes_db = [v - (0.0 if spec.samples[2 * t].fmt == "f32" else 30.0) for t, v in enumerate(spec.volumes_db)]
    check_against_oracle(spec, n_blocks, group_size=40, expect_exact=True)
    eng = build_engine(spec, max_blocks=n_blocks, group_size=40)
    eng.play()
    eng.render(n_blocks)
    eng.ctx.fetch()
    # family 1 (everything) when a clip needs per-frame taps (played faster than 0.999 of the session rate), else family 3:
    # the same modes without them, both channels of a frame per lane
    taps = any(0.999 < spec.samples[c.sample].rate / float(spec.sample_rate) * c.speed != 1.0 for c in spec.clips)
    assert eng.ctx.kernel_name() == ("wbx::mix_kernel<2, true, 4, 1, 1, 1, 1, 256>" if taps else "wbx::mix_kernel<1, true, 3, 3, 1, 1, 2, 128>")
    eng.close()


@pytest.mark.parametrize("masked", ["1", "0"])
@pytest.mark.parametrize("clip_blocks,block,channels,n_tracks,group", [(1.3, 512, 2, 40, 0), (0.7, 512, 2, 40, 16), (2.45, 1024, 2, 24, 0),
                                                                       (3.1, 1024, 1, 24, 5), (1.9, 512, 2, 300, 200)])
def test_clip_boundaries_in_the_hot_loop(monkeypatch, masked, clip_blocks, block, channels, n_tracks, group):
    """Track-blocks with a clip start / end inside them — one partial stream call, or two that do not overlap — are
    rendered by mix_kernel itself as masked rows (ROW_PAIRs staged as two records; WBX_MASKED_ROWS=0 sends them through
    the pre-render pass as before): stream-call log, peaks and master equal the oracle's either way.  group 200 of 300
    tracks: groups longer than one staged chunk, pairs on both sides of a chunk seam."""
    monkeypatch.setenv("WBX_MASKED_ROWS", masked)
    n_blocks = 7
    spec = _boundary_session(n_tracks, n_blocks, block, clip_blocks, channels)
    if group == 0:
        check_against_oracle(spec, n_blocks, group_size=n_tracks if n_tracks <= 128 else 0, expect_exact=n_tracks <= 128)
    else:
        check_against_oracle(spec, n_blocks, group_size=group)


@pytest.mark.parametrize("fmts,rates,family", [(("f32",), (44100, 48000), 0), (("i24", "i16"), (44100, 48000), 1), (("i16",), (44100,), 1)])
@pytest.mark.parametrize("clip_blocks,block,channels,instance", [(1.3, 128, 2, "1, 2, 1, 64>"), (2.2, 256, 2, "1, 1, 1, 128>"),
                                                                 (0.7, 512, 1, "1, 1, 1, 128>"), (1.7, 256, 1, "1, 1, 1, 64>")])
@pytest.mark.parametrize("packed", ["1", "0", "default"])
def test_clip_boundaries_in_the_hot_loop_short_blocks(monkeypatch, packed, clip_blocks, block, channels, instance, fmts, rates, family):
    """... and for blocks shorter than a 256-lane workgroup — 128-frame stereo, 256-frame stereo, 256 / 512-frame mono, the
    buffer sizes of a low-latency device: a session cut into clips takes instances that stage the sequencer's masked rows
    like the full-size ones: one block per workgroup (a wave, or two), or the PACKED instances (mix_kernel_x: 2 or 4 blocks
    per workgroup, the two-pass staging per sub-block) — the library's choice for 128-frame stereo blocks in renders of 8
    blocks and more, WBX_PACKED_X=1 / 0 forces them on every shape / off.  Families 0 and 1 hold both sets; the 16-bit-only
    and the no-per-frame-taps families borrow family 1's."""
    if packed != "default":
        monkeypatch.setenv("WBX_PACKED_X", packed)
    else:
        packed = "1" if (block, channels) == (128, 2) else "0"
    n_blocks = 9
    spec = _boundary_session(40, n_blocks, block, clip_blocks, channels)
    for i, smp in enumerate(spec.samples):
        smp.fmt = fmts[i % len(fmts)]
        smp.rate = rates[(i // 2) % len(rates)]
        smp.amp = 0.02 if smp.fmt == "f32" else 1.0
        smp.frames = int(smp.frames * 2.2)
    spec.volumes_db = [v - (0.0 if spec.samples[2 * t].fmt == "f32" else 30.0) for t, v in enumerate(spec.volumes_db)]
    check_against_oracle(spec, n_blocks, group_size=40, expect_exact=True)
    eng = build_engine(spec, max_blocks=n_blocks, group_size=40)
    eng.play()
    eng.render(n_blocks)
    eng.ctx.fetch()
    name = eng.ctx.kernel_name()
    sb, cw = {(128, 2): (4, 2), (256, 2): (2, 1), (512, 1): (2, 1), (256, 1): (4, 1)}[(block, channels)]
    if block == 256 and channels == 2 and fmts == ("i16",):   # (the 16-bit family has its own one-wave instance for this shape)
        assert name == "wbx::mix_kernel<2, true, 3, 2, 1, 1, 2, 64>"
    elif packed != "0":
        assert name == f"wbx::mix_kernel_x<2, 4, {family}, {sb}, {cw}, 1>", name
    elif block == 256 and channels == 2 and fmts == ("f32",):   # (... and so has the lean fp32 one)
        assert name == "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 64>"
    else:
        assert name == f"wbx::mix_kernel<2, true, 3, {family}, 1, " + instance[3:], name
    eng.close()


@pytest.mark.parametrize("packed", ["1"])
@pytest.mark.parametrize("block,channels,n_tracks,group,n_blocks", [(128, 2, 300, 0, 18), (256, 2, 200, 128, 11), (512, 1, 150, 70, 9),
                                                                      (256, 1, 130, 0, 14), (128, 2, 70, 33, 35)])
def test_packed_masked_rows_many_chunks(monkeypatch, packed, block, channels, n_tracks, group, n_blocks):
    """The packed masked-row instances over groups longer than one staged chunk (32 / 64 / 128 tracks per sub-block), render
    lengths that leave the last workgroup with empty sub-blocks, clips shorter than a block (pairs in most track-blocks) and
    longer ones: stream-call log, peaks and master against the oracle."""
    monkeypatch.setenv("WBX_PACKED_X", packed)
    for clip_blocks in (1.1, 2.3):
        spec = _boundary_session(n_tracks, n_blocks, block, clip_blocks, channels)
        check_against_oracle(spec, n_blocks, group_size=group if group else (n_tracks if n_tracks <= 128 else 0),
                             expect_exact=(group == 0 and n_tracks <= 128))
    eng = build_engine(spec, max_blocks=n_blocks, group_size=group)
    eng.play()
    eng.render(n_blocks)
    eng.ctx.fetch()
    assert eng.ctx.kernel_name().startswith("wbx::mix_kernel_x<2, "), eng.ctx.kernel_name()
    eng.close()


@pytest.mark.parametrize("salt", ["denormals_and_zeros", "nonfinite"])
def test_masked_rows_with_special_float_values(salt):
    """non-finite and denormal samples right at clip boundaries: a masked-out frame contributes an exact +0.0 whatever
    was loaded for it, a unity row inside a chunk of resampled rows copies its sample (no 0 * inf)"""
    n_blocks = 6
    spec = _boundary_session(20, n_blocks, 512, 0.9, salt=salt)
    om, opk, _, orows, _ = run_oracle(spec, n_blocks)
    eng = build_engine(spec, max_blocks=n_blocks, group_size=20)
    eng.play()
    eng.render(n_blocks)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    assert plan_rows(eng.fetch_plan()) == orows
    if salt != "nonfinite":
        assert np.array_equal(bits(m), bits(om))
        assert np.array_equal(pk, opk[..., :spec.channels])
    else:                                             # NaN where the reference has NaN, the same bits elsewhere
        assert np.array_equal(np.isnan(m), np.isnan(om))
        ok = ~np.isnan(om)
        assert np.array_equal(bits(m)[ok], bits(om)[ok])
    eng.close()


@pytest.mark.parametrize("salt", ["denormals_and_zeros", "huge", "nonfinite"])
@pytest.mark.parametrize("src_rate", [48000, 44100, 96000])
def test_special_float_values(salt, src_rate):
    """Denormal samples and products are kept (the reference build does not flush them), signed zeros follow the
    reference's additions, values near FLT_MAX overflow where the reference's do: master and peaks bit-equal.
    With infinities and NaNs in the clips the master still matches sample for sample (NaN where the reference has
    NaN — the clamp of engine.cpp:1627-1636 lets it through —, the same bits everywhere else).  The peak of a
    track-block that CONTAINS a NaN is the one documented deviation: the reference's math::max restarts after every
    NaN (its result depends on where the NaN sits in the block), the wave-parallel maximum ignores NaN."""
    base = synth.make_session("spv", 24, seek=True, n_blocks=4, seed=0x5F0 + src_rate // 100, src_rate=src_rate, amp=1e-3)
    spec = _SpecialValuesSpec(**{f.name: getattr(base, f.name) for f in dataclasses.fields(base)})
    spec.salt = salt
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = [-60.0, 0.0, -20.0][t % 3]
    om, opk, _, orows, _ = run_oracle(spec, 4)
    eng = build_engine(spec, max_blocks=4, group_size=24)
    eng.play()
    eng.render(4)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    assert plan_rows(eng.fetch_plan()) == orows
    if salt != "nonfinite":
        assert np.array_equal(bits(pk), bits(opk[..., :spec.channels]))
        assert np.array_equal(bits(m), bits(om))
    else:
        assert np.array_equal(np.isnan(m), np.isnan(om))
        ok = ~np.isnan(om)
        assert np.array_equal(bits(m)[ok], bits(om)[ok])
        assert not np.isnan(pk).any()
    eng.close()


def test_empty_and_tiny_samples():
    """Clips on samples of 0, 1 and 3 frames (shorter than a lane's four frames), at unity and resampled rates:
    the sampler's tail arithmetic (sampler.cpp:100-104) leaves nothing or a few frames to render."""
    spec = synth.make_session("tiny", 12, n_blocks=3, seed=0x717)
    for i, smp in enumerate(spec.samples):
        smp.frames = [0, 1, 3, 700][i % 4]
        smp.rate = [48000, 44100, 96000][i % 3]
    check_against_oracle(spec, 3, expect_exact=True)


def test_api_errors_leave_the_engine_usable():
    """Where the reference asserts (audio_buffer.h:35,50,74; track.cpp:687-688) the C ABI returns a status: invalid
    arguments are refused with WBX_ERR_INVALID and the engine keeps rendering the same bits afterwards."""
    spec = synth.make_session("err", 6, n_blocks=3, seed=0xE77)
    om, _, _, _, _ = run_oracle(spec, 3)
    eng = build_engine(spec, max_blocks=2)
    eng.play()
    with pytest.raises(W.WbxError):
        eng.render(3)                                   # more blocks than wbx_config.max_blocks
    with pytest.raises(W.WbxError):
        eng.render(0)
    with pytest.raises(W.WbxError):
        eng.add_audio_clip(eng.tracks[0], "x", 1.0, 2.0, 0.0, 999)          # unknown sample
    with pytest.raises(W.WbxError):
        eng.add_audio_clip(eng.tracks[0], "x", 3.0, 2.0, 0.0, 0)            # min_time > max_time
    with pytest.raises(W.WbxError):
        eng.delete_track(17)
    with pytest.raises(W.WbxError):
        eng.move_track(0, 17)
    with pytest.raises(W.WbxError):
        eng.move_clip(eng.tracks[0], 5, 0.25)                               # no such clip
    eng.tracks[0].set_bus(3)                 # defined, not an error: without such a bus the track feeds the master
    eng.render(2)
    m, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m), bits(om[:2]))
    eng.render(1)
    m, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m[0]), bits(om[2]))
    eng.close()
    # a track more than the configured maximum
    eng = W.Engine(2)
    eng.add_track()
    eng.add_track()
    with pytest.raises(W.WbxError):
        eng.add_track()
    eng.close()


def test_one_engine_20000_tracks():
    """More tracks on one device than any BASELINE single-GPU config: 20000 tracks (157 groups, the last one
    ragged) in one engine, clips generated on the device."""
    spec = synth.make_session("big", 20000, n_blocks=2, seed=0xB16, src_rate=44100)
    check_against_oracle(spec, 2, device_synth=True)


def test_extreme_playback_speeds():
    """Stretch factors at and beyond the bounds of the hot loop's row kinds: 0.001 (window, general tap selection),
    0.999 / 0.9990001 (window / per-frame taps), 4096 (per-frame taps) and 5000, 20000 (pre-render pass)."""
    block, n_blocks = 64, 4
    speeds = [0.001, 0.999, 0.9990001, 1.0, 4096.0, 4096.5, 5000.0, 20000.0, 37.25, 0.75, 0.7499999]
    beat_frames = 48000 * 60.0 / 120.0
    samples, clips = [], []
    for t, sp in enumerate(speeds):
        frames = int(block * (n_blocks + 2) * max(sp, 1.0)) + 64
        samples.append(synth.SampleSpec(seed_track=t, channels=2, rate=48000, frames=frames, fmt="f32" if t % 2 == 0 else "i16",
                                        amp=0.05 if t % 2 == 0 else 1.0))
        clips.append(synth.ClipSpec(t, 0.0, (n_blocks + 1) * block / beat_frames, start_offset=3.0, speed=sp, gain=0.5))
    n = len(speeds)
    spec = synth.SessionSpec(name="xs", n_tracks=n, seed=0xE5, samples=samples, clips=clips, volumes_db=[-30.0] * n,
                             pans=[0.1 * (i - 5) for i in range(n)], mutes=[False] * n, block=block)
    check_against_oracle(spec, n_blocks, expect_exact=True)
    spec.block = 512
    for smp, sp in zip(samples, speeds):
        smp.frames = int(512 * (n_blocks + 2) * max(sp, 1.0)) + 64
    check_against_oracle(spec, n_blocks, expect_exact=True)


def test_clamp_and_unclamped_partial():
    spec = synth.make_session("hot", 16, n_blocks=2, amp=0.5, seed=0x5EED0007)
    om, _, _, _, _ = run_oracle(spec, 2)
    assert (np.abs(om) == 1.0).any()
    eng = build_engine(spec, max_blocks=2)
    eng.play()
    eng.render(2)
    m, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m), bits(om))
    eng.close()
    # shard mode: un-clamped partial, then finalize (the clamp after the reduce)
    eng = build_engine(spec, max_blocks=2)
    eng.ctx.set_clamp(False)
    eng.play()
    eng.render(2)
    raw, _, _ = eng.ctx.fetch()
    assert np.abs(raw).max() > 1.0
    ptr, n = eng.ctx.partial_master()
    assert n == 2 * 2 * 512
    eng.ctx.finalize_master(ptr, 2, True)
    m2, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m2), bits(om))
    eng.close()
    # the same, out of place into pinned host memory (what the root rank of a multi-GPU run does after the reduce)
    import torch
    eng = build_engine(spec, max_blocks=2)
    eng.ctx.set_clamp(False)
    eng.play()
    eng.render(2)
    ptr, n = eng.ctx.partial_master()
    host = torch.zeros(n, dtype=torch.float32).pin_memory()
    eng.ctx.finalize_master_into(ptr, host.data_ptr(), 2, True)
    eng.ctx.sync()
    assert np.array_equal(bits(host.numpy().reshape(om.shape)), bits(om))
    eng.close()


def test_levels_running_max():
    spec = synth.make_session("lv", 10, n_blocks=4, seed=0x61)
    _, opk, _, _, _ = run_oracle(spec, 4)
    eng = build_engine(spec, max_blocks=4)
    eng.play()
    eng.render(4)
    lv = eng.levels()
    assert np.array_equal(lv, opk.max(axis=0))
    assert not eng.levels().any()          # VUMeter::update exchanges the level with 0
    eng.close()


def test_interleaved_output_formats():
    """Next-1 row: planar fp32 master -> interleaved device formats (audio_format_conv.cpp)."""
    spec = synth.make_session("conv", 16, n_blocks=2, amp=0.2, seed=0x71)
    om, _, _, _, _ = run_oracle(spec, 2)
    eng = build_engine(spec, max_blocks=2)
    eng.play()
    eng.render(2)
    L = O.lib()
    for fmt, dt in (("i16", np.int16), ("i24", np.uint8), ("i24_x8", np.int32), ("i32", np.int32), ("f32", np.float32)):
        got = eng.ctx.fetch_interleaved(fmt)
        exp = []
        for b in range(2):
            # packed 24-bit: 3 bytes per sample; the reference's writer leaves all but the first 3*F bytes of a block
            # untouched (its destination index has no channel term, audio_format_conv.cpp:22-43) — zero on both sides
            a = np.zeros(512 * 2 * (3 if fmt == "i24" else 1), dt)
            src = [np.ascontiguousarray(om[b][c]) for c in range(2)]
            getattr(L, "wbo_f32_to_interleaved_" + fmt)(a.ctypes.data, O.planar_ptrs(src), 0, 512, 2)
            exp.append(a)
        assert np.array_equal(got.view(np.uint8), np.concatenate(exp).view(np.uint8)), fmt
    eng.close()


def test_host_bound_master_of_a_long_render_leaves_through_the_staging_buffer():
    """A master bound for pinned host memory (wbx_set_master_target) of 4 MB and more is summed into a device staging buffer
    and copied out on the sum stream (the sum kernel's own PCIe stores held up the next mix); shorter renders keep the
    direct stores.  Planar fp32 and interleaved device formats, several renders through the staging ring, the same bits as
    the oracle either way."""
    from whitebox_amd.dist import PinnedBuffer
    K = 2048
    spec = synth.make_session("stage", 8, n_blocks=2 * K, seed=0x57A6, src_rate=44100, amp=0.2)
    om, _, _, _, _ = run_oracle(spec, 2 * K)
    host = PinnedBuffer(K * 2 * 512)
    eng = build_engine(spec, max_blocks=K)
    eng.ctx.set_master_target(host.ptr)
    eng.play()
    for r in range(2):                                   # 8 MB per render: staged
        eng.render(K)
        eng.ctx.sync()
        assert np.array_equal(bits(host.array.reshape(K, 2, 512)), bits(om[r * K:(r + 1) * K])), r
    eng.stop()
    eng.play()
    eng.render(256)                                      # 1 MB: the sum kernel stores it itself
    eng.ctx.sync()
    assert np.array_equal(bits(host.array.reshape(K, 2, 512)[:256]), bits(om[:256]))
    L = O.lib()
    for fmt, dt, per in (("i16", np.int16, 2), ("f32", np.float32, 4)):   # 2048 x 512 x 2 samples: 4 MB / 8 MB, staged
        eng.ctx.set_master_format(fmt)
        eng.stop()
        eng.play()
        eng.render(K)
        eng.ctx.sync()
        exp = np.zeros(K * 512 * 2, dt)
        for b in range(K):
            src = [np.ascontiguousarray(om[b][c]) for c in range(2)]
            getattr(L, "wbo_f32_to_interleaved_" + fmt)(exp[b * 1024:].ctypes.data, O.planar_ptrs(src), 0, 512, 2)
        got = host.array.view(np.uint8)[:K * 1024 * per]
        assert np.array_equal(got, exp.view(np.uint8)), fmt
    eng.ctx.set_master_format(None)
    eng.close()
    host.close()


@pytest.mark.parametrize("channels", [2, 1])
def test_device_format_as_the_sum_kernel_epilogue(channels):
    """wbx_engine_process_interleaved (the audio callback: Engine::process + interleave_samples_to in one call) and
    wbx_set_master_format (render-ahead): the conversion of audio_format_conv.cpp as the epilogue of the sum kernel — all
    five formats, stereo and mono out, a hot session (the clamp precedes the conversion), buses; bytes equal to the
    reference's converters over the oracle's master."""
    K = 3
    spec = synth.make_session("convf", 24, n_blocks=K, amp=0.3, seed=0x73, n_buses=3, src_rate=44100)
    spec.channels = channels
    om, _, _, _, _ = run_oracle(spec, K)
    assert (np.abs(om) == 1.0).any()
    L = O.lib()

    def expected(fmt, dt, b):
        a = np.zeros(512 * channels * (3 if fmt == "i24" else 1), dt)
        src = [np.ascontiguousarray(om[b][c]) for c in range(channels)]
        getattr(L, "wbo_f32_to_interleaved_" + fmt)(a.ctypes.data, O.planar_ptrs(src), 0, 512, channels)
        return a
    formats = (("i16", np.int16), ("i24", np.uint8), ("i24_x8", np.int32), ("i32", np.int32), ("f32", np.float32))
    eng = build_engine(spec, max_blocks=1)
    for fmt, dt in formats:
        eng.play()
        for b in range(K):
            got = eng.process_interleaved(fmt)
            assert np.array_equal(got.view(np.uint8), expected(fmt, dt, b).view(np.uint8)), (fmt, b)
        eng.stop()
    out = W.AudioBuffer(512, channels)                         # ... and the planar call is what it was
    eng.play()
    eng.process(None, out, 48000.0)
    assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om[0]))
    eng.close()
    eng = build_engine(spec, max_blocks=K)
    for fmt, dt in formats:
        eng.ctx.set_master_format(fmt)
        eng.play()
        eng.render(K)
        got = eng.ctx.fetch_interleaved(fmt)
        exp = np.concatenate([expected(fmt, dt, b) for b in range(K)])
        assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), fmt
        with pytest.raises(W.WbxError):
            eng.ctx.fetch()                                    # no planar master after such a render
        eng.stop()
    eng.ctx.set_master_format(None)
    eng.play()
    eng.render(K)
    m, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m), bits(om))
    eng.close()


def test_interleaved_output_of_an_unclamped_master():
    """wbx_set_clamp(0) (shard mode) or NaN in the master: the float -> integer conversions must give what the
    reference's x86 build gives — cvttss2si / cvttsd2si return 0x80000000 out of range, the 16- and 24-bit paths then
    truncate — not the GPU's saturating conversion."""
    spec = synth.make_session("hotconv", 16, n_blocks=2, amp=60000.0, seed=0x72)     # far above full scale
    spec.volumes_db = [12.0] * 16
    e = O.build_oracle_engine(spec)
    e.play()
    om = np.stack([e.process(clamp=False)[0] for _ in range(2)])
    e.close()
    assert np.abs(om).max() > 40000.0        # 32767 * |v| leaves the int32 range for part of the block
    eng = build_engine(spec, max_blocks=2)
    eng.ctx.set_clamp(False)
    eng.play()
    eng.render(2)
    m, _, _ = eng.ctx.fetch()
    assert np.array_equal(bits(m), bits(om))
    L = O.lib()
    for fmt, dt in (("i16", np.int16), ("i24", np.uint8), ("i24_x8", np.int32), ("i32", np.int32)):
        got = eng.ctx.fetch_interleaved(fmt)
        exp = []
        for b in range(2):
            a = np.zeros(512 * 2 * (3 if fmt == "i24" else 1), dt)
            src = [np.ascontiguousarray(om[b][c]) for c in range(2)]
            getattr(L, "wbo_f32_to_interleaved_" + fmt)(a.ctypes.data, O.planar_ptrs(src), 0, 512, 2)
            exp.append(a)
        assert np.array_equal(got.view(np.uint8), np.concatenate(exp).view(np.uint8)), fmt
    eng.close()


def test_effect_slot_is_kept_but_unimplemented():
    """the boundary keeps Track::plugin_instance / Engine::add_plugin_to_track; attaching a plugin is
    PluginResult::Unimplemented (-2) and leaves the slot empty, detaching and rendering work as before."""
    from whitebox_amd import _ffi
    spec = synth.make_session("fx", 4, n_blocks=2, seed=0x73)
    om, opk, _, _, _ = run_oracle(spec, 2)
    eng = build_engine(spec, max_blocks=2)
    assert eng.tracks[1].plugin_instance is None
    eng.add_plugin_to_track(eng.tracks[1], None)             # NULL: clears the (empty) slot
    with pytest.raises(W.WbxError) as ei:
        eng.add_plugin_to_track(eng.tracks[1], _ffi.Plugin(None, None))
    assert ei.value.status == -2
    assert eng.tracks[1].plugin_instance is None
    eng.delete_plugin_from_track(eng.tracks[1])
    eng.play()
    eng.render(2)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    assert np.array_equal(bits(m), bits(om)) and np.array_equal(pk, opk[..., :spec.channels])
    eng.close()


def test_abi_rejects_what_would_fault_the_device():
    """the C ABI is the trust boundary: segments with a negative / NaN position or a non-positive / NaN speed, and
    freeing a sample a clip list still names, are refused instead of reaching the kernels"""
    spec = synth.make_session("trust", 2, n_blocks=2, seed=0x74)
    eng = build_engine(spec, max_blocks=1)
    so, g = np.array([0, 1, 1], np.uint32), np.ones(4, np.float32)
    for bad in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, float("nan")), (0.0, 1e300)):
        with pytest.raises(W.WbxError) as ei:
            eng.ctx.submit(1, 2, [(bad[0], bad[1], 0, 0, 512, 1.0)], so, g)
        assert ei.value.status == -4, bad
    with pytest.raises(W.WbxError) as ei:
        _check_free(eng, 0)
    assert ei.value.status == -4
    with pytest.raises(W.WbxError) as ei:
        eng.delete_sample(1)                                 # the engine-side form (takes the editor lock): same rule
    assert ei.value.status == -4
    eng.delete_clip(eng.tracks[0], 0)
    _check_free(eng, 0)                                      # no clip names it any more
    eng.delete_clip(eng.tracks[1], 0)
    eng.delete_sample(1)
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    eng.process(None, out, float(spec.sample_rate))          # still usable
    eng.close()


def _check_free(eng, clip):
    st = eng.L.wbx_clip_free(eng.ctx.h, clip)
    if st != 0:
        raise W.WbxError(st, "wbx_clip_free", eng.L.wbx_last_error(eng.ctx.h).decode())


def test_master_ready_orders_a_foreign_stream():
    """the sum of a render runs on its own stream; a caller that reads a caller-owned master target
    on ANOTHER stream must be ordered after it with wbx_master_ready — without any host synchronisation."""
    import torch
    K = 16
    spec = synth.make_session("ready", 96, src_rate=44100, n_blocks=K, seed=0x75)
    om, _, _, _, _ = run_oracle(spec, K)
    eng = build_engine(spec, max_blocks=K)
    target = torch.zeros(K * 2 * 512, dtype=torch.float32, device="cuda")
    copy = torch.zeros_like(target)
    side = torch.cuda.Stream()
    eng.ctx.set_master_target(target.data_ptr())
    eng.play()
    for rep in range(3):                                     # also across renders in flight
        if rep:
            eng.stop()
            eng.play()
        eng.render(K)
        eng.ctx.master_ready(side.cuda_stream)
        with torch.cuda.stream(side):
            copy.copy_(target, non_blocking=True)
        side.synchronize()
        got = copy.cpu().numpy().reshape(K, 2, 512)
        assert np.array_equal(bits(got), bits(om)), rep
    eng.ctx.set_master_target(None)
    eng.close()


def test_batch_render_of_clips_that_outlast_their_audio():
    """a clip region much longer than its sample used to take one plan template per block and
    overflow the template array in long batches; the finished stream calls now share one template."""
    K = 256
    spec = synth.make_session("outlast", 3, n_blocks=4, seed=0x0A71)
    for s in spec.samples:
        s.frames = 700
    for c in spec.clips:
        c.max_beat = c.min_beat + (K + 8) * 512 / 24000.0
    check_against_oracle(spec, K, expect_exact=True)


# ---------------------------------------------------------------------------------------------------
# layer 1: host-sequenced segments (the reference keeps Track::process_event, the device mixes)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_rate,fmt,block", [(44100, "f32", 512), (96000, "f32", 512), (44100, "i16", 256),
                                                (44100, "i24", 128), (48000, "i16", 512)])
def test_layer1_submit_host_sequenced(src_rate, fmt, block):
    spec = synth.make_session("l1", 96, seek=True, src_rate=src_rate, n_blocks=5, seed=0x81, fmt=fmt, block=block)
    if fmt != "f32":
        for t in range(spec.n_tracks):
            spec.volumes_db[t] = -40.0
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    e.play()
    ctx = W.MixContext(spec.n_tracks, max_blocks=5, block=block, group_size=32)
    for i, s in enumerate(spec.samples):
        ctx.clip_upload(i, s.fmt, s.rate, [np.ascontiguousarray(a[:s.frames]) for a in spec.sample_data(i)])
    segs, offs, gains, masters, peaks, tracks = [], [0], [], [], [], []
    for b in range(5):
        m, _, tb = e.process_tracks()
        masters.append(m)
        tracks.append(tb)
        peaks.append(e.peaks())
        log = e.seglog()
        per_track = {}
        for (t, ds, ln, off, spd, g, smp) in log:
            per_track.setdefault(t, []).append((off, spd, smp, ds, ln, g))
        for t in range(spec.n_tracks):
            segs += per_track.get(t, [])
            offs.append(len(segs))
        gains.append(e.gains())
    ctx.submit(5, spec.n_tracks, segs, np.array(offs, np.uint32), np.stack(gains))
    m, pk, _ = ctx.fetch(peaks=True)
    assert np.array_equal(pk, np.stack(peaks))
    assert rms(m, np.stack(masters)) <= RMS_TOL
    GO.assert_grouped(m, np.stack(tracks), 32, what="submit")      # ... and groups of 32, bit for bit
    ctx.close()
    e.close()


def test_kernel_timer_reports():
    spec = synth.make_session("t", 64, n_blocks=2)
    eng = build_engine(spec, max_blocks=2)
    eng.play()
    eng.ctx.kernel_time(reset=True)
    eng.render(2)
    eng.render(2)
    ms, n = eng.ctx.kernel_time()
    assert n == 2 and ms > 0.0
    # the instance the library launched, as rocprofv3 prints it: a unity-speed stereo 512-frame session takes U = 4, W = 3
    assert eng.ctx.kernel_name() == "wbx::mix_kernel<4, true, 3, 0, 1, 1, 1, 256>"
    eng.close()


def test_kernel_name_follows_the_session(monkeypatch):
    """wbx_kernel_name: resampled stereo 512-frame sessions take the instance with both channels of a frame in one lane
    (CL = 2), WBX_NO_CL2 the one-channel-per-wave instance; both give the same master bit for bit."""
    spec = synth.make_session("r", 200, n_blocks=8, src_rate=44100, seek=True)   # (seek: clip boundaries inside blocks)
    outs = {}
    for no_cl2 in (False, True):
        if no_cl2:
            monkeypatch.setenv("WBX_NO_CL2", "1")
        eng = build_engine(spec, max_blocks=8)
        eng.play()
        eng.render(8)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        outs[no_cl2] = (m.copy(), pk.copy(), eng.ctx.kernel_name())
        eng.close()
    assert outs[False][2] == "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 128>"
    assert outs[True][2] == "wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>"
    assert np.array_equal(outs[False][0], outs[True][0]) and np.array_equal(outs[False][1], outs[True][1])
    # ... and a render of fewer than 8 blocks (the callback path: a handful of workgroups, each a chain of dependent rows)
    # takes the wave-per-channel-half instance by itself: four waves share the chain instead of two
    monkeypatch.delenv("WBX_NO_CL2")
    eng = build_engine(spec, max_blocks=8)
    eng.play()
    eng.render(5)
    m5, pk5, _ = eng.ctx.fetch(peaks=True)
    assert eng.ctx.kernel_name() == "wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>"
    assert np.array_equal(m5, outs[False][0][:5]) and np.array_equal(pk5, outs[False][1][:5])
    eng.close()


def test_one_resampling_ratio_reaches_the_kernel(monkeypatch):
    """MixArgs::uniform_speed: a session whose resampled clips all play at one ratio in [0.67, 0.999] (44.1 kHz clips in a 48 kHz
    session) tells the mix so (MODE_WNU / MODE_WINU: the products fl(j * speed) hoisted out of the track loop) — the value the
    kernel was launched with, bit for bit Sampler::reset_state's expression; a second ratio, or WBX_NO_UNIFORM=1, withdraws it;
    the master is the same bits either way.  (Rounds 3-4 carried the modes and never took them: the assignment had been lost.)"""
    spec = synth.make_session("u", 40, n_blocks=8, src_rate=44100)
    masters = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("WBX_NO_UNIFORM", "1")
        eng = build_engine(spec, max_blocks=8)
        eng.play()
        eng.render(8)
        m, _, _ = eng.ctx.fetch()
        masters.append(m.copy())
        assert eng.ctx.uniform_speed() == (0.0 if off else (44100.0 / 48000.0) * 1.0)
        eng.close()
    assert np.array_equal(bits(masters[0]), bits(masters[1]))
    monkeypatch.delenv("WBX_NO_UNIFORM")
    # a clip at another ratio: no promise any more
    spec2 = synth.make_session("u2", 40, n_blocks=8, src_rate=44100)
    spec2.clips[3].speed = 0.8
    eng = build_engine(spec2, max_blocks=8)
    eng.play()
    eng.render(8)
    eng.ctx.fetch()
    assert eng.ctx.uniform_speed() == 0.0
    eng.close()
    # ... and a session at the device rate has nothing to hoist
    eng = build_engine(synth.make_session("u3", 40, n_blocks=8, src_rate=48000), max_blocks=8)
    eng.play()
    eng.render(8)
    eng.ctx.fetch()
    assert eng.ctx.uniform_speed() == 0.0
    eng.close()


def test_cpp_host_through_the_adapter(tmp_path):
    """A C++ host written against include/wbx_adapter.hpp (reference-shaped Engine/Track/AudioBuffer),
    compiled with plain g++ and linked to libwbx.so, is bit-identical to the oracle."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adapter_smoke")
    O.lib()     # makes sure oracle/liboracle.so exists
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(root, "tests", "cpp", "adapter_smoke.cpp"),
                           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "oracle"),
                           "-L" + os.path.join(root, "whitebox_amd"), "-lwbx", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "whitebox_amd"), "-Wl,-rpath," + os.path.join(root, "oracle"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.check_output([exe]).decode()
    assert "adapter ok" in out


# ---------------------------------------------------------------------------------------------------
# clip edits: add with overlap / move / resize / delete / gain, while playing
# ---------------------------------------------------------------------------------------------------
# WBX_FUZZ3_FROM / WBX_FUZZ3_TO widen the seed range for a soak run (default: seeds 2024..2029; 2024 is the original
# all-fp32 512-frame script, the others also draw the block size, the storage formats and the sample rates)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ3_FROM", "2024")), int(os.environ.get("WBX_FUZZ3_TO", "2030"))))
def test_clip_edits_match_oracle_lists_and_audio(seed):
    """Random edit scripts applied to both engines through their reference-shaped APIs, between rendered
    blocks: the sorted clip lists (fp64 bit patterns), the sequencer's plan and the audio must stay equal."""
    spec = FZ.edit_session_spec(seed)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=2)
    e.enable_seglog()
    out = W.AudioBuffer(spec.block, spec.channels)

    def on_block(step, op):
        om, _ = e.process()
        eng.process(None, out, 48000.0)
        assert plan_rows(eng.fetch_plan()) == oracle_rows(e, 0), (seed, step, op)
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), (seed, step, op)

    FZ.run_edit_script(seed, spec, e, eng, on_block)
    e.close()
    eng.close()


@pytest.mark.parametrize("n_tracks", [6, 200])
def test_short_render_behind_a_batch_render_in_flight(n_tracks):
    """Regression (found by the edit scripts once they stopped fetching every render): a render of 8+ blocks leaves its sum
    pending on the sum stream; a short render issued right behind it — nobody fetched, nothing synchronised — sums on the
    main stream (a one-group session's mix even stores the master itself) into the same master buffer, and the batch
    render's late sum overwrote the head of its blocks.  The main stream now waits for the pending sum first.  Forty
    rounds of (10 blocks unfetched, then 1-3 blocks fetched), both session sizes: one group / several groups + sum launch."""
    rounds, K = 40, 10
    spec = synth.make_session("inflight", n_tracks, n_blocks=rounds * (K + 3), seed=0x1F17, src_rate=44100, amp=0.05)
    om, _, _, _, _ = run_oracle(spec, rounds * (K + 3))
    eng = build_engine(spec, max_blocks=K, group_size=n_tracks)
    eng.play()
    done = 0
    for r in range(rounds):
        eng.render(K)                      # not fetched: its sum is still pending when the next render is issued
        done += K
        k = 1 + r % 3
        eng.render(k)
        m, _, _ = eng.ctx.fetch()
        assert np.array_equal(bits(m), bits(om[done:done + k])), (r, k)
        done += k
    eng.close()


# WBX_FUZZ9_FROM / WBX_FUZZ9_TO widen the seed range for a soak run (default: seeds 2024..2031)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ9_FROM", "2024")), int(os.environ.get("WBX_FUZZ9_TO", "2032"))))
def test_clip_edits_between_renders_of_random_length(seed):
    """The same edit scripts, but between two edits the engine renders 1-12 blocks in one call — from 8 blocks on the batch
    path: the plan on its own stream two renders ahead of its consumer, the sum beside the next mix, the clip table
    re-uploaded (and the device's live clip flags merged back) while earlier renders may still be in flight."""
    spec = FZ.edit_session_spec(seed)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=12)
    e.enable_seglog()
    rng = np.random.default_rng(seed ^ 0xB10C)
    trail = []          # (k, fetched) of the renders so far: what a failure message needs

    def on_block(step, op):
        k = int(rng.integers(1, 13))
        oms, opks, rows = [], [], []
        for b in range(k):
            om, _ = e.process()
            oms.append(om)
            opks.append(e.peaks())
            rows += oracle_rows(e, b)
        eng.render(k)
        fetched = not rng.integers(0, 10) < 3
        trail.append((k, fetched))
        if not fetched:
            return          # nobody waits for this render: the next edit meets it in flight (its results are checked through
                            # the state every later render continues from)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        assert plan_rows(eng.fetch_plan()) == rows, (seed, step, op, trail[-4:])
        bad = [b for b in range(k) if not np.array_equal(bits(m[b]), bits(oms[b]))]
        badpk = [b for b in range(k) if not np.array_equal(pk[b], opks[b][:, :spec.channels])]
        assert not bad and not badpk, (seed, step, op, bad, badpk, trail[-4:], spec.block, spec.channels)

    FZ.run_edit_script(seed, spec, e, eng, on_block, steps=16)
    e.close()
    eng.close()


# ---------------------------------------------------------------------------------------------------
# integer PCM streamed directly by the hot loop
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i16", "i24", "i32"])
def test_integer_pcm_unity_fast_path(fmt):
    """All tracks in one storage format at unity speed: the mix kernel streams the integers itself
    (8 B per lane for 16-bit), with the reference's normalise-clamp-scale roundings (sampler.cpp:109-144)."""
    spec = synth.make_session("pcm_" + fmt, 192, fmt=fmt, n_blocks=4, seed=0xA16)
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -40.0 + (t % 7)
    check_against_oracle(spec, 4)                                     # grouped order: 3 groups of 64
    check_against_oracle(spec, 4, group_size=192, expect_exact=True)  # reference order: bit-exact


def test_mixed_storage_formats_in_one_group():
    """fp32, 16-bit, 24-bit, 32-bit and resampled tracks interleaved in the same group, with clip boundaries
    inside blocks (pre-rendered fp32 rows among integer rows): the per-row dispatch path."""
    spec = synth.make_session("mixfmt", 48, seek=True, n_blocks=6, seed=0xA17)
    fmts = ["f32", "i16", "i24", "i32"]
    for i, s in enumerate(spec.samples):
        s.fmt = fmts[i % 4]
        s.amp = 0.02 if s.fmt == "f32" else 1.0
        s.rate = 44100 if i % 5 == 0 else 48000
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -42.0
    check_against_oracle(spec, 6, expect_exact=True)


@pytest.mark.parametrize("block", [512, 256, 128])
def test_mixed_unity_formats_pipelined(block):
    """fp32, 16-bit, 24-bit and 32-bit clips, all at the session rate, interleaved in every group: the chunk runs
    pipelined with one 16-B load per row whatever its format (odd sample positions: 2-byte aligned 16-bit rows;
    clip boundaries inside blocks add pre-rendered fp32 rows)."""
    spec = synth.make_session("mu", 200, seek=True, n_blocks=6, block=block, seed=0xA18)
    fmts = ["f32", "i16", "i24", "i32", "i16"]
    for i, smp in enumerate(spec.samples):
        smp.fmt = fmts[i % 5]
        smp.amp = 0.02 if smp.fmt == "f32" else 1.0
    for i, c in enumerate(spec.clips):
        c.start_offset = float(i % 7)          # odd and even first samples
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -44.0
    check_against_oracle(spec, 6)
    check_against_oracle(spec, 6, group_size=200, expect_exact=True)


def test_resampled_fp32_next_to_integer_unity():
    """fp32 clips at another rate (window rows) in the same groups as 16/24-bit clips at the session rate."""
    spec = synth.make_session("mwf", 160, seek=True, n_blocks=5, seed=0xA19)
    for i, smp in enumerate(spec.samples):
        if i % 3 == 0:
            smp.rate = 44100
        else:
            smp.fmt = "i16" if i % 3 == 1 else "i24"
            smp.amp = 1.0
    for t in range(spec.n_tracks):
        spec.volumes_db[t] = -40.0 if t % 3 else 0.0
    check_against_oracle(spec, 5)
    check_against_oracle(spec, 5, group_size=160, expect_exact=True)


def test_long_batches_and_ragged_track_counts():
    """K up to the configured maximum, track counts that do not fill the last 64-lane plan workgroup, and
    batches of odd length."""
    for n_tracks, n_blocks in ((70, 13), (5, 1), (130, 27)):
        spec = synth.make_session("ragK", n_tracks, seek=n_blocks >= 4, src_rate=44100, n_blocks=n_blocks,
                                  seed=0xB00 + n_tracks)
        check_against_oracle(spec, n_blocks, group_size=32)
    spec = synth.make_session("bigK", 3, n_blocks=2048, seed=0xB10, src_rate=44100)
    e = O.build_oracle_engine(spec)
    e.play()
    eng = build_engine(spec, max_blocks=2048)
    eng.play()
    eng.render(2048)
    m, _, _ = eng.ctx.fetch()
    for b in range(2048):
        om, _ = e.process()
        if b % 97 == 0 or b > 2040:
            assert np.array_equal(bits(m[b]), bits(om)), b
    assert O.f64_bits(eng.transport()[0]) == O.f64_bits(e.playhead)
    e.close()
    eng.close()


def test_config5_32768_tracks_sharded_8way_on_one_gpu():
    """BASELINE config 5 at full size, the 8 shards rendered one after the other on this GPU: every shard's peaks
    equal the oracle's for its tracks, and the rank-ordered sum of the un-clamped partial masters, clamped after
    the sum (what the RCCL reduce + wbx_finalize_master do on a node), is within the RMS budget of the
    single-engine oracle over all 32768 tracks."""
    from test_dist_gloo import _shard_spec
    from whitebox_amd.dist import shard_tracks
    n_tracks, world, K = 32768, 8, 2
    spec = synth.make_session("c5", n_tracks, n_blocks=K, seed=0x5EED0006)
    om, opk, _, _, _ = run_oracle(spec, K)
    total = np.zeros_like(om)
    for rank in range(world):
        first, count = shard_tracks(n_tracks, world, rank)
        assert count == 4096
        eng = build_engine(_shard_spec(spec, first, count), max_blocks=K)
        eng.ctx.set_clamp(False)
        eng.play()
        eng.render(K)
        part, pk, _ = eng.ctx.fetch(peaks=True)
        assert np.array_equal(pk, opk[:, first:first + count, :spec.channels])
        sspec = _shard_spec(spec, first, count)                 # (one device's share: the grouped order, un-clamped, bit for bit)
        _, _, tracks = GO.oracle_tracks(sspec, K, clamp_master=False)
        groups = GO.render_partition(sspec, eng.ctx.render_order(K), 0, K)
        GO.assert_model(part, GO.grouped_sum(tracks, groups, do_clamp=False)[0], what=("shard", rank))
        total = (total + part).astype(np.float32)          # fp32 sum in rank order
        eng.close()
    clamped = np.where(total > 1.0, np.float32(1.0), np.where(total < -1.0, np.float32(-1.0), total))
    r = rms(clamped, om)
    print("config5 (8 shards) rms vs oracle:", r)
    assert r <= RMS_TOL, r


def test_tempo_change_and_playhead_jump_while_playing():
    """Engine::set_bpm (engine.cpp:24-30) and Engine::set_playhead_position (:32-41) between blocks of a running
    transport: the next block uses the new beat duration / playhead with the tracks' sequencer state untouched, as
    in the reference.  Master, peaks, the stream-call log and the transport doubles stay bit-equal to the oracle."""
    spec = synth.make_session("tempo", 40, seek=True, src_rate=44100, n_blocks=12, seed=0x7E)
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    eng = build_engine(spec, max_blocks=3, group_size=64)
    e.play()
    eng.play()
    done = 0

    def run(nblk):
        nonlocal done
        oms, opks, orow = [], [], []
        for b in range(nblk):
            om, _ = e.process()
            oms.append(om)
            opks.append(e.peaks())
            orow += oracle_rows(e, b)
        eng.render(nblk)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        assert plan_rows(eng.fetch_plan()) == orow, done
        assert np.array_equal(pk, np.stack(opks)), done
        assert np.array_equal(bits(m), bits(np.stack(oms))), done     # 40 tracks < one group: the oracle's order
        ph, sp, _ = eng.transport()
        assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(e.playhead), O.f64_bits(e.sample_position)), done
        done += nblk

    run(3)
    e.set_bpm(97.3)
    eng.set_bpm(97.3)
    run(3)
    e.set_playhead(0.013)          # a jump backwards while playing
    eng.set_playhead_position(0.013)
    run(3)
    e.set_bpm(151.0)
    eng.set_bpm(151.0)
    e.set_playhead(0.05)
    eng.set_playhead_position(0.05)
    run(2)
    e.close()
    eng.close()


# WBX_FUZZ_FROM / WBX_FUZZ_TO widen the seed range for a soak run (default: seeds 0..159)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ_FROM", "0")), int(os.environ.get("WBX_FUZZ_TO", "160"))))
def test_random_sessions_match_oracle(seed):
    spec, n_blocks = FZ.random_session(seed)
    # fewer tracks than one group and the oracle's bus order: everything bit-equal, including the stream-call log
    check_against_oracle(spec, n_blocks, expect_exact=True)


# WBX_FUZZ8_FROM / WBX_FUZZ8_TO widen the seed range for a soak run (default: seeds 0..23)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ8_FROM", "0")), int(os.environ.get("WBX_FUZZ8_TO", "24"))))
def test_random_sessions_rendered_in_random_pieces(seed, monkeypatch):
    """One engine, one transport, the session rendered in pieces of random length — batch renders of 8-24 blocks (plan and
    sum on their own streams, rings of three), short ones of 1-7 (everything on the main stream, the callback path's
    instances, one-group sessions without a sum launch) and single Engine::process calls, in random order: every piece
    equals the oracle's blocks at that position (peaks, sub-bus sums and master bit for bit — fewer tracks than a group),
    so nothing is lost or reordered when the path changes from one render to the next."""
    rng = np.random.default_rng(0x91EC + seed)
    kind = ["plain", "masked", "integer", "lean16", "everything"][seed % 5]
    monkeypatch.setenv("WBX_FUZZ_MAX_BLOCKS", "64")   # (sessions of up to 64 blocks: clips all the way through)
    if kind == "plain":
        spec, total = FZ.random_session(seed)
    else:
        spec, total = FZ.random_masked_session(seed, integer_unity=kind == "integer", lean16=kind == "lean16", everything=kind == "everything")
    total += 3                                          # (... and a few blocks past the end of the last clip)
    om, opk, obus, _, otr = run_oracle(spec, total, want_buses=bool(spec.n_buses))
    G = min(max(spec.n_tracks, 1), 128)
    if spec.n_tracks > G:   # more tracks than a workgroup's group: every path in groups of 128, against the grouped-order model
        _, _, tracks = GO.oracle_tracks(spec, total)
        om, obus = GO.grouped_sum(tracks, GO.spec_partition(spec, G), spec.n_buses)
    eng = build_engine(spec, max_blocks=24, group_size=G)
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    done = 0
    while done < total:
        mode = int(rng.integers(0, 3))
        k = 1 if mode == 0 else int(rng.integers(1, 8)) if mode == 1 else int(rng.integers(8, 25))
        k = min(k, total - done)
        if mode == 0:
            eng.process(None, out, float(spec.sample_rate))
            m = np.stack(out.channel_buffers)[None]
            _, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
        else:
            eng.render(k)
            m, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
        assert np.array_equal(bits(m), bits(om[done:done + k])), (done, k, mode)
        assert np.array_equal(pk, opk[done:done + k, :, :spec.channels]), (done, k, mode)
        if spec.n_buses:
            assert np.array_equal(bits(bus), bits(obus[done:done + k])), (done, k, mode)
        done += k
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(otr[0]), O.f64_bits(otr[1]))
    eng.close()


# WBX_FUZZ10_FROM / WBX_FUZZ10_TO widen the seed range for a soak run (default: seeds 0..23)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ10_FROM", "0")), int(os.environ.get("WBX_FUZZ10_TO", "24"))))
def test_random_pieces_with_controls_and_renders_in_flight(seed, monkeypatch):
    """The pieces again, now with what a host does between them — volume / pan / mute messages, stop, seek, play, a tempo
    change — and with a third of the renders never fetched, so that the next control or render meets them in flight (the
    parameter, patch and transport tables are rings the device reads in place; the sums of batch renders run beside what
    follows).  Every fetched piece equals the oracle's blocks at that position."""
    rng = np.random.default_rng(0xC0A7 + seed)
    monkeypatch.setenv("WBX_FUZZ_MAX_BLOCKS", "64")
    kind = ["plain", "masked", "integer", "lean16", "everything"][seed % 5]
    if kind == "plain":
        spec, total = FZ.random_session(seed)
    else:
        spec, total = FZ.random_masked_session(seed, integer_unity=kind == "integer", lean16=kind == "lean16", everything=kind == "everything")
    if spec.n_tracks == 0:
        pytest.skip("no tracks")
    total += 12
    # one workgroup walks all tracks (the reference's order: bit-exact) — or, every other seed, groups of 16 and a sum launch
    # (several groups also in short renders; the master then within the RMS budget, peaks and sub-bus membership still exact)
    exact = seed % 2 == 0 or spec.n_buses
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=24, group_size=spec.n_tracks if exact else 16)
    e.play()
    eng.play()
    cb_out = W.AudioBuffer(spec.block, spec.channels)
    done, trail, nt = 0, [], spec.n_tracks
    while done < total:
        r = rng.random()
        if r < 0.35:                                      # a parameter message (applied from the next block on, track.cpp:618-643)
            t, what = int(rng.integers(0, nt)), int(rng.integers(0, 3))
            if what == 0:
                v = float(rng.uniform(-30.0, 3.0))
                e.set_volume(t, v)
                eng.tracks[t].set_volume(v)
            elif what == 1:
                v = float(rng.uniform(-1.0, 1.0))
                e.set_pan(t, v)
                eng.tracks[t].set_pan(v)
            else:
                v = bool(rng.integers(0, 2))
                e.set_mute(t, v)
                eng.tracks[t].set_mute(v)
            trail.append(("param", t, what))
        elif r < 0.42:                                    # stop, seek, play
            beat = float(rng.uniform(0.0, 0.3))
            e.stop()
            eng.stop()
            e.set_playhead(beat)
            eng.set_playhead_position(beat)
            e.play()
            eng.play()
            trail.append(("seek", beat))
        elif r < 0.46:
            bpm = float(rng.choice([90.0, 120.0, 151.0]))
            e.set_bpm(bpm)
            eng.set_bpm(bpm)
            trail.append(("bpm", bpm))
        elif r < 0.50 and nt > 1:                          # the track list itself: the device state follows its Track
            a, b = int(rng.integers(0, nt)), int(rng.integers(0, nt))
            e.move_track(a, b)
            eng.move_track(a, b)
            trail.append(("move", a, b))
        elif r < 0.53:
            t = int(rng.integers(0, nt))
            e.solo_track(t)
            eng.solo_track(t)
            trail.append(("solo", t))
        elif r < 0.58 and spec.n_buses:                    # routing: a track moves to another sub-bus (or straight to the master)
            t, b = int(rng.integers(0, nt)), int(rng.integers(-1, spec.n_buses))
            e.set_bus(t, b)
            eng.tracks[t].set_bus(b)
            trail.append(("bus", t, b))
        elif r < 0.55 and nt > 2 and not spec.n_buses:
            t = int(rng.integers(0, nt))
            e.delete_track(t)
            eng.delete_track(t)
            nt -= 1
            trail.append(("delete", t))
        mode = int(rng.integers(0, 3))
        k = 1 if mode == 0 else int(rng.integers(1, 8)) if mode == 1 else int(rng.integers(8, 25))
        oms, opks, obus, tracks = [], [], [], []
        for _ in range(k):
            om, bu, tb = e.process_tracks(want_buses=bool(spec.n_buses))
            oms.append(om)
            opks.append(e.peaks())
            obus.append(bu)
            tracks.append(tb)
        done += k
        if mode == 0 and rng.random() < 0.5:              # the audio callback itself (waits for its block), amid whatever is in flight
            eng.process(None, cb_out, float(spec.sample_rate))
            trail.append(("process",))
            m = np.stack(cb_out.channel_buffers)[None]
            _, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
        else:
            eng.render(k)
            fetched = rng.random() >= 0.33 or os.environ.get("WBX_FUZZ_ALWAYS_FETCH") == "1"   # (diagnosis aid)
            trail.append((k, fetched))
            if not fetched:
                continue
            m, pk, bus = eng.ctx.fetch(peaks=True, buses=bool(spec.n_buses))
        if exact:
            bad = [b for b in range(k) if not np.array_equal(bits(m[b]), bits(oms[b]))]
        else:
            bad = [b for b in range(k) if rms(m[b], oms[b]) > RMS_TOL]
            # ... and the groups of 16 of the tracks as they are now, bit for bit
            bad += [("model", b) for b in range(k) if not GO.same_bits(
                m[b], GO.grouped_sum(tracks[b], GO.partition(tracks[b].shape[0], 16))[0]).all()]
        badpk = [b for b in range(k) if not np.array_equal(pk[b], opks[b][:, :spec.channels])]
        badbus = [b for b in range(k) if spec.n_buses and not np.array_equal(bits(bus[b]), bits(obus[b]))]
        assert not bad and not badpk and not badbus, (seed, bad, badpk, badbus, trail[-6:], spec.block, spec.channels, spec.n_tracks)
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(e.playhead), O.f64_bits(e.sample_position))
    e.close()
    eng.close()


@pytest.mark.parametrize("seed", [220, 270, 312, 426, 546])
def test_bus_sums_of_the_first_long_render_after_a_routing_change(seed):
    """Regression (found by the soak run once the random sessions drew renders of 8 blocks and more): sub-bus sums that
    live in their own buffer are cleared once after a routing change — that memset used to run on the mix stream behind
    the mix, while the sum of a render of >= 8 blocks runs beside on its own stream: it could wipe the bus sums the sum had
    just written.  These seeds (3 sub-buses, random assignment, 8-12 blocks) hit it; the clear now precedes the sum on the
    sum's stream."""
    spec, n_blocks = FZ.random_session(seed)
    assert spec.n_buses == 3 and n_blocks >= 8
    check_against_oracle(spec, n_blocks, expect_exact=True)


@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ2_FROM", "0")), int(os.environ.get("WBX_FUZZ2_TO", "40"))))
def test_random_sessions_grouped_and_callback(seed):
    """The same random sessions with small track groups (several chunks of records, ragged last group: plan rows,
    transport and per-track peaks bit-equal, master inside the RMS budget) and rendered one block per call
    (Engine::process) against the batch render of the same engine configuration: bit-identical."""
    spec, n_blocks = FZ.random_session(seed + 100000)
    gs = [1, 2, 3, 5, 8][seed % 5]
    check_against_oracle(spec, n_blocks, group_size=gs)
    eng = build_engine(spec, max_blocks=n_blocks, group_size=gs)
    eng.play()
    eng.render(n_blocks)
    batch, pk_b, _ = eng.ctx.fetch(peaks=True)
    eng.close()
    eng = build_engine(spec, max_blocks=1, group_size=gs)
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    for b in range(n_blocks):
        eng.process(None, out, float(spec.sample_rate))
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(batch[b])), b
        _, pk, _ = eng.ctx.fetch(peaks=True)
        assert np.array_equal(pk[0], pk_b[b]), b
    eng.close()


def test_track_management_while_playing():
    """Engine::move_track / delete_track / solo_track (engine.cpp:210-262) between blocks of a running transport:
    tracks keep their sequencer and sampler state, only their slots (= the summation order) change; solo goes
    through set_mute.  Master, peaks and transport stay bit-equal to the oracle."""
    spec = synth.make_session("tracks", 30, seek=True, src_rate=44100, n_blocks=16, seed=0x7A)
    e = O.build_oracle_engine(spec)
    eng = build_engine(spec, max_blocks=2)
    e.play()
    eng.play()

    def run(tag):
        oms, opks = [], []
        for _ in range(2):
            om, _ = e.process()
            oms.append(om)
            opks.append(e.peaks())
        eng.render(2)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        assert len(eng.tracks) == e.e.contents.n_tracks, tag
        assert np.array_equal(pk, np.stack(opks)), tag
        assert np.array_equal(bits(m), bits(np.stack(oms))), tag
        ph, sp, _ = eng.transport()
        assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(e.playhead), O.f64_bits(e.sample_position)), tag

    run("start")
    e.move_track(3, 17); eng.move_track(3, 17)
    run("move forward")
    e.move_track(20, 2); eng.move_track(20, 2)
    run("move back")
    e.solo_track(5); eng.solo_track(5)
    run("solo")
    e.solo_track(9); eng.solo_track(9)          # solo moves to another track
    run("solo other")
    e.solo_track(9); eng.solo_track(9)          # un-solo: everything audible again
    run("unsolo")
    e.delete_track(0); eng.delete_track(0)
    e.delete_track(11); eng.delete_track(11)
    run("delete")
    e.set_volume(4, -9.0); eng.tracks[4].set_volume(-9.0)     # indices follow the new slots
    run("param after delete")
    e.close()
    # Engine::clear_all: no tracks left -> silence, and the engine takes new tracks afterwards
    eng.clear_all()
    eng.render(2)
    m, _, _ = eng.ctx.fetch()
    assert not m.any()
    t = eng.add_track("again")
    assert t.index == 0 and len(eng.tracks) == 1
    eng.render(1)
    eng.close()


def test_pipelined_renders_without_host_sync():
    """Twelve renders issued back to back (no fetch, no sync in between): plans, mixes and sums of different renders
    overlap on their three streams and rotate through the ring of plan / partial-sum buffers.  Every render's master
    goes to its own device buffer; after one final sync all 48 blocks must equal the oracle's bit for bit."""
    import torch
    spec = synth.make_session("pipe", 100, seek=True, src_rate=44100, n_blocks=48, seed=0x91E)
    K, R = 4, 12
    om, opk, _, _, otr = run_oracle(spec, K * R)
    eng = build_engine(spec, max_blocks=K)
    n = K * spec.channels * spec.block
    outs = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(R)]
    torch.cuda.synchronize()
    eng.play()
    for r in range(R):
        eng.ctx.set_master_target(outs[r].data_ptr())
        eng.render(K)
    eng.ctx.sync()
    torch.cuda.synchronize()
    got = np.stack([o.cpu().numpy().reshape(K, spec.channels, spec.block) for o in outs]).reshape(K * R, spec.channels, spec.block)
    assert np.array_equal(bits(got), bits(om))
    _, pk, _ = eng.ctx.fetch(peaks=True)            # peaks of the last render
    assert np.array_equal(pk, opk[-K:, :, :spec.channels])
    ph, sp, _ = eng.transport()
    assert (O.f64_bits(ph), O.f64_bits(sp)) == (O.f64_bits(otr[0]), O.f64_bits(otr[1]))
    eng.ctx.set_master_target(None)
    eng.close()


def test_pipelined_renders_large():
    """The same at a size where renders really overlap on the device (2048 tracks, 8 x 32 blocks)."""
    import torch
    spec = synth.make_session("pipeL", 2048, src_rate=44100, n_blocks=256, seed=0x91F)
    K, R = 32, 8
    om, opk, _, _, _ = run_oracle(spec, K * R)
    eng = build_engine(spec, max_blocks=K, device_synth=True)
    n = K * spec.channels * spec.block
    outs = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(R)]
    torch.cuda.synchronize()
    eng.play()
    for r in range(R):
        eng.ctx.set_master_target(outs[r].data_ptr())
        eng.render(K)
    eng.ctx.sync()
    torch.cuda.synchronize()
    got = np.stack([o.cpu().numpy().reshape(K, spec.channels, spec.block) for o in outs]).reshape(K * R, spec.channels, spec.block)
    assert rms(got, om) <= RMS_TOL
    assert np.abs(got - om).max() < 1e-5
    _, em = GO.oracle_model(spec, K * R, GO.render_partition(spec, eng.ctx.render_order(K), 0, K))
    GO.assert_model(got, em, what="pipelined")
    _, pk, _ = eng.ctx.fetch(peaks=True)
    assert np.array_equal(pk, opk[-K:, :, :spec.channels])
    eng.ctx.set_master_target(None)
    eng.close()


def test_set_audio_channel_config_on_a_live_engine():
    """Engine::set_audio_channel_config (engine.cpp:43-57) when the audio backend is reconfigured: new block size, channel
    count and device rate — tracks, clips and samples stay; the next play renders like a fresh engine of that shape."""
    spec = synth.make_session("reconf", 40, seek=True, src_rate=44100, n_blocks=12, seed=0x76)
    eng = build_engine(spec, max_blocks=4)
    eng.play()
    eng.render(4)                                    # state on the device, renders in flight
    for block, channels, rate in ((256, 2, 48000), (1024, 1, 48000), (512, 2, 44100), (512, 2, 48000)):
        eng.stop()
        eng.set_audio_channel_config(0, channels, block, rate)
        sp2 = dataclasses.replace(spec, block=block, channels=channels, sample_rate=rate)
        om, opk, _, orows, otr = run_oracle(sp2, 4)
        eng.play()
        eng.render(4)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        assert plan_rows(eng.fetch_plan()) == orows, (block, channels, rate)
        assert np.array_equal(pk, opk[..., :channels]), (block, channels, rate)
        assert np.array_equal(bits(m), bits(om)), (block, channels, rate)
    eng.close()


@pytest.mark.parametrize("fmt,rates", [("f32", (44100, 48000, 96000)), ("i16", (44100, 48000, 44100)), ("i24", (44100, 48000, 22050))])
def test_rate_change_in_mid_play(fmt, rates):
    """set_audio_channel_config with a new device rate WITHOUT a stop: clips that are playing keep the playback speed their
    sampler was reset with (Sampler::reset_state ran at the old rate, sampler.h:18-27), clips that start afterwards take
    the new one — for a few blocks the session holds rows of both rates (e.g. 16-bit 44.1 kHz clips in a session switched
    from 48 kHz to 44.1 kHz: resampled rows next to unity rows).  The instance / chunk-mode flags must cover both."""
    n_tracks, K = 36, 3
    beat_frames = 48000 * 60.0 / 120.0
    total = 5 * K * 512
    samples, clips, vols, pans = [], [], [], []
    for t in range(n_tracks):
        samples.append(synth.SampleSpec(seed_track=t, channels=2, rate=44100, frames=int(total * 2.3) + 400, fmt=fmt,
                                        amp=0.02 if fmt == "f32" else 1.0))
        v, p = synth.track_params(0x4A7E, t)
        vols.append(float(v) - (0.0 if fmt == "f32" else 30.0))
        pans.append(float(p))
        L = 2.3 * 512
        pos = -((t * 37) % 101) / 101.0 * L
        while pos < total:
            a = max(pos, 0.0)
            clips.append(synth.ClipSpec(t, a / beat_frames, (pos + L) / beat_frames, start_offset=a * 0.9, sample=t))
            pos += L
    spec = synth.SessionSpec(name="ratechg", n_tracks=n_tracks, seed=0x4A7E, samples=samples, clips=clips, volumes_db=vols,
                             pans=pans, mutes=[False] * n_tracks, sample_rate=rates[0])
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    e.play()
    eng = build_engine(spec, max_blocks=K, group_size=n_tracks)
    eng.play()
    for step, rate in enumerate((rates[0], rates[1], rates[1], rates[2], rates[2])):
        e.e.contents.sample_rate = rate
        eng.set_audio_channel_config(0, 2, 512, rate)
        eng.render(K)
        m, pk, _ = eng.ctx.fetch(peaks=True)
        rows = []
        for b in range(K):
            om, _ = e.process()
            rows += oracle_rows(e, b)
            assert np.array_equal(pk[b], e.peaks()[:, :2]), (step, b)
            assert np.array_equal(bits(m[b]), bits(om)), (step, b, rms(m[b], om))
        assert plan_rows(eng.fetch_plan()) == rows, step
    e.close()
    eng.close()


@pytest.mark.parametrize("alt", ["0", "1"])
def test_alternating_mix_streams_keep_every_render_intact(monkeypatch, alt):
    """WBX_MIX_ALT=1: batch renders of layer 2 alternate between two streams so that consecutive mixes overlap; peaks
    live in one buffer per stream.  Twelve renders issued back to back without a host sync, results of each one checked
    (the master through pinned targets, the peaks of the last two through fetch)."""
    from whitebox_amd.dist import PinnedBuffer
    monkeypatch.setenv("WBX_MIX_ALT", alt)
    K, R = 8, 12
    spec = synth.make_session("alt", 70, seek=True, src_rate=44100, n_blocks=K * R, seed=0x77)
    om, opk, _, _, _ = run_oracle(spec, K * R)
    eng = build_engine(spec, max_blocks=K, group_size=70)
    outs = [PinnedBuffer(K * 2 * 512) for _ in range(R)]
    eng.play()
    for r in range(R):
        eng.ctx.set_master_target(outs[r].ptr)
        eng.render(K)
        if r == R - 2:
            _, pk_prev, _ = eng.ctx.fetch(peaks=True)          # joins everything so far
            assert np.array_equal(pk_prev, opk[r * K:(r + 1) * K, :, :2])
    eng.ctx.sync()
    for r in range(R):
        assert np.array_equal(bits(outs[r].array.reshape(K, 2, 512)), bits(om[r * K:(r + 1) * K])), r
    _, pk, _ = eng.ctx.fetch(peaks=True)
    assert np.array_equal(pk, opk[(R - 1) * K:, :, :2])
    assert np.array_equal(eng.levels(), opk.max(axis=0)[:, :2])
    eng.ctx.set_master_target(None)
    for o in outs:
        o.close()
    eng.close()


@pytest.mark.parametrize("clip_blocks", [0.7, 1.3])
def test_callback_mode_with_and_without_queued_pre_render_rows(clip_blocks):
    """Engine::process on an fp32 session leaves the pre-render launch out (clip boundaries stay in the hot loop, the
    queue is expected to be empty) and clears the plan counters in the sum kernel.  Clips shorter than a block put three
    stream calls into some blocks: those are queued after all, and the block is pre-rendered and mixed again — every
    block still equals the oracle's, peaks, levels and stream-call log included."""
    n_blocks = 9
    spec = _boundary_session(30, n_blocks, 512, clip_blocks)
    e = O.build_oracle_engine(spec)
    e.enable_seglog()
    e.play()
    eng = build_engine(spec, max_blocks=1, group_size=30)
    eng.play()
    out = W.AudioBuffer(spec.block, spec.channels)
    lv = np.zeros((30, 2), np.float32)
    for b in range(n_blocks):
        om, _ = e.process()
        eng.process(None, out, float(spec.sample_rate))
        assert np.array_equal(bits(np.stack(out.channel_buffers)), bits(om)), b
        assert plan_rows(eng.fetch_plan()) == oracle_rows(e, 0), b
        _, pk, _ = eng.ctx.fetch(peaks=True)
        assert np.array_equal(pk[0], e.peaks()[:, :2]), b
        lv = np.maximum(lv, e.peaks()[:, :2])
    assert np.array_equal(eng.levels(), lv)
    e.close()
    eng.close()


# WBX_FUZZ4_FROM / WBX_FUZZ4_TO widen the seed range for a soak run (default: seeds 0..59)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ4_FROM", "0")), int(os.environ.get("WBX_FUZZ4_TO", "60"))))
def test_random_masked_row_sessions(seed):
    """Random sessions the masked-row path takes (fuzz_util.random_masked_session): rendered as one batch — peaks, plan,
    transport bit-equal, the master bit-equal when one group holds all tracks — and, every third seed, block by block
    through Engine::process against the same oracle blocks."""
    check_masked_session(*FZ.random_masked_session(seed), seed)


# WBX_FUZZ5_FROM / WBX_FUZZ5_TO widen the seed range for a soak run (default: seeds 0..59)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ5_FROM", "0")), int(os.environ.get("WBX_FUZZ5_TO", "60"))))
def test_random_masked_row_sessions_integer_pcm(seed):
    """The same for sessions of 16 / 24 / 32-bit PCM clips (and fp32 among them) recorded at the session rate: their clip
    boundaries are partial KIND_UNITY_I16 / KIND_UNITY_I32 records in the hot loop (MODE_I16 / MODE_I32 / MODE_MU)."""
    check_masked_session(*FZ.random_masked_session(seed, integer_unity=True), seed)


# WBX_FUZZ6_FROM / WBX_FUZZ6_TO widen the seed range for a soak run (default: seeds 0..59)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ6_FROM", "0")), int(os.environ.get("WBX_FUZZ6_TO", "60"))))
def test_random_masked_row_sessions_16bit_resampled(seed):
    """Sessions of 16-bit PCM only, 44.1 / 48 kHz sources at stretch speeds up to 0.999 or exactly 1: the lean 16-bit family
    (mix_kernel<.., FAM = 2, ..>) with partial KIND_WINDOW_I16 / KIND_UNITY_I16 records in MODE_WI / MODE_WIN / MODE_WINU /
    MODE_I16, the chunks that hold a pre-rendered fp32 row in its one-row-at-a-time mode."""
    check_masked_session(*FZ.random_masked_session(seed, lean16=True), seed)


# WBX_FUZZ7_FROM / WBX_FUZZ7_TO widen the seed range for a soak run (default: seeds 0..59)
@pytest.mark.parametrize("seed", range(int(os.environ.get("WBX_FUZZ7_FROM", "0")), int(os.environ.get("WBX_FUZZ7_TO", "60"))))
def test_random_masked_row_sessions_everything_family(seed):
    """Sessions the everything family (mix_kernel<.., FAM = 1, ..>) serves — resampled 24 / 32-bit PCM, 16-bit resampled
    next to other formats, clips played faster than recorded: their clip boundaries are masked rows of the hot loop too
    (partial KIND_WINDOW / KIND_WINDOW_I16 / KIND_STRIDE / KIND_UNITY_* records in MODE_W / WN / WI / WIN / MW / MWN / G)."""
    check_masked_session(*FZ.random_masked_session(seed, everything=True), seed)


def check_masked_session(spec, n_blocks, seed):
    one_group = spec.n_tracks <= 128
    gs = spec.n_tracks if one_group else [0, 50, 128][seed % 3]
    check_against_oracle(spec, n_blocks, group_size=gs, expect_exact=one_group and not spec.n_buses)
    if seed % 3 == 0:
        om, opk, _, _, _ = run_oracle(spec, n_blocks)
        _, _, tracks = GO.oracle_tracks(spec, n_blocks)
        eng = build_engine(spec, max_blocks=1, group_size=gs)
        eng.play()
        out = W.AudioBuffer(spec.block, spec.channels)
        for b in range(n_blocks):
            eng.process(None, out, float(spec.sample_rate))
            m = np.stack(out.channel_buffers)
            if one_group and not spec.n_buses:
                assert np.array_equal(bits(m), bits(om[b])), b
            else:
                assert rms(m, om[b]) <= RMS_TOL
            GO.assert_grouped(m, tracks[b], GO.group_size_of(spec.n_tracks, gs, 1), spec.n_buses, spec.track_bus, what=("masked", b))
            _, pk, _ = eng.ctx.fetch(peaks=True)
            assert np.array_equal(pk[0], opk[b][:, :spec.channels]), b
        eng.close()



def test_clip_storage_slabs_grow_and_are_reused():
    """Clip audio lives in slabs (64 MiB, 256 MiB, 1 GiB ...) carved up in order: clips that spill over several slabs, a clip
    larger than a quarter slab (an allocation of its own), freeing and uploading again — every clip reads back what was
    uploaded."""
    ctx = W.MixContext(8, max_blocks=1)
    rng = np.random.default_rng(7)
    frames = 3_000_000                                     # 2 channels x 12 MB = 24 MB per clip: three clips fill the first slab
    data = {}
    for clip in range(9):
        data[clip] = [rng.standard_normal(frames).astype(np.float32) for _ in range(2)]
        ctx.clip_upload(clip, "f32", 48000, data[clip])
    big = [rng.integers(-30000, 30000, 80_000_000).astype(np.int16) for _ in range(2)]   # 320 MB: its own allocation
    ctx.clip_upload(9, "i16", 44100, big)
    for clip in (1, 4, 7):                                 # free some, upload others in their place
        st = ctx.L.wbx_clip_free(ctx.h, clip)
        assert st == 0
        data[clip] = [rng.standard_normal(frames // 2).astype(np.float32)]
        ctx.clip_upload(clip, "f32", 44100, data[clip])
    for clip, chans in data.items():
        for ch, a in enumerate(chans):
            assert np.array_equal(ctx.clip_download(clip, ch, len(a), np.float32), a), (clip, ch)
    for ch in range(2):
        assert np.array_equal(ctx.clip_download(9, ch, len(big[ch]), np.int16), big[ch])
    ctx.close()


INSTANCE_CASES = [
    (dict(), 512, "wbx::mix_kernel<4, true, 3, 0, 1, 1, 1, 256>"),                              # fp32 unity, one clip per track
    (dict(src_rate=44100), 512, "wbx::mix_kernel<2, true, 4, 0, 1, 1, 1, 256>"),                # fp32 resampled, one clip per track
    (dict(src_rate=44100, seek=True), 512, "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 128>"),     # ... tracks cut into clips
    (dict(fmt="i16"), 512, "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 128>"),                     # integer PCM at the session rate
    (dict(fmt="i16", src_rate=44100), 512, "wbx::mix_kernel<2, true, 3, 2, 1, 1, 2, 128>"),     # 16-bit only, resampled: the 16-bit family
    (dict(fmt="i24", src_rate=44100), 512, "wbx::mix_kernel<1, true, 3, 3, 1, 1, 2, 128>"),     # resampled 24-bit: everything but per-frame taps
    (dict(fmt="i24", src_rate=44100, seek=True), 256, "wbx::mix_kernel<2, true, 3, 1, 1, 1, 1, 128>"),   # ... cut, 256 frames: a wave per channel
    (dict(fmt="i24", src_rate=44100), 256, "wbx::mix_kernel<2, true, 4, 1, 2, 1, 1, 256>"),     # ... one clip per track: two blocks per workgroup
    (dict(src_rate=44100, seek=True), 128, "wbx::mix_kernel_x<2, 4, 0, 4, 2, 1>"),             # 128-frame blocks, cut: four blocks per workgroup, masked rows
    (dict(src_rate=96000), 512, "wbx::mix_kernel<2, true, 4, 1, 1, 1, 1, 256>"),                # per-frame taps: everything
    (dict(src_rate=44100), 256, "wbx::mix_kernel<2, true, 4, 0, 2, 1, 1, 256>"),                # 256-frame blocks, one clip per track
    (dict(src_rate=44100, seek=True), 256, "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 64>"),      # ... cut: one wave = one block
    (dict(fmt="i16", seek=True), 1024, "wbx::mix_kernel<2, true, 3, 0, 1, 1, 2, 256>"),         # 1024-frame blocks
    (dict(fmt="i16", src_rate=44100, seek=True), 256, "wbx::mix_kernel<2, true, 3, 2, 1, 1, 2, 64>"),    # the 16-bit family at 256 ...
    (dict(fmt="i16", src_rate=44100, seek=True), 1024, "wbx::mix_kernel<2, true, 3, 2, 1, 1, 2, 256>"),  # ... and 1024 frames
]


@pytest.mark.parametrize("kw,block,expect", INSTANCE_CASES,
                         ids=[f"kw{i}-{block}-{instance_id(expect)}" for i, (_, block, expect) in enumerate(INSTANCE_CASES)])
def test_instance_selection(kw, block, expect):
    """Which mix_kernel instance a session takes (wbx_shape.h: choose_shape) — and
    that it renders the session like the oracle."""
    spec = synth.make_session("sel", 40, n_blocks=8, block=block, seed=0x5E1EC7, **kw)
    om, opk, _, _, _ = run_oracle(spec, 8)
    eng = build_engine(spec, max_blocks=8)
    eng.play()
    eng.render(8)
    m, pk, _ = eng.ctx.fetch(peaks=True)
    assert eng.ctx.kernel_name() == expect
    assert np.array_equal(bits(m), bits(om)) and np.array_equal(pk, opk[:, :, :spec.channels])
    eng.close()


@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("block,channels,fmt", [(512, 2, "f32"), (512, 2, "i16"), (256, 2, "f32"), (128, 2, "f32"), (1024, 1, "f32")])
def test_masked_rows_with_the_boundary_at_every_frame(monkeypatch, fast, block, channels, fmt):
    """The clip boundary walks through the block three frames per block (clips of 1 + 3/F blocks, touching or with gaps): over the
    render it sits at every lane position — on a lane's first frame, inside a lane, one frame in front of a wave's end — and the
    calls at block edges are one, two, three frames long (shorter than a lane).  Round 6's cheap form of a masked row (wbx_mix.h
    fast_part: the unmasked arithmetic of a whole-wave call + frame masks, for calls that start >= 4 samples into their clip) and
    the clamped form (WBX_FAST_PARTIAL=0; also what the first clip of every track takes: it opens its sample) both give the
    oracle's stream calls, peaks and master bit for bit."""
    monkeypatch.setenv("WBX_FAST_PARTIAL", fast)
    n_blocks = 200 if block >= 512 else 120
    spec = _boundary_session(24, n_blocks, block, 1.0 + 3.0 / block, channels)
    if fmt != "f32":
        for smp in spec.samples:
            smp.fmt, smp.amp = fmt, 1.0
        spec.volumes_db = [v - 30.0 for v in spec.volumes_db]
    check_against_oracle(spec, n_blocks, group_size=24, expect_exact=True)
