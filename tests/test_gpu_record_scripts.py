"""The recorder's device path — staging slots, chunk table, recorder thread, the gather of stop_record, the clip publish — under
the model's whole script vocabulary: random call sequences (tests/record_scripts.py) run through the product engine, the model
(tests/record_model.py) and the oracle engine side by side; wbx_engine_process_interleaved_in; a take that runs past the chunk
table's 65536 entries; mono sessions, short inputs, the clip pool's accounting, and a take used as the pool clip it is.
Every comparison is bit for bit (uint32 / uint64 views) against the model, the oracle engine or grouped_order.interleaved."""
import time

import numpy as np
import pytest

import bounce_util as BU
import grouped_order as GO
import oracle_ffi as O
import record_model as RM
import record_scripts as RS
import whitebox_amd as W
from whitebox_amd import synth
from whitebox_amd.engine import build_engine
from test_gpu_record import Rig, bits, input_blocks

pytestmark = pytest.mark.gpu

GRANULE = 64 << 10      # the clip pool hands out extents in 64-KiB granules (DESIGN "Clip storage")


def pool_bytes(frames, channels):
    """what a clip of `frames` F32 frames occupies in the pool: rows of frames + the 16 frames of padding, each a multiple of
    256 bytes, the clip a multiple of the granule.  (Clips under 8 granules: no pseudo-random gap in front of them.)"""
    row = -(-(frames + 16) * 4 // 256) * 256
    size = -(-row * channels // GRANULE) * GRANULE
    assert size < 8 * GRANULE
    return size


class ScriptRig(Rig):
    """Rig for inputs that hold NaNs and are played back: the master holds NaN where the oracle's does and the same bits
    everywhere else, and the peaks are compared in every block whose oracle master is free of NaN — the peak of a track-block
    that contains a NaN is the library's one documented deviation (tests/test_gpu_parity.py::test_special_float_values)."""

    def check_block(self, m, om):
        if not np.isnan(om).any():
            return Rig.check_block(self, m, om)
        b = len(self.masters) - 1
        assert np.array_equal(np.isnan(m), np.isnan(om)), ("master NaN", b)
        ok = ~np.isnan(om)
        assert np.array_equal(bits(m)[ok], bits(om)[ok]), ("master", b)


# ---- 1: the model's whole script vocabulary, random scripts ---------------------------------------------------------------
@pytest.mark.parametrize("F,rate,chunk", RS.CONFIGS)
def test_random_scripts_on_the_device(F, rate, chunk):
    """RS.N_SCRIPTS random scripts per configuration (the host-code test runs 65-70 on the CPU).  Even scripts feed NaN
    payloads, +-inf, -0 and subnormals; odd ones audio-range values, so every played-back take is also compared without the
    NaN rule above.  record() reserves every chunk the script can fill, so the recorder thread decides nothing."""
    total, scripts_with = RS.census(F, rate)
    assert total[0] > RS.N_SCRIPTS // 2, "the scripts do make takes"
    all_with = sum(RS.census(f, r)[1] for f, r, _ in RS.CONFIGS)
    assert all_with[1] >= 1 and all_with[2] >= 1 and all_with[3] >= 1, "delete of a recording track / record while playing / block None"
    clips = 0
    for i, script in enumerate(RS.scripts(F)):
        spec = synth.make_session("recscr", script[0][1], n_blocks=40, seed=0x5C00 + i, block=F, sample_rate=rate)
        nb = RS.n_blocks(script)
        max_in = max(RS.max_inputs(script), 1)
        rig = ScriptRig(spec, script[1][1], chunk, spare=(nb * F) // chunk + 4, max_in=max_in,
                        spare_tracks=RS.added_tracks(script), check_now=True, collect=True)
        rig.inputs = input_blocks(np.random.default_rng(F * 1000 + i), nb, max_in, F, special=i % 2 == 0)
        try:
            rig.run(script[2:])
        except AssertionError as ex:
            raise AssertionError((F, i, len(rig.statuses), script[len(rig.statuses)], ex.args)) from ex
        assert rig.statuses == rig.m.statuses, (F, i)
        assert len(rig.made) == len(rig.m.clips) == RS.features(script, F, rate)[0]
        clips += len(rig.made)
        rig.close()
    assert clips == total[0]


# ---- 2: wbx_engine_process_interleaved_in ---------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [512, 480])
def test_interleaved_in_returns_the_oracles_bytes_and_captures_the_take(F):
    """every block leaves through wbx_engine_process_interleaved_in (blocks without an input through _interleaved): the bytes
    are the oracle master's in the device format, a stereo and a mono take per format equal the model's, earlier takes play
    back under the later ones; 512 frames: one launch per block, 480: the three-launch path"""
    spec = synth.make_session("recil", 4, n_blocks=60, seed=0xEC21, block=F)
    rig = Rig(spec, 3, 333, spare=64, check_now=True, collect=True)
    fmts = ("i16", "i24", "i24_x8", "i32", "f32")
    rig.inputs = input_blocks(np.random.default_rng(F + 21), 6 * len(fmts), 3, F, special=False)
    got = []
    rig.run([("input", 1, RM.STEREO, 0, True), ("input", 3, RM.MONO, 2, True)])
    for k, fmt in enumerate(fmts):
        rig.process = lambda inb, fmt=fmt: got.append(
            (fmt, (rig.eng.process_interleaved(fmt) if inb is None else rig.eng.process_interleaved_in(inb, fmt)).view(np.uint8)))
        script = [("playhead", 0.01 * k), ("record",)] + [("block", 6 * k + b) for b in range(6)]
        script += [("stop_record",), ("block", None), ("stop",)]
        rig.run(script)
        assert len(rig.m.clips) == 2 * (k + 1) and all(c["status"] == 0 for c in rig.m.clips)
    assert len(got) == len(rig.oracle_masters) == 7 * len(fmts)
    for b, ((fmt, data), om) in enumerate(zip(got, rig.oracle_masters)):
        assert np.array_equal(data, GO.interleaved(om[None], fmt)), (fmt, b)
    assert rig.statuses == rig.m.statuses
    if F == 512:
        assert rig.eng.callback_stats()[0] == len(got)      # one launch per block
    rig.close()


# ---- 3: overflow with a known set of lost blocks --------------------------------------------------------------------------
def test_a_take_past_the_chunk_table_loses_exactly_the_blocks_the_model_says():
    """Chunks of 3 frames: the chunk table's 65536 entries per take hold 196608 frames.  480-frame blocks 0..408 end at frame
    196319 and fit; block 409 is frames 196320..196799 — its first 288 frames lie in chunks the take has, its last frame in
    chunk 65599, which no take can have: lost whole, as every later block.  Two takes (stereo input 0, mono input 2) have a
    table row each; on the device every take has the same limit, so both lose the same blocks here — a take that loses blocks
    beside one that does not is shown by the model's tests and through record_sim only.

    Why the recorder thread is never the reason a block is lost.  A block is written iff every chunk up to the one of its last
    frame is published (`ready`), and the thread publishes a chunk right after it took it from the pool.  Before every block
    this test waits until wbx_clip_pool_stats shows the bytes of every chunk the thread is to hold by then — the chunks up to
    the block's last frame plus `spare` more, up to the table's limit; the thread fills take after take and chunk after
    chunk, so when the last spare chunk of the last take is in the pool, every chunk the block needs was published before
    it — and then sleeps one block period as test_long_take_grows_without_overflow does (which also covers the few
    microseconds between the pool's count and the publish once the table is full, and leaves the 8 staging slots free).  The
    wait only paces; no expected value comes from it.  Pool use: 2 x 65536 granules = 8 GiB, 3 % of the device's memory."""
    F, chunk, spare, cap, n = 480, 3, 512, 65536, 413
    first_lost = 409
    assert (first_lost * F - 1) // chunk < cap <= (first_lost * F + F - 1) // chunk and first_lost * F // chunk < cap
    spec = synth.make_session("recovf", 2, n_blocks=8, seed=0xEC31, block=F)
    model = RM.RecordModel(F, spec.sample_rate, spec.bpm, chunk=chunk, capacity=cap)
    rig = Rig(spec, 3, chunk, spare, model=model, check_now=True, collect=True)
    rig.inputs = input_blocks(np.random.default_rng(31), n, 3, F, special=False)
    base = rig.eng.ctx.pool_stats()[2]
    rig.run([("input", 0, RM.STEREO, 0, True), ("input", 1, RM.MONO, 2, True), ("playhead", 0.5), ("record",)])
    for b in range(n):
        held = min(-(-(b * F + F) // chunk) + spare, cap)          # chunks per take before block b: rec_chunks_needed
        t0 = time.monotonic()
        while rig.eng.ctx.pool_stats()[2] < base + 2 * held * GRANULE:
            assert time.monotonic() - t0 < 20, ("the recorder thread did not deliver", b, held)
            time.sleep(0.001)
        time.sleep(F / 48000)
        rig.op(("block", b), check=False)
        assert np.array_equal(bits(rig.masters[-1]), bits(rig.oracle_masters[-1])), b
    for t in (0, 1):
        info = rig.eng.record_info(t)
        assert info["recording"] and info["frames"] == n * F and info["status"] == RM.REC_OVERFLOW, info
    rig.op(("stop_record",))            # (check_now: frames, placement with max_time after all 413 blocks, record_info)
    assert rig.statuses[-1] == rig.m.statuses[-1] == -8
    assert rig.statuses == rig.m.statuses and len(rig.made) == 2
    for c, sid in rig.made:
        assert c["blocks"] == list(range(first_lost)) + [None] * (n - first_lost) and c["status"] == RM.REC_OVERFLOW
        for ch in range(c["channels"]):     # (said once more in plain words: exact up to the limit, zero bits from there on)
            got = rig.eng.ctx.clip_download(sid, ch, n * F, np.float32)
            want = np.concatenate([rig.inputs[b][c["ch0"] + ch] for b in range(first_lost)])
            assert np.array_equal(bits(got[:first_lost * F]), bits(want)) and not bits(got[first_lost * F:]).any()
    assert rig.eng.ctx.pool_stats()[2] - base < 64 << 20      # the chunks went back; the two takes stay
    # the clips play back as the oracle plays the model's takes: the seam at the limit and the silence behind it included
    rig.run([("stop",), ("playhead", 0.5), ("play",)])
    for _ in range(n + 2):
        rig.op(("block", None))
    rig.close()


# ---- 4: small cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1024, 480])
def test_mono_session_records_and_plays_back(F):
    """a one-channel session: 1024-frame blocks in the one-launch callback, 480 on the three-launch path; a stereo and a
    mono input recorded, then played back against the oracle"""
    spec = synth.make_session("recmono", 3, n_blocks=30, seed=0xEC41, block=F)
    spec.channels = 1
    rig = Rig(spec, 3, 1000, spare=32, check_now=True, collect=True)
    rig.inputs = input_blocks(np.random.default_rng(F + 41), 8, 3, F, special=False)
    script = [("input", 0, RM.STEREO, 0, True), ("input", 2, RM.MONO, 2, True), ("playhead", 0.05), ("record",)]
    script += [("block", b) for b in range(8)] + [("stop",), ("playhead", 0.0), ("play",)] + [("block", None)] * 12
    rig.run(script)
    assert len(rig.made) == 2 and [c["channels"] for c, _ in rig.made] == [2, 1]
    assert rig.statuses == rig.m.statuses
    if F == 1024:
        assert rig.eng.callback_stats()[0] == 20
    rig.close()


def test_an_input_with_too_few_channels_records_silence():
    """process_in with fewer channels than the takes read (the stereo take reads channels 2-3): the whole block is silence in
    EVERY take — the mono take on channel 0, which the short buffer does hold, included — and WBX_RECORD_SILENCE is set"""
    F = 512
    spec = synth.make_session("recshort", 2, n_blocks=8, seed=0xEC42, block=F)
    rig = Rig(spec, 4, 700, spare=8, check_now=True, collect=True)
    rig.inputs = input_blocks(np.random.default_rng(42), 3, 4, F)
    rig.run([("input", 0, RM.STEREO, 1, True), ("input", 1, RM.MONO, 0, True), ("record",), ("block", 0)])
    short = W.AudioBuffer(F, 3)
    for ch in range(3):
        short.channel_buffers[ch][:] = rig.inputs[1][ch]
    rig.m.run([("block", None)])              # what the model calls a block without (all of) its input
    rig.statuses.append(0)
    rig.eng.process(short, rig.out, float(spec.sample_rate))
    om, _ = rig.e.process()
    assert np.array_equal(bits(np.stack(rig.out.channel_buffers)), bits(om))
    rig.run([("block", 2), ("stop_record",)])
    assert [c["blocks"] for c in rig.m.clips] == [[0, None, 2]] * 2 and all(c["status"] == RM.REC_SILENCE for c in rig.m.clips)
    for c, sid in rig.made:
        got = rig.eng.ctx.clip_download(sid, 0, 3 * F, np.float32)
        assert not bits(got[F:2 * F]).any() and bits(got[:F]).any()
    rig.close()


def test_the_pool_holds_the_published_takes_and_nothing_else():
    """wbx_clip_pool_stats: while takes run bytes_live holds their chunks (one granule per 700-frame chunk: the chunks up to
    the next block's last frame plus the spare ones, per take); deleting a recording track gives its take's chunks back with
    the delete, clear_all mid-take those of every take; after stop_record bytes_live is what it was before record() plus the
    takes' clips (frames + 16 frames of padding per row, granule rounding).  The recorder thread adds chunks on its own
    time, so a figure taken while a take runs is waited for (the thread converges on it) — never read back as an expectation.
    An engine closed with a take running shuts down cleanly; its pool goes with it, so nothing is left to ask: that case
    asserts no byte count."""
    F = 512
    spec = synth.make_session("recpool", 4, n_blocks=8, seed=0xEC43, block=F)
    rig = Rig(spec, 3, 700, spare=6, check_now=True, collect=True)
    rig.inputs = input_blocks(np.random.default_rng(43), 40, 3, F)
    live = lambda: rig.eng.ctx.pool_stats()[2]
    spare, chunk = 6, 700

    def settles_at(want_bytes):
        t0 = time.monotonic()
        while live() != want_bytes and time.monotonic() - t0 < 5:
            time.sleep(0.001)
        # ... and stays there: ten reads over ten periods of the recorder thread's 2-ms sleep (a figure passed on the way
        # to another one does not count)
        for _ in range(10):
            if live() != want_bytes:
                return False
            time.sleep(0.002)
        return live() == want_bytes

    def chunks(written):        # per running take, once the recorder thread has caught up (rec_chunks_needed)
        return -(-(written + F) // chunk) + spare

    base = live()
    rig.run([("input", 0, RM.STEREO, 0, True), ("input", 1, RM.MONO, 2, True), ("input", 3, RM.MONO, 1, True), ("record",)])
    assert settles_at(base + 3 * chunks(0) * GRANULE)
    rig.run([("block", b) for b in range(5)])
    assert settles_at(base + 3 * chunks(5 * F) * GRANULE)
    rig.run([("delete", 1)])
    assert settles_at(base + 2 * chunks(5 * F) * GRANULE), "the deleted track's take gave its chunks back"
    rig.run([("block", b) for b in range(5, 9)])
    assert settles_at(base + 2 * chunks(9 * F) * GRANULE), "and it gets no more"
    rig.run([("stop_record",)])
    assert [(c["track"], c["channels"], len(c["blocks"])) for c in rig.m.clips] == [(0, 2, 9), (2, 1, 9)]
    want = base + pool_bytes(9 * F, 2) + pool_bytes(9 * F, 1)
    assert live() == want                       # the deleted track's take left nothing
    rig.run([("record",)] + [("block", b) for b in range(9, 12)] + [("stop_record",)])
    want += pool_bytes(3 * F, 2) + pool_bytes(3 * F, 1)
    assert live() == want and len(rig.made) == 4
    rig.run([("record",)] + [("block", b) for b in range(12, 20)] + [("clear_all",)])
    assert settles_at(want), "clear_all mid-take: every take's chunks went back"
    rig.run([("block", 20)])
    assert settles_at(want)
    rig.run([("stop_record",)])
    assert len(rig.made) == 4 and live() == want and not rig.eng.is_recording()    # samples stay, no take was added
    assert rig.statuses == rig.m.statuses
    # a take running when the engine goes: the recorder thread is joined and its chunks released (no pool is left to ask)
    rig.run([("tracks", 1), ("input", 0, RM.MONO, 0, True), ("record",), ("block", 21), ("block", 22)])
    assert rig.eng.is_recording() and rig.eng.record_info(0)["frames"] == 2 * F
    rig.close()


def test_a_take_is_an_ordinary_pool_clip():
    """mip-maps of a take against the oracle's summariser; the track that holds it bounced post-fader against the oracle's
    defining sequence (bounce_util); resize_clip from the left and delete_region cut into it, then playback against the
    oracle"""
    F, n = 512, 12
    spec = synth.make_session("recclip", 3, n_blocks=30, seed=0xEC44, block=F)
    rig = Rig(spec, 2, 700, spare=16, check_now=True, collect=True)
    rig.inputs = input_blocks(np.random.default_rng(44), n, 2, F, special=False)
    rig.run([("input", 1, RM.STEREO, 0, True), ("playhead", 0.125), ("record",)] + [("block", b) for b in range(n)] + [("stop",)])
    (c, sid), = rig.made
    audio = RM.take_frames(c, rig.inputs, F)
    eng, e = rig.eng, rig.e
    eng.ctx.build_mipmaps(sid, 1)
    levels = O.oracle_mip_levels(n * F)
    assert levels >= 1 and eng.L.wbx_mip_levels(n * F) == levels
    for lv in range(levels):
        mip = eng.ctx.fetch_mipmap(sid, lv, 2, n * F, 1)
        for ch in range(2):
            assert np.array_equal(mip[ch], O.oracle_mip("f32", audio[ch], lv, 1)), (lv, ch)
    # bounce: a range that starts before the take and ends inside it
    unit = BU.block_beats(F, spec.sample_rate, spec.bpm)
    lo, hi = 0.125 - 2.3 * unit, 0.125 + (n - 1.6) * unit
    frames, want, _, _ = BU.oracle_sequence(e, spec, lo, hi)
    (stem,), got_frames = eng.bounce(lo, hi, [("track", 1, "post")])
    assert got_frames == frames
    assert np.array_equal(bits(eng.bounce_download(stem, frames)), bits(want[1]))
    # edits that cut into the take
    take = [i for i, ci in enumerate(eng.clips(eng.tracks[1])) if ci[5] == sid]
    assert len(take) == 1       # (the clip lists are equal, check_now: the oracle's take has the same index)
    eng.resize_clip(eng.tracks[1], take[0], 3.4 * unit, 0.0, 1.0 / 96.0, True, False, False)
    e.resize_clip(1, take[0], 3.4 * unit, 0.0, 1.0 / 96.0, True, False, False)
    a, b = 0.125 + 6.2 * unit, 0.125 + 8.7 * unit
    eng.delete_region(eng.tracks[1], a, b)
    e.delete_region(1, a, b)
    got = [tuple(O.f64_bits(x) for x in ci[:4]) for ci in eng.clips(eng.tracks[1])]
    assert got == [tuple(O.f64_bits(x) for x in ci[:4]) for ci in e.clips(1)] and len(got) >= 2
    rig.run([("playhead", 0.0), ("play",)] + [("block", None)] * (n + 8))
    rig.close()
