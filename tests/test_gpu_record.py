"""Recording on the device (wbx_engine_record / _stop_record / _process_in, wbx_record.hip): every take bit for bit equal to
tests/record_model.py (the reference's semantics, engine.cpp:95-200, 1638-1649, 1677-1712), its clip placed where the model's
add_audio_clip puts it, the master untouched while recording (no monitoring) and, after stop_record, a take that plays back like
the oracle engine given the model's take through add_sample + add_audio_clip."""
import os
import subprocess
import time

import numpy as np
import pytest

import oracle_ffi as O
import record_model as RM
import whitebox_amd as W
from whitebox_amd import synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE = {RM.NONE: "none", RM.STEREO: "external_stereo", RM.MONO: "external_mono"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def input_blocks(rng, n, channels, F, special=True):
    """[channels][F] blocks of random bit patterns with NaN payloads, +-inf, -0 and subnormals mixed in (special=False: finite
    audio-range values, for takes that are played back)"""
    out = []
    for _ in range(n):
        if special:
            u = rng.integers(0, 2 ** 32, size=(channels, F), dtype=np.uint64).astype(np.uint32)
            pick = rng.integers(0, 8, size=(channels, F))
            u[pick == 0] = 0x7FC01234            # quiet NaN with a payload
            u[pick == 1] = 0xFF800001            # signalling NaN, sign set
            u[pick == 2] = 0x7F800000            # +inf
            u[pick == 3] = 0x80000000            # -0
            u[pick == 4] = rng.integers(1, 0x800000, size=int((pick == 4).sum()), dtype=np.uint64).astype(np.uint32)   # subnormal
            out.append(u.view(np.float32))
        else:
            out.append((rng.standard_normal((channels, F)) * 0.1).astype(np.float32))
    return out


class Rig:
    """One script through the product engine, the model and the oracle engine side by side: every op of record_model.py's
    script language.  `max_in`: the channel count of the buffer every process call hands over (the script's largest input
    count, so that "block i is captured" holds whatever ("inputs", n) says at the time); `model`: a RecordModel made by the
    caller (one with a capacity).  With `check_now` every take is checked the moment it is made — frames, placement, the
    track's whole clip list against the oracle's, record_info — since a later take may trim or replace its clip.  A call the product refuses raises, as every engine call does; with `collect` its
    status is kept instead (`statuses`, one per op, to be compared with the model's)."""

    def __init__(self, spec, n_inputs, chunk, spare, max_in=None, spare_tracks=0, model=None, check_now=False,
                 collect=False):
        self.spec, self.F = spec, spec.block
        self.e = O.build_oracle_engine(spec)
        self.eng = build_engine(spec, max_blocks=1, spare_tracks=spare_tracks)
        self.eng.set_record_chunk(chunk, spare)
        self.eng.set_audio_channel_config(n_inputs, spec.channels, spec.block, spec.sample_rate)
        self.m = model or RM.RecordModel(spec.block, spec.sample_rate, spec.bpm)
        self.m.run([("tracks", spec.n_tracks), ("inputs", n_inputs)])
        self.statuses = [0, 0]  # what the product returned for every call of the script (the two above: the constructor's)
        self.out = W.AudioBuffer(spec.block, spec.channels)
        self.inb = W.AudioBuffer(spec.block, n_inputs if max_in is None else max_in)
        self.inputs = []
        self.made = []          # (model clip, product sample id)
        self.masters, self.oracle_masters = [], []
        self.check_now = check_now
        self.collect = collect  # a call the product refuses: False — the error is raised, True — its status goes into statuses
        self.process = None     # a stand-in for eng.process(inb or None, out): returns the block's master [C][F] or None

    def _oracle_takes(self, before):
        for c in self.m.clips[before:]:
            fr = RM.take_frames(c, self.inputs, self.F)
            data = [np.concatenate([fr[ch], np.zeros(16, np.float32)]) for ch in range(c["channels"])]
            sid = self.e.add_sample("f32", c["channels"], self.spec.sample_rate, fr.shape[1], data)
            self.e.add_audio_clip(c["track"], c["args"][1], c["args"][2], 0.0, sid, 1.0, 1.0)
            # the product's clip: the one on that track whose sample is new
            sids = [ci[5] for ci in self.eng.clips(self.eng.tracks[c["track"]])]
            self.made.append((c, max(sids)))
            if self.check_now:
                self.check_take(c, max(sids))
                info = self.eng.record_info(c["track"])
                assert (info["frames"], info["status"], info["recording"]) == (len(c["blocks"]) * self.F, c["status"], False), \
                    (c["track"], info)
        if self.check_now:
            # every track's clip list is the oracle's after its trimming: no take but the model's was added anywhere
            assert len(self.eng.tracks) == len(self.m.tracks)
            for t in range(len(self.eng.tracks)):
                got = [tuple(O.f64_bits(x) for x in ci[:4]) + (np.float32(ci[4]),) for ci in self.eng.clips(self.eng.tracks[t])]
                want = [tuple(O.f64_bits(x) for x in ci[:4]) + (np.float32(ci[4]),) for ci in self.e.clips(t)]
                assert got == want, ("clip list", t)

    def _call(self, fn, *args):
        try:
            fn(*args)
        except W.WbxError as ex:
            if not self.collect:
                raise
            return ex.status
        return 0

    def op(self, op, block=None, check=True):
        k = op[0]
        was_rec_playing = self.m.recording and self.m.playing
        n_clips = len(self.m.clips)
        self.m.run([op])
        st = 0
        if k == "tracks":
            for _ in range(op[1]):
                st = st or self._call(self.eng.add_track)
                self.e.add_track()
        elif k == "inputs":     # the input count alone: set_audio_channel_config reconfigures the output, refused in a take
            st = W.lib().wbx_engine_set_input_channels(self.eng.h, op[1])
            assert st == 0 or self.collect, st
        elif k == "delete":
            st = self._call(self.eng.delete_track, op[1])
            if st == 0:
                self.e.delete_track(op[1])
        elif k == "clear_all":
            st = self._call(self.eng.clear_all)
            for slot in range(self.e.e.contents.n_tracks - 1, -1, -1):
                self.e.delete_track(slot)
        elif k == "input":
            st = self._call(self.eng.set_track_input, op[1], TYPE[op[2]], op[3], op[4])
        elif k == "arm":
            st = self._call(self.eng.arm_track_recording, op[1], op[2])
        elif k == "record":
            st = self._call(self.eng.record)
            if st == 0 and not was_rec_playing:
                self.e.play()       # record() -> play() (engine.cpp:102)
        elif k == "play":
            st = self._call(self.eng.play)
            self.e.play()
        elif k == "stop":
            st = self._call(self.eng.stop)
            self._oracle_takes(n_clips)
            self.e.stop()
        elif k == "stop_record":
            st = self._call(self.eng.stop_record)      # (-8: a take lost blocks; its clip is made all the same)
            self._oracle_takes(n_clips)
        elif k == "bpm":
            st = self._call(self.eng.set_bpm, op[1])
            self.e.set_bpm(op[1])
        elif k == "playhead":
            st = self._call(self.eng.set_playhead_position, op[1])
            self.e.set_playhead(op[1])
        elif k == "block":
            inb = None
            if op[1] is not None:
                for ch in range(self.inb.n_channels):
                    self.inb.channel_buffers[ch][:] = self.inputs[op[1]][ch]
                inb = self.inb
            if self.process is not None:
                m = self.process(inb)
            else:
                self.eng.process(inb, self.out, float(self.spec.sample_rate))
                m = np.stack(self.out.channel_buffers)
            om, _ = self.e.process()
            self.oracle_masters.append(om)
            if m is not None:       # (None: the stand-in kept the block in its own format)
                self.masters.append(m.copy())
                if check:
                    self.check_block(m, om)
        else:
            raise ValueError(op)
        self.statuses.append(st)

    def check_block(self, m, om):
        b = len(self.masters) - 1
        assert np.array_equal(bits(m), bits(om)), ("master", b)
        if len(self.eng.tracks):
            _, pk, _ = self.eng.ctx.fetch(peaks=True)
            assert np.array_equal(pk[0], self.e.peaks()[:, :self.spec.channels]), ("peaks", b)

    def run(self, script, check=True):
        for op in script:
            self.op(op, check=check)

    def check_take(self, c, sid):
        """the take equals the model's frames bit for bit, and its clip sits where the model's add_audio_clip put it"""
        want = RM.take_frames(c, self.inputs, self.F)
        for ch in range(c["channels"]):
            got = self.eng.ctx.clip_download(sid, ch, want.shape[1], np.float32)
            assert np.array_equal(bits(got), bits(want[ch])), (c["track"], ch)
        infos = [ci for ci in self.eng.clips(self.eng.tracks[c["track"]]) if ci[5] == sid]
        assert len(infos) == 1
        mn, mx, so, spd, g, _ = infos[0]
        t, wmn, wmx, wso, wspd, wg = c["args"]
        assert (O.f64_bits(mn), O.f64_bits(mx), O.f64_bits(so), O.f64_bits(spd), np.float32(g)) == \
            (O.f64_bits(wmn), O.f64_bits(wmx), O.f64_bits(wso), O.f64_bits(wspd), np.float32(wg))

    def check_takes(self):
        """every take of the script, at its end (scripts whose takes do not cut into each other)"""
        assert len(self.made) == len(self.m.clips)
        for c, sid in self.made:
            self.check_take(c, sid)

    def close(self):
        self.eng.close()
        self.e.close()


def capture_script(n_blocks, bpm_change_at):
    """4 of 6 tracks record: mono input 3, stereo input 1 (channels 2-3) on two tracks, mono input 0; tempo change mid-take"""
    s = [("input", 0, RM.MONO, 3, True), ("input", 1, RM.STEREO, 1, True), ("input", 2, RM.STEREO, 1, True),
         ("input", 4, RM.MONO, 0, True), ("input", 5, RM.MONO, 2, False), ("playhead", 0.25), ("record",)]
    for b in range(n_blocks):
        if b == bpm_change_at:
            s.append(("bpm", 97.5))
        s.append(("block", b))
    return s + [("stop_record",)]


@pytest.mark.parametrize("F,chunk", [(512, 100), (512, 700), (480, 333), (128, 48), (128, 200)])
def test_takes_are_exact_placed_exactly_and_not_monitored(F, chunk):
    """1-3: takes bit for bit (NaN payloads, inf, -0, subnormals; chunks smaller than and not a multiple of F), their clips'
    placement as fp64 bit patterns across a tempo change, and masters + peaks of every block equal to the oracle's."""
    spec = synth.make_session("rec", 6, n_blocks=20, seed=0xEC01, block=F)
    n_blocks = 14
    rig = Rig(spec, 4, chunk, spare=(n_blocks * F) // chunk + 4)   # every chunk reserved by record(): no race with the thread
    rig.inputs = input_blocks(np.random.default_rng(F + chunk), n_blocks, 4, F)
    rig.run(capture_script(n_blocks, 6))
    assert len(rig.m.clips) == 4
    rig.check_takes()
    for t in (0, 1, 2, 4):
        info = rig.eng.record_info(t)
        assert info["frames"] == n_blocks * F and info["status"] == 0 and not info["recording"]
    rig.close()


@pytest.mark.parametrize("F", [512, 128])
def test_take_plays_back_like_the_oracle_with_the_model_take(F):
    """4: after stop_record the take is a clip on its track — trimming the clips it overlaps — and playing from the start
    mixes exactly what the oracle mixes with the model's take added through add_sample + add_audio_clip."""
    spec = synth.make_session("recplay", 5, n_blocks=24, seed=0xEC02, block=F, seek=True)
    rig = Rig(spec, 2, 1000, spare=64)
    rig.inputs = input_blocks(np.random.default_rng(7), 10, 2, F, special=False)
    script = [("input", 1, RM.STEREO, 0, True), ("input", 3, RM.MONO, 1, True), ("playhead", 0.1), ("play",),
              ("block", None), ("record",)] + [("block", b) for b in range(10)] + [("stop_record",), ("block", None),
                                                                                  ("stop",), ("playhead", 0.0), ("play",)]
    script += [("block", None)] * 18
    rig.run(script)
    rig.check_takes()
    n1 = len(rig.eng.clips(rig.eng.tracks[1]))
    assert n1 == len(rig.e.clips(1)) and n1 >= 2     # the take split / trimmed the track's own clip(s) as the oracle's did
    rig.close()


def test_give_up_path_captures_each_block_once(monkeypatch):
    """5: a block mixed again after a give-up at the spread barrier (the recipe of test_gpu_callback.py) is captured once."""
    monkeypatch.setenv("WBX_CB_SPIN_BOUND", "0")
    spec = synth.make_session("recgu", 300, src_rate=44100, n_blocks=8, seed=0xC5B2)
    rig = Rig(spec, 2, 512, spare=16)
    rig.inputs = input_blocks(np.random.default_rng(3), 5, 2, 512)
    rig.run([("input", 7, RM.STEREO, 0, True), ("record",)] + [("block", b) for b in range(5)] + [("stop_record",)],
            check=False)
    launches, spread, give_ups, off = rig.eng.callback_stats()
    assert give_ups == 1 and launches == 5
    rig.check_takes()
    assert rig.eng.record_info(7)["frames"] == 5 * 512
    rig.close()


def test_one_launch_and_three_launch_paths_capture_each_block_once():
    """5: the one-launch callback (512-frame stereo) and the three-launch path (480 frames) both capture every block once."""
    for F in (512, 480):
        spec = synth.make_session("recpath", 4, n_blocks=8, seed=0xEC05, block=F)
        rig = Rig(spec, 1, 4096, spare=4)
        rig.inputs = input_blocks(np.random.default_rng(F), 6, 1, F)
        rig.run([("input", 2, RM.MONO, 0, True), ("record",)] + [("block", b) for b in range(6)] + [("stop",)])
        launches = rig.eng.callback_stats()[0]
        assert (launches == 6) if F == 512 else True
        rig.check_takes()
        assert rig.eng.record_info(2)["frames"] == 6 * F
        rig.close()


def test_long_take_grows_without_overflow():
    """6: a take 40 chunks long, the recorder thread one spare chunk ahead, blocks paced like an audio callback"""
    spec = synth.make_session("recgrow", 2, n_blocks=4, seed=0xEC06)
    rig = Rig(spec, 2, 1024, spare=1)
    n = 80
    rig.inputs = input_blocks(np.random.default_rng(11), n, 2, 512)
    rig.run([("input", 0, RM.STEREO, 0, True), ("input", 1, RM.MONO, 1, True), ("record",)])
    for b in range(n):
        rig.op(("block", b), check=False)
        time.sleep(512 / 48000)
    rig.op(("stop_record",))
    for t in (0, 1):
        info = rig.eng.record_info(t)
        assert info["status"] == 0 and info["frames"] == n * 512, info
    rig.check_takes()
    rig.close()


def test_refusals_and_silence():
    """6: render during a take, record on a redirected master, MIDI inputs and inputs past the channel count are refused;
    process calls without an input record silence and say so in the take's status."""
    spec = synth.make_session("recref", 2, n_blocks=6, seed=0xEC07)
    eng = build_engine(spec, max_blocks=4)
    eng.set_audio_channel_config(2, spec.channels, spec.block, spec.sample_rate)
    with pytest.raises(W.WbxError) as ex:
        eng.set_track_input(0, "midi", 0, True)
    assert ex.value.status == -3
    eng.set_track_input(0, "external_stereo", 1, True)     # channels 2-3 of 2
    with pytest.raises(W.WbxError) as ex:
        eng.record()
    assert ex.value.status == -4 and not eng.is_recording()
    eng.set_track_input(0, "external_mono", 1, True)
    p = W.lib()
    buf = __import__("ctypes").c_void_p()
    assert p.wbx_host_alloc(4 * spec.block * spec.channels * 4, __import__("ctypes").byref(buf)) == 0
    eng.ctx.set_master_target(buf.value)
    with pytest.raises(W.WbxError) as ex:
        eng.record()
    assert ex.value.status == -3
    eng.ctx.set_master_target(None)
    assert p.wbx_host_free(buf) == 0
    eng.record()
    assert eng.is_recording()
    with pytest.raises(W.WbxError) as ex:
        eng.render(2)
    assert ex.value.status == -3
    out = W.AudioBuffer(spec.block, spec.channels)
    for _ in range(3):
        eng.process(None, out, float(spec.sample_rate))
    info = eng.record_info(0)
    assert info["recording"] and info["frames"] == 3 * spec.block and info["status"] == RM.REC_SILENCE
    eng.stop_record()
    clips = eng.clips(eng.tracks[0])
    sid = max(c[5] for c in clips)
    got = eng.ctx.clip_download(sid, 0, 3 * spec.block, np.float32)
    assert not np.any(bits(got))
    eng.close()


def test_null_arguments_are_refused():
    L = W.lib()
    assert L.wbx_engine_record(None) == -4 and L.wbx_engine_stop_record(None) == -4
    assert L.wbx_engine_is_recording(None, None) == -4 and L.wbx_engine_set_input_channels(None, 2) == -4
    assert L.wbx_track_set_input(None, 0, 3, 0, 1) == -4 and L.wbx_engine_arm_track_recording(None, 0, 1) == -4
    assert L.wbx_engine_record_info(None, 0, None) == -4 and L.wbx_engine_set_record_chunk(None, 512, 1) == -4
    assert L.wbx_engine_process_in(None, None, 0, None) == -4
    assert L.wbx_engine_process_interleaved_in(None, None, 0, 9, None) == -4


def test_cpp_adapter_records_through_process(tmp_path):
    """7: a C++ host on include/wbx_adapter.hpp arms two tracks, records through wbx::Engine::process(input, output, sr),
    stops, and writes each take; they equal the model's takes."""
    exe = str(tmp_path / "adapter_record")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "adapter_record.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    dump = str(tmp_path / "takes.bin")
    out = subprocess.check_output([exe, dump], timeout=300).decode()
    assert "adapter record ok" in out, out
    F, NB = 512, 9
    # the adapter program's input: block b, channel c, frame i = (b * 4 + c) * 1000 + i, as float32
    inputs = [np.array([[(b * 4 + c) * 1000 + i for i in range(F)] for c in range(4)], dtype=np.float32) for b in range(NB)]
    script = [("tracks", 3), ("inputs", 4), ("input", 0, RM.STEREO, 1, True), ("input", 2, RM.MONO, 0, True), ("record",)]
    script += [("block", b) for b in range(NB)] + [("stop_record",)]
    clips = RM.run(script, F, 48000, 120.0)
    raw = np.fromfile(dump, dtype=np.float32)
    at = 0
    for c in clips:
        want = RM.take_frames(c, inputs, F)
        got = raw[at:at + want.size].reshape(want.shape)
        at += want.size
        assert np.array_equal(bits(got), bits(want)), c["track"]
    assert at == raw.size
    meta = [ln.split() for ln in out.splitlines() if ln.startswith("clip")]
    assert [(int(w[1]), float.fromhex(w[2]), float.fromhex(w[3])) for w in meta] == \
        [(c["track"], c["args"][1], c["args"][2]) for c in clips]
