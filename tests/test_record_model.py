"""Recording without a device: tests/record_model.py (the reference's semantics in plain Python) on hand-checked cases,
and the product's host-session record code (wbx_host.h compiled with g++ into tests/cpp/record_sim.cpp) against the model
on random call sequences, record_min_time / record_max_time compared bit for bit."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import record_model as RM
import record_scripts as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, SR = 512, 48000
BEATS = lambda bpm: (F / SR) / (60.0 / bpm)   # buffer_duration_in_beats of one block


def chain(x0, steps):
    """x0 + s0 + s1 + ... added one by one, as record_max_time is"""
    for s in steps:
        x0 += s
    return x0


# ---- hand-checked cases -------------------------------------------------------------------------------------------------

def test_mono_and_stereo_inputs_past_index_zero():
    clips = RM.run([("tracks", 3), ("inputs", 6), ("input", 0, RM.MONO, 3, True), ("input", 1, RM.STEREO, 2, True),
                    ("input", 2, RM.STEREO, 1, False), ("record",), ("block", 0), ("block", 1), ("stop_record",)])
    assert [(c["track"], c["ch0"], c["channels"]) for c in clips] == [(0, 3, 1), (1, 4, 2)]
    inputs = [np.arange(6 * F, dtype=np.float32).reshape(6, F) + 10000 * i for i in range(2)]
    fr = RM.take_frames(clips[1], inputs, F)
    assert fr.shape == (2, 2 * F)
    assert np.array_equal(fr[:, :F], inputs[0][4:6]) and np.array_equal(fr[:, F:], inputs[1][4:6])
    assert np.array_equal(RM.take_frames(clips[0], inputs, F)[0, F:], inputs[1][3])
    b = BEATS(120.0)
    assert clips[0]["args"] == (0, 0.0, chain(0.0, [b, b]), 0.0, 1.0, 1.0)


def test_stereo_index_past_the_input_count_is_refused():
    m = RM.RecordModel()
    m.run([("tracks", 1), ("inputs", 3), ("input", 0, RM.STEREO, 1, True), ("record",)])
    assert m.statuses[-1] == RM.INVALID and not m.recording
    assert RM.RecordModel().run([("tracks", 1), ("input", 0, RM.MIDI, 0, True)]) == []


def test_tempo_change_mid_take_changes_the_step():
    clips = RM.run([("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("playhead", 2.0), ("record",),
                    ("block", 0), ("bpm", 90.0), ("block", 1), ("block", 2), ("stop_record",)])
    want = chain(2.0, [BEATS(120.0), BEATS(90.0), BEATS(90.0)])
    assert clips[0]["args"] == (0, 2.0, want, 0.0, 1.0, 1.0)
    assert BEATS(120.0) == 0.021333333333333333 and BEATS(90.0) == 0.016


def test_two_tracks_on_one_input_get_a_copy_each():
    clips = RM.run([("tracks", 2), ("inputs", 2), ("input", 0, RM.STEREO, 0, True), ("input", 1, RM.STEREO, 0, True),
                    ("record",), ("block", 0), ("block", None), ("stop_record",)])
    assert [c["track"] for c in clips] == [0, 1]
    assert clips[0]["blocks"] == clips[1]["blocks"] == [0, None]
    assert clips[0]["status"] == RM.REC_SILENCE


def test_record_while_playing_restarts_the_take_at_playhead_start():
    m = RM.RecordModel()
    clips = m.run([("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("playhead", 4.0), ("play",),
                   ("block", 0), ("block", 1), ("record",), ("block", 2), ("record",), ("block", 3), ("stop_record",)])
    # the take starts at playhead_start, not where the transport was; the second record() while recording does nothing
    assert clips[0]["args"][1] == 4.0 and clips[0]["blocks"] == [2, 3]
    assert clips[0]["args"][2] == chain(4.0, [BEATS(120.0)] * 2)
    assert m.playing and not m.recording   # stop_record leaves playback running


def test_stop_during_a_take_makes_the_clip_first():
    m = RM.RecordModel()
    clips = m.run([("tracks", 2), ("inputs", 2), ("input", 1, RM.MONO, 1, True), ("record",), ("block", 0), ("stop",),
                   ("block", 1)])
    assert len(clips) == 1 and clips[0]["track"] == 1 and clips[0]["blocks"] == [0]
    assert not m.playing and not m.recording


def test_arm_changes_wait_for_the_next_record_and_deleted_tracks_lose_their_take():
    clips = RM.run([("tracks", 3), ("inputs", 2), ("input", 0, RM.MONO, 0, True), ("input", 2, RM.MONO, 1, True),
                    ("record",), ("block", 0), ("input", 1, RM.MONO, 0, True), ("arm", 0, False), ("play",), ("block", 1),
                    ("delete", 2), ("block", 2), ("stop_record",)])
    assert [c["track"] for c in clips] == [0]
    assert clips[0]["blocks"] == [0, 1, 2]
    assert clips[0]["args"][1:3] == (0.0, chain(0.0, [BEATS(120.0)] * 2))   # play() prepared the take again


def test_a_block_whose_last_frame_has_no_chunk_is_lost_whole():
    """chunks of 700 frames, 3 of them: frames 0..2099 have room.  512-frame blocks 0-3 end at frame 2047 (chunk 2) and fit;
    block 4 is frames 2048..2559: its first 52 frames lie in chunk 2, its last frame in chunk 3, which the take does not
    have — the whole block is lost, and so is every later one."""
    m = RM.RecordModel(F, SR, 120.0, chunk=700, capacity=3)
    script = [("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("playhead", 1.0), ("record",)]
    script += [("block", b) for b in range(7)] + [("stop_record",)]
    clips = m.run(script)
    assert m.statuses[-1] == RM.OVERFLOW == -8 and len(clips) == 1
    assert clips[0]["blocks"] == [0, 1, 2, 3, None, None, None]
    assert clips[0]["status"] == RM.REC_OVERFLOW          # lost blocks are not "no input" blocks
    assert clips[0]["args"] == (0, 1.0, chain(1.0, [BEATS(120.0)] * 7), 0.0, 1.0, 1.0)   # max_time advanced 7 times
    inputs = [np.full((1, F), b + 1, np.float32) for b in range(7)]
    fr = RM.take_frames(clips[0], inputs, F)
    assert fr.shape == (1, 7 * F)
    assert np.array_equal(fr[0, :4 * F], np.repeat(np.arange(1, 5, dtype=np.float32), F)) and not fr[0, 4 * F:].any()


def test_a_block_that_ends_on_the_last_frame_of_the_last_chunk_fits():
    # 4 chunks of 256 frames = 1024 frames = exactly two 512-frame blocks; the third is lost; 5 chunks of 205 = 1025 frames
    # hold two blocks as well (the third block's last frame, 1535, is in chunk 7)
    for chunk, cap in ((256, 4), (205, 5)):
        m = RM.RecordModel(F, SR, 120.0, chunk=chunk, capacity=cap)
        clips = m.run([("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("record",), ("block", 0), ("block", 1),
                       ("block", 2), ("stop",)])
        assert clips[0]["blocks"] == [0, 1, None] and clips[0]["status"] == RM.REC_OVERFLOW
    # one frame less room and the second block goes too; no capacity, or one that is never reached, loses nothing
    assert RM.run([("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("record",), ("block", 0), ("block", 1),
                   ("stop_record",)], chunk=1023, capacity=1)[0]["blocks"] == [0, None]
    m = RM.RecordModel(F, SR, 120.0, chunk=100, capacity=11)
    clips = m.run([("tracks", 1), ("inputs", 1), ("input", 0, RM.MONO, 0, True), ("record",), ("block", 0), ("block", None),
                   ("stop_record",)])
    assert clips[0]["blocks"] == [0, None] and clips[0]["status"] == RM.REC_SILENCE and m.statuses[-1] == RM.OK


def test_every_take_is_judged_by_its_own_capacity():
    """two takes of one record(): the first has 2 chunks of 600 frames (two blocks and 176 frames of a third), the second
    has room; a "no input" block after the limit sets REC_SILENCE on both; a later record() starts with empty takes"""
    m = RM.RecordModel(F, SR, 120.0, chunk=600, capacity=[2, None])
    script = [("tracks", 2), ("inputs", 3), ("input", 0, RM.STEREO, 0, True), ("input", 1, RM.MONO, 2, True), ("record",),
              ("block", 0), ("block", 1), ("block", 2), ("block", None), ("stop_record",), ("record",), ("block", 4),
              ("stop_record",)]
    clips = m.run(script)
    assert [(c["track"], c["blocks"], c["status"]) for c in clips] == [
        (0, [0, 1, None, None], RM.REC_OVERFLOW | RM.REC_SILENCE), (1, [0, 1, 2, None], RM.REC_SILENCE),
        (0, [4], 0), (1, [4], 0)]
    assert m.statuses[9] == RM.OVERFLOW and m.statuses[-1] == RM.OK
    assert clips[0]["args"][2] == clips[1]["args"][2] == chain(0.0, [BEATS(120.0)] * 4)


def test_a_deleted_tracks_take_does_not_turn_stop_record_into_an_overflow():
    m = RM.RecordModel(F, SR, 120.0, chunk=512, capacity=[1, None])
    clips = m.run([("tracks", 2), ("inputs", 2), ("input", 0, RM.MONO, 0, True), ("input", 1, RM.MONO, 1, True), ("record",),
                   ("block", 0), ("delete", 0), ("block", 1), ("stop_record",)])
    assert [(c["track"], c["blocks"], c["status"]) for c in clips] == [(0, [0, 1], 0)] and m.statuses[-1] == RM.OK


def test_the_device_scripts_do_something():
    """the random scripts the device runs (tests/record_scripts.py): more clips than half the scripts in every configuration,
    and among them a delete of a recording track, a record() that restarts a playing transport and an input-less block in a take"""
    with_feature = np.zeros(4, dtype=int)
    for block_frames, rate, chunk in RS.CONFIGS:
        assert chunk % block_frames and block_frames % chunk
        total, scripts_with = RS.census(block_frames, rate)
        assert total[0] > RS.N_SCRIPTS // 2
        with_feature += scripts_with
    assert (with_feature[1:] >= 1).all(), with_feature


# ---- the product's host code against the model -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def record_sim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("record_sim") / "record_sim")
    subprocess.check_call([cxx, "-std=c++20", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "record_sim.cpp"),
                           "-o", exe, "-lpthread"])
    return exe


def _script_text(script, block_frames, rate, chunk=None, capacity=None):
    lines = [f"frames {block_frames}", f"rate {rate}"]
    if capacity is not None:
        lines += [f"chunk {chunk}", f"capacity {capacity}"]
    for op in script:
        k = op[0]
        if k == "block":
            lines.append(f"block {-1 if op[1] is None else op[1]}")
        elif k in ("bpm", "playhead"):
            lines.append(f"{k} {op[1]!r}")
        else:
            lines.append(" ".join([k] + [str(int(a)) for a in op[1:]]))
    return "\n".join(lines) + "\n"


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def run_sim(exe, script, block_frames=F, rate=SR, chunk=None, capacity=None):
    r = subprocess.run([exe], input=_script_text(script, block_frames, rate, chunk, capacity), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    statuses, clips = [], []
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "status":
            statuses.append(int(w[1]))
        else:
            n = int(w[7])
            clips.append(dict(track=int(w[1]), min_bits=int(w[2], 16), max_bits=int(w[3], 16), ch0=int(w[4]),
                              channels=int(w[5]), status=int(w[6]), blocks=[None if int(b) < 0 else int(b) for b in w[8:8 + n]]))
    return statuses, clips


def compare(exe, script, block_frames=F, rate=SR, chunk=None, capacity=None):
    m = RM.RecordModel(block_frames, rate) if capacity is None else RM.RecordModel(block_frames, rate, 120.0, chunk, capacity)
    want = m.run(script)
    statuses, got = run_sim(exe, script, block_frames, rate, chunk, capacity)
    assert statuses == m.statuses
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["track"], g["ch0"], g["channels"], g["status"], g["blocks"]) == \
            (w["track"], w["ch0"], w["channels"], w["status"], w["blocks"])
        assert g["min_bits"] == _bits(w["args"][1]) and g["max_bits"] == _bits(w["args"][2])
    return len(want)


def test_host_code_matches_the_hand_checked_cases(record_sim):
    compare(record_sim, [("tracks", 2), ("inputs", 4), ("input", 0, RM.MONO, 3, True), ("input", 1, RM.STEREO, 1, True),
                         ("playhead", 1.5), ("record",), ("block", 0), ("bpm", 133.7), ("block", None), ("block", 2),
                         ("record",), ("play",), ("block", 3), ("stop",)])


@pytest.mark.parametrize("block_frames,rate,chunk,capacity", [(512, 48000, 700, 3), (480, 48000, 333, 7), (128, 44100, 64, 9),
                                                              (512, 48000, 256, 4)])
def test_host_code_carries_an_overflow_like_the_model(record_sim, block_frames, rate, chunk, capacity):
    """the overflow extension through the product's host session: lost blocks, the latched status, frames and record_max_time
    still advancing, stop_record's -8 with the clip made — a hand-written take past its capacity and 25 random scripts"""
    script = [("tracks", 2), ("inputs", 4), ("input", 0, RM.MONO, 3, True), ("input", 1, RM.STEREO, 0, True), ("record",)]
    script += [("block", b) for b in range(12)] + [("bpm", 90.0), ("block", None), ("stop_record",), ("record",), ("block", 13),
                                                   ("stop",)]
    m = RM.RecordModel(block_frames, rate, 120.0, chunk, capacity)
    clips = m.run(script)
    assert RM.OVERFLOW in m.statuses and all(c["status"] & RM.REC_OVERFLOW for c in clips[:2]) and clips[2]["status"] == 0
    compare(record_sim, script, block_frames, rate, chunk, capacity)
    rng = np.random.default_rng(0x0F10 + chunk)
    overflows = 0
    for _ in range(25):
        script = RM.random_script(rng)
        m = RM.RecordModel(block_frames, rate, 120.0, chunk, capacity)
        overflows += any(c["status"] & RM.REC_OVERFLOW for c in m.run(script))
        compare(record_sim, script, block_frames, rate, chunk, capacity)
    assert overflows >= 3   # the random takes do run past the capacity


@pytest.mark.parametrize("block_frames,rate", [(512, 48000), (128, 44100), (480, 48000)])
def test_host_code_matches_the_model_on_random_scripts(record_sim, block_frames, rate):
    rng = np.random.default_rng(0x5EC0 + block_frames)
    clips = 0
    n = 70 if block_frames == 512 else 65
    for _ in range(n):
        clips += compare(record_sim, RM.random_script(rng), block_frames, rate)
    assert clips > n // 2   # the scripts do make takes
