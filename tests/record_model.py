"""The reference's recording semantics restated in plain Python (no engine code): Engine::record / stop_record /
arm_track_recording / set_track_input (src/engine/engine.cpp:95-200), Engine::play / stop (:68-93), Track::prepare_record /
stop_record (track.cpp:234-246), the record_max_time steps of Track::process_event (track.cpp:281, 342, 448: one
`record_max_time += buffer_duration_in_beats` per played block) and the recorder tap of Engine::process (engine.cpp:1638-1649:
ExternalMono index i records input channel i, ExternalStereo index i channels 2i and 2i+1; every track of an input gets its own
copy, write_recorded_samples_ :1677-1697).

Where the reference is undefined the library's documented choices (DESIGN.md "Recording") are restated:
  * the take list is every armed track with an input at record(); input / arm edits during a take wait for the next record()
    (play() during a take prepares the tracks of the running take only);
  * a process call without an input records silence (status REC_SILENCE);
  * deleting a recording track (or clear_all) discards its take; a take of no frames adds no clip;
  * record() with an input past the configured input channel count is refused (INVALID), MIDI inputs are refused;
  * take storage is chunks of `chunk` frames and a take holds at most `capacity` of them (wbx_engine_set_record_chunk; the
    chunk table's 65536 entries per take on the device): a block whose LAST frame lies in a chunk the take does not have is
    lost whole — also its frames that lie in a chunk the take has —, it reads as silence, REC_OVERFLOW is latched, the frame
    count and record_max_time advance as for any block, and stop_record returns OVERFLOW (-8) with the clip still made.
    `capacity` is one number for every take or a list by position in the take list of a record() (None: no limit).

A script is a list of tuples:
    ("tracks", n)                 n new tracks                 ("delete", slot) / ("clear_all",)
    ("inputs", n)                 input channel count           ("bpm", bpm) / ("playhead", beat)
    ("input", slot, type, index, armed)                         ("arm", slot, armed)
    ("record",) ("stop_record",) ("play",) ("stop",)
    ("block", i)                  one process call whose input is block i of the caller's input list
    ("block", None)               one process call without an input
run() returns the clips stop_record makes, in order: dict(track, args, blocks, ch0, channels, status) where args are the exact
add_audio_clip arguments (track, min_time, max_time, start_offset 0.0, speed 1.0, gain 1.0) and blocks the input block index
(None: silence, a lost block included) of every F frames of the take; take_frames() turns that into the take's samples.
"""
from __future__ import annotations

import numpy as np

NONE, MIDI, STEREO, MONO = 0, 1, 2, 3          # TrackInputType, track_input.h:10-15
REC_OVERFLOW, REC_SILENCE = 1, 2
OK, UNSUPPORTED, INVALID, OVERFLOW = 0, -3, -4, -8


class _Track:
    def __init__(self):
        self.type, self.index, self.armed = NONE, 0, False
        self.recording, self.min_time, self.max_time = False, 0.0, 0.0


class _Take:
    def __init__(self, track, ch0, channels, capacity=None):
        self.track, self.ch0, self.channels = track, ch0, channels
        self.blocks, self.status = [], 0
        self.capacity = capacity      # chunks this take can hold (None: as many as it needs)


class RecordModel:
    def __init__(self, block_frames: int = 512, sample_rate: int = 48000, bpm: float = 120.0, chunk: int = 65536,
                 capacity=None):
        self.F, self.sr = block_frames, sample_rate
        self.chunk, self.capacity = chunk, capacity
        self.beat_duration = 60.0 / bpm
        self.tracks: list[_Track] = []
        self.input_channels = 0
        self.playing = self.recording = False
        self.playhead = self.playhead_start = 0.0
        self.takes: list[_Take] = []
        self.clips: list[dict] = []
        self.statuses: list[int] = []      # what every call returned

    # ---- Track ----
    @staticmethod
    def _prepare_record(t: _Track, time_pos: float):
        t.min_time = t.max_time = time_pos
        t.recording = True

    @staticmethod
    def _stop_record_track(t: _Track):
        t.min_time = t.max_time = 0.0
        t.recording = False

    # ---- Engine ----
    def play(self):
        if self.recording:
            for tk in self.takes:
                if tk.track is not None:
                    self._prepare_record(tk.track, self.playhead_start)
        self.playing = True
        return OK

    def record(self):
        if self.recording and self.playing:
            return OK
        for t in self.tracks:
            if t.armed and t.type != NONE:
                first, width = (2 * t.index, 2) if t.type == STEREO else (t.index, 1)
                if first + width > self.input_channels:
                    return INVALID
        self.takes = []
        for t in self.tracks:
            if t.armed and t.type != NONE:
                cap = self.capacity
                if isinstance(cap, (list, tuple)):
                    cap = cap[len(self.takes)] if len(self.takes) < len(cap) else None
                self.takes.append(_Take(t, 2 * t.index if t.type == STEREO else t.index, 2 if t.type == STEREO else 1, cap))
        self.recording = True
        self.play()
        return OK

    def stop_record(self):
        if not self.recording:
            return OK
        self.recording = False
        st = OK
        for slot, t in enumerate(self.tracks):
            for tk in self.takes:
                if tk.track is t and t.recording and tk.blocks:
                    self.clips.append(dict(track=slot, args=(slot, t.min_time, t.max_time, 0.0, 1.0, 1.0),
                                           blocks=list(tk.blocks), ch0=tk.ch0, channels=tk.channels, status=tk.status))
                    if tk.status & REC_OVERFLOW:
                        st = OVERFLOW
            self._stop_record_track(t)
        self.takes = []
        return st

    def stop(self):
        if self.recording:
            self.stop_record()
        self.playing = False
        self.playhead = self.playhead_start
        for t in self.tracks:
            self._stop_record_track(t)
        return OK

    def block(self, i):
        """Engine::process: process_event's record_max_time step on every recording track, the transport, the tap."""
        if not self.playing:
            return OK
        buffer_duration_in_beats = (self.F / self.sr) / self.beat_duration
        for t in self.tracks:
            if t.recording:
                t.max_time += buffer_duration_in_beats
        self.playhead = self.playhead + buffer_duration_in_beats
        if self.recording and self.takes:
            for tk in self.takes:
                last_chunk = (len(tk.blocks) * self.F + self.F - 1) // self.chunk     # the chunk of the block's last frame
                lost = tk.capacity is not None and last_chunk >= tk.capacity
                if lost and tk.track is not None:
                    tk.status |= REC_OVERFLOW
                tk.blocks.append(None if lost else i)
                if i is None:
                    tk.status |= REC_SILENCE
        return OK

    def set_track_input(self, slot, type_, index, armed):
        if type_ == MIDI:
            return UNSUPPORTED
        if slot >= len(self.tracks):
            return INVALID
        t = self.tracks[slot]
        t.type, t.index, t.armed = type_, index, bool(armed)
        return OK

    def delete_track(self, slot):
        if slot >= len(self.tracks):
            return INVALID
        t = self.tracks.pop(slot)
        for tk in self.takes:
            if tk.track is t:
                tk.track = None
        return OK

    def run(self, script):
        for op in script:
            k = op[0]
            if k == "tracks":
                self.tracks += [_Track() for _ in range(op[1])]
                st = OK
            elif k == "inputs":
                self.input_channels = op[1]
                st = OK
            elif k == "bpm":
                self.beat_duration = 60.0 / op[1]
                st = OK
            elif k == "playhead":
                self.playhead_start = self.playhead = op[1]
                st = OK
            elif k == "input":
                st = self.set_track_input(*op[1:])
            elif k == "arm":
                st = INVALID if op[1] >= len(self.tracks) else \
                    self.set_track_input(op[1], self.tracks[op[1]].type, self.tracks[op[1]].index, op[2])
            elif k == "record":
                st = self.record()
            elif k == "stop_record":
                st = self.stop_record()
            elif k == "play":
                st = self.play()
            elif k == "stop":
                st = self.stop()
            elif k == "block":
                st = self.block(op[1])
            elif k == "delete":
                st = self.delete_track(op[1])
            elif k == "clear_all":
                for s in range(len(self.tracks) - 1, -1, -1):
                    self.delete_track(s)
                st = OK
            else:
                raise ValueError(op)
            self.statuses.append(st)
        return self.clips


def run(script, block_frames=512, sample_rate=48000, bpm=120.0, chunk=65536, capacity=None):
    return RecordModel(block_frames, sample_rate, bpm, chunk, capacity).run(script)


def take_frames(clip: dict, inputs, block_frames: int) -> np.ndarray:
    """[channels][frames] float32 of a take: block i of `inputs` is an [input channels][F] array; None is silence."""
    out = np.zeros((clip["channels"], len(clip["blocks"]) * block_frames), dtype=np.float32)
    for j, i in enumerate(clip["blocks"]):
        if i is not None:
            out[:, j * block_frames:(j + 1) * block_frames] = inputs[i][clip["ch0"]:clip["ch0"] + clip["channels"], :block_frames]
    return out


def random_script(rng, n_ops=60, max_tracks=6, max_inputs=6):
    """A random call sequence (the C++ host harness and the model must agree on it bit for bit)."""
    script = [("tracks", int(rng.integers(1, max_tracks + 1))), ("inputs", int(rng.integers(0, max_inputs + 1)))]
    n_tracks = script[0][1]
    blocks = 0
    for _ in range(n_ops):
        r = rng.random()
        if r < 0.12:
            script.append(("input", int(rng.integers(0, n_tracks)), int(rng.choice([NONE, STEREO, MONO, MONO])),
                           int(rng.integers(0, 4)), bool(rng.random() < 0.7)))
        elif r < 0.17:
            script.append(("arm", int(rng.integers(0, n_tracks)), bool(rng.random() < 0.6)))
        elif r < 0.25:
            script.append(("record",))
        elif r < 0.29:
            script.append(("stop_record",))
        elif r < 0.32:
            script.append(("play",))
        elif r < 0.35:
            script.append(("stop",))
        elif r < 0.39:
            script.append(("bpm", float(rng.choice([90.0, 120.0, 133.7, 174.0, 61.25]))))
        elif r < 0.42:
            script.append(("playhead", float(rng.choice([0.0, 1.5, 7.25, 1e-3]))))
        elif r < 0.44 and n_tracks > 1:
            script.append(("delete", int(rng.integers(0, n_tracks))))
            n_tracks -= 1
        elif r < 0.46:
            script.append(("tracks", 1))
            n_tracks += 1
        elif r < 0.47:
            script.append(("inputs", int(rng.integers(0, max_inputs + 1))))
        else:
            script.append(("block", None if rng.random() < 0.08 else blocks))
            blocks += 1
    script.append(("stop",))
    return script
