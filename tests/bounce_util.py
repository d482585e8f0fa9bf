"""What the bounce tests share: the oracle running a bounce's defining sequence, the session draws, the CPU-side model of
the host code (length, passes, refusals, transport), and the twin of a session with every fader at unity."""
import dataclasses
import math

import numpy as np

import fuzz_util as FZ
import instance_census as IC
import oracle_ffi as O
from whitebox_amd import synth

OK, UNSUPPORTED, INVALID, OOM = 0, -3, -4, -7
TRACK, BUS, MASTER = 0, 1, 2
POST, PRE = 0, 1


def beat_to_samples(beat, sample_rate, beat_duration):
    """the oracle's beat_to_samples (core_math.h:209-212)"""
    return float(O.lib().wbo_beat_to_samples(float(beat), float(sample_rate), float(beat_duration)))


def bounce_frames(min_time, max_time, sample_rate, bpm):
    return int(beat_to_samples(max_time - min_time, sample_rate, 60.0 / bpm))     # int(): truncation, engine.cpp:1583


def block_beats(block, sample_rate, bpm):
    return (block / sample_rate) / (60.0 / bpm)


# ---- the model of the host code --------------------------------------------------------------------------------------
class BounceModel:
    """The transport of a session and what wbx_engine_bounce does to it, in plain Python: the defining sequence
    set_playhead_position(min), play(), K blocks, stop(), set_playhead_position(the playhead before)."""

    def __init__(self, block=512, rate=48000, max_blocks=8):
        self.F, self.rate, self.max_blocks = block, rate, max_blocks
        self.n_tracks = self.n_buses = 0
        self.beat_duration = 0.5
        self.playhead = self.playhead_start = self.sample_position = 0.0
        self.playing = self.recording = self.redirected = False
        self.edits = 0

    def set_playhead(self, beat):
        self.playhead = self.playhead_start = beat
        self.edits += 1

    def play(self):
        self.sample_position = 0.0
        self.playing = True
        self.edits += 1

    def stop(self):
        self.playing = False
        self.playhead = self.playhead_start
        self.edits += 1

    def block(self):
        bd = self.beat_duration
        dur = (self.F / float(self.rate)) / bd            # engine.cpp:1578-1582
        if self.playing:
            self.sample_position += (dur * bd) * float(self.rate)   # beat_to_samples: two rounded multiplies
            self.playhead = self.playhead + dur

    def check(self, min_time, max_time, sources):
        if self.playing or self.recording or self.redirected:
            return UNSUPPORTED, 0, 0
        if not sources or not (max_time > min_time):
            return INVALID, 0, 0
        for kind, index, tap in sources:
            ok = (kind == TRACK and index < self.n_tracks and tap in (POST, PRE)) or \
                 (kind == BUS and index < self.n_buses and tap == POST) or (kind == MASTER and index == 0 and tap == POST)
            if not ok:
                return INVALID, 0, 0
        n = int(beat_to_samples(max_time - min_time, self.rate, self.beat_duration))
        if n == 0:
            return INVALID, 0, 0
        if n >= 2147483632:
            return UNSUPPORTED, 0, 0
        return OK, n, -(-n // self.F)

    def bounce(self, min_time, max_time, sources, fail_alloc_at=-1):
        """-> (status, n_frames, passes [(first block, blocks)], sources kept in order, allocations released)"""
        st, n, K = self.check(min_time, max_time, sources)
        if st != OK:
            return st, 0, [], [], []
        if 0 <= fail_alloc_at < len(sources):
            return OOM, 0, [], [], list(range(fail_alloc_at))
        before = self.playhead
        self.set_playhead(min_time)
        self.play()
        passes, done = [], 0
        while done < K:
            k = min(self.max_blocks, K - done)
            passes.append((done, k))
            for _ in range(k):
                self.block()
            done += k
        self.stop()
        self.set_playhead(before)
        return OK, n, passes, list(sources), []


# ---- the oracle running the defining sequence ------------------------------------------------------------------------
def unity_twin(spec):
    """the same session with every track at 0 dB, pan 0, unmuted: gain exactly 1.0f on both channels"""
    n = spec.n_tracks
    return dataclasses.replace(spec, volumes_db=[0.0] * n, pans=[0.0] * n, mutes=[False] * n)


def oracle_sequence(e, spec, min_time, max_time, bpm=None):
    """the defining sequence on oracle engine `e` (stopped): -> n_frames, tracks [N][C][n], master [C][n], buses [NB][C][n]
    or None, each trimmed to n_frames"""
    n = bounce_frames(min_time, max_time, spec.sample_rate, bpm or spec.bpm)
    K = -(-n // spec.block)
    before = e.playhead
    e.set_playhead(min_time)
    e.play()
    tr, ms, bs = [], [], []
    for _ in range(K):
        m, b, t = e.process_tracks(want_buses=True)
        ms.append(m)
        tr.append(t)
        if b is not None:
            bs.append(b)
    e.stop()
    e.set_playhead(before)
    tracks = np.concatenate(tr, axis=2)[:, :, :n] if tr else np.zeros((0, spec.channels, n), np.float32)
    master = np.concatenate(ms, axis=1)[:, :n]
    buses = np.concatenate(bs, axis=2)[:, :, :n] if bs else None
    return n, tracks, master, buses


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- session draws ------------------------------------------------------------------------------------------------------
def census_entries():
    """Every census entry a bounce can reach: all mix_kernel / mix_kernel_x instances and the sum_kernel entries (whose
    sessions name the mix instance they take).  The callback_kernel entries are left out by construction, not by choice: a
    bounce renders through batch passes (render_locked outside wbx_engine_process), which never launch the one-block callback
    kernel.  No other entry needs a process of its own (proc_env): the per-context switches (env) are set before the engine
    is built."""
    return [e for e in IC.CENSUS if not e.callback]


def census_mix_name(entry):
    return entry.mix if entry.name.startswith(IC.S) else entry.name


def mix_family(name):
    """the row-mode family (0 fp32 lean, 1 everything, 2 16-bit lean, 3 resampled integer) out of an instance name"""
    args = [x.strip() for x in name[name.index("<") + 1:name.rindex(">")].split(",")]
    return int(args[2] if name.startswith(IC.X) else args[3])


def drawn_sessions():
    """(name, spec, n_blocks) of every session the stem test bounces whole (every track, both taps): 10 random_session and
    12 random_masked_session draws (3 seeds x fp32 masked rows / integer PCM at unity / 16-bit lean / the everything family,
    3 to 200 tracks), the BASELINE c1 / c2 shapes, a c3-shaped session (resampled 44.1 kHz, gain + pan) small enough for the
    oracle, whole and cut into clips, and the seek session.  The census sessions have a test of their own."""
    out = []
    for seed in range(10):
        spec, k = FZ.random_session(seed)
        out.append((f"fuzz{seed}", spec, k))
    for seed in range(3):
        for kw in ({}, {"integer_unity": True}, {"lean16": True}, {"everything": True}):
            spec, k = FZ.random_masked_session(seed, **kw)
            out.append((spec.name, spec, k))
    out.append(("c1", synth.make_session("c1", 8, clip_channels=1, n_blocks=8, unity_gain=True, seed=0x5EED0001), 8))
    out.append(("c2", synth.make_session("c2", 256, n_blocks=6, seed=0x5EED0002), 6))
    c3 = synth.make_session("c3", 96, src_rate=44100, n_blocks=12, seed=0x5EED0003)
    out.append(("c3", c3, 12))
    out.append(("c3cut", synth.cut_into_clips(c3, 5.3, 12), 12))
    out.append(("seek", synth.make_session("seek", 48, src_rate=44100, seek=True, n_blocks=8, seed=0x5EED00AA), 8))
    return out


def oracle_stems(spec, lo, hi, tracks=None):
    """post- and pre-fader track buffers [len(tracks)][C][n] of the defining sequence (pre: the unity twin), n_frames"""
    outs = []
    for sp in (spec, unity_twin(spec)):
        e = O.build_oracle_engine(sp)
        n = bounce_frames(lo, hi, spec.sample_rate, spec.bpm)
        e.set_playhead(lo)
        e.play()
        keep = []
        for _ in range(-(-n // spec.block)):
            _, _, t = e.process_tracks()
            keep.append(t if tracks is None else t[tracks])
        e.close()
        outs.append(np.concatenate(keep, axis=2)[:, :, :n])
    return n, outs[0], outs[1]


def bounce_range(spec, n_blocks):
    """a range that starts inside the first block (inside a clip, for the one-clip sessions), is not a whole number of
    blocks long and ends inside a block: [start + 0.37 blocks, start + (n_blocks - 0.45) blocks)"""
    unit = block_beats(spec.block, spec.sample_rate, spec.bpm)
    lo = spec.playhead_start + 0.37 * unit
    return lo, spec.playhead_start + (n_blocks - 0.45) * unit


def all_stems(spec):
    """every track post-fader, then every track pre-fader"""
    return [("track", t, "post") for t in range(spec.n_tracks)] + [("track", t, "pre") for t in range(spec.n_tracks)]
