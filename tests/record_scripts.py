"""The random recording scripts the DEVICE runs (tests/test_gpu_record_scripts.py): which ones, and what they contain — decided
here, on the CPU, from tests/record_model.py alone, so that the choice can be checked without a device
(tests/test_record_model.py::test_the_device_scripts_do_something).  The seeds are not those of the host-code test."""
import numpy as np

import record_model as RM

# (block frames, session rate, record chunk frames): the three pairs of test_host_code_matches_the_model_on_random_scripts; the
# chunks are no multiple or divisor of F, so blocks straddle chunk seams at ever different offsets
CONFIGS = [(512, 48000, 700), (128, 44100, 200), (480, 48000, 333)]
N_SCRIPTS = 65          # per configuration, as many as the host-code test runs on the CPU (≈0.03 s per script on the device)
SEED = 0xD5C0


def scripts(block_frames, n=N_SCRIPTS):
    rng = np.random.default_rng(SEED + block_frames)
    return [RM.random_script(rng) for _ in range(n)]


def max_inputs(script):
    return max(op[1] for op in script if op[0] == "inputs")


def added_tracks(script):
    return sum(op[1] for op in script[1:] if op[0] == "tracks")


def n_blocks(script):
    return sum(1 for op in script if op[0] == "block")


def features(script, block_frames, rate):
    """(clips made, deletes of a recording track, record() calls that restart a playing transport, input-less blocks inside
    a take that still has a track) — from the model alone"""
    m = RM.RecordModel(block_frames, rate)
    deletes = restarts = silent = 0
    for op in script:
        live = [tk for tk in m.takes if tk.track is not None]
        if op[0] == "delete" and m.recording and op[1] < len(m.tracks) and any(tk.track is m.tracks[op[1]] for tk in live):
            deletes += 1
        if op[0] == "record" and m.playing and not m.recording:
            restarts += 1
        if op[0] == "block" and op[1] is None and m.recording and m.playing and live:
            silent += 1
        m.run([op])
    return len(m.clips), deletes, restarts, silent


def census(block_frames, rate, n=N_SCRIPTS):
    """the features summed over a configuration's scripts, and in how many scripts each occurs"""
    f = np.array([features(s, block_frames, rate) for s in scripts(block_frames, n)])
    return f.sum(axis=0), (f > 0).sum(axis=0)
