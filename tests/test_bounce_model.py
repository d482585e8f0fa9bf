"""Bouncing without a device: the product's host code of wbx_engine_bounce (HostSession::bounce_locked, wbx_host.h, compiled
with g++ into tests/cpp/bounce_sim.cpp) against bounce_util.BounceModel (plain Python) and the oracle's beat_to_samples —
length and block count, pass splitting for several max_blocks, the refusal table, the transport afterwards, order and
duplicates of the sources, and what goes back to the pool when it cannot hold every destination.  Doubles as bit patterns."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bounce_util as BU
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.fixture(scope="module")
def bounce_sim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("bounce_sim") / "bounce_sim")
    subprocess.check_call([cxx, "-std=c++20", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "bounce_sim.cpp"),
                           "-o", exe, "-lpthread"])
    return exe


def _line(op):
    k = op[0]
    if k == "bounce":
        _, lo, hi, srcs = op
        return f"bounce {_bits(lo):016x} {_bits(hi):016x} {len(srcs)} " + " ".join(f"{a} {b} {c}" for a, b, c in srcs)
    if k in ("bpm", "playhead"):
        return f"{k} {op[1]!r}"
    return " ".join([k] + [str(int(a)) for a in op[1:]])


def run_sim(exe, script, block, rate, max_blocks):
    text = "\n".join([f"frames {block}", f"rate {rate}", f"max_blocks {max_blocks}"] + [_line(op) for op in script]) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out, cur = [], {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "bounce":
            npass = int(w[3])
            passes = [(int(w[4 + 2 * i]), int(w[5 + 2 * i])) for i in range(npass)]
            at = 4 + 2 * npass + 1
            npub = int(w[at])
            pub = [tuple(int(x) for x in w[at + 1 + 4 * i: at + 5 + 4 * i]) for i in range(npub)]
            at += 1 + 4 * npub + 1
            nrel = int(w[at])
            cur["bounce"] = (int(w[1]), int(w[2]), passes, pub, [int(x) for x in w[at + 1: at + 1 + nrel]])
        elif w[0] == "status":
            cur["status"] = int(w[1])
        else:
            cur["transport"] = (int(w[1], 16), int(w[2], 16), int(w[3], 16), int(w[4]), int(w[5]))
            out.append(cur)
            cur = {}
    return out[3:]          # (the three settings lines)


def run_model(script, block, rate, max_blocks):
    m = BU.BounceModel(block, rate, max_blocks)
    out, fail_at = [], -1
    for op in script:
        k, rec = op[0], {"status": 0}
        if k == "tracks":
            m.n_tracks += op[1]
        elif k == "buses":
            m.n_buses = op[1]
        elif k == "bpm":
            m.beat_duration = 60.0 / op[1]
        elif k == "playhead":
            m.set_playhead(op[1])
        elif k == "play":
            m.play()
        elif k == "stop":
            m.stop()
        elif k == "block":
            m.block()
        elif k == "recording":
            m.recording = bool(op[1])
        elif k == "redirected":
            m.redirected = bool(op[1])
        elif k == "fail_alloc":
            fail_at = op[1]
        elif k == "bounce":
            st, n, passes, kept, released = m.bounce(op[1], op[2], op[3], fail_at)
            rec = {"status": st, "bounce": (st, n, passes, [s + (i,) for i, s in enumerate(kept)], released)}
        rec["transport"] = (_bits(m.playhead), _bits(m.playhead_start), _bits(m.sample_position), int(m.playing), m.edits)
        out.append(rec)
    return out


def compare(exe, script, block=512, rate=48000, max_blocks=8):
    got, want = run_sim(exe, script, block, rate, max_blocks), run_model(script, block, rate, max_blocks)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, script[i], g, w)
    return want


T, B, M, POST, PRE = BU.TRACK, BU.BUS, BU.MASTER, BU.POST, BU.PRE


# ---- the model itself, by hand ---------------------------------------------------------------------------------------
def test_length_is_the_oracles_beat_to_samples_truncated():
    assert BU.bounce_frames(0.0, 1.0, 48000, 120.0) == 24000
    assert BU.bounce_frames(1.0, 1.0 + 1023.9 / 24000.0, 48000, 120.0) == 1023
    # a tempo where beat_to_samples is inexact: 60 / 97 s per beat; one beat is 29690.72... frames
    assert BU.bounce_frames(0.0, 1.0, 48000, 97.0) == 29690
    assert BU.beat_to_samples(1.0, 48000, 60.0 / 97.0) == (1.0 * (60.0 / 97.0)) * 48000.0     # two rounded multiplies
    m = BU.BounceModel(512, 48000, 8)
    m.n_tracks = 1
    st, n, passes, _, _ = m.bounce(0.25, 0.25 + 7.0, [(T, 0, POST)])
    assert (st, n) == (0, 168000) and passes == [(i * 8, 8) for i in range(41)] + [(328, 1)]   # 168000 = 328.125 blocks


def test_the_model_leaves_the_defining_sequences_transport():
    m = BU.BounceModel(512, 48000, 3)
    m.n_tracks = 2
    m.set_playhead(3.5)
    st, n, passes, kept, _ = m.bounce(1.0, 1.1, [(T, 1, PRE), (T, 1, POST), (T, 1, PRE)])
    assert st == 0 and n == 2400 and passes == [(0, 3), (3, 2)]
    assert kept == [(T, 1, PRE), (T, 1, POST), (T, 1, PRE)]
    assert (m.playhead, m.playhead_start, m.playing) == (3.5, 3.5, False)
    sp = 0.0
    for _ in range(5):
        sp += ((512 / 48000.0) / 0.5 * 0.5) * 48000.0
    assert m.sample_position == sp and m.edits == 5


# ---- the product's host code against the model -------------------------------------------------------------------------
def test_host_code_lengths_and_passes(bounce_sim):
    for block, rate, bpm in [(512, 48000, 120.0), (512, 48000, 97.0), (128, 44100, 140.5), (480, 48000, 61.3), (1024, 96000, 174.0),
                             (64, 22050, 333.3)]:
        unit = BU.block_beats(block, rate, bpm)
        for mb in (1, 3, 8, 4096):
            script = [("tracks", 2), ("bpm", bpm), ("playhead", 0.75)]
            for lo, length in [(0.0, 5 * unit), (0.3, 5.5 * unit), (1.0, 0.4 * unit), (2.0, 1.0), (0.1, 3.0001 * unit),
                               (7.0, unit), (0.0, 1.5 / (rate * 60.0 / bpm)), (3.0, 24.99 * unit)]:
                script.append(("bounce", lo, lo + length, [(T, 0, POST), (M, 0, POST)]))
            want = compare(bounce_sim, script, block, rate, mb)
            for op, w in zip(script[3:], want[3:]):
                st, n, passes, _, _ = w["bounce"]
                assert st == 0 and n == int(O.lib().wbo_beat_to_samples(op[2] - op[1], float(rate), 60.0 / bpm))
                assert sum(k for _, k in passes) == -(-n // block) and all(k <= mb for _, k in passes)
                assert [f for f, _ in passes] == [sum(k for _, k in passes[:i]) for i in range(len(passes))]


def test_host_code_refusal_table(bounce_sim):
    unit = BU.block_beats(512, 48000, 120.0)
    ok = [(T, 0, POST)]
    script = [("tracks", 3), ("buses", 2), ("playhead", 1.5),
              ("bounce", 0.0, 1.0, []), ("bounce", 1.0, 1.0, ok), ("bounce", 2.0, 1.0, ok), ("bounce", float("nan"), 1.0, ok),
              ("bounce", 1.0, 1.0 + 1e-9, ok),                                   # no frame
              ("bounce", 0.0, 1.0, [(T, 3, POST)]), ("bounce", 0.0, 1.0, [(B, 2, POST)]), ("bounce", 0.0, 1.0, [(B, 0, PRE)]),
              ("bounce", 0.0, 1.0, [(M, 0, PRE)]), ("bounce", 0.0, 1.0, [(M, 1, POST)]), ("bounce", 0.0, 1.0, [(3, 0, POST)]),
              ("bounce", 0.0, 1.0, [(T, 0, 2)]), ("bounce", 0.0, 1.0, [(T, 0, POST), (T, 0, PRE), (T, 9, POST)]),
              ("bounce", 0.0, 1e9, ok),                                          # 2^31-16 frames or more
              ("play",), ("block",), ("bounce", 0.0, unit, ok), ("stop",),
              ("recording", 1), ("bounce", 0.0, unit, ok), ("recording", 0),
              ("redirected", 1), ("bounce", 0.0, unit, ok), ("redirected", 0),
              ("bounce", 0.0, unit, ok)]
    want = compare(bounce_sim, script, max_blocks=4)
    sts = [w["status"] for w, op in zip(want, script) if op[0] == "bounce"]
    assert sts == [BU.INVALID] * 13 + [BU.UNSUPPORTED] * 4 + [BU.OK]
    for (prev, w), op in zip(zip(want, want[1:]), script[1:]):
        if op[0] == "bounce" and w["status"] != 0:
            assert w["transport"] == prev["transport"]          # a refusal leaves the transport (and the edit count) alone
            assert w["bounce"][2:] == ([], [], [])


def test_host_code_sources_order_duplicates_and_exhaustion(bounce_sim):
    srcs = [(B, 1, POST), (T, 2, PRE), (M, 0, POST), (T, 2, POST), (T, 2, PRE), (B, 1, POST), (T, 0, POST)]
    script = [("tracks", 3), ("buses", 2), ("bpm", 97.0), ("playhead", 2.0), ("bounce", 0.5, 0.9, srcs)]
    for k in (0, 3, 6):
        script += [("fail_alloc", k), ("bounce", 0.5, 0.9, srcs)]
    script += [("fail_alloc", -1), ("bounce", 0.5, 0.9, srcs[::-1])]
    want = compare(bounce_sim, script, max_blocks=3)
    b = [w["bounce"] for w in want if "bounce" in w]
    assert [x[3] for x in b[0][3]] == list(range(7)) and [x[:3] for x in b[0][3]] == srcs
    assert [(x[0], x[4]) for x in b[1:4]] == [(BU.OOM, []), (BU.OOM, [0, 1, 2]), (BU.OOM, [0, 1, 2, 3, 4, 5])]
    assert [x[:3] for x in b[4][3]] == srcs[::-1]


def test_host_code_matches_the_model_on_random_scripts(bounce_sim):
    rng = np.random.default_rng(0xB0C0)
    bounces = 0
    for _ in range(60):
        block = int(rng.choice([64, 128, 480, 512, 1024]))
        rate = int(rng.choice([44100, 48000, 96000]))
        mb = int(rng.choice([1, 2, 3, 8, 64]))
        nt, nb = int(rng.integers(0, 5)), int(rng.integers(0, 3))
        script = [("tracks", nt), ("buses", nb)]
        for _ in range(int(rng.integers(4, 14))):
            r = rng.random()
            if r < 0.5:
                unit = BU.block_beats(block, rate, 120.0)
                lo = float(rng.choice([0.0, rng.random() * 8]))
                length = float(rng.choice([rng.random() * 30 * unit, rng.random() * unit, 0.0, -1.0]))
                n = int(rng.integers(0, 6))
                srcs = [(int(rng.integers(0, 3)), int(rng.integers(0, 5)) if rng.random() < 0.7 else 0,
                         int(rng.integers(0, 2)) if rng.random() < 0.6 else 0) for _ in range(n)]
                script.append(("bounce", lo, lo + length, srcs))
                bounces += 1
            elif r < 0.6:
                script.append(("bpm", float(rng.choice([120.0, 97.0, 140.5, 61.3, 999.0]))))
            elif r < 0.7:
                script.append(("playhead", float(rng.random() * 10)))
            elif r < 0.78:
                script.append(("play",))
            elif r < 0.88:
                script.append(("stop",))
            elif r < 0.94:
                script.append(("block",))
            else:
                script.append(("fail_alloc", int(rng.integers(-1, 4))))
        compare(bounce_sim, script, block, rate, mb)
    assert bounces > 100


def test_no_drawn_session_is_refused():
    """the sessions test_gpu_bounce.py draws, through the model's refusal table: 0 refused of 27 drawn (0 %; the limit is
    10 %) — none redirects the master, all are stopped when bounced, every track index is in range, every range holds frames"""
    refused = 0
    sessions = BU.drawn_sessions()
    for name, spec, k in sessions:
        m = BU.BounceModel(spec.block, spec.sample_rate, 8)
        m.n_tracks, m.n_buses, m.beat_duration = spec.n_tracks, spec.n_buses, 60.0 / spec.bpm
        lo, hi = BU.bounce_range(spec, k)
        st, n, K = m.check(lo, hi, [(T, t, tap) for tap in (POST, PRE) for t in range(spec.n_tracks)])
        refused += st != 0
        assert st != 0 or (n % spec.block != 0 and K >= 2), name      # not a whole number of blocks
    assert len(sessions) == 27 and refused == 0


def test_the_census_cases_cover_every_mix_instance():
    """test_gpu_bounce.py::test_every_mix_instance_bounces_exactly asserts, per entry, that the bounce's pass launched the
    entry's instance; here: those entries name EVERY mix_kernel / mix_kernel_x instance of the census (which a test of its
    own holds equal to what the library compiles), all four families, cut (masked-row) and uncut sessions, the packed and the
    non-ragged instances; what is left out is the callback kernel alone, which a bounce cannot launch"""
    import instance_census as IC
    cases = BU.census_entries()
    names = {BU.census_mix_name(e) for e in cases}
    assert names == {e.name for e in IC.CENSUS if e.name.startswith((IC.M, IC.X))}
    assert {BU.mix_family(n) for n in names} == {0, 1, 2, 3}
    assert {BU.mix_family(n) for n in names if n.startswith(IC.X)} == {0, 1}
    assert {e.cut for e in cases} == {False, True} and any(e.env.get("WBX_RAGGED") == "0" for e in cases)
    assert all(not e.proc_env for e in cases)
    assert all(e.callback == e.name.startswith(IC.CB) for e in IC.CENSUS)
    assert len(cases) == 41
