"""Positions far into long clips, on the CPU: the product's sequencer source (wbx_seq.h, through tests/cpp/host_sim.cpp)
against the oracle and against the bounds of the hot loop's 32-bit index math, with clips of up to 2^31-17 frames — the
longest the ABI accepts — read around 2^24, 2^30, classify's bound 2147483000 and the clip's last frames, and at slow speeds
where the clip-tail quotient (count - offset) / speed passes a multiple of 2^32."""
import math

import numpy as np
import pytest

import host_sim as HS
import long_sessions as LS
import oracle_ffi as O
from sparse_clip import CAP, PAD

from long_sessions import KIND_GENERIC, KIND_MASK, KIND_NAMES, KIND_SILENT, landmark_tracks
SPEEDS = (1.0, 0.5, 44100 / 48000, 48000 / 44100, 0.999, 0.9990001, 1.088, 2.0, 3.7, 4096.0, 4097.0, 1e-3)
FMTS = ("f32", "i16", "i24", "i32")


def hot_records(sim, K, N):
    """(kind, plan record) of every stream call of a (block, track) the mix kernel's hot loop renders"""
    flags, kinds = sim.row_kinds(K * N)
    out = []
    for r in sim.fetch_plan():
        k = kinds[r[0] * N + r[1]]
        if k != 0xFF and (k & KIND_MASK) not in (KIND_SILENT, KIND_GENERIC):
            out.append((k & KIND_MASK, r))
    return out


# how far past the tap of a record's last frame the hot loop's loads reach (wbx_mix.h): a window row loads src[ix0..ix0+4]
# for each lane's four frames (load_window; load_window16's 4-B load at src + 4 also takes ix0+5), unity rows go through the
# same window loads with ix0 = (uint32_t)pos + j0, a stride row loads (int)x and x + 1 per frame (load_stride).  The last
# lane's ix0 is at most the last frame's tap: lanes past a partial row's last frame load from that frame (part_cf0).
READ_REACH = {1: 4, 2: 4, 4: 5, 5: 4, 6: 1, 7: 5}


def check_taps(kind, rec, count):
    """every sample the hot loop loads for this stream call lies in [0, count + 16) and below 2^31"""
    b, t, bo, ns, na, smp, off, sp, g, fl = rec
    if na == 0 or off >= count:
        return None
    x0, x1 = off, off + float(na - 1) * sp          # the kernel's fp64 positions of the first and last frame
    lo, hi = math.trunc(x0), math.trunc(x1)
    if kind in (1, 4, 5):                           # unity: (uint32_t)pos + j
        assert sp == 1.0
        hi = math.trunc(off) + na - 1
    top = hi + READ_REACH[kind]
    assert 0 <= lo and top < count + PAD and top < 2**31, (KIND_NAMES[kind], rec, count)
    return x1


def random_track(rng, F):
    """(format, count, playback speed, start offset, first block frame, last block frame) of one track's clip"""
    sp = float(rng.choice(SPEEDS))
    span = 3 * F * sp
    where = rng.integers(0, 4)
    if where == 0:          # through classify's bound
        start = LS.BOUND - float(rng.uniform(-0.5, 3.0)) * F * sp
        count = int(rng.integers(min(CAP, int(start) + 2), CAP + 1))
    elif where == 1:        # through the clip's last frames
        count = int(rng.integers(max(2, int(span) + 8), CAP + 1))
        start = count - float(rng.uniform(0.0, 3.5)) * F * sp
    elif where == 2:        # around 2^24 / 2^30
        start = float(rng.choice([2**24, 2**30])) - float(rng.uniform(-2.0, 2.0)) * F * sp
        count = int(rng.integers(int(start) + 2, CAP + 1))
    else:
        count = int(rng.integers(2, CAP + 1))
        start = float(rng.uniform(0, count))
    start = max(0.0, start if rng.random() < 0.5 else math.floor(start))
    first = 0.0 if rng.random() < 0.6 else float(rng.uniform(0, F))
    last = 1e12 if rng.random() < 0.6 else float(rng.uniform(F, 3 * F))
    return str(rng.choice(FMTS)), count, sp, start, first, last


def test_hot_loop_taps_stay_inside_the_clip_for_every_block_size():
    """The routing invariant: every record classify, masked_kind and the planner's runs hand to the hot loop has every
    sample its loads reach (READ_REACH) inside [0, count + 16) and below 2^31 — every accepted block size (4..32768, multiples of 4), every mask level,
    every streamed speed (4097 and 1e-3 included), positions up to classify's bound 2147483000 and clips up to 2^31-17
    frames.  classify itself bounds only the first frame's position; the last frame of a full-block row stays below 2^31
    because the row is full only while the clip-tail limit lets the whole block play, so its last position lies inside the
    clip — and the clip is shorter than 2^31-16 frames.  Without that cap the invariant would not hold."""
    n_hot, near_bound, kinds_seen = 0, 0, set()
    T, K = 6, 3
    for F in range(4, 32769, 4):
        rng = np.random.default_rng(F)
        sim = HS.HostSimEngine(T, F, 48000, 2, max_blocks=K)
        sim.set_masked_rows(int(F // 4) % 5)
        sim.set_bpm(120.0)
        fpb = 48000 * 60.0 / 120.0
        counts = []
        for t in range(T):
            fmt, count, sp, start, first, last = random_track(rng, F)
            sid = sim.add_sample_meta(fmt, 1, 48000, count)
            counts.append(count)
            tr = sim.add_track()
            sim.add_audio_clip(tr, "c", first / fpb, last / fpb, start, sid, sp, 1.0)
        sim.play()
        sim.render(K)
        for kind, rec in hot_records(sim, K, T):
            x1 = check_taps(kind, rec, counts[rec[5]])
            if x1 is not None:
                n_hot += 1
                kinds_seen.add(kind)
                near_bound += x1 >= 2147482000.0
        sim.close()
    assert n_hot > 20000 and near_bound > 500, (n_hot, near_bound)
    assert kinds_seen == set(KIND_NAMES), kinds_seen


def plan_rows(plan):
    return [(b, t, bo, ns, O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (b, t, bo, ns, na, smp, off, spd, g, fl) in plan]


def oracle_rows(e, block):
    return [(block, t, ds, min(ln, 0xFFFF), O.f64_bits(off), O.f64_bits(spd), O.f32_bits(g), smp)
            for (t, ds, ln, off, spd, g, smp) in e.seglog()]


def oracle_session_rows(spec, n_blocks):
    """the oracle's stream-call log and transport (clip data: none needed, the sequencing does not read it)"""
    import sparse_clip as SC
    data = [SC.sparse_sample_data(spec.seed, s, []) for s in spec.samples]
    e = O.build_oracle_engine(spec, sample_data=data)
    e.enable_seglog()
    e.play()
    rows = []
    for b in range(n_blocks):
        e.process()
        rows += oracle_rows(e, b)
    tr = (O.f64_bits(e.playhead), O.f64_bits(e.sample_position))
    e.close()
    return rows, tr


@pytest.mark.parametrize("fmt", ["f32", "i16", "i32"])
@pytest.mark.parametrize("F", [512, 4096])
def test_host_sequencer_at_large_positions_matches_oracle(fmt, F):
    """The product's sequencer source (batch, block by block, by segments, every mask level) against the oracle's stream
    calls on a 2^31-17-frame clip: tracks through 2147483000, 2^30, 2^24, the clip's end and cut clips near the bound"""
    n_blocks = 8
    speeds = (1.0, 44100 / 48000, 1.088, 2.0, 3.7) + ((4096.0, 4097.0) if F == 512 else ())
    spec = LS.session(f"lp_{fmt}_{F}", fmt, CAP, landmark_tracks(F, CAP, speeds, n_blocks), block=F)
    rows, tr = oracle_session_rows(spec, n_blocks)
    for masked, segments, batch in [(0, 0, True), (4, 0, True), (1, 0, False), (2, 2, True), (3, 0, True)]:
        sim = HS.build_sim_engine(spec, max_blocks=n_blocks, masked_rows=masked, segments=segments)
        sim.play()
        if batch:
            sim.render(n_blocks)
            got = plan_rows(sim.fetch_plan())
        else:
            got = []
            for b in range(n_blocks):
                sim.render(1)
                got += [(b,) + r[1:] for r in plan_rows(sim.fetch_plan())]
        assert got == rows, (masked, segments, batch)
        ph, sp, _ = sim.transport()
        assert (O.f64_bits(ph), O.f64_bits(sp)) == tr
        sim.close()


@pytest.mark.parametrize("count,speed,k", [(5_000_000, 1e-3, 1), (5_000_000, 1e-4, 11), (CAP, 2e-5, 24)])
@pytest.mark.parametrize("F", [512, 64])
def test_host_sequencer_tail_quotient_crossing_2_32(count, speed, k, F):
    """a slow clip whose tail quotient ceil((count - offset) / speed) passes k * 2^32 at frames 0, 1, F/2 and F-1 of a block
    (the reference plays that block short or silent, sampler.cpp:104): the sequencer's u32_of_ceil against the oracle, in
    batch and block-by-block plans"""
    n_blocks = 6
    tracks, where = [], []
    for r in (0, 1, F // 2, F - 1):
        sp, off, b = LS.crossing_track(count, speed, k, r, F, n_blocks)
        tracks.append((sp, off, 0.0, 1e12))
        where.append((b, r))
    spec = LS.session(f"q32_{F}", "f32", count, tracks, block=F)
    rows, tr = oracle_session_rows(spec, n_blocks)
    for masked in (0, 4):
        sim = HS.build_sim_engine(spec, max_blocks=n_blocks, masked_rows=masked)
        sim.play()
        sim.render(n_blocks)
        plan = sim.fetch_plan()
        assert plan_rows(plan) == rows
        na = {(b, t): n for (b, t, bo, ns, n, *_r) in plan}
        assert [na[(b, t)] for t, (b, r) in enumerate(where)] == [r for b, r in where]
        sim.close()
