"""Seeded session scripts for the differential against the reference's own sequencer / block driver (tests/ref_engine.py).
Shared by the `-m ref` test (oracle against oracle/_ref/wbref_engine, this container), by oracle/gen_golden.py (which records
the reference's answers into tests/golden/sequencer.npz) and by the tests that replay the recorded answers anywhere.

What a script may NOT do is what the compiled reference has no defined behaviour for: a mono clip resampled into a
stereo session (Q1: the linear path indexes the channel array without `% channels`), negative speeds or start offsets (Q12),
and — found per session, not by construction — the event_length wrap of track.cpp:669 (ref_engine.Wrapped)."""
import numpy as np

from whitebox_amd import synth

import ref_engine as R

PLAIN_RATES = [22050, 44100, 48000, 96000]
PLAIN_SPEEDS = [1.0, 1.0, 1.0, 0.5, 0.8, 0.91875, 0.999, 1.0625, 1.9, 0.3, 4.0]
WILD_RATES = [8000, 11025, 22050, 44100, 96000, 192000]
WILD_SPEEDS = [1.0, 0.01, 0.1, 0.9999999, 1.0000001, 3.99, 8.0, 33.0]
RATES, SPEEDS = PLAIN_RATES, PLAIN_SPEEDS


def _samples(rng, s: R.Script, seed, n, session_rate, out_channels, stereo_only=False):
    """n samples of every storage format; returns per sample whether it may be resampled (Q1)"""
    free = []
    for i in range(n):
        fmt = str(rng.choice(["f32", "f32", "i16", "i24", "i32"]))
        ch = int(rng.integers(1, 3))
        if stereo_only and out_channels == 2:
            ch = 2                         # the session rate may change in mid-play: a mono clip would end up resampled (Q1)
        rate = int(rng.choice(RATES + [session_rate] * 3))
        if ch == 1 and out_channels == 2:
            rate = session_rate            # a mono clip in a stereo session: unity path only
        frames = int(rng.choice([int(rng.integers(5, 300)), int(rng.integers(300, 6000)), int(rng.integers(6000, 30000))]))
        spec = synth.SessionSpec(name="s", n_tracks=1, seed=seed, samples=[synth.SampleSpec(i, ch, rate, frames, fmt,
                                                                                          0.2 if fmt == "f32" else 1.0)],
                                 clips=[], volumes_db=[0.0], pans=[0.0], mutes=[False])
        s.add_sample(fmt, ch, rate, frames, spec.sample_data(0), gen=(seed, i, 0.2 if fmt == "f32" else 1.0))
        free.append(not (ch == 1 and out_channels == 2))
    return free


def _clip_args(rng, t, si, resample_ok, pos, length, frames):
    speed = float(rng.choice(SPEEDS)) if resample_ok else 1.0
    so = float(rng.choice([0, 0, int(rng.integers(0, 400)), int(rng.integers(0, frames + 50))]))
    gain = float(np.float32(rng.choice([1.0, 1.0, 0.5, 1.3, 0.0])))
    return ("clip", t, float(pos), float(pos + length), so, si, speed, gain)


def session_script(seed, kind):
    """kind: 'static' (clip layouts only), 'controls' (transport / parameter / track operations between blocks), 'edits' (clip
    adds into free space, deletes aimed at the sounding clip, gains, moves), 'dense' (back-to-back clips, edges on block edges),
    'far' (the session past timeline frame 2^31 / 2^32: far_session_script)"""
    if kind == "far":
        return far_session_script(seed)
    rng = np.random.default_rng([seed, {"static": 1, "controls": 2, "edits": 3, "dense": 4, "wild": 5}[kind]])
    wild = kind == "wild"           # the corners of what the API accepts, all at once; otherwise an 'edits' script
    out_ch = int(rng.choice([1, 2, 2, 2]))
    block = int(rng.choice([32, 100, 128, 440, 1000, 2048] if wild else [64, 96, 128, 200, 256, 333, 512, 1024]))
    rate = int(rng.choice([22050, 32000, 88200, 192000, 48000] if wild else [44100, 48000, 48000, 96000]))
    bpm = float(rng.choice([20.0, 333.3, 999.0, 120.0] if wild else [120.0, 97.0, 140.5, 61.3, 174.0]))
    global RATES, SPEEDS
    RATES, SPEEDS = (WILD_RATES, WILD_SPEEDS) if wild else (PLAIN_RATES, PLAIN_SPEEDS)
    s = R.Script(out_ch, block, rate, bpm)
    n_tracks = int(rng.integers(1, 7))
    n_blocks = int(rng.integers(6, 25))
    beat_frames = rate * 60.0 / bpm
    total = n_blocks * block / beat_frames          # beats the session plays
    unit = block / beat_frames                      # beats per block
    resample_ok = _samples(rng, s, 0x5E90000 + seed, n_tracks, rate, out_ch, stereo_only=kind == "controls")
    for t in range(n_tracks):
        s.op("track")
        s.op("vol", t, float(np.float32(rng.uniform(-30, 3))))
        s.op("pan", t, float(np.float32(rng.uniform(-1, 1))))
        if rng.random() < 0.1:
            s.op("mute", t, 1)
    start = float(rng.choice([0.0, 0.0, total * 0.15]))
    # clip layouts: sequential per track (touching or with gaps), so that an add never needs reserve_track_region
    for t in range(n_tracks):
        si = int(rng.integers(0, n_tracks))
        frames = s.samples[si][3]
        pos = -0.2 * total * rng.random() if rng.random() < 0.3 else total * rng.random() * 0.3
        n_clips = int(rng.integers(0, 5)) if kind != "dense" else int(rng.integers(5, 40))
        for _ in range(n_clips):
            if wild and rng.random() < 0.4:           # sub-frame and few-frame clips
                length = float(rng.choice([0.3, 1.0, 2.5, 17.0])) / beat_frames
                s.op(*_clip_args(rng, t, si, resample_ok[si], pos, length, frames))
                pos += length + (0.0 if rng.random() < 0.5 else unit * rng.random())
                continue
            if kind == "dense":
                length = unit * float(rng.choice([0.2, 0.5, 1.0, 1.0, 2.0, 3.3, float(rng.uniform(0.05, 4))]))
                if rng.random() < 0.4:
                    pos = round(pos / unit) * unit           # an edge on a block edge
            else:
                length = total * (0.02 + 0.5 * rng.random())
            s.op(*_clip_args(rng, t, si, resample_ok[si], pos, length, frames))
            pos += length + (0.0 if rng.random() < (0.7 if kind == "dense" else 0.3) else total * 0.1 * rng.random())
    if start:
        s.op("seek", start)
    s.op("play")
    if kind in ("static", "dense"):
        s.op("run", n_blocks)
        s.op("clips")
        return s
    done = 0
    ntr = n_tracks
    while done < n_blocks:
        k = int(rng.integers(1, 4))
        s.op("run", k)
        done += k
        ph = start + done * unit                    # (about: tempo changes move it; good enough to aim edits)
        if kind == "controls":
            op = int(rng.integers(0, 11))
            t = int(rng.integers(0, ntr))
            if op == 10:     # the audio back end comes back with another device rate, in mid-play (set_audio_channel_config)
                s.op("rate", int(rng.choice([44100, 48000, 96000, 22050])))
            elif op == 0:
                s.op("vol", t, float(np.float32(rng.choice([rng.uniform(-40, 6), -72.0, -71.99, -100.0, 0.0, 6.0]))))
            elif op == 1:
                s.op("pan", t, float(np.float32(rng.choice([rng.uniform(-1, 1), -1.0, 1.0, 0.0]))))
            elif op == 2:
                s.op("mute", t, int(rng.integers(0, 2)))
            elif op == 3:
                s.op("stop"); s.op("play")
            elif op == 4:
                s.op("seek", float(rng.uniform(0, total)))
                if rng.random() < 0.5:
                    s.op("stop"); s.op("play")
            elif op == 5:
                s.op("bpm", float(rng.choice([120.0, 90.0, 133.3, 200.0])))
            elif op == 6:
                s.op("solo", t)
            elif op == 7 and ntr > 1:
                s.op("movetrack", t, int(rng.integers(0, ntr)))
            elif op == 8 and ntr > 1:
                s.op("deltrack", t); ntr -= 1
            else:
                s.op("stop"); s.op("run", 1); done += 1; s.op("play")
        else:
            op = int(rng.integers(0, 7))
            t = int(rng.integers(0, ntr))
            for _ in range(int(rng.integers(0, 3))):      # what add / move / resize / delete_region would hand to reserve_track_region:
                a = float(rng.uniform(-0.1, 1.2)) * total   # Track::query_clip_by_range on ranges that fall in gaps, span clips,
                b = a + float(rng.choice([rng.uniform(0, 0.5) * total, unit * rng.uniform(0, 2), -unit * rng.uniform(0, 2), 0.0]))   # are empty or INVERTED (Q11)
                s.op("query", int(rng.integers(0, ntr)), a, b)
            if op <= 1:      # delete a clip (index 0..3: often the one that sounds; out of range -> status 2 on both sides)
                s.op("delclip", t, int(rng.integers(0, 4)))
            elif op == 2:
                s.op("gain", t, int(rng.integers(0, 4)), float(np.float32(rng.uniform(0.0, 1.5))))
            elif op == 3:    # a clip far ahead: free space, and the pool chunk of whatever was destroyed last (Q10)
                si = int(rng.integers(0, n_tracks))
                mn = ph + total * float(rng.uniform(0.3, 0.6))
                s.op(*_clip_args(rng, t, si, resample_ok[si], mn, unit * float(rng.uniform(0.3, 4)), s.samples[si][3]))
            elif op == 4:    # a clip somewhere: mostly refused (lands on clips), sometimes a gap
                si = int(rng.integers(0, n_tracks))
                mn = float(rng.uniform(0, total))
                s.op(*_clip_args(rng, t, si, resample_ok[si], mn, unit * float(rng.uniform(0.1, 2)), s.samples[si][3]))
            elif op == 5:    # move: taken only when the destination is free of every clip, the moved one included
                s.op("move", t, int(rng.integers(0, 4)), float(rng.choice([-1, 1])) * total * float(rng.uniform(0.5, 3)))
            else:
                s.op("seek", float(rng.uniform(0, total))); s.op("stop"); s.op("play")
        s.op("clips")
    return s


FAR_FRAMES = [2**31, 2**32, 2**33, 2**31 + 2**30]


def far_session_script(seed):
    """Clips placed, and the playhead set, past timeline frame 2^31 and 2^32 (and 2^33), at several tempos and rates: the
    transport, the block windows and the clip time -> frame conversions with large beat and sample positions.  Between runs:
    seeks to other far landmarks (also just in front of a clip), tempo changes, stop / play, clip deletes, gains, adds far ahead
    and moves.  Its own generator stream: the scripts of the other kinds do not change."""
    global RATES, SPEEDS
    RATES, SPEEDS = PLAIN_RATES, PLAIN_SPEEDS
    rng = np.random.default_rng([seed, 6])
    block = int(rng.choice([64, 128, 256, 512, 1000, 1024]))
    rate = int(rng.choice([44100, 48000, 96000]))
    bpm = float(rng.choice([120.0, 97.0, 140.5, 61.3, 174.0, 20.0, 999.0]))
    s = R.Script(2, block, rate, bpm)
    n_tracks = int(rng.integers(1, 6))
    n_blocks = int(rng.integers(6, 20))
    beat_frames = rate * 60.0 / bpm
    unit = block / beat_frames
    total = n_blocks * unit
    resample_ok = _samples(rng, s, 0x5EA0000 + seed, n_tracks, rate, 2, stereo_only=True)
    for t in range(n_tracks):
        s.op("track")
        s.op("vol", t, float(np.float32(rng.uniform(-30, 3))))
        s.op("pan", t, float(np.float32(rng.uniform(-1, 1))))
    # the landmark, a fraction of a block off it, as a beat position
    base = (float(rng.choice(FAR_FRAMES)) + float(rng.uniform(-3, 3)) * block) / beat_frames
    for t in range(n_tracks):
        si = int(rng.integers(0, n_tracks))
        frames = s.samples[si][3]
        pos = base + total * float(rng.uniform(-0.2, 0.3))
        for _ in range(int(rng.integers(1, 4))):
            length = total * (0.02 + 0.5 * rng.random())
            s.op(*_clip_args(rng, t, si, resample_ok[si], pos, length, frames))
            pos += length + (0.0 if rng.random() < 0.3 else total * 0.1 * rng.random())
    s.op("seek", base + float(rng.choice([0.0, -0.5 * unit, total * 0.1])))
    s.op("play")
    done = 0
    while done < n_blocks:
        k = int(rng.integers(1, 4))
        s.op("run", k)
        done += k
        op = int(rng.integers(0, 8))
        t = int(rng.integers(0, n_tracks))
        if op == 0:          # to another landmark, just in front of the session's clips there
            far = (float(rng.choice(FAR_FRAMES)) - float(rng.uniform(0, 2)) * block) / beat_frames
            s.op("seek", float(rng.choice([far, base + total * float(rng.uniform(0, 0.5))])))
        elif op == 1:
            s.op("bpm", float(rng.choice([120.0, 90.0, 133.3, 200.0])))
        elif op == 2:
            s.op("stop"); s.op("play")
        elif op == 3:
            s.op("delclip", t, int(rng.integers(0, 3)))
        elif op == 4:
            s.op("gain", t, int(rng.integers(0, 3)), float(np.float32(rng.uniform(0.0, 1.5))))
        elif op == 5:        # a clip far ahead: free space
            si = int(rng.integers(0, n_tracks))
            mn = base + total * float(rng.uniform(1.5, 3.0))
            s.op(*_clip_args(rng, t, si, resample_ok[si], mn, unit * float(rng.uniform(0.3, 4)), s.samples[si][3]))
        elif op == 6:
            s.op("move", t, int(rng.integers(0, 3)), float(rng.choice([-1, 1])) * total * float(rng.uniform(0.5, 3)))
        else:
            s.op("seek", base + total * float(rng.uniform(0, 0.6)))
        s.op("clips")
    return s


# ---- kind 'overlap': edits aimed at every outcome of Engine::reserve_track_region --------------------------------------------
def _with(s: R.Script, extra):
    t = R.Script(s.channels, s.block, s.rate)
    t.ops, t.samples = list(s.ops) + list(extra), s.samples
    return t


def _candidates(rng, cl, t, ph, unit, n_samples, resample_ok, samples, family):
    """aimed edits on track t whose clip list (floats) is cl: [(op tuple)], several per caller; which class each one is, the
    reference says (overlap_script asks it)"""
    out, n = [], len(cl)
    under = [i for i, c in enumerate(cl) if c[0] <= ph < c[1]]

    def pick():
        return under[0] if under and rng.random() < 0.6 else int(rng.integers(0, n))

    def before(i):          # a point not after clip i's start and not inside the clip in front of it: the edge itself, the neighbour's edge, the gap
        c, lo = cl[i], (cl[i - 1][1] if i else max(cl[i][0] - 2 * unit, 0.0))
        return float(rng.choice([c[0], lo, 0.5 * (lo + c[0])]))

    def after(i):
        c, hi = cl[i], (cl[i + 1][0] if i + 1 < n else cl[i][1] + 2 * unit)
        return float(rng.choice([c[1], hi, 0.5 * (hi + c[1])]))

    def inside(i):
        c = cl[i]
        return c[0] + (c[1] - c[0]) * float(rng.uniform(0.15, 0.85))

    def a_range():
        i = pick()
        j = min(n - 1, i + int(rng.choice([0, 0, 1, 1, 2, 3])))
        mn = inside(i) if rng.random() < 0.5 else before(i)
        mx = inside(j) if rng.random() < 0.5 else after(j)
        return (mn, mx) if mn < mx else None

    for _ in range(6 if n else 0):
        r = a_range()
        if r:
            si = int(rng.integers(0, n_samples))
            out.append(_clip_args(rng, t, si, resample_ok[si], r[0], r[1] - r[0], samples[si][3]))
        r = a_range()
        if r:
            out.append(("delregion", t, r[0], r[1]))
    for _ in range(20 if n else 0):          # move: the new start aimed like a range's start, or so that the new END lies on an edge
        m = pick() if rng.random() < 0.3 else int(rng.integers(0, n))
        ln = cl[m][1] - cl[m][0]
        i = int(rng.integers(0, n)) if rng.random() < 0.4 else min(n - 1, max(0, m + int(rng.choice([-2, -1, 1, 2]))))
        to = float(rng.choice([inside(i), before(i), after(i) - ln, inside(i) - ln, cl[m][0] + ln * float(rng.uniform(-0.6, 0.6))]))
        if to >= 0.0 and to != cl[m][0]:
            out.append(("move", t, m, to - cl[m][0]))
    for _ in range(10 if n else 0):          # resize: the moving edge aimed into gaps, onto edges, into and past the neighbours
        m = pick() if rng.random() < 0.3 else int(rng.integers(0, n))
        c, ln = cl[m], cl[m][1] - cl[m][0]
        left = bool(rng.integers(0, 2))
        shift = bool(rng.integers(0, 2))
        stretch = bool(rng.integers(0, 2)) and resample_ok[c[5]]
        if family == "inverted":             # the edge dragged past the clip's other edge (resize_limit 0: DESIGN Q11)
            rel = (1 if left else -1) * ln * float(rng.uniform(1.05, 3.0))
            out.append(("resize", t, m, rel, 0.0, 1.0 / 96.0, left, False, False))
            continue
        j = max(0, m - int(rng.choice([1, 1, 2, 3]))) if left else min(n - 1, m + int(rng.choice([1, 1, 2, 3])))
        if rng.random() < 0.25 or j == m:
            to = (c[0] + ln * float(rng.uniform(-0.5, 0.8))) if left else (c[1] - ln * float(rng.uniform(-0.5, 0.8)))
        else:
            to = float(rng.choice([inside(j), before(j), after(j)]))
        rel = to - (c[0] if left else c[1])
        if to < 0.0 or rel == 0.0 or (rel > 0.9 * ln if left else rel < -0.9 * ln):
            continue
        out.append(("resize", t, m, rel, 0.0, 1.0 / 96.0, left, shift, stretch))
    return out


def overlap_script(seed, family="classes"):
    """Edits that land ON clips, aimed at every outcome class of Engine::reserve_track_region (ref_engine.classify) for every
    caller.  The script is grown edit by edit WITH the reference executable: before an edit the reference is asked for the
    track's clip list as it stands (a `clips` line after the script so far), some thirty candidate edits are aimed at it — range
    edges inside clips, in the gaps, exactly on a clip's or a neighbour's edge (the values read back from the reference's list,
    so equal bit for bit) — the reference answers a `query` line for each (the range from the reference's own clip_edit.h,
    libwbref.so), and the candidate of the class this script still lacks most is taken.  In front of every edit stand a `clips`
    and a `query` line, behind it a `clips` line: the comparison is per edit.  Sessions of 2-5 tracks, 10-40 blocks of 128-512
    frames, every storage format, assets at and off the session rate, speeds 1 and != 1; mostly playing with the playhead
    inside the clips (edits prefer the clip under it), sometimes stopped around the edits; runs of 1-4 edits between blocks;
    deletes followed by splits on the same track (the split's right half takes over the freed Pool<Clip> chunk).
    family 'inverted': ranges with min > max — a clip's right edge dragged left past its own start with resize_limit 0, what a
    user interface can reach (a region handed to delete_region backwards is not: the reference asserts min <= max there,
    track.cpp:113, and the product's wbx_engine_delete_region answers WBX_ERR_INVALID) — of which the Q11 ones answer status 3; the class scripts hold none.  Such an edit can leave a clip with max_time < min_time behind,
    and the reference has no defined behaviour for PLAYING one (or for searching a list that holds one): these scripts stop
    the engine first, never play again, and make at most one edit per track — status and clip lists are what they compare."""
    global RATES, SPEEDS
    RATES, SPEEDS = PLAIN_RATES, PLAIN_SPEEDS
    ref = R.O.ref()
    assert ref is not None and R.available(), "the overlap scripts are grown with the reference executable"
    rng = np.random.default_rng([seed, 7 if family == "classes" else 8])
    out_ch = int(rng.choice([1, 2, 2, 2]))
    block = int(rng.choice([128, 128, 256, 384, 512]))
    rate = int(rng.choice([44100, 48000, 48000, 96000]))
    bpm = float(rng.choice([120.0, 97.0, 140.5, 174.0]))
    s = R.Script(out_ch, block, rate, bpm)
    n_tracks = int(rng.integers(2, 6))
    n_blocks = int(rng.integers(10, 41 if block <= 256 else 21))
    if family == "inverted":
        n_blocks = n_tracks + 2
    untouched = list(range(n_tracks))
    beat_frames = rate * 60.0 / bpm
    unit = block / beat_frames
    resample_ok = _samples(rng, s, 0x5EB0000 + seed, n_tracks, rate, out_ch)
    for t in range(n_tracks):
        s.op("track")
        s.op("vol", t, float(np.float32(rng.uniform(-20, 0))))
        s.op("pan", t, float(np.float32(rng.uniform(-1, 1))))
    for t in range(n_tracks):                # 4-7 clips per track, touching or with gaps, the first around the start
        pos = unit * float(rng.uniform(0.0, 2.0))
        for _ in range(int(rng.integers(4, 8))):
            si = int(rng.integers(0, n_tracks))
            length = unit * float(rng.choice([rng.uniform(0.3, 1.0), rng.uniform(1.0, 3.0), rng.uniform(3.0, 7.0)]))   # short between long
            s.op(*_clip_args(rng, t, si, resample_ok[si], pos, length, s.samples[si][3]))
            pos += length + (0.0 if rng.random() < 0.4 else unit * float(rng.uniform(0.1, 1.0)))
    s.op("play")
    playing, done, since = True, 0, 0       # since: the block at which play last started the playhead from 0
    order = [p for p in R.GRID if R.unreachable(*p) is None]
    rng.shuffle(order)
    have = {}
    while done < n_blocks:
        k = int(rng.integers(1, 4))
        s.op("run", k)
        done += k
        ph = (done - since) * unit
        around = rng.random() < 0.25         # the engine stopped around this run of edits
        if family == "inverted":
            around = False
            if playing:
                s.op("stop")
                playing = False
            if not untouched:
                continue
        if around and playing:
            s.op("stop")
        for _ in range(int(rng.choice([1, 1, 2, 3, 4])) if family == "classes" else 1):
            t = int(rng.integers(0, n_tracks)) if family == "classes" else untouched.pop(int(rng.integers(0, len(untouched))))
            lists = R.records_clips(R.run_reference(_with(s, [("clips",)]))[-1][1])
            cl = lists[t]
            if len(cl) < 3 and family == "classes":                  # refill in free space behind the track's last clip
                pos = (cl[-1][1] if cl else ph) + unit * float(rng.uniform(0.1, 1.0))
                for _r in range(3):
                    si = int(rng.integers(0, n_tracks))
                    length = unit * float(rng.uniform(1.0, 4.0))
                    s.op(*_clip_args(rng, t, si, resample_ok[si], pos, length, s.samples[si][3]))
                    pos += length + unit * float(rng.choice([0.0, 0.5]))
                continue
            if rng.random() < 0.15 and family == "classes":          # a delete first: the next split on this track reuses the freed chunk (LIFO)
                s.op("delclip", t, int(rng.integers(0, len(cl))))
                lists = R.records_clips(R.run_reference(_with(s, [("clips",)]))[-1][1])
                cl = lists[t]
            cands = _candidates(rng, cl, t, ph, unit, n_tracks, resample_ok, s.samples, family)
            ranges = []
            for o in cands:
                r = R.edit_range(ref, "ref", cl, s.samples, 60.0 / bpm, o)
                if o[0] == "resize" and r is not None and o[8]:      # the stretched speed stays positive and sane (Q12)
                    d = [R.O.C.c_double() for _ in range(4)]
                    c = cl[o[2]]
                    ref.ref_calc_resize_clip(c[0], c[1], c[2], c[3], float(s.samples[c[5]][2]), float(s.samples[c[5]][3]), o[3], o[4],
                                             o[5], c[0], 60.0 / bpm, int(o[6]), int(o[7]), 1, 0, *[R.O.C.byref(x) for x in d])
                    if not 0.05 < d[3].value < 16.0:
                        r = None
                ranges.append(r)
            keep = [(o, r) for o, r in zip(cands, ranges) if r is not None]
            if not keep:
                continue
            ans = [x[1] for x in R.run_reference(_with(s, [("query", t, r[0], r[1]) for _o, r in keep])) if x[0] == "query"][-len(keep):]
            best, best_rank = None, None
            for (o, r), q in zip(keep, ans):
                cls = R.classify(cl, q, r[0], r[1], r[2])
                caller = {"clip": "add", "move": "move", "delregion": "delregion"}.get(o[0]) or ("resize_left" if o[6] else "resize_right")
                if family == "classes" and cls in ("q11", "inverted", "free"):
                    continue
                if family == "inverted" and cls not in ("q11", "inverted"):
                    continue
                rank = (have.get((caller, cls), 0), order.index((caller, cls)) if (caller, cls) in order else len(order))
                if best_rank is None or rank < best_rank:
                    best, best_rank = (o, r, caller, cls), rank
            if best is None:
                continue
            o, r, caller, cls = best
            have[(caller, cls)] = have.get((caller, cls), 0) + 1
            s.op("clips")
            s.op("query", t, r[0], r[1])
            s.op(*o)
            s.op("clips")
        if around and playing:
            s.op("play")
            since = done                     # play restarts at playhead_start (engine.cpp:70-79)
    s.op("run", 2)
    s.op("clips")
    return s
