"""Sample life scripts: random chains of everything that puts audio into the engine's clip pool and takes it out again —
uploads, derived / normalized / resampled / spliced / loudness-normalized / filtered / convolved / limited / dynamics-
processed / stretched / pitch-shifted samples, recorder takes, bounces, deletes — with placements, playback, measure,
loudness, f0, onsets, tempo, export and mip-maps in between, and the model of what every live sample must hold.
Pure Python (numpy): the generator works on shapes alone (tests/test_sample_scripts.py takes its census without a device),
Contents computes the exact fp32 planes from tests/clipfx_model.py, resample_model.py, splice_model.py, loudness_model.py,
filter_model.py, convolve_model.py, limit_model.py, dynamics_model.py, stretch_model.py and pitch_model.py, and a
consumer's records from f0_model.py and onset_model.py; takes and bounces get theirs from the rig that runs the script
(tests/test_gpu_sample_scripts.py), since they depend on the inputs fed and on the oracle engine's render.
TEST INFRASTRUCTURE — nothing here is shipped.

Every sample carries a bound of |x| kept on shapes alone (Meta.amp): a filter's is amp x the L1 norm of its cascade's
impulse response (filter_l1), a convolution's amp x amp x taps x gain, a limit's its ceiling, a dynamics call's amp x |drive|
x makeup, a stretch's its source's (two half-windows that sum to 1), a pitch shift's amp x the largest L1 norm of a phase of
its conversion table (pitch_l1).  tests/test_sample_scripts.py holds the contents model against these bounds.

A script is a list of tuples; `key` names a sample inside the script (the product's ids are the rig's business):
    ("add", key, fmt, channels, rate, frames, interleaved, seed, flavour)      flavour: "noise", or for F32 "tone" / "clicks"
                                                     (upload_planes), so that f0 hops are voiced and onsets fire
    ("derive", key, src, first, n, reverse, mode, gain, fade_in, fade_out, shape_in, shape_out)
    ("normalize", key, src, target_peak, first, n)
    ("resample", key, src, dst_rate, quality, first, n)
    ("splice", key, channels, n_frames, parts, status)    parts: tuples of splice_model.Part's fields, `src` a script key;
                                                     every source F32 and of ONE rate, mono and stereo mixed through the
                                                     channel modes that yield `channels`.  status 0, or what a REFUSED
                                                     splice returns (key None): -3 where a part names an i16 sample, -4
                                                     where two sources differ in rate
    ("loudnorm", key, src, target_lufs, ceiling, first, n, status)    a true-peak ceiling in (0, 1] is always set;
                                                     n >= 4 hops and oversampling * n <= MAX_FRAMES.  status 0, or -4 of
                                                     a REFUSED one (key None): a range shorter than 4 hops
    ("take", key, track, kind, index, first_input_block, n_blocks, beat)       kind: record_model.MONO / STEREO
    ("bounce", keys, lo, hi, sources)                sources: ("track", t, "post" | "pre") / ("master",), one key each
    ("place", pid, src, track, lo, hi, start_offset) / ("unplace", pid)        a take's clip is placement ("take", key)
    ("play", beat, n_blocks)
    ("measure", src, first, n) / ("export", src, fmt, clamp, first, n) / ("mip", src, quality)
    ("loudness", src, true_peak, first, n)           any F32 sample, any range (below one hop: no hop, integrated -inf);
                                                     with true_peak oversampling * n <= MAX_FRAMES
    ("delete", src, status)                          status: 0, or -4 while a clip names the sample
The six newer producers: (kind, key, src, first, n, ..., status), every result F32 at its source's rate; status 0, or what
a REFUSED one returns (key None), pinned from the feature model's check_args and include/wbx.h:
    ("filter", key, src, first, n, tail_frames, coef, status)       coef: 1 .. 8 stages of 5 (filter_menu); -3: an i16 source
    ("convolve", key, src, first, n, ir, ir_first, taps, out_first, out_frames, gain_db, status)
                                                     ir: another live F32 sample of the source's rate, mono or stereo;
                                                     -4: a response of another rate, -3: an i16 response
    ("limit", key, src, first, n, ceiling_db, drive_db, A, H, R, status)       -3: an i16 source
    ("dynamics", key, src, first, n, table, sense, key_sample, key_first, drive, key_gain, makeup, A, H, R, status)
                                                     table: dynamics_model.table's arguments; key_sample None (keyed by
                                                     itself) or as a response; -4: a key of another rate, -3: an i16 key
    ("stretch", key, src, first, n, out_frames, window, tolerance, status)     -3: an i16 source, or out_frames > 8 n
    ("pitch", key, src, first, n, out_frames, num, den, quality, window, tolerance, status)
                                                     -4: a ratio that reduces to 1, -3: one beyond 4 : 1 either way
The three consumers make no sample; the rig compares their records and info with the model and, as after every op, every
live sample and the pool:
    ("f0", src, window, hop, tau_min, tau_max, threshold, first, n)
    ("onsets", src, hop, floor_power, threshold, delta, w, a, first, n)
    ("tempo", src, hop, floor_power, window_hops, step_hops, lag_min, lag_max, threshold, first, n)
"""
from __future__ import annotations

import collections
import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import clipfx_model as FX
import convolve_model as CV
import dynamics_model as DYN
import f0_model as F0
import filter_model as FM
import limit_model as LIM
import loudness_model as LM
import onset_model as ON
import pitch_model as PM
import record_model as RM
import resample_model as RS
import splice_model as SP
import stretch_model as ST

F, RATE, BPM, TRACKS, INPUTS = 128, 48000, 120.0, 4, 2
CHUNK, SPARE = 700, 4                 # the recorder's chunks (frames) and how many it keeps ahead
G = 64 << 10
SEEDS = tuple(range(16))
N_OPS = 160
BUDGET = 40 << 20                     # bytes a script may allocate in all, recorder chunks included: under the first slab's tail
UNIT = (F / RATE) / (60.0 / BPM)      # beats per block
RATES = (44100, 48000, 96000, 32000)
QUALITIES = (RS.FAST, RS.GOOD, RS.BEST)
EXPORT_FORMATS = ("i16", "i24", "i24_x8", "i32", "f32")
MAX_FRAMES = 200_000                  # of a result (the longest menu entry is below it)
# clip lengths in frames.  Rows are (frames + 16) * 4 bytes rounded up to 256; a stereo clip is two rows rounded up to granules.
LENGTHS = (1, 7, 37,                                  # tiny
           48, 49, 1008, 1009, 4080,                  # (frames + 16) * 4 a multiple of 256, and one frame more
           8176, 8177, 24560, 24561,                  # stereo rows that fill 1 / 3 granules exactly, and one frame more
           300, 2500, 12000,
           70001, 131056, 190000)                     # stereo: 8.5 / 16 / 23.2 granules — the gap in front of the clip is active
# a splice result's lengths: the kernel's tile is 512 frames; 70001 stereo frames are an 8.5-granule clip with an active gap
SPLICE_LENGTHS = (1, 511, 512, 513, 2573, 70001)
SPLICE_PARTS = 6                      # at most (wbx_clip_splice takes 65536)
SPLICE_AMP = 1.15                     # the most the parts' amp x |gain| may add up to
LOUD_OPS = 10                         # loudness measurements a script may hold, normalizations included: the numpy twin takes
                                      # 0.2 .. 1 s for each, whatever the range (one python step per frame of three hops)
LONG_SHARE = 0.3                      # of the derives, normalizations and conversions: of 4 hops and more
# What a conversion may add to a bound of |x|: between the samples of noise whose peak is pinned (a peak normalization's
# result) the interpolated wave reaches 1.75 times the peak.  A source whose bound times this leaves audio range is not
# converted; a bounce's bound is the mixer's nominal 1.0, far above the sessions' levels, and stays convertible.
RESAMPLE_OVERSHOOT = 1.8
# factors on a loudness op's choice of source: results of the device's own producers, rarer among the long samples than uploads
MADE_ON_THE_DEVICE = dict(splice=8.0, derive=4.0, normalize=4.0, resample=4.0, filter=8.0)
REFUSED_I16, REFUSED_RATES, REFUSED_SHORT = -3, -4, -4   # as tests/test_gpu_splice.py and test_gpu_loudness.py pin them
REFUSED_RATIO, REFUSED_ONE = -3, -4   # a stretch beyond 8 n or a pitch ratio beyond 4 : 1 / a pitch ratio that reduces to 1
TARGETS_LOUD, TARGETS_SOFT = (-6.0, 0.0), (-42.0, -30.0)   # LUFS: the ceiling binds / the target does (noise of -10 .. -25)
OLD_PRODUCERS = ("add", "derive", "normalize", "resample", "take", "bounce", "splice", "loudnorm")
NEW_PRODUCERS = ("filter", "convolve", "limit", "dynamics", "stretch", "pitch")   # each: (kind, key, src, first, n, ..., status)
PRODUCERS = OLD_PRODUCERS + NEW_PRODUCERS
CONSUMERS = ("f0", "onsets", "tempo")                 # (kind, src, ..., first, n): records and an info, no sample
HAVE_A_STATUS = ("splice", "loudnorm") + NEW_PRODUCERS   # ops whose last field is the status the product must return
KINDS = PRODUCERS + ("place", "unplace", "play", "measure", "loudness", "export", "mip", "delete") + CONSUMERS
WEIGHTS = dict(add=7, derive=6, normalize=2.5, resample=7, take=3.5, bounce=3, splice=7, loudnorm=5.5, place=7, unplace=2,
               play=7, measure=2, loudness=4, export=2, mip=2, delete=9,
               filter=5, convolve=5.5, limit=5, dynamics=5.5, stretch=5, pitch=5, f0=3.5, onsets=3, tempo=3)
FLAVOURS = ("noise", "tone", "clicks")                # of an upload: upload_planes

# ---- the size menus of the six newer producers and the three consumers: the smallest at which each kernel can still go wrong,
# from the features' own tests (tests/test_gpu_filter.py .. test_gpu_onsets.py), mixed with random lengths.


def tile_edges(T):
    """1 frame, around a lane's 8 frames, around one tile of T frames, two tiles and a part"""
    return (1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 5)


FILTER_TOTALS = (511, 512, 513, 32767, 32768, 32769)  # n + tail: around one chunk, around the 64 chunks one wave owns
FILTER_TAILS = (0, 1, 700)
CONV_TAPS = (1, 2, 7, CV.SEGMENT - 1, CV.SEGMENT, CV.SEGMENT + 1, 2 * CV.SEGMENT + 3)
CONV_OUT = tile_edges(CV.TILE)                        # out_frames; or the full ring-out ("full")
CONV_WORK = 60_000_000                                # n x L of one convolution: numpy's twin takes 0.24 s for 70001 x 2048
CURVE_SIZES = tile_edges(LIM.TILE)                    # n of a limit and of a dynamics call
CURVE_TERMS = (1, 2, 7, LIM.SEGMENT - 1, LIM.SEGMENT, LIM.SEGMENT + 1, 2 * LIM.SEGMENT + 3)   # A + H + R
CURVE_WORK = 60_000_000                               # n x (A + H + R): the twin runs one vector step per term
STRETCH_WINDOWS = (32, 64, 256, 2048)
STRETCH_TOLERANCES = ("0", "Hs-1", "Hs", "Hs+1", "512")
STRETCH_FRAMES = 24_000                               # out_frames of a stretch, m' of a pitch: the twin's position search takes
                                                      # one python step per frame of a searched step
PITCH_RATIOS = ((9, 8), (8, 9), (3, 2), (2, 1), (1, 2), (4, 1), (1265, 1194))   # the last: L = 1194, the large table
F0_WINDOWS = (64, 72, 256, 1024)
F0_TAU_MAX = (100, 511, 512, 700)                     # tau_max + 1 lags: below, at (511, 512) and across a wave's 512
F0_HOPS = (1, 7, 64, 1000)
F0_TERMS = 30_000_000                                 # hops x W x (tau_max + 1) of one call (the twin: ~6 ns a term) ...
F0_TERMS_A_SCRIPT = 120_000_000                       # ... and of a script's f0 and tempo calls together, as LOUD_OPS caps loudness
ONSET_HOPS = (64, 192, 256, 1024, 2112)
TEMPO_SHAPES = ((64, 1, 2, 16), (72, 7, 4, 100), (64, 64, 8, 40))   # (window, step, lag_min, lag_max), in hops
DYN_TABLES = ((DYN.COMPRESS, -24.0, 4.0, 6.0, -np.inf), (DYN.COMPRESS, -12.0, np.inf, 0.0, -20.0),
              (DYN.GATE, -20.0, 4.0, 6.0, -40.0), (DYN.GATE, -30.0, 10.0, 0.0, -np.inf))   # dynamics_model.table's arguments


@functools.lru_cache(maxsize=None)
def dyn_table(spec):
    return DYN.table(*spec)


@functools.lru_cache(maxsize=None)
def filter_menu(rate):
    """cascades of 1 .. 8 stages at `rate`, each a tuple of 5-tuples (hashable: an op holds it)"""
    four, eight, d = FM.four_stages(rate), FM.eight_stages(rate), FM.design
    shelf = lambda f, gain: d(rate, "highshelf", f * rate, 0.7, gain)
    three = [shelf(.2, .5), shelf(.1, .7), shelf(.3, .6)]
    # the first five are gentle (an L1 norm of 1.0 .. 2.4: an upload's 0.5 stays in range; the 20 Hz high-pass has its poles
    # next to z = 1, where the carry matters), the feature tests' own cascades (6.3 .. 8.5) go to whoever is quiet enough
    menu = [[d(rate, "lowpass", 0.2 * rate)],
            [d(rate, "highpass", 20.0, 0.5), shelf(.2, .5)],
            three,
            [d(rate, "highpass", 20.0, 0.5), shelf(.2, .5), d(rate, "peak", 60.0, 2.0, 0.7), d(rate, "lowpass", 0.4 * rate, 0.5)],
            three + [shelf(.05, .8), shelf(.15, .8), d(rate, "lowpass", 0.3 * rate, 0.5), d(rate, "peak", 0.1 * rate, 0.7, 0.7),
                     d(rate, "lowshelf", 0.02 * rate, 0.7, 0.8)],
            four, eight[:6], eight]
    return tuple(tuple(tuple(float(c) for c in stage) for stage in k) for k in menu)


@functools.lru_cache(maxsize=None)
def pitch_l1(num, den, quality):
    """what a pitch shift's conversion may add to a bound of |x|, whatever the contents: the largest L1 norm of a phase of its
    table, 1.75 .. 2.53.  (RESAMPLE_OVERSHOOT, measured on noise, does not hold here: a pitch-shifted upload reached 1.854
    times its bound.)"""
    L, M = PM.ratio(num, den)
    taps = np.abs(np.asarray(PM.table(L, M, quality), dtype=np.float64)).reshape(L, -1)
    return float(taps.sum(axis=1).max()) * (1.0 + 1e-6)


@functools.lru_cache(maxsize=None)
def filter_l1(coef):
    """the L1 norm of a cascade's impulse response, from the model: what it may add to a bound of |x|, whatever the contents.
    2^19 frames of ring-out; the last 64 chunks hold nothing any more"""
    n = 1 << 19
    h = np.abs(FM.filter_plane(np.ones(1, dtype=np.float32), 0, 1, n - 1, np.array(coef)).astype(np.float64))
    assert h[-64 * FM.CHUNK:].sum() <= 1e-9 * h.sum(), "the impulse response has not died away"
    return float(h.sum()) * (1.0 + 1e-6)


def row_bytes(frames: int, fmt: str = "f32") -> int:
    return -(-(frames + 16) * (2 if fmt == "i16" else 4) // 256) * 256


def body_bytes(frames: int, channels: int, fmt: str = "f32") -> int:
    return -(-row_bytes(frames, fmt) * channels // G) * G


def pool_bounds(frames: int, channels: int, fmt: str = "f32") -> Tuple[int, int]:
    """what a clip takes from the pool: its body, and its body plus the widest gap in front of it"""
    body = body_bytes(frames, channels, fmt)
    return body, body + (min(16, body // G // 8 + 1) - 1) * G


def frames_that_fit(nbytes: int, channels: int) -> int:
    """pool_bounds the other way round: the most F32 frames of a clip that takes no more than nbytes from the pool, gap in
    front of it included (0: not even one frame)"""
    lo, hi = 0, nbytes // (4 * channels)              # pool_bounds grows with the frames: bisect
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if pool_bounds(mid, channels)[1] <= nbytes else (lo, mid - 1)
    return lo


@dataclasses.dataclass
class Meta:
    kind: str
    fmt: str
    channels: int
    rate: int
    frames: int
    lineage: Tuple[str, ...]          # the producers behind it, oldest first, its own last
    amp: float = 1.0                  # a bound of |x|
    quiet: bool = False               # may be all zero (a bounce, or made from one): never normalized
    gaps: bool = False                # may hold long stretches of zeros or next to nothing (frames of a splice that no part
                                      # of a loud source covers, what a gate closed on, noise convolved with noise: far
                                      # below its bound, never all zero): neither peak- nor loudness-normalized
    refs: int = 0                     # clips that name it
    flavour: str = "noise"            # of the upload behind it, while the newer producers alone stand between: what f0
                                      # ("tone") and onsets / tempo ("clicks") look for first

    @property
    def editable(self):
        return self.fmt == "f32"


def upload_planes(seed: int, fmt: str, channels: int, frames: int, flavour: str = "noise") -> List[np.ndarray]:
    """non-zero noise: whatever extent an upload reuses holds junk afterwards.  Two more flavours of an F32 upload, both
    within 0.5 and deterministic from the seed: "tone", three harmonics of a period of 30 .. 90 frames on noise of 0.01
    (voiced hops for f0), and "clicks", decaying noise bursts every 3000 .. 6000 frames on noise of 0.002 (onsets)"""
    if fmt == "f32" and flavour != "noise":
        rng = np.random.default_rng([0xADD, seed, FLAVOURS.index(flavour)])
        i = np.arange(frames, dtype=np.float64)
        out = []
        if flavour == "tone":
            period = rng.uniform(30.0, 90.0)
            for _ in range(channels):
                ph = rng.uniform(0.0, 1.0, 3)
                x = sum(a * np.sin(2.0 * np.pi * ((h + 1) * i / period + p)) for h, (a, p) in enumerate(zip((0.25, 0.12, 0.06), ph)))
                out.append(x + rng.uniform(-0.01, 0.01, frames))
        else:
            every, decay = int(rng.integers(3000, 6001)), rng.uniform(40.0, 200.0)
            at0 = int(rng.integers(0, max(1, min(every, frames) // 2)))
            env = np.where(i >= at0, np.exp(-((i - at0) % every) / decay), 0.0)
            out = [0.45 * env * rng.uniform(-1.0, 1.0, frames) + rng.uniform(-0.002, 0.002, frames) for _ in range(channels)]
        return [np.ascontiguousarray(p, dtype=np.float32) for p in out]
    rng = np.random.default_rng([0xADD, seed])
    if fmt == "i16":
        return [(rng.integers(1, 20000, frames) * rng.choice([-1, 1], frames)).astype(np.int16) for _ in range(channels)]
    x = [rng.uniform(0.05, 0.5, frames).astype(np.float32) * rng.choice([-1, 1], frames).astype(np.float32) for _ in range(channels)]
    return [np.ascontiguousarray(p, dtype=np.float32) for p in x]


AMP: Dict[Tuple[int, int], float] = {}  # (seed, key) -> the bound of |x| the generator kept for that sample (Meta.amp): what
                                        # tests/test_sample_scripts.py holds the contents model against


@functools.lru_cache(maxsize=None)
def make_script(seed: int, n_ops: int = N_OPS):
    """-> (ops, facts): facts is what the census counts"""
    rng = np.random.default_rng([0x11FE, seed])
    live: Dict[int, Meta] = {}
    order: List[int] = []             # live keys, oldest first
    placed: Dict[object, tuple] = {}  # pid -> (key, track, lo, hi, start_offset, tail frames at the session rate)
    ops: List[tuple] = []
    facts = collections.Counter()
    pending_holes: List[int] = []     # bytes of the deletes of a sample that was not the newest live one
    keys = iter(range(1 << 30))
    state = dict(beat=1.0, total=0, input_block=0, pid=0, loud=0, f0_terms=0)
    turns = collections.Counter()      # of every menu: cycle() deals a menu's entries in turn, from a start of the seed's own

    def fresh(meta: Meta, sources=None) -> int:
        """sources: the distinct source keys of a splice (every other producer's one source is in its lineage)"""
        key = next(keys)
        live[key] = meta
        order.append(key)
        if n_ops == N_OPS:
            AMP[seed, key] = meta.amp
        size = pool_bounds(meta.frames, meta.channels, meta.fmt)
        state["total"] += size[1]
        for chain in [meta.lineage] if sources is None else [live[s].lineage + (meta.kind,) for s in sources]:
            facts["source:" + "->".join(chain[-3:])] += len(chain) >= 3
            if len(chain) >= 2:
                facts["source:" + "->".join(chain[-2:])] += 1
                facts["as_source:" + chain[-2]] += 1
        for h in list(pending_holes):
            if size[1] <= h:
                pending_holes.remove(h)
                facts["hole_refilled"] += 1
                facts["hole_refilled:" + meta.kind] += 1
        return key

    def room(frames, channels, fmt="f32"):
        return state["total"] + pool_bounds(frames, channels, fmt)[1] <= BUDGET - (4 << 20)

    def region(beats):
        lo = state["beat"]
        state["beat"] = lo + beats + 4 * UNIT
        return lo

    def pick_source(editable=True, loud=False, chain=(), ok=None, boost=None):
        """ok(meta): who may be drawn at all; boost(meta): a factor on the weight of its kind"""
        c = [k for k in order if (live[k].editable or not editable) and not (loud and (live[k].quiet or live[k].gaps)) and
             (ok is None or ok(live[k]))]
        if not c:
            return None
        w = np.array([{"take": 5.0, "bounce": 4.0, "splice": 4.0, "resample": 2.5, "derive": 2.0, "normalize": 2.0,
                       "loudnorm": 2.0, "filter": 3.0, "convolve": 3.0, "limit": 3.0, "dynamics": 3.0, "stretch": 3.0,
                       "pitch": 3.0}.get(live[k].kind, 1.0) *
                      (6.0 if chain and live[k].lineage[-len(chain):] == chain else 1.0) *
                      (boost(live[k]) if boost else 1.0) for k in c])
        return c[rng.choice(len(c), p=w / w.sum())]

    def enough(m: Meta):
        """4 hops and more: a range of it has blocks for the gate, and may be normalized to a loudness"""
        return m.frames >= 4 * LM.hop_frames(m.rate)

    def off_rate_newcomer(m: Meta):
        """a result of one of the newer producers, of another rate than the session's: the padding behind it is read only
        when a placement of it plays through its end"""
        return m.kind in HAVE_A_STATUS and m.rate != RATE

    def pick_range(m: Meta, most=MAX_FRAMES, least=1):
        top = min(m.frames, most)
        n = int(rng.integers(min(least, top), top + 1)) if rng.random() < .6 else top
        first = int(rng.integers(0, m.frames - n + 1))
        if rng.random() < .3:
            first = m.frames - n      # up to the source's last frame
        return first, n

    def op_add(long=False):
        have_i16 = any(not m.editable for m in live.values())   # (what the refusals of the newer producers name)
        fmt = "i16" if rng.random() < (.15 if have_i16 else .4) and not long else "f32"
        channels, rate = int(rng.integers(1, 3)), int(rng.choice(RATES[:2]))
        menu = [n for n in LENGTHS if n >= 19200] if long else LENGTHS    # (long: 4 hops of loudness and more)
        frames = int(menu[rng.integers(len(menu))])
        if not room(frames, channels, fmt):
            frames = int(LENGTHS[rng.integers(8)])
        flavour = str(rng.choice(FLAVOURS, p=[.5, .25, .25])) if fmt == "f32" else "noise"
        key = fresh(Meta("add", fmt, channels, rate, frames, ("add",), amp=0.5, flavour=flavour))
        ops.append(("add", key, fmt, channels, rate, frames, bool(rng.integers(2)), int(rng.integers(1 << 30)), flavour))

    def pick_long(ok_too=None, **how):
        """now and then an edit of 4 hops and more of a sample that has them: what the loudness ops can measure afterwards
        -> (source, the least frames to take), (None, 1) otherwise"""
        fit = lambda m: enough(m) and (ok_too is None or ok_too(m))
        src = pick_source(ok=fit, **how) if rng.random() < LONG_SHARE else None
        return (src, 1) if src is None else (src, 4 * LM.hop_frames(live[src].rate))

    def op_derive():
        src, least = pick_long()
        if src is None and rng.random() < .3:             # (resample -> derive -> resample: a chain the census wants)
            src = pick_source(ok=lambda m: m.kind in ("resample", "bounce"))
        src = pick_source() if src is None else src
        if src is None:
            return op_add()
        m = live[src]
        first, n = pick_range(m, least=least)
        mode = int(rng.choice(FX.MODES_FOR[m.channels]))
        out_ch = FX.out_channels(m.channels, mode)
        if not room(n, out_ch):
            return op_delete()
        top = min(1.1, 1.15 / m.amp)
        gain = float(np.float32(rng.uniform(0.3, top) * rng.choice([-1, 1])))
        fi, fo = (int(rng.integers(0, n + 1)) if rng.random() < .5 else 0 for _ in range(2))
        key = fresh(Meta("derive", "f32", out_ch, m.rate, n, m.lineage + ("derive",), m.amp * abs(gain), m.quiet, m.gaps))
        ops.append(("derive", key, src, first, n, bool(rng.integers(2)), mode, gain, fi, fo, int(rng.integers(3)), int(rng.integers(3))))

    def op_normalize():
        src, least = pick_long(loud=True)
        src = pick_source(loud=True) if src is None else src
        if src is None:
            return op_add()
        m = live[src]
        first, n = pick_range(m, least=least)
        if n < 8:
            first, n = 0, m.frames
        if n < 2 or not room(n, m.channels):
            return op_delete()
        target = float(np.float32(rng.uniform(0.2, 1.0)))
        key = fresh(Meta("normalize", "f32", m.channels, m.rate, n, m.lineage + ("normalize",), target))
        ops.append(("normalize", key, src, target, first, n))

    def op_resample():
        in_range = lambda m: m.quiet or m.amp * RESAMPLE_OVERSHOOT <= 1.2
        src, least = pick_long(ok_too=in_range)
        if src is None and rng.random() < .4:             # (resample -> derive -> resample: a chain the census wants)
            src = pick_source(ok=lambda m: in_range(m) and m.lineage[-2:] == ("resample", "derive"))
        if src is None:
            src = pick_source(chain=("resample", "derive"), ok=in_range)
        if src is None:
            return op_add()
        m = live[src]
        dst = int(rng.choice([r for r in RATES if r != m.rate]))
        first, n = pick_range(m, most=MAX_FRAMES * m.rate // dst - 1, least=least + 64 * (least > 1))   # (4 hops of dst, too)
        n_out = RS.out_frames(m.rate, dst, n)
        if not room(n_out, m.channels):
            return op_delete()
        key = fresh(Meta("resample", "f32", m.channels, dst, n_out, m.lineage + ("resample",), m.amp * RESAMPLE_OVERSHOOT, m.quiet, m.gaps))
        ops.append(("resample", key, src, dst, int(rng.choice(QUALITIES)), first, n))

    def draw_part(src, channels, n_frames, n=None):
        """a part of `src` somewhere in a result of n_frames: menu and random mixed, as the lengths are -> Part fields, gain 1"""
        m = live[src]
        most = min(m.frames, n_frames)
        if n is None:
            n = most if rng.random() < .35 else int(rng.integers(1, most + 1))
        first = m.frames - n if rng.random() < .3 else int(rng.integers(0, m.frames - n + 1))
        free, r = n_frames - n, rng.random()
        if r < .2:
            at = 0
        elif r < .4:
            at = free                                     # ends on the result's last frame
        elif r < .65 and n >= 2 and n_frames > SP.TILE:   # straddles a tile edge (where the result's end lets it)
            edge = SP.TILE * int(rng.integers(1, -(-n_frames // SP.TILE)))
            at = min(max(edge - int(rng.integers(1, n)), 0), free)
        else:
            at = int(rng.integers(0, free + 1))
        mode = int(rng.choice([md for md in FX.MODES_FOR[m.channels] if FX.out_channels(m.channels, md) == channels]))
        fi, fo = (int(rng.integers(0, n + 1)) if rng.random() < .4 else 0 for _ in range(2))
        return [src, first, n, at, bool(rng.integers(2)), mode, 1.0, fi, fo, int(rng.integers(3)), int(rng.integers(3))]

    def follow_with_delete(named, fact, every=False):
        """after a refusal: a delete of one of its sources that no clip names must succeed (a pin left behind refuses it);
        `every`: of each of them (a call of two sources pins both)"""
        c = [k for k in dict.fromkeys(named) if not live[k].refs]
        if c and rng.random() < .8:
            facts[fact] += 1
            facts[fact + "_of_both"] += every and len(c) == 2
            for k in c if every else [c[rng.integers(len(c))]]:
                do_delete(k)

    def refused_splice():
        """-> whether one could be drawn: a part that names an i16 sample behind parts that are in order, or F32 sources of
        two rates"""
        f32 = [k for k in order if live[k].editable]
        i16 = [k for k in order if not live[k].editable]
        if not f32:
            return False
        good = f32[rng.integers(len(f32))]
        other = [k for k in f32 if live[k].rate != live[good].rate]
        if i16 and (not other or rng.random() < .85):
            bad, status = i16[rng.integers(len(i16))], REFUSED_I16
        elif other:
            bad, status = other[rng.integers(len(other))], REFUSED_RATES
        else:
            return False
        channels, n_frames = int(rng.integers(1, 3)), int(rng.choice(SPLICE_LENGTHS[1:5]))
        named = [good] * int(rng.integers(status == REFUSED_RATES, 3)) + [bad]
        parts = [draw_part(k, channels, n_frames) for k in named]
        for p in parts:
            p[6] = 0.5
        facts["refused_splice:%d" % status] += 1
        ops.append(("splice", None, channels, n_frames, tuple(tuple(p) for p in parts), status))
        follow_with_delete(named, "refused_splice_then_delete")
        return True

    def op_splice():
        if rng.random() < .18 and refused_splice():
            return
        off = rng.random() < .3                               # (takes and bounces are all at the session's rate)
        lead = pick_source(ok=lambda m: m.rate != RATE) if off else None
        lead = pick_source() if lead is None else lead
        if lead is None:
            return op_add()
        rate = live[lead].rate
        channels = int(rng.integers(1, 3))
        n_frames = int(SPLICE_LENGTHS[rng.integers(len(SPLICE_LENGTHS))]) if rng.random() < .75 else int(rng.integers(2, 4000))
        if rng.random() < .12:
            channels, n_frames = 2, SPLICE_LENGTHS[-1]        # 8 granules and more
        # a result of 4 hops and more that ONE part of a loud source covers whole: what a loudness normalization can take
        solid = pick_source(loud=True, ok=enough) if rng.random() < .25 else None
        if solid is not None:
            lead, rate, hop = solid, live[solid].rate, LM.hop_frames(live[solid].rate)
            longest = min(live[lead].frames, SPLICE_LENGTHS[-1])
            n_frames = longest if rng.random() < .3 else int(rng.integers(4 * hop, longest + 1))
        if not room(n_frames, channels):
            solid, n_frames = None, int(SPLICE_LENGTHS[rng.integers(5)])
        if not room(n_frames, channels):
            return op_delete()
        named = [lead] + [pick_source(ok=lambda m: m.rate == rate, boost=lambda m: 5.0 if m.kind == "pitch" else 1.0)
                          for _ in range(int(rng.integers(0, SPLICE_PARTS)))]
        parts = []
        if solid is not None:
            parts, named = [draw_part(lead, channels, n_frames, n=n_frames)], named[1:]
        if len(named) >= 2 and rng.random() < .4:            # a crossfade: two parts over the same frames, one going, one coming
            a = draw_part(named[0], channels, min(n_frames, live[named[1]].frames))
            b = draw_part(named[1], channels, n_frames, n=a[2])
            a[4] = b[4] = False
            a[7], a[8], b[3], b[7], b[8] = 0, a[2], a[3], a[2], 0
            parts, named = [a, b], named[2:]
            facts["splice_crossfade"] += 1
        parts += [draw_part(k, channels, n_frames) for k in named]
        # the bound of the result on shapes alone: sum of amp x |gain| <= SPLICE_AMP (wherever the parts lie)
        g = rng.uniform(0.3, 1.0, len(parts))
        total = float(sum(live[p[0]].amp * x for p, x in zip(parts, g)))
        g = g * min(1.0, 0.999 * SPLICE_AMP / total)
        for p, x in zip(parts, g):
            p[6] = float(np.float32(x * rng.choice([-1, 1])))
        amp = float(sum(live[p[0]].amp * abs(p[6]) for p in parts))
        assert amp <= SPLICE_AMP
        covered, sounding = np.zeros(n_frames, dtype=bool), np.zeros(n_frames, dtype=bool)
        for p in parts:
            covered[p[3]:p[3] + p[2]] = True
            if not (live[p[0]].quiet or live[p[0]].gaps):     # (noise under random gains: parts never cancel)
                sounding[p[3]:p[3] + p[2]] = True
            facts["splice_part_at_0"] += p[3] == 0
            facts["splice_part_to_the_end"] += p[3] + p[2] == n_frames
            facts["splice_part_straddles_a_tile"] += p[3] // SP.TILE != (p[3] + p[2] - 1) // SP.TILE
        srcs = list(dict.fromkeys(p[0] for p in parts))
        facts["splice_gap"] += not covered.all()
        facts["splice_both_channel_counts"] += len({live[k].channels for k in srcs}) == 2
        facts["splice_8_granules"] += body_bytes(n_frames, channels) >= 8 * G
        if n_frames in SPLICE_LENGTHS:
            facts["splice_frames:%d" % n_frames] += 1
        facts["splice_sounding_4_hops"] += bool(sounding.all()) and n_frames >= 4 * LM.hop_frames(rate)
        key = fresh(Meta("splice", "f32", channels, rate, n_frames, live[srcs[0]].lineage + ("splice",), amp,
                         all(live[k].quiet for k in srcs), not sounding.all()), sources=srcs)
        ops.append(("splice", key, channels, n_frames, tuple(tuple(p) for p in parts), 0))

    def op_loudnorm():
        if state["loud"] >= LOUD_OPS:
            return op_measure()
        refused = rng.random() < .15
        if refused:                                       # (no clip: the delete can follow)
            src = pick_source(loud=True, boost=lambda m: 1.0 if m.refs else 4.0)
        else:                                             # a long result of one of the device's producers first
            want = str(rng.choice(list(MADE_ON_THE_DEVICE), p=np.array(list(MADE_ON_THE_DEVICE.values())) / sum(MADE_ON_THE_DEVICE.values())))
            src = pick_source(loud=True, ok=lambda m: enough(m) and m.kind == want)
            src = pick_source(loud=True, ok=enough, boost=lambda m: MADE_ON_THE_DEVICE.get(m.kind, 1.0)) if src is None else src
        if src is None:
            return op_add(long=True)
        m = live[src]
        hop, cap = LM.hop_frames(m.rate), MAX_FRAMES // LM.oversampling(m.rate)
        ceiling = float(np.float32(rng.uniform(0.1, 1.0)))
        target = float(rng.uniform(*(TARGETS_LOUD if rng.random() < .5 else TARGETS_SOFT)))
        if refused:                                       # shorter than 4 hops: measured, then refused
            n = min(m.frames, int(rng.choice([4 * hop - 1, hop, int(rng.integers(1, 4 * hop))])))
            first = m.frames - n if rng.random() < .3 else int(rng.integers(0, m.frames - n + 1))
            facts["refused_loudnorm"] += 1
            ops.append(("loudnorm", None, src, target, ceiling, first, n, REFUSED_SHORT))
            return follow_with_delete([src], "refused_loudnorm_then_delete")
        most = min(m.frames, cap)
        n = int(rng.choice([4 * hop, most, int(rng.integers(4 * hop, most + 1))]))
        fits = [k for k in (frames_that_fit(h, m.channels) for h in pending_holes) if k >= 4 * hop]
        if fits and rng.random() < .9:                   # the longest result that takes over a freed extent
            n = min(max(fits), most)
        first = m.frames - n if rng.random() < .3 else int(rng.integers(0, m.frames - n + 1))
        if not room(n, m.channels):
            return op_delete()
        state["loud"] += 1
        key = fresh(Meta("loudnorm", "f32", m.channels, m.rate, n, m.lineage + ("loudnorm",), ceiling))
        ops.append(("loudnorm", key, src, target, ceiling, first, n, 0))

    def op_loudness():
        if state["loud"] >= LOUD_OPS:
            return op_measure()
        true_peak = bool(rng.random() < .5)
        no_hop = rng.random() < .2                        # the edge; every other measurement has hops, most have blocks
        if no_hop:
            src = pick_source()
        else:                                             # a long result of one of the device's producers, of another rate first
            want = str(rng.choice(list(MADE_ON_THE_DEVICE), p=np.array(list(MADE_ON_THE_DEVICE.values())) / sum(MADE_ON_THE_DEVICE.values())))
            boost = lambda m: MADE_ON_THE_DEVICE.get(m.kind, 1.0) * (5.0 if m.rate in (96000, 32000) else 2.0 if m.rate != RATE else 1.0)
            src = pick_source(ok=lambda m: enough(m) and m.kind == want, boost=boost)
            src = pick_source(ok=enough, boost=boost) if src is None else src
            if src is None:
                return op_add(long=True)                  # (nothing of 4 hops is alive yet)
        if src is None:
            return op_add()
        state["loud"] += 1
        m = live[src]
        hop = LM.hop_frames(m.rate)
        most = min(m.frames, MAX_FRAMES // LM.oversampling(m.rate)) if true_peak else m.frames
        if no_hop or most < hop:
            n = int(rng.integers(1, min(hop, most + 1)))
        else:                                             # the whole sample, anything above a hop, a few blocks, no block yet
            n = int(rng.choice([most, int(rng.integers(hop, most + 1)), min(most, int(rng.integers(4 * hop, 8 * hop))),
                                int(rng.integers(hop, 4 * hop))], p=[.3, .3, .3, .1]))
        first = m.frames - n if rng.random() < .3 else int(rng.integers(0, m.frames - n + 1))
        hops = n // hop
        facts["loudness_no_hop"] += hops == 0
        facts["loudness_hops"] += hops >= 1
        facts["loudness_blocks"] += hops >= 4
        if hops >= 1:
            facts["loudness_hops:" + m.kind] += 1
            facts["loudness_hops:%d" % m.rate] += 1
        if hops >= 4:
            facts["loudness_blocks:" + m.kind] += 1
        facts["loudness_to_the_last_frame"] += first + n == m.frames
        facts["loudness_true_peak_at_96000_or_32000"] += true_peak and m.rate in (96000, 32000)
        ops.append(("loudness", src, true_peak, first, n))

    # ---- the six newer producers and the three consumers
    def cycle(name, menu):
        """the menu's entries in turn (from a start of the seed's own): 40 draws of a menu of 8 reach every entry, which 40
        random draws do not promise"""
        if name not in turns:
            turns[name] = int(rng.integers(len(menu)))
        turns[name] += 1
        return menu[turns[name] % len(menu)]

    def drawn(name, value):
        facts["%s:%s" % (name, value)] += 1

    def child(m: Meta, kind, frames, amp, channels=None, gaps=None):
        return Meta(kind, "f32", m.channels if channels is None else channels, m.rate, frames, m.lineage + (kind,), amp, m.quiet,
                    m.gaps if gaps is None else gaps, flavour=m.flavour)

    def source_for(kinds=(), need=1, ok=None, share=.5, **how):
        """a source of `need` frames and more: in `share` of the draws one of another rate than the session's (so that its
        result can be played through its end), then one whose kind is in `kinds` (the chains the census wants) first"""
        fit = lambda m: m.frames >= need and (ok is None or ok(m))
        src = None
        if rng.random() < .35:
            src = pick_source(ok=lambda m: fit(m) and m.rate != RATE, **how)
        if src is None and kinds and rng.random() < share:
            src = pick_source(ok=lambda m: fit(m) and m.kind in kinds, **how)
        return pick_source(ok=fit, **how) if src is None else src

    def range_of(m: Meta, n):
        """where a range of n frames lies: now and then from frame 0 or up to the source's last frame"""
        r = rng.random()
        return 0 if r < .2 else m.frames - n if r < .5 else int(rng.integers(0, m.frames - n + 1))

    def refused_on_i16(kind, make_op):
        """-> whether one could be drawn: the producer on an i16 sample, every argument in order"""
        i16 = [k for k in order if not live[k].editable]
        if not i16:
            return False
        src = i16[rng.integers(len(i16))]
        m = live[src]
        n = int(rng.integers(1, min(m.frames, 3000) + 1))
        ops.append(make_op(src, m, range_of(m, n), n))
        facts["refused_%s:%d" % (kind, REFUSED_I16)] += 1
        follow_with_delete([src], "refused_%s_then_delete" % kind)
        return True

    def op_filter():
        if rng.random() < .15 and refused_on_i16("filter", lambda src, m, first, n: (
                "filter", None, src, first, n, int(rng.choice(FILTER_TAILS)), filter_menu(m.rate)[0], REFUSED_I16)):
            return
        menu = rng.random() < .7
        total = cycle("filter_total", FILTER_TOTALS) if menu else int(rng.integers(2, 20000))
        tail = min(cycle("filter_tail", FILTER_TAILS), total - 1)
        n = total - tail
        heavy = cycle("filter_heavy", (5, 6, 7))          # the feature tests' cascades first, where somebody is quiet enough
        fits = lambda i: any(m.editable and m.amp * filter_l1(filter_menu(m.rate)[i]) <= 1.2 for m in live.values())
        stages = heavy if fits(heavy) and rng.random() < .7 else cycle("filter_gentle", range(5))
        quiet_enough = lambda m: m.amp * filter_l1(filter_menu(m.rate)[stages]) <= 1.2
        src = source_for(("take", "bounce"), need=n, ok=quiet_enough)
        if src is None and stages == heavy:               # whoever is quiet enough, with the frames it has
            src = source_for(ok=quiet_enough)
            n = n if src is None else min(n, live[src].frames)
        if src is None:                                   # a gentle cascade, on whoever is quiet enough for it
            stages = cycle("filter_gentle", (0, 2, 4))
            src = source_for(("take",), ok=lambda m: m.amp * filter_l1(filter_menu(m.rate)[stages]) <= 1.2)
            if src is None:
                return op_add()
            n = min(n, live[src].frames)
        m = live[src]
        coef = filter_menu(m.rate)[stages]
        if not room(n + tail, m.channels):
            return op_delete()
        if n + tail in FILTER_TOTALS:
            drawn("filter_total", n + tail)
        drawn("filter_tail", tail)
        drawn("filter_cascade", stages)
        key = fresh(child(m, "filter", n + tail, m.amp * filter_l1(coef)))
        ops.append(("filter", key, src, range_of(m, n), n, tail, coef, 0))

    def second_of(m: Meta, need, kind):
        """the response or the key of a two-source call: another live F32 sample of the source's rate, mono and stereo in turn"""
        ch = cycle(kind + "_second_channels", (1, 2))
        c = [k for k in order if live[k] is not m and live[k].editable and live[k].rate == m.rate and live[k].frames >= need]
        c = [k for k in c if live[k].channels == ch] or c
        return c[rng.integers(len(c))] if c else None

    def refused_second(kind, src, make_op):
        """-> whether one could be drawn: a response / key of another rate (-4), or an i16 one of the source's rate (-3),
        make_op cutting the range to the frames it has; both named samples must be deletable afterwards"""
        m = live[src]
        other = [k for k in order if live[k].editable and live[k].rate != m.rate]
        i16 = [k for k in order if not live[k].editable and live[k].rate == m.rate]
        if i16 and (not other or rng.random() < .7):
            bad, status = i16[rng.integers(len(i16))], REFUSED_I16
        elif other:
            bad, status = other[rng.integers(len(other))], REFUSED_RATES
        else:
            return False
        ops.append(make_op(bad, status))
        facts["refused_%s:%d" % (kind, status)] += 1
        follow_with_delete([src, bad], "refused_%s_then_delete" % kind, every=True)
        return True

    def op_convolve():
        L = cycle("convolve_taps", CONV_TAPS) if rng.random() < .8 else int(rng.integers(3, 300))
        out = cycle("convolve_out", CONV_OUT + ("full",)) if rng.random() < .8 else None
        src, _ = source_of_frames(("splice",), 1 if out in (None, "full") else out, share=.6)
        if src is None:
            return op_add()
        m = live[src]
        most = min(m.frames, CONV_WORK // L, MAX_FRAMES - L)
        n = int(rng.integers(1, most + 1)) if rng.random() < .6 else most
        if out not in (None, "full"):                     # a range that has the window's frames, where the source has
            n = min(max(n, out + L), most)
        first = range_of(m, n)
        if rng.random() < .15:                            # (short ranges: every i16 sample and every rate has the frames)
            n, L = min(n, 48), min(L, 7)
            first = range_of(m, n)
            def make(bad, status):
                taps = min(L, live[bad].frames)
                return ("convolve", None, src, first, n, bad, range_of(live[bad], taps), taps, 0, n + taps - 1, -20.0, status)
            if refused_second("convolve", src, make):
                return
        ir = second_of(m, L, "convolve")
        if ir is None:                                    # nobody has L frames: the longest response there is
            ir = second_of(m, 1, "convolve")
            if ir is None:
                return op_add()
            L = min(L, live[ir].frames)
        r = live[ir]
        full = n + L - 1
        out_first = min(cycle("convolve_out_first", (0, 1, (L - 1) // 2)), full - 1)
        out = int(rng.integers(1, full - out_first + 1)) if out is None else out
        out_frames = full - out_first if out == "full" or out > full - out_first else out
        channels = max(m.channels, r.channels)
        if not room(out_frames, channels):
            return op_delete()
        # the bound on shapes alone: |y| <= src.amp x ir.amp x L x gain <= SPLICE_AMP
        worst = m.amp * r.amp * L
        gain_db = float(np.round(20.0 * np.log10(min(1.0, 0.99 * SPLICE_AMP / worst) * rng.uniform(0.5, 1.0)), 2))
        amp = worst * 10.0 ** (gain_db / 20.0)
        assert amp <= SPLICE_AMP
        if L in CONV_TAPS:
            drawn("convolve_taps", L)
        drawn("convolve_out", "full" if out_frames == full - out_first else out_frames)
        drawn("convolve_out_first", "mid" if out_first == (L - 1) // 2 and L > 3 else out_first)
        drawn("convolve_channels", "%d*%d" % (m.channels, r.channels))
        # noise against noise lies far below the bound: never normalized (gaps), never taken for all zero (not quiet)
        key = fresh(child(m, "convolve", out_frames, amp, channels, gaps=True))
        ops.append(("convolve", key, src, first, n, ir, r.frames - L if rng.random() < .4 else int(rng.integers(0, r.frames - L + 1)), L,
                    out_first, out_frames, gain_db, 0))

    def curve_shape():
        """-> (n at most n_most, A, H, R): the terms A + H + R from the menu, split several ways, n x terms within CURVE_WORK"""
        K = cycle("curve_terms", CURVE_TERMS) if rng.random() < .75 else int(rng.integers(3, 600))
        R = int([K, 1, max(1, K // 2), rng.integers(1, K + 1)][rng.integers(4)])
        A = int(min(LIM.MAX_LOOKAHEAD, [K - R, 0, (K - R) // 2][rng.integers(3)]))
        H = K - R - A
        r = rng.random()
        if r < .65:
            n = cycle("curve_frames", CURVE_SIZES)
        elif r < .8:
            n = int(rng.choice([x for x in LENGTHS if x >= 24560]))
        else:
            n = int(rng.integers(2, 20000))
        return min(n, CURVE_WORK // K), A, H, R, K

    def source_of_frames(kinds, n, **how):
        """-> (a source that has n frames where there is one, n or what the source has)"""
        src = source_for(kinds, need=n, **how)
        src = source_for(kinds, **how) if src is None else src
        return src, (n if src is None else min(n, live[src].frames))

    def curve_facts(kind, n, K):
        if n in CURVE_SIZES:
            drawn(kind + "_frames", n)
        if n >= 24560:
            drawn(kind + "_frames", "long")
        if K in CURVE_TERMS:
            drawn(kind + "_terms", K)

    def op_limit():
        if rng.random() < .15 and refused_on_i16("limit", lambda src, m, first, n: (
                "limit", None, src, first, n, -6.0, 0.0, 8, 0, 100, REFUSED_I16)):
            return
        n, A, H, R, K = curve_shape()
        src, n = source_of_frames(("bounce", "dynamics"), n, share=.7)
        if src is None:
            return op_add()
        m = live[src]
        if not room(n, m.channels):
            return op_delete()
        # on the bounds: the limiter works where drive x amp > ceiling, and idles for certain where it is not
        drive_db = float(np.round(rng.uniform(-6.0, min(6.0, 20.0 * np.log10(1.0 / m.amp))), 2))
        driven = m.amp * 10.0 ** (drive_db / 20.0)
        works = cycle("limit_works", (True, False))
        ceiling_db = float(np.round(20.0 * np.log10(driven * (rng.uniform(0.2, 0.7) if works else rng.uniform(1.02, 1.14))), 2))
        ceiling = float(np.float32(10.0 ** (ceiling_db / 20.0)))
        assert (driven > ceiling) == works
        facts["limit_works" if works else "limit_idles"] += 1
        curve_facts("limit", n, K)
        key = fresh(child(m, "limit", n, min(ceiling, driven * (1.0 + 1e-6))))
        ops.append(("limit", key, src, range_of(m, n), n, ceiling_db, drive_db, A, H, R, 0))

    def op_dynamics():
        n, A, H, R, K = curve_shape()
        src, n = source_of_frames(("limit",), n, share=.6)
        if src is None:
            return op_add()
        m = live[src]
        first = range_of(m, n)
        spec = cycle("dynamics_table", DYN_TABLES)
        drive = float(np.float32(rng.uniform(0.5, 1.5) * rng.choice([-1, 1])))
        makeup = float(np.float32(min(1.5, 1.15 / (m.amp * abs(drive))) * rng.uniform(0.6, 1.0)))
        key_gain = float(np.float32(rng.uniform(0.5, 4.0) * rng.choice([-1, 1])))
        how = cycle("dynamics_key", ("self", "key", "key", "self", "key", "refused"))
        make = lambda kkey, status, nn=n, f=first: ("dynamics", None if status else -1, src, f, nn, spec, spec[0], kkey,
                                                     range_of(live[kkey], nn) if kkey is not None else 0,
                                                     drive, key_gain, makeup, A, H, R, status)
        if how == "refused":                              # (the range cut to what the key has: its length is not the reason)
            if refused_second("dynamics", src, lambda bad, status: make(bad, status, min(n, live[bad].frames),
                                                                        min(first, m.frames - min(n, live[bad].frames)))):
                return
        kkey = second_of(m, n, "dynamics") if how == "key" else None
        if not room(n, m.channels):
            return op_delete()
        curve_facts("dynamics", n, K)
        drawn("dynamics_sense", spec[0])
        op = make(kkey, 0)
        if kkey is not None:
            drawn("dynamics_key_channels", live[kkey].channels)
            facts["dynamics_key_to_the_last_frame"] += op[8] + n == live[kkey].frames
        else:
            facts["dynamics_keyed_by_itself"] += 1
        amp = m.amp * abs(drive) * makeup
        assert amp <= SPLICE_AMP * (1.0 + 1e-6)
        key = fresh(child(m, "dynamics", n, amp * (1.0 + 1e-6), gaps=True if spec[0] == DYN.GATE else None))
        ops.append(op[:1] + (key,) + op[2:])

    def stretch_shape(kind):
        """-> (n, N, D, the name of D): windows and tolerances from the menus; ranges shorter than a window among them"""
        N = cycle(kind + "_window", STRETCH_WINDOWS)
        how = cycle(kind + "_tolerance", STRETCH_TOLERANCES)
        D = {"0": 0, "Hs-1": N // 2 - 1, "Hs": N // 2, "Hs+1": N // 2 + 1, "512": 512}[how]
        r = rng.random()
        n = int(rng.integers(1, N)) if r < .2 else int(rng.integers(N, 8 * N + 1)) if r < .5 else int(rng.integers(1, 48001))
        return n, N, D, how

    def inside_a_step(m, N, lo):
        """the nearest length at or below m (at or above lo) that ends inside a step and inside a 16-byte word"""
        while m > lo and (m % 4 == 0 or m % (N // 2) == 0):
            m -= 1
        return m

    def op_stretch():
        if rng.random() < .15 and refused_on_i16("stretch", lambda src, m, first, n: (
                "stretch", None, src, first, n, n + 1 + n % 2, 64, 24, REFUSED_I16)):
            return
        n, N, D, how = stretch_shape("stretch")
        src, n = source_of_frames(("resample",), n, share=.6)
        if src is None:
            return op_add()
        m = live[src]
        first = range_of(m, n)
        if rng.random() < .1 and not m.refs:              # beyond the eightfold: refused on the sizes alone
            facts["refused_stretch_beyond_8:%d" % REFUSED_RATIO] += 1
            ops.append(("stretch", None, src, first, n, 8 * n + int(rng.integers(1, 4)), N, D, REFUSED_RATIO))
            return follow_with_delete([src], "refused_stretch_then_delete")
        lo, hi = -(-n // 8), min(8 * n, STRETCH_FRAMES)
        out = inside_a_step(int([hi, lo, rng.integers(lo, hi + 1), rng.integers(lo, hi + 1)][rng.integers(4)]), N, lo)
        if not room(out, m.channels):
            return op_delete()
        drawn("stretch_window", N)
        drawn("stretch_tolerance", how)
        facts["stretch_shorter_than_a_window"] += n < N
        facts["stretch_ends_inside_a_word_and_a_step"] += out % 4 != 0 and out % (N // 2) != 0
        facts["stretch_longer" if out > n else "stretch_shorter"] += 1
        # the two half-windows sum to 1: a convex combination of two source frames (and one rounding to float32)
        key = fresh(child(m, "stretch", out, m.amp * (1.0 + 1e-6)))
        ops.append(("stretch", key, src, first, n, out, N, D, 0))

    def op_pitch():
        quality = int(cycle("pitch_quality", QUALITIES))
        num, den = cycle("pitch_ratio", PITCH_RATIOS)
        most = pitch_l1(num, den, quality)                # (the stretch in front of the conversion adds nothing: op_stretch)
        in_range = lambda m: m.quiet or m.amp * most <= 1.2   # the rule of a conversion: op_resample
        n, N, D, how = stretch_shape("pitch")
        src, n = source_of_frames(("stretch",), n, share=.6, ok=in_range)
        if src is None:
            return op_add()
        m = live[src]
        first = range_of(m, n)
        if rng.random() < .16 and not m.refs:             # a ratio that reduces to 1: -4; beyond 4 : 1: -3
            num, den, status = [(6, 6, REFUSED_ONE), (5, 1, REFUSED_RATIO), (2, 9, REFUSED_RATIO)][cycle("pitch_refused", (0, 0, 1, 2))]
            facts["refused_pitch:%d" % status] += 1
            ops.append(("pitch", None, src, first, n, n, num, den, quality, N, D, status))
            return follow_with_delete([src], "refused_pitch_then_delete")
        L, M = PM.ratio(num, den)
        # m' = ceil(out M / L) within n / 8 .. 8 n and the twin's cap; out the range's own length where that fits
        lo, hi = -(-n // 8), min(8 * n, STRETCH_FRAMES)
        out_lo, out_hi = -(-lo * L // M), hi * L // M
        if out_hi < max(out_lo, 1):
            return op_stretch()
        own = out_lo <= n <= out_hi and rng.random() < .5
        out = n if own else int(rng.integers(max(out_lo, 1), out_hi + 1))
        if PM.check_args(n, out, num, den, quality, N, D) or not room(out, m.channels):
            return op_delete()
        drawn("pitch_ratio", "%d/%d" % (num, den))
        drawn("pitch_quality", quality)
        drawn("pitch_window", N)
        drawn("pitch_tolerance", how)
        facts["pitch_own_length" if own else "pitch_another_length"] += 1
        key = fresh(child(m, "pitch", out, m.amp * most))
        ops.append(("pitch", key, src, first, n, out, num, den, quality, N, D, 0))

    def consumer_range(kind, m: Meta, least, most):
        """a range for a consumer: no hop (shorter than `least`), or hops; often up to the source's last frame"""
        top = min(m.frames, most)
        if top < least or cycle(kind + "_range", ("hops", "no_hop", "hops", "hops")) == "no_hop":
            n = int(rng.integers(1, min(least, m.frames + 1)))
        else:
            n = top if rng.random() < .4 else int(rng.integers(least, top + 1))
        first = m.frames - n if rng.random() < .4 else int(rng.integers(0, m.frames - n + 1))
        facts[kind + ("_hops" if n >= least else "_no_hop")] += 1
        facts[kind + "_to_the_last_frame"] += first + n == m.frames
        return first, n

    def heard(flavour, least):
        """a consumer's source: one with that flavour of upload behind it and frames for a hop first, so that hops are
        voiced and onsets fire; anybody else for the rest"""
        src = pick_source(ok=lambda m: m.flavour == flavour and m.frames >= least) if rng.random() < .6 else None
        return pick_source(boost=lambda m: (4.0 if m.flavour == flavour else 1.0) * (4.0 if m.frames >= least else 1.0)) if src is None else src

    def op_f0():
        Wn, H, tau_max = cycle("f0_window", F0_WINDOWS), cycle("f0_hop", F0_HOPS), cycle("f0_tau_max", F0_TAU_MAX)
        src = heard("tone", Wn + tau_max)
        left = F0_TERMS_A_SCRIPT - state["f0_terms"]
        if src is None or left < Wn * (tau_max + 1):
            return op_measure()
        m = live[src]
        hops = min(F0_TERMS, left) // (Wn * (tau_max + 1))
        first, n = consumer_range("f0", m, Wn + tau_max, Wn + tau_max + hops * H - 1)
        state["f0_terms"] += F0.hops(n, Wn, H, tau_max) * Wn * (tau_max + 1)
        drawn("f0_window", Wn)
        drawn("f0_hop", H)
        drawn("f0_tau_max", tau_max)
        ops.append(("f0", src, Wn, H, int(rng.integers(2, 25)), tau_max, float(rng.choice([0.1, 0.15, 0.3])), first, n))

    def op_onsets():
        H = cycle("onsets_hop", ONSET_HOPS)
        src = heard("clicks", 8 * H)
        if src is None:
            return op_add()
        first, n = consumer_range("onsets", live[src], H, MAX_FRAMES)
        drawn("onsets_hop", H)
        ops.append(("onsets", src, H, float(rng.choice([1e-9, 1e-6])), float(rng.choice([0.3, 0.5])), float(rng.choice([0.0, 0.1])),
                    int(rng.choice([0, 3, 8])), int(rng.choice([0, 8, 40])), first, n))

    def op_tempo():
        H = cycle("tempo_hop", ONSET_HOPS)
        Wn, step, lag_min, lag_max = cycle("tempo_shape", TEMPO_SHAPES)
        least = (Wn + lag_max) * H                       # hops of the novelty for one window
        src = heard("clicks", least)
        left = F0_TERMS_A_SCRIPT - state["f0_terms"]
        if src is None or left < Wn * (lag_max + 1):
            return op_measure()
        m = live[src]
        windows = min(F0_TERMS, left) // (Wn * (lag_max + 1))
        first, n = consumer_range("tempo", m, least, least + (windows * step) * H - 1)
        state["f0_terms"] += F0.hops(n // H, Wn, step, lag_max) * Wn * (lag_max + 1)
        drawn("tempo_hop", H)
        ops.append(("tempo", src, H, 1e-9, Wn, step, lag_min, lag_max, float(rng.choice([0.3, 0.5])), first, n))

    def op_take():
        n = int(rng.integers(2, 7))
        kind = int(rng.choice([RM.MONO, RM.STEREO]))
        channels = 2 if kind == RM.STEREO else 1
        chunks = (-(-(n * F + F) // CHUNK) + SPARE) * G * channels
        if state["total"] + chunks + 2 * G > BUDGET - (4 << 20):
            return op_delete()
        state["total"] += chunks
        track = int(rng.integers(TRACKS))
        lo = region(n * UNIT)
        key = fresh(Meta("take", "f32", channels, RATE, n * F, ("take",), amp=0.6, refs=1))
        placed[("take", key)] = (key, track, lo, None, 0.0, None)
        ops.append(("take", key, track, kind, 0 if kind == RM.STEREO else int(rng.integers(INPUTS)), state["input_block"], n, lo))
        state["input_block"] += n

    def op_bounce():
        if placed and rng.random() < .8:
            _, track, lo, _, _, _ = list(placed.values())[rng.integers(len(placed))]
            lo = lo - float(rng.uniform(0, 2)) * UNIT
        else:                         # the session's own clips, beats 0 .. 9 blocks
            track, lo = int(rng.integers(TRACKS)), float(rng.uniform(0, 4)) * UNIT
        hi = lo + float(rng.uniform(0.3, 8.0)) * UNIT
        frames = int((hi - lo) * (60.0 / BPM) * RATE)   # (the rig takes the exact figure from the oracle)
        menu = [("track", track, "post"), ("track", track, "pre"), ("master",), ("track", int(rng.integers(TRACKS)), "post")]
        sources = [menu[i] for i in sorted(rng.choice(len(menu), size=int(rng.integers(1, 4)), replace=False))]
        if frames < 1 or not room(frames + 1, 2 * len(sources)):
            return op_delete()
        ks = [fresh(Meta("bounce", "f32", 2, RATE, frames, ("bounce",), amp=1.0, quiet=True)) for _ in sources]
        ops.append(("bounce", tuple(ks), lo, hi, tuple(sources)))

    def op_place():
        src = pick_source(editable=False, boost=lambda m: (12.0 if m.kind == "loudnorm" else 4.0 if m.kind == "splice" else 8.0)
                          if off_rate_newcomer(m) else 1.0)
        if src is None:
            return op_add()
        m = live[src]
        tail = int(rng.integers(1, 2 * F + 1))                       # source frames that sound, up to the sample's last one
        start = max(0, m.frames - tail)
        sounding = (m.frames - start) * RATE / m.rate                # frames at the session rate
        lo = region((sounding / F + 2) * UNIT)
        hi = lo + (sounding / F + 1 + float(rng.uniform(0, 1))) * UNIT   # the clip ends BEHIND the sample's last frame
        pid = state["pid"] = state["pid"] + 1
        placed[pid] = (src, int(rng.integers(TRACKS)), lo, hi, float(start), sounding)
        m.refs += 1
        ops.append(("place", pid, src) + placed[pid][1:5])

    def op_unplace():
        if not placed:
            return op_place()
        pid = list(placed)[rng.integers(len(placed))]
        live[placed.pop(pid)[0]].refs -= 1
        ops.append(("unplace", pid))

    def op_play():
        c = [p for p in placed.values() if p[5] is not None]
        if not c:
            return op_place()
        w = np.array([(10.0 if live[p[0]].kind == "loudnorm" else 4.0 if live[p[0]].kind == "splice" else 8.0)
                      if off_rate_newcomer(live[p[0]]) else 1.0 for p in c])
        src, _, lo, hi, _, sounding = c[rng.choice(len(c), p=w / w.sum())]
        n = int(rng.integers(3, 7))
        start = lo - float(rng.uniform(0.1, 1.0)) * UNIT
        if start + n * UNIT > lo + (sounding + 2) / F * UNIT and live[src].rate != RATE:
            facts["play_through_the_end_off_rate"] += 1
            facts["play_through_the_end_off_rate:" + live[src].kind] += 1
        ops.append(("play", start, n))

    def op_measure():
        src = pick_source()
        if src is None:
            return op_add()
        ops.append(("measure", src) + pick_range(live[src]))

    def op_export():
        src = pick_source()
        if src is None:
            return op_add()
        ops.append(("export", src, str(rng.choice(EXPORT_FORMATS)), bool(rng.integers(2))) + pick_range(live[src], most=20000))

    def op_mip():
        c = [k for k in order if live[k].frames > 64]
        if not c:
            return op_add()
        ops.append(("mip", c[rng.integers(len(c))], int(rng.integers(2))))

    def op_delete():
        if not order:
            return op_add()
        c = [k for k in order if live[k].refs] if rng.random() < .12 else [k for k in order[:-1] if not live[k].refs]
        if not c:
            c = [k for k in order if not live[k].refs] or order
        key = c[rng.integers(len(c))]
        if live[key].refs:
            facts["refused_delete"] += 1
            ops.append(("delete", key, -4))
            return
        do_delete(key)

    def do_delete(key):
        if key != order[-1]:
            facts["delete_not_newest"] += 1
            pending_holes.append(pool_bounds(live[key].frames, live[key].channels, live[key].fmt)[0])
        order.remove(key)
        del live[key]
        ops.append(("delete", key, 0))

    table = dict(add=op_add, derive=op_derive, normalize=op_normalize, resample=op_resample, take=op_take, bounce=op_bounce,
                 splice=op_splice, loudnorm=op_loudnorm, place=op_place, unplace=op_unplace, play=op_play, measure=op_measure,
                 loudness=op_loudness, export=op_export, mip=op_mip, delete=op_delete, filter=op_filter, convolve=op_convolve,
                 limit=op_limit, dynamics=op_dynamics, stretch=op_stretch, pitch=op_pitch, f0=op_f0, onsets=op_onsets,
                 tempo=op_tempo)
    names = list(table)
    w = np.array([WEIGHTS[k] for k in names], dtype=float)
    for _ in range(3):
        op_add()
    while len(ops) < n_ops:
        table[names[rng.choice(len(names), p=w / w.sum())]]()
    for op in ops:
        facts["op:" + op[0]] += 1
    facts["total_bytes"] = state["total"]
    facts["input_blocks"] = state["input_block"]
    return tuple(ops), facts


def validate(ops) -> None:
    """every producing op is one the product must accept: ranges inside the source, descriptions that fit it, results
    below MAX_FRAMES, sources alive — replayed on shapes alone"""
    shape: Dict[int, Tuple[str, int, int, int]] = {}   # key -> (fmt, channels, rate, frames)
    for op in ops:
        k = op[0]
        if k == "add":
            shape[op[1]] = (op[2], op[3], op[4], op[5])
            assert op[5] >= 1 and op[3] in (1, 2)
        elif k in ("derive", "normalize", "resample", "measure", "export"):
            src = op[2] if k in ("derive", "normalize", "resample") else op[1]
            fmt, ch, rate, frames = shape[src]
            assert fmt == "f32"
            first, n = (op[3], op[4]) if k == "derive" else (op[-2], op[-1])
            assert n >= 1 and first >= 0 and first + n <= frames, op
            if k == "derive":
                assert op[6] in FX.MODES_FOR[ch] and op[8] <= n and op[9] <= n and op[7] != 0.0
                shape[op[1]] = ("f32", FX.out_channels(ch, op[6]), rate, n)
            elif k == "normalize":
                assert 0 < op[3] <= 1.0
                shape[op[1]] = ("f32", ch, rate, n)
            elif k == "resample":
                assert op[3] != rate and RS.plan(rate, op[3], op[4])
                shape[op[1]] = ("f32", ch, op[3], RS.out_frames(rate, op[3], n))
                assert 1 <= shape[op[1]][3] <= MAX_FRAMES
        elif k == "splice":
            _, key, channels, n_frames, parts, status = op
            assert channels in (1, 2) and 1 <= n_frames <= MAX_FRAMES and 1 <= len(parts) <= SPLICE_PARTS
            refusal, common = 0, None
            for p in (SP.Part(*p) for p in parts):        # the product's order: part by part, the first refusal found wins
                fmt, ch, rate, frames = shape[p.src]
                assert p.n >= 1 and p.first >= 0 and p.first + p.n <= frames and p.at >= 0 and p.at + p.n <= n_frames, op
                assert p.fade_in <= p.n and p.fade_out <= p.n and p.shape_in in range(3) and p.shape_out in range(3)
                assert p.mode in FX.MODES_FOR[ch] and FX.out_channels(ch, p.mode) == channels and p.gain != 0.0
                common = rate if common is None else common
                if fmt != "f32":
                    refusal = REFUSED_I16
                elif rate != common:
                    refusal = REFUSED_RATES
                if refusal:
                    break
            assert status == refusal and (key is None) == (status != 0), op
            if status == 0:
                shape[key] = ("f32", channels, common, n_frames)
        elif k == "loudnorm":
            _, key, src, target, ceiling, first, n, status = op
            fmt, ch, rate, frames = shape[src]
            assert fmt == "f32" and n >= 1 and first >= 0 and first + n <= frames and 0.0 < ceiling <= 1.0, op
            assert LM.oversampling(rate) * n <= MAX_FRAMES
            short = n < 4 * LM.hop_frames(rate)
            assert status == (REFUSED_SHORT if short else 0) and (key is None) == short, op
            if not short:
                shape[key] = ("f32", ch, rate, n)
        elif k == "loudness":
            _, src, true_peak, first, n = op
            fmt, ch, rate, frames = shape[src]
            assert fmt == "f32" and n >= 1 and first >= 0 and first + n <= frames, op
            assert not true_peak or LM.oversampling(rate) * n <= MAX_FRAMES
        elif k in NEW_PRODUCERS:
            key, src, first, n, status = op[1], op[2], op[3], op[4], op[-1]
            fmt, ch, rate, frames = shape[src]
            assert n >= 1 and first >= 0 and first + n <= frames, op
            refusal, out_ch = (0 if fmt == "f32" else REFUSED_I16), ch      # (every check of the arguments comes first)
            if k == "filter":
                tail, coef = op[5], op[6]
                assert FM.check(np.array(coef)) and 1 <= len(coef) <= 8 and tail >= 0
                out = n + tail
            elif k == "convolve":
                _, _, _, _, _, ir, ir_first, L, out_first, out, gain_db, _ = op
                ifmt, ich, irate, iframes = shape[ir]
                assert fmt == "f32" and ir != src and L >= 1 and ir_first >= 0 and ir_first + L <= iframes, op
                assert out >= 1 and out_first + out <= CV.full_frames(n, L) and n * L <= CONV_WORK and np.isfinite(gain_db), op
                assert irate == rate or ifmt == "f32"                        # (one reason at a time: the order is not pinned)
                refusal, out_ch = (REFUSED_RATES if irate != rate else 0 if ifmt == "f32" else REFUSED_I16), max(ch, ich)
            elif k == "limit":
                _, _, _, _, _, ceiling_db, drive_db, A, H, R, _ = op
                assert LIM.check_args(n, np.float32(10.0 ** (ceiling_db / 20.0)), 10.0 ** (drive_db / 20.0), A, H, R) == 0, op
                assert n * (A + H + R) <= CURVE_WORK
                out = n
            elif k == "dynamics":
                _, _, _, _, _, spec, sense, kkey, key_first, drive, key_gain, makeup, A, H, R, _ = op
                assert fmt == "f32" and sense == spec[0] and n * (A + H + R) <= CURVE_WORK, op
                assert DYN.check_args(n, dyn_table(spec), sense, drive, key_gain, makeup, A, H, R, kkey is not None) == 0, op
                if kkey is not None:
                    kfmt, _, krate, kframes = shape[kkey]
                    assert kkey != src and key_first >= 0 and key_first + n <= kframes and (krate == rate or kfmt == "f32"), op
                    refusal = REFUSED_RATES if krate != rate else 0 if kfmt == "f32" else REFUSED_I16
                out = n
            elif k == "stretch":
                _, _, _, _, _, out, N, D, _ = op
                refusal = ST.check_args(n, out, N, D) or refusal
                assert refusal in (0, REFUSED_I16) and (refusal or out <= STRETCH_FRAMES), op
            else:
                _, _, _, _, _, out, num, den, quality, N, D, _ = op
                assert fmt == "f32"
                refusal = PM.check_args(n, out, num, den, quality, N, D)
                assert refusal or PM.mid_frames(out, num, den) <= STRETCH_FRAMES, op
            assert status == refusal and (key is None) == (status != 0), op
            if status == 0:
                assert 1 <= out <= MAX_FRAMES, op
                shape[key] = ("f32", out_ch, rate, out)
        elif k in CONSUMERS:
            fmt, ch, rate, frames = shape[op[1]]
            first, n = op[-2], op[-1]
            assert fmt == "f32" and n >= 1 and first >= 0 and first + n <= frames, op
            if k == "f0":
                assert F0.check(n, *op[2:7]) == 0 and F0.hops(n, op[2], op[3], op[5]) * op[2] * (op[5] + 1) <= F0_TERMS, op
            elif k == "onsets":
                assert ON.check(n, *op[2:8]) == 0, op
            else:
                assert ON.tempo_check(n, *op[2:9]) == 0, op
        elif k == "take":
            assert 2 <= op[6] <= 6 and op[2] < TRACKS
            shape[op[1]] = ("f32", 2 if op[3] == RM.STEREO else 1, RATE, op[6] * F)
        elif k == "bounce":
            assert op[2] < op[3] and (op[3] - op[2]) / UNIT <= 8.0 and len(op[1]) == len(op[4])
            for key in op[1]:
                shape[key] = ("f32", 2, RATE, int((op[3] - op[2]) * (60.0 / BPM) * RATE))
        elif k in ("place", "mip"):
            assert (op[2] if k == "place" else op[1]) in shape
        elif k == "delete":
            assert op[1] in shape
            if op[2] == 0:
                del shape[op[1]]


def sources_of(op) -> set:
    """the script keys whose contents an op reads"""
    k = op[0]
    if k == "splice":
        return {p[0] for p in op[4]}
    if k in ("derive", "normalize", "resample", "loudnorm", "filter", "limit", "stretch", "pitch"):
        return {op[2]}
    if k == "convolve":
        return {op[2], op[5]}
    if k == "dynamics":
        return {op[2]} | ({op[7]} if op[7] is not None else set())
    if k in CONSUMERS + ("measure", "loudness", "export", "mip", "place"):
        return {op[2] if k == "place" else op[1]}
    return set()


def census(seeds=SEEDS):
    total, worst = collections.Counter(), 0
    for s in seeds:
        ops, facts = make_script(s)
        validate(ops)
        worst = max(worst, facts["total_bytes"])
        total.update({k: v for k, v in facts.items() if k != "total_bytes"})
    total["worst_total_bytes"] = worst
    return total


class Contents:
    """what every live sample holds: key -> (fmt, rate, [planes]).  The rig hands in a take's and a bounce's planes."""

    def __init__(self):
        self.s: Dict[object, Tuple[str, int, List[np.ndarray]]] = {}

    def put(self, key, fmt, rate, planes):
        self.s[key] = (fmt, rate, [np.ascontiguousarray(p) for p in planes])

    def apply(self, op) -> Optional[object]:
        """the ops whose result follows from the script alone; -> the new key"""
        k = op[0]
        if k == "add":
            self.put(op[1], op[2], op[4], upload_planes(op[7], op[2], op[3], op[5], op[8]))
        elif k == "derive":
            _, rate, planes = self.s[op[2]]
            self.put(op[1], "f32", rate, FX.derive(planes, op[3], op[4], op[5], op[6], np.float32(op[7]), op[8], op[9], op[10], op[11]))
        elif k == "normalize":
            _, rate, planes = self.s[op[2]]
            peak = max(FX.measure(planes, op[4], op[5])["peak"])
            self.gain = FX.normalize_gain(op[3], peak)
            self.put(op[1], "f32", rate, FX.derive(planes, op[4], op[5], gain=self.gain))
        elif k == "resample":
            _, rate, planes = self.s[op[2]]
            self.put(op[1], "f32", op[3], RS.resample(planes, op[5], op[6], rate, op[3], op[4], tab=_table(rate, op[3], op[4])))
        elif k == "splice" and op[-1] == 0:
            parts = [SP.Part(*p) for p in op[4]]
            rate = self.s[parts[0].src][1]
            self.put(op[1], "f32", rate, SP.splice({p.src: self.s[p.src][2] for p in parts}, op[2], op[3], parts))
        elif k == "loudnorm" and op[-1] == 0:
            self.apply_loudnorm(op, self.loudnorm_gains(op)[0])
        elif k in NEW_PRODUCERS and op[-1] == 0:
            _, rate, planes = self.s[op[2]]
            first, n = op[3], op[4]
            self.info = None                              # the statistics / info the call returns beside the sample
            if k == "filter":
                out = FM.filter_clip(planes, first, n, op[5], np.array(op[6]))
            elif k == "convolve":
                _, _, _, _, _, ir, ir_first, L, out_first, out_frames, gain_db, _ = op
                out = CV.convolve_clip(planes, first, n, self.s[ir][2], ir_first, L, out_first, out_frames, 10.0 ** (float(gain_db) / 20.0))
            elif k == "limit":
                _, _, _, _, _, ceiling_db, drive_db, A, H, R, _ = op
                out, self.info = LIM.limit_clip(planes, first, n, np.float32(10.0 ** (float(ceiling_db) / 20.0)),
                                                10.0 ** (float(drive_db) / 20.0), A, H, R)
            elif k == "dynamics":
                _, _, _, _, _, spec, sense, kkey, key_first, drive, key_gain, makeup, A, H, R, _ = op
                out, self.info = DYN.dynamics_clip(planes, first, n, dyn_table(spec), sense, drive, makeup, A, H, R,
                                                   None if kkey is None else self.s[kkey][2], key_first, key_gain)
            elif k == "stretch":
                out, _, self.info = ST.stretch_clip(planes, first, n, op[5], op[6], op[7])
            else:
                out, _, self.info = PM.pitch_clip(planes, first, n, *op[5:11])
            self.put(op[1], "f32", rate, out)
        elif k == "delete":
            if op[2] == 0:
                del self.s[op[1]]
            return None
        else:
            return None
        return op[1]

    def analyse(self, op):
        """a consumer's (records, info) from the feature's model"""
        planes, first, n = self.s[op[1]][2], op[-2], op[-1]
        if op[0] == "f0":
            return F0.f0_clip(planes, first, n, *op[2:7])
        if op[0] == "onsets":
            return ON.onsets_clip(planes, first, n, *op[2:8])
        return ON.tempo_clip(planes, first, n, *op[2:9])

    def loudnorm_gains(self, op):
        """-> float32 (the model's gain, the gain of the target alone, the gain of the ceiling alone): the smaller of the
        last two is the first"""
        _, _, src, target, ceiling, first, n, _ = op
        _, rate, planes = self.s[src]
        m = LM.measure(planes, first, n, rate, LM.TRUE_PEAK)
        peaks = m["true_peak"][:len(planes)]
        free = LM.normalize_gain(m["integrated"], target)
        return LM.normalize_gain(m["integrated"], target, ceiling, peaks), free, np.float32(ceiling) / np.float32(max(peaks))

    def apply_loudnorm(self, op, gain):
        """the result at `gain`: the model's, or the one the product used (pow's last place is not pinned)"""
        _, rate, planes = self.s[op[2]]
        self.put(op[1], "f32", rate, FX.derive(planes, op[5], op[6], gain=np.float32(gain)))


@functools.lru_cache(maxsize=None)
def _table(rs, rd, q):
    return RS.table(rs, rd, q)
