"""Sample life scripts: random chains of everything that puts audio into the engine's clip pool and takes it out again —
uploads, derived / normalized / resampled / spliced / loudness-normalized samples, recorder takes, bounces, deletes — with
placements, playback, measure, loudness, export and mip-maps in between, and the model of what every live sample must hold.
Pure Python (numpy): the generator works on shapes alone (tests/test_sample_scripts.py takes its census without a device),
Contents computes the exact fp32 planes from tests/clipfx_model.py, tests/resample_model.py, tests/splice_model.py and
tests/loudness_model.py; takes and bounces get theirs from the rig that runs the script
(tests/test_gpu_sample_scripts.py), since they depend on the inputs fed and on the oracle engine's render.
TEST INFRASTRUCTURE — nothing here is shipped.

A script is a list of tuples; `key` names a sample inside the script (the product's ids are the rig's business):
    ("add", key, fmt, channels, rate, frames, interleaved, seed)
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
"""
from __future__ import annotations

import collections
import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import clipfx_model as FX
import loudness_model as LM
import record_model as RM
import resample_model as RS
import splice_model as SP

F, RATE, BPM, TRACKS, INPUTS = 128, 48000, 120.0, 4, 2
CHUNK, SPARE = 700, 4                 # the recorder's chunks (frames) and how many it keeps ahead
G = 64 << 10
SEEDS = tuple(range(12))
N_OPS = 80
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
MADE_ON_THE_DEVICE = dict(splice=8.0, derive=4.0, normalize=4.0, resample=4.0)
REFUSED_I16, REFUSED_RATES, REFUSED_SHORT = -3, -4, -4   # as tests/test_gpu_splice.py and test_gpu_loudness.py pin them
TARGETS_LOUD, TARGETS_SOFT = (-6.0, 0.0), (-42.0, -30.0)   # LUFS: the ceiling binds / the target does (noise of -10 .. -25)
PRODUCERS = ("add", "derive", "normalize", "resample", "take", "bounce", "splice", "loudnorm")
KINDS = PRODUCERS + ("place", "unplace", "play", "measure", "loudness", "export", "mip", "delete")
WEIGHTS = dict(add=7, derive=6, normalize=2.5, resample=7, take=3.5, bounce=3, splice=7, loudnorm=6, place=5.5, unplace=2,
               play=5, measure=2, loudness=4, export=2, mip=2, delete=9)


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
    gaps: bool = False                # may hold long stretches of zeros (frames of a splice that no part of a loud source
                                      # covers): neither peak- nor loudness-normalized
    refs: int = 0                     # clips that name it

    @property
    def editable(self):
        return self.fmt == "f32"


def upload_planes(seed: int, fmt: str, channels: int, frames: int) -> List[np.ndarray]:
    """non-zero noise: whatever extent an upload reuses holds junk afterwards"""
    rng = np.random.default_rng([0xADD, seed])
    if fmt == "i16":
        return [(rng.integers(1, 20000, frames) * rng.choice([-1, 1], frames)).astype(np.int16) for _ in range(channels)]
    x = [rng.uniform(0.05, 0.5, frames).astype(np.float32) * rng.choice([-1, 1], frames).astype(np.float32) for _ in range(channels)]
    return [np.ascontiguousarray(p, dtype=np.float32) for p in x]


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
    state = dict(beat=1.0, total=0, input_block=0, pid=0, loud=0)

    def fresh(meta: Meta, sources=None) -> int:
        """sources: the distinct source keys of a splice (every other producer's one source is in its lineage)"""
        key = next(keys)
        live[key] = meta
        order.append(key)
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
                       "loudnorm": 2.0}.get(live[k].kind, 1.0) *
                      (6.0 if chain and live[k].lineage[-len(chain):] == chain else 1.0) *
                      (boost(live[k]) if boost else 1.0) for k in c])
        return c[rng.choice(len(c), p=w / w.sum())]

    def enough(m: Meta):
        """4 hops and more: a range of it has blocks for the gate, and may be normalized to a loudness"""
        return m.frames >= 4 * LM.hop_frames(m.rate)

    def off_rate_newcomer(m: Meta):
        """a splice or loudness-normalized result of another rate than the session's: the padding behind it is read only
        when a placement of it plays through its end"""
        return m.kind in ("splice", "loudnorm") and m.rate != RATE

    def pick_range(m: Meta, most=MAX_FRAMES, least=1):
        top = min(m.frames, most)
        n = int(rng.integers(min(least, top), top + 1)) if rng.random() < .6 else top
        first = int(rng.integers(0, m.frames - n + 1))
        if rng.random() < .3:
            first = m.frames - n      # up to the source's last frame
        return first, n

    def op_add(long=False):
        fmt = "i16" if rng.random() < .15 and not long else "f32"
        channels, rate = int(rng.integers(1, 3)), int(rng.choice(RATES[:2]))
        menu = [n for n in LENGTHS if n >= 19200] if long else LENGTHS    # (long: 4 hops of loudness and more)
        frames = int(menu[rng.integers(len(menu))])
        if not room(frames, channels, fmt):
            frames = int(LENGTHS[rng.integers(8)])
        key = fresh(Meta("add", fmt, channels, rate, frames, ("add",), amp=0.5))
        ops.append(("add", key, fmt, channels, rate, frames, bool(rng.integers(2)), int(rng.integers(1 << 30))))

    def pick_long(ok_too=None, **how):
        """now and then an edit of 4 hops and more of a sample that has them: what the loudness ops can measure afterwards
        -> (source, the least frames to take), (None, 1) otherwise"""
        fit = lambda m: enough(m) and (ok_too is None or ok_too(m))
        src = pick_source(ok=fit, **how) if rng.random() < LONG_SHARE else None
        return (src, 1) if src is None else (src, 4 * LM.hop_frames(live[src].rate))

    def op_derive():
        src, least = pick_long()
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
        if src is None:                                   # (resample -> derive -> resample: a chain the census wants)
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

    def follow_with_delete(named, fact):
        """after a refusal: a delete of one of its sources that no clip names must succeed (a pin left behind refuses it)"""
        c = [k for k in dict.fromkeys(named) if not live[k].refs]
        if c and rng.random() < .8:
            facts[fact] += 1
            do_delete(c[rng.integers(len(c))])

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
        named = [lead] + [pick_source(ok=lambda m: m.rate == rate) for _ in range(int(rng.integers(0, SPLICE_PARTS)))]
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
            boost = lambda m: MADE_ON_THE_DEVICE.get(m.kind, 1.0) * (3.0 if m.rate in (96000, 32000) else 2.0 if m.rate != RATE else 1.0)
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
        src = pick_source(editable=False, boost=lambda m: (12.0 if m.kind == "loudnorm" else 4.0) if off_rate_newcomer(m) else 1.0)
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
        w = np.array([(10.0 if live[p[0]].kind == "loudnorm" else 4.0) if off_rate_newcomer(live[p[0]]) else 1.0 for p in c])
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
                 loudness=op_loudness, export=op_export, mip=op_mip, delete=op_delete)
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
            self.put(op[1], op[2], op[4], upload_planes(op[7], op[2], op[3], op[5]))
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
        elif k == "delete":
            if op[2] == 0:
                del self.s[op[1]]
            return None
        else:
            return None
        return op[1]

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
