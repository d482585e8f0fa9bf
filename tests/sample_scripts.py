"""Sample life scripts: random chains of everything that puts audio into the engine's clip pool and takes it out again —
uploads, derived / normalized / resampled samples, recorder takes, bounces, deletes — with placements, playback, measure,
export and mip-maps in between, and the model of what every live sample must hold.  Pure Python (numpy): the generator works
on shapes alone (tests/test_sample_scripts.py takes its census without a device), Contents computes the exact fp32 planes
from tests/clipfx_model.py and tests/resample_model.py; takes and bounces get theirs from the rig that runs the script
(tests/test_gpu_sample_scripts.py), since they depend on the inputs fed and on the oracle engine's render.
TEST INFRASTRUCTURE — nothing here is shipped.

A script is a list of tuples; `key` names a sample inside the script (the product's ids are the rig's business):
    ("add", key, fmt, channels, rate, frames, interleaved, seed)
    ("derive", key, src, first, n, reverse, mode, gain, fade_in, fade_out, shape_in, shape_out)
    ("normalize", key, src, target_peak, first, n)
    ("resample", key, src, dst_rate, quality, first, n)
    ("take", key, track, kind, index, first_input_block, n_blocks, beat)       kind: record_model.MONO / STEREO
    ("bounce", keys, lo, hi, sources)                sources: ("track", t, "post" | "pre") / ("master",), one key each
    ("place", pid, src, track, lo, hi, start_offset) / ("unplace", pid)        a take's clip is placement ("take", key)
    ("play", beat, n_blocks)
    ("measure", src, first, n) / ("export", src, fmt, clamp, first, n) / ("mip", src, quality)
    ("delete", src, status)                          status: 0, or -4 while a clip names the sample
"""
from __future__ import annotations

import collections
import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

import clipfx_model as FX
import record_model as RM
import resample_model as RS

F, RATE, BPM, TRACKS, INPUTS = 128, 48000, 120.0, 4, 2
CHUNK, SPARE = 700, 4                 # the recorder's chunks (frames) and how many it keeps ahead
G = 64 << 10
SEEDS = tuple(range(12))
N_OPS = 48
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
PRODUCERS = ("add", "derive", "normalize", "resample", "take", "bounce")
KINDS = PRODUCERS + ("place", "unplace", "play", "measure", "export", "mip", "delete")
WEIGHTS = dict(add=7, derive=7, normalize=3, resample=7, take=3.5, bounce=3, place=5, unplace=2, play=4.5, measure=2,
               export=2, mip=2, delete=8)


def row_bytes(frames: int, fmt: str = "f32") -> int:
    return -(-(frames + 16) * (2 if fmt == "i16" else 4) // 256) * 256


def body_bytes(frames: int, channels: int, fmt: str = "f32") -> int:
    return -(-row_bytes(frames, fmt) * channels // G) * G


def pool_bounds(frames: int, channels: int, fmt: str = "f32") -> Tuple[int, int]:
    """what a clip takes from the pool: its body, and its body plus the widest gap in front of it"""
    body = body_bytes(frames, channels, fmt)
    return body, body + (min(16, body // G // 8 + 1) - 1) * G


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
    state = dict(beat=1.0, total=0, input_block=0, pid=0)

    def fresh(meta: Meta) -> int:
        key = next(keys)
        live[key] = meta
        order.append(key)
        size = pool_bounds(meta.frames, meta.channels, meta.fmt)
        state["total"] += size[1]
        facts["source:" + "->".join(meta.lineage[-3:])] += len(meta.lineage) >= 3
        if len(meta.lineage) >= 2:
            facts["source:" + "->".join(meta.lineage[-2:])] += 1
            facts["as_source:" + meta.lineage[-2]] += 1
        for h in list(pending_holes):
            if size[1] <= h:
                pending_holes.remove(h)
                facts["hole_refilled"] += 1
        return key

    def room(frames, channels, fmt="f32"):
        return state["total"] + pool_bounds(frames, channels, fmt)[1] <= BUDGET - (4 << 20)

    def region(beats):
        lo = state["beat"]
        state["beat"] = lo + beats + 4 * UNIT
        return lo

    def pick_source(editable=True, loud=False, chain=()):
        c = [k for k in order if (live[k].editable or not editable) and not (loud and live[k].quiet)]
        if not c:
            return None
        w = np.array([{"take": 5.0, "bounce": 4.0, "resample": 2.5, "derive": 2.0, "normalize": 2.0}.get(live[k].kind, 1.0) *
                      (6.0 if chain and live[k].lineage[-len(chain):] == chain else 1.0) for k in c])
        return c[rng.choice(len(c), p=w / w.sum())]

    def pick_range(m: Meta, most=MAX_FRAMES):
        n = int(rng.integers(1, min(m.frames, most) + 1)) if rng.random() < .6 else min(m.frames, most)
        first = int(rng.integers(0, m.frames - n + 1))
        if rng.random() < .3:
            first = m.frames - n      # up to the source's last frame
        return first, n

    def op_add():
        fmt = "i16" if rng.random() < .15 else "f32"
        channels, rate = int(rng.integers(1, 3)), int(rng.choice(RATES[:2]))
        frames = int(LENGTHS[rng.integers(len(LENGTHS))])
        if not room(frames, channels, fmt):
            frames = int(LENGTHS[rng.integers(8)])
        key = fresh(Meta("add", fmt, channels, rate, frames, ("add",), amp=0.5))
        ops.append(("add", key, fmt, channels, rate, frames, bool(rng.integers(2)), int(rng.integers(1 << 30))))

    def op_derive():
        src = pick_source()
        if src is None:
            return op_add()
        m = live[src]
        first, n = pick_range(m)
        mode = int(rng.choice(FX.MODES_FOR[m.channels]))
        out_ch = FX.out_channels(m.channels, mode)
        if not room(n, out_ch):
            return op_delete()
        top = min(1.1, 1.15 / m.amp)
        gain = float(np.float32(rng.uniform(0.3, top) * rng.choice([-1, 1])))
        fi, fo = (int(rng.integers(0, n + 1)) if rng.random() < .5 else 0 for _ in range(2))
        key = fresh(Meta("derive", "f32", out_ch, m.rate, n, m.lineage + ("derive",), m.amp * abs(gain), m.quiet))
        ops.append(("derive", key, src, first, n, bool(rng.integers(2)), mode, gain, fi, fo, int(rng.integers(3)), int(rng.integers(3))))

    def op_normalize():
        src = pick_source(loud=True)
        if src is None:
            return op_add()
        m = live[src]
        first, n = pick_range(m)
        if n < 8:
            first, n = 0, m.frames
        if n < 2 or not room(n, m.channels):
            return op_delete()
        target = float(np.float32(rng.uniform(0.2, 1.0)))
        key = fresh(Meta("normalize", "f32", m.channels, m.rate, n, m.lineage + ("normalize",), target))
        ops.append(("normalize", key, src, target, first, n))

    def op_resample():
        src = pick_source(chain=("resample", "derive"))   # (resample -> derive -> resample: a chain the census wants)
        if src is None:
            return op_add()
        m = live[src]
        dst = int(rng.choice([r for r in RATES if r != m.rate]))
        first, n = pick_range(m, most=MAX_FRAMES * m.rate // dst - 1)
        n_out = RS.out_frames(m.rate, dst, n)
        if not room(n_out, m.channels):
            return op_delete()
        key = fresh(Meta("resample", "f32", m.channels, dst, n_out, m.lineage + ("resample",), m.amp * 1.15, m.quiet))
        ops.append(("resample", key, src, dst, int(rng.choice(QUALITIES)), first, n))

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
        src = pick_source(editable=False)
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
        src, _, lo, hi, _, sounding = c[rng.integers(len(c))]
        n = int(rng.integers(3, 7))
        start = lo - float(rng.uniform(0.1, 1.0)) * UNIT
        if start + n * UNIT > lo + (sounding + 2) / F * UNIT and live[src].rate != RATE:
            facts["play_through_the_end_off_rate"] += 1
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
        if key != order[-1]:
            facts["delete_not_newest"] += 1
            pending_holes.append(pool_bounds(live[key].frames, live[key].channels, live[key].fmt)[0])
        order.remove(key)
        del live[key]
        ops.append(("delete", key, 0))

    table = dict(add=op_add, derive=op_derive, normalize=op_normalize, resample=op_resample, take=op_take, bounce=op_bounce,
                 place=op_place, unplace=op_unplace, play=op_play, measure=op_measure, export=op_export, mip=op_mip, delete=op_delete)
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
        elif k == "delete":
            if op[2] == 0:
                del self.s[op[1]]
            return None
        else:
            return None
        return op[1]


@functools.lru_cache(maxsize=None)
def _table(rs, rd, q):
    return RS.table(rs, rd, q)
