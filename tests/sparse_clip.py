"""Clips of up to 2^31-17 frames on the host without their memory: each channel is an anonymous private mapping made with
MAP_NORESERVE (pages appear on first touch, nothing is charged up front), filled only over the stretches a test reads, from
synth.py's index hash — the same values wbx_clip_synth writes on the device.  Every other frame reads 0, so a read outside
the filled stretches shows up as a wrong value: a test cannot pass on it by accident."""
from __future__ import annotations

import mmap
from typing import Iterable, List, Tuple

import numpy as np

from whitebox_amd import synth

CAP = 2**31 - 17          # the longest clip the ABI accepts (wbx.h: frames < 2^31-16)
PAD = 16                  # the reference's zero frames behind a clip (dsp/sample.h:19)
DTYPE = {"f32": np.float32, "i16": np.int16, "i24": np.int32, "i32": np.int32}
MAP_NORESERVE = getattr(mmap, "MAP_NORESERVE", 0x4000)   # (Linux; the module names it from Python 3.11 on)


def values(seed: int, s: synth.SampleSpec, chan: int, first: int, n: int) -> np.ndarray:
    """frames [first, first + n) of channel `chan` of sample `s`, as SessionSpec.sample_data makes them"""
    if s.fmt == "f32":
        return synth.clip_channel(seed, s.seed_track, chan, n, s.amp, first=first)
    if s.fmt == "i16":
        return synth.clip_channel_i16(seed, s.seed_track, chan, n, first=first)
    return synth.clip_channel_i32(seed, s.seed_track, chan, n, 24 if s.fmt == "i24" else 32, first=first)


def sparse_sample_data(seed: int, s: synth.SampleSpec, spans: Iterable[Tuple[int, int]]) -> List[np.ndarray]:
    """planar channel arrays of s.frames + 16 frames, the hash values over each [lo, hi) of `spans` (clamped to the clip),
    0 elsewhere (the 16 padding frames included)"""
    dt = np.dtype(DTYPE[s.fmt])
    spans = list(spans)
    out = []
    for c in range(s.channels):
        mm = mmap.mmap(-1, (s.frames + PAD) * dt.itemsize, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | MAP_NORESERVE)
        a = np.frombuffer(mm, dt)
        fill(a, seed, s, c, spans)
        out.append(a)
    return out


def fill(a: np.ndarray, seed: int, s: synth.SampleSpec, chan: int, spans: Iterable[Tuple[int, int]]) -> None:
    for lo, hi in spans:
        lo, hi = max(0, int(lo)), min(s.frames, int(hi))
        if hi > lo:
            a[lo:hi] = values(seed, s, chan, lo, hi - lo)


def clear(a: np.ndarray) -> None:
    """give every page of a sparse channel back: it reads 0 again"""
    a.base.obj.madvise(mmap.MADV_DONTNEED)   # (the array views the mapping through a memoryview)


def read_spans(records, samples, margin: int = 4) -> List[List[Tuple[int, int]]]:
    """per sample index, the frame stretches that stream calls (sample, sample_offset, num_actual, playback_speed) read —
    [floor(first x) - margin, floor(last x) + 2 + margin) — merged"""
    spans: List[List[Tuple[int, int]]] = [[] for _ in samples]
    for smp, off, n, sp in records:
        if n == 0 or off >= samples[smp].frames:
            continue
        lo = int(np.floor(off))
        hi = int(np.floor(off + (n - 1) * sp)) + 2
        spans[smp].append((lo - margin, hi + margin))
    merged = []
    for sp in spans:
        sp.sort()
        m: List[Tuple[int, int]] = []
        for lo, hi in sp:
            if m and lo <= m[-1][1]:
                m[-1] = (m[-1][0], max(m[-1][1], hi))
            else:
                m.append((lo, hi))
        merged.append(m)
    return merged


def rss_bytes() -> int:
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * mmap.PAGESIZE
