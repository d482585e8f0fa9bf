"""Python mirror of the reference's Engine / Track / AudioBuffer surface over the C ABI (include/wbx.h).

Same names and argument meaning as the reference (src/engine/engine.h, src/engine/track.h,
src/core/audio_buffer.h) so that the parity tests read like reference usage:

    eng = Engine(max_tracks=..., buffer_size=512, sample_rate=48000)     # set_audio_channel_config
    eng.set_bpm(120.0); t = eng.add_track("t"); t.set_volume(-3.0); t.set_pan(0.3)
    eng.add_audio_clip(t, "clip", min_time, max_time, start_offset, sample, speed=1.0, gain=1.0)
    eng.play(); eng.process(inp, out, 48000.0)

All arithmetic happens in libwbx.so on the GPU; this file only marshals.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import WbxError


class AudioBuffer:
    """Planar fp32 buffer with the reference's fields (core/audio_buffer.h:14-175): n_samples, n_channels,
    channel_buffers; clear() and mix() with the reference's meaning (host-side containers only)."""

    def __init__(self, sample_count: int = 0, channel_count: int = 0):
        self.n_samples = sample_count
        self.n_channels = channel_count
        self.channel_buffers = [np.zeros(sample_count, dtype=np.float32) for _ in range(channel_count)]

    def get_write_pointer(self, channel: int, sample_offset: int = 0) -> np.ndarray:
        assert channel < self.n_channels, "Channel out of range"
        return self.channel_buffers[channel][sample_offset:]

    get_read_pointer = get_write_pointer

    def clear(self) -> None:
        for b in self.channel_buffers:
            b[:] = 0

    def resize(self, samples: int, clear: bool = False) -> None:
        if samples == self.n_samples:
            return
        new = [np.zeros(samples, dtype=np.float32) for _ in range(self.n_channels)]
        if not clear:
            n = min(samples, self.n_samples)
            for a, b in zip(new, self.channel_buffers):
                a[:n] = b[:n]
        self.channel_buffers, self.n_samples = new, samples

    def resize_channel(self, channel_count: int) -> None:
        assert self.n_samples != 0
        while len(self.channel_buffers) < channel_count:
            self.channel_buffers.append(np.zeros(self.n_samples, dtype=np.float32))
        del self.channel_buffers[channel_count:]
        self.n_channels = channel_count

    def _ptrs(self):
        # (cached: the audio callback calls process() with the same buffer every block)
        key = tuple(b.ctypes.data for b in self.channel_buffers)
        if getattr(self, "_ptr_key", None) != key:
            arr_t = C.POINTER(C.c_float) * self.n_channels
            self._ptr_arr = arr_t(*[b.ctypes.data_as(C.POINTER(C.c_float)) for b in self.channel_buffers])
            self._ptr_key = key
        return self._ptr_arr


def _check(st: int, where: str, handle=None, engine: bool = False):
    if st != 0:
        L = _ffi.lib()
        detail = ""
        if handle:
            detail = (L.wbx_engine_last_error(handle) if engine else L.wbx_last_error(handle)).decode()
        raise WbxError(st, where, detail or L.wbx_status_string(st).decode())


def _export(fn, where, handle, engine, clip, fmt, channels, first_frame, n_frames, clamp, out):
    L = _ffi.lib()
    nbytes = L.wbx_export_bytes(_ffi.OUT_FMT[fmt], channels, n_frames)
    if out is None:
        out = np.zeros(max(nbytes, 1), dtype=np.uint8)[:nbytes].view(_ffi.OUT_DTYPE[fmt])
    else:
        assert out.nbytes >= nbytes and out.flags.c_contiguous and out.flags.writeable
    st = _ffi.ExportStats()
    _check(fn(handle, clip, first_frame, n_frames, _ffi.OUT_FMT[fmt], _ffi.EXPORT_CLAMP if clamp else 0, out.ctypes.data,
              C.byref(st)), where, handle, engine)
    return out, {"peak": [float(np.float32(st.peak[c])) for c in range(channels)],
                 "over": [int(st.over[c]) for c in range(channels)], "nans": [int(st.nans[c]) for c in range(channels)]}


def edit_desc(first_frame: int, n_frames: int, reverse: bool = False, channel_mode="keep", gain: float = 1.0,
              fade_in: int = 0, fade_out: int = 0, fade_in_shape="linear", fade_out_shape="linear", flags: Optional[int] = None):
    """a wbx_clip_edit_desc; mode and shapes by name or as the raw integers, `flags` overrides `reverse`"""
    return _ffi.ClipEditDesc(first_frame, n_frames, (_ffi.EDIT_REVERSE if reverse else 0) if flags is None else flags,
                             _ffi.CH_MODE.get(channel_mode, channel_mode), gain, 0, fade_in, fade_out,
                             _ffi.FADE_SHAPE.get(fade_in_shape, fade_in_shape), _ffi.FADE_SHAPE.get(fade_out_shape, fade_out_shape))


def splice_part(src_clip: int, first_frame: int, n_frames: int, at: int = 0, reverse: bool = False, channel_mode="keep",
                gain: float = 1.0, fade_in: int = 0, fade_out: int = 0, fade_in_shape="linear", fade_out_shape="linear",
                flags: Optional[int] = None):
    """a wbx_splice_part: edit_desc's edit of clip (or sample) `src_clip`, its first frame placed at output frame `at`"""
    return _ffi.SplicePart(src_clip, (_ffi.EDIT_REVERSE if reverse else 0) if flags is None else flags, first_frame, n_frames, at,
                           _ffi.CH_MODE.get(channel_mode, channel_mode), gain, fade_in, fade_out,
                           _ffi.FADE_SHAPE.get(fade_in_shape, fade_in_shape), _ffi.FADE_SHAPE.get(fade_out_shape, fade_out_shape))


def _part_array(parts):
    return (_ffi.SplicePart * len(parts))(*parts) if parts else None


def splice_plan(channels: int, n_frames: int, parts, sources, tables: bool = True):
    """wbx_splice_plan (host-only): the refusals of a part list against `sources` — {clip id: (channels, frames, rate, fmt)},
    fmt a name of _ffi.FMT — and the tile table.  Returns (tile_off, tile_parts) as uint32 arrays, or (n_tiles, n_entries)
    with tables=False; WbxError where the library refuses the list."""
    L = _ffi.lib()
    n_src = max(sources) + 1 if sources else 0
    src = (_ffi.SpliceSource * max(n_src, 1))()
    for k, (ch, frames, rate, fmt) in sources.items():
        src[k] = _ffi.SpliceSource(ch, rate, frames, _ffi.FMT.get(fmt, fmt), 0)
    arr = _part_array(parts)
    nt, ne = C.c_uint64(), C.c_uint64()
    _check(L.wbx_splice_plan(channels, n_frames, arr, len(parts), src, n_src, C.byref(nt), C.byref(ne), None, 0, None, 0),
           "wbx_splice_plan")
    if not tables:
        return nt.value, ne.value
    off, ent = np.zeros(nt.value + 1, dtype=np.uint32), np.zeros(max(ne.value, 1), dtype=np.uint32)
    _check(L.wbx_splice_plan(channels, n_frames, arr, len(parts), src, n_src, None, None, off.ctypes.data, off.size,
                             ent.ctypes.data, ent.size), "wbx_splice_plan")
    return off, ent[:ne.value]


def resample_plan(src_rate: int, dst_rate: int, quality="good") -> dict:
    """wbx_resample_plan (host-only): {"L", "M", "half_width", "taps", "table_floats"} of a conversion; WbxError where the
    library refuses it (status -4: a rate of 0, equal rates, unknown quality; -3: L > 1280 or more than 512 taps)"""
    info = _ffi.ResampleInfo()
    _check(_ffi.lib().wbx_resample_plan(src_rate, dst_rate, _ffi.SRC_QUALITY.get(quality, quality), C.byref(info)), "wbx_resample_plan")
    return {k: int(getattr(info, k)) for k, _ in _ffi.ResampleInfo._fields_}


def resample_frames(src_rate: int, dst_rate: int, n_frames: int) -> int:
    """wbx_resample_frames (host-only): ceil(n_frames * L / M), the length of the converted range; 0 when refused"""
    return int(_ffi.lib().wbx_resample_frames(src_rate, dst_rate, n_frames))


def _launch_shape(fn, what, *args) -> dict:
    v = [C.c_uint32() for _ in range(4)]
    _check(fn(*args, *[C.byref(x) for x in v]), what)
    return dict(zip(("tile", "span", "n_tiles", "grid"), (x.value for x in v)))


def clipfx_pass_frames() -> int:
    """wbx_clipfx_pass_frames (host-only): the frames one pass of the measure / derive kernel's capped grid covers"""
    return int(_ffi.lib().wbx_clipfx_pass_frames())


def resample_launch_shape(src_rate: int, dst_rate: int, quality, n_out: int) -> dict:
    """wbx_resample_launch_shape (host-only): {"tile", "span", "n_tiles", "grid"} of the conversion's launch for n_out output
    frames; n_tiles > grid means the grid's workgroups take a second pass over the tiles"""
    return _launch_shape(_ffi.lib().wbx_resample_launch_shape, "wbx_resample_launch_shape", src_rate, dst_rate,
                         _ffi.SRC_QUALITY.get(quality, quality), n_out)


def resample_table(src_rate: int, dst_rate: int, quality="good") -> np.ndarray:
    """wbx_resample_table (host-only): the fp32 coefficients in phase order, [L][taps]"""
    p = resample_plan(src_rate, dst_rate, quality)
    out = np.zeros((p["L"], p["taps"]), dtype=np.float32)
    _check(_ffi.lib().wbx_resample_table(src_rate, dst_rate, _ffi.SRC_QUALITY.get(quality, quality), out.ctypes.data, out.size),
           "wbx_resample_table")
    return out


def filter_design(rate: int, kind, freq: float, q: float = 0.7071067811865476, gain_db: float = 0.0) -> np.ndarray:
    """wbx_filter_design (host-only): b0 b1 b2 a1 a2 (a0 = 1) of one Audio-EQ-Cookbook biquad at `rate` — kind "lowpass" /
    "highpass" / "bandpass" / "notch" / "allpass" / "peak" / "lowshelf" / "highshelf" (or WBX_FILT_*); `gain_db` becomes the
    library's LINEAR amplitude ratio here, 10 ** (gain_db / 20).  WbxError (-4) where the library refuses the design"""
    out = np.zeros(5, dtype=np.float64)
    _check(_ffi.lib().wbx_filter_design(rate, _ffi.FILTER_KIND.get(kind, kind), float(freq), float(q),
                                        10.0 ** (float(gain_db) / 20.0), out.ctypes.data), "wbx_filter_design")
    return out


def _cascade(coef) -> np.ndarray:
    """[stages][5] fp64, contiguous (one stage may be given flat)"""
    k = np.ascontiguousarray(coef, dtype=np.float64)
    return k.reshape(-1, 5)


def filter_transition(coef) -> np.ndarray:
    """wbx_filter_transition (host-only): the carry matrix [D][D], D = 2 * stages + 2, of a cascade [stages][5] over one chunk
    of wbx_filter_chunk_frames() = 512 frames; WbxError (-4) for a cascade wbx_filter_check refuses"""
    k = _cascade(coef)
    D = 2 * len(k) + 2
    M = np.zeros((D, D), dtype=np.float64)
    _check(_ffi.lib().wbx_filter_transition(k.ctypes.data, len(k), M.ctypes.data, M.size), "wbx_filter_transition")
    return M


def fir_design(rate: int, kind, f1: float, f2: float = 0.0, n_taps: int = 255, beta: float = 8.6) -> np.ndarray:
    """wbx_fir_design (host-only): `n_taps` (odd, 3 .. 65535) fp32 taps of a linear-phase Kaiser-windowed sinc at `rate` —
    kind "lowpass" / "highpass" (edge f1) / "bandpass" / "bandstop" (edges f1 < f2), or WBX_FIR_*; beta 8.6 is about 90 dB
    of stop band.  The delay is (n_taps - 1) // 2 frames: convolve with out_first = that to drop it.  WbxError (-4) where
    the library refuses the design"""
    out = np.zeros(max(int(n_taps), 1), dtype=np.float32)
    _check(_ffi.lib().wbx_fir_design(rate, _ffi.FIR_KIND.get(kind, kind), float(f1), float(f2), n_taps, float(beta),
                                     out.ctypes.data, out.size), "wbx_fir_design")
    return out


def convolve_frames(n_frames: int, ir_frames: int) -> int:
    """wbx_convolve_frames (host-only): the full result's length n_frames + ir_frames - 1; 0 where every window is refused"""
    return int(_ffi.lib().wbx_convolve_frames(n_frames, ir_frames))


def limit_ramp(lookahead_frames: int, hold_frames: int, release_frames: int) -> np.ndarray:
    """wbx_limit_ramp (host-only): the A + H + R doubles of the limiter's ramp table, table[k + A] = ramp[k]: 0.0 through the
    look-ahead and the hold, then (k - H) / R.  WbxError (-4) where the library refuses the shape"""
    n = max(int(lookahead_frames) + int(hold_frames) + int(release_frames), 1)
    out = np.zeros(n, dtype=np.float64)
    _check(_ffi.lib().wbx_limit_ramp(lookahead_frames, hold_frames, release_frames, out.ctypes.data, out.size), "wbx_limit_ramp")
    return out


def limit_frames(rate: int, lookahead_ms: float = 1.5, hold_ms: float = 0.0, release_ms: float = 100.0) -> tuple:
    """(lookahead_frames, hold_frames, release_frames) of the times at `rate`, rounded to the nearest frame; the release is
    at least one frame.  A convenience of this module: not part of the bit-exact contract"""
    f = lambda ms: int(round(float(ms) * rate / 1000.0))
    return f(lookahead_ms), f(hold_ms), max(1, f(release_ms))


def _limit_stats(st) -> dict:
    return {"peak_in": st.peak_in, "min_gain": st.min_gain, "min_gain_frame": st.min_gain_frame, "limited_frames": st.limited_frames}


def dynamics_table(kind, threshold_db: float, ratio: float, knee_db: float = 0.0, range_db: float = -np.inf) -> np.ndarray:
    """wbx_dynamics_table (host-only): the WBX_DYN_TABLE = 3073 gains over level of the usual static curve — kind "compress"
    (above the threshold the gain in dB is (1 / ratio - 1) * (L - T)) or "gate" (a downward expander: below it,
    (ratio - 1) * (L - T)), with a quadratic knee of knee_db and never below range_db.  WbxError (-4) where the library
    refuses the design"""
    out = np.zeros(_ffi.DYN_TABLE, dtype=np.float64)
    _check(_ffi.lib().wbx_dynamics_table(_ffi.DYN_SENSE.get(kind, kind), float(threshold_db), float(ratio), float(knee_db),
                                         float(range_db), out.ctypes.data, out.size), "wbx_dynamics_table")
    return out


def _dyn_table(table) -> np.ndarray:
    t = np.ascontiguousarray(table, dtype=np.float64)
    assert t.shape == (_ffi.DYN_TABLE,), "a dynamics table has 3073 entries"
    return t


def dynamics_check(table, sense="compress") -> float:
    """wbx_dynamics_check (host-only): the smallest entry of a table the library accepts; WbxError (-4) for one it refuses
    (an entry that is not finite, carries a sign bit or exceeds 1.0)"""
    t, lo = _dyn_table(table), C.c_double()
    _check(_ffi.lib().wbx_dynamics_check(t.ctypes.data, _ffi.DYN_SENSE.get(sense, sense), C.byref(lo)), "wbx_dynamics_check")
    return lo.value


def dynamics_lookup(table, level: float) -> float:
    """wbx_dynamics_lookup (host-only): the gain the table gives one level (linear, >= 0), as the device interpolates it"""
    t, out = _dyn_table(table), C.c_double()
    _check(_ffi.lib().wbx_dynamics_lookup(t.ctypes.data, float(level), C.byref(out)), "wbx_dynamics_lookup")
    return out.value


def _dynamics_stats(st) -> dict:
    return {"min_gain": st.min_gain, "min_gain_frame": st.min_gain_frame, "reduced_frames": st.reduced_frames}


def saturate_table(kind="cubic", bias: float = 0.0) -> np.ndarray:
    """wbx_saturate_table (host-only): the WBX_SAT_TABLE = 16385 outputs over the driven level -8 .. +8 of a usual curve —
    kind "hard" (a clamp to +-1), "cubic" (z - 4 z^3 / 27, +-1 from |z| = 1.5 on) or "tanh" —, f(v + bias) - f(bias): a bias
    (|bias| <= 4) gives even harmonics.  WbxError (-4) where the library refuses the design"""
    out = np.zeros(_ffi.SAT_TABLE, dtype=np.float64)
    _check(_ffi.lib().wbx_saturate_table(_ffi.SAT_KIND.get(kind, kind), float(bias), out.ctypes.data, out.size), "wbx_saturate_table")
    return out


def _sat_table(table) -> np.ndarray:
    t = np.ascontiguousarray(table, dtype=np.float64)
    assert t.shape == (_ffi.SAT_TABLE,), "a saturate table has 16385 entries"
    return t


def saturate_check(table) -> None:
    """wbx_saturate_check (host-only): WbxError (-4) for a table the library refuses (an entry that is not finite or whose
    magnitude exceeds 2^32)"""
    _check(_ffi.lib().wbx_saturate_check(_sat_table(table).ctypes.data), "wbx_saturate_check")


def saturate_lookup(table, d: float) -> float:
    """wbx_saturate_lookup (host-only): what the table gives one driven sample `d`, as the device interpolates it"""
    t, out = _sat_table(table), C.c_double()
    _check(_ffi.lib().wbx_saturate_lookup(t.ctypes.data, float(d), C.byref(out)), "wbx_saturate_lookup")
    return out.value


def saturate_launch_shape(os: int, quality, channels: int, n_frames: int) -> dict:
    """wbx_saturate_launch_shape (host-only): how a wbx_clip_saturate call is launched — the tile (output frames per
    workgroup), the mid samples and source frames a tile computes and stages per channel, its LDS bytes and the tiles (the
    grid).  WbxError where the call would be refused for os, quality or n_frames"""
    v = [C.c_uint32() for _ in range(5)]
    _check(_ffi.lib().wbx_saturate_launch_shape(os, _ffi.SRC_QUALITY.get(quality, quality), channels, n_frames,
                                                *[C.byref(x) for x in v]), "wbx_saturate_launch_shape")
    return dict(zip(("tile", "mid_span", "src_span", "lds_bytes", "n_tiles"), (x.value for x in v)))


def _saturate_stats(st) -> dict:
    return {"peak_drive": st.peak_drive, "peak_index": st.peak_index, "beyond": st.beyond}


def denoise_tables(window_frames: int):
    """wbx_denoise_tables (host-only): the analysis and the synthesis tables of a window of `window_frames` (a power of two
    in 64 .. 2048) as float32 arrays [2][B][W] each — [0] the cosine table (AC / YC), [1] the sine table (AS / YS),
    B = W / 2 + 1.  WbxError (-4) for a window the call refuses"""
    W = int(window_frames)
    ok = 64 <= W <= 2048 and W & (W - 1) == 0
    B = W // 2 + 1 if ok else 1
    a, y = np.zeros((2, B, W if ok else 1), dtype=np.float32), np.zeros((2, B, W if ok else 1), dtype=np.float32)
    _check(_ffi.lib().wbx_denoise_tables(W, a.ctypes.data, y.ctypes.data), "wbx_denoise_tables")
    return a, y


def _vs_q(quality) -> int:
    return _ffi.SRC_QUALITY.get(quality, quality)


def _vs_knots(knots) -> np.ndarray:
    return np.ascontiguousarray(knots, dtype=np.int64)


def varispeed_plan(quality="good", guard_num: int = 1, guard_den: int = 1) -> dict:
    """wbx_varispeed_plan (host-only): {"H", "T", "P", "cutoff", "beta"} of the interpolator that protects speeds up to
    guard_num / guard_den (>= 1) from aliasing.  WbxError where the library refuses it"""
    v = _ffi.VarispeedInfo()
    _check(_ffi.lib().wbx_varispeed_plan(_vs_q(quality), guard_num, guard_den, C.byref(v)), "wbx_varispeed_plan")
    return {"H": v.half_width, "T": v.taps, "P": v.phases, "cutoff": v.cutoff, "beta": v.beta}


def varispeed_table(quality="good", guard_num: int = 1, guard_den: int = 1):
    """wbx_varispeed_table (host-only): (h float32[P + 1][T], d float32[P][T]) — the phase rows and their differences"""
    p = varispeed_plan(quality, guard_num, guard_den)
    h = np.zeros((p["P"] + 1, p["T"]), dtype=np.float32)
    d = np.zeros((p["P"], p["T"]), dtype=np.float32)
    _check(_ffi.lib().wbx_varispeed_table(_vs_q(quality), guard_num, guard_den, h.ctypes.data, d.ctypes.data, h.size), "wbx_varispeed_table")
    return h, d


def varispeed_position(knots, knot_shift: int, j: int) -> int:
    """wbx_varispeed_position (host-only): the position of output frame j on the curve, in 2^-32 source frames"""
    k, out = _vs_knots(knots), C.c_int64()
    _check(_ffi.lib().wbx_varispeed_position(k.ctypes.data, k.size, knot_shift, j, C.byref(out)), "wbx_varispeed_position")
    return out.value


def varispeed_check(knots, knot_shift: int, n_frames: int, out_frames: int, quality="good", guard_num: int = 1, guard_den: int = 1) -> int:
    """wbx_varispeed_check (host-only): the status a call with these sizes and this curve is refused with before its clip
    is looked at (0: accepted).  `knots` may be None (a NULL pointer)"""
    k = None if knots is None else _vs_knots(knots)
    return int(_ffi.lib().wbx_varispeed_check(None if k is None else k.ctypes.data, 0 if k is None else k.size, knot_shift, n_frames,
                                              out_frames, _vs_q(quality), guard_num, guard_den))


def varispeed_tiles(knots, knot_shift: int, n_frames: int, out_frames: int, quality="good", guard_num: int = 1, guard_den: int = 1) -> list:
    """wbx_varispeed_tiles (host-only): the tiles a call is launched over, [(first_out, n_out, lo_frame, span)].  WbxError
    where wbx_varispeed_check refuses the call"""
    k, n = _vs_knots(knots), C.c_uint64()
    L, args = _ffi.lib(), (knot_shift, n_frames, out_frames, _vs_q(quality), guard_num, guard_den)
    _check(L.wbx_varispeed_tiles(k.ctypes.data, k.size, *args, None, 0, C.byref(n)), "wbx_varispeed_tiles")
    rec = (_ffi.VarispeedTile * max(1, n.value))()
    _check(L.wbx_varispeed_tiles(k.ctypes.data, k.size, *args, C.addressof(rec), n.value, C.byref(n)), "wbx_varispeed_tiles")
    return [(t.first_out, t.n_out, t.lo_frame, t.span) for t in rec[:n.value]]


def _vs_guard(speed: float):
    """a guard >= max(1, speed) in sixteenths"""
    return (max(16, int(np.ceil(float(speed) * 16.0 - 1e-9))), 16)


def varispeed_knots(points, out_frames: int, knot_shift: int = 6, start: float = 0.0):
    """The knots of a speed curve given as breakpoints (out_frame, speed), ascending in out_frame, with LINEAR speed ramps
    between them (constant before the first and behind the last): the position is the integral of the speed from `start`
    (source frames) at output frame 0.  Float arithmetic on the host, outside the bit-exact contract; the call is exact for
    the knots returned.  Returns (knots int64[K], (guard_num, guard_den)) — the guard covers the fastest breakpoint"""
    pts = [(float(j), float(s)) for j, s in points]
    assert pts and all(a[0] < b[0] for a, b in zip(pts, pts[1:])), "varispeed_knots: breakpoints ascend in out_frame"
    G = 1 << knot_shift
    K = (out_frames + G - 1) // G + 1
    j = np.arange(K, dtype=np.float64) * G
    jp = np.array([p[0] for p in pts])
    sp = np.array([p[1] for p in pts])
    # position at the breakpoints (trapezoids), from output frame 0 where the speed is the first breakpoint's
    at = np.concatenate(([0.0], np.cumsum(0.5 * (sp[1:] + sp[:-1]) * np.diff(jp)))) + sp[0] * jp[0]
    seg = np.clip(np.searchsorted(jp, j, side="right") - 1, 0, len(pts) - 1)
    dj = j - jp[seg]
    slope = np.zeros(len(pts))
    slope[:-1] = np.diff(sp) / np.diff(jp)
    pos = np.where(j < jp[0], sp[0] * j, at[seg] + sp[seg] * dj + 0.5 * slope[seg] * dj * dj)
    knots = np.array([int(round((float(start) + float(v)) * 4294967296.0)) for v in pos], dtype=np.int64)
    return knots, _vs_guard(np.max(np.abs(sp)))


def denoise_threshold(sums, hops: int, strength: float) -> np.ndarray:
    """wbx_denoise_threshold (host-only): strength * (sums / hops) — the per-bin threshold of a profile's sums"""
    s = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    out = np.zeros_like(s)
    _check(_ffi.lib().wbx_denoise_threshold(s.ctypes.data, hops, s.size, float(strength), out.ctypes.data), "wbx_denoise_threshold")
    return out


def denoise_hops(n_frames: int, window_frames: int) -> int:
    """wbx_denoise_hops (host-only): T = ceil(n_frames / (window_frames / 4)) + 3; 0 where the call refuses either"""
    return int(_ffi.lib().wbx_denoise_hops(n_frames, window_frames))


def denoise_band_hops(window_frames: int, channels: int) -> int:
    """wbx_denoise_band_hops (host-only): the blocks of window_frames / 4 output frames one band of a call covers"""
    return int(_ffi.lib().wbx_denoise_band_hops(window_frames, channels))


def _denoise_thr(thr) -> np.ndarray:
    return np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)


def _denoise_stats(st) -> dict:
    return {"hops": st.hops, "cells": st.cells, "open_cells": st.open_cells, "bands": st.bands}


def stretch_steps(out_frames: int, window_frames: int) -> int:
    """wbx_stretch_steps (host-only): K = ceil(out_frames / (window_frames / 2)); 0 for a window a stretch refuses"""
    return int(_ffi.lib().wbx_stretch_steps(out_frames, window_frames))


def stretch_anchor(k: int, n_frames: int, out_frames: int, window_frames: int) -> int:
    """wbx_stretch_anchor (host-only): a_k = floor(k * (window_frames / 2) * n_frames / out_frames)"""
    return int(_ffi.lib().wbx_stretch_anchor(k, n_frames, out_frames, window_frames))


def stretch_window(window_frames: int) -> tuple:
    """wbx_stretch_window (host-only): (w_up, w_dn), the two halves of the overlap-add window, window_frames / 2 doubles
    each.  WbxError (-4) where the library refuses the window"""
    out = np.zeros(max(int(window_frames), 1), dtype=np.float64)
    _check(_ffi.lib().wbx_stretch_window(window_frames, out.ctypes.data, out.size), "wbx_stretch_window")
    return out[:window_frames // 2].copy(), out[window_frames // 2:].copy()


def _stretch_info(si) -> dict:
    return {"steps": si.steps, "searched_steps": si.searched_steps, "candidates": si.candidates, "max_shift": si.max_shift,
            "launches": si.launches}


def _warp_markers(markers):
    """(ctypes array or None, M) for a sequence of (src_frame, out_frame) pairs"""
    pairs = [(int(a), int(b)) for a, b in markers] if markers is not None else []
    if not pairs:
        return None, 0
    arr = (_ffi.WarpMarker * len(pairs))()
    for i, (a, b) in enumerate(pairs):
        arr[i].src_frame, arr[i].out_frame = a, b
    return arr, len(pairs)


def warp_check(n_frames: int, out_frames: int, markers, window_frames: int = 2048, tolerance_frames: int = 512) -> int:
    """wbx_warp_check (host-only): the status a warp call gets before its clip is looked at (0: none)"""
    arr, M = _warp_markers(markers)
    return int(_ffi.lib().wbx_warp_check(n_frames, out_frames, arr, M, window_frames, tolerance_frames))


def warp_steps(n_frames: int, out_frames: int, markers, window_frames: int = 2048) -> int:
    """wbx_warp_steps (host-only): K, the sum of the segments' ceil(m_j / Hs); 0 for a window or markers the call refuses"""
    arr, M = _warp_markers(markers)
    return int(_ffi.lib().wbx_warp_steps(n_frames, out_frames, arr, M, window_frames))


def warp_segments(n_frames: int, out_frames: int, markers, window_frames: int = 2048) -> list:
    """wbx_warp_segments (host-only): the S = M + 1 segments as (src_frame, out_frame, first_step, steps)"""
    arr, M = _warp_markers(markers)
    out = (_ffi.WarpSegment * (M + 1))()
    _check(_ffi.lib().wbx_warp_segments(n_frames, out_frames, arr, M, window_frames, out, M + 1), "wbx_warp_segments")
    return [(g.src_frame, g.out_frame, g.first_step, g.steps) for g in out]


def warp_launches(n_frames: int, out_frames: int, markers, window_frames: int = 2048, tolerance_frames: int = 512) -> int:
    """wbx_warp_launches (host-only): the kernel launches a warp call makes; 0 for a call wbx_warp_check refuses"""
    arr, M = _warp_markers(markers)
    return int(_ffi.lib().wbx_warp_launches(n_frames, out_frames, arr, M, window_frames, tolerance_frames))


def _warp_info(wi) -> dict:
    return {"steps": wi.steps, "searched_steps": wi.searched_steps, "candidates": wi.candidates, "max_shift": wi.max_shift,
            "launches": wi.launches, "segments": wi.segments, "longest_segment_steps": wi.longest_segment_steps}


def pitch_mid_frames(out_frames: int, num: int, den: int) -> int:
    """wbx_pitch_mid_frames (host-only): m' = ceil(out_frames * M / L), the frames of the stretched intermediate of a pitch
    shift by num / den (M / L in lowest terms); 0 where the call would refuse the ratio"""
    return int(_ffi.lib().wbx_pitch_mid_frames(out_frames, num, den))


def pitch_launch_shape(num: int, den: int, quality, out_frames: int) -> dict:
    """wbx_pitch_launch_shape (host-only): resample_launch_shape of a pitch call's last launch"""
    return _launch_shape(_ffi.lib().wbx_pitch_launch_shape, "wbx_pitch_launch_shape", num, den,
                         _ffi.SRC_QUALITY.get(quality, quality), out_frames)


def pitch_ratio(semitones: float, cents: float = 0.0) -> tuple:
    """(num, den) for a transposition by `semitones` and `cents` in equal temperament: the fraction with a denominator of
    at most 1280 nearest to 2 ** ((100 * semitones + cents) / 1200) — within 0.4 cent for every whole cent of two octaves
    either way.  A convenience outside the bit-exact contract.  ValueError where the fraction is 1 (nothing to shift)"""
    f = Fraction(2.0 ** ((100.0 * float(semitones) + float(cents)) / 1200.0)).limit_denominator(1280)
    if f == 1:
        raise ValueError("pitch_ratio: the ratio is 1 (use stretch_sample to change the length alone)")
    return f.numerator, f.denominator


def _pitch_info(pi) -> dict:
    return {k: getattr(pi, k) for k, _ in _ffi.PitchInfo._fields_}


# wbx_f0_frame as a numpy record: what clip_f0 and f0_sample return, one per hop
F0_DTYPE = np.dtype([("period", "<f8"), ("dip", "<f8"), ("energy", "<f8"), ("lag", "<u4"), ("voiced", "<u4")])


def f0_hops(n_frames: int, window_frames: int, hop_frames: int, tau_max: int) -> int:
    """wbx_f0_hops (host-only): the complete analysis frames of n_frames — (n - W - tau_max) // H + 1, or 0 where the range
    is shorter than W + tau_max or the call would refuse the shape"""
    return int(_ffi.lib().wbx_f0_hops(n_frames, window_frames, hop_frames, tau_max))


def _run_f0(fn, what, h, engine, ident, first_frame, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold):
    hops = f0_hops(n_frames, window_frames, hop_frames, tau_max)
    # the call's own argument check first, so that a refused call (2^31 hops of one frame, say) allocates no records
    _check(_ffi.lib().wbx_f0_check(n_frames, window_frames, hop_frames, tau_min, tau_max, threshold, 1, hops), "wbx_f0_check")
    rec = np.zeros(hops, dtype=F0_DTYPE)
    fi = _ffi.F0Info()
    _check(fn(h, ident, first_frame, n_frames, window_frames, hop_frames, tau_min, tau_max, threshold,
              rec.ctypes.data if rec.size else None, rec.size, C.byref(fi)), what, h, engine)
    return rec, {k: getattr(fi, k) for k, _ in _ffi.F0Info._fields_ if k != "_pad"}


# wbx_onset_frame as a numpy record: what clip_onsets and onsets_sample return, one per hop
ONSET_DTYPE = np.dtype([("energy", "<f8"), ("edge_energy", "<f8"), ("novelty", "<f8"), ("onset", "<u4"), ("_pad", "<u4")])


def onset_hops(n_frames: int, hop_frames: int) -> int:
    """wbx_onset_hops (host-only): the complete hops of n_frames — n // H, or 0 where the call would refuse the hop length"""
    return int(_ffi.lib().wbx_onset_hops(n_frames, hop_frames))


def _run_onsets(fn, what, h, engine, ident, first_frame, n_frames, hop_frames, floor_power, threshold, delta, w, a):
    hops = onset_hops(n_frames, hop_frames)
    # the call's own argument check first, so that a refused call allocates no records
    _check(_ffi.lib().wbx_onset_check(n_frames, hop_frames, floor_power, threshold, delta, w, a, 1, hops), "wbx_onset_check")
    rec = np.zeros(hops, dtype=ONSET_DTYPE)
    oi = _ffi.OnsetInfo()
    _check(fn(h, ident, first_frame, n_frames, hop_frames, floor_power, threshold, delta, w, a,
              rec.ctypes.data if rec.size else None, rec.size, C.byref(oi)), what, h, engine)
    return rec, {k: getattr(oi, k) for k, _ in _ffi.OnsetInfo._fields_ if k != "_pad"}


def _run_tempo(fn, what, h, engine, ident, first_frame, n_frames, hop_frames, floor_power, window_hops, step_hops, lag_min, lag_max,
               threshold):
    cap = f0_hops(onset_hops(n_frames, hop_frames), window_hops, step_hops, lag_max)   # (at most 2^20 / step_hops, or the call refuses)
    cap = min(cap, 1 << 20)
    rec = np.zeros(cap, dtype=F0_DTYPE)
    fi = _ffi.F0Info()
    _check(fn(h, ident, first_frame, n_frames, hop_frames, floor_power, window_hops, step_hops, lag_min, lag_max, threshold,
              rec.ctypes.data if rec.size else None, rec.size, C.byref(fi)), what, h, engine)
    return rec, {k: getattr(fi, k) for k, _ in _ffi.F0Info._fields_ if k != "_pad"}


# wbx_align_point as a numpy record: what clip_align and align_samples return as the curve, one per lag from lag_min upward
ALIGN_CURVE_DTYPE = np.dtype([("r", "<f8"), ("energy", "<f8")])
ALIGN_EITHER_POLARITY = _ffi.ALIGN_EITHER_POLARITY


def align_chunks(n_frames: int) -> int:
    """wbx_align_chunks (host-only): ceil(n_frames / 2048), or 0 where the call would refuse the template's length"""
    return int(_ffi.lib().wbx_align_chunks(n_frames))


def align_check(n_frames: int, m_frames: int, lag_min: int, lag_max: int, flags: int = 0, has_info: bool = True,
                has_curve: bool = False, curve_cap: int = 0) -> int:
    """wbx_align_check (host-only): the status a call of these sizes gets before its clips are looked at (0: none)"""
    return int(_ffi.lib().wbx_align_check(n_frames, m_frames, lag_min, lag_max, flags, int(has_info), int(has_curve), curve_cap))


def _run_align(fn, what, h, engine, ref, a_first, n_frames, ident, b_first, m_frames, lag_min, lag_max, either_polarity, curve):
    flags = ALIGN_EITHER_POLARITY if either_polarity is True else int(either_polarity)
    lags = lag_max - lag_min + 1
    # the call's own argument check first, so that a refused call allocates no curve
    _check(align_check(n_frames, m_frames, lag_min, lag_max, flags, True, bool(curve), max(lags, 0)), "wbx_align_check")
    pts = np.zeros(lags, dtype=ALIGN_CURVE_DTYPE) if curve else None
    ai = _ffi.AlignInfo()
    _check(fn(h, ref, a_first, n_frames, ident, b_first, m_frames, lag_min, lag_max, flags, C.byref(ai),
              pts.ctypes.data if curve else None, lags if curve else 0), what, h, engine)
    return {k: getattr(ai, k) for k, _ in _ffi.AlignInfo._fields_ if k != "_pad"}, pts


SPECTRUM_MID = _ffi.SPECTRUM_MID   # clip_spectrum's channel: f0's detector (mono the sample, stereo the rounded mean)


def spectrum_hops(n_frames: int, window_frames: int, hop_frames: int) -> int:
    """wbx_spectrum_hops (host-only): the complete analysis frames of n_frames — (n - W) // H + 1, or 0 where the range is
    shorter than W or the call would refuse the window or the hop length"""
    return int(_ffi.lib().wbx_spectrum_hops(n_frames, window_frames, hop_frames))


def spectrum_basis(window_frames: int, freqs, lengths=None, window="hann", kaiser_beta: float = 8.6) -> np.ndarray:
    """wbx_spectrum_basis (host-only): the 2 * B * W fp32 words of a basis for clip_spectrum — bin b at freqs[b] cycles per
    frame (0 .. 0.5) with its own window of lengths[b] frames (4 .. W; None: all W) centred in W; window "rect" / "hann" /
    "kaiser" (or WBX_WINDOW_*), normalised so that a full-scale sine on a bin has power 0.25.  WbxError (-4) where the
    library refuses the design"""
    f = np.ascontiguousarray(freqs, dtype=np.float64)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
    assert f.ndim == 1 and (ln is None or ln.shape == f.shape)
    frames = int(_ffi.lib().wbx_spectrum_basis_frames(window_frames, f.size))
    out = np.zeros(max(frames, 1), dtype=np.float32)
    _check(_ffi.lib().wbx_spectrum_basis(window_frames, f.size, f.ctypes.data, None if ln is None else ln.ctypes.data,
                                         _ffi.WINDOW_KIND.get(window, window), float(kaiser_beta), out.ctypes.data),
           "wbx_spectrum_basis")
    return out


def spectrum_log_freqs(f_min: float, bins_per_octave: float, n_bins: int):
    """wbx_spectrum_log_freqs (host-only): (f_min * 2 ** (b / bins_per_octave) for b in 0 .. n_bins - 1 in cycles per frame,
    without libm; how many were clamped at 0.5)"""
    out = np.zeros(max(int(n_bins), 1), dtype=np.float64)
    clamped = C.c_uint32()
    _check(_ffi.lib().wbx_spectrum_log_freqs(float(f_min), float(bins_per_octave), n_bins, out.ctypes.data, C.byref(clamped)),
           "wbx_spectrum_log_freqs")
    return out, clamped.value


def _run_spectrum(fn, what, h, engine, ident, first_frame, n_frames, channel, basis, window_frames, n_bins, hop_frames):
    channel = SPECTRUM_MID if channel in ("mid", None) else channel
    hops = spectrum_hops(n_frames, window_frames, hop_frames)
    # the call's own argument check first, so that a refused call allocates no cells
    _check(_ffi.lib().wbx_spectrum_check(n_frames, channel, window_frames, n_bins, hop_frames, 1, hops * n_bins), "wbx_spectrum_check")
    power = np.zeros((hops, n_bins), dtype=np.float32)
    si = _ffi.SpectrumInfo()
    _check(fn(h, ident, first_frame, n_frames, channel, basis, window_frames, n_bins, hop_frames,
              power.ctypes.data if power.size else None, power.size, C.byref(si)), what, h, engine)
    return power, {k: getattr(si, k) for k, _ in _ffi.SpectrumInfo._fields_}


def loudness_hops(rate: int, n_frames: int) -> int:
    """wbx_loudness_hops (host-only): complete 100 ms hops of n_frames at `rate` (hop = (rate + 5) // 10 frames); 0 outside
    the supported rates 8000 .. 384000"""
    return int(_ffi.lib().wbx_loudness_hops(rate, n_frames))


def true_peak_launch_shape(rate: int, n_frames: int) -> dict:
    """wbx_true_peak_launch_shape (host-only): {"factor", "n_tiles", "grid"} of the true peak's launch over n_frames at `rate`"""
    v = [C.c_uint32() for _ in range(3)]
    _check(_ffi.lib().wbx_true_peak_launch_shape(rate, n_frames, *[C.byref(x) for x in v]), "wbx_true_peak_launch_shape")
    return dict(zip(("factor", "n_tiles", "grid"), (x.value for x in v)))


def loudness_coefficients(rate: int) -> np.ndarray:
    """wbx_loudness_coefficients (host-only): the K filter's [10] fp64 coefficients at `rate` — stage 1's b0 b1 b2 a1 a2, then
    stage 2's"""
    out = np.zeros(10, dtype=np.float64)
    _check(_ffi.lib().wbx_loudness_coefficients(rate, out.ctypes.data), "wbx_loudness_coefficients")
    return out


def _loudness(st, channels: int) -> dict:
    """wbx_loudness -> a dict of its fields; "true_peak" one float32 per channel"""
    out = {k: getattr(st, k) for k, _ in _ffi.Loudness._fields_ if k != "true_peak"}
    out["true_peak"] = [np.float32(st.true_peak[c]) for c in range(channels)]
    return out


def loudness_gate(hop_energy: np.ndarray, hop_frames: int) -> dict:
    """wbx_loudness_gate (host-only): the BS.1770 gate over hop energies [channels][hops] (fp64) — every field of
    wbx_loudness but the true peak"""
    E = np.ascontiguousarray(hop_energy, dtype=np.float64)
    assert E.ndim == 2
    st = _ffi.Loudness()
    _check(_ffi.lib().wbx_loudness_gate(E.shape[0], E.shape[1], hop_frames, E.ctypes.data if E.size else None, C.byref(st)),
           "wbx_loudness_gate")
    out = _loudness(st, 0)
    del out["true_peak"], out["oversampling"]
    return out


def _run_loudness(fn, what, h, engine, ident, channels, rate, first_frame, n_frames, true_peak, energies):
    st = _ffi.Loudness()
    E = np.zeros((channels, loudness_hops(rate, n_frames)), dtype=np.float64) if energies else None
    _check(fn(h, ident, first_frame, n_frames, _ffi.LOUD_TRUE_PEAK if true_peak else 0, C.byref(st),
              E.ctypes.data if energies else None, E.size if energies else 0), what, h, engine)
    out = _loudness(st, channels)
    return (out, E) if energies else out


def _clip_stats(st, channels: int) -> dict:
    """wbx_clip_stats -> {"peak", "peak_frame", "min", "max", "over", "nans", "sum", "sum_sq"}, one entry per channel"""
    f32 = ("peak", "min", "max")
    return {k: [np.float32(getattr(st, k)[c]) if k in f32 else getattr(st, k)[c] for c in range(channels)]
            for k in ("peak", "peak_frame", "min", "max", "over", "nans", "sum", "sum_sq")}


def _config(device, max_tracks, max_blocks, block, channels, sample_rate, group_size, max_segments, stream):
    return _ffi.Config(device, max_tracks, max_blocks, block, channels, sample_rate, group_size, max_segments, stream)


class MixContext:
    """Layer 1 (wbx_ctx): clips in HBM + host-sequenced segments -> master / peaks / buses."""

    def __init__(self, max_tracks: int, max_blocks: int = 1, block: int = 512, channels: int = 2,
                 sample_rate: int = 48000, group_size: int = 0, device: int = 0, max_segments: int = 0,
                 stream: Optional[int] = None, _handle=None):
        self.L = _ffi.lib()
        self.block, self.channels, self.sample_rate = block, channels, sample_rate
        self._owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            cfg = _config(device, max_tracks, max_blocks, block, channels, sample_rate, group_size, max_segments, stream)
            _check(self.L.wbx_create(C.byref(cfg), C.byref(h)), "wbx_create")
            self.h = h
        else:
            self.h = _handle
        self.last = (0, 0)
        self.n_buses = 0
        self.num_input_channels = 0

    def close(self):
        if self._owned and self.h:
            self.L.wbx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clip_upload(self, clip: int, fmt: str, rate: int, data: Sequence[np.ndarray], frames: Optional[int] = None):
        frames = len(data[0]) if frames is None else frames
        ptrs = (C.c_void_p * len(data))(*[a.ctypes.data for a in data])
        _check(self.L.wbx_clip_upload(self.h, clip, _ffi.FMT[fmt], len(data), rate, frames, ptrs), "wbx_clip_upload", self.h)

    def clip_upload_interleaved(self, clip: int, fmt: str, rate: int, frames_by_channels: np.ndarray):
        """Decoder output [frames][channels] -> planar clip storage (deinterleave_samples, dsp/sample.cpp:29-43)."""
        a = np.ascontiguousarray(frames_by_channels)
        _check(self.L.wbx_clip_upload_interleaved(self.h, clip, _ffi.FMT[fmt], a.shape[1], rate, a.shape[0], a.ctypes.data),
               "wbx_clip_upload_interleaved", self.h)

    def clip_ingest_device(self, clip: int, fmt: str, channels: int, rate: int, frames: int, device_ptr: int):
        _check(self.L.wbx_clip_ingest_device(self.h, clip, _ffi.FMT[fmt], channels, rate, frames, device_ptr),
               "wbx_clip_ingest_device", self.h)

    def clip_download(self, clip: int, channel: int, frames: int, dtype) -> np.ndarray:
        out = np.empty(frames, dtype=dtype)
        _check(self.L.wbx_clip_download(self.h, clip, channel, out.ctypes.data), "wbx_clip_download", self.h)
        return out

    def clip_export(self, clip: int, fmt: str, channels: int, first_frame: int, n_frames: int, clamp: bool = True,
                    out: Optional[np.ndarray] = None):
        """wbx_clip_export: frames [first_frame, first_frame + n_frames) of a resident F32 clip as interleaved samples of
        `fmt` ("i16", "i24" — true packed interleave, bytes —, "i24_x8", "i32", "f32").  Returns (array, stats): the array
        is typed by the format ([n_frames * channels], bytes * 3 for "i24") unless `out`, a writable buffer of
        wbx_export_bytes bytes, is given; stats = {"peak", "over", "nans"}, one entry per channel."""
        return _export(self.L.wbx_clip_export, "wbx_clip_export", self.h, False, clip, fmt, channels, first_frame, n_frames,
                       clamp, out)

    def clip_measure(self, clip: int, channels: int, first_frame: int, n_frames: int) -> dict:
        """wbx_clip_measure: peak, its first frame, signed extremes, overs, NaNs, fp64 sum and sum of squares per channel
        of frames [first_frame, first_frame + n_frames) of a resident F32 clip, measured on the device"""
        st = _ffi.ClipStats()
        _check(self.L.wbx_clip_measure(self.h, clip, first_frame, n_frames, C.byref(st)), "wbx_clip_measure", self.h)
        return _clip_stats(st, channels)

    def clip_derive(self, src_clip: int, dst_clip: int, desc, stats_channels: int = 0):
        """wbx_clip_derive: `dst_clip` becomes a new F32 clip derived from `src_clip` by `desc` (edit_desc(...)); returns
        the result's statistics when `stats_channels` (its channel count) is given, else None"""
        st = _ffi.ClipStats()
        _check(self.L.wbx_clip_derive(self.h, src_clip, dst_clip, C.byref(desc) if desc is not None else None,
                                      C.byref(st) if stats_channels else None), "wbx_clip_derive", self.h)
        return _clip_stats(st, stats_channels) if stats_channels else None

    def clip_resample(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, dst_rate: int, quality="good",
                      stats_channels: int = 0):
        """wbx_clip_resample: `dst_clip` becomes a new F32 clip holding frames [first_frame, first_frame + n_frames) of
        `src_clip` converted to `dst_rate` ("fast" / "good" / "best", or WBX_SRC_*), resample_frames(...) frames long;
        returns the result's statistics when `stats_channels` (its channel count) is given, else None"""
        st = _ffi.ClipStats()
        _check(self.L.wbx_clip_resample(self.h, src_clip, dst_clip, first_frame, n_frames, dst_rate,
                                        _ffi.SRC_QUALITY.get(quality, quality), C.byref(st) if stats_channels else None),
               "wbx_clip_resample", self.h)
        return _clip_stats(st, stats_channels) if stats_channels else None

    def clip_filter(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, coef, tail_frames: int = 0,
                    stats_channels: int = 0):
        """wbx_clip_filter: `dst_clip` becomes a new F32 clip holding frames [first_frame, first_frame + n_frames) of
        `src_clip` run through the cascade `coef` ([stages][b0 b1 b2 a1 a2], filter_design(...) rows) and `tail_frames` of
        ring-out; returns the result's statistics when `stats_channels` (its channel count) is given, else None"""
        st = _ffi.ClipStats()
        k = _cascade(coef)
        _check(self.L.wbx_clip_filter(self.h, src_clip, dst_clip, first_frame, n_frames, tail_frames, k.ctypes.data, len(k),
                                      C.byref(st) if stats_channels else None), "wbx_clip_filter", self.h)
        return _clip_stats(st, stats_channels) if stats_channels else None

    def filter_phase_ms(self) -> tuple:
        """wbx_filter_phase_ms: device milliseconds (zero-state runs, carry, runs from the carried states) of the last filter"""
        out = np.zeros(3, dtype=np.float64)
        _check(self.L.wbx_filter_phase_ms(self.h, out.ctypes.data), "wbx_filter_phase_ms", self.h)
        return tuple(float(v) for v in out)

    def clip_convolve(self, src_clip: int, ir_clip: int, dst_clip: int, first_frame: int, n_frames: int, ir_first: int,
                      ir_frames: int, out_first: int = 0, out_frames: Optional[int] = None, gain: float = 1.0,
                      stats_channels: int = 0):
        """wbx_clip_convolve: `dst_clip` becomes a new F32 clip holding frames [out_first, out_first + out_frames) of the
        convolution of `src_clip`'s range with `ir_clip`'s (the impulse response), times `gain` (linear); out_frames
        defaults to the rest of the full result, n_frames + ir_frames - 1 - out_first.  Returns the result's statistics
        when `stats_channels` (its channel count) is given, else None"""
        if out_frames is None:
            out_frames = n_frames + ir_frames - 1 - out_first
        st = _ffi.ClipStats()
        _check(self.L.wbx_clip_convolve(self.h, src_clip, ir_clip, dst_clip, first_frame, n_frames, ir_first, ir_frames, out_first,
                                        out_frames, float(gain), C.byref(st) if stats_channels else None), "wbx_clip_convolve", self.h)
        return _clip_stats(st, stats_channels) if stats_channels else None

    def convolve_ms(self) -> float:
        """wbx_convolve_ms: device milliseconds of the last convolution's launches"""
        out = C.c_double()
        _check(self.L.wbx_convolve_ms(self.h, C.byref(out)), "wbx_convolve_ms", self.h)
        return out.value

    def clip_limit(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, ceiling: float, drive: float = 1.0,
                   lookahead_frames: int = 72, hold_frames: int = 0, release_frames: int = 4800, stats_channels: int = 0):
        """wbx_clip_limit: `dst_clip` becomes a new F32 clip of n_frames frames = the range of `src_clip` times `drive`
        (linear) through the look-ahead peak limiter: no sample above `ceiling` (linear, taken as a float32), no delay.
        Returns the limiter's statistics {"peak_in", "min_gain", "min_gain_frame", "limited_frames"}, and with
        `stats_channels` (the clip's channel count) the pair (those, the result's wbx_clip_measure statistics)"""
        ls, st = _ffi.LimitStats(), _ffi.ClipStats()
        _check(self.L.wbx_clip_limit(self.h, src_clip, dst_clip, first_frame, n_frames, np.float32(ceiling), float(drive),
                                     lookahead_frames, hold_frames, release_frames, C.byref(ls),
                                     C.byref(st) if stats_channels else None), "wbx_clip_limit", self.h)
        return (_limit_stats(ls), _clip_stats(st, stats_channels)) if stats_channels else _limit_stats(ls)

    def limit_ms(self) -> float:
        """wbx_limit_ms: device milliseconds of the last limit's launches"""
        out = C.c_double()
        _check(self.L.wbx_limit_ms(self.h, C.byref(out)), "wbx_limit_ms", self.h)
        return out.value

    def clip_dynamics(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, table, sense="compress",
                      key_clip: Optional[int] = None, key_first: int = 0, drive: float = 1.0, key_gain: float = 1.0,
                      makeup: float = 1.0, lookahead_frames: int = 72, hold_frames: int = 0, release_frames: int = 4800,
                      stats_channels: int = 0):
        """wbx_clip_dynamics: `dst_clip` becomes a new F32 clip of n_frames frames = the range of `src_clip` times `drive`,
        times the gain that `table` (dynamics_table(...), or any 3073 gains over level) gives the level of the clip itself
        or of `key_clip` from `key_first` on, shaped by look-ahead, hold and release in the `sense` "compress" or "gate",
        times `makeup` (all linear); no delay.  Returns the statistics {"min_gain", "min_gain_frame", "reduced_frames"},
        and with `stats_channels` (the clip's channel count) the pair (those, the result's wbx_clip_measure statistics)"""
        t, ds, st = _dyn_table(table), _ffi.DynamicsStats(), _ffi.ClipStats()
        _check(self.L.wbx_clip_dynamics(self.h, src_clip, _ffi.DYN_NO_KEY if key_clip is None else key_clip, dst_clip, first_frame,
                                        n_frames, key_first, _ffi.DYN_SENSE.get(sense, sense), t.ctypes.data, float(drive),
                                        float(key_gain), float(makeup), lookahead_frames, hold_frames, release_frames,
                                        C.byref(ds), C.byref(st) if stats_channels else None), "wbx_clip_dynamics", self.h)
        return (_dynamics_stats(ds), _clip_stats(st, stats_channels)) if stats_channels else _dynamics_stats(ds)

    def dynamics_ms(self) -> float:
        """wbx_dynamics_ms: device milliseconds of the last dynamics call's launches"""
        out = C.c_double()
        _check(self.L.wbx_dynamics_ms(self.h, C.byref(out)), "wbx_dynamics_ms", self.h)
        return out.value

    def clip_saturate(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, table, os: int = 4, quality="good",
                      drive: float = 1.0, makeup: float = 1.0, stats_channels: int = 0):
        """wbx_clip_saturate: `dst_clip` becomes a new F32 clip of n_frames frames = the range of `src_clip` converted up by
        `os` (1, 2, 4 or 8, at "fast" / "good" / "best"), times `drive`, through `table` (saturate_table(...), or any 16385
        outputs over the level -8 .. +8), times `makeup`, band-limited back; no delay, and NO ceiling guarantee (the
        band-limiting overshoots: clip_limit gives one).  Returns the statistics {"peak_drive", "peak_index", "beyond"}, and
        with `stats_channels` (the clip's channel count) the pair (those, the result's wbx_clip_measure statistics)"""
        t, ss, st = _sat_table(table), _ffi.SaturateStats(), _ffi.ClipStats()
        _check(self.L.wbx_clip_saturate(self.h, src_clip, dst_clip, first_frame, n_frames, os, _ffi.SRC_QUALITY.get(quality, quality),
                                        t.ctypes.data, float(drive), float(makeup), C.byref(ss),
                                        C.byref(st) if stats_channels else None), "wbx_clip_saturate", self.h)
        return (_saturate_stats(ss), _clip_stats(st, stats_channels)) if stats_channels else _saturate_stats(ss)

    def saturate_ms(self) -> float:
        """wbx_saturate_ms: device milliseconds of the last saturate call's launches"""
        out = C.c_double()
        _check(self.L.wbx_saturate_ms(self.h, C.byref(out)), "wbx_saturate_ms", self.h)
        return out.value

    def clip_varispeed(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, out_frames: int, knots,
                       knot_shift: int, quality="good", guard_num: int = 1, guard_den: int = 1, stats_channels: int = 0):
        """wbx_clip_varispeed: `dst_clip` becomes a new F32 clip of out_frames frames = the range of `src_clip` read along
        the position curve `knots` (int64, 2^-32 source frames relative to first_frame, one per 2^knot_shift output frames
        and one more) through the band-limited interpolator of `quality`, protected from aliasing up to the speed
        guard_num / guard_den.  `knots` may be None (refused).  With `stats_channels` (the clip's channel count) returns
        the result's wbx_clip_measure statistics"""
        k, st = (None if knots is None else _vs_knots(knots)), _ffi.ClipStats()
        _check(self.L.wbx_clip_varispeed(self.h, src_clip, dst_clip, first_frame, n_frames, out_frames,
                                         None if k is None else k.ctypes.data, 0 if k is None else k.size, knot_shift,
                                         _vs_q(quality), guard_num, guard_den, C.byref(st) if stats_channels else None),
               "wbx_clip_varispeed", self.h)
        return _clip_stats(st, stats_channels) if stats_channels else None

    def varispeed_ms(self) -> float:
        """wbx_varispeed_ms: device milliseconds of the last varispeed call's uploads and launch"""
        out = C.c_double()
        _check(self.L.wbx_varispeed_ms(self.h, C.byref(out)), "wbx_varispeed_ms", self.h)
        return out.value

    def clip_denoise(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, window_frames: int, thr,
                     floor: float = 0.1, smooth_hops: int = 2, smooth_bins: int = 1) -> dict:
        """wbx_clip_denoise: `dst_clip` becomes a new F32 clip of n_frames frames = the range of `src_clip` through the
        spectral gate: window_frames a power of two in 64 .. 2048, `thr` the per-channel, per-bin power thresholds
        [channels][window_frames / 2 + 1] (denoise_threshold of clip_denoise_profile's sums), `floor` the linear gain of a
        closed cell, the box of 2 smooth_hops + 1 hops x 2 smooth_bins + 1 bins.  No delay.  Returns {"hops", "cells",
        "open_cells", "bands"}"""
        t, st = _denoise_thr(thr), _ffi.DenoiseStats()
        _check(self.L.wbx_clip_denoise(self.h, src_clip, first_frame, n_frames, window_frames, smooth_hops, smooth_bins,
                                       t.ctypes.data, float(floor), dst_clip, C.byref(st)), "wbx_clip_denoise", self.h)
        return _denoise_stats(st)

    def clip_denoise_profile(self, clip: int, channels: int, first_frame: int, n_frames: int, window_frames: int):
        """wbx_clip_denoise_profile: (sums float64[channels * B], hops) — per channel and bin the sum of the cells' power
        over the complete windows of the range; a measurement, nothing allocated in the pool"""
        sums, hops = np.zeros(channels * (window_frames // 2 + 1), dtype=np.float64), C.c_uint64()
        _check(self.L.wbx_clip_denoise_profile(self.h, clip, first_frame, n_frames, window_frames, sums.ctypes.data, C.byref(hops)),
               "wbx_clip_denoise_profile", self.h)
        return sums, hops.value

    def denoise_ms(self) -> float:
        """wbx_denoise_ms: device milliseconds of the last denoise or profile call's launches"""
        out = C.c_double()
        _check(self.L.wbx_denoise_ms(self.h, C.byref(out)), "wbx_denoise_ms", self.h)
        return out.value

    def clip_stretch(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, out_frames: int,
                     window_frames: int = 2048, tolerance_frames: int = 512, positions: bool = False, stats_channels: int = 0):
        """wbx_clip_stretch: `dst_clip` becomes a new F32 clip of out_frames frames = the range of `src_clip` time-stretched
        by WSOLA: another length, the same pitch.  Returns the call's info {"steps", "searched_steps", "candidates",
        "max_shift", "launches"}; with `positions` the pair (info, the int32 positions p_k); with `stats_channels` (the
        clip's channel count) the result's wbx_clip_measure statistics as the last element"""
        si, st = _ffi.StretchInfo(), _ffi.ClipStats()
        K = stretch_steps(out_frames, window_frames) if positions else 0
        pos = np.zeros(max(K, 1), dtype=np.int32)
        _check(self.L.wbx_clip_stretch(self.h, src_clip, dst_clip, first_frame, n_frames, out_frames, window_frames, tolerance_frames,
                                       pos.ctypes.data if positions else None, pos.size if positions else 0, C.byref(si),
                                       C.byref(st) if stats_channels else None), "wbx_clip_stretch", self.h)
        out = (_stretch_info(si),) + ((pos[:K],) if positions else ()) + ((_clip_stats(st, stats_channels),) if stats_channels else ())
        return out[0] if len(out) == 1 else out

    def stretch_ms(self) -> float:
        """wbx_stretch_ms: device milliseconds of the last stretch call's launches"""
        out = C.c_double()
        _check(self.L.wbx_stretch_ms(self.h, C.byref(out)), "wbx_stretch_ms", self.h)
        return out.value

    def clip_warp(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, out_frames: int, markers,
                  window_frames: int = 2048, tolerance_frames: int = 512, positions: bool = False, stats_channels: int = 0):
        """wbx_clip_warp: `dst_clip` becomes a new F32 clip of out_frames frames = the range of `src_clip` warped along
        `markers`, a sequence of (src_frame, out_frame) pairs relative to the range: each source frame sounds at its
        output frame, the stretches between them are WSOLA.  Returns the call's info {"steps", "searched_steps",
        "candidates", "max_shift", "launches", "segments", "longest_segment_steps"}; `positions` and `stats_channels` as
        in clip_stretch"""
        arr, M = _warp_markers(markers)
        wi, st = _ffi.WarpInfo(), _ffi.ClipStats()
        K = warp_steps(n_frames, out_frames, markers, window_frames) if positions else 0
        pos = np.zeros(max(K, 1), dtype=np.int32)
        _check(self.L.wbx_clip_warp(self.h, src_clip, dst_clip, first_frame, n_frames, out_frames, arr, M, window_frames,
                                    tolerance_frames, pos.ctypes.data if positions else None, pos.size if positions else 0,
                                    C.byref(wi), C.byref(st) if stats_channels else None), "wbx_clip_warp", self.h)
        out = (_warp_info(wi),) + ((pos[:K],) if positions else ()) + ((_clip_stats(st, stats_channels),) if stats_channels else ())
        return out[0] if len(out) == 1 else out

    def warp_ms(self) -> float:
        """wbx_warp_ms: device milliseconds of the last warp call's launches"""
        out = C.c_double()
        _check(self.L.wbx_warp_ms(self.h, C.byref(out)), "wbx_warp_ms", self.h)
        return out.value

    def clip_pitch(self, src_clip: int, dst_clip: int, first_frame: int, n_frames: int, out_frames: int, num: int, den: int,
                   quality="good", window_frames: int = 2048, tolerance_frames: int = 512, positions: bool = False,
                   stats_channels: int = 0):
        """wbx_clip_pitch: `dst_clip` becomes a new F32 clip of out_frames frames = the range of `src_clip` transposed by
        num / den (above 1: up) at the source's rate: a stretch to pitch_mid_frames(out_frames, num, den) frames fed
        straight into a conversion by that ratio.  Returns the call's info {"steps", "searched_steps", "candidates",
        "mid_frames", "max_shift", "launches", "L", "M"}; with `positions` the pair (info, the int32 positions p_k of the
        stretch); with `stats_channels` (the clip's channel count) the result's wbx_clip_measure statistics as the last
        element"""
        pi, st = _ffi.PitchInfo(), _ffi.ClipStats()
        K = stretch_steps(pitch_mid_frames(out_frames, num, den), window_frames) if positions else 0
        pos = np.zeros(max(K, 1), dtype=np.int32)
        _check(self.L.wbx_clip_pitch(self.h, src_clip, dst_clip, first_frame, n_frames, out_frames, num, den,
                                     _ffi.SRC_QUALITY.get(quality, quality), window_frames, tolerance_frames,
                                     pos.ctypes.data if positions else None, pos.size if positions else 0, C.byref(pi),
                                     C.byref(st) if stats_channels else None), "wbx_clip_pitch", self.h)
        out = (_pitch_info(pi),) + ((pos[:K],) if positions else ()) + ((_clip_stats(st, stats_channels),) if stats_channels else ())
        return out[0] if len(out) == 1 else out

    def pitch_ms(self) -> float:
        """wbx_pitch_ms: device milliseconds of the last pitch call's launches"""
        out = C.c_double()
        _check(self.L.wbx_pitch_ms(self.h, C.byref(out)), "wbx_pitch_ms", self.h)
        return out.value

    def clip_f0(self, clip: int, first_frame: int, n_frames: int, window_frames: int = 1024, hop_frames: int = 256,
                tau_min: int = 24, tau_max: int = 1024, threshold: float = 0.15):
        """wbx_clip_f0: the period track of frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2
        channels, by YIN on the device: (records, info) — a structured array (F0_DTYPE: "period" in frames, "dip",
        "energy", "lag", "voiced"), one record per complete hop, and {"hops", "voiced_hops", "terms", "launches"}.  The
        frequency of a hop is the clip's rate over its period"""
        return _run_f0(self.L.wbx_clip_f0, "wbx_clip_f0", self.h, False, clip, first_frame, n_frames, window_frames, hop_frames,
                       tau_min, tau_max, threshold)

    def f0_ms(self) -> float:
        """wbx_f0_ms: device milliseconds of the last f0 call's launches"""
        out = C.c_double()
        _check(self.L.wbx_f0_ms(self.h, C.byref(out)), "wbx_f0_ms", self.h)
        return out.value

    def clip_onsets(self, clip: int, first_frame: int, n_frames: int, hop_frames: int = 256, floor_power: float = 1e-9,
                    threshold: float = 0.3, delta: float = 0.1, w: int = 3, a: int = 8):
        """wbx_clip_onsets: the onset-strength curve of frames [first_frame, first_frame + n_frames) of a resident F32 clip
        of 1 or 2 channels and the onsets picked from it: (records, info) — a structured array (ONSET_DTYPE: "energy",
        "edge_energy", "novelty", "onset"), one record per complete hop, and {"hops", "onsets", "launches"}.  An onset's frame
        is its hop times hop_frames"""
        return _run_onsets(self.L.wbx_clip_onsets, "wbx_clip_onsets", self.h, False, clip, first_frame, n_frames, hop_frames,
                           floor_power, threshold, delta, w, a)

    def clip_tempo(self, clip: int, first_frame: int, n_frames: int, hop_frames: int = 256, floor_power: float = 1e-9,
                   window_hops: int = 1024, step_hops: int = 64, lag_min: int = 56, lag_max: int = 188, threshold: float = 0.5):
        """wbx_clip_tempo: the period track of the range's onset-strength curve, which never leaves the device: (records,
        info) as clip_f0's, with periods in hops — bpm = 60 * rate / (hop_frames * period).  The default lags are 200 .. 60
        bpm at 48 kHz and hop_frames = 256"""
        return _run_tempo(self.L.wbx_clip_tempo, "wbx_clip_tempo", self.h, False, clip, first_frame, n_frames, hop_frames,
                          floor_power, window_hops, step_hops, lag_min, lag_max, threshold)

    def clip_spectrum(self, clip: int, first_frame: int, n_frames: int, basis_clip: int, window_frames: int, n_bins: int,
                      hop_frames: int, channel="mid"):
        """wbx_clip_spectrum: the power of frames [first_frame, first_frame + n_frames) of a resident F32 clip of 1 or 2
        channels at the n_bins frequencies of `basis_clip` (a resident mono F32 clip of spectrum_basis's words), one row per
        complete hop, as a direct transform on the device: (power float32[hops][n_bins], {"hops", "bins", "launches"}).
        channel 0, 1 or "mid" (SPECTRUM_MID).  Nothing is allocated in the pool."""
        return _run_spectrum(self.L.wbx_clip_spectrum, "wbx_clip_spectrum", self.h, False, clip, first_frame, n_frames, channel,
                             basis_clip, window_frames, n_bins, hop_frames)

    def clip_align(self, ref_clip: int, a_first: int, n_frames: int, clip: int, b_first: int, m_frames: int, lag_min: int,
                   lag_max: int, either_polarity=False, curve: bool = False):
        """wbx_clip_align: by how many frames `clip`'s range [b_first, b_first + m_frames) lags the template
        [a_first, a_first + n_frames) of `ref_clip` (n_frames a multiple of 8 in 64 .. 2^24), over the signed lags
        lag_min .. lag_max, by a chunked cross-correlation on the device: (info, curve) — {"lag", "inverted", "offset",
        "score", "r", "energy", "ref_energy", "confidence", "lags", "chunks", "terms", "launches"} and, with curve=True, a
        structured array (ALIGN_CURVE_DTYPE: "r", "energy") per lag, else None.  either_polarity: score r * r / E, so that
        an inverted copy is found (info["inverted"]).  Nothing is allocated in the pool."""
        return _run_align(self.L.wbx_clip_align, "wbx_clip_align", self.h, False, ref_clip, a_first, n_frames, clip, b_first,
                          m_frames, lag_min, lag_max, either_polarity, curve)

    def align_ms(self) -> float:
        """wbx_align_ms: device milliseconds of the last align call's launches"""
        out = C.c_double()
        _check(self.L.wbx_align_ms(self.h, C.byref(out)), "wbx_align_ms", self.h)
        return out.value

    def spectrum_ms(self) -> float:
        """wbx_spectrum_ms: device milliseconds of the last spectrum call's launches"""
        out = C.c_double()
        _check(self.L.wbx_spectrum_ms(self.h, C.byref(out)), "wbx_spectrum_ms", self.h)
        return out.value

    def onsets_ms(self) -> float:
        """wbx_onset_ms: device milliseconds of the energy pass of the last onsets or tempo call"""
        out = C.c_double()
        _check(self.L.wbx_onset_ms(self.h, C.byref(out)), "wbx_onset_ms", self.h)
        return out.value

    def clip_loudness(self, clip: int, channels: int, rate: int, first_frame: int, n_frames: int, true_peak=False,
                      energies: bool = False):
        """wbx_clip_loudness: ITU-R BS.1770-4 / EBU R 128 figures of frames [first_frame, first_frame + n_frames) of a
        resident F32 clip uploaded at `rate`, measured on the device: {"integrated", "gated_power", "momentary_max",
        "short_term_max", "range_lu", "true_peak", "hops", "blocks", "blocks_gated", "hop_frames", "oversampling"}; the true
        peak only with `true_peak`.  With `energies` returns (dict, the hop energies [channels][hops] as the device wrote them)"""
        return _run_loudness(self.L.wbx_clip_loudness, "wbx_clip_loudness", self.h, False, clip, channels, rate, first_frame,
                             n_frames, true_peak, energies)

    def clip_splice(self, dst_clip: int, channels: int, n_frames: int, parts, stats: bool = False):
        """wbx_clip_splice: `dst_clip` becomes a new F32 clip of `channels` x `n_frames` frames, the parts
        (splice_part(...)) assigned and added in list order; returns the result's statistics with `stats`, else None"""
        st = _ffi.ClipStats()
        _check(self.L.wbx_clip_splice(self.h, dst_clip, channels, n_frames, _part_array(parts), len(parts),
                                      C.byref(st) if stats else None), "wbx_clip_splice", self.h)
        return _clip_stats(st, channels) if stats else None

    def set_export_chunk(self, frames: int):
        """frames per staging chunk of later exports (a multiple of 8; 0: the default) — tests reach chunk seams with it"""
        _check(self.L.wbx_set_export_chunk(self.h, frames), "wbx_set_export_chunk", self.h)

    def build_mipmaps(self, clip: int, quality: int):
        """WaveformVisual::create (gfx/waveform_visual.cpp:181-246): quality 0 = Low (int8), 1 = High (int16)."""
        _check(self.L.wbx_clip_build_mipmaps(self.h, clip, quality), "wbx_clip_build_mipmaps", self.h)

    def fetch_mipmap(self, clip: int, level: int, channels: int, frames: int, quality: int) -> np.ndarray:
        n = self.L.wbx_mip_data_count(frames, level)
        out = np.empty((channels, n), dtype=np.int16 if quality else np.int8)
        _check(self.L.wbx_clip_fetch_mipmap(self.h, clip, level, out.ctypes.data), "wbx_clip_fetch_mipmap", self.h)
        return out

    def clip_synth(self, clip: int, fmt: str, channels: int, rate: int, frames: int, seed: int, key_track: int, amp: float):
        _check(self.L.wbx_clip_synth(self.h, clip, _ffi.FMT[fmt], channels, rate, frames, seed, key_track,
                                     np.float32(amp)), "wbx_clip_synth", self.h)

    def pool_stats(self):
        """(slabs, bytes reserved from the driver, bytes held by live clips) of the clip pool"""
        n, r, l = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(self.L.wbx_clip_pool_stats(self.h, C.byref(n), C.byref(r), C.byref(l)), "wbx_clip_pool_stats", self.h)
        return n.value, r.value, l.value

    def pool_limit(self, max_bytes_reserved: int):
        """bound what the clip pool reserves from the driver (0: no bound); a clip past it fails with WBX_ERR_OOM"""
        _check(self.L.wbx_clip_pool_limit(self.h, max_bytes_reserved), "wbx_clip_pool_limit", self.h)

    def set_routing(self, track_bus: Optional[Sequence[int]], n_buses: int, n_tracks: int):
        if track_bus is None or not n_buses:
            _check(self.L.wbx_set_routing(self.h, n_tracks, None, 0), "wbx_set_routing", self.h)
            self.n_buses = 0
        else:
            arr = (C.c_int32 * n_tracks)(*track_bus)
            _check(self.L.wbx_set_routing(self.h, n_tracks, arr, n_buses), "wbx_set_routing", self.h)
            self.n_buses = n_buses

    def set_clamp(self, on: bool):
        _check(self.L.wbx_set_clamp(self.h, int(on)), "wbx_set_clamp", self.h)

    def submit(self, n_blocks: int, n_tracks: int, segs: Sequence[tuple], seg_offsets: np.ndarray, gains: np.ndarray):
        """segs: (sample_offset, playback_speed, clip, buffer_offset, num_samples, gain)"""
        arr = (_ffi.Segment * max(1, len(segs)))()
        for i, s in enumerate(segs):
            arr[i] = _ffi.Segment(*s)
        so = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        g = np.ascontiguousarray(gains, dtype=np.float32)
        assert so.size == n_blocks * n_tracks + 1 and g.size == n_blocks * n_tracks * 2
        _check(self.L.wbx_submit(self.h, n_blocks, n_tracks, arr, so.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 g.ctypes.data_as(C.POINTER(C.c_float))), "wbx_submit", self.h)
        self.last = (n_blocks, n_tracks)

    def fetch(self, peaks: bool = False, buses: bool = False):
        K, N = self.last
        Cn, F = self.channels, self.block
        master = [np.zeros(K * F, dtype=np.float32) for _ in range(Cn)]
        mp = (C.POINTER(C.c_float) * Cn)(*[m.ctypes.data_as(C.POINTER(C.c_float)) for m in master])
        pk = np.zeros((K, N, Cn), dtype=np.float32) if peaks else None
        bs = np.zeros((K, self.n_buses, Cn, F), dtype=np.float32) if (buses and self.n_buses) else None
        _check(self.L.wbx_fetch(self.h, mp, pk.ctypes.data_as(C.POINTER(C.c_float)) if pk is not None else None,
                                bs.ctypes.data_as(C.POINTER(C.c_float)) if bs is not None else None), "wbx_fetch", self.h)
        m = np.stack(master).reshape(Cn, K, F).transpose(1, 0, 2)     # [K][C][F]
        return m, pk, bs

    def fetch_interleaved(self, fmt: str) -> np.ndarray:
        K, _ = self.last
        dt = {"i16": np.int16, "i24": np.uint8, "i24_x8": np.int32, "i32": np.int32, "f32": np.float32}[fmt]
        out = np.zeros(K * self.block * self.channels * (3 if fmt == "i24" else 1), dtype=dt)
        _check(self.L.wbx_fetch_interleaved(self.h, _ffi.OUT_FMT[fmt], out.ctypes.data), "wbx_fetch_interleaved", self.h)
        return out

    def set_master_format(self, fmt: Optional[str]):
        """Later renders leave their master as interleaved samples of `fmt` ("i16", "i24", "i24_x8", "i32", "f32"; None:
        planar fp32 again) — the conversion runs as the sum kernel's epilogue."""
        _check(self.L.wbx_set_master_format(self.h, _ffi.OUT_FMT[fmt] if fmt else 0), "wbx_set_master_format", self.h)

    def sync(self):
        _check(self.L.wbx_sync(self.h), "wbx_sync", self.h)

    def render_status(self):
        """wait, then raise if a chained render since the last report lost a hand-over (its master is invalid): what a host
        that reads its own master target instead of fetching must call before it trusts the buffer"""
        _check(self.L.wbx_render_status(self.h), "wbx_render_status", self.h)

    def master_ready(self, stream: Optional[int] = None):
        """Order `stream` (None: the ctx stream) after the kernels that write the last render's results."""
        _check(self.L.wbx_master_ready(self.h, stream), "wbx_master_ready", self.h)

    def set_master_target(self, device_ptr: Optional[int]):
        _check(self.L.wbx_set_master_target(self.h, device_ptr), "wbx_set_master_target", self.h)

    def set_master_init(self, device_ptr: Optional[int]):
        """Later renders continue the running (un-clamped) sum in `device_ptr` instead of starting from zero."""
        _check(self.L.wbx_set_master_init(self.h, device_ptr), "wbx_set_master_init", self.h)

    def render_order(self, n_blocks: int):
        """(groups per block, longest group, is it the reference's order) for a render of n_blocks blocks"""
        ng, lg, ref = C.c_uint32(), C.c_uint32(), C.c_int()
        _check(self.L.wbx_render_order(self.h, n_blocks, C.byref(ng), C.byref(lg), C.byref(ref)), "wbx_render_order", self.h)
        return ng.value, lg.value, bool(ref.value)

    def device_info(self):
        pci, name = C.create_string_buffer(32), C.create_string_buffer(128)
        _check(self.L.wbx_device_info(self.h, pci, 32, name, 128), "wbx_device_info", self.h)
        return {"pci": pci.value.decode(), "name": name.value.decode()}

    def partial_master(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.L.wbx_partial_master(self.h, C.byref(p), C.byref(n)), "wbx_partial_master", self.h)
        return p.value, n.value

    def finalize_master(self, device_ptr: int, n_blocks: int, clamp: bool = True, stream: Optional[int] = None):
        _check(self.L.wbx_finalize_master(self.h, device_ptr, n_blocks, int(clamp), stream), "wbx_finalize_master", self.h)

    def finalize_master_into(self, device_ptr: int, dst_ptr: int, n_blocks: int, clamp: bool = True, stream: Optional[int] = None):
        """Clamp the reduced master out of place; `dst_ptr` may be pinned host memory."""
        _check(self.L.wbx_finalize_master_into(self.h, device_ptr, dst_ptr, n_blocks, int(clamp), stream),
               "wbx_finalize_master_into", self.h)

    def kernel_time(self, reset: bool = False):
        ms, n = C.c_double(), C.c_uint64()
        _check(self.L.wbx_kernel_time(self.h, int(reset), C.byref(ms), C.byref(n)), "wbx_kernel_time", self.h)
        return ms.value, n.value


    def kernel_name(self) -> str:
        """The mix_kernel instance the last render launched, as rocprofv3 prints it."""
        return (self.L.wbx_kernel_name(self.h) or b"").decode()

    def xcd_count(self) -> int:
        """XCDs the workgroup ids of a launch are dealt to round-robin (wbx_create's probe); 0: no such layout"""
        return int(self.L.wbx_xcd_count(self.h))

    def uniform_speed(self) -> float:
        """MixArgs::uniform_speed of the last render (0.0: no single resampling ratio)."""
        return float(self.L.wbx_render_uniform_speed(self.h))

    def tail_time(self) -> float:
        ms = C.c_double()
        _check(self.L.wbx_tail_time(self.h, C.byref(ms)), "wbx_tail_time", self.h)
        return ms.value

    def gap_time(self):
        """(mean idle time in ms between two consecutive mix launches since the last kernel_time(reset=True), pairs timed)"""
        ms, n = C.c_double(), C.c_uint64()
        _check(self.L.wbx_gap_time(self.h, C.byref(ms), C.byref(n)), "wbx_gap_time", self.h)
        return ms.value, int(n.value)


class Track:
    """wb::Track surface used by the mix path (track.h:137-139)."""

    def __init__(self, engine: "Engine", index: int, name: str):
        self.engine, self.index, self.name = engine, index, name

    def set_volume(self, db: float):
        _check(self.engine.L.wbx_track_set_volume(self.engine.h, self.index, np.float32(db)), "Track::set_volume", self.engine.h, True)

    def set_pan(self, pan: float):
        _check(self.engine.L.wbx_track_set_pan(self.engine.h, self.index, np.float32(pan)), "Track::set_pan", self.engine.h, True)

    def set_mute(self, mute: bool):
        _check(self.engine.L.wbx_track_set_mute(self.engine.h, self.index, int(mute)), "Track::set_mute", self.engine.h, True)

    def set_bus(self, bus: int):
        _check(self.engine.L.wbx_track_set_bus(self.engine.h, self.index, bus), "Track::set_bus", self.engine.h, True)

    @property
    def plugin_instance(self):
        """Track::plugin_instance (track.h:124): the effect slot — always empty (None) in this path."""
        p = C.c_void_p()
        _check(self.engine.L.wbx_track_get_plugin(self.engine.h, self.index, C.byref(p)), "wbx_track_get_plugin",
               self.engine.h, True)
        return p.value


class Engine:
    """wb::Engine surface (engine.h:29-273) for the mix path."""

    def __init__(self, max_tracks: int, buffer_size: int = 512, sample_rate: int = 48000, output_channels: int = 2,
                 max_blocks: int = 1, group_size: int = 0, device: int = 0, max_segments: int = 0,
                 stream: Optional[int] = None):
        self.L = _ffi.lib()
        h = C.c_void_p()
        cfg = _config(device, max_tracks, max_blocks, buffer_size, output_channels, sample_rate, group_size,
                      max_segments, stream)
        _check(self.L.wbx_engine_create(C.byref(cfg), C.byref(h)), "wbx_engine_create")
        self.h = h
        self.audio_buffer_size, self.audio_sample_rate, self.num_output_channels = buffer_size, sample_rate, output_channels
        self.tracks: List[Track] = []
        self.ctx = MixContext(max_tracks, max_blocks, buffer_size, output_channels, sample_rate,
                              _handle=C.c_void_p(self.L.wbx_engine_ctx(h)))
        self.n_buses = 0
        self.max_blocks = max_blocks
        self._sample_shape = {}   # sample id -> (frames, channels) of the samples made through this object (export_sample)
        self._sample_rate = {}    # sample id -> the sample's own rate where this object knows it (wav.write_sample)

    def close(self):
        if self.h:
            self.L.wbx_engine_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference-shaped surface ----
    def set_audio_channel_config(self, input_channels: int, output_channels: int, buffer_size: int, sample_rate: int):
        """Engine::set_audio_channel_config (engine.cpp:43-57) on the live engine: tracks and clips stay."""
        _check(self.L.wbx_engine_set_audio_channel_config(self.h, output_channels, buffer_size, sample_rate),
               "Engine::set_audio_channel_config", self.h, True)
        _check(self.L.wbx_engine_set_input_channels(self.h, input_channels), "Engine::set_audio_channel_config", self.h, True)
        self.num_input_channels = input_channels
        self.audio_buffer_size, self.audio_sample_rate, self.num_output_channels = buffer_size, sample_rate, output_channels
        self.ctx.block, self.ctx.channels, self.ctx.sample_rate = buffer_size, output_channels, sample_rate

    def set_bpm(self, bpm: float):
        _check(self.L.wbx_engine_set_bpm(self.h, bpm), "Engine::set_bpm", self.h, True)

    def set_playhead_position(self, beat: float):
        _check(self.L.wbx_engine_set_playhead_position(self.h, beat), "Engine::set_playhead_position", self.h, True)

    def add_track(self, name: str = "") -> Track:
        idx = C.c_uint32()
        _check(self.L.wbx_engine_add_track(self.h, C.byref(idx)), "Engine::add_track", self.h, True)
        t = Track(self, idx.value, name)
        self.tracks.append(t)
        return t

    def set_buses(self, n: int):
        _check(self.L.wbx_engine_set_buses(self.h, n), "wbx_engine_set_buses", self.h, True)
        self.n_buses = n
        self.ctx.n_buses = n

    # ---- track management (engine.cpp:210-262): the Track objects keep their identity, their slots shift ----
    def _reindex(self):
        for i, t in enumerate(self.tracks):
            t.index = i

    def delete_track(self, slot: int):
        _check(self.L.wbx_engine_delete_track(self.h, slot), "Engine::delete_track", self.h, True)
        del self.tracks[slot]
        self._reindex()

    def clear_all(self):
        _check(self.L.wbx_engine_clear_all(self.h), "Engine::clear_all", self.h, True)
        self.tracks = []

    def move_track(self, from_slot: int, to_slot: int):
        _check(self.L.wbx_engine_move_track(self.h, from_slot, to_slot), "Engine::move_track", self.h, True)
        t = self.tracks.pop(from_slot)
        self.tracks.insert(to_slot, t)
        self._reindex()

    def solo_track(self, slot: int):
        _check(self.L.wbx_engine_solo_track(self.h, slot), "Engine::solo_track", self.h, True)

    def add_plugin_to_track(self, track: Track, plugin=None):
        """Engine::add_plugin_to_track (engine.h:227): the slot is kept, processing through it is Unimplemented."""
        _check(self.L.wbx_engine_add_plugin_to_track(self.h, track.index, C.byref(plugin) if plugin is not None else None),
               "Engine::add_plugin_to_track", self.h, True)

    def delete_plugin_from_track(self, track: Track):
        _check(self.L.wbx_engine_delete_plugin_from_track(self.h, track.index), "Engine::delete_plugin_from_track", self.h, True)

    def sequencer_stats(self):
        """(renders planned by segments, tracks with a seam that did not hold, segments planned again, segments per track)"""
        out = (C.c_uint64 * 4)()
        _check(self.L.wbx_engine_sequencer_stats(self.h, out), "wbx_engine_sequencer_stats", self.h, True)
        return tuple(int(x) for x in out)

    def callback_stats(self):
        """(blocks run as one launch, ... with the sum spread over the workgroups, blocks mixed again after a give-up at the
        spread barrier, 1 when the engine has stopped spreading)"""
        out = (C.c_uint64 * 4)()
        _check(self.L.wbx_engine_callback_stats(self.h, out), "wbx_engine_callback_stats", self.h, True)
        return tuple(int(x) for x in out)

    def perf_usage(self):
        """(Engine::perf_measurer.get_usage() — the callback's share of its period, exponential average, clamped to [0, 1] —,
        the wall time in ms of the last process call)"""
        u, d = C.c_double(), C.c_double()
        _check(self.L.wbx_engine_perf_usage(self.h, C.byref(u), C.byref(d)), "wbx_engine_perf_usage", self.h, True)
        return u.value, d.value

    def thread_stats(self):
        """(locked edits the last process / render had seen, per-track cumulative drained parameter messages)"""
        n = len(self.tracks)
        seen = C.c_uint64()
        dr = (C.c_uint64 * max(1, n))()
        _check(self.L.wbx_engine_thread_stats(self.h, C.byref(seen), dr, n), "wbx_engine_thread_stats", self.h, True)
        return seen.value, list(dr[:n])

    def add_sample(self, fmt: str, rate: int, data: Sequence[np.ndarray], frames: Optional[int] = None) -> int:
        """Sample asset -> HBM.  `data` planar channel arrays (padding is added by the library)."""
        frames = len(data[0]) if frames is None else frames
        ptrs = (C.c_void_p * len(data))(*[a.ctypes.data for a in data])
        sid = C.c_uint32()
        _check(self.L.wbx_engine_add_sample(self.h, _ffi.FMT[fmt], len(data), rate, frames, ptrs, C.byref(sid)),
               "wbx_engine_add_sample", self.h, True)
        self._sample_shape[sid.value] = (frames, len(data))
        self._sample_rate[sid.value] = rate
        return sid.value

    def add_sample_interleaved(self, fmt: str, rate: int, frames_by_channels: np.ndarray) -> int:
        """The same from a decoder's interleaved [frames][channels] buffer (Sample::load_file, dsp/sample.cpp:112-197)."""
        a = np.ascontiguousarray(frames_by_channels)
        sid = C.c_uint32()
        _check(self.L.wbx_engine_add_sample_interleaved(self.h, _ffi.FMT[fmt], a.shape[1], rate, a.shape[0], a.ctypes.data,
                                                        C.byref(sid)), "wbx_engine_add_sample_interleaved", self.h, True)
        self._sample_shape[sid.value] = (a.shape[0], a.shape[1])
        self._sample_rate[sid.value] = rate
        return sid.value

    def add_sample_synth(self, fmt: str, channels: int, rate: int, frames: int, seed: int, key_track: int, amp: float) -> int:
        sid = C.c_uint32()
        _check(self.L.wbx_engine_add_sample_synth(self.h, _ffi.FMT[fmt], channels, rate, frames, seed, key_track,
                                                  np.float32(amp), C.byref(sid)), "wbx_engine_add_sample_synth", self.h, True)
        self._sample_shape[sid.value] = (frames, channels)
        self._sample_rate[sid.value] = rate
        return sid.value

    def delete_sample(self, sample: int):
        _check(self.L.wbx_engine_delete_sample(self.h, sample), "wbx_engine_delete_sample", self.h, True)
        self._sample_shape.pop(sample, None)
        self._sample_rate.pop(sample, None)

    def add_audio_clip(self, track: Track, name: str, min_time: float, max_time: float, start_offset: float,
                       sample: int, speed: float = 1.0, gain: float = 1.0):
        _check(self.L.wbx_engine_add_audio_clip(self.h, track.index, min_time, max_time, start_offset, sample, speed,
                                                np.float32(gain)), "Engine::add_audio_clip", self.h, True)

    # ---- clip edits (engine.cpp:346-407,463-475,1460-1464); `clip` = index in the track's sorted clip list ----
    def move_clip(self, track: Track, clip: int, relative_pos: float):
        _check(self.L.wbx_engine_move_clip(self.h, track.index, clip, relative_pos), "Engine::move_clip", self.h, True)

    def resize_clip(self, track: Track, clip: int, relative_pos: float, resize_limit: float, min_length: float,
                    left_side: bool, shift: bool = False, stretch: bool = False):
        _check(self.L.wbx_engine_resize_clip(self.h, track.index, clip, relative_pos, resize_limit, min_length,
                                             int(left_side), int(shift), int(stretch)), "Engine::resize_clip", self.h, True)

    def delete_clip(self, track: Track, clip: int):
        _check(self.L.wbx_engine_delete_clip(self.h, track.index, clip), "Engine::delete_clip", self.h, True)

    def delete_region(self, track: Track, min_time: float, max_time: float):
        _check(self.L.wbx_engine_delete_region(self.h, track.index, min_time, max_time), "Engine::delete_region", self.h, True)

    def set_clip_gain(self, track: Track, clip: int, gain: float):
        _check(self.L.wbx_engine_set_clip_gain(self.h, track.index, clip, np.float32(gain)), "Engine::set_clip_gain", self.h, True)

    def clips(self, track: Track):
        """(min_time, max_time, start_offset, speed, gain, sample) of the track's sorted clip list"""
        n = C.c_uint32()
        _check(self.L.wbx_engine_clip_count(self.h, track.index, C.byref(n)), "wbx_engine_clip_count", self.h, True)
        out = []
        for i in range(n.value):
            ci = _ffi.ClipInfo()
            _check(self.L.wbx_engine_get_clip(self.h, track.index, i, C.byref(ci)), "wbx_engine_get_clip", self.h, True)
            out.append((ci.min_time, ci.max_time, ci.start_offset, ci.speed, ci.gain, ci.sample))
        return out

    def play(self):
        _check(self.L.wbx_engine_play(self.h), "Engine::play", self.h, True)

    def stop(self):
        _check(self.L.wbx_engine_stop(self.h), "Engine::stop", self.h, True)

    def process(self, input_buffer: Optional[AudioBuffer], output_buffer: AudioBuffer, sample_rate: float):
        """Engine::process(const AudioBuffer<float>&, AudioBuffer<float>&, double) — one block.  The input buffer (when
        given) is what a running take records (engine.cpp:1638-1649); without one a take records silence."""
        assert output_buffer.n_samples == self.audio_buffer_size and output_buffer.n_channels == self.num_output_channels
        assert float(sample_rate) == float(self.audio_sample_rate)
        if input_buffer is not None and input_buffer.n_channels > 0:
            assert input_buffer.n_samples >= self.audio_buffer_size
            st = self.L.wbx_engine_process_in(self.h, input_buffer._ptrs(), input_buffer.n_channels, output_buffer._ptrs())
        else:
            st = self.L.wbx_engine_process(self.h, output_buffer._ptrs())
        if st != 0:
            _check(st, "Engine::process", self.h, True)
        self.ctx.last = (1, len(self.tracks))

    def process_interleaved(self, fmt: str) -> np.ndarray:
        """Engine::process + the back end's interleave_samples_to(format) in one call: the block as F*C interleaved samples."""
        dt = {"i16": np.int16, "i24": np.uint8, "i24_x8": np.int32, "i32": np.int32, "f32": np.float32}[fmt]
        out = np.zeros(self.audio_buffer_size * self.num_output_channels * (3 if fmt == "i24" else 1), dtype=dt)
        _check(self.L.wbx_engine_process_interleaved(self.h, _ffi.OUT_FMT[fmt], out.ctypes.data), "Engine::process_interleaved",
               self.h, True)
        self.ctx.last = (1, len(self.tracks))
        return out

    def process_interleaved_in(self, input_buffer: AudioBuffer, fmt: str, n_in: Optional[int] = None) -> np.ndarray:
        """process_interleaved with the input buffer of Engine::process: what an audio back end calls while a take runs.
        `n_in`: how many of the buffer's channels to hand over (all of them by default)."""
        assert input_buffer.n_samples >= self.audio_buffer_size
        dt = {"i16": np.int16, "i24": np.uint8, "i24_x8": np.int32, "i32": np.int32, "f32": np.float32}[fmt]
        out = np.zeros(self.audio_buffer_size * self.num_output_channels * (3 if fmt == "i24" else 1), dtype=dt)
        n_in = input_buffer.n_channels if n_in is None else n_in
        _check(self.L.wbx_engine_process_interleaved_in(self.h, input_buffer._ptrs(), n_in, _ffi.OUT_FMT[fmt], out.ctypes.data),
               "Engine::process_interleaved_in", self.h, True)
        self.ctx.last = (1, len(self.tracks))
        return out

    # ---- recording (engine.cpp:95-200) ----
    def set_track_input(self, slot: int, type: str, index: int, armed: bool):
        """Engine::set_track_input; type: "none", "external_stereo", "external_mono" ("midi" is refused)."""
        _check(self.L.wbx_track_set_input(self.h, slot, _ffi.INPUT_TYPE[type], index, int(armed)), "Engine::set_track_input",
               self.h, True)

    def arm_track_recording(self, slot: int, armed: bool):
        _check(self.L.wbx_engine_arm_track_recording(self.h, slot, int(armed)), "Engine::arm_track_recording", self.h, True)

    def record(self):
        _check(self.L.wbx_engine_record(self.h), "Engine::record", self.h, True)

    def stop_record(self):
        """Engine::stop_record; raises WbxError (status -8) when a take overflowed — its clip is made all the same."""
        _check(self.L.wbx_engine_stop_record(self.h), "Engine::stop_record", self.h, True)

    def is_recording(self) -> bool:
        r = C.c_int()
        _check(self.L.wbx_engine_is_recording(self.h, C.byref(r)), "wbx_engine_is_recording", self.h, True)
        return bool(r.value)

    def record_info(self, slot: int) -> dict:
        ri = _ffi.RecordInfo()
        _check(self.L.wbx_engine_record_info(self.h, slot, C.byref(ri)), "wbx_engine_record_info", self.h, True)
        return {"recording": bool(ri.recording), "armed": bool(ri.armed), "input_type": ri.input_type,
                "input_index": ri.input_index, "min_time": ri.min_time, "max_time": ri.max_time, "frames": ri.frames,
                "status": ri.status}

    def set_record_chunk(self, frames: int, spare_chunks: int):
        _check(self.L.wbx_engine_set_record_chunk(self.h, frames, spare_chunks), "wbx_engine_set_record_chunk", self.h, True)

    def render(self, n_blocks: int):
        """K consecutive blocks in one device pass; fetch with self.ctx.fetch()."""
        _check(self.L.wbx_engine_render(self.h, n_blocks), "wbx_engine_render", self.h, True)
        self.ctx.last = (n_blocks, len(self.tracks))

    def bounce(self, min_time: float, max_time: float, sources: Sequence) -> tuple:
        """wbx_engine_bounce: render [min_time, max_time) offline and keep signals of it as samples in the clip pool.
        sources: ("track", index[, "post" | "pre"]), ("bus", index), ("master",) — or the raw (kind, index, tap) integers;
        order and duplicates are kept.  Returns (sample ids, frames of each); the ids go into add_audio_clip,
        bounce_download, ctx.build_mipmaps, delete_sample."""
        arr = (_ffi.BounceSource * max(1, len(sources)))()
        for i, s in enumerate(sources):
            s = tuple(s)
            kind = _ffi.BOUNCE_KIND.get(s[0], s[0])
            index = s[1] if len(s) > 1 else 0
            tap = s[2] if len(s) > 2 else 0
            arr[i] = _ffi.BounceSource(kind, index, _ffi.BOUNCE_TAP.get(tap, tap), 0)
        ids = (C.c_uint32 * max(1, len(sources)))()
        frames = C.c_uint64()
        _check(self.L.wbx_engine_bounce(self.h, min_time, max_time, arr, len(sources), ids, C.byref(frames)),
               "wbx_engine_bounce", self.h, True)
        K = -(-frames.value // self.audio_buffer_size)
        self.ctx.last = (K % self.max_blocks or self.max_blocks, len(self.tracks))   # the last pass is what a fetch sees
        for i in ids[:len(sources)]:
            self._sample_shape[i] = (frames.value, self.num_output_channels)
            self._sample_rate[i] = self.audio_sample_rate
        return list(ids[:len(sources)]), frames.value

    def export_sample(self, sample: int, out_format: str, first_frame: int = 0, n_frames: Optional[int] = None,
                      clamp: bool = True, channels: Optional[int] = None, frames: Optional[int] = None,
                      out: Optional[np.ndarray] = None):
        """wbx_engine_export_sample: a sample (a take's, a bounce's, any F32 sample) as interleaved samples of `out_format`
        — see MixContext.clip_export.  `n_frames` None: to the sample's end.  Length and channel count of samples made by
        add_sample* / bounce are known here; for a take's sample (made inside stop_record) pass `frames`
        (record_info()["frames"]) and `channels` (1 for a mono input).  May be called while another thread runs process();
        delete_sample of the sample is refused meanwhile."""
        known = self._sample_shape.get(sample, (None, self.num_output_channels))
        frames = known[0] if frames is None else frames
        channels = known[1] if channels is None else channels
        if n_frames is None:
            assert frames is not None, "export_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        return _export(self.L.wbx_engine_export_sample, "wbx_engine_export_sample", self.h, True, sample, out_format, channels,
                       first_frame, n_frames, clamp, out)

    def _shape_of(self, sample, frames, channels):
        known = self._sample_shape.get(sample, (None, self.num_output_channels))
        return (known[0] if frames is None else frames), (known[1] if channels is None else channels)

    def measure_sample(self, sample: int, first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                       frames: Optional[int] = None) -> dict:
        """wbx_engine_measure_sample — see MixContext.clip_measure; `frames` / `channels` as in export_sample.  May be
        called while another thread runs process()."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "measure_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        st = _ffi.ClipStats()
        _check(self.L.wbx_engine_measure_sample(self.h, sample, first_frame, n_frames, C.byref(st)), "wbx_engine_measure_sample",
               self.h, True)
        return _clip_stats(st, channels)

    def derive_sample(self, sample: int, desc, channels: Optional[int] = None) -> int:
        """wbx_engine_derive_sample: a new sample derived from `sample` by `desc` (edit_desc(...)): trim, reverse, channel
        mode, gain, fades — its id goes into add_audio_clip, export_sample, ctx.build_mipmaps, delete_sample.  `channels`:
        the SOURCE's channel count when this object did not make it.  May be called while another thread runs process()."""
        _, channels = self._shape_of(sample, None, channels)
        new = C.c_uint32()
        _check(self.L.wbx_engine_derive_sample(self.h, sample, C.byref(desc) if desc is not None else None, C.byref(new)),
               "wbx_engine_derive_sample", self.h, True)
        mode = {v: k for k, v in _ffi.CH_MODE.items()}.get(desc.channel_mode, "keep")
        self._sample_shape[new.value] = (desc.n_frames, _ffi.CH_MODE_OUT.get(mode, channels))
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value

    def normalize_sample(self, sample: int, target_peak: float, first_frame: int = 0, n_frames: Optional[int] = None,
                         channels: Optional[int] = None, frames: Optional[int] = None) -> tuple:
        """wbx_engine_normalize_sample: a new sample = the range times target_peak / (its peak), one fp32 division; returns
        (new sample id, the gain used).  A silent range or a peak that is not finite raises WbxError (status -4)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "normalize_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        new, gain = C.c_uint32(), C.c_float()
        _check(self.L.wbx_engine_normalize_sample(self.h, sample, first_frame, n_frames, target_peak, C.byref(new), C.byref(gain)),
               "wbx_engine_normalize_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, float(gain.value)

    def loudness_sample(self, sample: int, first_frame: int = 0, n_frames: Optional[int] = None, true_peak=False,
                        energies: bool = False, channels: Optional[int] = None, frames: Optional[int] = None,
                        rate: Optional[int] = None):
        """wbx_engine_loudness_sample — see MixContext.clip_loudness; `frames` / `channels` as in export_sample, `rate` the
        sample's rate where this object did not make it (needed with `energies` only).  May be called while another thread
        runs process(); delete_sample of the sample is refused meanwhile."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "loudness_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        return _run_loudness(self.L.wbx_engine_loudness_sample, "wbx_engine_loudness_sample", self.h, True, sample, channels,
                             rate, first_frame, n_frames, true_peak, energies)

    def normalize_loudness_sample(self, sample: int, target_lufs: float, true_peak_ceiling: float = 0.0, first_frame: int = 0,
                                  n_frames: Optional[int] = None, channels: Optional[int] = None,
                                  frames: Optional[int] = None) -> tuple:
        """wbx_engine_normalize_loudness_sample: a new sample = the range brought to `target_lufs` integrated loudness, the
        gain capped so that its true peak stays at or below `true_peak_ceiling` (linear; 0: no ceiling); returns (new sample
        id, the gain used).  A range without an integrated loudness (silent, shorter than 400 ms) raises WbxError (-4)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "normalize_loudness_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        new, gain = C.c_uint32(), C.c_float()
        _check(self.L.wbx_engine_normalize_loudness_sample(self.h, sample, first_frame, n_frames, target_lufs, true_peak_ceiling,
                                                           C.byref(new), C.byref(gain)),
               "wbx_engine_normalize_loudness_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, float(gain.value)

    def resample_sample(self, sample: int, dst_rate: int, quality="good", first_frame: int = 0, n_frames: Optional[int] = None,
                        channels: Optional[int] = None, frames: Optional[int] = None, src_rate: Optional[int] = None) -> int:
        """wbx_engine_resample_sample: a new sample = the range converted to `dst_rate` ("fast" / "good" / "best"),
        registered at that rate — see MixContext.clip_resample; `frames` / `channels` as in export_sample.  The new
        sample's length is known here when the source's rate is (`src_rate`, or a sample add_sample* made).  May be called
        while another thread runs process()."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "resample_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        new = C.c_uint32()
        _check(self.L.wbx_engine_resample_sample(self.h, sample, first_frame, n_frames, dst_rate,
                                                 _ffi.SRC_QUALITY.get(quality, quality), C.byref(new)),
               "wbx_engine_resample_sample", self.h, True)
        src_rate = self._sample_rate.get(sample) if src_rate is None else src_rate
        self._sample_shape[new.value] = (resample_frames(src_rate, dst_rate, n_frames) if src_rate else None, channels)
        self._sample_rate[new.value] = dst_rate
        return new.value

    def filter_sample(self, sample: int, coef, tail_frames: int = 0, first_frame: int = 0, n_frames: Optional[int] = None,
                      channels: Optional[int] = None, frames: Optional[int] = None) -> int:
        """wbx_engine_filter_sample: a new sample = the range run through the cascade `coef` plus `tail_frames` of ring-out,
        registered at the source's rate — see MixContext.clip_filter; `frames` / `channels` as in export_sample.  May be
        called while another thread runs process(); delete_sample of the source is refused meanwhile."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "filter_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        new = C.c_uint32()
        k = _cascade(coef)
        _check(self.L.wbx_engine_filter_sample(self.h, sample, first_frame, n_frames, tail_frames, k.ctypes.data, len(k),
                                               C.byref(new)), "wbx_engine_filter_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames + tail_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value

    def add_fir(self, rate: int, taps) -> int:
        """fir_design(...)'s taps (or any fp32 response) as a mono F32 sample: the `ir_sample` of convolve_sample"""
        return self.add_sample("f32", rate, [np.ascontiguousarray(taps, dtype=np.float32)])

    def convolve_sample(self, sample: int, ir_sample: int, gain_db: float = 0.0, out_first: int = 0,
                        out_frames: Optional[int] = None, first_frame: int = 0, n_frames: Optional[int] = None, ir_first: int = 0,
                        ir_frames: Optional[int] = None, channels: Optional[int] = None, frames: Optional[int] = None,
                        ir_channels: Optional[int] = None, ir_length: Optional[int] = None, stats: bool = False):
        """wbx_engine_convolve_sample: a new sample = the range of `sample` convolved with the range of `ir_sample` (the
        impulse response; add_fir makes one of designed taps), times 10 ** (gain_db / 20) — see MixContext.clip_convolve.
        The window defaults to the full ring-out from `out_first` on; out_first = (taps - 1) // 2 with out_frames = n_frames
        drops a linear-phase FIR's delay.  `frames` / `channels` (`ir_length` / `ir_channels`) as in export_sample, for
        samples this object did not make.  Both samples are pinned against delete_sample for the call's length; may be called
        while another thread runs process().  Returns the new id, with `stats` (id, statistics of the result)."""
        frames, channels = self._shape_of(sample, frames, channels)
        ir_length, ir_channels = self._shape_of(ir_sample, ir_length, ir_channels)
        if n_frames is None:
            assert frames is not None, "convolve_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        if ir_frames is None:
            assert ir_length is not None, "convolve_sample: give ir_frames, or ir_length (the response's length)"
            ir_frames = ir_length - ir_first
        if out_frames is None:
            out_frames = n_frames + ir_frames - 1 - out_first
        new, st = C.c_uint32(), _ffi.ClipStats()
        _check(self.L.wbx_engine_convolve_sample(self.h, sample, ir_sample, first_frame, n_frames, ir_first, ir_frames, out_first,
                                                 out_frames, 10.0 ** (float(gain_db) / 20.0), C.byref(new),
                                                 C.byref(st) if stats else None), "wbx_engine_convolve_sample", self.h, True)
        out_channels = max(channels, ir_channels)
        self._sample_shape[new.value] = (out_frames, out_channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return (new.value, _clip_stats(st, out_channels)) if stats else new.value

    def limit_sample(self, sample: int, ceiling_db: float = -1.0, lookahead_ms: float = 1.5, hold_ms: float = 0.0,
                     release_ms: float = 100.0, drive_db: float = 0.0, first_frame: int = 0, n_frames: Optional[int] = None,
                     channels: Optional[int] = None, frames: Optional[int] = None, rate: Optional[int] = None,
                     shape: Optional[tuple] = None, stats: bool = False):
        """wbx_engine_limit_sample: a new sample = the range of `sample` times 10 ** (drive_db / 20) through the look-ahead
        peak limiter — see MixContext.clip_limit: no sample above 10 ** (ceiling_db / 20) (rounded to float32), the source's
        length, no delay.  The times become frames at the sample's rate (`rate` where this object did not make it) through
        limit_frames; `shape` = (lookahead, hold, release) in frames overrides them.  These conversions happen here and are
        not part of the bit-exact contract.  `frames` / `channels` as in export_sample.  The source is pinned against
        delete_sample for the call's length; may be called while another thread runs process().  Returns (new id, the
        limiter's statistics), with `stats` (id, those, the result's statistics)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "limit_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        A, H, R = shape if shape is not None else limit_frames(rate, lookahead_ms, hold_ms, release_ms)
        new, ls, st = C.c_uint32(), _ffi.LimitStats(), _ffi.ClipStats()
        _check(self.L.wbx_engine_limit_sample(self.h, sample, first_frame, n_frames, np.float32(10.0 ** (float(ceiling_db) / 20.0)),
                                              10.0 ** (float(drive_db) / 20.0), A, H, R, C.byref(new), C.byref(ls),
                                              C.byref(st) if stats else None), "wbx_engine_limit_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return (new.value, _limit_stats(ls), _clip_stats(st, channels)) if stats else (new.value, _limit_stats(ls))

    def stretch_sample(self, sample: int, out_frames: int, window_frames: int = 2048, tolerance_frames: int = 512,
                       first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                       frames: Optional[int] = None):
        """wbx_engine_stretch_sample: a new sample of out_frames frames = the range of `sample` time-stretched by WSOLA —
        see MixContext.clip_stretch.  `frames` / `channels` as in export_sample.  The source is pinned against
        delete_sample for the call's length; may be called while another thread runs process().  Returns (new id, info)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "stretch_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        new, si = C.c_uint32(), _ffi.StretchInfo()
        _check(self.L.wbx_engine_stretch_sample(self.h, sample, first_frame, n_frames, out_frames, window_frames, tolerance_frames,
                                                C.byref(si), C.byref(new)), "wbx_engine_stretch_sample", self.h, True)
        self._sample_shape[new.value] = (out_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, _stretch_info(si)

    def warp_sample(self, sample: int, out_frames: int, markers, window_frames: int = 2048, tolerance_frames: int = 512,
                    first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                    frames: Optional[int] = None):
        """wbx_engine_warp_sample: a new sample of out_frames frames = the range of `sample` warped along `markers`
        ((src_frame, out_frame) pairs relative to the range) — see MixContext.clip_warp.  `frames` / `channels` as in
        export_sample.  The source is pinned against delete_sample for the call's length; may be called while another
        thread runs process().  Returns (new id, info)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "warp_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        arr, M = _warp_markers(markers)
        new, wi = C.c_uint32(), _ffi.WarpInfo()
        _check(self.L.wbx_engine_warp_sample(self.h, sample, first_frame, n_frames, out_frames, arr, M, window_frames,
                                             tolerance_frames, C.byref(wi), C.byref(new)), "wbx_engine_warp_sample", self.h, True)
        self._sample_shape[new.value] = (out_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, _warp_info(wi)

    def warp_to_markers(self, sample: int, events, targets, out_frames: Optional[int] = None, lead: Optional[int] = None,
                        window_frames: int = 2048, tolerance_frames: int = 512, **call):
        """A sample warped so that the event at source frame events[i] sounds at output frame targets[i] (both relative to
        the range; out_frames defaults to the range's length).  Each pair becomes the marker (event - lead, target - lead),
        lead = window_frames / 2 by default: a marker a hop early leaves the hop behind it to the natural continuation, so
        an attack stays intact.  The pairs are taken in ascending order of their event; a pair is DROPPED where its marker
        would break a rule of the call given the markers kept so far: a frame that is not above the last kept marker's (or
        0) in either column, a source frame not below n_frames or an output frame not below out_frames, or a ratio beyond
        8 either way of the segment from the last kept marker to it or of the segment from it to the end.  These choices
        happen here: a convenience outside the bit-exact contract; the samples are the model's for the markers reported
        back.  `call`: warp_sample's first_frame, n_frames, frames, channels.  Returns (new id, info, the markers used)."""
        frames, _ = self._shape_of(sample, call.get("frames"), call.get("channels"))
        n = call.get("n_frames")
        if n is None:
            assert frames is not None, "warp_to_markers: give n_frames, or frames (the sample's length)"
            n = frames - call.get("first_frame", 0)
        m = n if out_frames is None else int(out_frames)
        lead = window_frames // 2 if lead is None else int(lead)

        def fits(a, b):                      # a segment of a source frames into b output frames
            return a > 0 and b > 0 and b <= 8 * a and a <= 8 * b

        kept, last = [], (0, 0)
        for ev, tg in sorted((int(e), int(t)) for e, t in zip(events, targets)):
            s, t = ev - lead, tg - lead
            if s >= n or t >= m or not fits(s - last[0], t - last[1]) or not fits(n - s, m - t):
                continue
            kept.append((s, t))
            last = (s, t)
        new, info = self.warp_sample(sample, m, kept, window_frames, tolerance_frames, **call)
        return new, info, kept

    def quantize_sample(self, sample: int, bpm: float, division: int = 4, strength: float = 1.0, onsets: Optional[dict] = None,
                        rate: Optional[int] = None, **warp):
        """A sample with its onsets moved towards the grid: onsets_sample (`onsets`: its arguments), each onset frame moved
        by `strength` of the way to the nearest line of a grid of 60 * rate / (bpm * division) frames, then warp_to_markers
        at the range's own length (`warp`: its arguments).  Outside the bit-exact contract, like warp_to_markers.  Returns
        (new id, info, the markers used)."""
        onsets = dict(onsets or {})
        for k in ("first_frame", "n_frames", "frames", "channels"):
            if k in warp:
                onsets.setdefault(k, warp[k])
        rec, _ = self.onsets_sample(sample, **onsets)
        H = int(onsets.get("hop_frames", 256))
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        grid = 60.0 * rate / (float(bpm) * float(division))
        events = [int(h) * H for h in np.flatnonzero(rec["onset"])]
        targets = [int(round(e + float(strength) * (round(e / grid) * grid - e))) for e in events]
        return self.warp_to_markers(sample, events, targets, **warp)

    def stretch_to_tempo(self, sample: int, bpm_from: float, bpm_to: float, window_ms: float = 40.0, tolerance_ms: float = 10.0,
                         rate: Optional[int] = None, **call):
        """A sample recorded at `bpm_from` fitted to `bpm_to`: stretch_sample to round(n_frames * bpm_from / bpm_to) frames
        (at least 1), the window rounded to a multiple of 8 frames in 32 .. 8192 and the tolerance to a frame in 0 .. 4096 at
        the sample's rate (`rate` where this object did not make it).  These conversions happen here: a convenience
        outside the bit-exact contract.  `call`: stretch_sample's first_frame, n_frames, frames, channels"""
        frames, _ = self._shape_of(sample, call.get("frames"), call.get("channels"))
        n = call.get("n_frames")
        if n is None:
            assert frames is not None, "stretch_to_tempo: give n_frames, or frames (the sample's length)"
            n = frames - call.get("first_frame", 0)
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        out_frames = max(1, int(round(n * float(bpm_from) / float(bpm_to))))
        window = min(8192, max(32, 8 * int(round(float(window_ms) * rate / 8000.0))))
        tolerance = min(4096, max(0, int(round(float(tolerance_ms) * rate / 1000.0))))
        return self.stretch_sample(sample, out_frames, window, tolerance, **call)

    def pitch_sample(self, sample: int, num: int, den: int, out_frames: Optional[int] = None, quality="good",
                     window_frames: int = 2048, tolerance_frames: int = 512, first_frame: int = 0,
                     n_frames: Optional[int] = None, channels: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_pitch_sample: a new sample of out_frames frames (default: the range's own length) = the range of
        `sample` transposed by num / den at the sample's rate — see MixContext.clip_pitch.  `frames` / `channels` as in
        export_sample.  The source is pinned against delete_sample for the call's length; may be called while another thread
        runs process().  Returns (new id, info)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "pitch_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        out_frames = n_frames if out_frames is None else out_frames
        new, pi = C.c_uint32(), _ffi.PitchInfo()
        _check(self.L.wbx_engine_pitch_sample(self.h, sample, first_frame, n_frames, out_frames, num, den,
                                              _ffi.SRC_QUALITY.get(quality, quality), window_frames, tolerance_frames,
                                              C.byref(pi), C.byref(new)), "wbx_engine_pitch_sample", self.h, True)
        self._sample_shape[new.value] = (out_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, _pitch_info(pi)

    def transpose_sample(self, sample: int, semitones: float, cents: float = 0.0, window_ms: float = 40.0,
                         tolerance_ms: float = 10.0, quality="good", rate: Optional[int] = None, **call):
        """A sample transposed by `semitones` and `cents` at its own length: pitch_sample with pitch_ratio(semitones, cents),
        the window rounded to a multiple of 8 frames in 32 .. 8192 and the tolerance to a frame in 0 .. 4096 at the sample's
        rate (`rate` where this object did not make it), as stretch_to_tempo rounds them.  These conversions happen here: a
        convenience outside the bit-exact contract.  `call`: pitch_sample's out_frames, first_frame, n_frames, frames,
        channels"""
        num, den = pitch_ratio(semitones, cents)
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        window = min(8192, max(32, 8 * int(round(float(window_ms) * rate / 8000.0))))
        tolerance = min(4096, max(0, int(round(float(tolerance_ms) * rate / 1000.0))))
        return self.pitch_sample(sample, num, den, quality=quality, window_frames=window, tolerance_frames=tolerance, **call)

    def f0_sample(self, sample: int, window_frames: int = 1024, hop_frames: int = 256, tau_min: int = 24, tau_max: int = 1024,
                  threshold: float = 0.15, first_frame: int = 0, n_frames: Optional[int] = None,
                  channels: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_f0_sample — see MixContext.clip_f0; `frames` / `channels` as in export_sample.  Returns (records, info).
        May be called while another thread runs process(); delete_sample of the sample is refused meanwhile."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "f0_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        return _run_f0(self.L.wbx_engine_f0_sample, "wbx_engine_f0_sample", self.h, True, sample, first_frame, n_frames,
                       window_frames, hop_frames, tau_min, tau_max, threshold)

    def detect_note_sample(self, sample: int, rate: Optional[int] = None, floor_db: float = 40.0, a4_hz: float = 440.0, **call):
        """The note of a sample: f0_sample (`call`: its arguments), then the MEDIAN period of the voiced hops whose energy
        lies within `floor_db` of the loudest hop's.  Returns {"hz", "midi" (the nearest note, 69 = A4 at `a4_hz`), "cents"
        (off that note, -50 .. 50), "voiced" (the share of hops that are voiced), "period", "hops"}; hz, midi, cents and
        period are None where no such hop is voiced.  `rate` where this object did not make the sample.  The median, the
        logarithm and the rounding happen here: a convenience outside the bit-exact contract."""
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        rec, info = self.f0_sample(sample, **call)
        out = {"hz": None, "midi": None, "cents": None, "period": None, "hops": int(info["hops"]),
               "voiced": float(info["voiced_hops"]) / info["hops"] if info["hops"] else 0.0}
        if rec.size == 0:
            return out
        keep = (rec["voiced"] != 0) & (rec["energy"] >= rec["energy"].max() * 10.0 ** (-float(floor_db) / 10.0))
        if not keep.any():
            return out
        period = float(np.median(rec["period"][keep]))
        hz = float(rate) / period
        note = 69.0 + 12.0 * float(np.log2(hz / float(a4_hz)))
        midi = int(np.floor(note + 0.5))
        out.update(hz=hz, midi=midi, cents=100.0 * (note - midi), period=period)
        return out

    def tune_sample(self, sample: int, to_midi: Optional[int] = None, a4_hz: float = 440.0, detect: Optional[dict] = None,
                    **transpose):
        """A sample tuned to a note: detect_note_sample (`detect`: its arguments), then transpose_sample by the cents that
        bring the detected frequency to MIDI note `to_midi` (default: the nearest note) through pitch_ratio (`transpose`:
        transpose_sample's arguments).  Returns (new id, info, the detected note).  ValueError where no hop is voiced, or
        where the correction rounds to a ratio of 1 (the sample is in tune within pitch_ratio's grid)."""
        detect = dict(detect or {})
        if "rate" in transpose:
            detect.setdefault("rate", transpose["rate"])
        note = self.detect_note_sample(sample, a4_hz=a4_hz, **detect)
        if note["hz"] is None:
            raise ValueError("tune_sample: no voiced hop, so no pitch to tune")
        target = note["midi"] if to_midi is None else int(to_midi)
        cents = 100.0 * (target - note["midi"]) - note["cents"]
        new, info = self.transpose_sample(sample, 0.0, cents, **transpose)   # (pitch_ratio raises for a ratio of 1)
        return new, info, note

    def _range_of(self, what, sample, first_frame, n_frames, frames, channels):
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, what + ": give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        return n_frames

    def onsets_sample(self, sample: int, hop_frames: int = 256, floor_power: float = 1e-9, threshold: float = 0.3,
                      delta: float = 0.1, w: int = 3, a: int = 8, first_frame: int = 0, n_frames: Optional[int] = None,
                      channels: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_onsets_sample — see MixContext.clip_onsets; `frames` / `channels` as in export_sample.  Returns
        (records, info).  May be called while another thread runs process(); delete_sample of the sample is refused
        meanwhile."""
        n_frames = self._range_of("onsets_sample", sample, first_frame, n_frames, frames, channels)
        return _run_onsets(self.L.wbx_engine_onsets_sample, "wbx_engine_onsets_sample", self.h, True, sample, first_frame, n_frames,
                           hop_frames, floor_power, threshold, delta, w, a)

    def tempo_sample(self, sample: int, hop_frames: int = 256, floor_power: float = 1e-9, window_hops: int = 1024,
                     step_hops: int = 64, lag_min: int = 56, lag_max: int = 188, threshold: float = 0.5, first_frame: int = 0,
                     n_frames: Optional[int] = None, channels: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_tempo_sample — see MixContext.clip_tempo.  Returns (records, info); pinned like onsets_sample."""
        n_frames = self._range_of("tempo_sample", sample, first_frame, n_frames, frames, channels)
        return _run_tempo(self.L.wbx_engine_tempo_sample, "wbx_engine_tempo_sample", self.h, True, sample, first_frame, n_frames,
                          hop_frames, floor_power, window_hops, step_hops, lag_min, lag_max, threshold)

    def add_spectrum_basis(self, window_frames: int, freqs, lengths=None, window="hann", kaiser_beta: float = 8.6,
                           rate: Optional[int] = None) -> int:
        """spectrum_basis(...)'s words as a mono F32 sample: the `basis_sample` of spectrum_sample, as add_fir makes a
        response (`rate` is a label only: frequencies are in cycles per frame)"""
        words = spectrum_basis(window_frames, freqs, lengths, window, kaiser_beta)
        return self.add_sample("f32", self.audio_sample_rate if rate is None else rate, [words])

    def spectrum_sample(self, sample: int, basis_sample: int, window_frames: int, n_bins: int, hop_frames: int, channel="mid",
                        first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                        frames: Optional[int] = None):
        """wbx_engine_spectrum_sample — see MixContext.clip_spectrum; `frames` / `channels` as in export_sample.  Returns
        (power float32[hops][n_bins], info).  May be called while another thread runs process(); delete_sample of the
        sample or of the basis sample is refused meanwhile."""
        n_frames = self._range_of("spectrum_sample", sample, first_frame, n_frames, frames, channels)
        return _run_spectrum(self.L.wbx_engine_spectrum_sample, "wbx_engine_spectrum_sample", self.h, True, sample, first_frame,
                             n_frames, channel, basis_sample, window_frames, n_bins, hop_frames)

    def align_samples(self, ref_sample: int, sample: int, lag_min: int, lag_max: int, n_frames: Optional[int] = None,
                      a_first: int = 0, b_first: int = 0, m_frames: Optional[int] = None, either_polarity=False, curve: bool = False,
                      ref_frames: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_align_samples — see MixContext.clip_align: by how many frames `sample` lags `ref_sample`.  `n_frames`
        None: the reference from a_first to its end, rounded DOWN to a multiple of 8; `m_frames` None: the sample from
        b_first to its end; `ref_frames` / `frames`: the samples' lengths where this object did not make them.  Returns
        (info, curve or None).  May be called while another thread runs process(); delete_sample of either sample is refused
        meanwhile."""
        if n_frames is None:
            n_frames = min(self._range_of("align_samples", ref_sample, a_first, None, ref_frames, None), 1 << 24) & ~7
        m_frames = self._range_of("align_samples", sample, b_first, m_frames, frames, None)
        return _run_align(self.L.wbx_engine_align_samples, "wbx_engine_align_samples", self.h, True, ref_sample, a_first, n_frames,
                          sample, b_first, m_frames, lag_min, lag_max, either_polarity, curve)

    def aligned_sample(self, ref_sample: int, sample: int, max_lag: int, either_polarity: bool = True, ref_frames: Optional[int] = None,
                       frames: Optional[int] = None, channels: Optional[int] = None, **call):
        """A NEW sample: `sample` moved by the lag align_samples finds within -max_lag .. max_lag of `ref_sample` (`call`: its
        further arguments), so that its frame i is what lines up with the reference's frame i — its head trimmed (a derive)
        where it lags, silence put in front (a splice) where it leads — and its polarity flipped (gain -1) when
        either_polarity finds it inverted.  Built from existing calls, outside the bit-exact contract.  Returns
        (new sample, info)."""
        info, _ = self.align_samples(ref_sample, sample, -max_lag, max_lag, either_polarity=either_polarity, ref_frames=ref_frames,
                                     frames=frames, **call)
        total, channels = self._shape_of(sample, frames, channels)
        assert total is not None, "aligned_sample: give frames (the sample's length)"
        lag, gain = info["lag"], -1.0 if info["inverted"] else 1.0
        assert -total < lag < total, "aligned_sample: the lag leaves nothing of the sample"
        if lag >= 0:
            new = self.derive_sample(sample, edit_desc(lag, total - lag, gain=gain), channels)
        else:
            new = self.splice_samples(channels, total - lag, [splice_part(sample, 0, total, at=-lag, gain=gain)])
        return new, info

    def measure_latency(self, played: int, recorded: int, max_frames: int, played_frames: Optional[int] = None,
                        recorded_frames: Optional[int] = None, **call) -> int:
        """The round-trip latency of a loopback in frames: the lag in 0 .. max_frames at which the take `recorded` matches
        `played` best (align_samples over the whole of `played`, rounded down to a multiple of 8; `call`: its further
        arguments).  A take's length is record_info()["frames"]: pass it as recorded_frames."""
        info, _ = self.align_samples(played, recorded, 0, max_frames, ref_frames=played_frames, frames=recorded_frames, **call)
        return info["lag"]

    def spectrogram_sample(self, sample: int, f_min: float, bins_per_octave: float, n_bins: int, window: int = 2048,
                           hop: int = 512, constant_q: bool = False, cycles: Optional[float] = None, window_kind="hann",
                           channel="mid", **call):
        """A logarithmic spectrogram of a sample: a basis of n_bins frequencies from f_min (cycles per frame) upwards,
        bins_per_octave to the octave (spectrum_log_freqs: what would pass 0.5 sits at 0.5), designed, uploaded, measured by
        spectrum_sample (`call`: its first_frame, n_frames, frames, channels) and deleted again.  With constant_q each bin's
        window holds `cycles` of its periods (default: as many as the lowest bin has in `window`), a multiple of 4 frames in
        4 .. window.  Returns (power [hops][n_bins], freqs, info).  The lengths and their rounding happen here: a
        convenience outside the bit-exact contract — the cells equal the model's for the basis this designs."""
        freqs, _ = spectrum_log_freqs(f_min, bins_per_octave, n_bins)
        lengths = None
        if constant_q:
            cycles = float(window) * float(freqs[0]) if cycles is None else float(cycles)
            lengths = []
            for f in freqs:
                L = int(round(cycles / f))
                lengths.append(max(4, min(int(window), L - L % 4)))
        basis = self.add_spectrum_basis(window, freqs, lengths, window_kind)
        try:
            power, info = self.spectrum_sample(sample, basis, window, n_bins, hop, channel=channel, **call)
        finally:
            self.delete_sample(basis)
        return power, freqs, info

    def chroma_sample(self, sample: int, f_c: float, octaves: int = 5, window: int = 4096, hop: int = 1024, constant_q: bool = True,
                      **call):
        """A chromagram of a sample: spectrogram_sample over a semitone basis of 12 * octaves bins from f_c upwards (cycles
        per frame: the lowest C, or whichever pitch class 0 shall be), each hop's powers folded into 12 pitch classes on the
        host in fp64, the octaves added in ascending order from 0.0 (tests/spectrum_model.py chroma_fold).  Returns
        (chroma float64[hops][12], info)."""
        power, _, info = self.spectrogram_sample(sample, f_c, 12.0, 12 * int(octaves), window, hop, constant_q=constant_q, **call)
        cells = power.astype(np.float64)
        chroma = np.zeros((cells.shape[0], 12), dtype=np.float64)
        for o in range(int(octaves)):
            chroma = chroma + cells[:, 12 * o:12 * o + 12]
        return chroma, info

    def detect_tempo_sample(self, sample: int, bpm_min: float = 70.0, bpm_max: float = 180.0, rate: Optional[int] = None,
                            hop_frames: int = 256, window_hops: int = 1024, step_hops: int = 64, threshold: float = 0.5, **call):
        """The tempo of a sample: tempo_sample with the lags of bpm_max .. bpm_min at the sample's rate (`rate` where this
        object did not make it; `call`: tempo_sample's other arguments), then the MEDIAN period of the voiced windows.
        Returns {"bpm", "period" (in hops), "voiced" (the share of windows that are voiced), "windows"}; bpm and period are
        None where no window is voiced.  The lag range decides the octave: a loop at half of bpm_max or below may come out
        doubled.  The lags, the median and the division happen here: a convenience outside the bit-exact contract."""
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        per_minute = 60.0 * float(rate) / float(hop_frames)          # hops per minute: bpm = per_minute / period
        lag_min = max(2, int(np.floor(per_minute / float(bpm_max))))
        lag_max = min(4095, max(lag_min + 1, 8, int(np.ceil(per_minute / float(bpm_min)))))
        rec, info = self.tempo_sample(sample, hop_frames=hop_frames, window_hops=window_hops, step_hops=step_hops, lag_min=lag_min,
                                      lag_max=lag_max, threshold=threshold, **call)
        out = {"bpm": None, "period": None, "windows": int(info["hops"]),
               "voiced": float(info["voiced_hops"]) / info["hops"] if info["hops"] else 0.0}
        keep = rec["voiced"] != 0
        if keep.any():
            period = float(np.median(rec["period"][keep]))
            out.update(bpm=per_minute / period, period=period)
        return out

    def fit_sample_to_tempo(self, sample: int, bpm_to: float, detect: Optional[dict] = None, **stretch):
        """A sample of unknown tempo fitted to `bpm_to`: detect_tempo_sample (`detect`: its arguments), then stretch_to_tempo
        from the detected bpm (`stretch`: its arguments).  Returns (new id, info, the detected tempo).  ValueError where no
        window is voiced."""
        detect = dict(detect or {})
        for k in ("rate", "first_frame", "n_frames", "frames", "channels"):
            if k in stretch:
                detect.setdefault(k, stretch[k])
        tempo = self.detect_tempo_sample(sample, **detect)
        if tempo["bpm"] is None:
            raise ValueError("fit_sample_to_tempo: no voiced window, so no tempo to fit")
        new, info = self.stretch_to_tempo(sample, tempo["bpm"], bpm_to, **stretch)
        return new, info, tempo

    def slice_sample(self, sample: int, first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                     frames: Optional[int] = None, **onsets):
        """A sample cut at its onsets: onsets_sample (`onsets`: its arguments), then one derive_sample trim per stretch
        between consecutive onset frames h * hop_frames, the last reaching the end of the range.  Returns (the new ids, the
        (first frame, frames) of each piece): the pieces concatenate to the range from the first onset on.  No onset: no
        piece."""
        n_frames = self._range_of("slice_sample", sample, first_frame, n_frames, frames, channels)
        rec, _ = self.onsets_sample(sample, first_frame=first_frame, n_frames=n_frames, channels=channels, frames=frames, **onsets)
        H = int(onsets.get("hop_frames", 256))
        cuts = [first_frame + int(h) * H for h in np.flatnonzero(rec["onset"])] + [first_frame + n_frames]
        pieces = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]
        return [self.derive_sample(sample, edit_desc(at, n), channels=channels) for at, n in pieces], pieces

    def dynamics_sample(self, sample: int, table, sense="compress", key_sample: Optional[int] = None, key_first: int = 0,
                        drive: float = 1.0, key_gain: float = 1.0, makeup: float = 1.0, shape: tuple = (72, 0, 4800),
                        first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                        frames: Optional[int] = None, stats: bool = False):
        """wbx_engine_dynamics_sample: a new sample = the range of `sample` through the table-driven dynamics processor —
        see MixContext.clip_dynamics; `shape` = (lookahead, hold, release) in frames, gains linear.  `frames` / `channels` as
        in export_sample.  The source and the key are pinned against delete_sample for the call's length; may be called
        while another thread runs process().  Returns (new id, the statistics), with `stats` (id, those, the result's
        statistics)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "dynamics_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        A, H, R = shape
        t, new, ds, st = _dyn_table(table), C.c_uint32(), _ffi.DynamicsStats(), _ffi.ClipStats()
        _check(self.L.wbx_engine_dynamics_sample(self.h, sample, _ffi.DYN_NO_KEY if key_sample is None else key_sample, first_frame,
                                                 n_frames, key_first, _ffi.DYN_SENSE.get(sense, sense), t.ctypes.data, float(drive),
                                                 float(key_gain), float(makeup), A, H, R, C.byref(new), C.byref(ds),
                                                 C.byref(st) if stats else None), "wbx_engine_dynamics_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return (new.value, _dynamics_stats(ds), _clip_stats(st, channels)) if stats else (new.value, _dynamics_stats(ds))

    def saturate_sample(self, sample: int, table, os: int = 4, quality="good", drive: float = 1.0, makeup: float = 1.0,
                        first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                        frames: Optional[int] = None, stats: bool = False):
        """wbx_engine_saturate_sample: a new sample = the range of `sample` through the oversampled table waveshaper — see
        MixContext.clip_saturate; gains linear.  `frames` / `channels` as in export_sample.  The source is pinned against
        delete_sample for the call's length; may be called while another thread runs process().  Returns (new id, the
        statistics), with `stats` (id, those, the result's statistics)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "saturate_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        t, new, ss, st = _sat_table(table), C.c_uint32(), _ffi.SaturateStats(), _ffi.ClipStats()
        _check(self.L.wbx_engine_saturate_sample(self.h, sample, first_frame, n_frames, os, _ffi.SRC_QUALITY.get(quality, quality),
                                                 t.ctypes.data, float(drive), float(makeup), C.byref(new), C.byref(ss),
                                                 C.byref(st) if stats else None), "wbx_engine_saturate_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return (new.value, _saturate_stats(ss), _clip_stats(st, channels)) if stats else (new.value, _saturate_stats(ss))

    def varispeed_sample(self, sample: int, out_frames: int, knots, knot_shift: int, quality="good", guard_num: int = 1,
                         guard_den: int = 1, first_frame: int = 0, n_frames: Optional[int] = None,
                         channels: Optional[int] = None, frames: Optional[int] = None, stats: bool = False):
        """wbx_engine_varispeed_sample: a new sample of out_frames frames = the range of `sample` read along the position
        curve `knots` — see MixContext.clip_varispeed.  `frames` / `channels` as in export_sample.  The source is pinned
        against delete_sample for the call's length; may be called while another thread runs process().  Returns the new
        id, with `stats` (id, the result's statistics)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "varispeed_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        k, new, st = (None if knots is None else _vs_knots(knots)), C.c_uint32(), _ffi.ClipStats()
        _check(self.L.wbx_engine_varispeed_sample(self.h, sample, first_frame, n_frames, out_frames,
                                                  None if k is None else k.ctypes.data, 0 if k is None else k.size, knot_shift,
                                                  _vs_q(quality), guard_num, guard_den, C.byref(new), C.byref(st) if stats else None),
               "wbx_engine_varispeed_sample", self.h, True)
        self._sample_shape[new.value] = (out_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return (new.value, _clip_stats(st, channels)) if stats else new.value

    def _vs_range(self, what, sample, call):
        frames, _ = self._shape_of(sample, call.get("frames"), call.get("channels"))
        n = call.get("n_frames")
        if n is None:
            assert frames is not None, what + ": give n_frames, or frames (the sample's length)"
            n = frames - call.get("first_frame", 0)
        return n

    def tape_stop_sample(self, sample: int, at_frame: int, ramp_frames: int, quality="good", knot_shift: int = 6, **call):
        """A tape stop: the range plays at speed 1 up to output frame `at_frame`, then the speed falls linearly to 0 over
        `ramp_frames`; the result has at_frame + ramp_frames frames.  The knots come from varispeed_knots: a convenience
        outside the bit-exact contract, the samples are the model's for the knots reported back.  `call`:
        varispeed_sample's first_frame, n_frames, frames, channels.  Returns (new id, {"knots", "knot_shift", "out_frames",
        "guard"})"""
        self._vs_range("tape_stop_sample", sample, call)
        out_frames = int(at_frame) + int(ramp_frames)
        pts = [(0, 1.0), (int(at_frame), 1.0), (out_frames, 0.0)] if at_frame > 0 else [(0, 1.0), (out_frames, 0.0)]
        knots, guard = varispeed_knots(pts, out_frames, knot_shift)
        new = self.varispeed_sample(sample, out_frames, knots, knot_shift, quality, guard[0], guard[1], **call)
        return new, {"knots": knots, "knot_shift": knot_shift, "out_frames": out_frames, "guard": guard}

    def vibrato_sample(self, sample: int, rate_hz: float, depth_cents: float, quality="good", knot_shift: int = 4,
                       rate: Optional[int] = None, **call):
        """Vibrato (wow, flutter): the range at its own length, read at j + a sin(2 pi rate_hz j / rate), a chosen so that
        the speed swings between 2^(-depth_cents / 1200) and 2^(depth_cents / 1200) about 1.  Outside the bit-exact
        contract, like tape_stop_sample.  Returns (new id, {"knots", "knot_shift", "out_frames", "guard"})"""
        n = self._vs_range("vibrato_sample", sample, call)
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        dev = 2.0 ** (float(depth_cents) / 1200.0) - 1.0
        w = 2.0 * np.pi * float(rate_hz) / float(rate)
        G = 1 << knot_shift
        j = np.arange((n + G - 1) // G + 1, dtype=np.float64) * G
        pos = j + (dev / w) * np.sin(w * j)
        knots = np.array([int(round(float(v) * 4294967296.0)) for v in pos], dtype=np.int64)
        guard = _vs_guard(1.0 + dev)
        new = self.varispeed_sample(sample, n, knots, knot_shift, quality, guard[0], guard[1], **call)
        return new, {"knots": knots, "knot_shift": knot_shift, "out_frames": n, "guard": guard}

    def drift_sample(self, sample: int, ppm: float, quality="good", knot_shift: int = 10, **call):
        """A recording whose clock ran `ppm` parts per million fast conformed: the range read at the constant speed
        1 + ppm / 10^6 into round(n / speed) frames (guard 1: the interpolator's own margin covers a drift).  The knots are
        exact integers of that speed as a fraction.  Returns (new id, {"knots", "knot_shift", "out_frames", "guard"})"""
        n = self._vs_range("drift_sample", sample, call)
        speed = 1 + Fraction(float(ppm)).limit_denominator(10 ** 9) / 10 ** 6
        out_frames = max(1, int(round(n / speed)))
        G = 1 << knot_shift
        K = (out_frames + G - 1) // G + 1
        knots = np.array([int((i * G * speed * (1 << 32)).__floor__()) for i in range(K)], dtype=np.int64)
        new = self.varispeed_sample(sample, out_frames, knots, knot_shift, quality, 1, 1, **call)
        return new, {"knots": knots, "knot_shift": knot_shift, "out_frames": out_frames, "guard": (1, 1)}

    def pitch_curve_sample(self, sample: int, segments, quality="good", window_frames: int = 2048, tolerance_frames: int = 512,
                           **call):
        """Pitch that changes over time at unchanged timing: `segments` = [(first_frame, ratio)] relative to the range, the
        first at 0, each ratio (within 1/8 .. 8) holding up to the next segment.  warp_sample stretches each segment by its
        ratio into an intermediate sample; this call then plays the intermediate back at that ratio (knot_shift 4), so every
        boundary keeps its frame and the result has the range's length.  Boundaries are moved to multiples of 16 frames (a
        knot stands there); the intermediate is deleted.  Outside the bit-exact contract, like tape_stop_sample: the result
        is warp's model followed by this call's model for the markers and knots reported back.  Returns (new id, {"markers",
        "mid_frames", "knots", "knot_shift", "out_frames", "guard"})"""
        n = self._vs_range("pitch_curve_sample", sample, call)
        seg = sorted((min(n, (int(f) + 8) // 16 * 16), Fraction(float(r)).limit_denominator(1 << 12)) for f, r in segments)
        assert seg and seg[0][0] == 0, "pitch_curve_sample: the first segment starts at frame 0"
        bounds, ratios = [], []
        for f, r in seg:
            if bounds and f == bounds[-1]:
                ratios[-1] = r
            elif f < n:
                bounds.append(f)
                ratios.append(r)
        bounds.append(n)
        mid = [0]
        for a, b, r in zip(bounds, bounds[1:], ratios):
            mid.append(mid[-1] + max(1, int(round((b - a) * r))))
        markers = list(zip(bounds[1:-1], mid[1:-1]))
        tmp, _ = self.warp_sample(sample, mid[-1], markers, window_frames, tolerance_frames, **call)
        K = (n + 15) // 16 + 1
        knots, s = np.zeros(K, dtype=np.int64), 0
        for i in range(K):
            j = i * 16
            while s + 2 < len(bounds) and j >= bounds[s + 1]:
                s += 1
            knots[i] = (mid[s] << 32) + ((j - bounds[s]) * ((mid[s + 1] - mid[s]) << 32)) // (bounds[s + 1] - bounds[s])
        guard = _vs_guard(max(float(r) for r in ratios))
        try:
            new = self.varispeed_sample(tmp, n, knots, 4, quality, guard[0], guard[1], frames=mid[-1], channels=call.get("channels"))
        finally:
            self.delete_sample(tmp)
        return new, {"markers": markers, "mid_frames": mid[-1], "knots": knots, "knot_shift": 4, "out_frames": n, "guard": guard}

    def denoise_sample(self, sample: int, window_frames: int, thr, floor: float = 0.1, smooth_hops: int = 2, smooth_bins: int = 1,
                       first_frame: int = 0, n_frames: Optional[int] = None, channels: Optional[int] = None,
                       frames: Optional[int] = None):
        """wbx_engine_denoise_sample: a new sample = the range of `sample` through the spectral gate — see
        MixContext.clip_denoise.  `frames` / `channels` as in export_sample.  The source is pinned against delete_sample for
        the call's length; may be called while another thread runs process().  Returns (new id, the statistics)."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "denoise_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        t, new, st = _denoise_thr(thr), C.c_uint32(), _ffi.DenoiseStats()
        _check(self.L.wbx_engine_denoise_sample(self.h, sample, first_frame, n_frames, window_frames, smooth_hops, smooth_bins,
                                                t.ctypes.data, float(floor), C.byref(new), C.byref(st)),
               "wbx_engine_denoise_sample", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if sample in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[sample]
        return new.value, _denoise_stats(st)

    def denoise_profile_sample(self, sample: int, window_frames: int, first_frame: int = 0, n_frames: Optional[int] = None,
                               channels: Optional[int] = None, frames: Optional[int] = None):
        """wbx_engine_denoise_profile_sample — see MixContext.clip_denoise_profile; `frames` / `channels` as in
        export_sample.  Returns (sums float64[channels * B], hops).  May be called while another thread runs process();
        delete_sample of the sample is refused meanwhile."""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "denoise_profile_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        sums, hops = np.zeros(channels * (window_frames // 2 + 1), dtype=np.float64), C.c_uint64()
        _check(self.L.wbx_engine_denoise_profile_sample(self.h, sample, first_frame, n_frames, window_frames, sums.ctypes.data,
                                                        C.byref(hops)), "wbx_engine_denoise_profile_sample", self.h, True)
        return sums, hops.value

    def reduce_noise_sample(self, sample: int, noise_first: int, noise_frames: int, reduction_db: float = 20.0,
                            sensitivity: float = 3.0, window: int = 1024, smooth_hops: int = 2, smooth_bins: int = 1,
                            noise_sample: Optional[int] = None, **call):
        """Noise reduction in one step: the profile of frames [noise_first, noise_first + noise_frames) of `noise_sample`
        (None: of `sample` itself) — a stretch that holds the noise alone —, the threshold denoise_threshold(sums, hops,
        sensitivity), floor = 10 ** (-reduction_db / 20), then denoise_sample.  The dB are converted here: a convenience
        outside the bit-exact contract.  `call`: denoise_sample's first_frame, n_frames, frames, channels.  Returns (new id,
        the statistics)"""
        src = sample if noise_sample is None else noise_sample
        sums, hops = self.denoise_profile_sample(src, window, noise_first, noise_frames, channels=call.get("channels"))
        thr = denoise_threshold(sums, hops, sensitivity)
        return self.denoise_sample(sample, window, thr, floor=10.0 ** (-float(reduction_db) / 20.0), smooth_hops=smooth_hops,
                                   smooth_bins=smooth_bins, **call)

    def soft_clip_sample(self, sample: int, ceiling_db: float = -1.0, drive_db: float = 0.0, kind="cubic", oversample: int = 4,
                         guarantee: bool = True, bias: float = 0.0, quality="good", **call):
        """A soft clipper: saturate_sample with saturate_table(kind, bias), drive = 10 ** (drive_db / 20) / ceiling and
        makeup = ceiling, so the curve's +-1 lands on the ceiling.  The band-limiting overshoots it; with `guarantee` a
        limit_sample at the ceiling follows (the intermediate sample is deleted), so the limiter's promise holds for the
        overshoot.  dB are converted here: a convenience outside the bit-exact contract.  `call`: saturate_sample's
        first_frame, n_frames, frames, channels.  Returns (new id, the saturate statistics)"""
        ceiling = 10.0 ** (float(ceiling_db) / 20.0)
        new, ss = self.saturate_sample(sample, saturate_table(kind, bias), os=oversample, quality=quality,
                                       drive=10.0 ** (float(drive_db) / 20.0) / ceiling, makeup=ceiling, **call)
        if not guarantee:
            return new, ss
        out, _ = self.limit_sample(new, ceiling_db=ceiling_db)
        self.delete_sample(new)
        return out, ss

    def _dynamics_shape(self, sample, rate, attack_ms, hold_ms, release_ms):
        rate = self._sample_rate.get(sample, self.audio_sample_rate) if rate is None else rate
        return limit_frames(rate, attack_ms, hold_ms, release_ms)

    def compress_sample(self, sample: int, threshold_db: float = -18.0, ratio: float = 4.0, knee_db: float = 6.0,
                        makeup_db: float = 0.0, attack_ms: float = 5.0, hold_ms: float = 0.0, release_ms: float = 100.0,
                        range_db: float = -np.inf, rate: Optional[int] = None, **call):
        """A compressor: dynamics_sample in the compress sense with dynamics_table("compress", ...); the attack is the
        look-ahead (the gain is down when the loud passage arrives).  dB and ms are converted here (limit_frames): a
        convenience outside the bit-exact contract.  `call`: dynamics_sample's first_frame, n_frames, frames, channels,
        stats, drive"""
        return self.dynamics_sample(sample, dynamics_table("compress", threshold_db, ratio, knee_db, range_db), "compress",
                                    makeup=10.0 ** (float(makeup_db) / 20.0),
                                    shape=self._dynamics_shape(sample, rate, attack_ms, hold_ms, release_ms), **call)

    def gate_sample(self, sample: int, threshold_db: float = -40.0, ratio: float = 10.0, knee_db: float = 0.0,
                    range_db: float = -80.0, attack_ms: float = 1.0, hold_ms: float = 20.0, release_ms: float = 100.0,
                    rate: Optional[int] = None, **call):
        """A downward expander or gate: dynamics_sample in the gate sense with dynamics_table("gate", ...): open `attack_ms`
        before the signal crosses the threshold, held, closed over `release_ms`, never below `range_db`.  Conversions as in
        compress_sample"""
        return self.dynamics_sample(sample, dynamics_table("gate", threshold_db, ratio, knee_db, range_db), "gate",
                                    shape=self._dynamics_shape(sample, rate, attack_ms, hold_ms, release_ms), **call)

    def duck_sample(self, sample: int, key_sample: int, amount_db: float = 12.0, threshold_db: float = -30.0,
                    knee_db: float = 6.0, attack_ms: float = 10.0, hold_ms: float = 50.0, release_ms: float = 300.0,
                    key_first: int = 0, key_gain_db: float = 0.0, rate: Optional[int] = None, **call):
        """Sidechain ducking: `sample` turned down by up to `amount_db` while `key_sample` (a voice-over, a kick) is above
        `threshold_db`: the compress sense, keyed, with an infinite ratio and range_db = -amount_db.  Conversions as in
        compress_sample"""
        table = dynamics_table("compress", threshold_db, np.inf, knee_db, -abs(float(amount_db)))
        return self.dynamics_sample(sample, table, "compress", key_sample=key_sample, key_first=key_first,
                                    key_gain=10.0 ** (float(key_gain_db) / 20.0),
                                    shape=self._dynamics_shape(sample, rate, attack_ms, hold_ms, release_ms), **call)

    def maximize_sample(self, sample: int, target_lufs: float, ceiling_db: float = -1.0, lookahead_ms: float = 1.5,
                        hold_ms: float = 0.0, release_ms: float = 100.0, first_frame: int = 0, n_frames: Optional[int] = None,
                        channels: Optional[int] = None, frames: Optional[int] = None, rate: Optional[int] = None):
        """Loudness maximizing in one pass, no iteration: loudness_sample measures the range, the drive is what takes its
        integrated loudness to `target_lufs`, limit_sample limits the driven range under `ceiling_db`, and loudness_sample
        (with the true peak) measures the result.  Returns (new id, {"loudness": the result's integrated LUFS, "true_peak":
        per channel, linear, "drive_db", "limit": the limiter's statistics}).  Where the limiter has work to do the result
        comes out under the target by what it took away.  A range without an integrated loudness raises WbxError (-4)"""
        frames, channels = self._shape_of(sample, frames, channels)
        if n_frames is None:
            assert frames is not None, "maximize_sample: give n_frames, or frames (the sample's length)"
            n_frames = frames - first_frame
        before = self.loudness_sample(sample, first_frame, n_frames, channels=channels, frames=frames, rate=rate)
        if not np.isfinite(before["integrated"]):
            raise WbxError(-4, "maximize_sample", "the range has no integrated loudness (silent, or shorter than 400 ms)")
        drive_db = float(target_lufs) - before["integrated"]
        new, ls = self.limit_sample(sample, ceiling_db, lookahead_ms, hold_ms, release_ms, drive_db, first_frame, n_frames,
                                    channels=channels, frames=frames, rate=rate)
        if rate is not None:
            self._sample_rate[new] = rate
        after = self.loudness_sample(new, true_peak=True, rate=rate)
        return new, {"loudness": after["integrated"], "true_peak": after["true_peak"], "drive_db": drive_db, "limit": ls}

    def splice_samples(self, channels: int, n_frames: int, parts) -> int:
        """wbx_engine_splice_samples: a new sample of `channels` x `n_frames` frames made of the parts (splice_part(...),
        src_clip = a sample id) — see MixContext.clip_splice.  Every source is pinned against delete_sample for the call's
        life.  May be called while another thread runs process()."""
        new = C.c_uint32()
        _check(self.L.wbx_engine_splice_samples(self.h, channels, n_frames, _part_array(parts), len(parts), C.byref(new)),
               "wbx_engine_splice_samples", self.h, True)
        self._sample_shape[new.value] = (n_frames, channels)
        if parts[0].src_clip in self._sample_rate:
            self._sample_rate[new.value] = self._sample_rate[parts[0].src_clip]
        return new.value

    def join_samples(self, samples, overlap: int = 0, shape="linear", frames=None, channels: Optional[int] = None) -> int:
        """the samples one after the other as ONE new sample, each seam a crossfade of `overlap` frames: the earlier sample's
        last `overlap` frames fade out (`shape`) while the later one's first `overlap` fade in.  Pure host: it builds the
        part list of splice_samples.  `frames`: the samples' lengths where this object did not make them."""
        assert len(samples) >= 1
        lens = [self._shape_of(s, None if frames is None else frames[i], channels)[0] for i, s in enumerate(samples)]
        assert all(n is not None for n in lens), "join_samples: give frames (the samples' lengths)"
        assert all(overlap <= n for n in lens), "join_samples: the overlap is longer than a sample"
        channels = self._shape_of(samples[0], None, channels)[1]
        parts, at = [], 0
        for i, (s, n) in enumerate(zip(samples, lens)):
            parts.append(splice_part(s, 0, n, at, fade_in=overlap if i else 0, fade_out=overlap if i + 1 < len(samples) else 0,
                                     fade_in_shape=shape, fade_out_shape=shape))
            at += n - overlap
        return self.splice_samples(channels, at + overlap, parts)

    def crossfade_samples(self, a: int, b: int, overlap: int, shape="linear", frames=None, channels: Optional[int] = None) -> int:
        """sample `a` crossfading into sample `b` over `overlap` frames as one new sample (join_samples of the two)"""
        return self.join_samples([a, b], overlap, shape, frames, channels)

    def bounce_download(self, sample: int, frames: int) -> np.ndarray:
        """a bounced sample back on the host: [C][frames] fp32 (wbx_clip_download per channel)"""
        return np.stack([self.ctx.clip_download(sample, c, frames, np.float32) for c in range(self.num_output_channels)])

    def transport(self):
        ph, sp, pl = C.c_double(), C.c_double(), C.c_int()
        _check(self.L.wbx_engine_transport(self.h, C.byref(ph), C.byref(sp), C.byref(pl)), "wbx_engine_transport", self.h, True)
        return ph.value, sp.value, bool(pl.value)

    def levels(self) -> np.ndarray:
        n = len(self.tracks)
        out = np.zeros((n, self.num_output_channels), dtype=np.float32)
        _check(self.L.wbx_engine_levels(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), n), "wbx_engine_levels", self.h, True)
        return out

    def fetch_plan_array(self) -> np.ndarray:
        """the whole plan of the last render as a structured array (PLAN_DTYPE), ordered by (block, track, call): what a
        check of blocks deep inside a long render slices (millions of records: no Python list)"""
        n = C.c_size_t()
        self.L.wbx_engine_fetch_plan(self.h, None, 0, C.byref(n))
        buf = np.zeros(max(1, n.value), dtype=PLAN_DTYPE)
        _check(self.L.wbx_engine_fetch_plan(self.h, buf.ctypes.data_as(C.POINTER(_ffi.PlanRecord)), n.value, C.byref(n)),
               "wbx_engine_fetch_plan", self.h, True)
        return buf[:n.value]

    def fetch_plan(self, max_records: Optional[int] = None):
        """The Sampler::stream calls of the last render, ordered by (block, track, call); `max_records` keeps the first
        ones only (the head of a long render)."""
        n = C.c_size_t()
        if max_records is None:
            self.L.wbx_engine_fetch_plan(self.h, None, 0, C.byref(n))
        else:
            n.value = max_records
        arr = (_ffi.PlanRecord * max(1, n.value))()
        _check(self.L.wbx_engine_fetch_plan(self.h, arr, n.value, C.byref(n)), "wbx_engine_fetch_plan", self.h, True)
        got = n.value if max_records is None else min(n.value, max_records)
        return [(r.block, r.track, r.buffer_offset, r.num_samples, r.num_actual, r.sample, r.sample_offset,
                 r.playback_speed, r.gain, r.flags) for r in arr[:got]]


PLAN_DTYPE = np.dtype([("block", "<u4"), ("track", "<u4"), ("buffer_offset", "<u4"), ("num_samples", "<u4"), ("num_actual", "<u4"),
                       ("sample", "<u4"), ("sample_offset", "<f8"), ("playback_speed", "<f8"), ("gain", "<f4"), ("flags", "<u4")])


def plan_rows_of_blocks(plan: np.ndarray, blocks) -> dict:
    """{block: [(track, buffer_offset, num_samples, offset bits, speed bits, gain bits), ...]} of a fetch_plan_array result"""
    out = {}
    for b in blocks:
        lo, hi = np.searchsorted(plan["block"], [b, b + 1])
        p = plan[lo:hi]
        out[int(b)] = list(zip(p["track"].tolist(), p["buffer_offset"].tolist(), p["num_samples"].tolist(),
                               p["sample_offset"].view(np.uint64).tolist(), p["playback_speed"].view(np.uint64).tolist(),
                               p["gain"].view(np.uint32).tolist()))
    return out


def build_engine(spec, max_blocks: int = 8, group_size: int = 0, device: int = 0, device_synth: bool = False,
                 interleaved_ingest: bool = False, spare_tracks: int = 0) -> Engine:
    """Build a product Engine from a synth.SessionSpec through the reference-shaped API."""
    eng = Engine(max(spec.n_tracks, 1) + spare_tracks, spec.block, spec.sample_rate, spec.channels, max_blocks=max_blocks,
                 group_size=group_size, device=device)
    eng.set_bpm(spec.bpm)
    if spec.playhead_start:
        eng.set_playhead_position(spec.playhead_start)
    if spec.n_buses:
        eng.set_buses(spec.n_buses)
    ids = []
    for i, s in enumerate(spec.samples):
        if device_synth:
            ids.append(eng.add_sample_synth(s.fmt, s.channels, s.rate, s.frames, spec.seed, s.seed_track, s.amp))
        else:
            data = [np.ascontiguousarray(a[:s.frames]) for a in spec.sample_data(i)]
            if interleaved_ingest:   # as a decoder would deliver the file: [frames][channels]
                ids.append(eng.add_sample_interleaved(s.fmt, s.rate, np.stack(data, axis=1)))
            else:
                ids.append(eng.add_sample(s.fmt, s.rate, data, s.frames))
    for t in range(spec.n_tracks):
        tr = eng.add_track(f"t{t}")
        tr.set_volume(spec.volumes_db[t])
        tr.set_pan(spec.pans[t])
        if spec.mutes[t]:
            tr.set_mute(True)
        if spec.track_bus is not None:
            tr.set_bus(spec.track_bus[t])
    for c in spec.clips:
        sidx = c.sample if c.sample is not None else c.track
        eng.add_audio_clip(eng.tracks[c.track], "clip", c.min_beat, c.max_beat, c.start_offset, ids[sidx], c.speed, c.gain)
    return eng
