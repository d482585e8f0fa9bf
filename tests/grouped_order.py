"""The library's grouped summation order, restated in plain numpy: what a single device computes when a render adds track
groups instead of walking every member list whole.  Its inputs are each track's post-gain block buffer, as the oracle
(wbo_engine_process_tracks) hands them out, so the model needs nothing from the device but the partition.

  partition  build_routing (wbx_runtime.hip): the direct tracks in index order, then the members of bus 0, bus 1, ...; each
             list cut into pieces of G tracks.  G is the context's group_size, 128 by default; a context that renders one
             block per call (max_blocks == 1) with no explicit group_size takes the callback rule (callback_group).
  sum        wbx_sum.h: each group is a running fp32 sum from +0.0 of its members in order; the master is +0.0 + the direct
             groups in order, then + bus 0, + bus 1, ...; bus u is +0.0 + its groups in order; then the compare-based clamp
             of engine.cpp:1627-1636 (NaN passes).

With G >= every member list (one group per list) this IS the reference's order: the model must equal the oracle's master
and bus sums bit for bit, which is what the CPU tests check before any device result is held against it.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

import oracle_ffi as O

DEFAULT_GROUP = 128       # kStage: one staging round of a batch render's workgroup
WHOLE = 1 << 30           # "every member list one group": the reference's order


def callback_group(n_tracks: int) -> int:
    """the group size a max_blocks = 1 context picks for itself (build_routing's callback rule)"""
    return 64 if n_tracks <= 16 else 1 if n_tracks <= 64 else 4 if n_tracks <= 256 else 8 if n_tracks <= 512 else 16


def group_size_of(n_tracks: int, group_size: int = 0, max_blocks: int = 8) -> int:
    """G as wbx_create + build_routing decide it: an explicit group_size wins; otherwise the callback rule on one-block
    contexts and 128 on the others"""
    if group_size:
        return group_size
    return callback_group(n_tracks) if max_blocks == 1 else DEFAULT_GROUP


def member_lists(n_tracks: int, n_buses: int = 0, track_bus: Optional[Sequence[int]] = None) -> List[Tuple[int, List[int]]]:
    """[(bus, tracks)]: the direct list (bus -1) first, then bus 0, 1, ... — a track whose bus is not in [0, n_buses) is direct"""
    direct, per_bus = [], [[] for _ in range(n_buses)]
    for t in range(n_tracks):
        b = track_bus[t] if (n_buses and track_bus is not None and t < len(track_bus)) else -1
        if 0 <= b < n_buses:
            per_bus[b].append(t)
        else:
            direct.append(t)
    return [(-1, direct)] + [(u, per_bus[u]) for u in range(n_buses)]


def partition(n_tracks: int, G: int, n_buses: int = 0, track_bus: Optional[Sequence[int]] = None) -> List[Tuple[int, List[int]]]:
    """[(bus, tracks)] per group, in the order the sums run: every member list cut into pieces of G"""
    out = []
    for bus, members in member_lists(n_tracks, n_buses, track_bus):
        for i in range(0, len(members), G):
            out.append((bus, members[i:i + G]))
    return out


def spec_partition(spec, G: int):
    return partition(spec.n_tracks, G, spec.n_buses, spec.track_bus)


def shape_of(groups) -> Tuple[int, int]:
    """(n_groups, longest group): what wbx_render_order reports for the same partition"""
    return len(groups), max((len(m) for _, m in groups), default=0)


def clamp(m: np.ndarray) -> np.ndarray:
    """engine.cpp:1627-1636: compares, not min / max — NaN passes unchanged"""
    one = np.float32(1.0)
    return np.where(m > one, one, np.where(m < -one, -one, m)).astype(np.float32)


def grouped_sum(tracks: np.ndarray, groups, n_buses: int = 0, do_clamp: bool = True):
    """tracks: [..., T, C, F] fp32 post-gain block buffers (leading axes: blocks).  -> (master [..., C, F], buses [..., n_buses, C, F])
    Every add is one fp32 add, sequential over tracks and groups, vectorised over samples and blocks."""
    tracks = np.asarray(tracks, dtype=np.float32)
    lead, CF = tracks.shape[:-3], tracks.shape[-2:]
    zero = np.zeros(lead + CF, dtype=np.float32)
    master = zero.copy()
    buses = np.zeros(lead + (n_buses,) + CF, dtype=np.float32)
    busacc, cur = None, -1

    def close_bus():
        nonlocal master
        if cur >= 0:
            buses[..., cur, :, :] = busacc
            master = master + busacc

    with np.errstate(all="ignore"):   # (infinities and NaN in the clips are part of what is checked)
        for bus, members in groups:
            g = zero.copy()
            for t in members:
                g = g + tracks[..., t, :, :]
            if bus != cur:
                close_bus()
                busacc, cur = zero.copy(), bus
            if bus < 0:
                master = master + g
            else:
                busacc = busacc + g
        close_bus()
    return (clamp(master) if do_clamp else master), buses


def model_for(spec, tracks: np.ndarray, G: int, do_clamp: bool = True):
    return grouped_sum(tracks, spec_partition(spec, G), spec.n_buses, do_clamp)


# ---- oracle side: the track buffers of K blocks
def oracle_tracks(spec, n_blocks: int, clamp_master: bool = True):
    """-> (master [K][C][F], buses [K][n_buses][C][F] or None, tracks [K][T][C][F]) of the oracle's first n_blocks blocks"""
    e = O.build_oracle_engine(spec)
    e.play()
    ms, bs, ts = [], [], []
    for _ in range(n_blocks):
        m, b, t = e.process_tracks(want_buses=bool(spec.n_buses), clamp=clamp_master)
        ms.append(m)
        bs.append(b)
        ts.append(t)
    e.close()
    return np.stack(ms), (np.stack(bs) if spec.n_buses else None), np.stack(ts)


def render_partition(spec, render_order, group_size: int = 0, max_blocks: int = 8):
    """the partition a render took, from what wbx_render_order reports for it: groups of G, or — reference order — one group
    per member list, which a chained render cuts into workgroup-sized pieces of 128 (the additions are the same).  The
    reported (n_groups, longest group) must be the partition's."""
    n_groups, longest, ref = render_order
    if not ref:
        groups = spec_partition(spec, group_size_of(spec.n_tracks, group_size, max_blocks))
    else:
        groups = spec_partition(spec, WHOLE)
        if n_groups != len(groups):
            groups = spec_partition(spec, DEFAULT_GROUP)
    assert (n_groups, longest) == shape_of(groups), ((n_groups, longest), shape_of(groups))
    return groups


def assert_grouped(m, tracks, G: int, n_buses: int = 0, track_bus=None, bus=None, what=""):
    """one single-device render ([..., C, F]) against the grouped order with groups of G over the oracle's track buffers
    ([..., T, C, F]; T: the tracks as they are now); bus: the device's bus sums, if it fetched them"""
    groups = partition(tracks.shape[-3], G, n_buses, track_bus)
    em, ebus = grouped_sum(tracks, groups, n_buses)
    assert_model(m, em, bus, ebus if (n_buses and bus is not None) else None, what=what)


def oracle_model(spec, n_blocks: int, groups):
    """the oracle's master and the model's over `groups`, block by block — for renders too long to keep every track buffer"""
    e = O.build_oracle_engine(spec)
    e.play()
    om, mm = [], []
    for _ in range(n_blocks):
        m, _, t = e.process_tracks()
        om.append(m)
        mm.append(grouped_sum(t, groups, spec.n_buses)[0])
    e.close()
    return np.stack(om), np.stack(mm)


# ---- interleaved device formats of a planar master (the reference's converters, audio_format_conv.cpp)
FORMATS = {"i16": np.int16, "i24": np.uint8, "i24_x8": np.int32, "i32": np.int32, "f32": np.float32}


def interleaved(master: np.ndarray, fmt: str) -> np.ndarray:
    """master [K][C][F] -> the bytes a render in device format `fmt` leaves (packed 24-bit: zeros where its writer never writes)"""
    K, C, F = master.shape
    L = O.lib()
    out = []
    for b in range(K):
        a = np.zeros(F * C * (3 if fmt == "i24" else 1), FORMATS[fmt])
        src = [np.ascontiguousarray(master[b][c], dtype=np.float32) for c in range(C)]
        getattr(L, "wbo_f32_to_interleaved_" + fmt)(a.ctypes.data, O.planar_ptrs(src), 0, F, C)
        out.append(a)
    return np.concatenate(out).view(np.uint8)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, exp) -> np.ndarray:
    """elementwise: the same fp32 bits, or NaN on both sides (a NaN's payload is the one thing the device does not carry
    over from x86: tests/test_gpu_parity.py test_special_float_values)"""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    return (bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp))


def first_difference(got, exp) -> str:
    """where two fp32 arrays first differ, for assertion messages"""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    d = np.argwhere(~same_bits(got, exp))
    if not len(d):
        return "equal"
    i = tuple(d[0])
    return f"{len(d)} samples differ, first at {i}: {got[i]!r} vs {exp[i]!r}"


def assert_model(got_master, exp_master, got_buses=None, exp_buses=None, what=""):
    """exact bits of the master (and bus sums) against the model"""
    assert np.shape(got_master) == np.shape(exp_master), (what, np.shape(got_master), np.shape(exp_master))
    assert same_bits(got_master, exp_master).all(), (what, "master", first_difference(got_master, exp_master))
    if exp_buses is not None and got_buses is not None:
        assert np.shape(got_buses) == np.shape(exp_buses), (what, np.shape(got_buses), np.shape(exp_buses))
        assert same_bits(got_buses, exp_buses).all(), (what, "buses", first_difference(got_buses, exp_buses))
