"""Script interface to oracle/_ref/wbref_engine — the reference's OWN clip sequencer and block driver (Track::process_event,
Track::process, Engine::process ... cut out of engine/track.cpp / engine.cpp where they lie and compiled unmodified:
oracle/Makefile, oracle/ref_engine_driver.cpp) — and the same script replayed on the oracle.  Test infrastructure only.

A script is a list of operations; `run` operations process blocks.  The reference answers every non-run operation with a
status: 1 taken, 2 bad argument, 3 quirk Q11 (an inverted range on which the compiled reference's
reserve_track_region dies — the driver predicts it from the reference's own range query and does not enter).  The oracle side
PREDICTS status 3 with its own restatement of the range query, so the prediction is itself compared.  Overlap trimming
(Engine::reserve_track_region, engine_r3b.inc) runs as reference code: no edit is refused for needing it."""
import os
import struct
import subprocess
import tempfile
from typing import List, Optional

import numpy as np

import oracle_ffi as O

EXE = os.path.join(O.ORACLE_DIR, "_ref", "wbref_engine")

CUTS = {   # build output under oracle/_ref/ -> the reference source it must be a verbatim, contiguous region of
    "eng/vu_meter_h_body.inc": "engine/vu_meter.h", "eng/track_h_body.inc": "engine/track.h",
    "eng/audio_record_h_body.inc": "engine/audio_record.h", "eng/engine_h_body.inc": "engine/engine.h",
    "eng/track_cpp_body.inc": "engine/track.cpp",
    "eng/engine_r1.inc": "engine/engine.cpp", "eng/engine_r2.inc": "engine/engine.cpp", "eng/engine_r3.inc": "engine/engine.cpp",
    "eng/engine_r3b.inc": "engine/engine.cpp", "eng/engine_r4.inc": "engine/engine.cpp", "eng/engine_r5.inc": "engine/engine.cpp", "eng/engine_r6.inc": "engine/engine.cpp",
    "eng/assets_r1.inc": "engine/assets_table.cpp", "eng/assets_r2.inc": "engine/assets_table.cpp",
    "eng/assets_r3.inc": "engine/assets_table.cpp", "eng/sample_r1.inc": "dsp/sample.cpp",
    "deinterleave_impl.inc": "dsp/sample.cpp", "mip_impl.inc": "gfx/waveform_visual.cpp", "vu_meter_struct.inc": "engine/vu_meter.h",
}


# the one cut that is a region LESS ONE LINE (oracle/Makefile: the whole-line Log::error("...") statement of reserve_track_region)
CUTS_LESS_ONE_LINE = {"eng/engine_r3b.inc": r'^[ \t]*Log::error\("[^"]*"\);[ \t]*$'}


def cut_region_less_one_line(text: str, whole: str, drop_re: str) -> Optional[tuple]:
    """(first line, last line, dropped line) of the region of `whole` that `text` is byte for byte once the ONE line of that
    region which matches drop_re is left out; None if it is no such region"""
    import re
    src, out = whole.split("\n"), text.split("\n")[:-1]
    if not out:
        return None
    for first in (i for i, l in enumerate(src) if l == out[0]):
        region = src[first:first + len(out) + 1]
        drops = [i for i, l in enumerate(region) if re.match(drop_re, l)]
        if len(drops) == 1 and region[:drops[0]] + region[drops[0] + 1:] == out:
            return first + 1, first + len(out) + 1, first + drops[0] + 1
    return None


def cut_region(text: str, whole: str) -> Optional[tuple]:
    """(first line, last line) of the region of `whole` that the cut `text` is byte for byte; None if it is no such region"""
    at = whole.find(text)
    if at < 0 and whole.endswith(text[:-1]):     # (a region that runs to the end of a file without a final newline: awk adds one)
        at = len(whole) - len(text) + 1
    if at < 0 or not text.strip():
        return None
    first = whole.count("\n", 0, at) + 1
    return first, first + text.count("\n") - 1


def available(build: bool = True) -> bool:
    """is the reference executable there?  build=True (the tests, this container): oracle/Makefile's `ref` target runs first where
    /root/reference exists; build=False (bench.py): the prebuilt file or nothing — a bench run reads nothing of the reference"""
    if build and not O.build_ref():
        return False
    if not os.path.exists(EXE):
        return False
    if not os.access(EXE, os.X_OK):          # (a copy of the tree that dropped the mode bits)
        try:
            os.chmod(EXE, 0o755)
        except OSError:
            return False
    return os.access(EXE, os.X_OK)


class Script:
    """operations as tuples; samples as (fmt, channels, rate, frames, [planar arrays incl. 16 pad frames])"""

    def __init__(self, channels=2, block=512, rate=48000, bpm=120.0):
        self.channels, self.block, self.rate = channels, block, rate
        self.ops = [("cfg", channels, block, rate), ("bpm", float(bpm))]
        self.samples = []

    def add_sample(self, fmt, channels, rate, frames, data, gen=None):
        """gen = (seed, seed_track, amp) of whitebox_amd.synth's keyed generator when the data came from it (fixtures store the
        key, not the audio)"""
        self.samples.append((fmt, channels, rate, frames, data, gen))
        self.ops.append(("sample", len(self.samples) - 1))
        return len(self.samples) - 1

    def op(self, *a):
        self.ops.append(tuple(a))


def script_to_json(s: Script) -> str:
    """ops with their floats as hex strings (exact), samples as generator keys"""
    import json
    def enc(x):
        if isinstance(x, (float, np.floating)):
            return {"f": float(x).hex()}
        return int(x) if isinstance(x, (int, np.integer)) and not isinstance(x, bool) else x
    assert all(smp[5] is not None for smp in s.samples)
    return json.dumps({"channels": s.channels, "block": s.block, "rate": s.rate,
                       "samples": [[smp[0], smp[1], smp[2], smp[3], list(smp[5][:2]) + [float(smp[5][2]).hex()]] for smp in s.samples],
                       "ops": [[enc(x) for x in o] for o in s.ops]})


def script_from_json(text: str) -> Script:
    import json
    from whitebox_amd import synth
    d = json.loads(text)
    s = Script(d["channels"], d["block"], d["rate"])
    s.ops = []
    for fmt, ch, rate, frames, (seed, seed_track, amp) in d["samples"]:
        amp = float.fromhex(amp)
        spec = synth.SessionSpec(name="s", n_tracks=1, seed=seed, samples=[synth.SampleSpec(seed_track, ch, rate, frames, fmt, amp)],
                                 clips=[], volumes_db=[0.0], pans=[0.0], mutes=[False])
        s.samples.append((fmt, ch, rate, frames, spec.sample_data(0), (seed, seed_track, amp)))
    for o in d["ops"]:
        s.ops.append(tuple(float.fromhex(x["f"]) if isinstance(x, dict) else x for x in o))
    return s


def script_from_spec(spec, n_blocks: int) -> Script:
    """a whitebox_amd.synth.SessionSpec (the BASELINE configs, the fuzz generators' sessions ...) as a script: fp32 samples come
    from the driver's own copy of the keyed generator (`synth` operation: no audio in the script or the data file), other
    formats through the data file; clips in list order, as build_oracle_engine / build_engine add them"""
    s = Script(spec.channels, spec.block, spec.sample_rate, spec.bpm)
    for i, smp in enumerate(spec.samples):
        if smp.fmt == "f32":
            s.samples.append(("f32", smp.channels, smp.rate, smp.frames, spec.sample_data(i), (spec.seed, smp.seed_track, smp.amp)))
            s.ops.append(("synth", len(s.samples) - 1))
        else:
            s.add_sample(smp.fmt, smp.channels, smp.rate, smp.frames, spec.sample_data(i), gen=(spec.seed, smp.seed_track, smp.amp))
    for t in range(spec.n_tracks):
        s.op("track")
        s.op("vol", t, float(np.float32(spec.volumes_db[t])))
        s.op("pan", t, float(np.float32(spec.pans[t])))
        if spec.mutes[t]:
            s.op("mute", t, 1)
    for c in spec.clips:
        s.op("clip", c.track, float(c.min_beat), float(c.max_beat), float(c.start_offset),
             c.sample if c.sample is not None else c.track, float(c.speed), float(np.float32(c.gain)))
    if spec.playhead_start:
        s.op("seek", float(spec.playhead_start))
    s.op("play")
    s.op("run", n_blocks)
    return s


def script_from_bus_spec(spec, n_blocks: int) -> Script:
    """a session with sub-buses (extension A13; config 4) for the driver's `bus` / `runbus` operations: one reference Engine per
    bus holding that bus's tracks in track order, the buses added in order — SURVEY A13's composition of reference functions"""
    assert spec.n_buses and spec.track_bus is not None
    s = Script(spec.channels, spec.block, spec.sample_rate, spec.bpm)
    for i, smp in enumerate(spec.samples):
        assert smp.fmt == "f32"
        s.samples.append(("f32", smp.channels, smp.rate, smp.frames, None, (spec.seed, smp.seed_track, smp.amp)))
        s.ops.append(("synth", len(s.samples) - 1))
    for b in range(spec.n_buses):
        s.op("bus", b)
        members = [t for t in range(spec.n_tracks) if spec.track_bus[t] == b]
        local = {t: i for i, t in enumerate(members)}
        for t in members:
            s.op("track")
            s.op("vol", local[t], float(np.float32(spec.volumes_db[t])))
            s.op("pan", local[t], float(np.float32(spec.pans[t])))
            if spec.mutes[t]:
                s.op("mute", local[t], 1)
        for c in spec.clips:
            if c.track in local:
                s.op("clip", local[c.track], float(c.min_beat), float(c.max_beat), float(c.start_offset),
                     c.sample if c.sample is not None else c.track, float(c.speed), float(np.float32(c.gain)))
    s.op("play")
    s.op("runbus", n_blocks)
    return s


def _hx(x: float) -> str:
    return float(x).hex()


def run_reference(s: Script, timeout=60, want_raw=False):
    """-> list of records: ("op", status) | ("run", [block dicts]) | ("clips", [[clip tuples] per track])"""
    blob, offs = bytearray(), []
    synth_ops = {o[1] for o in s.ops if o[0] == "synth"}
    for i, (fmt, ch, rate, frames, data, _g) in enumerate(s.samples):
        offs.append(len(blob))
        if i in synth_ops:
            continue                      # generated by the driver from its key
        for c in range(ch):
            blob += np.ascontiguousarray(data[c][:frames]).tobytes()
    lines = []
    for o in s.ops:
        k = o[0]
        if k == "sample":
            fmt, ch, rate, frames = s.samples[o[1]][:4]
            lines.append(f"sample {O.FMT[fmt]} {ch} {rate} {frames} {offs[o[1]]}")
        elif k == "synth":
            fmt, ch, rate, frames, _d, (seed, kt, amp) = s.samples[o[1]]
            lines.append(f"synth {ch} {rate} {frames} {seed} {kt} {_hx(np.float32(amp))}")
        elif k == "clip":
            _, t, mn, mx, so, si, sp, g = o
            lines.append(f"clip {t} {_hx(mn)} {_hx(mx)} {_hx(so)} {si} {_hx(sp)} {_hx(np.float32(g))}")
        elif k == "gain":
            lines.append(f"gain {o[1]} {o[2]} {_hx(np.float32(o[3]))}")
        elif k == "move":
            lines.append(f"move {o[1]} {o[2]} {_hx(o[3])}")
        elif k == "resize":
            _, t, i, rel, lim, ml, left, shift, stretch = o
            lines.append(f"resize {t} {i} {_hx(rel)} {_hx(lim)} {_hx(ml)} {int(left)} {int(shift)} {int(stretch)}")
        elif k == "delregion":
            lines.append(f"delregion {o[1]} {_hx(o[2])} {_hx(o[3])}")
        elif k == "query":
            lines.append(f"query {o[1]} {_hx(o[2])} {_hx(o[3])}")
        elif k in ("vol", "pan"):
            lines.append(f"{k} {o[1]} {float(np.float32(o[2]))!r}")
        elif k in ("bpm", "seek"):
            lines.append(f"{k} {float(o[1])!r}")
        else:
            lines.append(" ".join(str(x) for x in o))
    with tempfile.TemporaryDirectory() as d:
        sp, dp, rp = (os.path.join(d, n) for n in ("script.txt", "data.bin", "result.bin"))
        open(sp, "w").write("\n".join(lines) + "\n")
        open(dp, "wb").write(bytes(blob))
        r = subprocess.run([EXE, sp, dp, rp], timeout=timeout, capture_output=True)
        if r.returncode != 0:
            raise RuntimeError(f"wbref_engine rc={r.returncode} {r.stderr[-300:]!r}")
        raw = open(rp, "rb").read()
    return (raw, parse_results(raw, s.channels, s.block)) if want_raw else parse_results(raw, s.channels, s.block)


def parse_results(raw: bytes, C: int, F: int):
    """The records of an answer file.  It opens with a layout-version record (2: a clip record ends in a state word), which
    answers no script line and is not handed on.  A file without one comes from an executable built from an earlier driver
    (oracle/_ref travels prebuilt and may be older than the tree): its clip records have no state word and are read so, every
    clip as live — an edit never leaves a marked clip in the list, all of them end in update_clip_ordering."""
    pos, out, version = 0, [], 1

    def u32():
        nonlocal pos
        v = struct.unpack_from("<I", raw, pos)[0]; pos += 4
        return v

    def f64bits():
        nonlocal pos
        v = struct.unpack_from("<Q", raw, pos)[0]; pos += 8
        return v

    while pos < len(raw):
        tag = u32()
        if tag == 0x56455200:
            version = u32()
            assert version == 2, version
        elif tag == 0x4F500000:
            out.append(("op", u32()))
        elif tag == 0x52554E00:
            n, blocks = u32(), []
            for _ in range(n):
                assert u32() == 0x424C4B00
                b = {"block": u32()}
                b["master"] = np.frombuffer(raw, np.uint32, C * F, pos).reshape(C, F).copy(); pos += 4 * C * F
                b["playhead"], b["sample_position"] = f64bits(), f64bits()
                tr = []
                for _t in range(u32()):
                    ev = []
                    for _e in range(u32()):
                        typ, boff = u32(), u32()
                        time, speed, so = f64bits(), f64bits(), f64bits()
                        ev.append((typ, boff, time, speed, so))
                    cur = u32()
                    spd, soff = f64bits(), f64bits()
                    lv = (u32(), u32())
                    tr.append({"events": ev, "current": cur, "speed": spd, "offset": soff, "level": lv})
                b["tracks"] = tr
                blocks.append(b)
            out.append(("run", blocks))
        elif tag == 0x51525900:
            has, first, last = u32(), u32(), u32()
            fo, lo = f64bits(), f64bits()
            out.append(("query", (has, first, last) if has else (0, 0, 0)))
        elif tag == 0x52554200:
            n, nb = u32(), u32()
            blocks = []
            for _ in range(n):
                m = np.frombuffer(raw, np.uint32, C * F, pos).reshape(C, F).copy(); pos += 4 * C * F
                bus = np.frombuffer(raw, np.uint32, nb * C * F, pos).reshape(nb, C, F).copy(); pos += 4 * nb * C * F
                peak = struct.unpack_from("<f", raw, pos)[0]; pos += 4
                blocks.append({"master": m, "buses": bus, "peak": peak, "playhead": f64bits(), "sample_position": f64bits()})
            out.append(("runbus", blocks))
        elif tag == 0x42454E00:
            n, passes = u32(), u32()
            secs = struct.unpack_from("<d", raw, pos)[0]; pos += 8
            cnt = u32()
            head = np.frombuffer(raw, np.float32, cnt, pos).copy(); pos += 4 * cnt
            out.append(("bench", {"blocks": n, "passes": passes, "seconds": secs, "head": head.reshape(-1, C, F)}))
        elif tag == 0x434C5000:
            lists = []
            for _t in range(u32()):
                cl = []
                for _c in range(u32()):
                    mn, mx, so, spd = f64bits(), f64bits(), f64bits(), f64bits()
                    g, ai = u32(), u32()
                    state = u32() if version >= 2 else CLIP_LIVE
                    cl.append((mn, mx, so, spd, g, ai, state))
                lists.append(cl)
            out.append(("clips", lists))
        else:
            raise RuntimeError(f"bad tag {tag:#x} at {pos}")
    return out


CLIP_LIVE = 1          # the state word of a clip record: bit 0 active, bit 1 marked deleted (never left behind by an edit)


def clip_records(clips):
    """[(min, max, start_offset, speed, gain, sample)] of an engine's clip list as the `clips` record writes them (bit patterns;
    what an API hands out is live clips only)"""
    return [(O.f64_bits(a), O.f64_bits(b), O.f64_bits(c), O.f64_bits(d), O.f32_bits(g), s, CLIP_LIVE) for (a, b, c, d, g, s) in clips]


def edit_range(L, prefix, clips, samples, beat_duration, o):
    """(min, max, index of the ignored clip or None) that the edit `o` hands to Track::query_clip_by_range and then to
    reserve_track_region, or None where it asks nothing (engine.cpp: add_to_cliplist :409-440, move_clip :346-351, resize_clip
    :374-379, delete_region :463-464).  clips: [(min, max, start_offset, speed, ...)] floats; the move / resize arithmetic is
    clip_edit.h's, from library L (prefix 'wbo': the oracle's; 'ref': the reference's own, compiled into libwbref.so)"""
    k = o[0]
    if k == "clip":
        mn, mx = o[2], o[3]
        if not clips or clips[-1][1] < mn or clips[0][0] > mx:
            return None
        return mn, mx, None
    if k == "delregion":
        return o[2], o[3], None
    if k not in ("move", "resize") or o[2] >= len(clips) or o[3] == 0.0:
        return None
    c = clips[o[2]]
    d = [O.C.c_double() for _ in range(4)]
    if k == "move":
        getattr(L, prefix + "_calc_move_clip")(c[0], c[1], o[3], 0.0, O.C.byref(d[0]), O.C.byref(d[1]))
    else:
        smp = samples[c[5]]
        getattr(L, prefix + "_calc_resize_clip")(c[0], c[1], c[2], c[3], float(smp[2]), float(smp[3]), o[3], o[4], o[5], c[0],
                                                 beat_duration, int(o[6]), int(o[7]), int(o[8]), 0, *[O.C.byref(x) for x in d])
    return d[0].value, d[1].value, o[2]


def is_q11(clips, query, mx, ignore) -> bool:
    """the statement at engine.cpp:547 with last_clip == 0 in reserve_track_region's multi-clip branch: `last_clip--` wraps"""
    has, first, last = query
    return bool(has) and first != last and last == 0 and ignore != 0 and mx < clips[0][1]


def classify(clips, query, mn, mx, ignore):
    """The outcome class of reserve_track_region (engine.cpp:478-569) for an edit, from the clip list BEFORE the edit (floats),
    the reference's answer to a `query` line over [mn, mx) and the index of the ignored clip: never from oracle or product.
    -> 'free' (no hit) | 'q11' | 'inverted' | single: 'ignored' 'split' 'trim_right' 'trim_left' 'covered' |
    several: 'm:<first><last><interior>' with first / last T trimmed, N not trimmed (deleted), I ignored and interior
    - none, d deleted, i the ignored clip in the interior"""
    has, first, last = query
    if not has:
        return "free"
    if is_q11(clips, query, mx, ignore):
        return "q11"
    if first > last:
        return "inverted"
    if first == last:
        c = clips[first]
        if first == ignore:
            return "ignored"
        if mn > c[0] and mx < c[1]:
            return "split"
        if mn > c[0]:
            return "trim_right"
        if mx < c[1]:
            return "trim_left"
        return "covered"
    f = "I" if first == ignore else ("T" if mn > clips[first][0] else "N")
    l = "I" if last == ignore else ("T" if mx < clips[last][1] else "N")
    inner = "-" if last - first == 1 else ("i" if ignore is not None and first < ignore < last else "d")
    return f"m:{f}{l}{inner}"


def edge_tags(clips, query, mn, mx):
    """which exactly-equal edges the range has: min == a hit clip's min_time, max == a hit clip's max_time, the range touching
    a neighbour that is not hit (max == next.min_time, min == prev.max_time)"""
    has, first, last = query
    tags = set()
    if not has or first > last:
        return tags
    if mn == clips[first][0]:
        tags.add("min==c.min")
    if mx == clips[last][1]:
        tags.add("max==c.max")
    if last + 1 < len(clips) and mx == clips[last + 1][0]:
        tags.add("max==next.min")
    if first > 0 and mn == clips[first - 1][1]:
        tags.add("min==prev.max")
    return tags


class Wrapped(Exception):
    """the session drives the reference into its event_length wrap (track.cpp:669: a write past the block buffer, undefined
    behaviour in the reference) — nothing to compare"""


def _oracle_q11(e, s: Script, o) -> bool:
    """the oracle's own prediction of status 3: its clip list, its restated clip_edit.h and range query"""
    cl = e.clips(o[1])
    r = edit_range(e.L, "wbo", cl, s.samples, e.e.contents.beat_duration, o)
    if r is None:
        return False
    f, l = O.C.c_uint32(), O.C.c_uint32()
    has = e.L.wbo_track_query_clip_by_range(e.e, o[1], O.C.c_double(r[0]), O.C.c_double(r[1]), O.C.byref(f), O.C.byref(l))
    return is_q11(cl, (int(bool(has)), f.value, l.value), r[1], r[2])


def run_oracle(s: Script):
    """the same script on the oracle; same record shapes as run_reference (bit patterns)"""
    e = O.OracleEngine(s.channels, s.block, s.rate)
    e.enable_seglog(True)
    out, block_no = [], 0
    fb = O.f64_bits
    for o in s.ops:
        k, st = o[0], 1
        if k == "cfg":
            pass
        elif k == "bpm":
            e.set_bpm(o[1])
        elif k == "seek":
            e.set_playhead(o[1])
        elif k == "rate":
            e.e.contents.sample_rate = int(o[1])      # Engine::process is handed the new rate (engine.cpp:1576), nothing else changes
        elif k == "play":
            e.play()
        elif k == "stop":
            e.stop()
        elif k in ("sample", "synth"):
            fmt, ch, rate, frames, data = s.samples[o[1]][:5]
            e.add_sample(fmt, ch, rate, frames, data)
        elif k == "track":
            e.add_track()
        elif k == "vol":
            e.set_volume(o[1], o[2])
        elif k == "pan":
            e.set_pan(o[1], o[2])
        elif k == "mute":
            e.set_mute(o[1], o[2])
        elif k == "clip":
            _, t, mn, mx, so, si, sp, g = o
            if _oracle_q11(e, s, o):
                st = 3
            else:
                assert e.add_audio_clip(t, mn, mx, so, si, sp, g) == 0
        elif k == "delclip":
            if o[2] >= len(e.clips(o[1])):
                st = 2
            else:
                e.delete_clip(o[1], o[2])
        elif k == "gain":
            if o[2] >= len(e.clips(o[1])):
                st = 2
            else:
                e.set_clip_gain(o[1], o[2], o[3])
        elif k in ("move", "resize"):
            if o[2] >= len(e.clips(o[1])):
                st = 2
            elif _oracle_q11(e, s, o):
                st = 3
            elif k == "move":
                e.move_clip(o[1], o[2], float(o[3]))
            else:
                e.resize_clip(o[1], o[2], float(o[3]), float(o[4]), float(o[5]), bool(o[6]), bool(o[7]), bool(o[8]))
        elif k == "delregion":
            if _oracle_q11(e, s, o):
                st = 3
            else:
                e.delete_region(o[1], float(o[2]), float(o[3]))
        elif k == "query":
            f, l = O.C.c_uint32(), O.C.c_uint32()
            has = int(bool(e.L.wbo_track_query_clip_by_range(e.e, o[1], O.C.c_double(o[2]), O.C.c_double(o[3]), O.C.byref(f), O.C.byref(l))))
            out.append(("query", (has, f.value, l.value) if has else (0, 0, 0)))
            continue
        elif k == "deltrack":
            e.delete_track(o[1])
        elif k == "movetrack":
            e.move_track(o[1], o[2])
        elif k == "solo":
            e.solo_track(o[1])
        elif k == "run":
            blocks = []
            for _ in range(o[1]):
                m, _b = e.process()
                for sg in e.seglog():
                    if sg[1] + sg[2] > s.block:
                        raise Wrapped()
                nt = e.e.contents.n_tracks
                tr = []
                for t in range(nt):
                    T = e.track(t)
                    ev = [(x.type, x.buffer_offset, fb(x.time), fb(x.speed) if x.type == 2 else 0,
                           int(x.sample_offset) if x.type == 2 else 0) for x in T.events[:T.n_events]]
                    tr.append({"events": ev, "current": T.current_event.type, "speed": fb(T.sampler.playback_speed),
                               "offset": fb(T.sampler.sample_offset), "level": (O.f32_bits(T.level[0]), O.f32_bits(T.level[1]))})
                blocks.append({"block": block_no, "master": m.view(np.uint32).copy(), "playhead": fb(e.playhead),
                               "sample_position": fb(e.sample_position), "tracks": tr})
                block_no += 1
            out.append(("run", blocks))
            continue
        elif k == "clips":
            nt = e.e.contents.n_tracks
            out.append(("clips", [clip_records(e.clips(t)) for t in range(nt)]))
            continue
        else:
            st = 2
        out.append(("op", st))
    e.close()
    return out


CLIP_FIELDS = ("min_time", "max_time", "start_offset", "speed", "gain", "asset", "state")


def compare_clip_lists(ref, got) -> Optional[str]:
    """first difference between two `clips` records ([track][clip] of bit-pattern tuples, in list order), or None: the number of
    tracks, the number of clips of a track, then field by field — one ulp in one field is a difference, and so is the same set
    of clips in another order"""
    if len(ref) != len(got):
        return f"{len(ref)} tracks against {len(got)}"
    for t, (a, b) in enumerate(zip(ref, got)):
        if len(a) != len(b):
            return f"track {t}: {len(a)} clips against {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            for name, u, v in zip(CLIP_FIELDS, x, y):
                if u != v:
                    return f"track {t} clip {i} {name}: {u:#x} against {v:#x}"
    return None


def compare(ref, orc, what="") -> Optional[str]:
    """first difference between two record lists, or None"""
    if len(ref) != len(orc):
        return f"{what}: {len(ref)} records against {len(orc)}"
    for i, (r, o) in enumerate(zip(ref, orc)):
        if r[0] != o[0]:
            return f"{what}: record {i} kinds {r[0]} / {o[0]}"
        if r[0] == "op":
            if r[1] != o[1]:
                return f"{what}: operation {i} status reference {r[1]} oracle {o[1]}"
        elif r[0] == "query":
            if r[1] != o[1]:
                return f"{what}: range query {i}: reference {r[1]} oracle {o[1]}"
        elif r[0] == "clips":
            d = compare_clip_lists(r[1], o[1])
            if d:
                return f"{what}: clip lists differ at record {i}: {d}"
        else:
            for br, bo in zip(r[1], o[1]):
                b = br["block"]
                for key in ("playhead", "sample_position"):
                    if br[key] != bo[key]:
                        return f"{what}: block {b} {key} {br[key]:#x} / {bo[key]:#x}"
                if len(br["tracks"]) != len(bo["tracks"]):
                    return f"{what}: block {b} track count"
                for t, (tr, to) in enumerate(zip(br["tracks"], bo["tracks"])):
                    for key in ("events", "current", "speed", "offset", "level"):
                        if tr[key] != to[key]:
                            return f"{what}: block {b} track {t} {key}: reference {tr[key]} oracle {to[key]}"
                if not np.array_equal(br["master"], bo["master"]):
                    d = np.argwhere(br["master"] != bo["master"])
                    return f"{what}: block {b} master differs at {d[:4].tolist()} ({len(d)} samples)"
    return None


# ---- the outcome classes of overlap trimming (Engine::reserve_track_region) ------------------------------------------------
CALLERS = ("add", "move", "resize_left", "resize_right", "delregion")
SINGLE = ("ignored", "split", "trim_right", "trim_left", "covered")
SEVERAL = tuple(f"m:{f}{l}{i}" for f in "TNI" for l in "TNI" for i in "-di")
GRID = [(c, k) for c in CALLERS for k in SINGLE + SEVERAL]


def unreachable(caller, cls) -> Optional[str]:
    """why no script can make `caller` reach outcome `cls`; None where one can"""
    has_ignore = caller in ("move", "resize_left", "resize_right")
    f, l, inner = (cls[2], cls[3], cls[4]) if cls.startswith("m:") else ("", "", "")
    if not has_ignore and (cls == "ignored" or "I" in (f, l) or inner == "i"):
        return "add_to_cliplist and delete_region pass ignore_clip = nullptr (engine.cpp:454, 468)"
    if f == "I" and l == "I":
        return "one clip cannot be both the first and the last of several hits"
    if inner == "i" and "I" in (f, l):
        return "the one ignored clip is either an end of the hits or interior, not both"
    if inner == "i" and caller == "move":
        return ("a moved clip keeps its length (calc_move_clip, clip_edit.h:10-16): a range that holds all of it between two "
                "other hits would have to be longer than the clip")
    if caller == "resize_right":
        if cls in SINGLE and cls != "ignored":
            return "the new range starts at the clip's own min_time (clip_edit.h:70): a single hit is the clip itself"
        if f != "I" and f:
            return "the new range starts at the clip's own min_time (clip_edit.h:70): the resized clip is the first hit"
    if caller == "resize_left":
        if cls in SINGLE and cls != "ignored":
            return "the new range ends at the clip's own max_time (clip_edit.h:122): a single hit is the clip itself"
        if l != "I" and l:
            return "the new range ends at the clip's own max_time (clip_edit.h:122): the resized clip is the last hit"
    return None


def records_clips(rec):
    """a `clips` record's tracks as float tuples (min, max, start_offset, speed, gain bits, sample, state)"""
    def f(b):
        return struct.unpack("<d", struct.pack("<Q", b))[0]
    return [[(f(c[0]), f(c[1]), f(c[2]), f(c[3]), c[4], c[5], c[6]) for c in tr] for tr in rec]


def edit_classes(s: Script, recs):
    """every edit of a script that has a `clips` and a `query` line in front of it (the `overlap` kind):
    -> [(caller, class, edge tags, status, playing, number of the edit in its run between two blocks)].  The class comes from
    the REFERENCE's records only: the clip list of its last `clips` record and its answer to the `query` line (classify)."""
    out, lists, q, playing, in_row = [], None, None, False, 0
    for o, r in zip(s.ops, recs):
        k = o[0]
        if k == "clips":
            lists = records_clips(r[1])
        elif k == "query":
            q = (o, r[1])
        elif k in ("play", "stop"):
            playing = k == "play"
        elif k == "run":
            in_row = 0
        elif k in ("clip", "move", "resize", "delregion"):
            if q is not None and lists is not None and q[0][1] == o[1]:
                caller = {"clip": "add", "move": "move", "delregion": "delregion"}.get(k) or ("resize_left" if o[6] else "resize_right")
                ignore = o[2] if k in ("move", "resize") else None
                cl = lists[o[1]]
                in_row += 1
                out.append((caller, classify(cl, q[1], q[0][2], q[0][3], ignore), edge_tags(cl, q[1], q[0][2], q[0][3]),
                            r[1], playing, in_row))
            q = None
    return out
