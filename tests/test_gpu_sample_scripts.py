"""Sample life scripts on the device (tests/sample_scripts.py): uploads, derived, normalized, resampled, spliced,
loudness-normalized, filtered, convolved, limited, dynamics-processed, stretched and pitch-shifted samples, recorder takes,
bounces and deletes chained at random in ONE clip pool, with placements, playback, measure, loudness, f0, onsets, tempo,
export and mip-maps in between.  Every feature's own test checks its own result; this one
checks THE OTHERS: after every op every live sample is downloaded and compared bit for bit (uint32 views) with the model —
an extent handed to two clips, or a store past a row, corrupts whoever lies beside the clip a feature test looks at — and
the padding behind every producer's result shows when a clip of another rate plays to its end against the oracle engine,
whose copy of the sample is the model's planes + 16 zeros.  The pool's three figures are checked after every op and are
the starting ones at the end.

A splice's sources are takes, bounces, earlier splices and everything else of one rate; a loudness normalization's gain is
the model's within one spacing (pow's last place) and the fp32 quotient where the ceiling binds, its planes the model's
derive at the gain the product used; a loudness measurement is compared as tests/test_gpu_loudness.py compares one (hop
energies and the true peak bit for bit) and, being a consumer, must leave every sample and the pool alone.  A refused
splice (an i16 source: -3, two rates: -4) or normalization (fewer than 4 hops: -4) returns its status, makes no sample id
and changes nothing; the script often deletes one of its sources next, which a pin left behind would refuse.

The six newer producers (LifeRig.newer_producer) take anybody's result as their source — and a convolution's response and
a dynamics call's key are a second live sample — in sizes around their kernels' tiles, chunks, segments and windows, ending
inside a 16-byte word, back to back on one context whose work buffers (taps, gain-curve tables, positions, carried states)
grow and are reused from call to call.  Each result is compared bit for bit with the feature's model, a limit's and a
dynamics call's statistics and a stretch's and a pitch shift's info exactly; refused ones (an i16 source, response or key:
-3; a response or key of another rate: -4; a stretch beyond 8 n or a ratio beyond 4 : 1: -3; a ratio of 1: -4) as above,
with BOTH samples of a two-source call deleted next.  The consumers f0, onsets and tempo return the model's records (as
64-bit patterns) and info, and leave every sample and the pool alone.

Measured on an MI355X: 1.6 - 2.9 s per case, 30.5 s for the module's sixteen cases of 160 ops (0.84 - 1.7 s and 15.3 s for
twelve of 80 ops before these nine joined; the time is still numpy's twin of the loudness filter; MEASUREMENTS.md "Sample
life scripts"); no time is asserted."""
import ctypes as C

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import loudness_model as LM
import oracle_ffi as O
import record_model as RM
import sample_scripts as SS
import splice_model as SP
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from test_gpu_clipfx import check_stats
from test_gpu_loudness import assert_result, bits64
from test_gpu_export import expected_bytes, expected_stats, same_stats
from test_gpu_record import Rig, input_blocks

pytestmark = pytest.mark.gpu
DT = {"f32": np.float32, "i16": np.int16}
NEW = object()                                              # LifeRig.refused: where the new id's out-parameter goes


class LifeRig(Rig):
    """test_gpu_record.Rig (product engine, record model and oracle engine side by side) with the sample vocabulary on top:
    a second oracle engine with every fader at unity for pre-fader bounces, the contents model, and product / oracle ids of
    every script key."""

    def __init__(self, seed):
        self.spec = synth.make_session("life", SS.TRACKS, n_blocks=8, block=SS.F, sample_rate=SS.RATE, bpm=SS.BPM, seed=0x11FE00 + seed)
        Rig.__init__(self, self.spec, SS.INPUTS, SS.CHUNK, SS.SPARE, check_now=True, collect=True)
        self.tw = O.build_oracle_engine(BU.unity_twin(self.spec))
        self.base = self.eng.ctx.pool_stats()              # right after build_engine
        self.c = SS.Contents()
        self.sid, self.osid, self.pids = {}, {}, {}
        self.n_oracle = len(self.spec.samples)
        for i, s in enumerate(self.spec.samples):           # the session's own samples: bystanders nobody may touch
            self.sid[("base", i)] = sorted(self.eng._sample_shape)[i]
            self.c.put(("base", i), s.fmt, s.rate, [a[:s.frames] for a in self.spec.sample_data(i)])
        self.script_keys = []

    # ---- ids
    def oracle_id(self, key):
        """the oracle engines' copy of a sample: the model's planes + the reference's 16 zero frames, made when first placed"""
        if key not in self.osid:
            fmt, rate, planes = self.c.s[key]
            data = [np.concatenate([p, np.zeros(16, p.dtype)]) for p in planes]
            ids = [e.add_sample(fmt, len(planes), rate, len(planes[0]), data) for e in (self.e, self.tw)]
            assert ids == [self.n_oracle] * 2
            self.n_oracle += 1
            self.osid[key] = ids[0]
        return self.osid[key]

    def _oracle_takes(self, before):
        Rig._oracle_takes(self, before)                     # (the take's sample and clip in self.e, and every check of a take)
        for c in self.m.clips[before:]:
            fr = RM.take_frames(c, self.inputs, self.F)
            data = [np.concatenate([fr[ch], np.zeros(16, np.float32)]) for ch in range(c["channels"])]
            assert self.tw.add_sample("f32", c["channels"], self.spec.sample_rate, fr.shape[1], data) == self.n_oracle
            assert self.tw.add_audio_clip(c["track"], c["args"][1], c["args"][2], 0.0, self.n_oracle, 1.0, 1.0) == 0
            self.n_oracle += 1

    # ---- checks
    def new_sample(self, key, sid, frames, channels, rate):
        assert key in self.c.s and (len(self.c.s[key][2][0]), len(self.c.s[key][2]), self.c.s[key][1]) == (frames, channels, rate)
        self.sid[key] = sid
        self.script_keys.append(key)
        self.check_sample(key)                              # the new sample itself, bit for bit
        if sid in self.eng._sample_shape:                   # (a take's sample is made inside stop_record: not registered here)
            assert self.eng._sample_shape[sid] == (frames, channels) and self.eng._sample_rate.get(sid, rate) == rate, (key, sid)
        if self.c.s[key][0] == "f32":                       # registered length: the frame behind the last one does not exist
            with pytest.raises(W.WbxError):
                self.eng.measure_sample(sid, frames, 1, channels=channels, frames=frames + 1)

    def check_sample(self, key):
        fmt, _, planes = self.c.s[key]
        for ch, want in enumerate(planes):
            got = self.eng.ctx.clip_download(self.sid[key], ch, len(want), DT[fmt])
            bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
            assert bad.size == 0, ("sample", key, "channel", ch, "first wrong byte", int(bad[0]), "of", want.nbytes)

    def check_bystanders(self):
        """EVERY live sample against the model, and the pool's figures"""
        for key in self.c.s:
            self.check_sample(key)
        n, reserved, live = self.eng.ctx.pool_stats()
        assert (n, reserved) == self.base[:2], "the pool grew"
        bounds = [SS.pool_bounds(len(p[0]), len(p), fmt) for key, (fmt, _, p) in self.c.s.items() if not isinstance(key, tuple)]
        lo, hi = self.base[2] + sum(b[0] for b in bounds), self.base[2] + sum(b[1] for b in bounds)
        assert lo <= live <= hi, (lo, live, hi)             # (exact where no clip has 8 granules: lo == hi)

    def clip_index(self, track, sid, lo):
        got = [i for i, ci in enumerate(self.eng.clips(self.eng.tracks[track])) if ci[5] == sid and O.f64_bits(ci[0]) == O.f64_bits(lo)]
        assert len(got) == 1, (track, sid, lo)
        return got[0]

    def same_clip_lists(self):
        for t in range(len(self.eng.tracks)):
            got = [tuple(O.f64_bits(x) for x in ci[:4]) for ci in self.eng.clips(self.eng.tracks[t])]
            for e in (self.e, self.tw):
                assert got == [tuple(O.f64_bits(x) for x in ci[:4]) for ci in e.clips(t)], ("clip list", t)

    # ---- the ops
    def life_op(self, op):
        """-> the status the product returned"""
        k, eng, c = op[0], self.eng, self.c
        try:
            if k == "add":
                _, key, fmt, channels, rate, frames, interleaved, _, _ = op
                c.apply(op)
                planes = c.s[key][2]
                sid = eng.add_sample_interleaved(fmt, rate, np.stack(planes, axis=1)) if interleaved else eng.add_sample(fmt, rate, planes)
                self.new_sample(key, sid, frames, channels, rate)
            elif k == "derive":
                _, key, src, first, n, rev, mode, gain, fi, fo, si, so = op
                c.apply(op)
                sid = eng.derive_sample(self.sid[src], W.edit_desc(first, n, rev, mode, gain, fi, fo, si, so), channels=len(c.s[src][2]))
                self.new_sample(key, sid, n, len(c.s[key][2]), c.s[src][1])
            elif k == "normalize":
                _, key, src, target, first, n = op
                c.apply(op)
                sid, gain = eng.normalize_sample(self.sid[src], target, first, n, channels=len(c.s[src][2]), frames=len(c.s[src][2][0]))
                assert np.float32(gain).tobytes() == np.float32(c.gain).tobytes()
                self.new_sample(key, sid, n, len(c.s[src][2]), c.s[src][1])
            elif k == "resample":
                _, key, src, dst, q, first, n = op
                c.apply(op)
                sid = eng.resample_sample(self.sid[src], dst, q, first, n, channels=len(c.s[src][2]), frames=len(c.s[src][2][0]),
                                          src_rate=c.s[src][1])
                self.new_sample(key, sid, len(c.s[key][2][0]), len(c.s[src][2]), dst)
            elif k == "splice":
                _, key, channels, n_frames, parts, status = op
                ffi = [SP.to_ffi(W, SP.Part(*p)._replace(src=self.sid[p[0]])) for p in parts]
                if status:                                   # refused: the status, and no sample id
                    return self.refused(eng.L.wbx_engine_splice_samples, channels, n_frames, (_ffi.SplicePart * len(ffi))(*ffi), len(ffi))
                c.apply(op)
                sid = eng.splice_samples(channels, n_frames, ffi)
                self.new_sample(key, sid, n_frames, channels, c.s[parts[0][0]][1])
            elif k == "loudnorm":
                _, key, src, target, ceiling, first, n, status = op
                if status:
                    return self.refused(eng.L.wbx_engine_normalize_loudness_sample, self.sid[src], first, n, target, ceiling)
                model, free, top = c.loudnorm_gains(op)
                planes = c.s[src][2]
                sid, gain = eng.normalize_loudness_sample(self.sid[src], target, ceiling, first, n, channels=len(planes), frames=len(planes[0]))
                assert abs(np.float32(gain) - model) <= np.spacing(model), ("gain", gain, model, free, top)   # pow's last place
                if top < free - np.spacing(free):            # the ceiling binds whatever pow's last place: the fp32 quotient
                    assert np.float32(gain).tobytes() == np.float32(top).tobytes(), ("gain under the ceiling", gain, top)
                c.apply_loudnorm(op, np.float32(gain))
                self.new_sample(key, sid, n, len(planes), c.s[src][1])
            elif k == "loudness":
                _, src, true_peak, first, n = op
                _, rate, planes = c.s[src]
                got, E = eng.loudness_sample(self.sid[src], first, n, true_peak=true_peak, energies=True, channels=len(planes),
                                             frames=len(planes[0]), rate=rate)
                want_E = LM.hop_energies(planes, first, n, rate)
                assert E.shape == want_E.shape == (len(planes), n // LM.hop_frames(rate))
                bad = np.flatnonzero(bits64(E).ravel() != bits64(want_E).ravel())
                assert bad.size == 0, ("hop energies", src, bad[:8].tolist(), bad.size)
                assert_result(got, LM.gate(want_E, LM.hop_frames(rate)), ("loudness", src))
                want_peak = LM.true_peak(planes, first, n, rate) if true_peak else [np.float32(0.0)] * len(planes)
                assert got["oversampling"] == (LM.oversampling(rate) if true_peak else 0)
                assert BU.bits(np.array(got["true_peak"], dtype=np.float32)).tolist() == BU.bits(np.array(want_peak, dtype=np.float32)).tolist(), \
                    ("true peak", src, got["true_peak"], want_peak)
            elif k in SS.NEW_PRODUCERS:
                return self.newer_producer(op)
            elif k in SS.CONSUMERS:
                _, rate, planes = c.s[op[1]]
                sid, first, n = self.sid[op[1]], op[-2], op[-1]
                shape = dict(first_frame=first, n_frames=n, channels=len(planes), frames=len(planes[0]))
                got, info = (eng.f0_sample(sid, *op[2:7], **shape) if k == "f0" else
                             eng.onsets_sample(sid, *op[2:8], **shape) if k == "onsets" else eng.tempo_sample(sid, *op[2:9], **shape))
                want, want_info = c.analyse(op)
                # the records as 64-bit patterns (three doubles and two 32-bit counts each), the info exactly
                assert got.dtype == want.dtype and got.shape == want.shape, (k, op[1], got.shape, want.shape)
                bad = np.flatnonzero(got.view(np.uint64).reshape(-1, 4) != want.view(np.uint64).reshape(-1, 4))
                assert bad.size == 0, (k, op[1], "first wrong record", int(bad[0]) // 4, got[int(bad[0]) // 4], want[int(bad[0]) // 4], bad.size)
                assert {f: info[f] for f in want_info} == want_info, (k, op[1], info, want_info)
            elif k == "take":
                _, key, track, kind, index, b0, n, beat = op
                made = len(self.made)
                self.run([("input", track, kind, index, True), ("playhead", beat), ("record",)] +
                         [("block", b0 + b) for b in range(n)] + [("stop_record",), ("stop",), ("input", track, RM.NONE, 0, False)])
                assert self.statuses[-(n + 6):] == [0] * (n + 6) == self.m.statuses[-(n + 6):]
                assert len(self.made) == made + 1
                clip, sid = self.made[-1]
                c.put(key, "f32", SS.RATE, list(RM.take_frames(clip, self.inputs, self.F)))
                self.osid[key] = self.n_oracle - 1           # (_oracle_takes made it, in both oracle engines)
                self.pids[("take", key)] = (track, sid, clip["args"][1])
                assert O.f64_bits(clip["args"][1]) == O.f64_bits(beat) and clip["channels"] == (2 if kind == RM.STEREO else 1)
                self.new_sample(key, sid, n * self.F, clip["channels"], SS.RATE)
            elif k == "bounce":
                _, keys, lo, hi, sources = op
                frames, post, master, _ = BU.oracle_sequence(self.e, self.spec, lo, hi)
                _, pre, _, _ = BU.oracle_sequence(self.tw, self.spec, lo, hi)
                ids, got_frames = eng.bounce(lo, hi, list(sources))
                assert got_frames == frames == int((hi - lo) * (60.0 / SS.BPM) * SS.RATE)
                for key, sid, s in zip(keys, ids, sources):
                    want = master if s[0] == "master" else (pre if s[2] == "pre" else post)[s[1]]
                    c.put(key, "f32", SS.RATE, list(want))
                    self.new_sample(key, sid, frames, 2, SS.RATE)
            elif k == "place":
                _, pid, src, track, lo, hi, start = op
                osid = self.oracle_id(src)
                eng.add_audio_clip(eng.tracks[track], "life", lo, hi, start, self.sid[src], 1.0, 1.0)
                for e in (self.e, self.tw):
                    assert e.add_audio_clip(track, lo, hi, start, osid, 1.0, 1.0) == 0
                self.pids[pid] = (track, self.sid[src], lo)
                self.same_clip_lists()
            elif k == "unplace":
                track, sid, lo = self.pids.pop(op[1])
                i = self.clip_index(track, sid, lo)
                eng.delete_clip(eng.tracks[track], i)
                for e in (self.e, self.tw):
                    assert O.f64_bits(e.clips(track)[i][0]) == O.f64_bits(lo) and e.delete_clip(track, i) == 0
                self.same_clip_lists()
            elif k == "play":
                self.run([("playhead", op[1]), ("play",)] + [("block", None)] * op[2] + [("stop",)])   # master and peaks: check_block
            elif k == "measure":
                _, src, first, n = op
                planes = c.s[src][2]
                got = eng.measure_sample(self.sid[src], first, n, channels=len(planes), frames=len(planes[0]))
                check_stats(got, FX.measure(planes, first, n), n, ("measure", src))
            elif k == "export":
                _, src, fmt, clamp, first, n = op
                planes = [p[first:first + n] for p in c.s[src][2]]
                got, st = eng.export_sample(self.sid[src], fmt, first, n, clamp=clamp, channels=len(planes), frames=len(c.s[src][2][0]))
                assert np.array_equal(got.view(np.uint8), expected_bytes(planes, fmt, clamp)), ("export", src, fmt)
                assert same_stats(st, expected_stats(planes)), ("export stats", src)
            elif k == "mip":
                _, src, quality = op
                fmt, _, planes = c.s[src]
                frames = len(planes[0])
                levels = O.oracle_mip_levels(frames)
                assert levels >= 1 and eng.L.wbx_mip_levels(frames) == levels
                eng.ctx.build_mipmaps(self.sid[src], quality)
                for lv in range(levels):
                    mip = eng.ctx.fetch_mipmap(self.sid[src], lv, len(planes), frames, quality)
                    for ch, p in enumerate(planes):
                        assert np.array_equal(mip[ch], O.oracle_mip(fmt, p, lv, quality)), ("mip", src, lv, ch)
            elif k == "delete":
                eng.delete_sample(self.sid[op[1]])
                c.apply(op)
                del self.sid[op[1]]
            else:
                raise ValueError(op)
        except W.WbxError as ex:
            return ex.status
        return 0

    def newer_producer(self, op):
        """filter, convolve, limit, dynamics, stretch, pitch: (kind, key, src, first, n, ..., status) -> the status.  The
        sample against the feature's model bit for bit (new_sample), the statistics / info beside it exactly; a refused one
        through the C entry point, whose out-parameter must stay untouched"""
        k, key, src, first, n, status = op[0], op[1], op[2], op[3], op[4], op[-1]
        eng, c, L, sid = self.eng, self.c, self.eng.L, self.sid[op[2]]
        planes = c.s[src][2]
        shape = dict(first_frame=first, n_frames=n, channels=len(planes), frames=len(planes[0]))
        info = None
        if k == "filter":
            tail, coef = op[5], np.ascontiguousarray(op[6], dtype=np.float64)
            if status:
                return self.refused(L.wbx_engine_filter_sample, sid, first, n, tail, coef.ctypes.data, len(coef), NEW)
            new = eng.filter_sample(sid, coef, tail, **shape)
        elif k == "convolve":
            _, _, _, _, _, ir, ir_first, taps, out_first, out_frames, gain_db, _ = op
            if status:
                return self.refused(L.wbx_engine_convolve_sample, sid, self.sid[ir], first, n, ir_first, taps, out_first, out_frames,
                                    10.0 ** (gain_db / 20.0), NEW, None)
            new = eng.convolve_sample(sid, self.sid[ir], gain_db, out_first, out_frames, ir_first=ir_first, ir_frames=taps,
                                      ir_channels=len(c.s[ir][2]), ir_length=len(c.s[ir][2][0]), **shape)
        elif k == "limit":
            _, _, _, _, _, ceiling_db, drive_db, A, H, R, _ = op
            if status:
                ls = _ffi.LimitStats()
                return self.refused(L.wbx_engine_limit_sample, sid, first, n, np.float32(10.0 ** (ceiling_db / 20.0)),
                                    10.0 ** (drive_db / 20.0), A, H, R, NEW, C.byref(ls), None)
            new, info = eng.limit_sample(sid, ceiling_db=ceiling_db, drive_db=drive_db, shape=(A, H, R), rate=c.s[src][1], **shape)
        elif k == "dynamics":
            _, _, _, _, _, spec, sense, kkey, key_first, drive, key_gain, makeup, A, H, R, _ = op
            table = np.ascontiguousarray(SS.dyn_table(spec), dtype=np.float64)
            if status:
                ds = _ffi.DynamicsStats()
                return self.refused(L.wbx_engine_dynamics_sample, sid, self.sid[kkey], first, n, key_first, sense, table.ctypes.data,
                                    drive, key_gain, makeup, A, H, R, NEW, C.byref(ds), None)
            new, info = eng.dynamics_sample(sid, table, sense, key_sample=None if kkey is None else self.sid[kkey], key_first=key_first,
                                            drive=drive, key_gain=key_gain, makeup=makeup, shape=(A, H, R), **shape)
        elif k == "stretch":
            _, _, _, _, _, out, N, D, _ = op
            if status:
                si = _ffi.StretchInfo()
                return self.refused(L.wbx_engine_stretch_sample, sid, first, n, out, N, D, C.byref(si), NEW)
            new, info = eng.stretch_sample(sid, out, N, D, **shape)
        else:
            _, _, _, _, _, out, num, den, quality, N, D, _ = op
            if status:
                pi = _ffi.PitchInfo()
                return self.refused(L.wbx_engine_pitch_sample, sid, first, n, out, num, den, quality, N, D, C.byref(pi), NEW)
            new, info = eng.pitch_sample(sid, num, den, out, quality, N, D, **shape)
        c.apply(op)
        if k in ("limit", "dynamics"):                       # the statistics field by field, exactly
            assert info == c.info, (k, key, info, c.info)
        elif info is not None:                               # the info, without its launches
            assert {f: info[f] for f in c.info} == c.info, (k, key, info, c.info)
        self.new_sample(key, new, len(c.s[key][2][0]), len(c.s[key][2]), c.s[src][1])
        return 0

    def refused(self, fn, *args):
        """a producer the product must refuse -> its status; no sample id and no gain came back.  NEW among the arguments
        stands for the new id's out-parameter (where it is not the last one)"""
        new, gain = C.c_uint32(0xFEED), C.c_float(7.0)
        if any(a is NEW for a in args):
            args, tail = [C.byref(new) if a is NEW else a for a in args], ()
        else:
            tail = (C.byref(new), C.byref(gain)) if fn is self.eng.L.wbx_engine_normalize_loudness_sample else (C.byref(new),)
        status = fn(self.eng.h, *args, *tail)
        assert status != 0 and new.value == 0xFEED and gain.value == 7.0, ("a refused producer made a sample", status, new.value)
        return status

    def close(self):
        Rig.close(self)
        self.tw.close()


@pytest.mark.parametrize("seed", SS.SEEDS)
def test_every_sample_outlives_its_neighbours(seed):
    ops, facts = SS.make_script(seed)
    rig = LifeRig(seed)
    rig.inputs = input_blocks(np.random.default_rng(0x11FE + seed), max(facts["input_blocks"], 1), SS.INPUTS, SS.F, special=False)
    try:
        rig.check_bystanders()
        for i, op in enumerate(ops):
            try:
                status = rig.life_op(op)
                assert status == (op[2] if op[0] == "delete" else op[-1] if op[0] in SS.HAVE_A_STATUS else 0), ("status", status)
                rig.check_bystanders()
            except AssertionError as ex:
                raise AssertionError((seed, i, op[:3], ex.args)) from ex
        # everything the script placed and made goes; the pool is what it was after build_engine
        for pid in list(rig.pids):
            assert rig.life_op(("unplace", pid)) == 0
        for key in [k for k in rig.script_keys if k in rig.sid]:
            assert rig.life_op(("delete", key, 0)) == 0
            rig.check_bystanders()
        assert rig.eng.ctx.pool_stats() == rig.base
    finally:
        rig.close()
