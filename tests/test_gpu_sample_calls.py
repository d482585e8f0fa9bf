"""The protocol every wbx_engine_*_sample(s) entry point follows, pinned in ONE table: what an unknown id, a refusing
check, a success and a NULL out-pointer do, whichever operation is asked for.  The operations' own results are their own
tests' business (tests/test_gpu_clipfx.py .. test_gpu_align.py); here each call gets the smallest legal arguments of those
tests on a tiny session — one track, two F32 stereo samples of 4096 frames at 48 kHz and one I16 sample — re-added for
every row.  Every case is a refusal the API defines, or a success.

For each of the twenty entry points (wbx_engine_dynamics_sample twice: with a key sample, and with WBX_DYN_NO_KEY):
  1. an unknown id (and, for a call of two samples, an unknown second one) returns -4 with its exact message;
  2. a call its check refuses returns the check's status — -4 for a range past the clip's end, -3 for an I16 sample (the
     second one, where the call names two) — and every named source can be deleted afterwards: no pin was left;
  3. a success: a producer's new id is the pool's next, registered with the frames, channels and rate the entry point
     states (the frames are also read back from the engine: a range of that length measures, one frame more is refused;
     the rate too: wbx_engine_align_samples refuses two samples of different rates), and the sources can be deleted;
  4. a NULL new_sample (a NULL stats for the measurement) returns -4 with its exact message, and nothing is pinned.
Two calls measure, then derive: their refusal in the middle (a silent range; a range without an integrated loudness)
leaves no pin either."""
import ctypes as C

import numpy as np
import pytest

import whitebox_amd as W
from whitebox_amd import _ffi

pytestmark = pytest.mark.gpu

N, RATE, NOBODY = 4096, 48000, 9999
LOUD = 19200                          # 4 hops of 100 ms at 48 kHz: the shortest range that has an integrated loudness
INVALID, UNSUPPORTED = -4, -3


class Rig:
    """the session, and the pool's next id kept beside it"""

    def __init__(self):
        self.eng = W.Engine(1, buffer_size=128, sample_rate=RATE)
        self.eng.add_track("t")
        self.next = None

    def add(self, fmt, planes):
        sid = self.eng.add_sample(fmt, RATE, planes)
        assert self.next is None or sid == self.next
        self.next = sid + 1
        return sid

    def noise(self, seed, frames=N):
        rng = np.random.default_rng([0x5A3, seed])
        return self.add("f32", [rng.uniform(-0.5, 0.5, frames).astype(np.float32) for _ in range(2)])

    def i16(self):
        rng = np.random.default_rng(0x116)
        return self.add("i16", [rng.integers(-20000, 20000, N).astype(np.int16) for _ in range(2)])

    def error(self):
        return self.eng.L.wbx_engine_last_error(self.eng.h).decode()

    def refused(self, call, status, message=None):
        with pytest.raises(W.WbxError) as err:
            call()
        assert err.value.status == status, (err.value, status)
        if message is not None:
            assert self.error() == message

    def unpinned(self, *ids):
        for k in dict.fromkeys(ids):
            self.eng.delete_sample(k)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.eng.close()


KEPT = {}


def coef():
    """one low-pass stage, as the fp64 words the raw call takes"""
    if "coef" not in KEPT:
        KEPT["coef"] = np.ascontiguousarray(W.filter_design(RATE, "lowpass", 1000.0), dtype=np.float64)
    return KEPT["coef"]


def table():
    if "table" not in KEPT:
        KEPT["table"] = np.ascontiguousarray(W.dynamics_table("compress", -18.0, 4.0), dtype=np.float64)
    return KEPT["table"]


# ---- the table.  call(eng, s, t, n): the entry point on sample s (and t, where it names a second one) over n frames from
# frame 0, through the Python wrapper -> the new id (producers).  shape(n): (frames, channels, rate) of what a producer
# registers.  null(L, h, s, t): the raw call with a NULL new_sample.
def splice_parts(s, t, n):
    return [W.splice_part(s, 0, n, 0), W.splice_part(t, 0, 100, 0)]


ROWS = {
    "export": dict(
        call=lambda e, s, t, n: e.export_sample(s, "i16", 0, n), unknown="export: unknown sample"),
    "measure": dict(
        call=lambda e, s, t, n: e.measure_sample(s, 0, n), unknown="measure_sample: unknown sample",
        null=lambda L, h, s, t: L.wbx_engine_measure_sample(h, s, 0, N, None), null_text="measure_sample: stats is NULL"),
    "derive": dict(
        call=lambda e, s, t, n: e.derive_sample(s, W.edit_desc(0, n)), unknown="derive_sample: unknown sample",
        shape=lambda n: (n, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_derive_sample(h, s, C.byref(W.edit_desc(0, N)), None),
        null_text="derive_sample: new_sample is NULL"),
    "normalize": dict(
        call=lambda e, s, t, n: e.normalize_sample(s, 0.5, 0, n)[0], unknown="normalize_sample: unknown sample",
        shape=lambda n: (n, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_normalize_sample(h, s, 0, N, 0.5, None, None),
        null_text="normalize_sample: new_sample is NULL"),
    "resample": dict(
        call=lambda e, s, t, n: e.resample_sample(s, 44100, "fast", 0, n), unknown="resample_sample: unknown sample",
        shape=lambda n: (W.resample_frames(RATE, 44100, n), 2, 44100),
        null=lambda L, h, s, t: L.wbx_engine_resample_sample(h, s, 0, N, 44100, 0, None),
        null_text="resample_sample: new_sample is NULL"),
    "filter": dict(
        call=lambda e, s, t, n: e.filter_sample(s, coef(), 5, 0, n), unknown="filter_sample: unknown sample",
        shape=lambda n: (n + 5, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_filter_sample(h, s, 0, N, 5, coef().ctypes.data, 1, None),
        null_text="filter_sample: new_sample is NULL"),
    "convolve": dict(
        call=lambda e, s, t, n: e.convolve_sample(s, t, first_frame=0, n_frames=n, ir_first=0, ir_frames=8),
        unknown="convolve_sample: unknown sample", second="convolve_sample: unknown response sample",
        shape=lambda n: (n + 8 - 1, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_convolve_sample(h, s, t, 0, N, 0, 8, 0, N + 7, 1.0, None, None),
        null_text="convolve_sample: new_sample is NULL"),
    "limit": dict(
        call=lambda e, s, t, n: e.limit_sample(s, ceiling_db=-6.0, shape=(8, 0, 100), first_frame=0, n_frames=n)[0],
        unknown="limit_sample: unknown sample", shape=lambda n: (n, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_limit_sample(h, s, 0, N, 0.5, 1.0, 8, 0, 100, None, None, None),
        null_text="limit_sample: new_sample is NULL"),
    "dynamics": dict(
        call=lambda e, s, t, n: e.dynamics_sample(s, table(), "compress", key_sample=t, shape=(8, 0, 100), first_frame=0, n_frames=n)[0],
        unknown="dynamics_sample: unknown sample", second="dynamics_sample: unknown key sample", shape=lambda n: (n, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_dynamics_sample(h, s, t, 0, N, 0, 0, table().ctypes.data,
                                                             1.0, 1.0, 1.0, 8, 0, 100, None, None, None),
        null_text="dynamics_sample: new_sample is NULL"),
    "dynamics_no_key": dict(
        call=lambda e, s, t, n: e.dynamics_sample(s, table(), "compress", shape=(8, 0, 100), first_frame=0, n_frames=n)[0],
        unknown="dynamics_sample: unknown sample", shape=lambda n: (n, 2, RATE)),
    "stretch": dict(
        call=lambda e, s, t, n: e.stretch_sample(s, 4000, 256, 96, 0, n)[0], unknown="stretch_sample: unknown sample",
        shape=lambda n: (4000, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_stretch_sample(h, s, 0, N, 4000, 256, 96, None, None),
        null_text="stretch_sample: new_sample is NULL"),
    "warp": dict(
        call=lambda e, s, t, n: e.warp_sample(s, 4001, [(2000, 2100)], 256, 96, 0, n)[0], unknown="warp_sample: unknown sample",
        shape=lambda n: (4001, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_warp_sample(h, s, 0, N, 4001, None, 0, 256, 96, None, None),
        null_text="warp_sample: new_sample is NULL"),
    "pitch": dict(
        call=lambda e, s, t, n: e.pitch_sample(s, 3, 2, 4000, "fast", 64, 24, 0, n)[0], unknown="pitch_sample: unknown sample",
        shape=lambda n: (4000, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_pitch_sample(h, s, 0, N, 4000, 3, 2, 0, 64, 24, None, None),
        null_text="pitch_sample: new_sample is NULL"),
    "loudness": dict(
        call=lambda e, s, t, n: e.loudness_sample(s, 0, n), unknown="loudness_sample: unknown sample"),
    "f0": dict(
        call=lambda e, s, t, n: e.f0_sample(s, 64, 64, 2, 100, 0.15, 0, n), unknown="f0_sample: unknown sample"),
    "spectrum": dict(
        call=lambda e, s, t, n: e.spectrum_sample(s, t, 32, 2, 64, first_frame=0, n_frames=n),
        unknown="spectrum_sample: unknown sample", second="clip spectrum: unknown basis clip", second_is_basis=True),
    "align": dict(
        call=lambda e, s, t, n: e.align_samples(s, t, -8, 8, n_frames=(n + 7) & ~7, m_frames=N),
        unknown="align_samples: unknown reference sample", second="clip align: unknown clip"),
    "onsets": dict(
        call=lambda e, s, t, n: e.onsets_sample(s, 64, first_frame=0, n_frames=n), unknown="onsets_sample: unknown sample"),
    "tempo": dict(
        call=lambda e, s, t, n: e.tempo_sample(s, 64, 1e-9, 64, 1, 2, 16, first_frame=0, n_frames=n),
        unknown="tempo_sample: unknown sample"),
    "normalize_loudness": dict(
        call=lambda e, s, t, n: e.normalize_loudness_sample(s, -20.0, 0.9, 0, n)[0], unknown="normalize_loudness_sample: unknown sample",
        shape=lambda n: (n, 2, RATE), frames=LOUD,
        null=lambda L, h, s, t: L.wbx_engine_normalize_loudness_sample(h, s, 0, N, -20.0, 0.9, None, None),
        null_text="normalize_loudness_sample: new_sample is NULL"),
    "splice": dict(
        call=lambda e, s, t, n: e.splice_samples(2, n, splice_parts(s, t, n)),
        unknown="clip splice: unknown source clip", second="clip splice: unknown source clip", shape=lambda n: (n, 2, RATE),
        null=lambda L, h, s, t: L.wbx_engine_splice_samples(h, 2, N, (_ffi.SplicePart * 2)(*splice_parts(s, t, N)), 2, None),
        null_text="splice_samples: new_sample is NULL"),
}


def registered(rig, new, frames, rate, probe):
    """what the ENGINE holds for sample `new`: a range of `frames` measures and one frame more is refused; an alignment with
    `probe` (48 kHz) runs where the rates agree and is refused where they differ"""
    eng = rig.eng
    eng.measure_sample(new, 0, frames, channels=2)
    rig.refused(lambda: eng.measure_sample(new, 0, frames + 1, channels=2), INVALID)
    if rate == RATE:
        eng.align_samples(probe, new, 0, 0, n_frames=64, m_frames=64)
    else:
        rig.refused(lambda: eng.align_samples(probe, new, 0, 0, n_frames=64, m_frames=64), UNSUPPORTED,
                    "clip align: the clips' sample rates differ")


@pytest.mark.parametrize("name", list(ROWS))
def test_entry_point_follows_the_protocol(rig, name):
    row, eng = ROWS[name], rig.eng
    n = row.get("frames", N)
    call = row["call"]

    def fresh():
        s = rig.noise(1, n)
        t = rig.add("f32", [W.spectrum_basis(32, [0.1, 0.2])]) if row.get("second_is_basis") else rig.noise(2)
        return s, t

    two = "second" in row

    # 1: an unknown id, and an unknown second one
    s, t = fresh()
    rig.refused(lambda: call(eng, NOBODY, t, n), INVALID, row["unknown"])
    if two:
        rig.refused(lambda: call(eng, s, NOBODY, n), INVALID, row["second"])
    rig.unpinned(s, t)

    # 2: the check refuses a range past the clip's end, and an I16 sample (the second one, where the call names two)
    s, t = fresh()
    rig.refused(lambda: call(eng, s, t, n + 1), INVALID)
    rig.unpinned(s, t)
    if two:
        s, i = rig.noise(1, n), rig.i16()
        rig.refused(lambda: call(eng, s, i, n), UNSUPPORTED)
        rig.unpinned(s, i)
    else:
        i = rig.i16()
        rig.refused(lambda: call(eng, i, i, N), UNSUPPORTED)
        rig.unpinned(i)

    # 3: a success
    s, t = fresh()
    new = call(eng, s, t, n)
    if "shape" in row:
        frames, channels, rate = row["shape"](n)
        assert new == rig.next
        rig.next += 1
        assert eng._sample_shape[new] == (frames, channels) and eng._sample_rate[new] == rate
        registered(rig, new, frames, rate, t)
        rig.unpinned(new)
    rig.unpinned(s, t)

    # 4: a NULL out-pointer
    if "null" in row:
        s, t = fresh()
        assert row["null"](eng.L, eng.h, s, t) == INVALID
        assert rig.error() == row["null_text"]
        rig.unpinned(s, t)


def test_a_refusal_between_the_two_runs_leaves_no_pin(rig):
    """normalize_sample and normalize_loudness_sample measure, decide on the host, then derive under one pin: a silent range
    and a range without an integrated loudness are refused after the measurement, with nothing registered"""
    eng = rig.eng
    silent = rig.add("f32", [np.zeros(N, dtype=np.float32)] * 2)
    rig.refused(lambda: eng.normalize_sample(silent, 0.5, 0, N), INVALID, "normalize_sample: the range is silent, or its peak is not finite")
    rig.unpinned(silent)
    short = rig.noise(3)
    rig.refused(lambda: eng.normalize_loudness_sample(short, -20.0, 0.9, 0, N), INVALID,
                "normalize_loudness_sample: the range has no integrated loudness (silent, or shorter than 4 hops)")
    rig.refused(lambda: eng.normalize_loudness_sample(short, -20.0, -1.0, 0, N), INVALID,
                "normalize_loudness_sample: a negative ceiling, or a NaN")
    assert eng.derive_sample(short, W.edit_desc(0, N)) == rig.next     # the refusals registered nothing
    rig.next += 1
    rig.unpinned(short)


def test_null_engine():
    """every entry point refuses a NULL engine with -4 before it touches anything"""
    L = W.lib()
    assert L.wbx_engine_export_sample(None, 0, 0, 1, 0, 0, None, None) == INVALID
    assert L.wbx_engine_measure_sample(None, 0, 0, 1, None) == INVALID
    assert L.wbx_engine_derive_sample(None, 0, None, None) == INVALID
    assert L.wbx_engine_normalize_sample(None, 0, 0, 1, 0.5, None, None) == INVALID
    assert L.wbx_engine_resample_sample(None, 0, 0, 1, 44100, 0, None) == INVALID
    assert L.wbx_engine_filter_sample(None, 0, 0, 1, 0, None, 1, None) == INVALID
    assert L.wbx_engine_convolve_sample(None, 0, 0, 0, 1, 0, 1, 0, 1, 1.0, None, None) == INVALID
    assert L.wbx_engine_limit_sample(None, 0, 0, 1, 0.5, 1.0, 8, 0, 100, None, None, None) == INVALID
    assert L.wbx_engine_dynamics_sample(None, 0, 0, 0, 1, 0, 0, None, 1.0, 1.0, 1.0, 8, 0, 100, None, None, None) == INVALID
    assert L.wbx_engine_stretch_sample(None, 0, 0, 1, 1, 256, 96, None, None) == INVALID
    assert L.wbx_engine_warp_sample(None, 0, 0, 1, 1, None, 0, 256, 96, None, None) == INVALID
    assert L.wbx_engine_pitch_sample(None, 0, 0, 1, 1, 3, 2, 0, 64, 24, None, None) == INVALID
    assert L.wbx_engine_loudness_sample(None, 0, 0, 1, 0, None, None, 0) == INVALID
    assert L.wbx_engine_f0_sample(None, 0, 0, 1, 64, 64, 2, 100, 0.15, None, 0, None) == INVALID
    assert L.wbx_engine_spectrum_sample(None, 0, 0, 1, 0, 0, 32, 2, 64, None, 0, None) == INVALID
    assert L.wbx_engine_align_samples(None, 0, 0, 64, 0, 0, 64, 0, 0, 0, None, None, 0) == INVALID
    assert L.wbx_engine_onsets_sample(None, 0, 0, 1, 64, 1e-9, 0.3, 0.1, 3, 8, None, 0, None) == INVALID
    assert L.wbx_engine_tempo_sample(None, 0, 0, 1, 64, 1e-9, 64, 1, 2, 16, 0.5, None, 0, None) == INVALID
    assert L.wbx_engine_normalize_loudness_sample(None, 0, 0, 1, -20.0, 0.9, None, None) == INVALID
    assert L.wbx_engine_splice_samples(None, 2, 1, None, 0, None) == INVALID
