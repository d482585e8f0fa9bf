"""wbx_clip_loudness, wbx_engine_loudness_sample and wbx_engine_normalize_loudness_sample on the device.  Hop energies come
back through `hop_energy` and are compared BIT FOR BIT (uint64 views) with tests/loudness_model.py, the numpy twin of the
header's text; every field of the result equals the twin's gate over those energies (powers and counts exactly, the
logarithmic figures within 1e-12: libm's last place is not pinned); the true peak is bit-equal to the twin's.  Shapes are the
smallest at which the kernels can still go wrong: at 8000 Hz (hop 800) ranges of no hop, of the sequential prefix, around the
first block, the first short-term window, a full wave of 64 hops, one lane past it and more than two waves; true-peak ranges
around the filter's half width, its taps and one tile; ranges that start at the clip's frame 0 and ranges that end at its
last frame, inside clips whose frames beside the range are NOT zero."""
import ctypes as C
import math
import threading
import time

import numpy as np
import pytest

import bounce_util as BU
import clipfx_model as FX
import loudness_model as M
import resample_model as RS
import second_pass as SP
import whitebox_amd as W
from whitebox_amd import _ffi, synth
from whitebox_amd.engine import build_engine

pytestmark = pytest.mark.gpu

HOP = 800
LENGTHS = [HOP - 1, HOP, HOP + 1, 3 * HOP, 3 * HOP + 1, 4 * HOP - 1, 4 * HOP, 4 * HOP + 1, 30 * HOP, 63 * HOP, 64 * HOP,
           65 * HOP + 7, 129 * HOP + 7]
FIRSTS = [0, 1, 5, 299]
CLIP_LEN = 129 * HOP + 7 + 299 + 190
OTHER_RATES = {44100: 4410, 22050: 2205, 11025: 1103}
PEAK_LENGTHS = [1, 2, 23, 24, 47, 48, 49, 255, 256, 257, 1500]      # H = 24, T = 48; 256 source frames are one tile at 4x
PEAK_RATES = (48000, 96000)
PEAK_CLIP_LEN = 2100
bits = BU.bits


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def source(channels, rate, n):
    """noise whose level steps every 4000 frames (5 hops at 8000 Hz) through loud, quiet and below-the-gate stretches: both
    gates have work to do"""
    rng = np.random.default_rng(0x10AD + 7 * rate + channels)
    levels = np.array([1.2, 0.3, 1e-4, 0.05, 0.8, 1e-5, 0.01], dtype=np.float64)
    env = levels[(np.arange(n) // 4000) % len(levels)]
    return [(rng.uniform(-1.0, 1.0, n) * env).astype(np.float32) for _ in range(channels)]


def clip_id(channels, rate):
    return 1 + [8000, 11025, 22050, 44100, 48000, 96000, 192000].index(rate) * 2 + (channels - 1)


def matrix_cases():
    """a sparse walk over the axes of the matrix; the asserts below are the coverage asked for"""
    out = []
    for li, n in enumerate(LENGTHS):
        for ch in (1, 2):
            first = CLIP_LEN - n if (li + 2 * ch) % 5 == 0 else FIRSTS[(li + ch) % 4]
            out.append((8000, ch, li, n, first))
    for rate, hop in OTHER_RATES.items():
        out.append((rate, 1 + len(out) % 2, -1, 5 * hop + 3, FIRSTS[len(out) % 4]))
    at8k = [c for c in out if c[0] == 8000]
    hops = {c[3] // HOP for c in at8k}
    assert {c[2] for c in at8k} == set(range(len(LENGTHS))) and {c[1] for c in at8k} == {1, 2}
    assert hops >= {0, 1, 3, 4, 30, 63, 64, 65, 129}              # no hop .. more than two waves
    assert set(FIRSTS) <= {c[4] for c in at8k} and any(c[4] + c[3] == CLIP_LEN for c in at8k)
    assert all(c[4] + c[3] <= CLIP_LEN for c in at8k) and {c[0] for c in out} == {8000} | set(OTHER_RATES)
    assert {c[1] for c in at8k if c[4] == 0} == {1, 2} == {c[1] for c in at8k if c[4] + c[3] == CLIP_LEN}
    return out


CASES = matrix_cases()


@pytest.fixture(scope="module")
def ctx():
    c = W.MixContext(4, block=128)
    c.src = {}
    for rate, n in [(8000, CLIP_LEN)] + [(r, 5 * h + 3 + 299 + 50) for r, h in OTHER_RATES.items()] + \
            [(r, PEAK_CLIP_LEN) for r in PEAK_RATES + (192000,)]:
        for ch in (1, 2):
            c.src[(ch, rate)] = source(ch, rate, n)
            c.clip_upload(clip_id(ch, rate), "f32", rate, c.src[(ch, rate)])
    yield c
    c.close()


def assert_result(got, want, what):
    for k in M.FIELDS_EXACT:
        assert (bits64(got[k]) == bits64(want[k])) if k == "gated_power" else got[k] == want[k], (what, k, got[k], want[k])
    for k in M.FIELDS_LUFS:
        g, w = got[k], want[k]
        assert (g == w) if math.isinf(w) or math.isinf(g) else abs(g - w) <= 1e-12, (what, k, g, w)


# ---- 1: hop energies and the full result ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_hop_energies_and_every_field(ctx, case):
    rate, ch, _, n, first = case
    planes = ctx.src[(ch, rate)]
    assert first + n <= len(planes[0])
    want_E = M.hop_energies(planes, first, n, rate)
    got, E = ctx.clip_loudness(clip_id(ch, rate), ch, rate, first, n, energies=True)
    assert E.shape == want_E.shape == (ch, n // M.hop_frames(rate))
    bad = np.flatnonzero(bits64(E).ravel() != bits64(want_E).ravel())
    assert bad.size == 0, (case, bad[:8], bad.size)
    want = M.gate(want_E, M.hop_frames(rate))
    print(case, {k: want[k] for k in ("integrated", "blocks", "blocks_gated", "range_lu")})
    assert_result(got, want, case)
    assert_result(got, W.loudness_gate(E, M.hop_frames(rate)), (case, "the library's own gate"))
    assert got["oversampling"] == 0 and all(p == 0.0 for p in got["true_peak"])
    if n < 4 * M.hop_frames(rate):
        assert got["blocks"] == 0 and got["integrated"] == -math.inf
    assert ctx.clip_loudness(clip_id(ch, rate), ch, rate, first, n) == got      # hop_energy is optional


def test_the_matrix_exercises_both_gates(ctx):
    """the longest range of the matrix drops blocks at the absolute gate AND at the relative one"""
    E = M.hop_energies(ctx.src[(2, 8000)], 0, 129 * HOP + 7, 8000)
    want = M.gate(E, HOP)
    z = np.array([E[:, j:j + 4].sum() / (4 * HOP) for j in range(126)])
    below_abs = int(np.count_nonzero(z <= M.ABS_GATE))
    assert want["blocks"] == 126 and below_abs > 0 and want["blocks_gated"] > 0
    assert 126 - below_abs - want["blocks_gated"] > 0 and want["range_lu"] > 0.0


# ---- 2: true peak -----------------------------------------------------------------------------------------------------------
def peak_cases():
    out = []
    for rate in PEAK_RATES:
        for li, n in enumerate(PEAK_LENGTHS):
            ch = 1 + (li + (rate == 96000)) % 2
            first = PEAK_CLIP_LEN - n if li % 4 == 3 else FIRSTS[(li + ch) % 4]
            out.append((rate, ch, n, first))
    assert {(c[0], c[2]) for c in out} == {(r, n) for r in PEAK_RATES for n in PEAK_LENGTHS}
    assert {(c[0], c[1]) for c in out} == {(r, ch) for r in PEAK_RATES for ch in (1, 2)}
    assert any(c[3] == 0 for c in out) and any(c[3] + c[2] == PEAK_CLIP_LEN for c in out)
    return out


@pytest.mark.parametrize("case", peak_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_true_peak_equals_the_model(ctx, case):
    rate, ch, n, first = case
    planes = ctx.src[(ch, rate)]
    want = M.true_peak(planes, first, n, rate)
    got = ctx.clip_loudness(clip_id(ch, rate), ch, rate, first, n, true_peak=True)
    assert got["oversampling"] == M.oversampling(rate) == (4 if rate == 48000 else 2)
    assert bits(np.array(got["true_peak"], dtype=np.float32)).tolist() == bits(np.array(want, dtype=np.float32)).tolist(), (got, want)
    sample_peak = [np.max(np.abs(p[first:first + n])) for p in planes]
    assert all(t >= s for t, s in zip(got["true_peak"], sample_peak))
    assert got["hops"] == 0 and got["integrated"] == -math.inf


@pytest.mark.parametrize("channels", [1, 2])
def test_true_peak_at_192000_is_the_sample_peak(ctx, channels):
    first, n = 5, PEAK_CLIP_LEN - 9
    got = ctx.clip_loudness(clip_id(channels, 192000), channels, 192000, first, n, true_peak=True)
    st = ctx.clip_measure(clip_id(channels, 192000), channels, first, n)
    assert got["oversampling"] == 1 and got["true_peak"] == st["peak"] and all(p > 0 for p in st["peak"])
    assert got["true_peak"] == M.true_peak(ctx.src[(channels, 192000)], first, n, 192000)


# ---- 2b: the second pass of true_peak_kernel's grid -------------------------------------------------------------------------
PAD = 64                                                        # frames of silence kept around a burst: more than H = 24


def burst_material(n, seam):
    """stereo silence with three noise bursts per channel: inside tile 0, straddling source frame `seam` (the first of the
    second pass), ending on the last frame.  Channel 0's loudest lies on the seam burst's second-pass side, channel 1's in
    tile 0; (planes, the bursts' [a, b) per channel)"""
    rng = np.random.default_rng(0x7EA4)
    planes = [np.zeros(n, dtype=np.float32) for _ in range(2)]
    spans = [[(40, 140), (seam - 50, seam + 50), (n - 60, n)], [(60, 160), (seam - 40, seam + 60), (n - 70, n)]]
    amps = [[0.4, None, 0.5], [0.9, 0.4, 0.5]]
    for p, sp, am in zip(planes, spans, amps):
        for (a, b), amp in zip(sp, am):
            p[a:b] = rng.uniform(-1.0, 1.0, b - a) * (amp if amp is not None else np.where(np.arange(a, b) < seam, 0.3, 0.9))
    return planes, spans


def peak_over_windows(plane, first, n, spans):
    """the model's true peak of the range [first, first + n) of a plane that is silent outside `spans`: the maximum over
    windows of PAD frames around each burst, cut to the range.  A zero frame adds nothing to any output, and none lies within
    H frames of a window's ends (tests/test_loudness_host.py holds the model to that)"""
    best = np.float32(0.0)
    for a, b in spans:
        w0, w1 = max(first, a - PAD), min(first + n, b + PAD)
        if w1 > w0:
            best = max(best, M.true_peak([plane[w0:w1]], 0, w1 - w0, SP.TRUE_PEAK_RATE)[0])
    return best


def test_true_peak_of_tiles_past_the_grid_cap():
    """48000 Hz, factor 4: G tiles and 767 frames (tests/second_pass.py, from wbx_true_peak_launch_shape), so workgroups 0, 1 and
    2 take a second tile; `off` / `row` are computed once outside the tile loop and the lane maxima live across it.  Channel
    0's peak is found only by the second pass; channel 1's is workgroup 0's FIRST tile's and must survive its second (for
    that channel removing the second-pass bursts cannot change the expected value — its part is to show that the running
    maximum is not reset between the iterations; the assertion about removal is made where it can hold, on channel 0)"""
    n, sh, G, tile_frames = SP.true_peak_case()
    seam = G * tile_frames
    assert sh["n_tiles"] == G + 3 > sh["grid"] == G and n - seam == 767
    planes, spans = burst_material(n, seam)
    rate = SP.TRUE_PEAK_RATE
    want = [peak_over_windows(p, 0, n, s) for p, s in zip(planes, spans)]
    # on the CPU, through the model alone: what each channel's figure depends on
    cut = [p.copy() for p in planes]
    for p in cut:
        p[seam:] = 0.0
    without = [peak_over_windows(p, 0, n, s) for p, s in zip(cut, spans)]
    assert without[0] < want[0] and without[1] == want[1]
    assert want[1] == peak_over_windows(planes[1], 0, n, spans[1][:1]) > peak_over_windows(planes[1], 0, n, spans[1][1:])
    a, b = spans[0][1]
    up = RS.resample([planes[0][a - PAD:b + PAD]], 0, b - a + 2 * PAD, rate, 4 * rate, RS.GOOD)[0]
    at = 4 * (a - PAD) + int(np.argmax(np.abs(up)))
    assert np.abs(up).max() == want[0] and at >= G * 1024 + 4 * 24, "channel 0's peak is an output of the second pass alone"
    assert want[0] > max(np.abs(planes[0]).max(), 0.9), "an inter-sample peak"

    c = W.MixContext(4, block=128)
    c.clip_upload(1, "f32", rate, planes)
    c.clip_upload(2, "f32", rate, planes[:1])
    got = c.clip_loudness(1, 2, rate, 0, n, true_peak=True)
    assert got["oversampling"] == 4
    assert bits(np.array(got["true_peak"], dtype=np.float32)).tolist() == bits(np.array(want, dtype=np.float32)).tolist(), (got, want)
    mono = c.clip_loudness(2, 1, rate, 0, n, true_peak=True)
    assert bits(np.float32(mono["true_peak"][0])) == bits(np.float32(want[0])), (mono, want)
    # the range from frame 3 on: every tile moves by three source frames, the last still ragged
    first = 3
    assert W.true_peak_launch_shape(rate, n - first) == sh
    want3 = [peak_over_windows(p, first, n - first, s) for p, s in zip(planes, spans)]
    got3 = c.clip_loudness(1, 2, rate, first, n - first, true_peak=True)
    assert bits(np.array(got3["true_peak"], dtype=np.float32)).tolist() == bits(np.array(want3, dtype=np.float32)).tolist(), (got3, want3)
    c.close()


# ---- 3: one known answer per family -----------------------------------------------------------------------------------------
def test_ebu_3341_case_5_on_the_device(ctx):
    rate = 48000
    t = np.arange(int(60.1 * rate), dtype=np.float64)
    level = np.where((t >= 20 * rate) & (t < 40.1 * rate), 10.0 ** (-20 / 20.0), 10.0 ** (-26 / 20.0))
    x = (level * np.sin(2.0 * np.pi * 1000.0 * t / rate)).astype(np.float32)
    ctx.clip_upload(40, "f32", rate, [x, x])
    got = ctx.clip_loudness(40, 2, rate, 0, len(x))
    print("EBU 3341 case 5 on the device: %.4f LUFS" % got["integrated"])
    assert abs(got["integrated"] - -23.0) <= 0.1
    assert got["hops"] == 601 and got["blocks"] == 598
    assert ctx.L.wbx_clip_free(ctx.h, 40) == 0


def test_true_peak_of_a_faded_quarter_rate_sine(ctx):
    """fs / 4 at 45 degrees: every sample is +-0.7071 while the wave between them reaches 1.0"""
    rate, n, fade = 48000, 4800, 480
    k = np.arange(n, dtype=np.float64)
    env = np.minimum(1.0, np.minimum(k, n - 1 - k) / fade)
    x = (env * np.sin(2.0 * np.pi * k / 4.0 + np.pi / 4.0)).astype(np.float32)
    want = M.true_peak([x], 0, n, rate)[0]
    print("faded fs/4 sine: sample peak %.6f, true peak of the model %.7f (%.4f dB)" % (np.max(np.abs(x)), want, 20 * math.log10(want)))
    assert abs(20.0 * math.log10(float(want))) <= 0.01
    assert abs(float(np.max(np.abs(x))) - 0.7071) <= 1e-4
    ctx.clip_upload(41, "f32", rate, [x])
    got = ctx.clip_loudness(41, 1, rate, 0, n, true_peak=True)
    assert bits(np.float32(got["true_peak"][0])) == bits(np.float32(want))
    assert ctx.L.wbx_clip_free(ctx.h, 41) == 0


def test_a_nan_sample_enters_as_zero(ctx):
    n = 6 * HOP
    x = source(2, 8000, n)
    y = [p.copy() for p in x]
    for p, q in zip(x, y):
        p[[7, 1900, n - 1]] = np.nan
        q[[7, 1900, n - 1]] = 0.0
    ctx.clip_upload(42, "f32", 8000, x)
    ctx.clip_upload(43, "f32", 8000, y)
    a, Ea = ctx.clip_loudness(42, 2, 8000, 0, n, true_peak=True, energies=True)
    b, Eb = ctx.clip_loudness(43, 2, 8000, 0, n, true_peak=True, energies=True)
    assert np.array_equal(bits64(Ea), bits64(Eb)) and np.array_equal(bits64(Ea), bits64(M.hop_energies(y, 0, n, 8000)))
    assert_result(a, b, "nan")
    assert bits(np.array(a["true_peak"], dtype=np.float32)).tolist() == bits(np.array(M.true_peak(x, 0, n, 8000), dtype=np.float32)).tolist()
    for i in (42, 43):
        assert ctx.L.wbx_clip_free(ctx.h, i) == 0


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_device(ctx):
    L = W.lib()
    s2 = clip_id(2, 8000)
    ctx.clip_upload(60, "i16", 8000, [np.arange(4000, dtype=np.int16)] * 2)
    ctx.clip_upload(61, "f32", 7999, [np.ones(4000, dtype=np.float32)])
    ctx.clip_upload(62, "f32", 384001, [np.ones(4000, dtype=np.float32)])
    ctx.clip_synth(63, "f32", 1, 48000, 540_000_000, 7, 0, 0.5)  # 4 x 540e6 >= 2^31 - 16
    st = _ffi.Loudness()
    E = np.full(2 * 5, 7.0)

    def refused(status, clip, first, n, flags, out=st, energy=None, cap=0):
        before = ctx.pool_stats()
        got = L.wbx_clip_loudness(ctx.h, clip, first, n, flags, C.byref(out) if out is not None else None,
                                  energy.ctypes.data if energy is not None else None, cap)
        assert got == status, (got, status, clip, first, n, flags, L.wbx_last_error(ctx.h))
        assert ctx.pool_stats() == before and np.all(E == 7.0)

    refused(-4, 999, 0, 4000, 0)                                # unknown clip
    refused(-4, s2, 0, 4000, 0, out=None)                       # NULL out
    refused(-4, s2, 0, 0, 0)                                    # no frames
    refused(-4, s2, CLIP_LEN - 10, 11, 0)                       # past the clip
    refused(-4, s2, CLIP_LEN + 1, 1, 0)
    refused(-4, s2, 0, 4000, 2)                                 # unknown flag
    refused(-4, s2, 0, 4000, 0, energy=E, cap=9)                # 2 x 5 hops need 10 doubles
    refused(-3, 60, 0, 4000, 0)                                 # not F32 (a clip of more than 2 channels cannot exist in the pool)
    refused(-3, 61, 0, 4000, 0)                                 # rates outside 8000 .. 384000
    refused(-3, 62, 0, 4000, 0)
    refused(-3, 63, 0, 540_000_000, 1)                          # the oversampled range would have 2^31 - 16 frames or more
    assert L.wbx_clip_loudness(ctx.h, s2, 0, 4000, 0, C.byref(st), E.ctypes.data, 10) == 0 and st.hops == 5 and not np.any(E == 7.0)
    for i in (60, 61, 62, 63):
        assert L.wbx_clip_free(ctx.h, i) == 0


# ---- 5: through the engine: normalize to a loudness target --------------------------------------------------------------------
def download(c, clip, channels, n):
    return [c.clip_download(clip, k, n, np.float32) for k in range(channels)]


def test_normalize_to_a_target_and_under_a_ceiling():
    rate, n = 8000, 12 * HOP + 5
    spec = synth.make_session("loudnorm", 2, n_blocks=2, block=128, seed=0x10AD01)
    eng = build_engine(spec, max_blocks=2)
    planes = source(2, rate, n + 40)
    src = eng.add_sample("f32", rate, planes)
    first = 20
    want = M.measure(planes, first, n, rate, M.TRUE_PEAK)
    got = eng.loudness_sample(src, first, n, true_peak=True)
    assert_result(got, want, "engine")
    assert bits(np.array(got["true_peak"], dtype=np.float32)).tolist() == bits(np.array(want["true_peak"], dtype=np.float32)).tolist()

    def check(target, ceiling):
        new, gain = eng.normalize_loudness_sample(src, target, ceiling, first_frame=first, n_frames=n)
        g_model = M.normalize_gain(want["integrated"], target, ceiling, want["true_peak"])
        assert abs(np.float32(gain) - g_model) <= np.spacing(g_model), (gain, g_model)      # pow's last place
        derived = FX.derive(planes, first, n, gain=np.float32(gain))
        assert eng._sample_shape[new] == (n, 2)
        assert bits(np.stack(download(eng.ctx, new, 2, n))).tolist() == bits(np.stack(derived)).tolist()
        again = eng.loudness_sample(new, true_peak=True)
        return gain, g_model, again

    gain, _, again = check(-23.0, 0.0)
    print("normalized to -23 LUFS: gain %.6f, re-measured %.5f" % (gain, again["integrated"]))
    assert abs(again["integrated"] - -23.0) <= 0.01
    ceiling = 0.25
    free = M.normalize_gain(want["integrated"], -10.0)
    assert free * max(want["true_peak"]) > ceiling * 1.5, "the ceiling would not bind: the case checks nothing"
    gain, g_model, again = check(-10.0, ceiling)
    assert np.float32(gain) == g_model == np.float32(ceiling) / np.float32(max(want["true_peak"]))
    print("ceiling %.3f: gain %.6f, true peak of the result %.7f" % (ceiling, gain, max(again["true_peak"])))
    assert max(again["true_peak"]) <= ceiling * (1.0 + 2.0 ** -22)
    assert again["integrated"] < -10.0
    # refusals create no sample: a silent range, one shorter than 4 hops, a negative ceiling
    silent = eng.add_sample("f32", rate, [np.zeros(8 * HOP, dtype=np.float32)] * 2)
    L, new, g = W.lib(), C.c_uint32(12345), C.c_float(7.0)
    before = eng.ctx.pool_stats()
    assert L.wbx_engine_normalize_loudness_sample(eng.h, silent, 0, 8 * HOP, -23.0, 0.0, C.byref(new), C.byref(g)) == -4
    assert L.wbx_engine_normalize_loudness_sample(eng.h, src, 0, 4 * HOP - 1, -23.0, 0.0, C.byref(new), C.byref(g)) == -4
    assert L.wbx_engine_normalize_loudness_sample(eng.h, src, 0, n, -23.0, -1.0, C.byref(new), C.byref(g)) == -4
    assert L.wbx_engine_normalize_loudness_sample(eng.h, 9999, 0, n, -23.0, 0.0, C.byref(new), C.byref(g)) == -4
    assert new.value == 12345 and g.value == 7.0 and eng.ctx.pool_stats() == before
    assert eng.loudness_sample(silent)["integrated"] == -math.inf
    eng.close()


# ---- 6: beside the audio thread ---------------------------------------------------------------------------------------------
def test_loudness_beside_the_audio_thread():
    """The shape of the conversions' test (test_gpu_resample.py): a clip far behind the played range names the big sample
    while the threads run, so a delete of it can never succeed — between two measurements it is refused for the clip (-4),
    inside one for the pin (-3, asked first) — one thread deletes without pause while the other measures until a refusal for
    the pin has been seen.  The master is what it is without the measurements."""
    NB, FR, WAIT, CALLS = 300, 1 << 20, 60.0, 64
    spec = synth.make_session("loudthr", 2, n_blocks=NB, block=128, seed=0x10AD12)
    rng = np.random.default_rng(33)
    planes = [rng.uniform(-1.0, 1.0, FR).astype(np.float32) for _ in range(2)]

    def with_big(eng):                                            # the same session in both runs
        sid = eng.add_sample("f32", 44100, planes)
        eng.add_audio_clip(eng.tracks[0], "far", 1000.0, 1001.0, 0.0, sid, 1.0, 1.0)
        return sid

    def run_blocks(eng, sink):
        out = W.AudioBuffer(spec.block, spec.channels)
        eng.play()
        for _ in range(NB):
            eng.process(None, out, float(spec.sample_rate))
            sink.append(np.stack(out.channel_buffers).copy())

    alone = []
    ref = build_engine(spec, max_blocks=1)
    with_big(ref)
    run_blocks(ref, alone)
    ref.close()

    eng = build_engine(spec, max_blocks=1)
    big = with_big(eng)
    first, n = 5, FR - 8
    L = W.lib()
    began, finished, refused = threading.Event(), threading.Event(), threading.Event()
    heard, seen, results = [], {}, {"calls": 0}

    def deleter():
        if not began.wait(WAIT):
            return
        end = time.monotonic() + WAIT
        while not finished.is_set() and time.monotonic() < end:
            st = L.wbx_engine_delete_sample(eng.h, big)
            key = (st, bytes(L.wbx_engine_last_error(eng.h)) if st else b"")
            seen[key] = seen.get(key, 0) + 1
            if st == -3:
                refused.set()

    def editor():
        try:
            began.set()
            while results["calls"] < CALLS and not refused.is_set():
                results["big"] = eng.loudness_sample(big, first, n, true_peak=True, energies=True, channels=2, rate=44100)
                results["calls"] += 1
        finally:
            began.set()
            finished.set()

    threads = [threading.Thread(target=f, args=a) for f, a in ((run_blocks, (eng, heard)), (deleter, ()), (editor, ()))]
    for th in threads:
        th.start()
    for th in threads:
        th.join(WAIT)
    assert not any(th.is_alive() for th in threads), "a thread did not finish in time"
    assert len(heard) == NB and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(heard, alone))
    print("loudness calls", results["calls"], "deletes", {k: v for k, v in seen.items()})
    pinned = [k for k in seen if k[0] == -3]
    assert pinned and all(b"being edited" in m for _, m in pinned), seen
    assert all(st == -3 or (st == -4 and b"still referenced" in m) for st, m in seen), seen
    # every measurement read a live source: the result is the model's
    got, E = results["big"]
    want_E = M.hop_energies(planes, first, n, 44100)
    assert np.array_equal(bits64(E), bits64(want_E))
    assert_result(got, M.gate(want_E, 4410), "beside the audio thread")
    # afterwards: no pin is left (the clip is what refuses now), and with the clip gone the delete succeeds
    assert L.wbx_engine_delete_sample(eng.h, big) == -4 and b"still referenced" in L.wbx_engine_last_error(eng.h)
    eng.delete_clip(eng.tracks[0], len(eng.clips(eng.tracks[0])) - 1)
    assert L.wbx_engine_delete_sample(eng.h, big) == 0
    st = _ffi.Loudness()
    assert L.wbx_engine_loudness_sample(eng.h, big, 0, 8000, 0, C.byref(st), None, 0) == -4
    eng.close()
