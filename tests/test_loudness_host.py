"""Measuring a clip's loudness, the part that needs no device: the symbols and the struct of include/wbx.h "Measuring a
clip's loudness" exist and match their binding twins, the adapter's methods compile, the library's K-filter coefficients equal
the numpy twin (tests/loudness_model.py) BIT FOR BIT, a math.tan rendering within 4 ulps and the standard's table to its 14
decimals, the library's gate equals the twin's in every power and count — and the twin is a meter, not merely
self-consistent: the EBU Tech 3341 and 3342 signals come out at the values those documents ask for."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import loudness_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_loudness_hop_frames", "wbx_loudness_hops", "wbx_loudness_coefficients", "wbx_loudness_gate", "wbx_true_peak_launch_shape",
       "wbx_clip_loudness",
       "wbx_engine_loudness_sample", "wbx_engine_normalize_loudness_sample"]
RATES = (8000, 11025, 22050, 44100, 48000, 96000, 192000)
FIELDS = ["integrated", "gated_power", "momentary_max", "short_term_max", "range_lu", "true_peak", "hops", "blocks",
          "blocks_gated", "hop_frames", "oversampling"]


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def assert_gate_equal(got, want, what):
    """powers and counts exactly; the logarithmic figures within 1e-12 (a few ulps of log10 at magnitudes <= 100: libm's
    last place is not pinned)"""
    for k in M.FIELDS_EXACT:
        assert bits(got[k]) == bits(want[k]) if k == "gated_power" else got[k] == want[k], (what, k, got[k], want[k])
    for k in M.FIELDS_LUFS:
        g, w = got[k], want[k]
        assert (g == w) if math.isinf(w) or math.isinf(g) else abs(g - w) <= 1e-12, (what, k, g, w)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.loudness_hops) and callable(W.loudness_coefficients) and callable(W.loudness_gate)
    assert hasattr(W.MixContext, "clip_loudness")
    assert hasattr(W.Engine, "loudness_sample") and hasattr(W.Engine, "normalize_loudness_sample")


def test_struct_and_flag_equal_the_headers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\n'
                   'int main(void) { printf("%zu", sizeof(wbx_loudness));\n'
                   + "".join('  printf(" %%zu", offsetof(wbx_loudness, %s));\n' % f for f in FIELDS)
                   + '  printf(" %d\\n", WBX_LOUD_TRUE_PEAK); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.Loudness
    assert [f for f, _ in S._fields_] == FIELDS
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_ffi.LOUD_TRUE_PEAK]
    assert got[0] == 80 and got[1:-1] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76] and got[-1] == M.TRUE_PEAK


def test_adapter_with_loudness_compiles(tmp_path):
    """a translation unit that uses Engine::loudness_sample / normalize_loudness_sample (never run: it would need a device)"""
    src = tmp_path / "adapter_loudness.cpp"
    src.write_text('#include "wbx_adapter.hpp"\n'
                   'uint32_t deliver(wbx::Engine& e, uint32_t bounce, uint64_t n, double* lufs) {\n'
                   '  const wbx_loudness m = e.loudness_sample(bounce, 0, n, WBX_LOUD_TRUE_PEAK);\n'
                   '  *lufs = m.integrated;\n  float g = 0.0f;\n'
                   '  return e.normalize_loudness_sample(bounce, 0, n, -14.0, 0.891f, &g);\n}\n'
                   'int main() { return sizeof(wbx_loudness) == 80 && wbx_loudness_hop_frames(48000) == 4800 ? 0 : 1; }\n')
    exe = str(tmp_path / "adapter_loudness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx", "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.call([exe]) == 0


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    L = W.lib()
    st, new, g = _ffi.Loudness(), C.c_uint32(), C.c_float()
    assert L.wbx_clip_loudness(None, 0, 0, 8000, 0, C.byref(st), None, 0) == -4
    assert L.wbx_engine_loudness_sample(None, 0, 0, 8000, 0, C.byref(st), None, 0) == -4
    assert L.wbx_engine_normalize_loudness_sample(None, 0, 0, 8000, -23.0, 0.0, C.byref(new), C.byref(g)) == -4
    assert L.wbx_loudness_coefficients(48000, None) == -4
    k = np.full(10, 7.0)
    assert L.wbx_loudness_coefficients(7999, k.ctypes.data) == -3 and L.wbx_loudness_coefficients(384001, k.ctypes.data) == -3
    assert np.all(k == 7.0)
    E = np.ones(8)
    assert L.wbx_loudness_gate(1, 8, 800, E.ctypes.data, None) == -4
    assert L.wbx_loudness_gate(0, 8, 800, E.ctypes.data, C.byref(st)) == -4 and L.wbx_loudness_gate(3, 2, 800, E.ctypes.data, C.byref(st)) == -4
    assert L.wbx_loudness_gate(1, 8, 0, E.ctypes.data, C.byref(st)) == -4 and L.wbx_loudness_gate(1, 8, 800, None, C.byref(st)) == -4
    assert L.wbx_loudness_gate(2, 0, 800, None, C.byref(st)) == 0 and st.blocks == 0 and st.integrated == -math.inf


def test_hops():
    L = W.lib()
    for rate, hop in ((8000, 800), (11025, 1103), (22050, 2205), (44100, 4410), (48000, 4800), (96000, 9600), (384000, 38400)):
        assert L.wbx_loudness_hop_frames(rate) == hop == M.hop_frames(rate)
        for n in (0, 1, hop - 1, hop, hop + 1, 4 * hop - 1, 4 * hop, 1234567, (1 << 31) - 17):
            assert W.loudness_hops(rate, n) == n // hop == M.hops(rate, n)
    assert L.wbx_loudness_hop_frames(7999) == 0 and L.wbx_loudness_hop_frames(384001) == 0 and W.loudness_hops(0, 100) == 0


# ---- the coefficients -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_coefficients_equal_the_model_bit_for_bit(rate):
    got, want = W.loudness_coefficients(rate), M.coefficients(rate)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (10,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (rate, got, want)


@pytest.mark.parametrize("rate", RATES)
def test_coefficients_within_4_ulps_of_libm(rate):
    got, ref = W.loudness_coefficients(rate), M.coefficients_libm(rate)
    worst = max(abs(float(g) - float(r)) / math.ulp(float(r)) for g, r in zip(got, ref))
    print("coefficients", rate, "worst distance from the math.tan rendering: %.1f ulps" % worst)
    assert worst <= 4.0


def test_coefficients_at_48000_are_the_standards_table():
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    got = W.loudness_coefficients(48000)
    for g, t in zip(got, table):
        assert "%.14f" % g == "%.14f" % t, (g, t)


# ---- the gate ---------------------------------------------------------------------------------------------------------------
def test_gate_on_random_energies():
    rng = np.random.default_rng(1770)
    for case in range(60):
        ch = 1 + case % 2
        H = [0, 1, 2, 3, 4, 5, 29, 30, 31, 39, 40, 41, 200, 1000][case % 14]
        hop = [800, 1103, 4800][case % 3]
        E = 10.0 ** rng.uniform(-12.0 if case % 4 else -9.0, 0.0 if case % 4 else -3.0, (ch, H)) * hop
        if case % 5 == 0 and H:
            E[:, rng.integers(0, H, H // 3)] = 0.0
        assert_gate_equal(W.loudness_gate(E, hop), M.gate(E, hop), ("random", case))


def test_gate_exactly_on_and_beside_the_absolute_threshold():
    """4 * hop = 4096, so z = s / 4096 is exact: hops of ABS * 1024 give blocks exactly ON the gate (they fail: the test is >)"""
    hop, H = 1024, 12
    on = float(M.ABS_GATE) * 1024.0
    for ch in (1, 2):
        for e, passing in ((on, 0), (np.nextafter(on, 1.0), H - 3), (np.nextafter(on, 0.0), 0)):
            E = np.full((ch, H), e / ch)                      # (two channels of half the energy add up exactly)
            got, want = W.loudness_gate(E, hop), M.gate(E, hop)
            assert_gate_equal(got, want, ("absolute", ch, e))
            assert got["blocks"] == H - 3 and got["blocks_gated"] == passing, (ch, e, got)
            assert (got["integrated"] == -math.inf) == (passing == 0)
    mixed = np.full((1, 40), on)
    mixed[0, 20:] = np.nextafter(on, 1.0)                       # blocks 0..16 on the gate, 20..36 above it, 17..19 as they round
    got = W.loudness_gate(mixed, hop)
    assert_gate_equal(got, M.gate(mixed, hop), "absolute, mixed")
    assert 17 <= got["blocks_gated"] <= 20


def test_gate_exactly_on_and_beside_the_relative_threshold():
    """P hops of energy 1 then P of 19, 4 * hop = 1024: every sum is a small integer, the mean of the blocks is 40 / 1024 for
    any P and fl(40 * 0.1) = 4, so the quiet blocks (4 / 1024) sit exactly ON the relative gate and fail it"""
    hop, P = 256, 25
    E = np.concatenate([np.full(P, 1.0), np.full(P, 19.0)])[None, :]
    got = W.loudness_gate(E, hop)
    assert_gate_equal(got, M.gate(E, hop), "relative, on")
    assert got["blocks"] == 2 * P - 3 and got["blocks_gated"] == P
    seen = set()
    for steps in range(-6, 7):                                  # the quiet level a few ulps to either side
        q = 1.0
        for _ in range(abs(steps)):
            q = float(np.nextafter(q, 2.0 if steps > 0 else 0.0))
        E2 = E.copy()
        E2[0, :P] = q
        got = W.loudness_gate(E2, hop)
        assert_gate_equal(got, M.gate(E2, hop), ("relative", steps))
        seen.add(got["blocks_gated"])
    assert seen == {P, 2 * P - 3}                               # the scan crosses the threshold
    halves = np.stack([E[0] * 0.5, E[0] * 0.5])                 # the same powers from two channels
    assert_gate_equal(W.loudness_gate(halves, hop), M.gate(halves, hop), "relative, stereo")
    assert W.loudness_gate(halves, hop)["blocks_gated"] == P


# ---- the model is a meter ---------------------------------------------------------------------------------------------------
def tone(freq, rate, segments):
    """segments of (dBFS, seconds), phase continuous"""
    parts, t0 = [], 0
    for db, sec in segments:
        n = int(round(sec * rate))
        t = np.arange(t0, t0 + n, dtype=np.float64)
        parts.append(10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * freq * t / rate))
        t0 += n
    return np.concatenate(parts).astype(np.float32)


def stereo_of_one(x, rate):
    """the model's result for a stereo signal whose channels are both x (channels are filtered independently: E of one)"""
    E = M.hop_energies([x], 0, len(x), rate)
    return M.gate(np.concatenate([E, E]), M.hop_frames(rate))


EBU_3341 = {1: ([(-23, 20)], -23.0), 2: ([(-33, 20)], -33.0), 3: ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
            4: ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0), 5: ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)}


@pytest.mark.parametrize("case", sorted(EBU_3341))
def test_model_on_ebu_3341_integrated_loudness(case):
    segments, want = EBU_3341[case]
    got = stereo_of_one(tone(1000.0, 48000, segments), 48000)["integrated"]
    print("EBU 3341 case", case, "integrated %.4f LUFS, expected %.1f +- 0.1" % (got, want))
    assert abs(got - want) <= 0.1


def test_model_on_a_full_scale_mono_997_hz_tone():
    x = tone(997.0, 48000, [(0, 5)])
    got = M.measure([x], 0, len(x), 48000)["integrated"]
    print("mono 997 Hz 0 dBFS: %.4f LUFS" % got)
    assert abs(got - -3.01) <= 0.1


EBU_3342 = {1: ([(-20, 20), (-30, 20)], 10.0), 2: ([(-20, 20), (-15, 20)], 5.0), 3: ([(-40, 20), (-20, 20)], 20.0),
            4: ([(-50, 20), (-35, 20), (-20, 20), (-35, 20), (-50, 20)], 15.0)}


@pytest.mark.parametrize("case", sorted(EBU_3342))
def test_model_on_ebu_3342_loudness_range(case):
    segments, want = EBU_3342[case]
    got = stereo_of_one(tone(1000.0, 48000, segments), 48000)["range_lu"]
    print("EBU 3342 case", case, "range %.3f LU, expected %.0f +- 1" % (got, want))
    assert abs(got - want) <= 1.0


@pytest.mark.parametrize("rate", (8000, 48000))
def test_segmented_energies_against_one_sequential_pass(rate):
    """uniform noise on a DC offset, the worst case for the high-pass's tail: the first three hops ARE the sequential pass"""
    rng = np.random.default_rng(rate)
    x = (rng.uniform(-0.5, 0.5, 12 * M.hop_frames(rate) + 17) + 0.25).astype(np.float32)
    seg, seq = M.hop_energies([x], 0, len(x), rate)[0], M.sequential_energies(x, 0, len(x), rate)
    assert len(seg) == len(seq) == 12
    assert np.array_equal(seg[:3].view(np.uint64), seq[:3].view(np.uint64))
    worst = float(np.max(np.abs(seg / seq - 1.0)))
    print("segmented against sequential at", rate, "worst relative difference", worst)
    assert worst <= 1e-12


def test_model_range_rules():
    """frames beside the range and a NaN inside it: the first count for nothing, the second enters as 0.0"""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, 6000).astype(np.float32)
    alone = M.hop_energies([x[300:300 + 4100].copy()], 0, 4100, 8000)
    inside = M.hop_energies([x], 300, 4100, 8000)
    assert alone.shape == (1, 5) and np.array_equal(alone.view(np.uint64), inside.view(np.uint64))
    y, z = x.copy(), x.copy()
    y[1000], z[1000] = np.nan, 0.0
    assert np.array_equal(M.hop_energies([y], 0, 6000, 8000).view(np.uint64), M.hop_energies([z], 0, 6000, 8000).view(np.uint64))
    assert M.true_peak([y], 0, 6000, 192000)[0] == np.max(np.abs(z))


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def test_coefficients_and_gate_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/loudness_main.cpp: wbx_loudness.h alone, stand-alone (its own main), over random and degenerate energies"""
    exe = str(tmp_path / "loudness_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "loudness_main.cpp"), "-o", exe])
    rng = np.random.default_rng(3341)
    cases = []
    for H in (0, 1, 2, 3):                                      # no block at all
        cases += [(ch, 800, 10.0 ** rng.uniform(-6, 0, (ch, H))) for ch in (1, 2)]
    cases += [(2, 4800, np.zeros((2, 50))), (1, 800, np.zeros((1, 4)))]                  # all zero
    cases += [(1, 800, np.full((1, 64), 1e-9)), (2, 1103, rng.uniform(0, 4e-5, (2, 45)))]   # everything below the absolute gate
    cases += [(1 + i % 2, (800, 2205, 4410)[i % 3], 10.0 ** rng.uniform(-10, 0, (1 + i % 2, int(rng.integers(4, 400))))) for i in range(12)]
    cases += [(1, 4800, np.full((1, 33), np.inf)), (1, 800, np.concatenate([np.full(20, 1e-30), np.full(20, 1e300)])[None, :])]
    text = ["%d %s" % (len(RATES), " ".join(str(r) for r in RATES))]
    for ch, hop, E in cases:
        text.append("%d %d %d %s" % (ch, E.shape[1], hop, " ".join("%016x" % bits(v) for v in E.ravel())))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(text) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(RATES) + len(cases) + 1 and lines[-1] == "hops ok"
    for rate, line in zip(RATES, lines):
        words = line.split()
        assert int(words[0]) == rate and [int(w, 16) for w in words[1:]] == [bits(v) for v in M.coefficients(rate)], rate
    for i, ((ch, hop, E), line) in enumerate(zip(cases, lines[len(RATES):])):
        w = line.split()
        got = dict(gated_power=struct.unpack("<d", struct.pack("<Q", int(w[0], 16)))[0], hops=int(w[1]), blocks=int(w[2]),
                   blocks_gated=int(w[3]), hop_frames=int(w[4]), integrated=float(w[5]), momentary_max=float(w[6]),
                   short_term_max=float(w[7]), range_lu=float(w[8]))
        with np.errstate(all="ignore"):
            want = M.gate(E, hop)
        assert_gate_equal(got, want, ("stand-alone", i))
