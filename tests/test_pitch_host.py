"""Pitch-shifting a clip, the part that needs no device: the symbols of include/wbx.h "Pitch-shifting a clip" exist and match
their binding twins, the adapter's method compiles, NULL handles are refused, wbx_pitch_mid_frames equals the Python twin
(tests/pitch_model.py), every refusal of the argument check, the model itself has the properties the header states,
pitch_ratio covers every whole cent of two octaves — and wbx_pitch.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_model as M
import resample_model as RS
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_pitch_mid_frames", "wbx_pitch_max_steps", "wbx_pitch_launch_shape", "wbx_pitch_ms", "wbx_clip_pitch", "wbx_engine_pitch_sample"]
EDGE = M.MAX_FRAMES - 1                                        # the longest result
RATIOS = [(3, 2), (2, 3), (2, 1), (1, 2), (4, 1), (1, 4), (1265, 1194), (1194, 1265), (967, 1024), (6, 4), (1280, 1279), (1279, 1280)]
REFUSED_RATIOS = [(0, 1), (1, 0), (0, 0), (1, 1), (7, 7), (5, 1), (1, 5), (4001, 1000), (1000, 4001), (1282, 1281), (1281, 1283),
                  (2563, 2562)]


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    """the ten new names: five C entry points, wbx_pitch_info, and Python's pitch_mid_frames, pitch_ratio, clip_pitch /
    pitch_ms, pitch_sample / transpose_sample"""
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.pitch_mid_frames) and callable(W.pitch_ratio) and callable(W.pitch_launch_shape)
    assert hasattr(W.MixContext, "clip_pitch") and hasattr(W.MixContext, "pitch_ms")
    for m in ("pitch_sample", "transpose_sample"):
        assert hasattr(W.Engine, m), m
    flat = re.sub(r"\s*\*\s*", " ", header)
    assert "Pitch-shifting a clip" in flat and "Not offered: pitch shifting" not in flat
    assert L.wbx_pitch_max_steps() == 1 << 22 == M.MAX_STEPS
    assert "pitch_sample" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    fields = ["steps", "searched_steps", "candidates", "mid_frames", "max_shift", "launches", "L", "M"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", '
                   "sizeof(wbx_pitch_info), " + ", ".join("offsetof(wbx_pitch_info, %s)" % f for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.PitchInfo
    assert got == [48, 0, 8, 16, 24, 32, 36, 40, 44] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert re.search(r"wbx_pitch_info\s*\{\s*/\* 48 bytes \*/", open(os.path.join(ROOT, "include", "wbx.h")).read())


def test_adapter_with_pitch_compiles(tmp_path):
    """tests/cpp/adapter_pitch.cpp uses Engine::pitch_sample; it is compiled and linked here and run by
    tests/test_gpu_pitch.py (it needs a device)"""
    exe = str(tmp_path / "adapter_pitch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_pitch.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    new, pi, st, ms = C.c_uint32(77), _ffi.PitchInfo(), _ffi.ClipStats(), C.c_double(5.0)
    pi.mid_frames = 123
    pos = np.full(8, 9, dtype=np.int32)
    assert L.wbx_clip_pitch(None, 0, 1, 0, 64, 64, 3, 2, 1, 32, 8, pos.ctypes.data, 8, C.byref(pi), C.byref(st)) == -4 and np.all(pos == 9)
    assert L.wbx_engine_pitch_sample(None, 0, 0, 64, 64, 3, 2, 1, 32, 8, C.byref(pi), C.byref(new)) == -4 and new.value == 77
    assert L.wbx_pitch_ms(None, C.byref(ms)) == -4 and ms.value == 5.0 and pi.mid_frames == 123


# ---- wbx_pitch_mid_frames ---------------------------------------------------------------------------------------------------
def test_mid_frames_equal_the_model_over_a_grid():
    rng = np.random.default_rng(0x917C)
    ms = [0, 1, 2, 3, 7, 1000, 9600, (1 << 22) * 16, EDGE - 1, EDGE, EDGE + 1, 1 << 40, (1 << 64) - 1] + [int(v) for v in rng.integers(1, EDGE, 20)]
    for num, den in RATIOS:
        g = math.gcd(num, den)
        for m in ms:
            want = M.mid_frames(m, num, den)
            assert W.pitch_mid_frames(m, num, den) == want, (m, num, den)
            if m < 1 << 50:
                assert want == -(-m * (num // g) // (den // g))
    assert W.pitch_mid_frames(EDGE, 4, 1) == 4 * EDGE and W.pitch_mid_frames(EDGE, 1, 4) == (EDGE + 3) // 4
    assert W.pitch_mid_frames(EDGE, 1265, 1194) == -(-EDGE * 1265 // 1194)
    assert W.pitch_mid_frames((1 << 64) - 1, 4, 1) == (1 << 64) - 1          # what does not fit 64 bits


def test_mid_frames_are_zero_for_every_refused_ratio():
    for num, den in REFUSED_RATIOS:
        assert M.ratio(num, den) is None, (num, den)
        for m in (1, 1000, EDGE):
            assert W.pitch_mid_frames(m, num, den) == 0 == M.mid_frames(m, num, den), (m, num, den)
    for num, den in RATIOS:
        assert M.ratio(num, den) is not None and W.pitch_mid_frames(1000, num, den) > 0


# ---- the argument check -----------------------------------------------------------------------------------------------------
OK = dict(n=1000, m=1000, num=3, den=2, q=RS.GOOD, N=128, D=24, cap=None)
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(m=0), -4), (dict(num=0), -4), (dict(den=0), -4), (dict(num=2), -4), (dict(num=7, den=7), -4),
          (dict(q=3), -4), (dict(q=-1), -4), (dict(q=RS.FAST), 0), (dict(q=RS.BEST), 0),
          (dict(m=M.MAX_FRAMES, n=M.MAX_FRAMES - 1), -4), (dict(m=EDGE, n=EDGE, num=2, den=3, N=8192), 0),
          (dict(m=EDGE, n=EDGE), -4),                           # m' = 3 m / 2 reaches 2^31 - 16: the stretch's refusal
          (dict(n=M.MAX_FRAMES, m=EDGE, num=2, den=3), -4), (dict(n=1 << 63, m=1 << 63), -4),
          (dict(num=4, den=1, m=500), 0), (dict(num=1, den=4, m=4000), 0), (dict(num=5, den=1), -3), (dict(num=1, den=5), -3),
          (dict(num=4001, den=1000), -3), (dict(num=1000, den=4001), -3),
          (dict(num=1280, den=1279), 0), (dict(num=1282, den=1281), -3), (dict(num=1281, den=1283), -3), (dict(num=2563, den=2562), -3),
          (dict(num=1265, den=1194), 0), (dict(num=1194, den=1265), 0), (dict(num=967, den=1024), 0),
          (dict(N=24), -4), (dict(N=8200), -4), (dict(N=36), -4), (dict(N=0), -4), (dict(N=32), 0), (dict(N=8192), 0),
          (dict(D=4096), 0), (dict(D=4097), -4),
          (dict(cap=0), -4), (dict(cap=23), -4), (dict(cap=24), 0),           # m' = 1500, Hs = 64: K' = 24
          (dict(m=5333), 0), (dict(m=5334), -3),                # m' = 8000 / 8001 against 8 n
          (dict(n=12000), 0), (dict(n=12001), -3),              # n against 8 m' = 12000
          (dict(n=1, m=1, num=4, den=1), 0), (dict(n=1, m=3, num=4, den=1), -3),
          (dict(num=5, den=1, N=36), -3),                       # the ratio is judged before the stretch's arguments
          (dict(num=5, den=1, q=7), -4), (dict(num=5, den=1, m=0), -4), (dict(m=5334, N=36), -4), (dict(m=5334, cap=0), -4),
          (dict(n=1 << 25, m=(1 << 26) * 2 // 3, N=32), 0),     # m' = 2^26 - 1: K' = 2^22, the cap
          (dict(n=1 << 25, m=(1 << 26) * 2 // 3 + 12, N=32), -3),   # m' = 2^26 + 17: K' = 2^22 + 2
          (dict(n=1 << 25, m=(1 << 26) * 2 // 3 + 12, N=64), 0)]


def test_check_args_of_the_model_every_refusal_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check_args(a["n"], a["m"], a["num"], a["den"], a["q"], a["N"], a["D"], a["cap"]) == want, change
    a = dict(OK, n=1 << 25, m=(1 << 26) * 2 // 3 + 12, N=32)
    mid = M.mid_frames(a["m"], 3, 2)
    assert M.ST.steps(mid, 32) == M.MAX_STEPS + 2 and M.ST.steps(M.mid_frames((1 << 26) * 2 // 3, 3, 2), 32) == M.MAX_STEPS
    assert {w for _, w in CHECKS} == {0, -4, -3}


# ---- properties of the model --------------------------------------------------------------------------------------------------
def test_every_kept_frame_lies_inside_the_intermediate():
    rng = np.random.default_rng(0xF100)
    cases = [(int(m), int(a), int(b)) for m, a, b in zip(rng.integers(1, EDGE, 4000), rng.integers(1, 5200, 4000), rng.integers(1, 1281, 4000))]
    cases += [(m, num, den) for num, den in RATIOS for m in (1, 2, 3, 4, 5, 1023, 1024, 1025, EDGE)]
    seen = 0
    for m, num, den in cases:
        r = M.ratio(num, den)
        if r is None:
            continue
        L, Mm = r
        mid = M.mid_frames(m, num, den)
        assert (m - 1) * Mm // L < mid, (m, num, den)
        assert -(-mid * L // Mm) >= m                           # the conversion of m' frames has at least m
        seen += 1
    assert seen > 1000


def test_the_result_has_m_frames_and_the_models_info():
    rng = np.random.default_rng(0xA11)
    src = [(0.5 * rng.standard_normal(900)).astype(np.float32) for _ in range(2)]
    for n, m, num, den, q in ((700, 700, 3, 2, RS.FAST), (700, 701, 2, 3, RS.GOOD), (16, 1, 2, 1, RS.FAST), (1, 1, 1, 2, RS.FAST),
                              (700, 350, 1265, 1194, RS.FAST), (700, 1400, 1, 2, RS.BEST)):
        out, p, info = M.pitch_clip(src, 100, n, m, num, den, q, 64, 24)
        mid = M.mid_frames(m, num, den)
        assert len(out) == 2 and all(len(o) == m and o.dtype == np.float32 for o in out)
        assert info["mid_frames"] == mid and info["steps"] == len(p) == -(-mid // 32) and (info["L"], info["M"]) == M.ratio(num, den)
    with pytest.raises(M.Refused):
        M.pitch_clip(src, 0, 700, 700, 5, 1, RS.GOOD, 64, 24)


def rms(v):
    return float(np.sqrt(np.mean(np.asarray(v, dtype=np.float64) ** 2)))


@pytest.mark.parametrize("ratio,want_hz", [((3, 2), 660.0), ((2, 3), 440.0 * 2 / 3)], ids=["up-a-fifth", "down-a-fifth"])
def test_a_sine_moves_to_the_new_pitch_at_its_level(ratio, want_hz):
    """440 Hz at 48 kHz, n = m = 9600, N = 512, D = 128: the largest bin of a Hann-windowed 2^18-point FFT lies within 1 % of
    the transposed frequency, and the RMS stays within 5 % of the source's"""
    n, rate = 9600, 48000
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / rate).astype(np.float32)
    out, _, info = M.pitch_clip([x], 0, n, n, ratio[0], ratio[1], RS.GOOD, 512, 128)
    y = out[0].astype(np.float64)
    spec = np.abs(np.fft.rfft(y * np.hanning(n), 1 << 18))
    hz = float(np.argmax(spec)) * rate / (1 << 18)
    print("ratio %d/%d: peak at %.1f Hz (wanted %.2f), rms %.4f against %.4f, %d of %d steps searched"
          % (ratio[0], ratio[1], hz, want_hz, rms(y), rms(x), info["searched_steps"], info["steps"]))
    assert len(y) == n and abs(hz - want_hz) <= 0.01 * want_hz
    assert abs(rms(y) - rms(x)) <= 0.05 * rms(x)


# ---- pitch_ratio ------------------------------------------------------------------------------------------------------------
def test_pitch_ratio_over_every_whole_cent_of_two_octaves():
    worst = 0.0
    for cents in range(-2400, 2401):
        if cents == 0:
            continue
        num, den = W.pitch_ratio(0, cents)
        assert num != den and 1 <= den <= 1280 and math.gcd(num, den) == 1, cents
        err = abs(1200.0 * math.log2(num / den) - cents)
        worst = max(worst, err)
        assert err <= 0.5, (cents, num, den, err)
        assert M.ratio(num, den) == (den, num)                  # within two octaves, L <= 1280: the call takes it ...
        for q in RS.QUALITY:                                    # ... at every quality
            assert M.check_args(48000, 48000, num, den, q, 2048, 512) == 0, (cents, q)
    print("worst error %.3f cent" % worst)
    assert W.pitch_ratio(7) == W.pitch_ratio(0, 700) == W.pitch_ratio(6, 100) and W.pitch_ratio(12) == (2, 1) and W.pitch_ratio(-24) == (1, 4)
    for args in ((0, 0), (0,), (1, -100)):
        with pytest.raises(ValueError):
            W.pitch_ratio(*args)


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/pitch_main.cpp: wbx_pitch.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "pitch_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "pitch_main.cpp"), "-o", exe])
    lines, want = [], []
    for num, den in RATIOS + REFUSED_RATIOS:
        for m in (0, 1, 9600, EDGE, (1 << 64) - 1):
            lines.append("m %d %d %d" % (m, num, den))
            want.append("m %d" % M.mid_frames(m, num, den))
        r = M.ratio(num, den)
        lines.append("r %d %d" % (num, den))
        want.append("r %d %d %d" % ((1,) + r if r else (0, 0, 0)))
    for change, status in CHECKS:
        a = dict(OK, **change)
        lines.append("c %d %d %d %d %d %d %d %d %d" % (a["n"], a["m"], a["num"], a["den"], a["q"], a["N"], a["D"], a["cap"] is not None,
                                                       a["cap"] or 0))
        if status:
            want.append("c %d 0 0 0 0 0 0" % status)
        else:
            p, mid = RS.plan(a["num"], a["den"], a["q"]), M.mid_frames(a["m"], a["num"], a["den"])
            want.append("c 0 %d %d %d %d %d %d" % (mid, M.ST.steps(mid, a["N"]), p["L"], p["M"], p["H"], p["T"]))
    for num, den in RATIOS:                                     # the tile: a multiple of 4 whose span fits 4096 floats
        for q in RS.QUALITY:
            p = RS.plan(num, den, q)
            tile = min(1024, ((4096 - p["T"]) * p["L"] // p["M"] + 1) & ~3)
            span = (p["L"] - 1 + (tile - 1) * p["M"]) // p["L"] + p["T"]
            assert tile >= 4 and tile % 4 == 0 and span <= 4096
            lines.append("t %d %d %d" % (p["L"], p["M"], p["T"]))
            want.append("t %d %d" % (tile, span))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "pitch ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
