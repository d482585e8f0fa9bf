"""Tracking a clip's pitch, the part that needs no device: the symbols of include/wbx.h "Tracking a clip's pitch" exist and
match their binding twins, the two structs have the header's layout, the adapter's method compiles, NULL handles are refused,
wbx_f0_hops / _check / _launch_hops equal the Python twin (tests/f0_model.py), every refusal of the argument check, the model
itself finds tones within half a cent and leaves noise and silence unvoiced — and wbx_f0.h runs stand-alone under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import f0_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_f0_hops", "wbx_f0_check", "wbx_f0_max_hops", "wbx_f0_launch_terms", "wbx_f0_launch_hops", "wbx_f0_ms", "wbx_clip_f0",
       "wbx_engine_f0_sample"]
RATE = 48000
TONES = [55.0, 82.41, 110.0, 146.83, 220.0, 329.63, 440.0, 659.26, 987.77]   # A1 E2 A2 D3 A3 E4 A4 E5 B5
YIN = dict(W=1024, H=256, tau_min=24, tau_max=1024, threshold=0.15)


@pytest.fixture(autouse=True)
def library_with_f0():
    """every test here, those of the model alone included, stands on a library that has the calls: the model is the reference
    of tests/test_gpu_f0.py and means nothing without them"""
    L = W.lib()
    assert all(hasattr(L, n) for n in NEW)


def terms():
    return int(W.lib().wbx_f0_launch_terms())


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.f0_hops) and W.F0_DTYPE == M.DTYPE and W.F0_DTYPE.itemsize == 32
    assert hasattr(W.MixContext, "clip_f0") and hasattr(W.MixContext, "f0_ms")
    for m in ("f0_sample", "detect_note_sample", "tune_sample"):
        assert hasattr(W.Engine, m), m
    flat = re.sub(r"\s*\*\s*", " ", header)
    assert "Tracking a clip's pitch" in flat and "pitch correction or detection" not in flat
    assert L.wbx_f0_max_hops() == 1 << 20 == M.MAX_HOPS and L.wbx_f0_launch_terms() >= 8192 * 4096
    assert "f0_sample" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()


def test_the_structs_have_the_headers_size_and_layout(tmp_path):
    frame, info = ["period", "dip", "energy", "lag", "voiced"], ["hops", "voiced_hops", "terms", "launches"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * (len(frame) + len(info) + 1)
                   + '\\n", sizeof(wbx_f0_frame), ' + ", ".join("offsetof(wbx_f0_frame, %s)" % f for f in frame) + ", sizeof(wbx_f0_info), "
                   + ", ".join("offsetof(wbx_f0_info, %s)" % f for f in info) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    F, I = _ffi.F0Frame, _ffi.F0Info
    assert got == [32, 0, 8, 16, 24, 28, 32, 0, 8, 16, 24]
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in frame] + [C.sizeof(I)] + [getattr(I, f).offset for f in info]
    assert [M.DTYPE.fields[f][1] for f in frame] == got[1:6] and M.DTYPE.itemsize == 32
    text = open(os.path.join(ROOT, "include", "wbx.h")).read()
    assert re.search(r"wbx_f0_frame\s*\{\s*/\* 32 bytes \*/", text) and re.search(r"wbx_f0_info\s*\{\s*/\* 32 bytes \*/", text)


def test_adapter_with_f0_compiles(tmp_path):
    """tests/cpp/adapter_f0.cpp uses Engine::f0_sample; it is compiled and linked here and run by tests/test_gpu_f0.py (it
    needs a device)"""
    exe = str(tmp_path / "adapter_f0")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_f0.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    fi, ms = _ffi.F0Info(), C.c_double(5.0)
    fi.hops = 123
    rec = np.zeros(8, dtype=M.DTYPE)
    rec["lag"] = 9
    assert L.wbx_clip_f0(None, 0, 0, 4000, 1024, 256, 24, 1024, 0.15, rec.ctypes.data, 8, C.byref(fi)) == -4
    assert L.wbx_engine_f0_sample(None, 0, 0, 4000, 1024, 256, 24, 1024, 0.15, rec.ctypes.data, 8, C.byref(fi)) == -4
    assert L.wbx_f0_ms(None, C.byref(ms)) == -4 and ms.value == 5.0 and fi.hops == 123 and np.all(rec["lag"] == 9)


# ---- wbx_f0_hops, wbx_f0_check, the launches ----------------------------------------------------------------------------------
EDGE = M.MAX_FRAMES - 1
OK = dict(n=4000, W=1024, H=256, tau_min=24, tau_max=1024, thr=0.15, out=True, cap=None)
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=M.MAX_FRAMES), -4), (dict(n=1 << 63), -4), (dict(n=EDGE, H=4096, cap=1 << 20), 0), (dict(n=1), 0),
          (dict(W=56), -4), (dict(W=64, tau_max=63), 0), (dict(W=68), -4), (dict(W=8192), 0), (dict(W=8200), -4), (dict(W=0), -4),
          (dict(tau_max=7, tau_min=2), -4), (dict(tau_max=8, tau_min=2), 0), (dict(tau_max=4095), 0), (dict(tau_max=4096), -4),
          (dict(tau_min=1), -4), (dict(tau_min=0), -4), (dict(tau_min=2), 0), (dict(tau_min=1023), 0), (dict(tau_min=1024), -4),
          (dict(tau_min=5000), -4), (dict(H=0), -4), (dict(H=1, cap=2000), 0), (dict(H=1 << 20), 0), (dict(H=(1 << 20) + 1), -4),
          (dict(thr=0.0), -4), (dict(thr=-0.5), -4), (dict(thr=1.0), 0), (dict(thr=1.0000001), -4), (dict(thr=5e-324), 0),
          (dict(thr=float("nan")), -4), (dict(thr=float("inf")), -4), (dict(thr=float("-inf")), -4),
          (dict(out=False), -4), (dict(out=False, n=2047), 0),   # no hops need no buffer
          (dict(cap=7), -4), (dict(cap=8), 0), (dict(cap=0), -4), (dict(cap=0, n=2047), 0),   # (4000 - 2048) // 256 + 1 = 8 hops
          (dict(n=2047), 0), (dict(n=2048, cap=0), -4), (dict(n=2048, cap=1), 0),
          (dict(n=72 + (1 << 20) - 1, W=64, H=1, tau_min=2, tau_max=8, cap=1 << 20), 0),        # 2^20 hops: the most
          (dict(n=72 + (1 << 20), W=64, H=1, tau_min=2, tau_max=8, cap=(1 << 20) + 1), -3),     # one more
          (dict(n=72 + (1 << 20), W=64, H=1, tau_min=2, tau_max=8, cap=1 << 20), -4),           # the capacity is asked first
          (dict(n=72 + (1 << 20), W=64, H=1, tau_min=2, tau_max=8, out=False, cap=1 << 21), -4),
          (dict(n=EDGE, H=1, cap=1 << 40), -3), (dict(n=EDGE, H=1, W=68, cap=1 << 40), -4)]


def lib_check(a):
    cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["W"], a["H"], a["tau_max"])
    return W.lib().wbx_f0_check(a["n"], a["W"], a["H"], a["tau_min"], a["tau_max"], a["thr"], int(a["out"]), cap)


def test_check_every_refusal_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check(a["n"], a["W"], a["H"], a["tau_min"], a["tau_max"], a["thr"], a["out"], a["cap"]) == want, change
        assert lib_check(a) == want, change
    assert {w for _, w in CHECKS} == {0, -4, -3}


def test_hops_equal_the_model_over_a_grid():
    rng = np.random.default_rng(0xF0)
    assert W.f0_hops(1024 + 1024 - 1, 1024, 256, 1024) == 0 == M.hops(2047, 1024, 256, 1024)
    assert W.f0_hops(1024 + 1024, 1024, 256, 1024) == 1 == M.hops(2048, 1024, 256, 1024)
    for Wn, tau_max, H in [(64, 8, 1), (72, 15, 7), (256, 511, 64), (1024, 1024, 256), (8192, 4095, 1 << 20), (2048, 1023, 512)]:
        need = Wn + tau_max
        ns = [0, 1, need - 1, need, need + 1, need + H - 1, need + H, need + H + 1, need + 17 * H - 1, EDGE, EDGE + 1, 1 << 40, (1 << 64) - 1]
        ns += [int(v) for v in rng.integers(1, EDGE, 10)]
        for n in ns:
            want = M.hops(n, Wn, H, tau_max)
            assert W.f0_hops(n, Wn, H, tau_max) == want, (n, Wn, H, tau_max)
            assert want == (0 if n < need else (n - need) // H + 1)
    for Wn, H, tau_max in [(60, 1, 8), (68, 1, 8), (8200, 1, 8), (64, 0, 8), (64, (1 << 20) + 1, 8), (64, 1, 7), (64, 1, 4096)]:
        assert W.f0_hops(1 << 20, Wn, H, tau_max) == 0 == M.hops(1 << 20, Wn, H, tau_max)     # a refused shape


def test_launch_hops_equal_the_model():
    L, T = W.lib(), terms()
    seen = set()
    for Wn in (64, 72, 256, 1024, 2048, 8192):
        for tau_max in (8, 15, 63, 511, 512, 1023, 4095):
            per = L.wbx_f0_launch_hops(Wn, tau_max)
            assert per == M.launch_hops(Wn, tau_max, T) >= 1, (Wn, tau_max)
            assert per == 1 << 20 or per * Wn * (tau_max + 1) <= T or per == 1
            assert per < 8 or per % 8 == 0
            seen.add(per)
    assert len(seen) > 3
    assert L.wbx_f0_launch_hops(68, 8) == 0 and L.wbx_f0_launch_hops(64, 7) == 0 and L.wbx_f0_launch_hops(64, 4096) == 0


# ---- properties of the model --------------------------------------------------------------------------------------------------
def sine(hz, n):
    return np.sin(2 * np.pi * hz * np.arange(n) / RATE).astype(np.float32)


def harmonic(hz, n, harmonics=8):
    i = np.arange(n, dtype=np.float64)
    return (0.3 * sum(np.sin(2 * np.pi * hz * k * i / RATE + k) / k for k in range(1, harmonics + 1))).astype(np.float32)


def worst_cents(x, hz):
    rec = M.track(x.astype(np.float64), YIN["W"], YIN["H"], YIN["tau_min"], YIN["tau_max"], YIN["threshold"])
    assert len(rec) == 4 and np.all(rec["voiced"] == 1), (hz, rec)
    assert np.all(rec["dip"] < YIN["threshold"]) and np.all(rec["energy"] > 0.0)
    return float(np.abs(1200.0 * np.log2(RATE / rec["period"] / hz)).max())


@pytest.mark.parametrize("kind", ["sine", "harmonic"])
def test_tones_are_voiced_in_every_hop_within_half_a_cent(kind):
    """nine tones of 55 .. 987.77 Hz at 48 kHz, W = 1024, lags 24 .. 1024, H = 256, threshold 0.15, 4 hops each: the limit
    is 0.5 cent (0.177 measured); an octave error would show as 1200"""
    n = YIN["W"] + YIN["tau_max"] + 3 * YIN["H"]
    worst = 0.0
    for hz in TONES:
        cents = worst_cents(sine(hz, n) if kind == "sine" else harmonic(hz, n), hz)
        worst = max(worst, cents)
        assert cents <= 0.5, (kind, hz, cents)
    print("%s: worst error %.3f cent" % (kind, worst))


def test_the_tune_tests_input_is_found_within_its_share_of_the_bound():
    """the 452 Hz 8-harmonic tone tests/test_gpu_f0.py tunes, and a 440 Hz one: within 0.18 cent, so that with pitch_ratio's
    0.4 the tuned sample's 1 cent holds"""
    n = YIN["W"] + YIN["tau_max"] + 3 * YIN["H"]
    for hz in (452.0, 440.0):
        assert worst_cents(harmonic(hz, n), hz) <= 0.18, hz


def test_noise_and_silence_are_unvoiced():
    rng = np.random.default_rng(1)
    rec = M.track(rng.standard_normal(3000).astype(np.float32).astype(np.float64), **{k: YIN[k] for k in ("W", "H", "tau_min", "tau_max", "threshold")})
    assert len(rec) == 4 and not rec["voiced"].any() and np.all(rec["dip"] > 0.5) and np.all(rec["dip"] < 1.0)
    assert np.all((rec["lag"] >= 24) & (rec["lag"] <= 1023))
    rec = M.track(np.zeros(3000), **{k: YIN[k] for k in ("W", "H", "tau_min", "tau_max", "threshold")})
    assert len(rec) == 4 and not rec["voiced"].any()
    assert np.all(rec["lag"] == 24) and np.all(rec["period"] == 24.0) and np.all(rec["dip"] == 1.0) and np.all(rec["energy"] == 0.0)


def test_the_run_of_8_prefix_stays_beside_a_flat_sum():
    """S in the header's two-level order against a flat ascending sum of the same dd: below 1e-12 relative"""
    rng = np.random.default_rng(0x5F0)
    worst = 0.0
    for tau_max in (8, 15, 63, 513, 1024, 4095):
        x = (rng.standard_normal(256 + tau_max) * np.exp(rng.standard_normal(256 + tau_max))).astype(np.float32).astype(np.float64)
        dd, _ = M.difference(x, [0], 256, tau_max)
        S = M.run_sums(dd[0])
        flat = np.zeros(tau_max + 1)
        acc = 0.0
        for t in range(tau_max + 1):
            acc = acc + dd[0][t]
            flat[t] = acc
        rel = float(np.max(np.abs(S[1:] - flat[1:]) / flat[1:]))
        worst = max(worst, rel)
        assert rel < 1e-12, (tau_max, rel)
        assert np.array_equal(S[:8], flat[:8])                      # the first run IS the flat sum
    print("worst relative difference %.3e" % worst)


def test_only_picks_hops_of_the_whole_track():
    rng = np.random.default_rng(7)
    x = (np.sin(2 * np.pi * np.arange(2000) / 37.3) + 0.1 * rng.standard_normal(2000)).astype(np.float32).astype(np.float64)
    full = M.track(x, 72, 7, 2, 63, 0.3)
    some = [0, 5, len(full) - 1, 3]
    part = M.track(x, 72, 7, 2, 63, 0.3, only=some, chunk=3)
    assert np.array_equal(part.view(np.uint64), np.ascontiguousarray(full[some]).view(np.uint64))


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def shape_of(Wn, H, tau_max):
    """wbx_f0.h's f0_shape and f0_span_words: (G, F, words)"""
    waves, G = -(-(tau_max + 1) // 512), 1
    while G < waves:
        G *= 2
    F = 8 // G
    words = lambda F: (F - 1) * H + Wn + 512 * G + 16
    while F > 1 and words(F) > 14336:
        F //= 2
    return G, F, words(F)


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/f0_main.cpp: wbx_f0.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "f0_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "f0_main.cpp"), "-o", exe])
    T = terms()
    lines, want = [], []
    for Wn, tau_max, H in [(64, 8, 1), (72, 15, 7), (256, 511, 64), (1024, 1024, 256), (8192, 4095, 1 << 20), (60, 8, 1), (64, 7, 1), (64, 8, 0)]:
        for n in (0, 1, Wn + tau_max - 1, Wn + tau_max, Wn + tau_max + 17 * max(H, 1), EDGE, (1 << 64) - 1):
            lines.append("h %d %d %d %d" % (n, Wn, H, tau_max))
            want.append("h %d" % M.hops(n, Wn, H, tau_max))
    for change, status in CHECKS:
        a = dict(OK, **change)
        cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["W"], a["H"], a["tau_max"])
        lines.append("c %d %d %d %d %d %r %d %d" % (a["n"], a["W"], a["H"], a["tau_min"], a["tau_max"], a["thr"], a["out"], cap))
        want.append("c %d" % status)
    shapes = set()
    for Wn in (64, 72, 256, 1024, 2048, 8192):
        for tau_max in (8, 15, 63, 511, 512, 513, 1023, 1024, 2047, 2048, 4095):
            lines.append("l %d %d" % (Wn, tau_max))
            want.append("l %d" % M.launch_hops(Wn, tau_max, T))
            for hops in (0, 1, 17, 1 << 20):
                lines.append("n %d %d %d" % (hops, Wn, tau_max))
                want.append("n %d" % M.launches(hops, Wn, tau_max, T))
            for H in (1, 7, 64, 512, 1000, 2000, 13000, 1 << 20):
                G, F, words = shape_of(Wn, H, tau_max)
                assert words <= 14336 and G * F <= 8 and 512 * G > tau_max
                shapes.add((G, F))
                lines.append("s %d %d %d" % (Wn, H, tau_max))
                want.append("s %d %d %d" % (G, F, words))
    assert {(1, 8), (1, 4), (1, 2), (1, 1), (2, 4), (2, 1), (4, 2), (4, 1), (8, 1)} <= shapes
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "f0 ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
