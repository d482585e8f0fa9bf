"""Convolving a clip, the part that needs no device: the symbols of include/wbx.h "Convolving a clip" exist and match their
binding twins, the adapter's method compiles, NULL handles are refused, wbx_convolve_frames counts, wbx_fir_design refuses
what the header says it refuses, equals the numpy twin (tests/convolve_model.py) BIT FOR BIT, is exactly symmetric and IS
the filter it claims to be — and wbx_convolve.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import convolve_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_fir_design", "wbx_convolve_frames", "wbx_convolve_tile_frames", "wbx_convolve_segment_taps", "wbx_convolve_ms",
       "wbx_clip_convolve", "wbx_engine_convolve_sample"]
RATES = (8000, 44100, 48000, 192000, 384000)
TAPS = (3, 255, 4095)
BETAS = (0.0, 5.0, 8.6, 14.0)
KIND_NAMES = ["lowpass", "highpass", "bandpass", "bandstop"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def lib_design(rate, kind, f1, f2, n_taps, beta, cap=None, out=None):
    """(status, the buffer): cap floats, 7.0f where nothing was written"""
    buf = np.full(n_taps if cap is None else cap, 7.0, dtype=np.float32) if out is None else out
    st = W.lib().wbx_fir_design(rate, kind, float(f1), float(f2), n_taps, float(beta), buf.ctypes.data, buf.size)
    return st, buf


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.fir_design) and callable(W.convolve_frames)
    assert hasattr(W.MixContext, "clip_convolve") and hasattr(W.Engine, "convolve_sample") and hasattr(W.Engine, "add_fir")
    assert L.wbx_convolve_tile_frames() == 2048 == M.TILE and L.wbx_convolve_segment_taps() == 2048 == M.SEGMENT
    text = re.sub(r"\s*\*\s*", " ", header)
    assert "Convolving a clip" in text and "FIR / convolution" not in text


def test_kinds_equal_the_headers(tmp_path):
    src = tmp_path / "kinds.c"
    src.write_text('#include <stdio.h>\n#include "wbx.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                   % (" ".join(["%d"] * 4), ", ".join("WBX_FIR_" + n.upper() for n in KIND_NAMES)))
    exe = str(tmp_path / "kinds")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [_ffi.FIR_KIND[n] for n in KIND_NAMES] == [M.KINDS[n] for n in KIND_NAMES] == list(range(4))


def test_adapter_with_convolve_compiles(tmp_path):
    """a translation unit that uses Engine::convolve_sample (never called: it would need a device); main runs the host calls"""
    src = tmp_path / "adapter_convolve.cpp"
    src.write_text('#include "wbx_adapter.hpp"\n'
                   'uint32_t lowpassed(wbx::Engine& e, uint32_t stem, uint32_t fir, uint64_t n) {\n'
                   '  wbx_clip_stats st{};\n'
                   '  return e.convolve_sample(stem, fir, 0, n, 0, 255, 127, n, 1.0, &st) + e.convolve_sample(stem, fir, 0, n, 0, 255, 0, n + 254);\n}\n'
                   'int main() {\n  float h[255];\n'
                   '  if (wbx_fir_design(48000, WBX_FIR_LOWPASS, 6000.0, 0.0, 255, 8.6, h, 255) != WBX_OK) return 1;\n'
                   '  if (h[0] != h[254] || !(h[127] > 0.2f)) return 2;\n'
                   '  if (wbx_convolve_frames(48000, 255) != 48254 || wbx_convolve_frames(0, 255) != 0) return 3;\n'
                   '  return wbx_convolve_tile_frames() == 2048 && wbx_convolve_segment_taps() == 2048 ? 0 : 4;\n}\n')
    exe = str(tmp_path / "adapter_convolve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx", "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.call([exe]) == 0


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    new, st, ms = C.c_uint32(77), _ffi.ClipStats(), C.c_double(5.0)
    assert L.wbx_clip_convolve(None, 0, 1, 2, 0, 64, 0, 8, 0, 71, 1.0, C.byref(st)) == -4
    assert L.wbx_engine_convolve_sample(None, 0, 1, 0, 64, 0, 8, 0, 71, 1.0, C.byref(new), C.byref(st)) == -4 and new.value == 77
    assert L.wbx_convolve_ms(None, C.byref(ms)) == -4 and ms.value == 5.0


def test_convolve_frames():
    for n, l in ((1, 1), (1, 7), (48000, 255), (10, 1 << 20), ((1 << 31) - 17, 4096), (1 << 40, 1 << 20), ((1 << 64) - (1 << 20), 1 << 20)):
        assert W.convolve_frames(n, l) == M.full_frames(n, l) == n + l - 1, (n, l)
    for n, l in ((0, 5), (5, 0), (0, 0), (5, (1 << 20) + 1), (5, 1 << 63), ((1 << 64) - 1, 2), ((1 << 64) - (1 << 20) + 1, 1 << 20)):
        assert W.convolve_frames(n, l) == M.full_frames(n, l) == 0, (n, l)


# ---- wbx_fir_design ---------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_design_writes_nothing():
    ok = dict(rate=48000, kind=M.BANDPASS, f1=3000.0, f2=9000.0, n_taps=255, beta=8.6)

    def refused(cap=None, **change):
        a = dict(ok, **change)
        st, buf = lib_design(a["rate"], a["kind"], a["f1"], a["f2"], a["n_taps"], a["beta"], cap=cap if cap is not None else 70000)
        assert st == -4 and np.all(buf == 7.0), change
        if cap is None:
            with pytest.raises(M.Refused):
                M.fir_design(a["rate"], a["kind"], a["f1"], a["f2"], a["n_taps"], a["beta"])

    assert lib_design(**ok)[0] == 0
    assert W.lib().wbx_fir_design(48000, M.BANDPASS, 3000.0, 9000.0, 255, 8.6, None, 255) == -4      # NULL out
    refused(cap=254)                                            # a capacity below n_taps
    refused(kind=4)
    refused(kind=-1)
    refused(rate=0)
    for n in (0, 1, 2, 4, 254, 65536, 65537, (1 << 32) - 1):    # even, or out of range
        refused(n_taps=n)
    for f in (0.0, -1.0, 24000.0, 30000.0, np.nan, np.inf):     # an edge not inside (0, rate / 2)
        refused(f1=f)
        refused(f2=f)
        refused(kind=M.LOWPASS, f1=f)
        refused(kind=M.HIGHPASS, f1=f)
    refused(f1=9000.0, f2=3000.0)                               # f2 <= f1 for the band kinds
    refused(f1=3000.0, f2=3000.0)
    refused(kind=M.BANDSTOP, f1=9000.0, f2=3000.0)
    for b in (-0.5, 14.5, np.nan, np.inf, -np.inf):
        refused(beta=b)
    # what is NOT refused: the limits themselves, and an f2 the kind does not look at
    for a in (dict(n_taps=3), dict(n_taps=65535), dict(beta=0.0), dict(beta=14.0), dict(kind=M.LOWPASS, f2=-5.0),
              dict(kind=M.HIGHPASS, f2=np.nan), dict(kind=M.LOWPASS, f1=23999.9)):
        b = dict(ok, **a)
        st, buf = lib_design(b["rate"], b["kind"], b["f1"], b["f2"], b["n_taps"], b["beta"])
        assert st == 0 and np.all(np.isfinite(buf)) and not np.any(buf == 7.0), a
    with pytest.raises(W.WbxError):
        W.fir_design(48000, "lowpass", 6000.0, n_taps=256)


@pytest.mark.parametrize("rate", RATES)
def test_designs_equal_the_model_bit_for_bit_and_are_symmetric(rate):
    n = 0
    for kind in range(4):
        for taps in TAPS:
            for beta in BETAS:
                for f1, f2 in ((0.125 * rate, 0.375 * rate), (1000.0, 0.45 * rate)):
                    st, got = lib_design(rate, kind, f1, f2, taps, beta)
                    want = M.fir_design(rate, kind, f1, f2, taps, beta)
                    assert st == 0 and same_bits(got, want), (rate, kind, taps, beta, f1, f2)
                    assert np.array_equal(got.view(np.uint32), got[::-1].view(np.uint32)), (rate, kind, taps, beta, f1, f2)
                    n += 1
    assert n == 4 * 3 * 4 * 2
    # ... and through the Python mirror, by name and with its defaults
    assert same_bits(W.fir_design(rate, "highpass", 0.1 * rate), M.fir_design(rate, M.HIGHPASS, 0.1 * rate, 0.0, 255, 8.6))
    assert same_bits(W.fir_design(rate, "bandstop", 0.1 * rate, 0.2 * rate, n_taps=31, beta=5.0),
                     M.fir_design(rate, "bandstop", 0.1 * rate, 0.2 * rate, 31, 5.0))


def test_the_longest_design_equals_the_model():
    st, got = lib_design(48000, M.BANDPASS, 300.0, 3400.0, 65535, 14.0)
    assert st == 0 and same_bits(got, M.fir_design(48000, M.BANDPASS, 300.0, 3400.0, 65535, 14.0))
    assert np.array_equal(got, got[::-1])


def test_a_design_writes_n_taps_floats_and_no_more():
    buf = np.full(300, 7.0, dtype=np.float32)
    st, _ = lib_design(48000, M.LOWPASS, 6000.0, 0.0, 255, 8.6, out=buf)
    assert st == 0 and np.all(buf[255:] == 7.0) and not np.any(buf[:255] == 7.0)


def response_db(h, rate, freqs):
    """|H(f)| in dB of the fp32 taps, by the defining sum in fp64 (numpy's exp: a measurement, not the twin)"""
    k = np.arange(len(h), dtype=np.float64)
    H = np.exp(-2j * np.pi * np.outer(np.asarray(freqs, dtype=np.float64), k) / rate) @ h.astype(np.float64)
    return 20.0 * np.log10(np.abs(H))


def test_what_a_design_is_worth():
    """48 kHz, 255 taps, beta 8.6, edges 6000 Hz or 3000 / 9000 Hz, every Hz from 0 to Nyquist.  The pass and stop bands begin
    half of Kaiser's transition width away from each edge: the width is (A - 7.95) / (14.36 * 254) * rate = 1037 Hz with
    A = 8.6 / 0.1102 + 8.7 = 86.7 dB, its half 518.5 Hz.  Measured with numpy's sin and i0: stop band at most -85.3 dB
    (asserted <= -84), pass band within 4.7e-4 dB (<= 1e-3), -6.0206 dB at every edge (within 0.01 dB)."""
    rate, half = 48000, 0.5 * (8.6 / 0.1102 + 8.7 - 7.95) / (14.36 * 254) * 48000
    assert abs(2 * half - 1037.0) < 1.0
    fs = np.arange(0.0, 24000.5, 1.0)
    worst = [0.0, -1000.0]
    for kind, edges in ((M.LOWPASS, (6000.0,)), (M.HIGHPASS, (6000.0,)), (M.BANDPASS, (3000.0, 9000.0)), (M.BANDSTOP, (3000.0, 9000.0))):
        h = W.fir_design(rate, kind, edges[0], edges[-1] if len(edges) > 1 else 0.0, n_taps=255, beta=8.6)
        db = response_db(h, rate, fs)
        if len(edges) == 1:
            below, above = fs <= edges[0] - half, fs >= edges[0] + half
            pas, stp = (below, above) if kind == M.LOWPASS else (above, below)
        else:
            inside, outside = (fs >= edges[0] + half) & (fs <= edges[1] - half), (fs <= edges[0] - half) | (fs >= edges[1] + half)
            pas, stp = (inside, outside) if kind == M.BANDPASS else (outside, inside)
        assert pas.sum() > 4000 and stp.sum() > 4000
        stop, ripple = float(db[stp].max()), float(np.abs(db[pas]).max())
        at_edges = [float(db[int(e)]) for e in edges]
        print(KIND_NAMES[kind], "stop band %.2f dB, pass band within %.2e dB, edges" % (stop, ripple), at_edges)
        assert stop <= -84.0, (kind, stop)
        assert ripple <= 1e-3, (kind, ripple)
        for v in at_edges:
            assert abs(v - 20.0 * np.log10(0.5)) <= 0.01, (kind, at_edges)
        worst = [max(worst[0], ripple), max(worst[1], stop)]
    assert worst[1] > -90.0 and worst[0] > 1e-4                 # (the bands are no easier than stated)


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def test_design_and_frames_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/convolve_main.cpp: wbx_convolve.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "convolve_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "convolve_main.cpp"), "-o", exe])
    hexd = lambda v: "%016x" % np.float64(v).view(np.uint64)
    hexf = lambda a: " ".join("%08x" % v for v in np.asarray(a, dtype=np.float32).view(np.uint32))
    lines, want = [], []
    for rate in (8000, 48000, 384000):
        for kind in range(4):
            for taps, beta in ((3, 0.0), (255, 8.6), (1023, 14.0)):
                f1, f2 = 0.1 * rate, 0.3 * rate
                lines.append("f %d %d %s %s %d %s %d" % (rate, kind, hexd(f1), hexd(f2), taps, hexd(beta), taps))
                want.append("f 0 " + hexf(M.fir_design(rate, kind, f1, f2, taps, beta)))
    for bad in ((0, 0, 100.0, 0.0, 255, 8.6, 255), (48000, 4, 100.0, 0.0, 255, 8.6, 255), (48000, 0, 100.0, 0.0, 255, 8.6, 254),
                (48000, 0, 100.0, 0.0, 256, 8.6, 256), (48000, 0, 24000.0, 0.0, 255, 8.6, 255), (48000, 2, 200.0, 100.0, 255, 8.6, 255),
                (48000, 0, 100.0, 0.0, 255, 14.5, 255), (48000, 0, np.nan, 0.0, 255, 8.6, 255), (48000, 0, 100.0, 0.0, 1, 8.6, 8)):
        lines.append("f %d %d %s %s %d %s %d" % (bad[0], bad[1], hexd(bad[2]), hexd(bad[3]), bad[4], hexd(bad[5]), bad[6]))
        want.append(("f -4 " + hexf(np.full(bad[6], 7.0))).strip())
    for n, l in ((5, 3), (0, 3), (3, 0), (7, 1 << 20), (7, (1 << 20) + 1), ((1 << 64) - 1, 2), ((1 << 64) - 1, 1)):
        lines.append("n %d %d" % (n, l))
        want.append("n %d" % M.full_frames(n, l))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "convolve ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
