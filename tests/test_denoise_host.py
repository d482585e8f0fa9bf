"""Reducing a clip's noise, the part that needs no device: the symbols of include/wbx.h "Reducing a clip's noise" exist and
match their binding twins, the struct has the header's layout, the adapter's methods compile, NULL handles are refused,
wbx_denoise_tables / _threshold / _hops / _profile_hops / _band_hops / _launches / _check equal the numpy twin
(tests/denoise_model.py), every refusal of the argument check one by one with the order where two apply, the model itself
shows that the transform pair is an identity, that a closed gate is the floor and what the gate does to noise under a
signal — and wbx_denoise.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import denoise_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_denoise_tables", "wbx_denoise_threshold", "wbx_denoise_hops", "wbx_denoise_profile_hops", "wbx_denoise_band_hops",
       "wbx_denoise_launches", "wbx_denoise_check", "wbx_denoise_ms", "wbx_clip_denoise_profile", "wbx_clip_denoise",
       "wbx_engine_denoise_sample", "wbx_engine_denoise_profile_sample"]
WINDOWS = [64, 256, 2048]


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hexd(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).reshape(-1).view(np.uint8).tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    for f in ("denoise_tables", "denoise_threshold", "denoise_hops", "denoise_band_hops"):
        assert callable(getattr(W, f)), f
    for f in ("clip_denoise", "clip_denoise_profile", "denoise_ms"):
        assert hasattr(W.MixContext, f), f
    for f in ("denoise_sample", "denoise_profile_sample", "reduce_noise_sample"):
        assert hasattr(W.Engine, f), f
    flat = re.sub(r"\s*\*\s*", " ", header)
    start, end = flat.index("Reducing a clip's noise: frames"), flat.index("Stretching a clip: frames")
    assert flat.index("Saturating a clip: frames") < start < end
    text = flat[start:end]
    for word in ("BIT FOR BIT", "no FFT", "ONE IEEE fp64 operation", "exactly four windows", "in this order", "MEASUREMENT",
                 "linked-stereo", "at render time", "windows above 2048", "de-hum", "click repair", "no NaN is ever produced"):
        assert word in text, word
    adapter = open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()
    assert "denoise_sample" in adapter and "denoise_profile_sample" in adapter
    make = open(os.path.join(ROOT, "whitebox_amd", "csrc", "Makefile")).read()
    assert make.count("wbx_denoise.hip") == 1 and make.count("wbx_denoise.h ") == 1 and re.search(r"for f in .*\bwbx_denoise\b", make)


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    fields = ["hops", "cells", "open_cells", "bands", "reserved"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(wbx_denoise_stats), ' + ", ".join("offsetof(wbx_denoise_stats, %s)" % f for f in fields)
                   + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.DenoiseStats
    assert got == [32, 0, 8, 16, 24, 28] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert re.search(r"wbx_denoise_stats\s*\{\s*/\* 32 bytes \*/", open(os.path.join(ROOT, "include", "wbx.h")).read())


def test_adapter_with_denoise_compiles(tmp_path):
    """tests/cpp/adapter_denoise.cpp uses Engine::denoise_sample and ::denoise_profile_sample; it is compiled and linked here
    and run by tests/test_gpu_denoise.py (it needs a device)"""
    exe = str(tmp_path / "adapter_denoise")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_denoise.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    thr = np.ones(2 * 33)
    st, ms, new, hops, sums = _ffi.DenoiseStats(), C.c_double(5.0), C.c_uint32(77), C.c_uint64(66), np.full(66, 5.5)
    st.hops, st.cells, st.open_cells, st.bands = 9, 8, 7, 6
    assert L.wbx_clip_denoise(None, 0, 0, 64, 64, 2, 1, thr.ctypes.data, 0.1, 1, C.byref(st)) == -4
    assert L.wbx_clip_denoise_profile(None, 0, 0, 64, 64, sums.ctypes.data, C.byref(hops)) == -4
    assert L.wbx_engine_denoise_sample(None, 0, 0, 64, 64, 2, 1, thr.ctypes.data, 0.1, C.byref(new), C.byref(st)) == -4
    assert L.wbx_engine_denoise_profile_sample(None, 0, 0, 64, 64, sums.ctypes.data, C.byref(hops)) == -4
    assert L.wbx_denoise_ms(None, C.byref(ms)) == -4 and ms.value == 5.0
    assert (st.hops, st.cells, st.open_cells, st.bands, new.value, hops.value) == (9, 8, 7, 6, 77, 66) and np.all(sums == 5.5)


# ---- the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", WINDOWS)
def test_tables_equal_the_model_bit_for_bit(win):
    a, y = W.denoise_tables(win)
    AC, AS, YC, YS = M.tables(win)
    for got, want, name in ((a[0], AC, "AC"), (a[1], AS, "AS"), (y[0], YC, "YC"), (y[1], YS, "YS")):
        bad = np.flatnonzero(bits32(got).reshape(-1) != bits32(want).reshape(-1))
        assert bad.size == 0, (win, name, bad[:4])
    # rows 0 and B - 1 of the sine tables are all +-0 (here: +0.0), which the device's packing rests on
    for t in (a[1], y[1]):
        assert np.all(bits32(t[0]) & 0x7FFFFFFF == 0) and np.all(bits32(t[-1]) & 0x7FFFFFFF == 0)
        assert np.all(bits32(t[0]) == 0) and np.all(bits32(t[-1]) == 0)
    # the window: its squares over four overlapping hops add up to 2; the analysis row 0 is the window over W
    s = y[0][0].astype(np.float64) / 0.5
    H = win // 4
    assert np.allclose(sum(s[u * H:(u + 1) * H] ** 2 for u in range(4)), 2.0, atol=1e-6)
    assert np.allclose(a[0][0].astype(np.float64) * win, s, rtol=1e-6)


def test_tables_refusals_write_nothing():
    L = W.lib()
    out = np.full(8, 7.0, np.float32)
    for win in (0, 32, 63, 96, 4096, 2049):
        assert L.wbx_denoise_tables(win, out.ctypes.data, out.ctypes.data) == -4 and np.all(out == 7.0), win
    assert L.wbx_denoise_tables(64, None, None) == -4
    only = np.zeros(2 * 33 * 64, np.float32)
    assert L.wbx_denoise_tables(64, None, only.ctypes.data) == 0 and np.array_equal(bits32(only[:33 * 64]), bits32(M.tables(64)[2]).reshape(-1))


def test_threshold_equals_the_model():
    rng = np.random.default_rng(0x7E5)
    sums = rng.uniform(0.0, 3.0, 66) * 10.0 ** rng.integers(-12, 3, 66)
    for hops, strength in ((1, 1.0), (13, 3.0), (1 << 20, 0.0), (7, 1e-3), (184, 2.5)):
        assert np.array_equal(bits64(W.denoise_threshold(sums, hops, strength)), bits64(M.threshold(sums, hops, strength)))
    L = W.lib()
    out = np.full(66, 7.0)
    for hops, strength, s, o in ((0, 1.0, sums, out), (5, -1.0, sums, out), (5, np.nan, sums, out), (5, np.inf, sums, out), (5, 1.0, None, out),
                                 (5, 1.0, sums, None)):
        st = L.wbx_denoise_threshold(None if s is None else s.ctypes.data, hops, 66, strength, None if o is None else o.ctypes.data)
        assert st == -4 and np.all(out == 7.0)


def test_hops_bands_and_launches_equal_the_model():
    L = W.lib()
    for win in (64, 128, 256, 512, 1024, 2048, 32, 96, 4096):
        H = max(win // 4, 1)
        for n in (0, 1, H - 1, H, H + 1, win - 1, win, win + 1, 5 * H + 3, 1 << 20, (1 << 31) - 17, (1 << 31) - 16, 1 << 33):
            assert W.denoise_hops(n, win) == M.hops(n, win), (n, win)
            assert L.wbx_denoise_profile_hops(n, win) == M.profile_hops(n, win), (n, win)
            for ch in (0, 1, 2, 3):
                assert W.denoise_band_hops(win, ch) == M.band_hops(win, ch), (win, ch)
                assert L.wbx_denoise_launches(n, win, ch) == M.launches(n, win, ch), (n, win, ch)
    assert W.denoise_hops(1, 64) == 4 and W.denoise_hops(16, 64) == 4 and W.denoise_hops(17, 64) == 5
    assert W.denoise_band_hops(64, 2) == 32757 and W.denoise_band_hops(2048, 2) == 1013
    per = W.denoise_band_hops(64, 2)
    assert [L.wbx_denoise_launches(b * 16, 64, 2) for b in (per, per + 1, 2 * per, 2 * per + 1)] == [1, 2, 2, 3]


# ---- the check ------------------------------------------------------------------------------------------------------------------
OK = dict(n=4096, win=256, S=2, F=1, thr="good", ch=2, floor=0.1, at=0, entry=1.0)
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=(1 << 31) - 16), -4), (dict(n=(1 << 31) - 17), 0), (dict(n=1), 0),
          (dict(win=32), -4), (dict(win=96), -4), (dict(win=4096), -4), (dict(win=64), 0), (dict(win=2048), 0), (dict(win=0), -4),
          (dict(S=5), -4), (dict(S=4), 0), (dict(S=0), 0), (dict(F=9), -4), (dict(F=8), 0), (dict(F=0), 0), (dict(thr=None), -4),
          (dict(entry=-1e-300), -4), (dict(entry=np.nan), -4), (dict(entry=np.inf), -4), (dict(entry=-np.inf), -4), (dict(entry=0.0), 0),
          (dict(entry=-0.0), 0), (dict(entry=1.7e308), 0), (dict(at=128, entry=np.nan), -4), (dict(at=129, entry=np.nan), -4),
          (dict(at=257, entry=-1.0), -4), (dict(at=129, entry=np.nan, ch=1), 0),      # the second row is not read for one channel
          (dict(floor=-1e-9), -4), (dict(floor=1.0000001), -4), (dict(floor=np.nan), -4), (dict(floor=np.inf), -4), (dict(floor=0.0), 0),
          (dict(floor=1.0), 0), (dict(floor=-0.0), 0),
          # the order: n, the window, S, F, a NULL thr, its entries, the floor — each pair refused as the first would be alone
          (dict(n=0, win=96), -4), (dict(win=96, S=5), -4), (dict(S=5, F=9), -4), (dict(F=9, thr=None), -4), (dict(thr=None, floor=2.0), -4),
          (dict(entry=np.nan, floor=2.0), -4)]
ORDER = [(dict(n=0, win=96), "no frames"), (dict(win=96, S=5), "power of two"), (dict(S=5, F=9), "smooth_hops"), (dict(F=9, thr=None), "smooth_bins"),
         (dict(thr=None, floor=2.0), "threshold is NULL"), (dict(entry=np.nan, floor=2.0), "threshold entry"), (dict(floor=2.0), "floor")]


def thr_of(a):
    if a["thr"] is None:
        return None
    win = a["win"] if M.window_ok(a["win"]) else 64
    t = np.ones(2 * (win // 2 + 1))
    if a["at"] < t.size:
        t[a["at"]] = a["entry"]
    return t


def test_every_refusal_of_the_check_one_by_one():
    L = W.lib()
    for change, status in CHECKS:
        a = dict(OK, **change)
        t = thr_of(a)
        got = L.wbx_denoise_check(a["n"], a["win"], a["S"], a["F"], None if t is None else t.ctypes.data, a["ch"], float(a["floor"]))
        assert got == status == M.check(a["n"], a["win"], a["S"], a["F"], t, a["ch"], a["floor"]), (change, got)


def test_profile_check_equals_the_model():
    for n, win in ((0, 64), (63, 64), (64, 64), (1 << 20, 2048), (2047, 2048), ((1 << 31) - 16, 64), (4096, 100)):
        assert (W.lib().wbx_denoise_profile_hops(n, win) == 0) == (M.profile_check(n, win) != 0), (n, win)


# ---- the model's properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [64, 256, 1024])
def test_identity_and_all_floor_on_the_model(win):
    """thr = 0 returns the source (the model measures 3.8e-8 / 3.4e-8 / 6.9e-8 of the peak at W = 64 / 256 / 1024 on this
    noise: the fp32 roundings of the tables, the cells and the result), thr = 1e30 with floor 0.25 a quarter of it
    (9.6e-9 / 8.6e-9 / 1.7e-8)"""
    n, B = 5 * win + 37, win // 2 + 1
    x = (0.25 * np.random.default_rng(win).standard_normal(n)).astype(np.float32)
    peak = np.max(np.abs(x)).astype(np.float64)
    out, n_open = M.denoise_channel(x, win, 2, 1, np.zeros(B), 0.1)
    err = np.max(np.abs(out.astype(np.float64) - x)) / peak
    print("identity W %d: %.3g of the peak" % (win, err))
    assert err <= 1e-7 and n_open == M.hops(n, win) * B
    out, n_open = M.denoise_channel(x, win, 2, 1, np.full(B, 1e30), 0.25)
    err = np.max(np.abs(out.astype(np.float64) - 0.25 * x.astype(np.float64))) / peak
    print("all floor W %d: %.3g of the peak" % (win, err))
    assert err <= 5e-8 and n_open == 0


def test_the_gate_lowers_the_noise_and_keeps_the_signal():
    """2 s at 48 kHz: three decaying harmonic bursts over N(0, 0.01^2) noise, the profile from a separate second of the
    same noise, W = 1024, S = 2, F = 1, strength 3, floor 0.1"""
    rate, n, win = 48000, 96000, 1024
    rng = np.random.default_rng(0xD3)
    t = np.arange(n, dtype=np.float64) / rate
    clean = np.zeros(n)
    for start, f0 in ((0.5, 220.0), (1.0, 330.0), (1.5, 440.0)):
        on = t >= start
        env = np.where(on, np.exp(-(t - start) / 0.15), 0.0)
        for h in range(1, 5):
            clean += env * (0.3 / h) * np.sin(2 * np.pi * f0 * h * (t - start))
    noisy = (clean + 0.01 * rng.standard_normal(n)).astype(np.float32)
    noise = (0.01 * rng.standard_normal(rate)).astype(np.float32)
    sums, hops = M.profile_clip([noise], 0, rate, win)
    thr = M.threshold(sums, hops, 3.0)
    x = M.inputs(noisy)
    T, H, B = M.hops(n, win), win // 4, win // 2 + 1
    r, i = M.cells(x, win, (np.arange(T, dtype=np.int64) - M.LEAD) * H)
    mr, mi, is_open = M.gate(r, i, 2, 1, thr, 0.1)
    out = M.overlap_add(M.chains(mr, mi, win), n, win).astype(np.float64)
    quiet = rate // 4
    drop = 10.0 * np.log10(np.sum(noisy[:quiet].astype(np.float64) ** 2) / np.sum(out[:quiet] ** 2))
    head = quiet // H - 3                                          # the hops that lie wholly in the first quarter second
    share = is_open[:head].mean()
    snr_in = 10.0 * np.log10(np.sum(clean ** 2) / np.sum((noisy - clean) ** 2))
    snr_out = 10.0 * np.log10(np.sum(clean ** 2) / np.sum((out - clean) ** 2))
    _, _, open_plain = M.gate(r, i, 0, 0, thr, 0.1)
    share_plain = open_plain[:head].mean()
    print("drop %.2f dB, open share %.4f %% (unsmoothed %.3f %%), SNR %.2f -> %.2f dB" % (drop, 100 * share, 100 * share_plain, snr_in, snr_out))
    assert drop >= 19.0
    assert share < 0.01
    assert snr_out - snr_in >= 10.0
    assert share_plain > share


# ---- the header alone -----------------------------------------------------------------------------------------------------------
def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/denoise_main.cpp: wbx_denoise.h alone, stand-alone (its own main): the tables, the device's packing of them,
    the hop counts, the bands, the launch shape, the threshold and the two checks"""
    exe = str(tmp_path / "denoise_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "denoise_main.cpp"), "-o", exe])
    lines, want = [], []
    for win in (64, 256):
        AC, AS, YC, YS = M.tables(win)
        lines.append("t %d" % win)
        want.append("t 0 %016x %016x" % (fnv(np.concatenate([AC.reshape(-1), AS.reshape(-1)])), fnv(np.concatenate([YC.reshape(-1), YS.reshape(-1)]))))
        # the device's tables, restated from the model's: a cell row's words, a masked row's words
        half = win // 2
        A, Y = np.zeros((win, win), np.float32), np.zeros((win, win), np.float32)
        A[:, 0], A[:, 1] = AC[0], AC[half]
        A[:, 2::2], A[:, 3::2] = AC[1:half].T, AS[1:half].T
        Y[0], Y[win - 1] = YC[0], YC[half]
        Y[1:win - 1:2], Y[2:win - 1:2] = YC[1:half], YS[1:half]
        lines.append("d %d" % win)
        want.append("d %016x %016x" % (fnv(A), fnv(Y)))
    for win in (32, 96, 4096):
        lines.append("t %d" % win)
        want.append("t -4 %016x %016x" % (fnv(np.full(1, 7.0, np.float32)), fnv(np.full(1, 7.0, np.float32))))
    for win in (64, 2048, 100):
        for n in (0, 1, win - 1, win, 5 * (win // 4) + 3, (1 << 31) - 17, (1 << 31) - 16):
            lines.append("h %d %d" % (n, win))
            want.append("h %d %d" % (M.hops(n, win), M.profile_hops(n, win)))
            for ch in (1, 2, 3):
                lines.append("b %d %d %d" % (n, win, ch))
                want.append("b %d %d" % (M.band_hops(win, ch), M.launches(n, win, ch)))
    shapes = {64: (1, 1, 32, 64, 1), 128: (1, 1, 32, 128, 1), 256: (2, 1, 16, 256, 1), 512: (2, 2, 8, 512, 1), 1024: (2, 4, 4, 512, 1),
              2048: (2, 4, 4, 512, 2)}
    for win, s in shapes.items():
        lines.append("s %d" % win)
        want.append("s %d %d %d %d %d" % s)
    sums = np.random.default_rng(5).uniform(0.0, 1e-3, 5)
    for hops, strength, status in ((13, 3.0, 0), (0, 1.0, -4), (4, -1.0, -4), (4, np.nan, -4)):
        lines.append("q %d %s %d %s" % (hops, hexd(strength), sums.size, " ".join(hexd(v) for v in sums)))
        out = M.threshold(sums, hops, strength) if status == 0 else np.full(sums.size, 7.0)
        want.append("q %d %s" % (status, " ".join(hexd(v) for v in out)))
    for change, status in CHECKS:
        a = dict(OK, **change)
        lines.append("c %d %d %d %d %d %d %s %d %s" % (a["n"], a["win"], a["S"], a["F"], a["thr"] is not None, a["ch"], hexd(a["floor"]), a["at"],
                                                       hexd(a["entry"])))
        want.append("c %d" % status)
    for n, win, hs, hh, status in ((64, 64, 1, 1, 0), (0, 64, 1, 1, -4), (63, 64, 1, 1, -4), (64, 96, 1, 1, -4), (64, 64, 0, 1, -4), (64, 64, 1, 0, -4),
                                   ((1 << 31) - 16, 64, 1, 1, -4)):
        lines.append("p %d %d %d %d" % (n, win, hs, hh))
        want.append("p %d" % status)
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    got = subprocess.check_output([exe, str(cases)], timeout=120).decode().strip().split("\n")
    assert got[-1] == "denoise ok"
    assert got[:-1] == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_the_refusals_order_is_the_headers():
    """the call's own message names the FIRST reason (the order of wbx.h): read through a context-free path, the engine's
    NULL handle has no message, so the order is checked where a message exists — tests/test_gpu_denoise.py — and here by
    status and by the stand-alone program's `why`; this test pins the reasons' texts in the header's order"""
    src = open(os.path.join(ROOT, "whitebox_amd", "csrc", "wbx_denoise.h")).read()
    body = src[src.index("inline wbx_status denoise_check_args"):src.index("inline wbx_status denoise_profile_check_args")]
    at = [body.index(text) for _, text in ORDER]
    assert at == sorted(at), at
