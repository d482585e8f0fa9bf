"""Saturating a clip, the part that needs no device: the symbols of include/wbx.h "Saturating a clip" exist and match their
binding twins, the struct has the header's layout, the adapter's method compiles, NULL handles are refused,
wbx_saturate_table / _check / _lookup / _launch_shape equal the numpy twin (tests/saturate_model.py), every refusal of the
argument check one by one with the order where two apply, the model itself shows what oversampling buys (aliasing falls by more
than 8 dB per doubling) and what it costs (the band-limited result overshoots) — and wbx_saturate.h runs stand-alone under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import saturate_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_saturate_table", "wbx_saturate_check", "wbx_saturate_lookup", "wbx_saturate_launch_shape", "wbx_saturate_ms",
       "wbx_clip_saturate", "wbx_engine_saturate_sample"]
KINDS = {"hard": M.HARD, "cubic": M.CUBIC, "tanh": M.TANH}
BIASES = [0.0, 0.25, -4.0]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def hand_drawn(seed=0x5A7):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, M.TABLE)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    for f in ("saturate_table", "saturate_check", "saturate_lookup", "saturate_launch_shape"):
        assert callable(getattr(W, f)), f
    assert hasattr(W.MixContext, "clip_saturate") and hasattr(W.MixContext, "saturate_ms")
    assert hasattr(W.Engine, "saturate_sample") and hasattr(W.Engine, "soft_clip_sample")
    flat = re.sub(r"\s*\*\s*", " ", header)
    start, end = flat.index("Saturating a clip: frames"), flat.index("Stretching a clip: frames")
    assert flat.index("Dynamics of a clip: frames") < start < end
    text = flat[start:end]
    for word in ("BY DEFINITION", "NO CEILING GUARANTEE", "wbx_clip_limit", "No NaN and no infinity", "in this order", "at render time",
                 "oversampling above 8", "unlinked per-channel tables", "true-peak-safe", "T = 768 > 512", "NOT shape(0)"):
        assert word in text, word
    assert re.search(r"#define\s+WBX_SAT_TABLE\s+16385", header) and _ffi.SAT_TABLE == M.TABLE == 16385
    assert re.search(r"WBX_SAT_HARD = 0, WBX_SAT_CUBIC = 1, WBX_SAT_TANH = 2", header) and _ffi.SAT_KIND == KINDS
    assert "saturate_sample" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()
    make = open(os.path.join(ROOT, "whitebox_amd", "csrc", "Makefile")).read()
    assert make.count("wbx_saturate.hip") == 1 and make.count("wbx_saturate.h ") == 1 and re.search(r"for f in .*\bwbx_saturate\b", make)


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    fields = ["peak_drive", "peak_index", "beyond"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * len(fields)
                   + '\\n", sizeof(wbx_saturate_stats), ' + ", ".join("offsetof(wbx_saturate_stats, %s)" % f for f in fields)
                   + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.SaturateStats
    assert got == [24, 0, 8, 16] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert re.search(r"wbx_saturate_stats\s*\{\s*/\* 24 bytes \*/", open(os.path.join(ROOT, "include", "wbx.h")).read())


def test_adapter_with_saturate_compiles(tmp_path):
    """tests/cpp/adapter_saturate.cpp uses Engine::saturate_sample; it is compiled and linked here and run by
    tests/test_gpu_saturate.py (it needs a device)"""
    exe = str(tmp_path / "adapter_saturate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_saturate.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    tab = hand_drawn()
    ss, ms, new = _ffi.SaturateStats(), C.c_double(5.0), C.c_uint32(77)
    ss.peak_drive, ss.peak_index, ss.beyond = 9.0, 8, 7
    assert L.wbx_clip_saturate(None, 0, 1, 0, 16, 4, 1, tab.ctypes.data, 1.0, 1.0, C.byref(ss), None) == -4
    assert L.wbx_engine_saturate_sample(None, 0, 0, 16, 4, 1, tab.ctypes.data, 1.0, 1.0, C.byref(new), C.byref(ss), None) == -4
    assert L.wbx_saturate_ms(None, C.byref(ms)) == -4 and ms.value == 5.0
    assert (ss.peak_drive, ss.peak_index, ss.beyond, new.value) == (9.0, 8, 7, 77)


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_table_equals_the_model_bit_for_bit(kind):
    for bias in BIASES:
        got, want = W.saturate_table(kind, bias), M.table(KINDS[kind], bias)
        bad = np.flatnonzero(bits64(got) != bits64(want))
        assert bad.size == 0, (kind, bias, bad[:4], got[bad[:4]], want[bad[:4]])
        assert M.check(got) == 0
        W.saturate_check(got)
    t = W.saturate_table(kind, 0.25)
    assert np.all(np.diff(t) >= 0.0) and t[0] < -0.9 and t[-1] > 0.7     # monotone, asymmetric: f(v + b) - f(b)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bias_zero_is_bitwise_odd_with_an_exact_zero_in_the_middle(kind):
    t = W.saturate_table(kind)
    assert struct.pack("<d", t[8192]) == struct.pack("<d", 0.0)          # +0.0, not -0.0
    assert np.array_equal(bits64(t[8193:]), bits64(-t[:8192][::-1]))
    assert t[-1] == 1.0 or kind == "tanh" and 1.0 - 1e-6 < t[-1] <= 1.0
    unit = 8192 + 1024                                                    # the level 1.0
    assert {"hard": t[unit] == 1.0, "cubic": t[unit] == 1.0 - 4.0 / 27.0, "tanh": abs(t[unit] - np.tanh(1.0)) < 1e-15}[kind]
    assert abs(t[8192 + 100] - {"hard": 100 / 1024, "cubic": 100 / 1024 - 4 / 27 * (100 / 1024) ** 3, "tanh": np.tanh(100 / 1024)}[kind]) < 1e-15


def test_table_design_refusals_write_nothing():
    L = W.lib()
    out = np.full(M.TABLE, 7.0)
    for kind, bias, cap in ((3, 0.0, M.TABLE), (-1, 0.0, M.TABLE), (0, 4.0000001, M.TABLE), (1, -4.5, M.TABLE), (2, np.nan, M.TABLE),
                            (2, np.inf, M.TABLE), (0, 0.0, M.TABLE - 1), (0, 0.0, 0)):
        assert L.wbx_saturate_table(kind, bias, out.ctypes.data, cap) == -4 and np.all(out == 7.0), (kind, bias, cap)
        if cap == M.TABLE:
            with pytest.raises(M.Refused):
                M.table(kind, bias)
    assert L.wbx_saturate_table(0, 0.0, None, M.TABLE) == -4
    assert L.wbx_saturate_table(0, 4.0, out.ctypes.data, M.TABLE) == 0 and L.wbx_saturate_table(2, -4.0, out.ctypes.data, M.TABLE) == 0


def test_check_refuses_inf_nan_and_two_to_the_33():
    L = W.lib()
    good = hand_drawn()
    assert L.wbx_saturate_check(good.ctypes.data) == 0 == M.check(good) and L.wbx_saturate_check(None) == -4
    for at in (0, 8192, M.TABLE - 1):
        for v, want in ((np.inf, -4), (-np.inf, -4), (np.nan, -4), (2.0 ** 33, -4), (-2.0 ** 33, -4), (np.nextafter(2.0 ** 32, 1e99), -4),
                        (2.0 ** 32, 0), (-2.0 ** 32, 0), (-0.0, 0), (5e-324, 0)):
            t = good.copy()
            t[at] = v
            assert L.wbx_saturate_check(t.ctypes.data) == want == M.check(t), (at, v)
            if want:
                with pytest.raises(W.WbxError):
                    W.saturate_check(t)


# ---- the lookup --------------------------------------------------------------------------------------------------------------
def lookup_points():
    edges = (np.arange(M.TABLE, dtype=np.float64) - 8192.0) / 1024.0       # every cell edge: f == 0 there
    eps = np.finfo(np.float64).eps
    tiny = [-5e-324, -1e-300, -2.0 ** -64, -2.0 ** -63, -eps / 1024.0, -eps / 4096.0]       # a - floor(a) rounds to 1.0
    near = [np.nextafter(8.0, 0.0), np.nextafter(-8.0, 0.0), np.nextafter(8.0, 9.0), np.nextafter(-8.0, -9.0), 8.0, -8.0]
    other = [0.0, -0.0, 5e-324, 1e30, -1e30, np.inf, -np.inf, 2.0 ** 32 * 3.4e38, 0.3, -0.3, 1.0 / 3.0, -7.99951171875 + 1e-9]
    rnd = np.random.default_rng(0x100C).uniform(-8.5, 8.5, 4000)
    return np.concatenate([edges, np.nextafter(edges, 9.0), np.nextafter(edges, -9.0), tiny, near, other, rnd])


def test_lookup_equals_the_model_at_every_edge_and_corner():
    L = W.lib()
    tab = hand_drawn()
    d = lookup_points()
    want, past = M.lookup(tab, d)
    got = np.zeros_like(d)
    out = C.c_double()
    for i, v in enumerate(d):
        assert L.wbx_saturate_lookup(tab.ctypes.data, float(v), C.byref(out)) == 0
        got[i] = out.value
    bad = np.flatnonzero(bits64(got) != bits64(want))
    assert bad.size == 0, (bad[:4], d[bad[:4]], got[bad[:4]], want[bad[:4]])
    # what the points are for
    assert np.array_equal(bits64(want[:M.TABLE]), bits64(np.concatenate([tab[:1], tab[1:-1], tab[-1:]])))     # an edge gives its entry
    a = -5e-324 * 1024.0
    assert a - np.floor(a) == 1.0 and W.saturate_lookup(tab, -5e-324) == tab[8191] + 1.0 * (tab[8192] - tab[8191])
    assert W.saturate_lookup(tab, 8.0) == tab[-1] and W.saturate_lookup(tab, -8.0) == tab[0]
    assert W.saturate_lookup(tab, np.nextafter(8.0, 0.0)) != tab[-1] and W.saturate_lookup(tab, 0.0) == W.saturate_lookup(tab, -0.0) == tab[8192]
    assert past[M.TABLE - 1] and past[0] and not past[1] and int(past.sum()) > 100
    # refusals: a NaN, NULLs; out untouched
    out.value = 3.0
    assert L.wbx_saturate_lookup(tab.ctypes.data, float("nan"), C.byref(out)) == -4 and out.value == 3.0
    assert L.wbx_saturate_lookup(None, 0.5, C.byref(out)) == -4 and L.wbx_saturate_lookup(tab.ctypes.data, 0.5, None) == -4


# ---- the call's check --------------------------------------------------------------------------------------------------------
TOP = (1 << 31) - 16
OK = dict(n=4096, os=4, q=M.GOOD, tab="good", drive=1.0, makeup=1.0)
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=1), 0),
          (dict(os=0), -4), (dict(os=3), -4), (dict(os=16), -4), (dict(os=1), 0), (dict(os=2), 0), (dict(os=8), 0),
          (dict(q=-1), -4), (dict(q=3), -4), (dict(q=M.FAST), 0), (dict(q=M.BEST), 0), (dict(os=1, q=3), -4),
          (dict(tab=None), -4), (dict(tab="inf"), -4), (dict(tab="nan"), -4), (dict(tab="big"), -4), (dict(tab="edge"), 0),
          (dict(drive=0.0), -4), (dict(drive=-0.0), -4), (dict(drive=np.nan), -4), (dict(drive=np.inf), -4), (dict(drive=2.0 ** 32), 0),
          (dict(drive=-2.0 ** 32), 0), (dict(drive=np.nextafter(2.0 ** 32, 1e99)), -4), (dict(drive=5e-324), 0),
          (dict(makeup=0.0), 0), (dict(makeup=-0.0), 0), (dict(makeup=-3.0), 0), (dict(makeup=2.0 ** 32), 0), (dict(makeup=-2.0 ** 32), 0),
          (dict(makeup=np.nextafter(2.0 ** 32, 1e99)), -4), (dict(makeup=np.nan), -4), (dict(makeup=-np.inf), -4),
          (dict(os=1, n=TOP - 1), 0), (dict(os=1, n=TOP), -4), (dict(os=2, n=TOP // 2 - 1), 0), (dict(os=2, n=TOP // 2), -4),
          (dict(os=8, n=TOP // 8 - 1), 0), (dict(os=8, n=TOP // 8), -4), (dict(n=1 << 62), -4), (dict(n=(1 << 64) - 1), -4),
          (dict(os=8, q=M.BEST), -3), (dict(os=4, q=M.BEST), 0), (dict(os=1, q=M.BEST), 0),
          # the order: n, os, quality, the table, drive, makeup, the length — all INVALID — and only then the plans
          (dict(n=0, os=3), -4), (dict(os=3, q=7), -4), (dict(q=7, tab=None), -4), (dict(tab="nan", drive=0.0), -4),
          (dict(drive=0.0, makeup=np.nan), -4), (dict(makeup=np.nan, n=TOP), -4),
          (dict(os=8, q=M.BEST, n=0), -4), (dict(os=8, q=M.BEST, tab=None), -4), (dict(os=8, q=M.BEST, drive=0.0), -4),
          (dict(os=8, q=M.BEST, makeup=np.inf), -4), (dict(os=8, q=M.BEST, n=TOP // 8), -4)]


def tables():
    good = hand_drawn()
    out = {"good": good, None: None}
    for name, v in (("inf", np.inf), ("nan", np.nan), ("big", 2.0 ** 33), ("edge", -2.0 ** 32)):
        out[name] = good.copy()
        out[name][12345] = v
    return out


def model_check(a, tabs):
    """the model's verdict.  The library's own check needs a context for the call itself, so without a device it is reached
    through the launch shape (n, os, quality: below) and through the stand-alone program, which runs wbx_saturate.h's
    saturate_check_args on every one of these cases (the last test of this file); tests/test_gpu_saturate.py runs them
    through wbx_clip_saturate"""
    t = tabs[a["tab"]]
    return M.check_args(a["n"], a["os"], a["q"], t, a["drive"], a["makeup"])


def test_check_every_refusal_one_by_one_in_the_model_and_the_shape_getter():
    tabs = tables()
    L = W.lib()
    v = [C.c_uint32() for _ in range(5)]
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert model_check(a, tabs) == want, change
        if not set(change) & {"tab", "drive", "makeup"}:           # what the shape getter judges too, with the same statuses
            assert L.wbx_saturate_launch_shape(a["os"], a["q"], 2, a["n"], *[C.byref(x) for x in v]) == want, change
    assert {w for _, w in CHECKS} == {0, -4, -3}


def test_launch_shape_over_the_grid():
    L = W.lib()
    seen = set()
    for os_ in (1, 2, 4, 8):
        for q in (M.FAST, M.GOOD, M.BEST):
            for ch in (1, 2):
                for n in (1, 255, 256, 1023, 1024, 1025, 100000, TOP // os_ - 1):
                    if os_ == 8 and q == M.BEST:
                        with pytest.raises(W.WbxError) as e:
                            W.saturate_launch_shape(os_, q, ch, n)
                        assert e.value.status == -3
                        continue
                    s = W.saturate_launch_shape(os_, q, ch, n)
                    assert s == M.launch_shape(os_, q, ch, n), (os_, q, ch, n)
                    Z = M.RM.QUALITY[q][0]
                    assert s["tile"] % 256 == 0 and 256 <= s["tile"] <= 1024 and s["lds_bytes"] <= 65536 and s["n_tiles"] == -(-n // s["tile"]) <= 1 << 21
                    if os_ > 1:
                        assert s["lds_bytes"] == ch * 4 * ((s["tile"] + 2 * Z) * os_ + s["tile"] + 4 * Z) and 2 * s["lds_bytes"] <= 160 * 1024
                        assert s["mid_span"] == (s["tile"] + 2 * Z) * os_ and s["src_span"] == s["tile"] + 4 * Z - 1
                        # the greatest such tile
                        assert s["tile"] == 1024 or ch * 4 * ((s["tile"] + 256 + 2 * Z) * os_ + s["tile"] + 256 + 4 * Z) > 65536
                        assert (s["tile"] + 2 * Z) / s["tile"] <= 1.19          # the halo the up conversion recomputes
                    else:
                        assert (s["tile"], s["mid_span"], s["src_span"], s["lds_bytes"]) == (1024, 1024, 1024, 0)
                    seen.add(s["tile"])
    assert seen == {768, 1024}
    v = [C.c_uint32() for _ in range(5)]
    p = [C.byref(x) for x in v]
    assert L.wbx_saturate_launch_shape(4, 1, 0, 100, *p) == -4 and L.wbx_saturate_launch_shape(4, 1, 3, 100, *p) == -4
    assert L.wbx_saturate_launch_shape(4, 1, 2, 100, None, *p[1:]) == -4 and L.wbx_saturate_launch_shape(4, 1, 2, 100, *p[:4], None) == -4


# ---- properties of the model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clipped_sine():
    """x = 0.5 sin(2 pi 601 t / 8192) through a hard table at drive 8, makeup 1, GOOD: per os the ratio in dB of the
    non-harmonic to the harmonic RMS over the rfft of 8192 analysed frames (1024 of run-in and run-out beside them; the
    harmonic bins are the multiples of 601 below Nyquist), and the result's peak"""
    N, K, PAD = 8192, 601, 1024
    t = np.arange(-PAD, N + PAD, dtype=np.float64)
    x = (0.5 * np.sin(2.0 * np.pi * K * t / N)).astype(np.float32)
    tab = M.table(M.HARD)
    out = {}
    for os_ in (1, 2, 4, 8):
        y, st = M.saturate([x], 0, len(x), os_, M.GOOD, tab, drive=8.0, makeup=1.0)
        assert 3.9 < st["peak_drive"] < 4.2 and st["beyond"] == 0             # 8 * 0.5, and what the up filter adds
        spec = np.abs(np.fft.rfft(y[0][PAD:PAD + N].astype(np.float64))) ** 2
        harm = np.zeros(len(spec), dtype=bool)
        harm[np.arange(K, N // 2, K)] = True
        harm[0] = False
        rest = ~harm
        rest[0] = False
        out[os_] = (10.0 * np.log10(spec[rest].sum() / spec[harm].sum()), float(np.max(np.abs(y[0]))))
    return out


def test_each_doubling_of_os_buys_at_least_8_db_of_aliasing(clipped_sine):
    """measured on this model: -21.1 / -41.3 / -53.1 / -64.1 dB at os 1 / 2 / 4 / 8 (steps of 20.2, 11.8, 11.0)"""
    r = {k: v[0] for k, v in clipped_sine.items()}
    print("non-harmonic / harmonic, dB:", {k: round(v, 2) for k, v in r.items()})
    assert r[1] > -30.0                                            # the input really aliases at the clip's own rate
    for lo, hi in ((1, 2), (2, 4), (4, 8)):
        assert r[lo] - r[hi] >= 8.0, (lo, hi, r)


def test_the_band_limited_result_overshoots_the_curve(clipped_sine):
    """no ceiling guarantee: the hard table never gives more than 1.0, the band-limited result peaks above 1.1 at os 4
    (measured: 1.156) — what soft_clip_sample(guarantee=True) puts a limiter behind"""
    print("peaks:", {k: round(v[1], 4) for k, v in clipped_sine.items()})
    assert clipped_sine[1][1] == 1.0 and clipped_sine[4][1] > 1.1


def test_the_composition_is_the_three_models_in_a_row_and_counts_every_mid_sample_once():
    rng = np.random.default_rng(0xC0)
    x = [rng.uniform(-1.0, 1.0, 700).astype(np.float32) for _ in range(2)]
    x[1][300] = np.float32(np.nan)
    tab = hand_drawn()
    y, st = M.saturate(x, 100, 500, 4, M.FAST, tab, drive=20.0, makeup=0.5)
    u = M.RM.resample(x, 100, 500, 1, 4, M.FAST)
    s, st2 = M.shape(u, tab, 20.0, 0.5)
    back = M.RM.resample(s, 0, 2000, 4, 1, M.FAST)
    assert st == st2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(y, back))
    assert all(len(p) == 500 and np.all(np.isfinite(p)) for p in y)
    d = [np.where(np.isfinite(p), 20.0 * p.astype(np.float64), 0.0) for p in u]
    assert st["beyond"] == sum(int(np.sum(np.abs(p) >= 8.0)) for p in d) > 0 and st["peak_drive"] == max(np.abs(p).max() for p in d)
    assert st["peak_index"] == min(int(np.flatnonzero(np.abs(p) == st["peak_drive"])[0]) for p in d if np.abs(p).max() == st["peak_drive"])
    assert int(np.sum(np.isnan(u[1]))) == 2 * 12 * 4 and np.all(d[1][np.isnan(u[1])] == 0.0)      # a NaN spreads over 2 Z source indices' mid samples


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def hexd(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def fnv(table):
    h = 1469598103934665603
    for b in np.ascontiguousarray(table, dtype=np.float64).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def lcg_table(seed):
    x, out = seed, np.zeros(M.TABLE)
    for i in range(M.TABLE):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = float(x >> 11) * 2.0 ** -51 - 2.0
    return out


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/saturate_main.cpp: wbx_saturate.h alone, stand-alone (its own main): the table, the check, the lookup, the
    call's check and the launch shape"""
    exe = str(tmp_path / "saturate_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "saturate_main.cpp"), "-o", exe])
    lines, want = [], []
    for kind in range(3):
        for bias in BIASES:
            lines.append("t %d %s" % (kind, hexd(bias)))
            want.append("t 0 %016x" % fnv(M.table(kind, bias)))
    last = M.table(2, BIASES[-1])
    for kind, bias in ((3, 0.0), (0, 4.5), (1, np.nan)):          # refused: the table stays
        lines.append("t %d %s" % (kind, hexd(bias)))
        want.append("t -4 %016x" % fnv(last))
    tab = lcg_table(0x5EED)
    assert np.abs(tab).max() <= 2.0 and np.unique(tab).size == M.TABLE
    lines += ["r %d" % 0x5EED, "k"]
    want += ["r", "k 0"]
    d = lookup_points()[::7]
    looked, _ = M.lookup(tab, d)
    for v, w in zip(d, looked):
        lines.append("l %s" % hexd(v))
        want.append("l %s" % hexd(w))
    for change, status in CHECKS:
        a = dict(OK, **change)
        if a["tab"] not in ("good", None):
            continue
        lines.append("c %d %d %d %d %s %s" % (a["n"], a["os"], a["q"], a["tab"] is not None, hexd(a["drive"]), hexd(a["makeup"])))
        want.append("c %d" % status)
    for v, status in ((np.inf, -4), (2.0 ** 32, 0), (np.nan, -4), (1.0, 0), (2.0 ** 33, -4), (-2.0 ** 32, 0)):
        lines += ["p 16384 %s" % hexd(v), "k", "c 4096 4 1 1 %s %s" % (hexd(1.0), hexd(1.0))]
        want += ["p", "k %d" % status, "c %d" % status]
    for os_ in (1, 2, 4, 8):
        for q in range(3):
            if (os_, q) == (8, M.BEST):
                continue
            for ch in (1, 2):
                for n in (1, 1024, 1025, 3000, TOP // os_ - 1):
                    s = M.launch_shape(os_, q, ch, n)
                    lines.append("s %d %d %d %d" % (os_, q, ch, n))
                    want.append("s %d %d %d %d %d" % (s["tile"], s["mid_span"], s["src_span"], s["lds_bytes"], s["n_tiles"]))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "saturate ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
