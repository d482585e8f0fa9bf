"""Limiting a clip, the part that needs no device: the symbols of include/wbx.h "Limiting a clip" exist and match their
binding twins, the adapter's method compiles, NULL handles are refused, wbx_limit_ramp equals the numpy twin
(tests/limit_model.py) BIT FOR BIT and refuses what the header says it refuses, the model itself keeps the guarantee the
header states — and wbx_limit.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import limit_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_limit_ramp", "wbx_limit_tile_frames", "wbx_limit_segment_terms", "wbx_limit_band_frames", "wbx_limit_ms",
       "wbx_clip_limit", "wbx_engine_limit_sample"]
LOOKAHEADS, HOLDS, RELEASES = (0, 1, 72, 4096), (0, 1, 65536), (1, 2, 4800, 1 << 20)


def lib_ramp(A, H, R, cap=None):
    """(status, the buffer): cap doubles, 7.0 where nothing was written"""
    buf = np.full(A + H + R if cap is None else cap, 7.0, dtype=np.float64)
    st = W.lib().wbx_limit_ramp(A, H, R, buf.ctypes.data, buf.size)
    return st, buf


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.limit_ramp) and callable(W.limit_frames)
    assert hasattr(W.MixContext, "clip_limit") and hasattr(W.Engine, "limit_sample") and hasattr(W.Engine, "maximize_sample")
    assert L.wbx_limit_tile_frames() == 2048 == M.TILE and L.wbx_limit_segment_terms() == 2048 == M.SEGMENT
    assert L.wbx_limit_band_frames() == 1 << 20 == M.BAND
    assert "Limiting a clip" in re.sub(r"\s*\*\s*", " ", header)


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(wbx_limit_stats), offsetof(wbx_limit_stats, peak_in), offsetof(wbx_limit_stats, min_gain), '
                   'offsetof(wbx_limit_stats, min_gain_frame), offsetof(wbx_limit_stats, limited_frames)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.LimitStats
    assert got == [32, 0, 8, 16, 24] == [C.sizeof(S), S.peak_in.offset, S.min_gain.offset, S.min_gain_frame.offset, S.limited_frames.offset]


def test_adapter_with_limit_compiles(tmp_path):
    """a translation unit that uses Engine::limit_sample (never called: it would need a device); main runs the host calls"""
    src = tmp_path / "adapter_limit.cpp"
    src.write_text('#include "wbx_adapter.hpp"\n'
                   'uint32_t mastered(wbx::Engine& e, uint32_t mix, uint64_t n) {\n'
                   '  wbx_limit_stats ls{};\n  wbx_clip_stats st{};\n'
                   '  return e.limit_sample(mix, 0, n, 0.891251f, 2.0, 72, 0, 4800, &ls, &st) + e.limit_sample(mix, 0, n, 1.0f, 1.0, 0, 0, 1);\n}\n'
                   'int main() {\n  double t[8];\n'
                   '  if (wbx_limit_ramp(2, 1, 4, t, 7) != WBX_OK) return 1;\n'
                   '  if (t[3] != 0.0 || t[4] != 0.25 || t[6] != 0.75) return 2;\n'
                   '  if (wbx_limit_ramp(2, 1, 4, t, 6) != WBX_ERR_INVALID || wbx_limit_ramp(2, 1, 0, t, 8) != WBX_ERR_INVALID) return 3;\n'
                   '  return wbx_limit_tile_frames() == 2048 && wbx_limit_segment_terms() == 2048 && wbx_limit_band_frames() == (1u << 20) ? 0 : 4;\n}\n')
    exe = str(tmp_path / "adapter_limit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx", "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.call([exe]) == 0


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    new, ls, st, ms = C.c_uint32(77), _ffi.LimitStats(), _ffi.ClipStats(), C.c_double(5.0)
    assert L.wbx_clip_limit(None, 0, 1, 0, 64, 1.0, 1.0, 8, 0, 48, C.byref(ls), C.byref(st)) == -4
    assert L.wbx_engine_limit_sample(None, 0, 0, 64, 1.0, 1.0, 8, 0, 48, C.byref(new), C.byref(ls), C.byref(st)) == -4 and new.value == 77
    assert L.wbx_limit_ms(None, C.byref(ms)) == -4 and ms.value == 5.0


# ---- wbx_limit_ramp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", LOOKAHEADS)
def test_ramps_equal_the_model_bit_for_bit(A):
    for H in HOLDS:
        for R in RELEASES:
            st, got = lib_ramp(A, H, R)
            want = M.ramp(A, H, R)
            assert st == 0 and same_bits64(got, want), (A, H, R)
            assert got.size == A + H + R and not np.any(got[:A + H + 1]) and np.all(np.diff(got[A + H:]) > 0.0), (A, H, R)
            assert got[-1] == (np.float64(R - 1) * (np.float64(1.0) / np.float64(R)) if R > 1 else 0.0)
    assert same_bits64(W.limit_ramp(A, 3, 7), M.ramp(A, 3, 7))


def test_a_ramp_writes_its_terms_and_no_more_and_refusals_write_nothing():
    st, buf = lib_ramp(5, 3, 9, cap=40)
    assert st == 0 and np.all(buf[17:] == 7.0) and not np.any(buf[:17] == 7.0)
    for A, H, R, cap in ((5, 3, 9, 16), (4097, 0, 1, 5000), (0, 65537, 1, 70000), (0, 0, 0, 8), (0, 0, (1 << 20) + 1, 8),
                         ((1 << 32) - 1, 0, 1, 8), (0, (1 << 32) - 1, 2, 8), (0, 0, 1, 0)):
        st, buf = lib_ramp(A, H, R, cap=cap)
        assert st == -4 and np.all(buf == 7.0), (A, H, R, cap)
        if A + H + R <= cap:                                    # (refused for its shape, not for the capacity)
            with pytest.raises(M.Refused):
                M.ramp(A, H, R)
    assert W.lib().wbx_limit_ramp(1, 1, 1, None, 3) == -4
    with pytest.raises(W.WbxError):
        W.limit_ramp(0, 0, 0)
    assert W.limit_frames(48000) == (72, 0, 4800) and W.limit_frames(44100, 0.0, 10.0, 0.0) == (0, 441, 1)


# ---- the model's own properties ---------------------------------------------------------------------------------------------
def random_case(rng):
    ch, n = int(rng.integers(1, 3)), int(rng.integers(1, 700))
    planes = [(rng.standard_normal(n) * rng.choice([0.05, 0.5, 2.0])).astype(np.float32) for _ in range(ch)]
    for p in planes:
        for _ in range(int(rng.integers(0, 4))):
            p[rng.integers(0, n)] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.0, -4.0])
    ceiling = np.float32(rng.choice([1.0, 0.891251, 0.5, 0.1]))
    drive = float(rng.choice([1.0, -1.0, 0.25, 3.0]))
    return planes, ceiling, drive, int(rng.integers(0, 70)), int(rng.integers(0, 50)), int(rng.integers(1, 300))


def test_the_model_keeps_the_guarantee_on_random_inputs():
    rng = np.random.default_rng(0x11417)
    limited = 0
    for _ in range(150):
        planes, ceiling, drive, A, H, R = random_case(rng)
        n = len(planes[0])
        out, stats = M.limit_clip(planes, 0, n, ceiling, drive, A, H, R)
        d, p, need, y, g = M.gains(planes, ceiling, drive, A, H, R)
        assert all(np.all(np.abs(o) <= ceiling) for o in out), (ceiling, drive, A, H, R)
        assert np.all(g > 0.0) and np.all(g <= need) and np.all(need <= 1.0)
        assert np.all(y > 0.0) and np.all(y <= 1.0) and y.size == n + A
        assert stats["limited_frames"] == np.count_nonzero(g < 1.0) and stats["min_gain"] == g.min() and stats["peak_in"] == p.max()
        assert g[stats["min_gain_frame"]] == g.min() and not np.any(g[:stats["min_gain_frame"]] == g.min())
        limited += stats["limited_frames"] > 0
    assert limited > 50


def test_the_model_passes_a_clip_under_the_ceiling_through():
    rng = np.random.default_rng(0x9A55)
    for ch in (1, 2):
        planes = [rng.uniform(-0.8, 0.8, 900).astype(np.float32) for _ in range(ch)]
        planes[0][:3] = -0.0, 0.8912, -0.891251
        out, stats = M.limit_clip(planes, 0, 900, np.float32(0.891251), 1.0, 40, 10, 100)
        assert all(np.array_equal(o.view(np.uint32), p.view(np.uint32)) for o, p in zip(out, planes))
        assert stats["limited_frames"] == 0 and stats["min_gain"] == 1.0 and stats["min_gain_frame"] == 0


def test_the_model_shapes_an_isolated_peak_as_the_header_says():
    """one sample of 2.0 at frame 300 under a ceiling of 1.0, A = 4, H = 5, R = 40: the gain is 1.0 until the look-ahead
    sees the peak, ramps down over A frames, is exactly 0.5 at the peak and through the hold, then rises by 1 / R per
    frame (the curve is straight from the hold's end until it reaches 1.0 after R / 2 frames; the average of A + 1 curve
    frames is straight where its whole window is) with rounded corners of A frames, and is 1.0 again afterwards"""
    x = np.full(600, 0.25, dtype=np.float32)
    x[300] = 2.0
    A, H, R = 4, 5, 40
    d, p, need, y, g = M.gains([x], np.float32(1.0), 1.0, A, H, R)
    assert np.all(g[:300 - A] == 1.0) and np.all(np.diff(g[300 - A - 1:301]) < 0.0) and g[300] == 0.5
    assert np.all(y[A + 300 - A:A + 300 + H + 1] == 0.5)        # the curve: look-ahead and hold at the needed gain
    assert np.all(g[300:300 + H + 1] == 0.5)                    # ... which the average of A + 1 equal values returns exactly
    rise = np.diff(g[300 + H + A:300 + H + R // 2 + 1])
    assert rise.size == R // 2 - A and np.all(np.abs(rise - 1.0 / R) < 1e-12)
    assert np.all(g[300 + A + H + R // 2 + 1:] == 1.0) and np.all(np.diff(g[300 + H:300 + A + H + R]) >= 0.0)


def test_check_args_of_the_model():
    ok = dict(n=1000, ceiling=1.0, drive=1.0, A=72, H=0, R=4800)
    assert M.check_args(**ok) == 0
    for change, want in ((dict(n=0), -4), (dict(ceiling=0.0), -4), (dict(ceiling=np.nan), -4), (dict(drive=0.0), -4),
                         (dict(drive=2.0 ** 33), -4), (dict(A=4097), -4), (dict(R=0), -4), (dict(n=M.MAX_FRAMES), -4),
                         (dict(n=1 << 30, R=1 << 20), -3), (dict(n=1 << 24, A=0, R=1 << 20), 0), (dict(n=(1 << 24) + 1, A=0, R=1 << 20), -3)):
        assert M.check_args(**dict(ok, **change)) == want, change


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def fnv(values):
    h = 1469598103934665603
    for b in np.ascontiguousarray(values, dtype=np.float64).view(np.uint8).tolist():
        h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_ramp_check_and_bands_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/limit_main.cpp: wbx_limit.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "limit_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "limit_main.cpp"), "-o", exe])
    hexd = lambda v: "%016x" % np.float64(v).view(np.uint64)
    hexf = lambda v: "%08x" % np.float32(v).view(np.uint32)
    lines, want = [], []
    for A, H, R in ((0, 0, 1), (0, 0, 2), (1, 1, 1), (72, 0, 4800), (4096, 1, 2), (0, 65536, 7), (3, 5, 1 << 14)):
        t = M.ramp(A, H, R)
        lines.append("r %d %d %d %d" % (A, H, R, t.size))
        want.append("r 0 %016x %s %s" % (fnv(t), hexd(t[0]), hexd(t[-1])))
    for A, H, R, cap in ((5, 3, 9, 16), (4097, 0, 1, 4100), (0, 65537, 1, 9), (0, 0, 0, 9), (0, 0, (1 << 20) + 1, 9)):
        lines.append("r %d %d %d %d" % (A, H, R, cap))
        want.append("r -4 %016x %s %s" % (fnv(np.full(cap, 7.0)), hexd(7.0), hexd(7.0)))
    checks = [(1000, 1.0, 1.0, 72, 0, 4800), (0, 1.0, 1.0, 72, 0, 4800), (1000, M.FLT_MIN, 1.0, 0, 0, 1), (1000, M.FLT_MIN / 2, 1.0, 0, 0, 1),
              (1000, -1.0, 1.0, 0, 0, 1), (1000, np.inf, 1.0, 0, 0, 1), (1000, np.nan, 1.0, 0, 0, 1), (1000, 1.0, 0.0, 0, 0, 1),
              (1000, 1.0, -0.0, 0, 0, 1), (1000, 1.0, -2.0 ** 32, 0, 0, 1), (1000, 1.0, 2.0 ** 32 * (1 + 2.0 ** -52), 0, 0, 1),
              (1000, 1.0, np.nan, 0, 0, 1), (1000, 1.0, -np.inf, 0, 0, 1), (1000, 1.0, 5e-324, 0, 0, 1), (1000, 1.0, 1.0, 4096, 65536, 1 << 20),
              (1000, 1.0, 1.0, 4097, 0, 1), (1000, 1.0, 1.0, 0, 65537, 1), (1000, 1.0, 1.0, 0, 0, 0), (1000, 1.0, 1.0, 0, 0, (1 << 20) + 1),
              (M.MAX_FRAMES - 1, 1.0, 1.0, 0, 0, 1), (M.MAX_FRAMES, 1.0, 1.0, 0, 0, 1), (1 << 63, 1.0, 1.0, 0, 0, 1),
              (1 << 24, 1.0, 1.0, 0, 0, 1 << 20), ((1 << 24) + 1, 1.0, 1.0, 0, 0, 1 << 20), (1 << 30, 1.0, 1.0, 4096, 65536, 1 << 20)]
    for n, c, d, A, H, R in checks:
        lines.append("c %d %s %s %d %d %d" % (n, hexf(c), hexd(d), A, H, R))
        want.append("c %d" % M.check_args(n, c, d, A, H, R))
    for n, A in ((1, 0), (2047, 9), (1 << 20, 4096), ((1 << 20) + 1, 4096), ((1 << 20) + 2053, 72), (5 * (1 << 20) - 3, 1), (M.MAX_FRAMES - 1, 4096)):
        bands = -(-n // M.BAND)
        sizes = [min(M.BAND, n - i * M.BAND) for i in range(bands)]
        lines.append("b %d %d" % (n, A))
        want.append("b %d %d %d %d %d" % (bands, n, n + bands * A, sum(-(-(s + A) // M.TILE) for s in sizes), sum(-(-s // M.TILE) for s in sizes)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "limit ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w for w in want if w.startswith("c ")} == {"c 0", "c -4", "c -3"}
