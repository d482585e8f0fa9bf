"""Stretching a clip, the part that needs no device: the symbols of include/wbx.h "Stretching a clip" exist and match their
binding twins, the adapter's method compiles, NULL handles are refused, wbx_stretch_steps / _anchor / _window equal the
numpy twin (tests/stretch_model.py) BIT FOR BIT, every refusal of the argument check, the model itself has the properties the
header states — and wbx_stretch.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stretch_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_stretch_steps", "wbx_stretch_anchor", "wbx_stretch_window", "wbx_stretch_band_steps", "wbx_stretch_launch_terms",
       "wbx_stretch_step_terms", "wbx_stretch_launch_steps", "wbx_stretch_ms", "wbx_clip_stretch", "wbx_engine_stretch_sample"]
EDGE = M.MAX_FRAMES - 1                                        # the longest range and the longest result


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.stretch_steps) and callable(W.stretch_anchor) and callable(W.stretch_window)
    assert hasattr(W.MixContext, "clip_stretch") and hasattr(W.MixContext, "stretch_ms")
    for m in ("stretch_sample", "stretch_to_tempo"):
        assert hasattr(W.Engine, m), m
    assert "Stretching a clip" in re.sub(r"\s*\*\s*", " ", header)
    assert L.wbx_stretch_band_steps() >= 1 and L.wbx_stretch_launch_terms() >= 8193 * 4096


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(wbx_stretch_info), offsetof(wbx_stretch_info, steps), offsetof(wbx_stretch_info, searched_steps), '
                   'offsetof(wbx_stretch_info, candidates), offsetof(wbx_stretch_info, max_shift), offsetof(wbx_stretch_info, launches)); '
                   'return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.StretchInfo
    assert got == [32, 0, 8, 16, 24, 28] == [C.sizeof(S), S.steps.offset, S.searched_steps.offset, S.candidates.offset,
                                              S.max_shift.offset, S.launches.offset]
    assert re.search(r"wbx_stretch_info\s*\{\s*/\* 32 bytes \*/", open(os.path.join(ROOT, "include", "wbx.h")).read())


def test_adapter_with_stretch_compiles(tmp_path):
    """tests/cpp/adapter_stretch.cpp uses Engine::stretch_sample; it is compiled and linked here and run by
    tests/test_gpu_stretch.py (it needs a device)"""
    exe = str(tmp_path / "adapter_stretch")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_stretch.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    new, si, st, ms = C.c_uint32(77), _ffi.StretchInfo(), _ffi.ClipStats(), C.c_double(5.0)
    pos = np.full(8, 9, dtype=np.int32)
    assert L.wbx_clip_stretch(None, 0, 1, 0, 64, 96, 32, 8, pos.ctypes.data, 8, C.byref(si), C.byref(st)) == -4 and np.all(pos == 9)
    assert L.wbx_engine_stretch_sample(None, 0, 0, 64, 96, 32, 8, C.byref(si), C.byref(new)) == -4 and new.value == 77
    assert L.wbx_stretch_ms(None, C.byref(ms)) == -4 and ms.value == 5.0


# ---- host functions against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 64, 2048, 8192])
def test_the_window_equals_the_model_bit_for_bit(N):
    up, dn = W.stretch_window(N)
    mu, md = M.window(N)
    assert len(up) == len(dn) == N // 2 and same_bits64(up, mu) and same_bits64(dn, md)
    assert up[0] == 0.0 and dn[0] == 1.0 and np.all(np.diff(up) > 0.0) and np.all(up < 1.0)
    # w_up + w_dn within one ulp of 1 (w_dn = 1 - w_up is one rounding, the sum another)
    assert np.all(np.abs((up + dn) - 1.0) <= 2.0 ** -52)
    assert abs(up[N // 4] - 0.5) < 1e-15                        # sin^2(pi / 4)


def test_window_refusals_write_nothing():
    L = W.lib()
    for N, cap in ((24, 64), (8200, 8200), (36, 64), (0, 64), (64, 63), (64, 0)):
        buf = np.full(max(cap, 1), 7.0)
        assert L.wbx_stretch_window(N, buf.ctypes.data, cap) == -4 and np.all(buf == 7.0), (N, cap)
    assert L.wbx_stretch_window(64, None, 64) == -4
    buf = np.full(70, 7.0)
    assert L.wbx_stretch_window(64, buf.ctypes.data, 70) == 0 and np.all(buf[64:] == 7.0) and not np.any(buf[:64] == 7.0)
    with pytest.raises(W.WbxError):
        W.stretch_window(40 + 4)
    with pytest.raises(M.Refused):
        M.window(44)


def test_steps_and_anchors_equal_the_model_at_the_edges():
    rng = np.random.default_rng(0x57E7)
    for N in (32, 40, 64, 2048, 8192):
        Hs = N // 2
        for m in (1, Hs - 1, Hs, Hs + 1, 5 * Hs + 3, 1 << 24, EDGE - 1, EDGE):
            K = M.steps(m, N)
            assert W.stretch_steps(m, N) == K and (K - 1) * Hs < m <= K * Hs
            for n in (1, 7, m, max(1, m // 8), min(EDGE, 8 * m), EDGE):
                for k in {0, min(1, K - 1), K // 2, K - 1} | set(int(v) for v in rng.integers(0, K, 3)):
                    a = M.anchor(k, n, m, N)
                    assert W.stretch_anchor(k, n, m, N) == a and 0 <= a <= n - 1, (k, n, m, N)
    assert M.steps(EDGE, 32) == (EDGE + 15) // 16 < 1 << 27
    assert W.stretch_anchor((EDGE + 15) // 16 - 1, EDGE, EDGE, 32) == M.anchor((EDGE + 15) // 16 - 1, EDGE, EDGE, 32)
    for N in (0, 24, 36, 8200):                                 # a window the call refuses: 0
        assert W.stretch_steps(1000, N) == 0 == M.steps(1000, N) and W.stretch_anchor(3, 10, 10, N) == 0
    assert W.stretch_anchor(3, 10, 0, 64) == 0
    # any 64-bit arguments may be asked about: the product is taken in 128 bits
    assert W.stretch_anchor((1 << 40) + 1, (1 << 40) + 3, 1 << 41, 8192) == ((1 << 40) + 1) * 4096 * ((1 << 40) + 3) >> 41


def test_launch_planning_getters():
    L = W.lib()
    T, S, B = L.wbx_stretch_launch_terms(), L.wbx_stretch_step_terms(), L.wbx_stretch_band_steps()
    for n, N, D in ((700, 32, 4096), (100000, 32, 40), (1 << 20, 2048, 512), (1 << 20, 8192, 4096), (5, 32, 0), (1 << 30, 32, 0)):
        cand = min(2 * D + 1, n)
        assert L.wbx_stretch_launch_steps(n, N, D) == min(B, max(1, T // (cand * (N // 2) + S))), (n, N, D)
    assert L.wbx_stretch_launch_steps(0, 32, 0) == 0 == L.wbx_stretch_launch_steps(100, 33, 0)


# ---- the argument check -----------------------------------------------------------------------------------------------------
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(m=0), -4), (dict(n=M.MAX_FRAMES, m=M.MAX_FRAMES), -4), (dict(n=EDGE, m=EDGE), 0),
          (dict(m=M.MAX_FRAMES, n=M.MAX_FRAMES // 2), -4), (dict(n=1 << 63, m=1 << 63), -4), (dict(N=24), -4), (dict(N=8200), -4),
          (dict(N=36), -4), (dict(N=0), -4), (dict(N=32), 0), (dict(N=8192), 0), (dict(N=40), 0), (dict(D=4096), 0), (dict(D=4097), -4),
          (dict(cap=0), -4), (dict(cap=23), -4), (dict(cap=24), 0), (dict(m=8000), 0), (dict(m=8001), -3), (dict(n=12000), 0),
          (dict(n=12001), -3), (dict(n=1, m=9), -3), (dict(n=1, m=8), 0), (dict(m=8001, N=36), -4), (dict(m=8001, cap=0), -4),
          (dict(n=0, m=8001), -4)]


def test_check_args_of_the_model():
    ok = dict(n=1000, m=1500, N=128, D=24, cap=None)
    for change, want in CHECKS:
        a = dict(ok, **change)
        assert M.check_args(a["n"], a["m"], a["N"], a["D"], a["cap"]) == want, change


# ---- properties of the model --------------------------------------------------------------------------------------------------
def noise_and_sine(n, channels=1, seed=0x5EED):
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n)
    return [(0.3 * rng.standard_normal(n) + np.sin(2 * np.pi * i / (41.7 + 9 * c))).astype(np.float32) for c in range(channels)]


def test_a_range_stretched_to_its_own_length_is_a_copy_and_a_frame_more_or_less_takes_no_search():
    for ch in (1, 2):
        src = noise_and_sine(1000, ch)
        src[0][[3, 500]] = np.float32(-0.0), np.float32(1e-42)
        for N, D in ((32, 0), (64, 24), (256, 96), (2048, 512)):
            out, p, info = M.stretch_clip(src, 0, 1000, 1000, N, D)
            assert all(same_bits32(o, s) for o, s in zip(out, src)) and info["searched_steps"] == 0 and info["max_shift"] == 0
            assert np.array_equal(p, np.arange(len(p)) * (N // 2))
            for m in (999, 1001):                               # the anchors drift from k Hs by under one frame in all: with a
                out, p, info = M.stretch_clip(src, 0, 1000, m, N, max(D, 1))   # tolerance of 1 the continuation always holds
                assert info["searched_steps"] == 0 and info["max_shift"] <= 1
                assert all(same_bits32(o[:999], s[:999]) for o, s in zip(out, src))


def test_without_a_tolerance_the_positions_are_the_anchors():
    """D = 0 is plain overlap-add: p_k = a_k whenever the continuation misses, and it can only hit where it IS a_k"""
    src = noise_and_sine(3000)
    for m in (1000, 2000, 4505, 6000):
        for N in (32, 256):
            _, p, info = M.stretch_clip(src, 0, 3000, m, N, 0)
            assert p.tolist() == [M.anchor(k, 3000, m, N) for k in range(len(p))] and info["max_shift"] == 0
            assert info["candidates"] == info["searched_steps"] > 0


def test_silence_and_opposite_channels_pick_the_lowest_candidate():
    n = 2000
    loud = noise_and_sine(n)[0]
    for src in ([np.zeros(n, dtype=np.float32)], [loud, -loud], [np.full(n, np.nan, dtype=np.float32)]):
        for m, N, D in ((3000, 64, 24), (1300, 256, 96), (500, 64, 40)):
            out, p, info = M.stretch_clip(src, 0, n, m, N, D)
            prev, Hs = -(N // 2), N // 2
            for k, pk in enumerate(p):
                a = M.anchor(k, n, m, N)
                lo, hi = max(a - D, 0), min(a + D, n - 1)
                assert pk == (prev + Hs if lo <= prev + Hs <= hi else lo), (k, m, N, D)
                prev = int(pk)
            assert info["searched_steps"] > 0 and all(np.all(np.isfinite(o)) for o in out)


def rms(v):
    return float(np.sqrt(np.mean(np.asarray(v, dtype=np.float64) ** 2)))


@pytest.mark.parametrize("shape", [(64, 24, 1500), (256, 96, 12000)], ids=lambda s: "N%d-D%d-n%d" % s)
@pytest.mark.parametrize("kind", ["sine", "chirp"])
def test_the_search_keeps_the_level_better_than_plain_overlap_add(kind, shape):
    """a relation between two runs of the model: the WSOLA result's RMS is closer to the source's than the D = 0 result's
    (misaligned grains cancel in the crossfade); no absolute figure is fixed"""
    N, D, n = shape
    i = np.arange(n, dtype=np.float64)
    x = np.sin(2 * np.pi * i / 37.3) if kind == "sine" else np.sin(2 * np.pi * (i / 90 + i * i / (60 * n)))
    src = [x.astype(np.float32)]
    for m in (n // 4, 2 * n // 3, 3 * n // 2 + 5, 2 * n, 4 * n):
        with_search, _, info = M.stretch_clip(src, 0, n, m, N, D)
        plain, _, _ = M.stretch_clip(src, 0, n, m, N, 0)
        e_search, e_plain = abs(rms(with_search[0]) - rms(src[0])), abs(rms(plain[0]) - rms(src[0]))
        print("%s N %d n %d m %d: rms error %.4f with the search, %.4f without" % (kind, N, n, m, e_search, e_plain))
        assert info["searched_steps"] > 0 and e_search < e_plain, (m, e_search, e_plain)


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def fnv(values):
    h = 1469598103934665603
    for b in np.ascontiguousarray(values, dtype=np.float64).view(np.uint8).tolist():
        h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_steps_anchors_window_check_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/stretch_main.cpp: wbx_stretch.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "stretch_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "stretch_main.cpp"), "-o", exe])
    hexd = lambda v: "%016x" % np.float64(v).view(np.uint64)
    L = W.lib()
    B = L.wbx_stretch_band_steps()
    lines, want = [], []
    for m, N in ((1, 32), (15, 32), (16, 32), (17, 32), (EDGE, 32), (EDGE, 8192), (1000, 36)):
        lines.append("s %d %d" % (m, N))
        want.append("s %d" % M.steps(m, N))
    for k, n, m, N in ((0, 5, 9, 32), (7, 1000, 1500, 64), ((EDGE + 15) // 16 - 1, EDGE, EDGE, 32), (EDGE // 4096, EDGE, EDGE // 8 + 1, 8192),
                       (3, 10, 0, 64), ((1 << 40) + 1, (1 << 40) + 3, 1 << 41, 8192)):
        lines.append("a %d %d %d %d" % (k, n, m, N))
        want.append("a %d" % M.anchor(k, n, m, N))
    for N in (32, 40, 2048, 8192):
        lines.append("w %d %d" % (N, N))
        t = np.concatenate(M.window(N))
        want.append("w 0 %016x %s %s" % (fnv(t), hexd(t[0]), hexd(t[-1])))
    lines.append("w 64 67")
    t = np.concatenate(list(M.window(64)) + [np.full(3, 7.0)])
    want.append("w 0 %016x %s %s" % (fnv(t), hexd(t[0]), hexd(7.0)))
    for N, cap in ((64, 63), (36, 64), (8200, 8200), (64, 0)):
        lines.append("w %d %d" % (N, cap))
        want.append("w -4 %016x %s %s" % (fnv(np.full(cap, 7.0)), hexd(7.0) if cap else "%016x" % 0, hexd(7.0) if cap else "%016x" % 0))
    ok = dict(n=1000, m=1500, N=128, D=24, cap=None)
    for change, status in CHECKS:
        a = dict(ok, **change)
        lines.append("c %d %d %d %d %d %d" % (a["n"], a["m"], a["N"], a["D"], a["cap"] is not None, a["cap"] or 0))
        want.append("c %d" % status)
    for n, N, D in ((700, 32, 4096), (1 << 20, 2048, 512), (1 << 20, 8192, 4096), (5, 32, 0), (0, 32, 0)):
        lines.append("l %d %d %d" % (n, N, D))
        want.append("l %d" % L.wbx_stretch_launch_steps(n, N, D))
    for K, per in ((1, 1), (B, B), (B + 1, B), (3 * B + 5, 7), (1 << 27, 1 << 14)):
        lines.append("b %d %d" % (K, per))
        bands = -(-K // B)
        searches = sum(-(-min(B, K - i * B) // per) for i in range(bands))
        want.append("b %d %d %d %d" % (bands, searches + bands, K, searches))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "stretch ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w for w in want if w.startswith("c ")} == {"c 0", "c -4", "c -3"}
