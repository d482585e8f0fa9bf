"""Warping a clip, the part that needs no device: the symbols of include/wbx.h "Warping a clip" exist and match their
binding twins, the adapter's method compiles, NULL handles are refused, wbx_warp_check / _steps / _segments / _launches equal
the numpy twin (tests/warp_model.py), every refusal of the argument check one by one, the model itself has the three
consequences the header states — and wbx_warp.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stretch_model as SM
import warp_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_warp_check", "wbx_warp_steps", "wbx_warp_segments", "wbx_warp_max_markers", "wbx_warp_max_steps",
       "wbx_warp_launch_segments", "wbx_warp_launches", "wbx_warp_ms", "wbx_clip_warp", "wbx_engine_warp_sample"]
EDGE = SM.MAX_FRAMES - 1                                       # the longest range and the longest result


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def noise_and_sine(n, channels=1, seed=0x3A9F):
    rng = np.random.default_rng(seed + channels)
    i = np.arange(n)
    return [(0.3 * rng.standard_normal(n) + np.sin(2 * np.pi * i / (41.7 + 9 * c))).astype(np.float32) for c in range(channels)]


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.warp_check) and callable(W.warp_steps) and callable(W.warp_segments) and callable(W.warp_launches)
    assert hasattr(W.MixContext, "clip_warp") and hasattr(W.MixContext, "warp_ms")
    for m in ("warp_sample", "warp_to_markers", "quantize_sample"):
        assert hasattr(W.Engine, m), m
    assert "Warping a clip" in re.sub(r"\s*\*\s*", " ", header)
    assert L.wbx_warp_max_markers() == 65535 == M.MAX_MARKERS and L.wbx_warp_max_steps() == 1 << 22 == M.MAX_STEPS
    assert L.wbx_warp_launch_segments() >= 1


def test_the_structs_have_the_headers_sizes_and_layouts(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(wbx_warp_marker), offsetof(wbx_warp_marker, out_frame), sizeof(wbx_warp_info), '
                   'offsetof(wbx_warp_info, candidates), offsetof(wbx_warp_info, max_shift), offsetof(wbx_warp_info, launches), '
                   'offsetof(wbx_warp_info, segments), offsetof(wbx_warp_info, longest_segment_steps), sizeof(wbx_warp_segment), '
                   'offsetof(wbx_warp_segment, steps)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    K, I, S = _ffi.WarpMarker, _ffi.WarpInfo, _ffi.WarpSegment
    assert got == [16, 8, 40, 16, 24, 28, 32, 36, 32, 24] == [C.sizeof(K), K.out_frame.offset, C.sizeof(I), I.candidates.offset,
                                                             I.max_shift.offset, I.launches.offset, I.segments.offset,
                                                             I.longest_segment_steps.offset, C.sizeof(S), S.steps.offset]
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    for name, size in (("marker", 16), ("info", 40), ("segment", 32)):
        assert re.search(r"wbx_warp_%s\s*\{\s*/\* %d bytes \*/" % (name, size), header), name


def test_adapter_with_warp_compiles(tmp_path):
    """tests/cpp/adapter_warp.cpp uses Engine::warp_sample; it is compiled and linked here and run by
    tests/test_gpu_warp.py (it needs a device)"""
    exe = str(tmp_path / "adapter_warp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_warp.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_arguments_are_refused_without_a_device():
    L = W.lib()
    new, wi, st, ms = C.c_uint32(77), _ffi.WarpInfo(), _ffi.ClipStats(), C.c_double(5.0)
    wi.steps = 123
    pos = np.full(8, 9, dtype=np.int32)
    mk = (_ffi.WarpMarker * 1)()
    mk[0].src_frame, mk[0].out_frame = 30, 40
    assert L.wbx_clip_warp(None, 0, 1, 0, 64, 96, mk, 1, 32, 8, pos.ctypes.data, 8, C.byref(wi), C.byref(st)) == -4
    assert np.all(pos == 9) and wi.steps == 123
    assert L.wbx_engine_warp_sample(None, 0, 0, 64, 96, mk, 1, 32, 8, C.byref(wi), C.byref(new)) == -4 and new.value == 77
    assert L.wbx_warp_ms(None, C.byref(ms)) == -4 and ms.value == 5.0
    assert L.wbx_warp_check(64, 96, None, 1, 32, 8) == -4 and L.wbx_warp_steps(64, 96, None, 1, 32) == 0
    assert L.wbx_warp_launches(64, 96, None, 1, 32, 8) == 0
    seg = (_ffi.WarpSegment * 2)()
    seg[0].steps = 55
    assert L.wbx_warp_segments(64, 96, mk, 1, 32, None, 2) == -4 and L.wbx_warp_segments(64, 96, None, 1, 32, seg, 2) == -4
    assert L.wbx_warp_segments(64, 96, mk, 1, 32, seg, 1) == -4 and seg[0].steps == 55
    assert L.wbx_warp_check(64, 96, None, 0, 32, 8) == 0 and L.wbx_warp_steps(64, 96, None, 0, 32) == 6


# ---- host functions against the model ---------------------------------------------------------------------------------------
def seeded_markers(rng, n, m, M_):
    """M_ strictly ascending pairs inside (0, n) x (0, m) with every segment's ratio within 8"""
    s = np.sort(rng.choice(np.arange(1, n), M_, replace=False)) if M_ else np.zeros(0, dtype=np.int64)
    out, last = [], (0, 0)
    for a in s.tolist():
        d = a - last[0]
        lo, hi = max(1, -(-d // 8)), 8 * d
        t = last[1] + int(rng.integers(lo, hi + 1))
        out.append((a, t))
        last = (a, t)
    return out


def marker_sets():
    rng = np.random.default_rng(0xA11CE)
    sets = []
    for N in (32, 256, 2048):
        Hs = N // 2
        # segments of m_j < Hs, = Hs, = Hs + 1, then the rest
        t = [Hs - 1, 2 * Hs - 1, 3 * Hs]
        mk = [(40, t[0]), (40 + Hs, t[1]), (40 + 2 * Hs + 3, t[2])]
        sets.append((40 + 2 * Hs + 3 + 500, t[2] + 777, mk, N))
        # ratios at exactly 8 and 1 / 8
        sets.append((1000 + 8 * 50 + 300, 8000 + 50 + 301, [(1000, 8000), (1000 + 8 * 50, 8000 + 50)], N))
        for M_ in (1, 3, 17, 200):
            n = int(rng.integers(3000, 20000))
            mk = seeded_markers(rng, n, 1 << 40, M_)
            d = n - (mk[-1][0] if mk else 0)
            m = (mk[-1][1] if mk else 0) + int(rng.integers(max(1, -(-d // 8)), 8 * d + 1))
            sets.append((n, m, mk, N))
    # frames at the 2^31 - 16 edge: a marker in the last frame of the range and of the result
    sets.append((EDGE, EDGE, [(EDGE - 1, EDGE - 1)], 8192))
    sets.append((EDGE, EDGE, [(1, 1), (EDGE // 2, EDGE // 2 + 5)], 8192))
    return sets


def test_check_steps_segments_and_launches_equal_the_model():
    L = W.lib()
    LS = L.wbx_warp_launch_segments()
    for n, m, mk, N in marker_sets():
        for D in (0, 24, 4096):
            want = M.check(n, m, mk, N, D)
            assert W.warp_check(n, m, mk, N, D) == want, (n, m, N, D)
            assert W.warp_launches(n, m, mk, N, D) == M.launches(n, m, mk, N, D, LS), (n, m, N, D)
        assert W.warp_steps(n, m, mk, N) == M.steps(n, m, mk, N)
        segs = M.segments(n, m, mk, N)
        assert W.warp_segments(n, m, mk, N) == segs
        assert segs[0][:3] == (0, 0, 0) and all(g[3] >= 1 for g in segs)
        assert all(a[2] + a[3] == b[2] for a, b in zip(segs[:-1], segs[1:]))
    n, m, mk, N = marker_sets()[0]
    assert [g[3] for g in M.segments(n, m, mk, N)[:3]] == [1, 1, 2]     # m_j = Hs - 1, Hs, Hs + 1
    for N in (0, 24, 36, 8200):                                 # a window the call refuses: 0
        assert W.warp_steps(1000, 1000, [(5, 5)], N) == 0 == M.steps(1000, 1000, [(5, 5)], N)


def test_65535_markers_and_one_more():
    L = W.lib()
    mk = [(5 * j + 5, 40 * j + 40) for j in range(65535)]       # every segment: 5 source frames into 40 output frames, ratio 8
    n, m = 5 * 65536, 40 * 65536
    assert W.warp_check(n, m, mk, 32, 8) == 0 == M.check(n, m, mk, 32, 8)
    assert W.warp_steps(n, m, mk, 32) == 65536 * 3 == M.steps(n, m, mk, 32)
    segs = W.warp_segments(n, m, mk, 32)
    assert len(segs) == 65536 and segs[-1] == (5 * 65535, 40 * 65535, 3 * 65535, 3) and segs == M.segments(n, m, mk, 32)
    assert W.warp_launches(n, m, mk, 32, 8) == -(-65536 // L.wbx_warp_launch_segments()) + 1
    arr = (_ffi.WarpMarker * 65536)()
    for j in range(65536):
        arr[j].src_frame, arr[j].out_frame = 4 * j + 4, 32 * j + 32
    assert L.wbx_warp_check(4 * 65537, 32 * 65537, arr, 65535, 32, 8) == 0
    assert L.wbx_warp_check(4 * 65537, 32 * 65537, arr, 65536, 32, 8) == -4
    assert M.check(4 * 65537, 32 * 65537, [(4 * j + 4, 32 * j + 32) for j in range(65536)], 32, 8) == -4


# ---- the argument check -----------------------------------------------------------------------------------------------------
OK = dict(n=1000, m=1500, N=128, D=24, mk=[(300, 400), (600, 1000)])
CHECKS = [(dict(), 0), (dict(mk=[]), 0), (dict(n=0), -4), (dict(m=0), -4), (dict(n=SM.MAX_FRAMES, m=SM.MAX_FRAMES, mk=[]), -4),
          (dict(n=EDGE, m=EDGE, mk=[], N=8192), 0), (dict(n=EDGE, m=EDGE, mk=[]), -3), (dict(N=24), -4), (dict(N=8200), -4), (dict(N=36), -4), (dict(N=0), -4), (dict(N=32), 0),
          (dict(N=8192), 0), (dict(D=4096), 0), (dict(D=4097), -4),
          # the markers, one rule at a time
          (dict(mk=[(0, 400)]), -4), (dict(mk=[(300, 0)]), -4), (dict(mk=[(1000, 1400)]), -4), (dict(mk=[(999, 1499)]), 0),
          (dict(mk=[(900, 1500)]), -4), (dict(mk=[(300, 400), (300, 1000)]), -4), (dict(mk=[(300, 400), (600, 400)]), -4),
          (dict(mk=[(300, 400), (299, 1000)]), -4), (dict(mk=[(300, 400), (600, 399)]), -4), (dict(mk=[(300, 400), (301, 401)]), 0),
          # a segment's ratio: 8 is taken, beyond it is not; the whole range's ratio is not judged on its own
          (dict(mk=[(100, 800)]), 0), (dict(mk=[(100, 801)]), -3), (dict(mk=[(800, 100)]), 0), (dict(mk=[(801, 100)]), -3),
          (dict(n=1000, m=8000, mk=[]), 0), (dict(n=1000, m=8001, mk=[]), -3), (dict(n=12001, m=1500, mk=[]), -3),
          (dict(n=1000, m=1500, mk=[(990, 1400)]), -3),          # the last segment: 10 source frames into 100
          (dict(n=1000, m=8001, mk=[(100, 801)]), -3),
          # invalid beats unsupported
          (dict(mk=[(100, 801)], N=36), -4), (dict(n=1000, m=8001, mk=[(0, 5)]), -4)]


def test_every_refusal_of_the_check_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check(a["n"], a["m"], a["mk"], a["N"], a["D"]) == want, change
        assert W.warp_check(a["n"], a["m"], a["mk"], a["N"], a["D"]) == want, change
        if want:
            assert W.warp_launches(a["n"], a["m"], a["mk"], a["N"], a["D"]) == 0, change
    assert {w for _, w in CHECKS} == {0, -4, -3}
    # K one past the step limit: 2^22 segments' worth of steps at N = 32 is 2^26 output frames
    m = (1 << 22) * 16
    assert W.warp_check(m, m, [], 32, 0) == 0 == M.check(m, m, [], 32, 0)
    assert W.warp_check(m + 1, m + 1, [], 32, 0) == -3 == M.check(m + 1, m + 1, [], 32, 0)
    assert W.warp_check(m, m, [(5, 5)], 32, 0) == -3 == M.check(m, m, [(5, 5)], 32, 0)    # a marker off the hop grid: one more step
    assert W.warp_check(m, m, [(16, 16)], 32, 0) == 0
    # positions_cap below K (the model's; the library's is checked on the device, where the call exists)
    assert M.check(1000, 1500, OK["mk"], 128, 24, positions_cap=M.steps(1000, 1500, OK["mk"], 128) - 1) == -4
    assert M.check(1000, 1500, OK["mk"], 128, 24, positions_cap=M.steps(1000, 1500, OK["mk"], 128)) == 0


# ---- the launch plan ----------------------------------------------------------------------------------------------------------
def test_a_later_round_has_fewer_workgroups_and_a_round_is_cut_into_slices():
    L = W.lib()
    LS = L.wbx_warp_launch_segments()
    # rounds: N = 32, D = 4096 on a range of 30 000: one segment with more steps than one workgroup's launch, beside short ones
    n, N, D = 30000, 32, 4096
    Sr = L.wbx_stretch_launch_steps(n, N, D)
    assert Sr == M.launch_steps(n, N, D) and Sr >= 1
    long_m = (Sr + 7) * 16
    mk = [(200, 100), (400, 333), (400 + long_m // 8 + 50, 333 + long_m)]
    m_ = mk[-1][1] + 3000
    assert long_m < 8 * (mk[2][0] - mk[1][0]) and W.warp_check(n, m_, mk, N, D) == 0
    live = M.rounds(n, m_, mk, N, D)
    assert live == [4, 1] and W.warp_launches(n, m_, mk, N, D) == 3 == M.launches(n, m_, mk, N, D, LS)
    # slices: more segments than one launch takes, read from the getter
    S = LS + 5
    mk = [(30 * j, 30 * j) for j in range(1, S)]
    assert M.rounds(30 * S, 30 * S, mk, 32, 8) == [S] and W.warp_launches(30 * S, 30 * S, mk, 32, 8) == 3
    assert M.launches(30 * S, 30 * S, mk, 32, 8, LS) == 3


# ---- the consequences the header states, on the model -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1000, 1500, 64, 24), (2, 1000, 667, 256, 96), (1, 3000, 2999, 32, 1), (2, 700, 5600, 32, 40),
                                   (1, 4000, 500, 64, 0)], ids=lambda s: "ch%d-n%d-m%d-N%d-D%d" % s)
def test_without_markers_the_model_is_the_stretch_model(shape):
    ch, n, m, N, D = shape
    src = noise_and_sine(n + 40, ch)
    src[0][[25, 300]] = np.float32(np.nan), np.float32(np.inf)
    out, p, info = M.warp_clip(src, 20, n, m, [], N, D)
    ref, rp, rinfo = SM.stretch_clip(src, 20, n, m, N, D)
    assert np.array_equal(p, rp) and all(same_bits32(a, b) for a, b in zip(out, ref))
    assert {k: info[k] for k in rinfo} == rinfo and info["segments"] == 1 and info["longest_segment_steps"] == info["steps"]
    assert info["searched_steps"] > 0 or D == 1


def test_a_segments_positions_depend_on_nothing_outside_it_but_the_source():
    n, m, N, D = 9000, 11000, 64, 24
    src = noise_and_sine(n)
    base = [(2000, 2500), (4100, 5003), (7000, 8001)]
    _, p0, _ = M.warp_clip(src, 0, n, m, base, N, D)
    s0 = M.segments(n, m, base, N)
    for other in ([(2100, 2400), (4100, 5003), (7000, 8001)], [(4100, 5003), (7000, 8001)], [(500, 900), (2000, 2500), (4100, 5003), (7000, 8001)],
                  [(2000, 2500), (4100, 5003), (7000, 8001), (8000, 9500)]):
        out, p1, _ = M.warp_clip(src, 0, n, m, other, N, D)
        s1 = M.segments(n, m, other, N)
        a, b = [g for g in s0 if g[:2] == (4100, 5003)][0], [g for g in s1 if g[:2] == (4100, 5003)][0]
        assert a[3] == b[3] and np.array_equal(p0[a[2]:a[2] + a[3]], p1[b[2]:b[2] + b[3]]), other
    assert len(out[0]) == m


def click_take():
    """nine clicks on a noise floor; each should land on a target that is no multiple of 4"""
    N, D, Hs = 256, 64, 128
    rng = np.random.default_rng(0xC11C)
    ratios = [0.87, 1.25, 1.0, 0.93, 1.1, 1.21, 0.9, 1.05, 1.17, 1.0]
    events = [1500 + 1600 * i for i in range(9)]
    n = events[-1] + 1700
    x = (0.01 * rng.standard_normal(n)).astype(np.float32)
    for e in events:
        x[e:e + 40] += (np.exp(-np.arange(40) / 8.0) * np.cos(np.arange(40) * 0.9)).astype(np.float32)
    targets, t, s_prev = [], 0, 0
    for e, r in zip(events, ratios):
        t = t + int(round((e - s_prev) / r)) | 1                # odd: no multiple of 4
        targets.append(t)
        s_prev = e
    m = targets[-1] + int(round((n - events[-1]) / ratios[-1]))
    return [x], n, m, events, targets, N, D


def test_markers_a_hop_early_keep_an_attack_intact():
    src, n, m, events, targets, N, D = click_take()
    Hs = N // 2
    mk = [(e - Hs, t - Hs) for e, t in zip(events, targets)]
    assert M.check(n, m, mk, N, D) == 0 and all(t % 4 for t in targets)
    edges = [(0, 0)] + mk + [(n, m)]
    for (s0, t0), (s1, t1) in zip(edges[:-1], edges[1:]):
        assert Hs * abs(1 - (s1 - s0) / (t1 - t0)) <= D         # the step after the pinned one keeps its continuation
    out, p, info = M.warp_clip(src, 0, n, m, mk, N, D)
    segs = M.segments(n, m, mk, N)
    for (s_j, t_j, base, Kj), e, t in zip(segs[1:], events, targets):
        assert p[base] == e - Hs and p[base + 1] == e           # pinned, then the natural continuation
        assert same_bits32(out[0][t:t + Hs], src[0][e:e + Hs])  # the hop behind the click: a copy, bit for bit
    assert info["segments"] == 10


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def checksum(segs):
    return sum((j + 1) * (g[0] + 3 * g[1] + 5 * g[2] + 7 * g[3]) for j, g in enumerate(segs)) & ((1 << 64) - 1)


def test_check_steps_segments_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/warp_main.cpp: wbx_warp.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "warp_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "warp_main.cpp"), "-o", exe])
    L = W.lib()
    LS = L.wbx_warp_launch_segments()
    flat = lambda mk: " ".join("%d %d" % q for q in mk)
    lines, want = [], []
    for change, status in CHECKS:
        a = dict(OK, **change)
        lines.append("c %d %d %d %d %d %s" % (a["n"], a["m"], a["N"], a["D"], len(a["mk"]), flat(a["mk"])))
        want.append("c %d" % status)
    big = [(5 * j + 5, 40 * j + 40) for j in range(65535)]
    sets = marker_sets() + [(5 * 65536, 40 * 65536, big, 32)]
    for n, m, mk, N in sets:
        lines.append("s %d %d %d %d %s" % (n, m, N, len(mk), flat(mk)))
        want.append("s %d" % M.steps(n, m, mk, N))
        lines.append("g %d %d %d %d %s" % (n, m, N, len(mk), flat(mk)))
        want.append("g 0 %d %d" % (len(mk) + 1, checksum(M.segments(n, m, mk, N))))
        for D in (0, 4096):
            lines.append("l %d %d %d %d %d %s" % (n, m, N, D, len(mk), flat(mk)))
            want.append("l %d" % M.launches(n, m, mk, N, D, LS))
            if M.check(n, m, mk, N, D) == 0 and M.steps(n, m, mk, N) < 1 << 20:
                lines.append("p %d %d %d %d %d %s" % (n, m, N, D, len(mk), flat(mk)))
                cut = []
                for r, live in enumerate(M.rounds(n, m, mk, N, D)):
                    cut += ["%d:%d" % (r, min(LS, live - at)) for at in range(0, live, LS)]
                want.append("p %d %d %s" % (M.launch_steps(n, N, D), max(g[3] for g in M.segments(n, m, mk, N)), " ".join(cut)))
    lines.append("g 1000 1500 36 1 300 400")
    want.append("g -4 2 0")
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert got[-1] == "warp ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
