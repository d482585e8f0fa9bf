"""Finding a clip's onsets and tempo, the part that needs no device: the symbols of include/wbx.h "Finding a clip's onsets and
tempo" exist and match their binding twins, the two structs have the header's layout, the adapter's methods compile, NULL
handles are refused, wbx_onset_hops / _check / _pick equal the Python twin (tests/onset_model.py), every refusal of the
argument check, the model itself finds the tempo and the onsets of synthetic drum loops — and wbx_onset.h runs stand-alone
under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import f0_model as F0
import onset_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_onset_hops", "wbx_onset_check", "wbx_onset_max_hops", "wbx_onset_pick", "wbx_onset_ms", "wbx_clip_onsets",
       "wbx_clip_tempo", "wbx_engine_onsets_sample", "wbx_engine_tempo_sample"]
RATE, H = 48000, 256
TEMPO = dict(W=1024, step=64, lag_min=56, lag_max=188, threshold=0.5)   # lags of 200 .. 60 bpm at H = 256 and 48 kHz
# twice the worst relative tempo error measured on the model for this file's own loops (0.203 %, the 174 bpm loop)
TEMPO_BOUND = 2 * 0.00203


@pytest.fixture(autouse=True)
def library_with_onsets():
    """every test here, those of the model alone included, stands on a library that has the calls: the model is the reference
    of tests/test_gpu_onsets.py and means nothing without them"""
    L = W.lib()
    assert all(hasattr(L, n) for n in NEW)


@pytest.fixture(scope="module")
def loops():
    """bpm -> (novelty records of the loop with the default pick, its true onset frames): computed once, never changed"""
    out = {}
    for bpm in (120, 128, 174, 72, 93):
        x, at = M.drum_loop(bpm, RATE)
        rec = M.records(x.astype(np.float64), H, 1e-9, 0.3, 0.1, 3, 8)
        rec.setflags(write=False)
        out[bpm] = (rec, at)
    return out


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.onset_hops) and W.ONSET_DTYPE == M.DTYPE and W.ONSET_DTYPE.itemsize == 32
    for m in ("clip_onsets", "clip_tempo", "onsets_ms"):
        assert hasattr(W.MixContext, m), m
    for m in ("onsets_sample", "tempo_sample", "detect_tempo_sample", "fit_sample_to_tempo", "slice_sample"):
        assert hasattr(W.Engine, m), m
    flat = re.sub(r"\s*\*\s*", " ", header)
    assert "Finding a clip's onsets and tempo" in flat and "onset or tempo detection" not in flat
    for what in ("beat phase or downbeats", "a tempo prior against octave errors", "sample-accurate onset refinement"):
        assert what in flat, what
    assert L.wbx_onset_max_hops() == 1 << 20 == M.MAX_HOPS
    adapter = open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()
    assert "onsets_sample" in adapter and "tempo_sample" in adapter


def test_the_structs_have_the_headers_size_and_layout(tmp_path):
    frame, info = ["energy", "edge_energy", "novelty", "onset", "_pad"], ["hops", "onsets", "launches", "_pad"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * (len(frame) + len(info) + 1)
                   + '\\n", sizeof(wbx_onset_frame), ' + ", ".join("offsetof(wbx_onset_frame, %s)" % f for f in frame)
                   + ", sizeof(wbx_onset_info), " + ", ".join("offsetof(wbx_onset_info, %s)" % f for f in info) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    F, I = _ffi.OnsetFrame, _ffi.OnsetInfo
    assert got == [32, 0, 8, 16, 24, 28, 24, 0, 8, 16, 20]
    assert got == [C.sizeof(F)] + [getattr(F, f).offset for f in frame] + [C.sizeof(I)] + [getattr(I, f).offset for f in info]
    assert [M.DTYPE.fields[f][1] for f in frame] == got[1:6] and M.DTYPE.itemsize == 32
    text = open(os.path.join(ROOT, "include", "wbx.h")).read()
    assert re.search(r"wbx_onset_frame\s*\{\s*/\* 32 bytes \*/", text) and re.search(r"wbx_onset_info\s*\{\s*/\* 24 bytes \*/", text)


def test_adapter_with_onsets_compiles(tmp_path):
    """tests/cpp/adapter_onsets.cpp uses Engine::onsets_sample and Engine::tempo_sample; it is compiled and linked here and
    run by tests/test_gpu_onsets.py (it needs a device)"""
    exe = str(tmp_path / "adapter_onsets")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_onsets.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    oi, fi, ms = _ffi.OnsetInfo(), _ffi.F0Info(), C.c_double(5.0)
    oi.hops, fi.hops = 123, 321
    rec = np.zeros(8, dtype=M.DTYPE)
    rec["onset"] = 9
    trk = np.zeros(8, dtype=F0.DTYPE)
    trk["lag"] = 9
    assert L.wbx_clip_onsets(None, 0, 0, 2048, 256, 1e-9, 0.3, 0.1, 3, 8, rec.ctypes.data, 8, C.byref(oi)) == -4
    assert L.wbx_engine_onsets_sample(None, 0, 0, 2048, 256, 1e-9, 0.3, 0.1, 3, 8, rec.ctypes.data, 8, C.byref(oi)) == -4
    assert L.wbx_clip_tempo(None, 0, 0, 1 << 20, 256, 1e-9, 1024, 64, 56, 188, 0.5, trk.ctypes.data, 8, C.byref(fi)) == -4
    assert L.wbx_engine_tempo_sample(None, 0, 0, 1 << 20, 256, 1e-9, 1024, 64, 56, 188, 0.5, trk.ctypes.data, 8, C.byref(fi)) == -4
    assert L.wbx_onset_ms(None, C.byref(ms)) == -4 and ms.value == 5.0
    assert oi.hops == 123 and fi.hops == 321 and np.all(rec["onset"] == 9) and np.all(trk["lag"] == 9)


# ---- wbx_onset_hops, wbx_onset_check ------------------------------------------------------------------------------------------
EDGE = M.MAX_FRAMES - 1
OK = dict(n=4000, H=256, fl=1e-9, thr=0.3, delta=0.1, w=3, a=8, out=True, cap=None)
NAN, INF = float("nan"), float("inf")
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=M.MAX_FRAMES), -4), (dict(n=1 << 63), -4), (dict(n=EDGE, H=16384, cap=1 << 20), 0), (dict(n=1), 0),
          (dict(H=0), -4), (dict(H=32), -4), (dict(H=64), 0), (dict(H=65), -4), (dict(H=96), -4), (dict(H=320), 0), (dict(H=16384), 0),
          (dict(H=16448), -4), (dict(H=1 << 31), -4),
          (dict(fl=1e-30), 0), (dict(fl=0.9e-30), -4), (dict(fl=0.0), -4), (dict(fl=1.0), 0), (dict(fl=1.0000001), -4), (dict(fl=-1e-9), -4),
          (dict(fl=NAN), -4), (dict(fl=INF), -4),
          (dict(thr=0.0), -4), (dict(thr=-0.5), -4), (dict(thr=5e-324), 0), (dict(thr=2.0), 0), (dict(thr=2.0000001), -4), (dict(thr=NAN), -4),
          (dict(thr=INF), -4),
          (dict(delta=0.0), 0), (dict(delta=-1e-300), -4), (dict(delta=2.0), 0), (dict(delta=2.0000001), -4), (dict(delta=NAN), -4),
          (dict(delta=-INF), -4),
          (dict(w=0), 0), (dict(w=64), 0), (dict(w=65), -4), (dict(w=(1 << 32) - 1), -4),
          (dict(a=0), 0), (dict(a=256), 0), (dict(a=257), -4), (dict(a=(1 << 32) - 1), -4),
          (dict(out=False), -4), (dict(out=False, n=255), 0),     # no hops need no buffer
          (dict(cap=14), -4), (dict(cap=15), 0), (dict(cap=0), -4), (dict(cap=0, n=255), 0),   # 4000 // 256 = 15 hops
          (dict(n=255), 0), (dict(n=256, cap=0), -4), (dict(n=256, cap=1), 0),
          (dict(n=64 << 20, H=64, cap=1 << 20), 0),                                   # 2^20 hops: the most
          (dict(n=(64 << 20) + 63, H=64, cap=1 << 20), 0),
          (dict(n=(64 << 20) + 64, H=64, cap=(1 << 20) + 1), -3),                    # one more
          (dict(n=(64 << 20) + 64, H=64, cap=1 << 20), -4),                          # the capacity is asked first
          (dict(n=(64 << 20) + 64, H=64, out=False, cap=1 << 21), -4),
          (dict(n=EDGE, H=64, cap=1 << 40), -3), (dict(n=EDGE, H=65, cap=1 << 40), -4), (dict(n=EDGE, H=64, w=65, cap=1 << 40), -4)]
TEMPO_OK = dict(n=1 << 20, H=256, fl=1e-9, W=1024, step=64, lo=56, hi=188, thr=0.5, out=True, cap=None)
TEMPO_CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=M.MAX_FRAMES), -4), (dict(H=100), -4), (dict(fl=0.0), -4), (dict(fl=NAN), -4),
                (dict(W=1020), -4), (dict(W=8200), -4), (dict(step=0), -4), (dict(lo=1), -4), (dict(lo=188), -4), (dict(hi=4096), -4),
                (dict(thr=0.0), -4), (dict(thr=1.5), -4), (dict(thr=NAN), -4),
                (dict(n=255), 0), (dict(n=255, out=False, cap=0), 0), (dict(n=255, W=1020), -4),   # no hops: the shape alone
                (dict(n=256 * 1211), 0), (dict(n=256 * 1211, out=False, cap=0), 0),              # hops, but no window yet
                (dict(n=256 * 1212, out=False), -4), (dict(n=256 * 1212, cap=0), -4), (dict(n=256 * 1212, cap=1), 0),
                (dict(cap=45), -4), (dict(cap=46), 0),                                           # (4096 - 1212) // 64 + 1 = 46 windows
                (dict(n=64 << 20, H=64, cap=1 << 20), 0), (dict(n=(64 << 20) + 64, H=64, cap=1 << 21), -3),
                (dict(n=(64 << 20) + 64, H=64, W=1020, cap=1 << 21), -3)]                      # the hops are judged before the track


def lib_check(a):
    cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["H"])
    return W.lib().wbx_onset_check(a["n"], a["H"], a["fl"], a["thr"], a["delta"], a["w"], a["a"], int(a["out"]), cap)


def test_check_every_refusal_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check(a["n"], a["H"], a["fl"], a["thr"], a["delta"], a["w"], a["a"], a["out"], a["cap"]) == want, change
        assert lib_check(a) == want, change
    assert {w for _, w in CHECKS} == {0, -4, -3}
    for change, want in TEMPO_CHECKS:
        a = dict(TEMPO_OK, **change)
        assert M.tempo_check(a["n"], a["H"], a["fl"], a["W"], a["step"], a["lo"], a["hi"], a["thr"], a["out"], a["cap"]) == want, change
    assert {w for _, w in TEMPO_CHECKS} == {0, -4, -3}


def test_hops_equal_the_model_over_a_grid():
    rng = np.random.default_rng(0x0A5E7)
    for Hn in (64, 128, 192, 256, 320, 1024, 4096, 16384):
        ns = [0, 1, Hn - 1, Hn, Hn + 1, 17 * Hn - 1, 17 * Hn, EDGE, EDGE + 1, 1 << 40, (1 << 64) - 1] + [int(v) for v in rng.integers(1, EDGE, 10)]
        for n in ns:
            assert W.onset_hops(n, Hn) == M.hops(n, Hn) == n // Hn, (n, Hn)
    for Hn in (0, 1, 32, 63, 65, 100, 16384 + 64, 1 << 20):
        assert W.onset_hops(1 << 24, Hn) == 0 == M.hops(1 << 24, Hn)     # a refused hop length


# ---- the pick ---------------------------------------------------------------------------------------------------------------
def curves():
    """novelty curves with plateaus of equal values, peaks on the first and last hop, zeros, and lengths around w and a"""
    rng = np.random.default_rng(0x91C)
    out = [np.zeros(0, dtype=np.float32), np.array([0.5], dtype=np.float32), np.array([0.5, 0.5], dtype=np.float32),
           np.array([1.0, 0.2, 0.2, 1.0], dtype=np.float32), np.full(40, 0.7, dtype=np.float32), np.zeros(33, dtype=np.float32)]
    for n in (3, 17, 64, 200, 700):
        o = (rng.random(n) ** 4 * 1.9).astype(np.float32)
        o[rng.random(n) < 0.3] = 0.0
        out.append(o)
        q = (np.round(rng.random(n) * 6) / np.float32(4.0)).astype(np.float32)    # few levels: many equals and plateaus
        q[0] = q[-1] = 1.75
        out.append(q)
    return out


PICKS = [(0.3, 0.1, 3, 8), (0.3, 0.0, 0, 0), (5e-324, 0.0, 1, 0), (2.0, 0.0, 3, 8), (0.25, 2.0, 3, 8), (0.25, 0.05, 64, 256), (0.5, 0.25, 0, 256),
         (0.5, 0.0, 64, 0), (0.75, 0.1, 1, 1), (1.75, 0.0, 2, 3)]


def lib_pick(o, thr, delta, w, a):
    rec = np.zeros(len(o), dtype=M.DTYPE)
    rec["novelty"], rec["onset"], rec["energy"] = o.astype(np.float64), 7, 3.0
    count = C.c_uint64(99)
    st = W.lib().wbx_onset_pick(rec.ctypes.data if len(o) else None, len(o), thr, delta, w, a, C.byref(count))
    assert st == 0 and np.all(rec["energy"] == 3.0) and np.array_equal(rec["novelty"], o.astype(np.float64)) and not rec["_pad"].any()
    return rec["onset"], count.value


def slow_pick(o, thr, delta, w, a):
    """the header's four conditions, hop by hop in plain Python"""
    o = [float(v) for v in o]
    out = []
    for h in range(len(o)):
        on = o[h] >= thr and all(not o[g] >= o[h] for g in range(max(0, h - w), h))
        on = on and all(not o[g] > o[h] for g in range(h + 1, min(len(o) - 1, h + w) + 1))
        m, cnt = 0.0, 0
        for g in range(max(0, h - a), min(len(o) - 1, h + a) + 1):
            m, cnt = m + o[g], cnt + 1
        out.append(1 if on and o[h] >= m / cnt + delta else 0)
    return np.array(out, dtype=np.uint32)


def test_pick_equals_the_model_on_plateaus_and_at_both_ends():
    seen_first = seen_last = seen_plateau = 0
    for o in curves():
        for thr, delta, w, a in PICKS:
            want = M.pick(o, thr, delta, w, a)
            got, count = lib_pick(o, thr, delta, w, a)
            assert np.array_equal(got, want) and count == int(want.sum()), (len(o), thr, delta, w, a)
            assert np.array_equal(want, slow_pick(o, thr, delta, w, a)), (len(o), thr, delta, w, a)
            if len(o):
                seen_first += int(want[0])
                seen_last += int(want[-1])
            if w and len(o) > 1:
                assert not np.any(want[1:] & want[:-1])           # of equal neighbours only the earliest
                seen_plateau += int(np.any((np.diff(o) == 0) & (want[:-1] == 1)))
    assert seen_first > 5 and seen_last > 5 and seen_plateau > 5
    L = W.lib()
    rec = np.zeros(4, dtype=M.DTYPE)
    rec["onset"] = 7
    for bad in ((0.0, 0.1, 3, 8), (NAN, 0.1, 3, 8), (2.5, 0.1, 3, 8), (0.3, -0.1, 3, 8), (0.3, NAN, 3, 8), (0.3, 2.5, 3, 8), (0.3, 0.1, 65, 8),
                (0.3, 0.1, 3, 257)):
        assert L.wbx_onset_pick(rec.ctypes.data, 4, *bad, None) == -4 and np.all(rec["onset"] == 7), bad
    assert L.wbx_onset_pick(None, 4, 0.3, 0.1, 3, 8, None) == -4 and L.wbx_onset_pick(None, 0, 0.3, 0.1, 3, 8, None) == 0
    assert L.wbx_onset_pick(rec.ctypes.data, 4, 0.3, 0.1, 3, 8, None) == 0 and not rec["onset"].any()


# ---- properties of the model --------------------------------------------------------------------------------------------------
def test_energies_are_the_plain_sums_within_rounding():
    """A and B of the model against np.sum of the squares: the order differs, the values agree to 1e-13 relative; d[-1] = 0"""
    rng = np.random.default_rng(5)
    for Hn in (64, 128, 320, 16384):
        d = rng.standard_normal(3 * Hn + 17).astype(np.float32).astype(np.float64)
        A, B = M.energies(d, Hn)
        assert len(A) == 3 == len(B)
        e = np.diff(np.concatenate([[0.0], d]))
        for h in range(3):
            assert abs(A[h] / np.sum(d[h * Hn:(h + 1) * Hn] ** 2) - 1) < 1e-13 and abs(B[h] / np.sum(e[h * Hn:(h + 1) * Hn] ** 2) - 1) < 1e-13


def bpm_of(rec):
    track = F0.track(rec["novelty"], TEMPO["W"], TEMPO["step"], TEMPO["lag_min"], TEMPO["lag_max"], TEMPO["threshold"])
    assert len(track) == 23 and np.all(track["voiced"] == 1), track
    return 60.0 * RATE / (H * track["period"])


@pytest.mark.parametrize("bpm,octave", [(120, 1), (128, 1), (174, 1), (72, 2), (93, 2)])
def test_drum_loops_give_their_tempo_in_every_window(loops, bpm, octave):
    """14 s loops at 48 kHz, H = 256, windows of 1024 hops every 64, lags of 200 .. 60 bpm, threshold 0.5: every window is
    voiced and within TEMPO_BOUND = 0.406 % of the true tempo — of its double for the 72 and 93 bpm loops, whose eighths
    fall inside the lag range.  Measured on the model: 0.132, 0.067, 0.203, 0.116 and 0.105 %"""
    est = bpm_of(loops[bpm][0])
    err = float(np.abs(est / (octave * bpm) - 1.0).max())
    print("%d bpm: %.3f .. %.3f, worst error %.3f %%" % (bpm, est.min(), est.max(), 100 * err))
    assert err <= TEMPO_BOUND, (bpm, est)


@pytest.mark.parametrize("bpm", [120, 128, 174, 72, 93])
def test_drum_loops_give_their_onsets_within_a_hop(loops, bpm):
    """every true onset has a picked one within one hop, and the picked ones without a true one are at most a quarter of the
    true count (measured: 1 .. 4 extras for 34 .. 81 onsets)"""
    rec, at = loops[bpm]
    found = np.flatnonzero(rec["onset"])
    missed = [int(t) for t in at if not np.any(np.abs(found - t // H) <= 1)]
    extra = [int(f) for f in found if not np.any(np.abs(f - at // H) <= 1)]
    print("%d bpm: %d true, %d found, %d extra" % (bpm, len(at), len(found), len(extra)))
    assert not missed and 4 * len(extra) <= len(at), (missed, extra)
    assert np.all(rec["novelty"] >= 0.0) and np.all(rec["novelty"] <= 2.0)


def test_silence_gives_no_novelty_and_a_steady_sine_one_onset():
    rec = M.records(np.zeros(20000), H, 1e-9, 0.3, 0.1, 3, 8)
    assert len(rec) == 78 and not rec["novelty"].any() and not rec["onset"].any() and not rec["energy"].any()
    tone = np.sin(2 * np.pi * 440.0 * np.arange(RATE) / RATE).astype(np.float32).astype(np.float64)
    rec = M.records(tone, H, 1e-9, 0.3, 0.1, 3, 8)
    assert list(np.flatnonzero(rec["onset"])) == [0]


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def shape_of(Hn, hops):
    """wbx_onset.h's onset_shape: (q, row, grid, lds_bytes)"""
    q = Hn // 64
    row = 0 if q in (1, 2, 4) else (min(q, 32) | 1)
    return q, row, min(-(-hops // 4), 2048), 4 * 64 * row * 4


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/onset_main.cpp: wbx_onset.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "onset_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onset_main.cpp"), "-o", exe])
    lines, want = [], []
    for Hn in (64, 128, 192, 320, 16384, 0, 63, 100, 16448):
        for n in (0, 1, Hn - 1 if Hn else 5, Hn, 17 * Hn + 3, EDGE, (1 << 64) - 1):
            lines.append("h %d %d" % (n, Hn))
            want.append("h %d" % M.hops(n, Hn))
    for change, status in CHECKS:
        a = dict(OK, **change)
        cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["H"])
        lines.append("c %d %d %r %r %r %d %d %d %d" % (a["n"], a["H"], a["fl"], a["thr"], a["delta"], a["w"], a["a"], a["out"], cap))
        want.append("c %d" % status)
    for change, status in TEMPO_CHECKS:
        a = dict(TEMPO_OK, **change)
        cap = a["cap"] if a["cap"] is not None else F0.hops(M.hops(a["n"], a["H"]), a["W"], a["step"], a["hi"])
        lines.append("t %d %d %r %d %d %d %d %r %d %d" % (a["n"], a["H"], a["fl"], a["W"], a["step"], a["lo"], a["hi"], a["thr"], a["out"], cap))
        want.append("t %d" % status)
    rows = set()
    for Hn in range(64, 16384 + 1, 64):
        for hops in ((0, 1, 5, 8191, 8192, 8193, 1 << 20) if Hn in (64, 320, 16384) else (9,)):
            lines.append("s %d %d" % (Hn, hops))
            want.append("s %d %d %d %d" % shape_of(Hn, hops))
            rows.add(shape_of(Hn, hops)[1])
    assert rows == {0} | set(range(3, 34, 2))
    for o in curves():
        for thr, delta, w, a in PICKS:
            flags = M.pick(o, thr, delta, w, a)
            lines.append("p %r %r %d %d %d %s" % (thr, delta, w, a, len(o), " ".join("%.9g" % v for v in o)))
            want.append("p %d %s" % (int(flags.sum()), "".join(str(int(f)) for f in flags)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.rstrip("\n").split("\n")
    assert got[-1] == "onset ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g.rstrip() == w.rstrip(), line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
