"""Seeing a clip's spectrum, the part that needs no device: the symbols of include/wbx.h "Seeing a clip's spectrum" exist and
match their binding twins, the info struct has the header's layout, the adapter's method compiles, NULL handles are refused,
wbx_spectrum_hops / _check / _launch_hops / _basis_frames equal the Python twin (tests/spectrum_model.py), every refusal of
the argument check, wbx_spectrum_basis and wbx_spectrum_log_freqs equal the model bit for bit, the model itself gives the
known answers of a windowed transform — and wbx_spectrum.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spectrum_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_spectrum_hops", "wbx_spectrum_check", "wbx_spectrum_max_cells", "wbx_spectrum_launch_terms", "wbx_spectrum_launch_hops",
       "wbx_spectrum_basis_frames", "wbx_spectrum_basis", "wbx_spectrum_log_freqs", "wbx_spectrum_ms", "wbx_clip_spectrum",
       "wbx_engine_spectrum_sample"]
KINDS = {"rect": M.RECT, "hann": M.HANN, "kaiser": M.KAISER}


@pytest.fixture(autouse=True)
def library_with_spectrum():
    """every test here, those of the model alone included, stands on a library that has the calls: the model is the reference
    of tests/test_gpu_spectrum.py and means nothing without them"""
    L = W.lib()
    assert all(hasattr(L, n) for n in NEW)


def terms():
    return int(W.lib().wbx_spectrum_launch_terms())


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.spectrum_hops) and callable(W.spectrum_basis) and callable(W.spectrum_log_freqs)
    assert W.SPECTRUM_MID == M.MID == 2 and re.search(r"#define WBX_SPECTRUM_MID 2u", header)
    assert re.search(r"WBX_WINDOW_RECT = 0, WBX_WINDOW_HANN = 1, WBX_WINDOW_KAISER = 2", header) and _ffi.WINDOW_KIND == KINDS
    assert hasattr(W.MixContext, "clip_spectrum") and hasattr(W.MixContext, "spectrum_ms")
    for m in ("add_spectrum_basis", "spectrum_sample", "spectrogram_sample", "chroma_sample"):
        assert hasattr(W.Engine, m), m
    assert L.wbx_spectrum_max_cells() == 1 << 25 == M.MAX_CELLS and L.wbx_spectrum_launch_terms() >= 2 * M.MAX_BASIS * 16
    assert "spectrum_sample" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    info = ["hops", "bins", "launches"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * len(info)
                   + '\\n", sizeof(wbx_spectrum_info), ' + ", ".join("offsetof(wbx_spectrum_info, %s)" % f for f in info) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    I = _ffi.SpectrumInfo
    assert got == [16, 0, 8, 12]
    assert got == [C.sizeof(I)] + [getattr(I, f).offset for f in info]
    assert re.search(r"wbx_spectrum_info\s*\{\s*/\* 16 bytes \*/", open(os.path.join(ROOT, "include", "wbx.h")).read())


def test_adapter_with_spectrum_compiles(tmp_path):
    """tests/cpp/adapter_spectrum.cpp uses Engine::spectrum_sample; it is compiled and linked here and run by
    tests/test_gpu_spectrum.py (it needs a device)"""
    exe = str(tmp_path / "adapter_spectrum")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_spectrum.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_arguments_are_refused_without_a_device():
    L = W.lib()
    si, ms = _ffi.SpectrumInfo(), C.c_double(5.0)
    si.hops = 123
    cells = np.full(64, 9.0, dtype=np.float32)
    assert L.wbx_clip_spectrum(None, 0, 0, 4000, 2, 1, 256, 4, 64, cells.ctypes.data, 64, C.byref(si)) == -4
    assert L.wbx_engine_spectrum_sample(None, 0, 0, 4000, 2, 1, 256, 4, 64, cells.ctypes.data, 64, C.byref(si)) == -4
    assert L.wbx_spectrum_ms(None, C.byref(ms)) == -4 and ms.value == 5.0 and si.hops == 123 and np.all(cells == 9.0)
    f = np.array([0.1, 0.2], dtype=np.float64)
    out = np.full(2 * 2 * 32, 9.0, dtype=np.float32)
    assert L.wbx_spectrum_basis(32, 2, None, None, 1, 0.0, out.ctypes.data) == -4
    assert L.wbx_spectrum_basis(32, 2, f.ctypes.data, None, 1, 0.0, None) == -4
    assert L.wbx_spectrum_log_freqs(0.01, 12.0, 2, None, None) == -4 and np.all(out == 9.0)
    assert L.wbx_spectrum_log_freqs(0.01, 12.0, 2, f.ctypes.data, None) == 0 and f[0] == 0.01      # clamped may be NULL


# ---- wbx_spectrum_hops, wbx_spectrum_check, the launches ------------------------------------------------------------------------
EDGE = M.MAX_FRAMES - 1
OK = dict(n=4000, ch=M.MID, W=256, B=8, H=64, out=True, cap=None)
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=M.MAX_FRAMES), -4), (dict(n=1 << 63), -4), (dict(n=EDGE, H=65536, B=1), 0), (dict(n=1), 0),
          (dict(ch=0), 0), (dict(ch=1), 0), (dict(ch=3), -4), (dict(ch=0xFFFFFFFF), -4),
          (dict(W=28), -4), (dict(W=32), 0), (dict(W=34), -4), (dict(W=36), 0), (dict(W=8192), 0), (dict(W=8196), -4), (dict(W=0), -4),
          (dict(B=0), -4), (dict(B=1), 0), (dict(B=1024), 0), (dict(B=1025), -4), (dict(W=8192, B=256), 0), (dict(W=8192, B=257), -4),
          (dict(W=2048, B=1024), 0), (dict(W=2052, B=1024), -4),
          (dict(H=0), -4), (dict(H=1), 0), (dict(H=65536), 0), (dict(H=65537), -4),
          (dict(out=False), -4), (dict(out=False, n=255), 0),    # no hops need no buffer
          (dict(cap=471), -4), (dict(cap=472), 0), (dict(cap=0), -4), (dict(cap=0, n=255), 0),   # (4000 - 256) // 64 + 1 = 59 hops of 8 bins
          (dict(n=255), 0), (dict(n=256, cap=7), -4), (dict(n=256, cap=8), 0),
          (dict(n=32 + (1 << 20) - 1, W=32, H=1, B=1), 0),                                       # 2^20 hops: the most
          (dict(n=32 + (1 << 20), W=32, H=1, B=1, cap=(1 << 20) + 1), -3),                       # one more
          (dict(n=32 + (1 << 20), W=32, H=1, B=1, cap=1 << 20), -4),                             # the capacity is asked first
          (dict(n=32 + (1 << 20), W=32, H=1, B=1, out=False, cap=1 << 21), -4),
          (dict(n=32 + (1 << 19) - 1, W=32, H=1, B=64), 0),                                      # 2^25 cells: the most
          (dict(n=32 + (1 << 19), W=32, H=1, B=64), -3),                                         # 64 more
          (dict(n=32 + (1 << 19), W=32, H=1, B=64, cap=1 << 25), -4),
          (dict(n=EDGE, H=1, cap=1 << 40), -3), (dict(n=EDGE, H=1, W=34, cap=1 << 40), -4)]


def lib_check(a):
    cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["W"], a["H"]) * a["B"]
    return W.lib().wbx_spectrum_check(a["n"], a["ch"], a["W"], a["B"], a["H"], int(a["out"]), cap)


def test_check_every_refusal_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check(a["n"], a["ch"], a["W"], a["B"], a["H"], a["out"], a["cap"]) == want, change
        assert lib_check(a) == want, change
    assert {w for _, w in CHECKS} == {0, -4, -3}


def test_hops_and_basis_frames_equal_the_model_over_a_grid():
    rng = np.random.default_rng(0x5BEC)
    assert W.spectrum_hops(255, 256, 64) == 0 == M.hops(255, 256, 64) and W.spectrum_hops(256, 256, 64) == 1 == M.hops(256, 256, 64)
    for Wn, H in [(32, 1), (36, 7), (256, 64), (2048, 512), (8192, 65536), (256, 261)]:
        ns = [0, 1, Wn - 1, Wn, Wn + 1, Wn + H - 1, Wn + H, Wn + H + 1, Wn + 17 * H - 1, EDGE, EDGE + 1, 1 << 40, (1 << 64) - 1]
        ns += [int(v) for v in rng.integers(1, EDGE, 10)]
        for n in ns:
            want = M.hops(n, Wn, H)
            assert W.spectrum_hops(n, Wn, H) == want, (n, Wn, H)
            assert want == (0 if n < Wn else (n - Wn) // H + 1)
    for Wn, H in [(28, 1), (34, 1), (8196, 1), (32, 0), (32, 65537)]:
        assert W.spectrum_hops(1 << 20, Wn, H) == 0 == M.hops(1 << 20, Wn, H)                  # a refused shape
    L = W.lib()
    for Wn, B in [(32, 1), (36, 7), (256, 130), (2048, 1024), (8192, 256), (8192, 257), (34, 4), (32, 0), (32, 1025)]:
        assert L.wbx_spectrum_basis_frames(Wn, B) == M.basis_frames(Wn, B), (Wn, B)
    assert M.basis_frames(8192, 256) == 1 << 22 and M.basis_frames(8192, 257) == 0


def test_launch_hops_equal_the_model():
    L, T = W.lib(), terms()
    seen = set()
    for Wn in (32, 36, 256, 1024, 2048, 8192):
        for B in (1, 2, 7, 64, 65, 130, 256, 1024):
            per = L.wbx_spectrum_launch_hops(Wn, B)
            assert per == M.launch_hops(Wn, B, T), (Wn, B)
            if B * Wn > M.MAX_BASIS:
                assert per == 0
                continue
            assert per >= 4096 and per % 32 == 0 and per * Wn * 2 * B <= T and per * B <= M.STAGE_CELLS and per <= 1 << 20
            seen.add(per)
    assert len(seen) > 3
    assert L.wbx_spectrum_launch_hops(34, 8) == 0 and L.wbx_spectrum_launch_hops(32, 0) == 0 and L.wbx_spectrum_launch_hops(32, 1025) == 0


# ---- the basis and the frequencies, bit for bit -----------------------------------------------------------------------------------
def basis_cases():
    """(W, B, freqs, lengths or None, kind, beta): every window length of the issue, the three kinds, per-bin lengths, f = 0,
    0.5 and irrational values"""
    rng = np.random.default_rng(0xBA5)
    out = []
    for Wn, B in ((32, 5), (36, 7), (256, 9), (8192, 4)):
        f = np.concatenate([[0.0, 0.5, 1.0 / np.sqrt(2.0) / 2.0, np.pi / 100.0], rng.random(B - 4) * 0.5])
        ln = np.concatenate([[4, Wn, Wn - 1, 5], rng.integers(4, Wn + 1, B - 4)]).astype(np.uint32)
        for kind, beta in (("rect", 0.0), ("hann", 0.0), ("kaiser", 8.6), ("kaiser", 0.0), ("kaiser", 20.0)):
            for lengths in (None, ln):
                if Wn == 8192 and (kind == "kaiser" and beta != 8.6 or lengths is None and kind == "rect"):
                    continue                                     # (the longest window once per kind)
                out.append((Wn, B, f, lengths, kind, beta))
    return out


def test_basis_equals_the_model_bit_for_bit():
    for Wn, B, f, lengths, kind, beta in basis_cases():
        got = W.spectrum_basis(Wn, f, lengths, kind, beta)
        want = M.basis(Wn, B, f, lengths, KINDS[kind], beta)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (2 * B * Wn,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (Wn, B, kind, beta, lengths is None)
        tab = got.reshape(Wn, B, 2)
        assert np.all(tab[:, 0, 1] == 0.0) and np.all(tab[:, 0, 0] >= 0.0)                      # f = 0: C = wn, S = -0 or 0
        if lengths is not None:                                  # zero outside each bin's own window, centred
            for b in range(B):
                off = (Wn - int(lengths[b])) // 2
                assert not tab[:off, b].any() and not tab[off + int(lengths[b]):, b].any() and tab[off, b, 0] != 0.0
        assert abs(float(tab[:, 0, 0].astype(np.float64).sum()) - 1.0) < 1e-6                   # the window sums to 1


def test_basis_refusals():
    L = W.lib()
    f = np.array([0.1, 0.2, 0.3], dtype=np.float64)
    out = np.full(2 * 3 * 32, 9.0, dtype=np.float32)
    ln = np.array([4, 32, 16], dtype=np.uint32)

    def call(Wn=32, B=3, freqs=f, lengths=None, kind=1, beta=0.0):
        fr = np.ascontiguousarray(freqs, dtype=np.float64)
        st = L.wbx_spectrum_basis(Wn, B, fr.ctypes.data, None if lengths is None else lengths.ctypes.data, kind, beta, out.ctypes.data)
        assert st == 0 or np.all(out == 9.0)
        return st

    for bad in (dict(Wn=28), dict(Wn=34), dict(B=0), dict(B=1025), dict(kind=3), dict(kind=-1), dict(kind=2, beta=-0.1), dict(kind=2, beta=20.5),
                dict(kind=2, beta=float("nan")), dict(freqs=[0.1, -1e-9, 0.3]), dict(freqs=[0.1, 0.5000001, 0.3]),
                dict(freqs=[0.1, float("nan"), 0.3]), dict(lengths=np.array([3, 32, 16], dtype=np.uint32)),
                dict(lengths=np.array([4, 33, 16], dtype=np.uint32))):
        assert call(**bad) == -4, bad
        assert M.basis(bad.get("Wn", 32), bad.get("B", 3), bad.get("freqs", f), bad.get("lengths"), bad.get("kind", 1), bad.get("beta", 0.0)) is None, bad
    assert call(kind=1, beta=float("nan")) == 0                  # beta is the Kaiser window's alone
    assert call(lengths=ln, kind=2, beta=20.0) == 0
    with pytest.raises(W.WbxError) as err:
        W.spectrum_basis(34, f)
    assert err.value.status == -4


def test_log_freqs_equal_the_model_bit_for_bit():
    for f_min, bpo, B in [(0.001, 12.0, 130), (0.0005, 24.0, 240), (55.0 / 48000.0, 12.0, 60), (0.01, 3.5, 64), (0.5, 12.0, 4), (1e-300, 1.0, 1024),
                          (0.25, 1.0, 3), (0.001, 1e-3, 5), (5e-324, 12.0, 8)]:
        got, clamped = W.spectrum_log_freqs(f_min, bpo, B)
        want, want_clamped = M.log_freqs(f_min, bpo, B)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (f_min, bpo, B)
        assert clamped == want_clamped and clamped <= int((got == 0.5).sum()), (f_min, bpo, B)
        assert got[0] == f_min and np.all(np.diff(got) >= 0.0) and got.max() <= 0.5
    f, c = W.spectrum_log_freqs(0.001, 12.0, 130)
    assert c == 22 and abs(f[12] / f[0] - 2.0) < 1e-15 and abs(f[1] / f[0] - 2.0 ** (1.0 / 12.0)) < 1e-15
    f, c = W.spectrum_log_freqs(0.25, 1.0, 3)
    assert list(f) == [0.25, 0.5, 0.5] and c == 1                # exactly 0.5 is not clamped, 1.0 is
    L = W.lib()
    out = np.full(4, 9.0, dtype=np.float64)
    for f_min, bpo, B in [(0.0, 12.0, 4), (-0.1, 12.0, 4), (0.5000001, 12.0, 4), (float("nan"), 12.0, 4), (0.01, 0.0, 4), (0.01, -1.0, 4),
                          (0.01, float("inf"), 4), (0.01, float("nan"), 4), (0.01, 12.0, 0), (0.01, 12.0, 1025)]:
        assert L.wbx_spectrum_log_freqs(f_min, bpo, B, out.ctypes.data, None) == -4 and np.all(out == 9.0), (f_min, bpo, B)


# ---- known answers on the model -----------------------------------------------------------------------------------------------------
def tone(f, n, amp=0.5, phase=0.3):
    return (amp * np.sin(2.0 * np.pi * (f * np.arange(n, dtype=np.float64)) + phase)).astype(np.float32).astype(np.float64)


def test_a_tone_on_its_bin_its_neighbour_and_far_bins():
    """a tone of amplitude 0.5 at 0.1 cycles per frame, W = 256, Hann, against the sinpi-built basis: its bin reads
    0.5^2 / 4 = 0.0625 within 1e-4 relative (measured: see the print), the bin 1 / W away a quarter of that within 1e-3 (a
    Hann window's first neighbour has half the amplitude), bins k / W away with k = 4 or more below 1e-9 (whole k: there this
    window's transform has its zeros, and what is left is the tone's image at -0.1)"""
    Wn = 256
    offs = [0, 1, -1, 4, -4, 5, 8, 20, 60, -24]
    freqs = np.array([0.1 + k / Wn for k in offs])
    words = M.basis(Wn, len(freqs), freqs, None, M.HANN)
    p = M.power(tone(0.1, Wn + 3 * 64), words, Wn, len(freqs), 64).astype(np.float64)
    assert p.shape == (4, len(freqs))
    on, near, far = p[:, 0], p[:, 1:3], p[:, 3:]
    print("on-bin error %.3e, neighbour error %.3e, far max %.3e" % (np.abs(on / 0.0625 - 1).max(), np.abs(near / (0.0625 / 4) - 1).max(), far.max()))
    assert np.all(np.abs(on / 0.0625 - 1.0) < 1e-4)
    assert np.all(np.abs(near / (0.0625 / 4.0) - 1.0) < 1e-3)
    assert np.all(far < 1e-9)
    full = M.power(tone(0.1, Wn, amp=1.0), words[:], Wn, len(freqs), 64).astype(np.float64)
    assert abs(full[0, 0] / 0.25 - 1.0) < 1e-4                   # a full-scale sine on a bin has power 0.25


def test_rectangular_bins_at_k_over_w_equal_numpys_rfft_power():
    """a rectangular window with f_b = k / W is the DFT divided by W: the powers equal |rfft|^2 / W^2 within 1e-6 relative
    (of the row's largest: bins that cancel to nothing have no relative error to speak of)"""
    rng = np.random.default_rng(0xFF7)
    for Wn in (32, 36, 256):
        x = (rng.standard_normal(Wn + 2 * 16) * 0.3).astype(np.float32).astype(np.float64)
        freqs = np.arange(Wn // 2 + 1) / Wn
        words = M.basis(Wn, len(freqs), freqs, None, M.RECT)
        p = M.power(x, words, Wn, len(freqs), 16).astype(np.float64)
        for h in range(3):
            want = np.abs(np.fft.rfft(x[16 * h:16 * h + Wn])) ** 2 / Wn ** 2
            rel = np.abs(p[h] - want).max() / want.max()
            assert rel < 1e-6, (Wn, h, rel)
            big = want > 1e-3 * want.max()
            assert np.all(np.abs(p[h][big] / want[big] - 1.0) < 1e-6), np.abs(p[h][big] / want[big] - 1.0).max()


def test_the_chroma_of_an_a_major_triad():
    """A3 + C#4 + E4 at 48 kHz through a semitone basis over 5 octaves from C1, constant-Q windows, folded by chroma_fold: the
    three largest classes are A (9), C# (1) and E (4)"""
    rate, Wn, octaves = 48000.0, 8192, 5
    c1 = 440.0 * 2.0 ** (-45.0 / 12.0) / rate                     # C1 = 45 semitones below A4
    freqs, clamped = M.log_freqs(c1, 12.0, 12 * octaves)
    assert clamped == 0
    lengths = M.constant_q_lengths(freqs, Wn, Wn * freqs[36])    # the full window at C4, shorter above, capped below
    words = M.basis(Wn, len(freqs), freqs, lengths, M.HANN)
    n = Wn + 2048
    x = sum(tone(440.0 * 2.0 ** (k / 12.0) / rate, n, amp=0.3, phase=0.1 * k) for k in (-12, -8, -5))
    x = x.astype(np.float32).astype(np.float64)
    chroma = M.chroma_fold(M.power(x, words, Wn, len(freqs), 2048), octaves)
    assert chroma.shape == (2, 12)
    for row in chroma:
        assert set(np.argsort(row)[-3:]) == {9, 1, 4}, row
        assert np.sort(row)[-3] > 4.0 * np.sort(row)[-4]


def test_only_picks_hops_of_the_whole_spectrum_and_non_finite_basis_rows_stay_in_their_bins():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(900) * 0.3).astype(np.float32).astype(np.float64)
    freqs = rng.random(5) * 0.5
    words = M.basis(36, 5, freqs, None, M.KAISER, 6.0)
    full = M.power(x, words, 36, 5, 7)
    some = [0, 5, len(full) - 1, 3]
    part = M.power(x, words, 36, 5, 7, only=some, chunk=3)
    assert np.array_equal(part.view(np.uint32), np.ascontiguousarray(full[some]).view(np.uint32))
    bad = words.copy().reshape(36, 5, 2)
    bad[3, 2, 0] = np.nan
    bad[9, 4, 1] = np.inf
    hurt = M.power(x, bad.reshape(-1), 36, 5, 7)
    assert np.array_equal(hurt[:, [0, 1, 3]].view(np.uint32), full[:, [0, 1, 3]].view(np.uint32)) and not np.isfinite(hurt[:, [2, 4]]).any()


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def shape_of(Wn, B, H):
    """wbx_spectrum.h's spectrum_shape: (K, G, F, chunk, stride, span)"""
    K = 1 if B <= 64 else 2
    waves, G = -(-B // (64 * K)), 1
    while G < waves and G < 4:
        G *= 2
    F = (4 // G) * (8 // K)
    chunk = min(Wn, 512, 8192 // F)
    stride = min(H, chunk)
    return K, G, F, chunk, stride, (F - 1) * stride + chunk


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/spectrum_main.cpp: wbx_spectrum.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "spectrum_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "spectrum_main.cpp"), "-o", exe])
    T = terms()
    lines, want, words = [], [], []
    for Wn, H in [(32, 1), (36, 7), (256, 64), (8192, 65536), (28, 1), (32, 0)]:
        for n in (0, 1, Wn - 1, Wn, Wn + 17 * max(H, 1), EDGE, (1 << 64) - 1):
            lines.append("h %d %d %d" % (n, Wn, H))
            want.append("h %d" % M.hops(n, Wn, H))
    for change, status in CHECKS:
        a = dict(OK, **change)
        cap = a["cap"] if a["cap"] is not None else M.hops(a["n"], a["W"], a["H"]) * a["B"]
        lines.append("c %d %d %d %d %d %d %d" % (a["n"], a["ch"], a["W"], a["B"], a["H"], a["out"], cap))
        want.append("c %d" % status)
    shapes = set()
    for Wn in (32, 36, 256, 512, 516, 2048, 8192):
        for B in (1, 2, 7, 64, 65, 128, 129, 130, 256, 257, 512, 513, 1024):
            lines.append("l %d %d" % (Wn, B))
            want.append("l %d" % M.launch_hops(Wn, B, T))
            lines.append("f %d %d" % (Wn, B))
            want.append("f %d" % M.basis_frames(Wn, B))
            for hops in (0, 1, 17, 1 << 20):
                lines.append("n %d %d %d" % (hops, Wn, B))
                want.append("n %d" % M.launches(hops, Wn, B, T))
            for H in (1, 7, 64, 511, 512, 513, 1000, 14000, 65536):
                s = shape_of(Wn, B, H)
                assert s[5] <= 8192 and s[1] * s[2] * s[0] == 32
                shapes.add((s[0], s[1], s[2], s[4] == H))
                lines.append("s %d %d %d" % (Wn, B, H))
                want.append("s %d %d %d %d %d %d" % s)
    assert shapes == {(2, G, 16 // G, sh) for G in (1, 2, 4) for sh in (True, False)} | {(1, 1, 32, True), (1, 1, 32, False)}
    for Wn, B, f, lengths, kind, beta in basis_cases():
        lines.append("b %d %d %d %r %d %s%s" % (Wn, B, KINDS[kind], beta, lengths is not None, " ".join(float(v).hex() for v in f),
                                               "" if lengths is None else " " + " ".join(str(int(v)) for v in lengths)))
        want.append("b 0")
        words.append(M.basis(Wn, B, f, lengths, KINDS[kind], beta))
    for line, st in (("b 34 2 1 0.0 0 0x1p-3 0x1p-2", -4), ("b 32 2 3 0.0 0 0x1p-3 0x1p-2", -4), ("b 32 2 1 0.0 0 0x1p-3 nan", -4),
                     ("b 32 2 1 0.0 1 0x1p-3 0x1p-2 3 32", -4), ("b 32 2 2 inf 0 0x1p-3 0x1p-2", -4), ("b 32 1025 1 0.0 0", -4)):
        lines.append(line)
        want.append("b %d" % st)
    for f_min, bpo, B in [(0.001, 12.0, 130), (55.0 / 48000.0, 12.0, 60), (0.01, 3.5, 64), (1e-300, 1.0, 1024), (0.25, 1.0, 3)]:
        f, clamped = M.log_freqs(f_min, bpo, B)
        lines.append("g %s %s %d" % (float(f_min).hex(), float(bpo).hex(), B))
        want.append(("g 0 %d " % clamped) + " ".join(float(v).hex() for v in f))
    for f_min, bpo, B in [("0x0p+0", "0x1.8p+3", 4), ("nan", "0x1.8p+3", 4), ("0x1p-7", "inf", 4), ("0x1p-7", "0x1.8p+3", 0), ("0x1p-7", "0x1.8p+3", 1025)]:
        lines.append("g %s %s %d" % (f_min, bpo, B))
        want.append("g -4 0")
    path, dump = tmp_path / "cases.txt", tmp_path / "words.bin"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path), str(dump)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert got[-1] == "spectrum ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        if w.startswith("g 0"):                                  # (%a and float.hex spell the same double differently)
            gs, ws = g.split(), w.split()
            assert gs[:3] == ws[:3] and [float.fromhex(v) for v in gs[3:]] == [float.fromhex(v) for v in ws[3:]], line[:80]
        else:
            assert g.strip() == w.strip(), line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
    all_words = np.fromfile(str(dump), dtype=np.float32)
    assert np.array_equal(all_words.view(np.uint32), np.concatenate(words).view(np.uint32))
