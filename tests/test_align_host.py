"""Aligning two clips, the part that needs no device: the symbols of include/wbx.h "Aligning two clips" exist and match their
binding twins, the two structs have the header's layout, the adapter's method compiles, NULL handles are refused,
wbx_align_chunks / _check / _band_chunks / _launches equal the Python twin (tests/align_model.py), every refusal of the argument
check in the stated order, the model itself finds moved and inverted copies of seeded noise — and wbx_align.h runs stand-alone
under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_align_check", "wbx_align_chunks", "wbx_align_max_lags", "wbx_align_chunk_frames", "wbx_align_band_chunks",
       "wbx_align_launches", "wbx_align_ms", "wbx_clip_align", "wbx_engine_align_samples"]


@pytest.fixture(autouse=True)
def library_with_align():
    """every test here, those of the model alone included, stands on a library that has the calls: the model is the reference
    of tests/test_gpu_align.py and means nothing without them"""
    L = W.lib()
    assert all(hasattr(L, n) for n in NEW)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.align_check) and callable(W.align_chunks)
    assert W.ALIGN_CURVE_DTYPE == M.CURVE_DTYPE and W.ALIGN_CURVE_DTYPE.itemsize == 16
    assert hasattr(W.MixContext, "clip_align") and hasattr(W.MixContext, "align_ms")
    for m in ("align_samples", "aligned_sample", "measure_latency"):
        assert hasattr(W.Engine, m), m
    flat = re.sub(r"\s*\*\s*", " ", header)
    assert "Aligning two clips" in flat and "two-level order IS the definition" in flat
    assert flat.index("Tracking a clip's pitch: the period") < flat.index("Aligning two clips: by how many") < flat.index("Finding a clip's onsets and tempo: an")
    for word in ("more than 2 channels", "unlinked stereo", "drifts over time", "at render time"):
        assert word in flat[flat.index("Aligning two clips: by how many"):flat.index("Finding a clip's onsets and tempo: an")], word
    assert re.search(r"#define\s+WBX_ALIGN_EITHER_POLARITY\s+1u", header) and W.ALIGN_EITHER_POLARITY == M.EITHER == 1
    assert L.wbx_align_max_lags() == 1 << 17 == M.MAX_LAGS and L.wbx_align_chunk_frames() == 2048 == M.CHUNK
    assert "align_samples" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()


def test_the_structs_have_the_headers_size_and_layout(tmp_path):
    info = [f for f in M.INFO_FIELDS]
    point = ["r", "energy"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * (len(info) + len(point) + 1)
                   + '\\n", sizeof(wbx_align_info), ' + ", ".join("offsetof(wbx_align_info, %s)" % f for f in info) + ", sizeof(wbx_align_point), "
                   + ", ".join("offsetof(wbx_align_point, %s)" % f for f in point) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    I, P = _ffi.AlignInfo, _ffi.AlignPoint
    assert got == [80, 0, 4, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 16, 0, 8]
    assert got == [C.sizeof(I)] + [getattr(I, f).offset for f in info] + [C.sizeof(P)] + [getattr(P, f).offset for f in point]
    assert [M.CURVE_DTYPE.fields[f][1] for f in point] == got[14:] and M.CURVE_DTYPE.itemsize == 16
    assert I.lag.size == 4 and I._fields_[0][1] is C.c_int32      # the lag is signed
    text = open(os.path.join(ROOT, "include", "wbx.h")).read()
    assert re.search(r"wbx_align_info\s*\{\s*/\* 80 bytes \*/", text) and re.search(r"wbx_align_point\s*\{\s*/\* 16 bytes \*/", text)


def test_adapter_with_align_compiles(tmp_path):
    """tests/cpp/adapter_align.cpp uses Engine::align_samples; it is compiled and linked here and run by
    tests/test_gpu_align.py (it needs a device)"""
    exe = str(tmp_path / "adapter_align")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_align.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    ai, ms = _ffi.AlignInfo(), C.c_double(5.0)
    ai.lag, ai.lags = -77, 123
    pts = np.zeros(17, dtype=M.CURVE_DTYPE)
    pts["r"] = 9.0
    assert L.wbx_clip_align(None, 0, 0, 64, 1, 0, 100, -8, 8, 0, C.byref(ai), pts.ctypes.data, 17) == -4
    assert L.wbx_engine_align_samples(None, 0, 0, 64, 1, 0, 100, -8, 8, 0, C.byref(ai), pts.ctypes.data, 17) == -4
    assert L.wbx_align_ms(None, C.byref(ms)) == -4 and ms.value == 5.0
    assert ai.lag == -77 and ai.lags == 123 and np.all(pts["r"] == 9.0) and np.all(pts["energy"] == 0.0)


# ---- wbx_align_check, the chunks, the bands -------------------------------------------------------------------------------------
TOP = 1 << 24
OK = dict(n=4096, m=10000, lo=-100, hi=100, flags=0, info=True, curve=False, cap=0)
# (change, status): one refusal each, the boundaries beside them, and the order where two apply
CHECKS = [(dict(), 0), (dict(n=0), -4), (dict(n=56), -4), (dict(n=64), 0), (dict(n=68), -4), (dict(n=72), 0), (dict(n=TOP), 0),
          (dict(n=TOP + 8), -4), (dict(n=1 << 63), -4),
          (dict(m=0), -4), (dict(m=1), 0), (dict(m=M.MAX_M - 1), 0), (dict(m=M.MAX_M), -4), (dict(m=1 << 40), -4),
          (dict(lo=-TOP, hi=-TOP), 0), (dict(lo=-TOP - 1, hi=-TOP), -4), (dict(lo=TOP, hi=TOP), 0), (dict(lo=TOP, hi=TOP + 1), -4),
          (dict(lo=TOP + 1, hi=TOP + 1), -4), (dict(lo=-(1 << 40)), -4), (dict(hi=1 << 40), -4),
          (dict(lo=5, hi=4), -4), (dict(lo=5, hi=5), 0), (dict(lo=0, hi=-1), -4),
          (dict(flags=1), 0), (dict(flags=2), -4), (dict(flags=3), -4), (dict(flags=1 << 31), -4),
          (dict(info=False), -4), (dict(info=False, curve=True, cap=201), 0), (dict(curve=True, cap=201), 0),
          (dict(curve=True, cap=200), -4), (dict(curve=True, cap=0), -4), (dict(curve=False, cap=0), 0),
          (dict(lo=0, hi=(1 << 17) - 1), 0), (dict(lo=0, hi=1 << 17), -3), (dict(lo=-(1 << 16), hi=1 << 16), -3),
          (dict(lo=-(1 << 16), hi=(1 << 16) - 1, curve=True, cap=1 << 17), 0),
          (dict(lo=0, hi=1 << 17, curve=True, cap=1 << 17), -4),             # the capacity is asked first
          (dict(lo=0, hi=1 << 17, curve=True, cap=(1 << 17) + 1), -3),
          (dict(lo=-TOP, hi=TOP), -3), (dict(lo=-TOP, hi=TOP, info=False), -4),
          # the order: n, m, lag_min, lag_max, their order, the flags, the outputs, the capacity, the number of lags
          (dict(n=68, m=0), -4), (dict(m=0, lo=-TOP - 1), -4), (dict(lo=TOP + 1, hi=0), -4), (dict(lo=5, hi=4, flags=2), -4),
          (dict(flags=2, info=False), -4), (dict(n=68, lo=0, hi=1 << 17), -4), (dict(m=0, lo=0, hi=1 << 17), -4),
          (dict(flags=2, lo=0, hi=1 << 17), -4), (dict(info=False, lo=0, hi=1 << 17), -4)]


def lib_check(a):
    return W.lib().wbx_align_check(a["n"], a["m"], a["lo"], a["hi"], a["flags"], int(a["info"]), int(a["curve"]), a["cap"])


def test_check_every_refusal_one_by_one():
    for change, want in CHECKS:
        a = dict(OK, **change)
        assert M.check(a["n"], a["m"], a["lo"], a["hi"], a["flags"], a["info"], a["curve"], a["cap"]) == want, change
        assert lib_check(a) == want, change
        assert W.align_check(a["n"], a["m"], a["lo"], a["hi"], a["flags"], a["info"], a["curve"], a["cap"]) == want
    assert {w for _, w in CHECKS} == {0, -4, -3}


def test_the_check_says_why_in_the_stated_order(tmp_path):
    """the reasons, read out of wbx_align.h in the order they are tested: n, m, lag_min, lag_max, their order, the flags, the
    outputs, the capacity — all INVALID — and only then the number of lags, UNSUPPORTED"""
    text = open(os.path.join(ROOT, "whitebox_amd", "csrc", "wbx_align.h")).read()
    body = text[text.index("inline wbx_status align_check("):text.index("// chunks one band takes")]
    why = re.findall(r'\*why = "clip align: ([^"]+)", (WBX_ERR_\w+)', body)
    assert [w for _, w in why] == ["WBX_ERR_INVALID"] * 8 + ["WBX_ERR_UNSUPPORTED"]
    keys = ["n_frames", "m_frames", "lag_min outside", "lag_max outside", "lag_min is above", "flag", "both NULL", "curve_cap", "2^17 lags"]
    assert all(k in msg for k, (msg, _) in zip(keys, why)), why


def test_chunks_bands_and_launches_equal_the_model_over_a_grid():
    L = W.lib()
    rng = np.random.default_rng(0xA11)
    ns = [0, 8, 56, 64, 72, 2040, 2048, 2056, 4096, 4100, 3 * 2048, 33 * 2048, TOP - 8, TOP, TOP + 8, 1 << 40, (1 << 64) - 1]
    ns += [int(v) * 8 for v in rng.integers(8, TOP // 8, 12)]
    for n in ns:
        assert L.wbx_align_chunks(n) == M.chunks(n) == W.align_chunks(n), n
        assert M.chunks(n) == (-(-n // 2048) if 64 <= n <= TOP and n % 8 == 0 else 0)
    lag_counts = [0, 1, 17, 511, 512, 513, 4096, 4097, 4101, 127100, 127101, (1 << 17) - 1, 1 << 17, (1 << 17) + 1, 1 << 40]
    lag_counts += [int(v) for v in rng.integers(1, 1 << 17, 12)]
    seen = set()
    for lags in lag_counts:
        per = L.wbx_align_band_chunks(lags)
        assert per == M.band_chunks(lags), lags
        if 1 <= lags <= 1 << 17:
            assert per >= 1 and per * lags <= 1 << 22 and per * lags * 2048 <= 1 << 39 and (per + 1) * lags > 1 << 22
        else:
            assert per == 0
        seen.add(per)
        for n in ns:
            want = M.launches(n, lags)
            assert L.wbx_align_launches(n, lags) == want, (n, lags)
            assert want == (2 * -(-M.chunks(n) // per) + 2 if per and M.chunks(n) else 0)
    assert len(seen) > 8
    assert M.launches(64, 17) == 4 and M.launches(TOP, 1 << 17) == 2 * 256 + 2


def test_the_band_seam_shape_has_two_bands():
    """tests/align_shapes.py: what tests/test_gpu_align.py runs across a band seam really has one"""
    import align_shapes
    L = W.lib()
    n, lags, per = align_shapes.band_seam_case()
    chunks = L.wbx_align_chunks(n)
    assert chunks == per + 1 and L.wbx_align_launches(n, lags) == 2 * 2 + 2 and W.align_check(n, n + lags, 0, lags - 1) == 0
    assert L.wbx_align_launches(n - 2048, lags) == 2 + 2 and L.wbx_align_launches(n, lags - 1) == 2 + 2     # the smallest
    assert (n, lags) == (33 * 2048, 127101)                        # with a stage of 2^22 partials


# ---- properties of the model --------------------------------------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("shift", [-37, 0, 53])
def test_a_moved_copy_is_found_exactly_with_confidence_one(shift):
    """B holds A's template `shift` frames later (or earlier): lag == shift, confidence within rounding of 1 — the two
    chains see the same products in the same order, so r == E == Ea bit for bit.  B is zero in front of its range, so a
    template found at a NEGATIVE lag loses its head there: the template starts with 64 silent frames, which lose nothing"""
    n, pad = 2048 + 64, 80
    x = noise(n + 2 * pad, 0xA0 + shift)
    x[pad:pad + 64] = 0.0
    a = x[pad:pad + n]
    info, curve = M.align_clips([a], 0, n, [x], 0, len(x), -64 - pad, 64 + pad)
    # x[pad + i] == a[i], so db[i + L] == da[i] at L = pad; move B's range instead of the data
    assert info["lag"] == pad and info["inverted"] == 0 and abs(info["confidence"] - 1.0) < 1e-15 and info["r"] == info["energy"] == info["ref_energy"]
    b_first = pad - shift                                          # B's range starts there: the template lies `shift` in
    info, _ = M.align_clips([a], 0, n, [x[b_first:]], 0, len(x) - b_first, -64, 64)
    assert info["lag"] == shift and info["inverted"] == 0 and abs(info["confidence"] - 1.0) <= 4 * np.finfo(np.float64).eps
    assert abs(info["offset"]) <= 0.5 and info["lags"] == 129 and info["chunks"] == 2 and info["terms"] == 129 * n


def test_an_inverted_copy_needs_either_polarity():
    n, pad = 1024, 40
    x = noise(n + 2 * pad, 0x1F)
    a = x[pad + 11:pad + 11 + n]
    info, curve = M.align_clips([a], 0, n, [-x], 0, len(x), -pad, 2 * pad, flags=M.EITHER)
    assert info["lag"] == pad + 11 and info["inverted"] == 1 and info["r"] < 0.0 and abs(info["confidence"] - 1.0) <= 1e-15
    plain, same_curve = M.align_clips([a], 0, n, [-x], 0, len(x), -pad, 2 * pad)
    assert np.array_equal(curve.view(np.uint64), same_curve.view(np.uint64))       # the flag changes the score alone
    assert plain["lag"] != pad + 11 and plain["confidence"] < 0.1 and plain["score"] >= 0.0
    assert abs(info["offset"]) <= 0.5 and abs(plain["offset"]) <= 0.5


def test_the_offset_stays_within_half_a_frame_and_silence_picks_lag_min():
    rng = np.random.default_rng(0x0FF)
    for trial in range(40):
        n = 64 + 8 * int(rng.integers(0, 20))
        a, b = noise(n, 1000 + trial), noise(n + 60, 2000 + trial)
        if trial % 4 == 0:
            b = np.round(b * 2).astype(np.float32)                 # ties and zeros
        info, _ = M.align_clips([a], 0, n, [b], 0, len(b), -20, 70, flags=trial & 1)
        assert abs(info["offset"]) <= 0.5 and -20 <= info["lag"] <= 70, trial
    z = np.zeros(256, dtype=np.float32)
    for a, b in ((z, noise(300, 5)), (noise(256, 6), np.zeros(300, dtype=np.float32))):
        info, _ = M.align_clips([a], 0, 256, [b], 0, 300, -9, 30)
        assert info["lag"] == -9 and info["score"] == 0.0 and info["confidence"] == 0.0 and info["offset"] == 0.0 and info["inverted"] == 0


def test_chosen_lags_equal_the_whole_curve_and_the_chunks_are_the_definition():
    x, y = noise(2048 + 72, 7), noise(2600, 8)
    _, full = M.align_clips([x], 0, len(x), [y], 0, len(y), -300, 500)
    some = [500, -300, 0, 17, -1]
    _, part = M.align_clips([x], 0, len(x), [y], 0, len(y), -300, 500, only=some)
    assert np.array_equal(part.view(np.uint64), np.ascontiguousarray(full[[s + 300 for s in some]]).view(np.uint64))
    # a flat ascending sum over the whole template differs from the two-level one in the last bits, and only there
    da, db = M.detector_of([x], 0, len(x)), M.detector_of([y], 0, len(y))
    flat = 0.0
    for i in range(len(x)):
        flat = flat + da[i] * db[i + 17]
    two = full["r"][317]
    assert abs(flat - two) <= 1e-12 * max(1.0, abs(two))
    stereo = M.detector_of([x, np.roll(x, 3)], 0, len(x))
    assert np.array_equal(stereo, (0.5 * (x.astype(np.float64) + np.roll(x, 3).astype(np.float64))).astype(np.float32).astype(np.float64))


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/align_main.cpp: wbx_align.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "align_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "align_main.cpp"), "-o", exe])
    lines, want = [], []
    ns = [0, 56, 64, 68, 2048, 2056, 33 * 2048, TOP, TOP + 8, (1 << 64) - 1]
    for n in ns:
        lines.append("k %d" % n)
        want.append("k %d" % M.chunks(n))
    for change, status in CHECKS:
        a = dict(OK, **change)
        lines.append("c %d %d %d %d %d %d %d %d" % (a["n"], a["m"], a["lo"], a["hi"], a["flags"], a["info"], a["curve"], a["cap"]))
        want.append("c %d" % status)
    shapes = set()
    for lags in (0, 1, 17, 512, 513, 606, 1024, 1025, 4095, 4096, 4097, 4101, 8192, 127101, 1 << 17, (1 << 17) + 1):
        lines.append("b %d" % lags)
        want.append("b %d" % M.band_chunks(lags))
        for n in ns:
            lines.append("n %d %d" % (n, lags))
            want.append("n %d" % M.launches(n, lags))
        if lags >= 1:
            waves, blocks = M.shape(lags)
            shapes.add(waves)
            lines.append("s %d" % lags)
            want.append("s %d %d %d" % (waves, blocks, 4 * (2048 + 16 + M.span_words(2048, waves))))
    assert shapes == {1, 2, 3, 8}
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "align ok" and len(got) == len(want) + 1
    for g, w, line in zip(got, want, lines):
        assert g == w, line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"0", "-4", "-3"}
