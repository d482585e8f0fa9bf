"""Reading a clip along a position curve, the part that needs no device: the symbols of include/wbx.h "Reading a clip along
a position curve" exist and match their binding twins, the structs have the header's layout, the adapter's method compiles,
NULL handles are refused, wbx_varispeed_plan / _table / _position / _check / _tiles equal the numpy twin
(tests/varispeed_model.py), every refusal of the argument check one by one with the order where two apply, the model holds
the conversion's SNR floors and equals tests/resample_model.py bit for bit where a curve is a conversion — and
wbx_varispeed.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_model as RM
import varispeed_model as M
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_varispeed_plan", "wbx_varispeed_table", "wbx_varispeed_position", "wbx_varispeed_check", "wbx_varispeed_tiles",
       "wbx_varispeed_max_knots", "wbx_varispeed_ms", "wbx_clip_varispeed", "wbx_engine_varispeed_sample"]
QUALITIES = {"fast": M.FAST, "good": M.GOOD, "best": M.BEST}
GUARDS = [(1, 1), (3, 2), (4, 1)]
ONE = 1 << 32


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    for f in ("varispeed_plan", "varispeed_table", "varispeed_position", "varispeed_check", "varispeed_tiles", "varispeed_knots"):
        assert callable(getattr(W, f)), f
    assert hasattr(W.MixContext, "clip_varispeed") and hasattr(W.MixContext, "varispeed_ms")
    for f in ("varispeed_sample", "tape_stop_sample", "vibrato_sample", "drift_sample", "pitch_curve_sample"):
        assert hasattr(W.Engine, f), f
    flat = re.sub(r"\s*\*\s*", " ", header)
    text = flat[flat.index("Reading a clip along a position curve"):flat.index("Stretching a clip: frames")]
    for word in ("NOT an identity", "in this order", "arithmetic", "never an fma", "0x7FC00000", "smaller knot_shift", "at render time",
                 "2^22", "bit for bit", "ZERO outside"):
        assert word in text, word
    assert "varispeed_sample" in open(os.path.join(ROOT, "include", "wbx_adapter.hpp")).read()
    make = open(os.path.join(ROOT, "whitebox_amd", "csrc", "Makefile")).read()
    assert make.count("wbx_varispeed.hip") == 1 and make.count("wbx_varispeed.h ") == 1 and re.search(r"for f in .*\bwbx_varispeed\b", make)
    assert L.wbx_varispeed_max_knots() == M.MAX_KNOTS == 1 << 22


def test_the_structs_have_the_headers_size_and_layout(tmp_path):
    info = ["half_width", "taps", "phases", "cutoff", "beta"]
    tile = ["first_out", "n_out", "lo_frame", "span"]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu' + " %zu" * (len(info) + len(tile) + 1)
                   + '\\n", sizeof(wbx_varispeed_info), ' + ", ".join("offsetof(wbx_varispeed_info, %s)" % f for f in info)
                   + ", sizeof(wbx_varispeed_tile), " + ", ".join("offsetof(wbx_varispeed_tile, %s)" % f for f in tile) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    I, T = _ffi.VarispeedInfo, _ffi.VarispeedTile
    assert got == [32, 0, 4, 8, 16, 24, 24, 0, 4, 8, 16]
    assert got == [C.sizeof(I)] + [getattr(I, f).offset for f in info] + [C.sizeof(T)] + [getattr(T, f).offset for f in tile]
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    assert re.search(r"wbx_varispeed_info\s*\{\s*/\* 32 bytes \*/", header) and re.search(r"wbx_varispeed_tile\s*\{\s*/\* 24 bytes \*/", header)


def test_adapter_with_varispeed_compiles(tmp_path):
    """tests/cpp/adapter_varispeed.cpp uses Engine::varispeed_sample; it is compiled and linked here and run by
    tests/test_gpu_varispeed.py (it needs a device)"""
    exe = str(tmp_path / "adapter_varispeed")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_varispeed.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    kn = M.constant_knots(16, 4, 1, 1)
    ms, new, st = C.c_double(5.0), C.c_uint32(77), _ffi.ClipStats()
    assert L.wbx_clip_varispeed(None, 0, 1, 0, 16, 16, kn.ctypes.data, 2, 4, 1, 1, 1, C.byref(st)) == -4
    assert L.wbx_engine_varispeed_sample(None, 0, 0, 16, 16, kn.ctypes.data, 2, 4, 1, 1, 1, C.byref(new), C.byref(st)) == -4
    assert L.wbx_varispeed_ms(None, C.byref(ms)) == -4 and ms.value == 5.0 and new.value == 77
    assert L.wbx_varispeed_plan(1, 1, 1, None) == -4
    pos, n = C.c_int64(9), C.c_uint64(9)
    assert L.wbx_varispeed_position(None, 2, 4, 0, C.byref(pos)) == -4 and L.wbx_varispeed_position(kn.ctypes.data, 2, 4, 0, None) == -4
    assert L.wbx_varispeed_tiles(kn.ctypes.data, 2, 4, 16, 16, 1, 1, 1, None, 0, None) == -4
    assert L.wbx_varispeed_tiles(kn.ctypes.data, 2, 4, 16, 16, 1, 1, 1, None, 1, C.byref(n)) == -4 and (pos.value, n.value) == (9, 9)


# ---- plan and tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", sorted(QUALITIES))
def test_plan_and_both_tables_equal_the_model_bit_for_bit(quality):
    q = QUALITIES[quality]
    for gn, gd in GUARDS:
        got, want = W.varispeed_plan(quality, gn, gd), M.plan(q, gn, gd)
        assert got == {k: want[k] for k in got}, (gn, gd, got, want)
        assert got["P"] == {"fast": 256, "good": 512, "best": 2048}[quality]
        r = RM.plan(gn, gd, q) if gn != gd else None               # the conversion gn -> gd has M / L = gn / gd
        assert r is None or (r["H"], r["T"], r["cutoff"], r["beta"]) == (got["H"], got["T"], got["cutoff"], got["beta"])
        (h, d), (mh, md) = W.varispeed_table(quality, gn, gd), M.tables(q, gn, gd)
        assert h.shape == (got["P"] + 1, got["T"]) and d.shape == (got["P"], got["T"])
        assert np.array_equal(bits32(h), bits32(mh)) and np.array_equal(bits32(d), bits32(md)), (gn, gd)
    assert W.varispeed_plan(quality, 6, 4) == W.varispeed_plan(quality, 3, 2)      # the gcd
    g1 = W.varispeed_plan(quality)
    assert g1["H"] == RM.QUALITY[q][0] and g1["cutoff"] == RM.QUALITY[q][2]        # guard 1: H = Z, cutoff = frac


@pytest.mark.parametrize("quality", sorted(QUALITIES))
def test_rows_0_and_half_are_the_conversion_1_to_2s_two_rows(quality):
    h, _ = W.varispeed_table(quality)
    t = RM.table(1, 2, QUALITIES[quality])
    P = h.shape[0] - 1
    assert np.array_equal(bits32(h[0]), bits32(t[0])) and np.array_equal(bits32(h[P // 2]), bits32(t[1]))
    got = np.zeros_like(t)
    assert W.lib().wbx_resample_table(1, 2, QUALITIES[quality], got.ctypes.data, got.size) == 0
    assert np.array_equal(bits32(got), bits32(t))                  # the shared row function left the conversion's table alone


def test_plan_and_table_refusals():
    L = W.lib()
    v = _ffi.VarispeedInfo()
    for q, gn, gd, want in ((3, 1, 1, -4), (-1, 1, 1, -4), (1, 0, 1, -4), (1, 1, 0, -4), (1, 1, 2, -4), (1, 999, 1000, -4),
                            (0, 22, 1, -3), (0, 21, 1, 0), (1, 11, 1, -3), (1, 32, 3, 0), (2, 16, 3, 0), (2, 17, 3, -3)):
        assert L.wbx_varispeed_plan(q, gn, gd, C.byref(v)) == want, (q, gn, gd)
        if want:
            with pytest.raises(M.Refused) as e:
                M.plan(q, gn, gd)
            assert e.value.status == want
    h = np.full(257 * 24, 7.0, dtype=np.float32)
    assert L.wbx_varispeed_table(0, 1, 1, h.ctypes.data, None, h.size - 1) == -4 and np.all(h == 7.0)
    assert L.wbx_varispeed_table(0, 1, 2, h.ctypes.data, None, h.size) == -4 and np.all(h == 7.0)
    assert L.wbx_varispeed_table(0, 1, 1, h.ctypes.data, None, h.size) == 0 and np.array_equal(bits32(h), bits32(M.tables(0)[0].ravel()))


# ---- positions ---------------------------------------------------------------------------------------------------------------
def curves():
    rng = np.random.default_rng(0x7A9E)
    down = np.array([1000 * ONE - 3 * i * ONE - 7 * i * i - i for i in range(9)], dtype=np.int64)     # descending, odd differences
    below = np.array([-(1 << 48) + i * 12345678901 for i in range(9)], dtype=np.int64)                  # from -2^16 frames up
    zig = (rng.integers(0, 600, 9) * ONE + rng.integers(0, ONE, 9)).astype(np.int64)
    return {"down": down, "below": below, "zig": zig}


@pytest.mark.parametrize("g", [4, 7, 10])
def test_positions_equal_the_model_and_pythons_floor(g):
    L = W.lib()
    for name, kn in curves().items():
        last = (len(kn) - 1) << g
        js = sorted(set([0, 1, (1 << g) - 1, 1 << g, (1 << g) + 1, last - 1, last] + list(range(3, last, max(1, last // 97)))))
        for j in js:
            got = W.varispeed_position(kn, g, j)
            i, r = j >> g, j & ((1 << g) - 1)
            want = int(kn[i]) + (((int(kn[min(i + 1, len(kn) - 1)]) - int(kn[i])) * r) >> g)
            assert got == want == M.position(kn, g, j), (name, j)
        assert np.array_equal(M.positions(kn, g, 0, last), np.array([M.position(kn, g, j) for j in range(last)], dtype=np.int64))
        pos = C.c_int64(5)
        for j in (last + 1, last + (1 << g), 1 << 40):             # past the curve
            assert L.wbx_varispeed_position(kn.ctypes.data, len(kn), g, j, C.byref(pos)) == -4 and pos.value == 5
        for bad in (3, 11):
            assert L.wbx_varispeed_position(kn.ctypes.data, len(kn), bad, 0, C.byref(pos)) == -4
    down = curves()["down"]
    d = int(down[1]) - int(down[0])
    assert d < 0 and d % (1 << g) and W.varispeed_position(down, g, 1) == int(down[0]) + (d >> g) < int(down[0]) + int(d / (1 << g))


# ---- tiles --------------------------------------------------------------------------------------------------------------------
def tile_cases():
    T = M.plan(M.GOOD)["T"]
    out = {}
    out["constant"] = (4, 5000, M.constant_knots(5000, 4, 3, 4))
    K = M.n_knots(3000, 6)
    out["zigzag"] = (6, 3000, np.array([(500 + (300 if i % 2 else -250) + i) * ONE + i * 999 for i in range(K)], dtype=np.int64))
    K = M.n_knots(4096, 8)
    slow = [i * 100 * ONE for i in range(K)]
    for i in range(5, K):                                           # interval 4 alone moves 4000 frames: a tile of its own
        slow[i] += 3900 * ONE
    out["one fast interval"] = (8, 4096, np.array(slow, dtype=np.int64))
    big = (M.SPAN_MAX - 2 - T + 1) * ONE - 1                        # the largest legal difference: (big >> 32) + 2 + T == 4096
    out["largest interval"] = (10, 2048, np.array([5, 5 + big, 5], dtype=np.int64))
    return out


@pytest.mark.parametrize("case", ["constant", "zigzag", "one fast interval", "largest interval"])
def test_tiles_equal_the_model(case):
    g, out_frames, kn = tile_cases()[case]
    n = 1 << 20
    assert M.check(kn, len(kn), g, n, out_frames, M.GOOD, 1, 1) == (0, "") and W.varispeed_check(kn, g, n, out_frames) == 0
    p = M.plan(M.GOOD)
    got, want = W.varispeed_tiles(kn, g, n, out_frames), M.tiles(kn, out_frames, g, p)
    assert got == want, (got[:4], want[:4])
    assert sum(t[1] for t in got) == out_frames and all(t[1] <= 1024 and t[3] <= 4096 and t[0] % 16 == 0 for t in got)
    for first, n_out, lo, span in got:                              # every tap of every position lies inside the staged span
        f = M.positions(kn, g, first, first + n_out) >> 32
        assert f.min() - (p["H"] - 1) >= lo and f.max() + p["H"] < lo + span
    if case == "constant":
        assert [t[1] for t in got] == [1024] * 4 + [5000 - 4096]
    if case == "one fast interval":
        assert (4 << g, 1 << g) in [(t[0], t[1]) for t in got]      # interval 4 stands alone
    if case == "largest interval":
        assert [t[3] for t in got] == [4095, 4095]
        worse = kn.copy()
        worse[1] += 1
        assert W.varispeed_check(worse, g, n, out_frames) == -3 and M.check(worse, 3, g, n, out_frames, M.GOOD, 1, 1) == (-3, "interval 0")
    rec, cnt = (_ffi.VarispeedTile * 2)(), C.c_uint64()
    assert W.lib().wbx_varispeed_tiles(kn.ctypes.data, len(kn), g, n, out_frames, 1, 1, 1, C.addressof(rec), 1, C.byref(cnt)) == 0
    assert cnt.value == len(want) and (rec[0].first_out, rec[0].n_out, rec[0].lo_frame, rec[0].span) == want[0] and rec[1].n_out == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
BASE = dict(n=1000, out=100, g=4, q=M.GOOD, gn=1, gd=1, knots="ok", nk=None)
TOP = (1 << 31) - 16
# one refusal each, in the header's order; further down, two at a time: the earlier one wins
REFUSALS = [
    (dict(n=0), -4, "frames"), (dict(out=0), -4, "frames"), (dict(n=TOP), -4, "frames"), (dict(out=TOP), -4, "frames"),
    (dict(g=3), -4, "knot_shift"), (dict(g=11), -4, "knot_shift"),
    (dict(knots=None), -4, "null"),
    (dict(nk=7), -4, "n_knots"), (dict(nk=9), -4, "n_knots"),
    (dict(q=3), -4, "quality"), (dict(q=-1), -4, "quality"),
    (dict(gn=0), -4, "guard"), (dict(gd=0), -4, "guard"), (dict(gn=2, gd=3), -4, "guard"),
    (dict(gn=11), -3, "taps"),
    (dict(knots="low"), -4, "bounds"), (dict(knots="high"), -4, "bounds"),
    (dict(knots="fast"), -3, "interval 2"),
]
ORDER = [
    (dict(n=0, g=3), "frames"), (dict(g=3, knots=None), "knot_shift"), (dict(knots=None, nk=7), "null"), (dict(nk=7, q=3), "n_knots"),
    (dict(q=3, gn=0), "quality"), (dict(gn=0, knots="low"), "guard"), (dict(gn=11, knots="low"), "taps"),
    (dict(knots="low+fast"), "bounds"),
]


def refusal_call(change):
    a = dict(BASE, **change)
    K = M.n_knots(max(a["out"], 1), min(max(a["g"], 4), 10)) if a["out"] < TOP else 8
    kn = np.arange(K, dtype=np.int64) * (ONE << 4)
    kind = a["knots"]
    if kind is None:
        kn = None
    else:
        if "low" in kind:
            kn[0] = -(M.MARGIN << 32) - 1
        if kind == "high":
            kn[-1] = ((a["n"] + M.MARGIN) << 32) + 1
        if "fast" in kind:
            kn[3:] += 4100 * ONE
    nk = a["nk"] if a["nk"] is not None else (0 if kn is None else len(kn))
    return a, kn, nk


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_every_refusal_one_by_one(i):
    change, status, reason = REFUSALS[i]
    a, kn, nk = refusal_call(change)
    assert M.check(kn, nk, a["g"], a["n"], a["out"], a["q"], a["gn"], a["gd"]) == (status, reason)
    got = W.lib().wbx_varispeed_check(None if kn is None else kn.ctypes.data, nk, a["g"], a["n"], a["out"], a["q"], a["gn"], a["gd"])
    assert got == status, change
    n = C.c_uint64(3)
    assert W.lib().wbx_varispeed_tiles(None if kn is None else kn.ctypes.data, nk, a["g"], a["n"], a["out"], a["q"], a["gn"], a["gd"],
                                       None, 0, C.byref(n)) == status and n.value == 3


def test_refusals_come_in_the_headers_order_and_the_edges_are_accepted():
    a, kn, nk = refusal_call({})
    assert M.check(kn, nk, 4, 1000, 100, M.GOOD, 1, 1) == (0, "") and W.varispeed_check(kn, 4, 1000, 100) == 0
    for change, reason in ORDER:
        a, kn, nk = refusal_call(change)
        status, why = M.check(kn, nk, a["g"], a["n"], a["out"], a["q"], a["gn"], a["gd"])
        assert why == reason, change
        assert W.lib().wbx_varispeed_check(None if kn is None else kn.ctypes.data, nk, a["g"], a["n"], a["out"], a["q"], a["gn"],
                                           a["gd"]) == status
    # the bounds themselves are legal: -2^16 and n + 2^16 frames, also where (n + 2^16) * 2^32 needs 64 bits
    for n in (1000, TOP - 1):
        edge = np.array([-(M.MARGIN << 32), -(M.MARGIN << 32)], dtype=np.int64)
        assert W.varispeed_check(edge, 4, n, 16) == 0 == M.check(edge, 2, 4, n, 16, M.GOOD, 1, 1)[0]
    top = np.array([(1000 + M.MARGIN) << 32] * 2, dtype=np.int64)
    assert W.varispeed_check(top, 4, 1000, 16) == 0 and W.varispeed_check(top + 1, 4, 1000, 16) == -4
    huge = np.array([np.iinfo(np.int64).max] * 2, dtype=np.int64)    # below (2^31 - 17 + 2^16) * 2^32, which 63 bits cannot hold
    assert W.varispeed_check(huge, 4, TOP - 1, 16) == 0 == M.check(huge, 2, 4, TOP - 1, 16, M.GOOD, 1, 1)[0]
    # K > 2^22 is refused as UNSUPPORTED, after the guard and before the knots are read
    out = (M.MAX_KNOTS << 4) + 1
    kn = np.zeros(M.n_knots(out, 4), dtype=np.int64)
    kn[0] = -(1 << 62)
    assert W.varispeed_check(kn, 4, 1000, out) == -3 and M.check(kn, len(kn), 4, 1000, out, M.GOOD, 1, 1) == (-3, "knots")
    assert W.varispeed_check(kn, 4, 1000, out, guard_num=0) == -4
    assert W.varispeed_check(kn[:M.MAX_KNOTS], 4, 1000, (M.MAX_KNOTS - 1) << 4) == -4   # K = 2^22 exactly: the knot is read and refused


# ---- what the form is worth -----------------------------------------------------------------------------------------------------
SPEED = 2.0 ** (-1.0 / 12.0)                                        # 0.94387...


def snr_db(quality, f, knots, g, out):
    n = 20200
    src = (0.5 * np.sin(2 * np.pi * f * np.arange(n))).astype(np.float32)
    y = M.varispeed([src], 0, n, out, knots, g, quality)[0].astype(np.float64)
    ref = 0.5 * np.sin(2 * np.pi * f * (M.positions(knots, g, 0, out).astype(np.float64) / 2.0 ** 32))
    return 10.0 * np.log10(np.sum(ref * ref) / np.sum((y - ref) ** 2))


@pytest.mark.parametrize("quality,floor", [("fast", 70.0), ("good", 96.0), ("best", 130.0)])
def test_the_model_holds_the_conversions_snr_floors(quality, floor):
    """0.5-amplitude sines of 20 000 frames at the constant speed 2^(-1/12) against the analytic sine at the model's own
    positions.  Measured on the CPU: FAST 76.9 / 78.5 dB at 997/48000 / 0.30 Rs, GOOD 104.6 / 103.1, BEST 149.5 / 146.4; the
    asserted floors are the conversion's (70 / 96 / 130 dB).  A +-40-frame vibrato at GOOD: 104.8 dB"""
    out, g = 20000, 6
    kn = np.array([int(round((100 + i * 64 * SPEED) * 2.0 ** 32)) for i in range(M.n_knots(out, g))], dtype=np.int64)
    assert M.check(kn, len(kn), g, 20200, out, QUALITIES[quality], 1, 1) == (0, "")
    for f in (997.0 / 48000.0, 0.30):
        got = snr_db(QUALITIES[quality], f, kn, g, out)
        print(quality, f, got)
        assert got >= floor, (quality, f, got)
    if quality == "good":
        j = np.arange(M.n_knots(out, 4)) * 16.0
        vib = np.array([int(round((100 + v + 40.0 * np.sin(2 * np.pi * v / 4000.0)) * 2.0 ** 32)) for v in j], dtype=np.int64)
        got = snr_db(M.GOOD, 997.0 / 48000.0, vib, 4, out)
        print("vibrato", got)
        assert got >= floor


@pytest.mark.parametrize("src,dst,guard", [(1, 2, (1, 1)), (1, 4, (1, 1)), (2, 1, (2, 1)), (3, 2, (3, 2))])
def test_the_model_is_the_conversions_model_where_the_curve_is_a_conversion(src, dst, guard):
    x = [np.random.default_rng(5 + c).standard_normal(2500).astype(np.float32) for c in range(2)]
    for q in QUALITIES.values():
        want = RM.resample(x, 0, 2500, src, dst, q)
        out = len(want[0])
        kn = M.constant_knots(out, 4, src, dst)
        assert M.check(kn, len(kn), 4, 2500, out, q, *guard) == (0, "")
        got = M.varispeed(x, 0, 2500, out, kn, 4, q, *guard)
        for a, b in zip(got, want):
            assert np.array_equal(bits32(a), bits32(b)), (src, dst, q)


def test_varispeed_knots_integrates_the_speed():
    kn, guard = W.varispeed_knots([(0, 1.0), (640, 1.0), (1280, 0.0)], 1280, 6)
    assert len(kn) == 21 and kn[0] == 0 and kn[10] == 640 * ONE and kn[20] == (640 + 320) * ONE and guard == (16, 16)
    assert np.all(np.diff(kn) >= 0) and W.varispeed_check(kn, 6, 2000, 1280) == 0
    kn, guard = W.varispeed_knots([(0, 1.5)], 100, 4, start=2.0)
    assert kn[1] == 26 * ONE and guard == (24, 16)


# ---- the header alone -----------------------------------------------------------------------------------------------------------
def fnv(words):
    h = 1469598103934665603
    for b in np.ascontiguousarray(words, dtype=np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_header_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/varispeed_main.cpp: wbx_varispeed.h alone, stand-alone (its own main): the plan, both tables and the device
    copy word by word, positions, the call's check and the tiles"""
    exe = str(tmp_path / "varispeed_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "varispeed_main.cpp"), "-o", exe])
    lines, want = [], []
    for q in (M.FAST, M.GOOD):
        for gn, gd in GUARDS:
            p, (h, d) = M.plan(q, gn, gd), M.tables(q, gn, gd)
            row = (2 * p["T"] + 15) // 16 * 16
            dev = np.zeros((p["P"], row), dtype=np.float32)
            dev[:, 0:2 * p["T"]:2], dev[:, 1:2 * p["T"]:2] = h[:-1], d
            lines.append("t %d %d %d" % (q, gn, gd))
            want.append("t 0 %d %d %d %016x %016x %016x" % (p["H"], p["T"], p["P"], fnv(h), fnv(d), fnv(dev)))
    for q, gn, gd, st in ((3, 1, 1, -4), (1, 0, 1, -4), (1, 1, 2, -4), (0, 22, 1, -3)):
        lines.append("t %d %d %d" % (q, gn, gd))
        want.append("t %d" % st)
    for name, kn in curves().items():
        for g in (4, 10):
            lines.append("k %d %d %s" % (g, len(kn), " ".join(str(int(v)) for v in kn)))
            want.append("k")
            for j in (0, 1, (1 << g) - 1, (1 << g) + 1, (len(kn) - 1 << g) - 1, len(kn) - 1 << g):
                lines.append("p %d" % j)
                want.append("p %d" % M.position(kn, g, j))
    for case, (g, out, kn) in tile_cases().items():
        lines.append("k %d %d %s" % (g, len(kn), " ".join(str(int(v)) for v in kn)))
        want.append("k")
        lines.append("l %d %d %d 1 1" % (1 << 20, out, M.GOOD))
        t = M.tiles(kn, out, g, M.plan(M.GOOD))
        want.append("l %d %s" % (len(t), " ".join("%d:%d:%d:%d" % r for r in t)))
    for change, status, _ in REFUSALS:
        a, kn, nk = refusal_call(change)
        base = np.zeros(nk, dtype=np.int64)                          # the program's curve has nk knots; a NULL curve is a flag
        if kn is not None:
            base[:min(nk, len(kn))] = kn[:min(nk, len(kn))]
        if a["g"] < 4 or a["g"] > 10:
            continue                                                 # (the program sets the shift with the curve: legal ones only)
        lines.append("k %d %d %s" % (a["g"], nk, " ".join(str(int(v)) for v in base)))
        want.append("k")
        lines.append("c %d %d %d %d %d %d" % (a["n"], a["out"], a["q"], a["gn"], a["gd"], kn is not None))
        want.append("c %d" % status)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.strip().split("\n")
    assert got[-1] == "varispeed ok" and len(got) == len(want) + 1
    for g_, w, line in zip(got, want, lines):
        assert g_ == w, line[:80]
    assert {w.split()[1] for w in want if w.startswith("c ")} == {"-4", "-3"}
