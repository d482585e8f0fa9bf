"""Dynamics of a clip, the part that needs no device: the symbols of include/wbx.h "Dynamics of a clip" exist and match their
binding twins, the adapter's method compiles, NULL handles are refused, wbx_dynamics_table and wbx_dynamics_lookup equal the
numpy twin (tests/dynamics_model.py) BIT FOR BIT and refuse what the header says they refuse, the designed table is
accurate against a long double rendering of the same curve and close to the ideal curve, the model itself has the
properties the header states — and wbx_dynamics.h runs stand-alone under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dynamics_model as M
import limit_model as LM
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_dynamics_table", "wbx_dynamics_check", "wbx_dynamics_lookup", "wbx_dynamics_ms", "wbx_clip_dynamics",
       "wbx_engine_dynamics_sample"]
THRESHOLDS, RATIOS, KNEES, RANGES = (-60.0, -18.0, -0.1, 0.0), (1.0, 1.5, 4.0, 100.0, np.inf), (0.0, 6.0, 24.0), (0.0, -12.0, -80.0, -np.inf)
GRID = [(kind, T, r, k, g) for kind in (M.COMPRESS, M.GATE) for T in THRESHOLDS for r in RATIOS for k in KNEES for g in RANGES]
LD = np.longdouble
CELL_DB = 20.0 * np.log10(1.0 + 1.0 / 64.0)                     # 0.1347 dB: the widest cell


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def lib_table(kind, T, ratio, knee, rng, cap=M.TABLE):
    buf = np.full(cap, 7.0, dtype=np.float64)
    return W.lib().wbx_dynamics_table(kind, T, ratio, knee, rng, buf.ctypes.data, buf.size), buf


def lib_lookup(tab, level):
    out = C.c_double(7.0)
    st = W.lib().wbx_dynamics_lookup(tab.ctypes.data, float(level), C.byref(out))
    return st, out.value


def refused_by_both(kind, T, r, k, g):
    return kind == M.GATE and not np.isfinite(r)                # the one kind of design of the grid that the header refuses


@pytest.fixture(scope="module")
def designs():
    """every design of the grid, made once by the library: {parameters: table, or None where it is refused}"""
    out = {}
    for p in GRID:
        st, buf = lib_table(*p)
        assert st == (-4 if refused_by_both(*p) else 0), p
        out[p] = buf if st == 0 else None
    return out


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n
    assert callable(W.dynamics_table) and callable(W.dynamics_check) and callable(W.dynamics_lookup)
    assert hasattr(W.MixContext, "clip_dynamics") and hasattr(W.MixContext, "dynamics_ms")
    for m in ("dynamics_sample", "compress_sample", "gate_sample", "duck_sample"):
        assert hasattr(W.Engine, m), m
    text = re.sub(r"\s*\*\s*", " ", header)
    assert "Dynamics of a clip" in text and "compressors, expanders and gates (their gain is computed in dB" not in text
    assert re.search(r"#define\s+WBX_DYN_TABLE\s+3073\b", header) and M.TABLE == 3073 == _ffi.DYN_TABLE
    assert re.search(r"WBX_DYN_COMPRESS = 0, WBX_DYN_GATE = 1", header) and _ffi.DYN_SENSE == {"compress": M.COMPRESS, "gate": M.GATE}
    assert re.search(r"#define\s+WBX_DYN_NO_KEY\s+0xFFFFFFFFu", header) and _ffi.DYN_NO_KEY == 0xFFFFFFFF


def test_the_struct_has_the_headers_size_and_layout(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(wbx_dynamics_stats), offsetof(wbx_dynamics_stats, min_gain), offsetof(wbx_dynamics_stats, min_gain_frame), '
                   'offsetof(wbx_dynamics_stats, reduced_frames)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = _ffi.DynamicsStats
    assert got == [24, 0, 8, 16] == [C.sizeof(S), S.min_gain.offset, S.min_gain_frame.offset, S.reduced_frames.offset]


def test_adapter_with_dynamics_compiles(tmp_path):
    """tests/cpp/adapter_dynamics.cpp uses Engine::dynamics_sample; it is compiled and linked here and run by
    tests/test_gpu_dynamics.py (it needs a device)"""
    exe = str(tmp_path / "adapter_dynamics")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "adapter_dynamics.cpp"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx",
                           "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    tab = np.ones(M.TABLE)
    new, ds, st, ms = C.c_uint32(77), _ffi.DynamicsStats(), _ffi.ClipStats(), C.c_double(5.0)
    assert L.wbx_clip_dynamics(None, 0, _ffi.DYN_NO_KEY, 1, 0, 64, 0, 0, tab.ctypes.data, 1.0, 1.0, 1.0, 8, 0, 48, C.byref(ds), C.byref(st)) == -4
    assert L.wbx_engine_dynamics_sample(None, 0, _ffi.DYN_NO_KEY, 0, 64, 0, 0, tab.ctypes.data, 1.0, 1.0, 1.0, 8, 0, 48, C.byref(new),
                                        C.byref(ds), C.byref(st)) == -4 and new.value == 77
    assert L.wbx_dynamics_ms(None, C.byref(ms)) == -4 and ms.value == 5.0


# ---- wbx_dynamics_table -----------------------------------------------------------------------------------------------------
def test_tables_equal_the_model_bit_for_bit(designs):
    made = 0
    for p, got in designs.items():
        if got is None:
            with pytest.raises(M.Refused):
                M.table(*p)
            continue
        want = M.table(*p)
        assert same_bits64(got, want), (p, np.flatnonzero(got != want)[:4])
        lo = M.table_check(got, p[0])                           # every design passes the check, in either sense
        assert W.dynamics_check(got, "compress") == lo == W.dynamics_check(got, "gate") == got.min()
        kind, T, r, k, g = p
        L_db = M.entry_octaves() * float(M.DB_PER_OCTAVE)
        idle = L_db <= T - k / 2 if kind == M.COMPRESS else L_db >= T + k / 2
        assert np.all(got[idle] == 1.0) and np.all(np.diff(got) <= 0.0 if kind == M.COMPRESS else np.diff(got) >= 0.0), p
        if np.isfinite(g):                                      # never below the range (one rounding of 10 ** (g / 20) allowed)
            assert lo >= 10.0 ** (g / 20.0) * (1.0 - 1e-12), p
        made += 1
    assert made == len(GRID) - 4 * 3 * 4
    assert same_bits64(W.dynamics_table("gate", -40.0, 10.0, 0.0, -80.0), M.table(M.GATE, -40.0, 10.0, 0.0, -80.0))
    t = M.table(M.GATE, 0.0, 100.0, 0.0, -np.inf)               # -inf: no floor, and what falls under 2^-1021 is 0.0
    assert t[0] == 0.0 and np.all(t[t > 0.0] >= 2.0 ** -1021.5) and np.any(t == 0.0) and t[-1] == 1.0


def ideal_db(kind, T, ratio, knee, rng, L):
    """the static curve's gain in dB at the levels L (dB), in long double with libm: the reference, not the code under test"""
    L, T, W_, one = LD(1) * L, LD(T), LD(knee), LD(1)
    s = (one / LD(ratio) - one) if kind == M.COMPRESS else LD(ratio) - one
    over = L - T
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == M.COMPRESS:
            G = np.where(2 * over <= -W_, 0, np.where(2 * over < W_, s * (over + W_ / 2) ** 2 / (2 * W_), s * over))
        else:
            G = np.where(2 * over >= W_, 0, np.where(2 * over > -W_, -s * (over - W_ / 2) ** 2 / (2 * W_), s * over))
    return np.maximum(G.astype(LD), LD(rng))


def test_designed_entries_are_accurate_to_2_to_the_minus_40(designs):
    """Against numpy long double + libm.  Bound: 2^-40 relative per entry, entries of 0.0 and 1.0 exact (the issue's bound:
    the gain is exp2(y), y good to a few units in its last place, |y| up to 1021 octaves before the entry is flushed to 0.0,
    so the error is near 1021 * ln 2 * a few * 2^-53 = 2^-42; at |y| <= 48 octaves of a 2:1 curve it is near 2^-46).
    Measured worst case (printed below, and in DESIGN.md 7k): 1.63e-13 = 2^-42.5 at the 100:1 expander with no floor, whose
    entries reach 2^-1021 — a level's rounding (2^-48 near 40 octaves) times the slope of 99; 1.69e-14 = 2^-45.8 at slopes
    of at most 3 dB per dB."""
    if np.finfo(LD).nmant < 60:
        pytest.skip("long double is no wider than double on this host: no reference")
    e, k = M.entry_levels()
    L = (e.astype(LD) + np.log2(LD(1) + k.astype(LD) / LD(64))) * (LD(20) * np.log10(LD(2)))
    worst, worst_small, at = 0.0, 0.0, None
    for p, got in designs.items():
        if got is None:
            continue
        G = ideal_db(*p, L)
        want = np.power(LD(10), G / LD(20))
        exact = (G == 0)
        assert np.all(got[exact] == 1.0), p
        flushed = G < LD(-1021.0) * LD(20) * np.log10(LD(2)) * (1 - LD(1e-12))
        near_flush = ~flushed & (G < LD(-1021.0) * LD(20) * np.log10(LD(2)) * (1 + LD(1e-12)))
        assert np.all(got[flushed] == 0.0), p
        live = ~exact & ~flushed & ~near_flush
        rel = np.abs((got[live].astype(LD) - want[live]) / want[live]).astype(np.float64)
        if rel.size:
            if rel.max() > worst:
                worst, at = float(rel.max()), p
            if p[2] <= 4.0 or p[0] == M.COMPRESS:               # |slope| <= 3: the level's own rounding is not multiplied by 99
                worst_small = max(worst_small, float(rel.max()))
    print("design accuracy: worst relative error %.3g = 2^%.2f at %s; for slopes of at most 3 dB per dB %.3g = 2^%.2f" % (
        worst, np.log2(worst), at, worst_small, np.log2(worst_small)))
    assert worst <= 2.0 ** -40


def power_law_interpolation_db(s):
    """the largest error in dB of interpolating p^s linearly in p across one cell [1, 1 + 1/64] (long double): what a table
    of this grid costs where the ideal curve is a straight line of slope s in dB per dB"""
    u = np.linspace(LD(0), LD(1), 129)
    r = LD(1) + LD(1) / LD(64)
    lin = (1 - u) + u * r ** LD(s)
    return float(np.max(np.abs(LD(20) * np.log10(lin / (1 - u + u * r) ** LD(s)))))


def test_the_table_follows_the_ideal_curve(designs):
    """The lookup at three points inside every cell against the ideal curve, in dB.  Derived bound, for a curve whose slope
    (dB of gain per dB of level) changes by at most D at a corner: D * cell / 4 for a corner inside a cell (a hard knee, the
    range's floor) — the chord of a corner; cell^2 / 8 * |slope| / knee for the knee's curvature; and the error of
    interpolating a power law linearly in the level (power_law_interpolation_db), taken at the curve's steepest slope.
    Points whose ideal gain lies under 2^-1000 are left out: there the table is flushed to 0.0.  Measured, for the issue's
    figures: printed below and written into DESIGN.md 7k"""
    e, k = M.entry_levels()
    inside = []
    for u in (0.25, 0.5, 0.75):
        inside.append((2.0 ** e[:-1].astype(np.float64)) * (1.0 + (k[:-1] + u) / 64.0))
    p = np.concatenate(inside)
    L = LD(20) * np.log10(p.astype(LD))
    report = {}
    for d, tab in designs.items():
        if tab is None:
            continue
        kind, T, r, knee, rng = d
        s = float((1.0 / r - 1.0) if kind == M.COMPRESS else r - 1.0)
        G = ideal_db(*d, L)
        live = G > -6000.0
        got = M.lookup(tab, p)[live]
        assert np.all(got > 0.0), d
        err = float(np.max(np.abs(LD(20) * np.log10(got.astype(LD)) - G[live]))) if np.any(live) else 0.0
        corner = abs(s) * CELL_DB / 4.0
        bound = (corner if knee == 0.0 else CELL_DB ** 2 / 8.0 * abs(s) / knee) + (corner if np.isfinite(rng) else 0.0) \
            + max(power_law_interpolation_db(s * f) for f in (0.25, 0.5, 0.75, 1.0))
        assert err <= bound * 1.001 + 1e-9, (d, err, bound)
        report[d] = err
    hard = report[(M.COMPRESS, -18.0, np.inf, 0.0, -np.inf)]
    soft4, softinf = report[(M.COMPRESS, -18.0, 4.0, 6.0, -np.inf)], report[(M.COMPRESS, -18.0, np.inf, 6.0, -np.inf)]
    print("table against the ideal curve: inf:1 hard knee %.4f dB (bound %.4f), 6 dB knee 4:1 %.2e dB, inf:1 %.2e dB" % (
        hard, CELL_DB / 4.0 + power_law_interpolation_db(-1.0), soft4, softinf))
    assert hard <= 0.0337 + 6e-4


def test_table_refusals_write_nothing():
    ok = dict(kind=M.COMPRESS, T=-18.0, ratio=4.0, knee=6.0, rng=-40.0)
    st, buf = lib_table(**ok, cap=M.TABLE + 5)
    assert st == 0 and np.all(buf[M.TABLE:] == 7.0) and not np.any(buf[:M.TABLE] == 7.0)
    for change in (dict(cap=M.TABLE - 1), dict(cap=0), dict(kind=2), dict(kind=-1), dict(T=np.nan), dict(T=np.inf), dict(T=1000.5),
                   dict(ratio=0.99), dict(ratio=np.nan), dict(ratio=-np.inf), dict(kind=M.GATE, ratio=np.inf), dict(knee=-1.0),
                   dict(knee=np.nan), dict(knee=1001.0), dict(rng=0.5), dict(rng=np.nan), dict(rng=np.inf)):
        st, buf = lib_table(**dict(ok, **change))
        assert st == -4 and np.all(buf == 7.0), change
        if "cap" not in change:
            with pytest.raises(M.Refused):
                M.table(*[dict(ok, **change)[q] for q in ("kind", "T", "ratio", "knee", "rng")])
    assert W.lib().wbx_dynamics_table(0, -18.0, 4.0, 6.0, -40.0, None, M.TABLE) == -4
    with pytest.raises(W.WbxError):
        W.dynamics_table("gate", -40.0, np.inf)
    assert lib_table(M.COMPRESS, 0.0, np.inf, 0.0, -0.0)[0] == 0   # a range of -0.0 dB is a range of 0 dB


def test_check_refusals():
    L = W.lib()
    good = M.table(M.COMPRESS, -18.0, 4.0, 6.0, -40.0)
    lo = C.c_double(7.0)
    assert L.wbx_dynamics_check(good.ctypes.data, 0, C.byref(lo)) == 0 and lo.value == good.min()
    assert L.wbx_dynamics_check(good.ctypes.data, 1, None) == 0
    for sense in (2, -1):
        assert L.wbx_dynamics_check(good.ctypes.data, sense, None) == -4
    assert L.wbx_dynamics_check(None, 0, None) == -4
    for at in (0, 1, 1500, M.TABLE - 1):
        for v in (np.nan, -np.nan, np.inf, -np.inf, -0.0, -1e-300, 1.0 + 2.0 ** -52, 2.0, -0.5):
            bad = good.copy()
            bad[at] = v
            lo.value = 7.0
            assert L.wbx_dynamics_check(bad.ctypes.data, 0, C.byref(lo)) == -4 and lo.value == 7.0, (at, v)
            with pytest.raises(M.Refused):
                M.table_check(bad)
            with pytest.raises(W.WbxError):
                W.dynamics_check(bad)
    for v in (0.0, 5e-324, 1.0):                                # the limits themselves
        ok = good.copy()
        ok[7] = v
        assert W.dynamics_check(ok) == min(v, good.min())


# ---- wbx_dynamics_lookup ----------------------------------------------------------------------------------------------------
def edge_levels():
    """the levels the issue lists: 0, the smallest subnormal float times a drive, just below and exactly 2^-40, every cell
    boundary of one octave, the top of a cell (low 46 mantissa bits all ones), exactly 2^8, 3e38 * 2^32"""
    sub = float(np.float32(1e-45))
    top = np.array([(1023 - 3) << 52 | (17 << 46) | ((1 << 46) - 1), (1023 + 7) << 52 | ((1 << 52) - 1), (1023 - 40) << 52 | ((1 << 46) - 1)],
                   dtype=np.uint64).view(np.float64)
    return np.concatenate([[0.0, sub, sub * 3.0, sub * 2.0 ** 32, np.nextafter(2.0 ** -40, 0.0), 2.0 ** -40, np.nextafter(2.0 ** -40, 1.0)],
                           0.25 * (1.0 + np.arange(65) / 64.0), top, [np.nextafter(256.0, 0.0), 256.0, np.nextafter(256.0, 1e9),
                                                                     float(np.float32(3e38)) * 2.0 ** 32, 1.0, 0.1234]])


def test_lookups_equal_the_model_bit_for_bit_at_every_edge():
    rng = np.random.default_rng(0x0D1A)
    tables = [M.table(M.COMPRESS, -18.0, 4.0, 6.0, -40.0), M.table(M.GATE, -40.0, 10.0, 0.0, -80.0), rng.uniform(0.0, 1.0, M.TABLE)]
    levels = edge_levels()
    for tab in tables:
        want = M.lookup(tab, levels)
        for p, w in zip(levels, want):
            st, got = lib_lookup(tab, p)
            assert st == 0 and np.float64(got).view(np.uint64) == np.float64(w).view(np.uint64), (p, got, w)
        assert lib_lookup(tab, 0.0)[1] == tab[0] == lib_lookup(tab, np.nextafter(2.0 ** -40, 0.0))[1]
        assert lib_lookup(tab, 2.0 ** -40)[1] == tab[0] and lib_lookup(tab, 256.0)[1] == tab[-1] == lib_lookup(tab, 1e48)[1]
        for c in range(65):                                     # a cell boundary returns its entry
            assert lib_lookup(tab, 0.25 * (1.0 + c / 64.0))[1] == tab[(40 - 2) * 64 + c]
        assert W.dynamics_lookup(tab, 0.1234) == want[-1]
    assert lib_lookup(tables[0], -1.0) == (-4, 7.0) and lib_lookup(tables[0], np.nan) == (-4, 7.0)
    assert W.lib().wbx_dynamics_lookup(None, 1.0, C.byref(C.c_double())) == -4
    assert W.lib().wbx_dynamics_lookup(tables[0].ctypes.data, 1.0, None) == -4


def test_a_lookup_stays_between_its_two_entries_on_random_tables():
    """containment: want lies in [min, max] of tab[idx], tab[idx + 1], mantissas at the top of their cell included"""
    rng = np.random.default_rng(0xC0A7)
    for trial in range(40):
        tab = rng.uniform(0.0, 1.0, M.TABLE) if trial % 2 else np.sort(rng.uniform(0.0, 1.0, M.TABLE) ** 8)
        if trial % 5 == 0:
            tab[rng.integers(0, M.TABLE, 300)] = rng.choice([0.0, 1.0, 5e-324, 2.0 ** -1022], 300)
        e = rng.integers(1023 - 40, 1023 + 8, 4000).astype(np.uint64)
        cell = rng.integers(0, 64, 4000).astype(np.uint64)
        low = rng.integers(0, 1 << 46, 4000).astype(np.uint64)
        low[::3] = np.uint64((1 << 46) - 1) - rng.integers(0, 3, low[::3].size).astype(np.uint64)   # the top of the cell
        low[1::7] = rng.integers(0, 3, low[1::7].size).astype(np.uint64)
        p = (e << np.uint64(52) | cell << np.uint64(46) | low).view(np.float64)
        idx = (e.astype(np.int64) - (1023 - 40)) * 64 + cell.astype(np.int64)
        want = M.lookup(tab, p)
        a, b = np.minimum(tab[idx], tab[idx + 1]), np.maximum(tab[idx], tab[idx + 1])
        assert np.all(want >= a) and np.all(want <= b) and np.all(want >= tab.min()) and np.all(want <= 1.0)
        for q in range(0, 4000, 401):
            assert lib_lookup(tab, p[q])[1] == want[q]


# ---- the argument check -----------------------------------------------------------------------------------------------------
def test_check_args_of_the_model():
    tab = M.table(M.COMPRESS, -18.0, 4.0, 6.0, -40.0)
    ok = dict(n=1000, tab=tab, sense=M.COMPRESS, drive=1.0, key_gain=1.0, makeup=1.0, A=72, H=0, R=4800, keyed=True)
    assert M.check_args(**ok) == 0
    bad = tab.copy()
    bad[9] = 1.5
    for change, want in ((dict(n=0), -4), (dict(tab=None), -4), (dict(tab=bad), -4), (dict(sense=2), -4), (dict(drive=0.0), -4),
                         (dict(drive=np.nan), -4), (dict(drive=2.0 ** 33), -4), (dict(key_gain=0.0), -4), (dict(key_gain=np.inf), -4),
                         (dict(key_gain=0.0, keyed=False), 0), (dict(makeup=-1.0), -4), (dict(makeup=np.inf), -4), (dict(makeup=0.0), 0),
                         (dict(A=4097), -4), (dict(H=65537), -4), (dict(R=0), -4), (dict(n=LM.MAX_FRAMES), -4),
                         (dict(n=1 << 30, R=1 << 20), -3), (dict(n=1 << 24, A=0, R=1 << 20), 0), (dict(n=(1 << 24) + 1, A=0, R=1 << 20), -3)):
        assert M.check_args(**dict(ok, **change)) == want, change


# ---- the model's own properties ---------------------------------------------------------------------------------------------
def random_case(rng):
    ch, n = int(rng.integers(1, 3)), int(rng.integers(1, 700))
    planes = [(rng.standard_normal(n) * rng.choice([0.001, 0.05, 0.5, 2.0])).astype(np.float32) for _ in range(ch)]
    for p in planes:
        for _ in range(int(rng.integers(0, 4))):
            p[rng.integers(0, n)] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30, 3.0, -4.0, 0.0])
    return planes, float(rng.choice([1.0, -1.0, 0.25, 3.0])), int(rng.integers(0, 70)), int(rng.integers(0, 50)), int(rng.integers(1, 300))


def test_a_table_of_ones_returns_the_driven_input_times_the_makeup():
    rng = np.random.default_rng(0x0E5)
    ones = np.ones(M.TABLE)
    for sense in (M.COMPRESS, M.GATE):
        for _ in range(20):
            planes, drive, A, H, R = random_case(rng)
            makeup = float(rng.choice([1.0, 0.5, 1.7, 0.0]))
            out, stats = M.dynamics_clip(planes, 0, len(planes[0]), ones, sense, drive, makeup, A, H, R)
            for o, d in zip(out, LM.driven(planes, drive)):
                assert np.array_equal(o.view(np.uint32), ((d * 1.0) * np.float64(makeup)).astype(np.float32).view(np.uint32))
            assert stats == {"min_gain": 1.0, "min_gain_frame": 0, "reduced_frames": 0}


def test_the_gain_lies_between_the_smallest_entry_and_one():
    """g <= 1.0 exactly.  From below the header promises lo only up to the rounding of the window's sum: A + 1 additions
    and one division, each within 2^-53 relative — g >= lo * (1 - (A + 2) * 2^-53).  (The issue asks for g in [lo, 1]; the
    sum of A + 1 copies of lo, divided by A + 1, need not return lo: measured below.)"""
    rng = np.random.default_rng(0x6A19)
    tables = [(M.table(M.COMPRESS, -30.0, 4.0, 6.0, -24.0), M.COMPRESS), (M.table(M.GATE, -30.0, 3.0, 6.0, -50.0), M.GATE),
              (rng.uniform(0.0, 1.0, M.TABLE), M.COMPRESS), (rng.uniform(0.0, 1.0, M.TABLE), M.GATE)]
    below = 0
    for i in range(120):
        tab, sense = tables[i % 4]
        planes, drive, A, H, R = random_case(rng)
        d, p, want, y, g = M.gains(planes, tab, sense, drive, A, H, R)
        lo = tab.min()
        assert np.all(want >= lo) and np.all(want <= 1.0) and np.all(y >= lo) and np.all(y <= 1.0) and y.size == len(p) + A
        assert np.all(g <= 1.0) and np.all(g >= lo * (1.0 - (A + 2) * 2.0 ** -53))
        below += int(np.count_nonzero(g < lo))
    print("frames whose gain rounded below the smallest entry:", below)


def test_an_isolated_bursts_gate_opens_early_holds_and_closes():
    """a burst of 0.5 on frames 300 .. 309 in silence; a table that is lo = 0.125 under 2^-4 and 1.0 from 2^-3 on; A = 4,
    H = 5, R = 40: the curve is lo, jumps to 1.0 A frames before the burst, stays through the burst and the hold, then
    falls by 1 / R per frame until it reaches lo after (1 - lo) * R frames"""
    lo, A, H, R = 0.125, 4, 5, 40
    e, k = M.entry_levels()
    tab = np.where(e >= -3, 1.0, lo)
    tab[(e == -4)] = lo + (1.0 - lo) * k[e == -4] / 64.0
    x = np.zeros(600, dtype=np.float32)
    x[300:310] = 0.5
    d, p, want, y, g = M.gains([x], tab, M.GATE, 1.0, A, H, R)
    j = lambda f: f + A                                         # curve frame f lives at y[f + A]
    assert np.all(y[:j(300 - A)] == lo) and np.all(y[j(300 - A):j(309 + H) + 1] == 1.0)
    fall = y[j(309 + H):j(309 + H) + 36]
    assert np.all(np.abs(np.diff(fall) + 1.0 / R) < 1e-15) and np.all(y[j(309 + H + 35) + 1:] == lo)
    # the gain is the average of the curve frames i - A .. i: it rises over the A frames in front of the burst, is 1.0 from
    # the burst's first frame to the hold's end, and is back at lo A frames after the curve
    assert np.all(g[:300 - A] == lo) and np.all(np.diff(g[300 - A - 1:301]) > 0.0)
    assert np.all(g[300:310 + H] == 1.0) and np.all(np.diff(g[309 + H:309 + H + 36 + A]) < 0.0) and np.all(g[309 + H + 36 + A:] == lo)
    out, stats = M.dynamics_clip([x], 0, 600, tab, M.GATE, 1.0, 1.0, A, H, R)
    assert np.array_equal(out[0], x) and stats["min_gain"] == lo and stats["min_gain_frame"] == 0


def test_the_compress_sense_with_a_limiting_table_tracks_the_limiter():
    """tab = min(1, c / level) at the grid levels: the curve is the limiter's with want in place of need, to within the
    table's interpolation.  Above c, c / p is convex in p, so a cell's chord lies above it by at most
    (1/8) (1/64)^2 * 2 = 6.2e-5 relative; in the one cell that holds c the chord cuts the corner and lies below by at most
    the cell's drop, 1 - 1 / (1 + 1/64) < 1/64 (nothing, where c is a grid level: 0.5).  Adding the ramp and taking minima
    keeps both relative bounds; with A = 0 the gain IS the curve in both models"""
    rng = np.random.default_rng(0x11A1)
    e, k = M.entry_levels()
    levels = 2.0 ** e.astype(np.float64) * (1.0 + k / 64.0)
    for c, under in ((np.float32(0.5), 1e-15), (np.float32(0.891251), 1.0 / 64.0)):
        tab = np.minimum(1.0, np.float64(c) / levels)
        for i in range(16):
            planes, drive, A, H, R = random_case(rng)
            for q in planes:                                    # (above 2^8, the table's last level, the table is flat)
                q[np.abs(q) > 60.0] = 3.0
            A = 0 if i % 2 else A
            d, p, want, y, g = M.gains(planes, tab, M.COMPRESS, drive, A, H, R)
            _, _, need, ly, lg = LM.gains(planes, c, drive, A, H, R)
            assert np.all(want >= need * (1.0 - under)) and np.all(want <= need * (1.0 + 6.2e-5))
            assert np.all(y >= ly * (1.0 - under)) and np.all(y <= ly * (1.0 + 6.2e-5))
            if A == 0:
                assert np.array_equal(g, y) and np.array_equal(lg, ly)


# ---- the host code under a sanitizer ----------------------------------------------------------------------------------------
def fnv(values):
    h = 1469598103934665603
    for b in np.ascontiguousarray(values, dtype=np.float64).view(np.uint8).tolist():
        h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_table_lookup_and_check_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/dynamics_main.cpp: wbx_dynamics.h alone, stand-alone (its own main)"""
    exe = str(tmp_path / "dynamics_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "dynamics_main.cpp"), "-o", exe])
    hexd = lambda v: "%016x" % np.float64(v).view(np.uint64)
    lines, want = [], []

    def design(kind, T, r, k, g, cap=M.TABLE):
        lines.append("t %d %s %s %s %s %d" % (kind, hexd(T), hexd(r), hexd(k), hexd(g), cap))

    for p in ((M.COMPRESS, -18.0, 4.0, 6.0, -40.0), (M.COMPRESS, 0.0, np.inf, 0.0, -np.inf), (M.GATE, -60.0, 100.0, 24.0, -80.0),
              (M.GATE, 0.0, 100.0, 0.0, -np.inf), (M.COMPRESS, -0.1, 1.0, 0.0, 0.0)):
        t = M.table(*p)
        design(*p)
        want.append("t 0 %016x %s %s" % (fnv(t), hexd(t[0]), hexd(t[-1])))
    design(M.COMPRESS, -18.0, 4.0, 6.0, -40.0, cap=M.TABLE + 3)
    t = np.concatenate([M.table(M.COMPRESS, -18.0, 4.0, 6.0, -40.0), np.full(3, 7.0)])
    want.append("t 0 %016x %s %s" % (fnv(t), hexd(t[0]), hexd(7.0)))
    for p, cap in (((M.COMPRESS, -18.0, 4.0, 6.0, -40.0), M.TABLE - 1), ((2, -18.0, 4.0, 6.0, -40.0), M.TABLE), ((M.GATE, -18.0, np.inf, 6.0, -40.0), M.TABLE),
                   ((M.COMPRESS, np.nan, 4.0, 6.0, -40.0), M.TABLE), ((M.COMPRESS, -18.0, 0.5, 6.0, -40.0), M.TABLE), ((M.COMPRESS, -18.0, 4.0, -6.0, -40.0), M.TABLE),
                   ((M.COMPRESS, -18.0, 4.0, 6.0, 1.0), M.TABLE)):
        design(*p, cap=cap)
        want.append("t -4 %016x %s %s" % (fnv(np.full(cap, 7.0)), hexd(7.0), hexd(7.0)))
    cur = M.table(M.GATE, -40.0, 10.0, 6.0, -80.0)
    design(M.GATE, -40.0, 10.0, 6.0, -80.0)
    want.append("t 0 %016x %s %s" % (fnv(cur), hexd(cur[0]), hexd(cur[-1])))
    for sense in (0, 1, 2):
        lines.append("k %d" % sense)
        want.append("k %d %s" % ((0, hexd(cur.min())) if sense < 2 else (-4, hexd(7.0))))
    for p, w in zip(edge_levels(), M.lookup(cur, edge_levels())):
        lines.append("l %s" % hexd(p))
        want.append("l %s" % hexd(w))
    checks = [(1000, 0, 1.0, 1.0, 1.0, 72, 0, 4800, 1, 1), (0, 0, 1.0, 1.0, 1.0, 72, 0, 4800, 1, 1), (1000, 2, 1.0, 1.0, 1.0, 0, 0, 1, 0, 1),
              (1000, 1, 1.0, 1.0, 1.0, 0, 0, 1, 0, 0), (1000, 1, 0.0, 1.0, 1.0, 0, 0, 1, 0, 1), (1000, 1, -2.0 ** 32, 1.0, 1.0, 0, 0, 1, 0, 1),
              (1000, 1, 2.0 ** 32 * (1 + 2.0 ** -52), 1.0, 1.0, 0, 0, 1, 0, 1), (1000, 1, np.nan, 1.0, 1.0, 0, 0, 1, 0, 1),
              (1000, 0, 1.0, 0.0, 1.0, 0, 0, 1, 1, 1), (1000, 0, 1.0, 0.0, 1.0, 0, 0, 1, 0, 1), (1000, 0, 1.0, np.inf, 1.0, 0, 0, 1, 1, 1),
              (1000, 0, 1.0, 1.0, -0.5, 0, 0, 1, 0, 1), (1000, 0, 1.0, 1.0, np.nan, 0, 0, 1, 0, 1), (1000, 0, 1.0, 1.0, np.inf, 0, 0, 1, 0, 1),
              (1000, 0, 1.0, 1.0, 0.0, 0, 0, 1, 0, 1), (1000, 0, 1.0, 1.0, 1.0, 4096, 65536, 1 << 20, 0, 1), (1000, 0, 1.0, 1.0, 1.0, 4097, 0, 1, 0, 1),
              (1000, 0, 1.0, 1.0, 1.0, 0, 65537, 1, 0, 1), (1000, 0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 1), (1000, 0, 1.0, 1.0, 1.0, 0, 0, (1 << 20) + 1, 0, 1),
              (LM.MAX_FRAMES - 1, 0, 1.0, 1.0, 1.0, 0, 0, 1, 0, 1), (LM.MAX_FRAMES, 0, 1.0, 1.0, 1.0, 0, 0, 1, 0, 1), (1 << 63, 0, 1.0, 1.0, 1.0, 0, 0, 1, 0, 1),
              (1 << 24, 0, 1.0, 1.0, 1.0, 0, 0, 1 << 20, 0, 1), ((1 << 24) + 1, 0, 1.0, 1.0, 1.0, 0, 0, 1 << 20, 0, 1)]
    for n, sense, d, kg, mk, A, H, R, keyed, has in checks:
        lines.append("c %d %d %s %s %s %d %d %d %d %d" % (n, sense, hexd(d), hexd(kg), hexd(mk), A, H, R, keyed, has))
        want.append("c %d" % M.check_args(n, cur if has else None, sense, d, kg, mk, A, H, R, bool(keyed)))
    for at, v in ((5, -0.0), (3072, np.nan), (0, 1.0 + 2.0 ** -52)):   # a spoiled table is refused by the check and by the call
        lines += ["m %d %s" % (at, hexd(v)), "k 0", "c 1000 0 %s %s %s 0 0 1 0 1" % (hexd(1.0), hexd(1.0), hexd(1.0)), "m %d %s" % (at, hexd(cur[at]))]
        want += ["k -4 %s" % hexd(7.0), "c -4"]
    lines.append("k 1")
    want.append("k 0 %s" % hexd(cur.min()))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert got[-1] == "dynamics ok" and len(got) == len(want) + 1
    printing = [l for l in lines if not l.startswith("m ")]
    for g, w, line in zip(got, want, printing):
        assert g == w, line[:80]
    assert {w for w in want if w.startswith("c ")} == {"c 0", "c -4", "c -3"}
