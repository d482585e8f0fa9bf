"""Editing clips, the part that needs no device: the symbols and structs of include/wbx.h "Editing clips" exist and match
their binding twins, the adapter's three methods compile, NULL handles are refused, and the host model (tests/clipfx_model.py)
has the properties the device tests lean on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clipfx_model as M
import oracle_ffi as O
import whitebox_amd as W
from whitebox_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wbx_clipfx_pass_frames", "wbx_clip_measure", "wbx_clip_derive", "wbx_engine_measure_sample", "wbx_engine_derive_sample", "wbx_engine_normalize_sample"]


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wbx.h")).read()
    L = W.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(L, n) and n in _ffi.SYMBOLS, n


def test_struct_sizes_equal_the_headers(tmp_path):
    """sizeof / offsetof as the C compiler lays the header's structs out, against the ctypes twins"""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wbx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wbx_clip_stats), sizeof(wbx_clip_edit_desc),\n'
                   '  offsetof(wbx_clip_stats, peak_frame), offsetof(wbx_clip_stats, sum), offsetof(wbx_clip_edit_desc, gain),\n'
                   '  offsetof(wbx_clip_edit_desc, fade_in), offsetof(wbx_clip_edit_desc, fade_out_shape)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S, D = _ffi.ClipStats, _ffi.ClipEditDesc
    assert got == [C.sizeof(S), C.sizeof(D), S.peak_frame.offset, S.sum.offset, D.gain.offset, D.fade_in.offset, D.fade_out_shape.offset]
    assert got[:2] == [104, 56]
    enums = dict(re.findall(r"\b(WBX_(?:EDIT|CH|FADE)_[A-Z_]+) = (\d+)", open(os.path.join(ROOT, "include", "wbx.h")).read()))
    assert int(enums["WBX_EDIT_REVERSE"]) == _ffi.EDIT_REVERSE == M.REVERSE
    for name, val in _ffi.CH_MODE.items():
        assert int(enums["WBX_CH_" + name.upper()]) == val == getattr(M, name.upper())
    for name, val in _ffi.FADE_SHAPE.items():
        assert int(enums["WBX_FADE_" + name.upper()]) == val == getattr(M, name.upper())


def test_adapter_with_the_edit_methods_compiles(tmp_path):
    """a translation unit that uses Engine::measure_sample / derive_sample / normalize_sample (never run: it would need a device)"""
    src = tmp_path / "adapter_clipfx.cpp"
    src.write_text('#include "wbx_adapter.hpp"\n'
                   'uint32_t tidy(wbx::Engine& e, uint32_t take, uint64_t n) {\n'
                   '  float gain = 0.0f;\n'
                   '  const uint32_t loud = e.normalize_sample(take, 0, n, 0.5f, &gain);\n'
                   '  const wbx_clip_stats st = e.measure_sample(loud, 0, n);\n'
                   '  wbx_clip_edit_desc d{};\n'
                   '  d.first_frame = st.peak_frame[0]; d.n_frames = n - d.first_frame; d.channel_mode = WBX_CH_KEEP; d.gain = 1.0f;\n'
                   '  d.fade_out = d.n_frames / 2; d.fade_out_shape = WBX_FADE_SMOOTH; d.flags = WBX_EDIT_REVERSE;\n'
                   '  return e.derive_sample(loud, d);\n}\n'
                   'int main() { return sizeof(wbx_clip_stats) == 104 && sizeof(wbx_clip_edit_desc) == 56 ? 0 : 1; }\n')
    exe = str(tmp_path / "adapter_clipfx")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx", "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.call([exe]) == 0


def test_null_handles_are_refused_without_a_device():
    L = W.lib()
    st, d, new, g = _ffi.ClipStats(), W.edit_desc(0, 8), C.c_uint32(), C.c_float()
    assert L.wbx_clip_measure(None, 0, 0, 8, C.byref(st)) == -4
    assert L.wbx_clip_derive(None, 0, 1, C.byref(d), None) == -4
    assert L.wbx_engine_measure_sample(None, 0, 0, 8, C.byref(st)) == -4
    assert L.wbx_engine_derive_sample(None, 0, C.byref(d), C.byref(new)) == -4
    assert L.wbx_engine_normalize_sample(None, 0, 0, 8, 0.5, C.byref(new), C.byref(g)) == -4


# ---- the model's own properties ---------------------------------------------------------------------------------------------
def planes(channels, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.5, 1.5, n).astype(np.float32) for _ in range(channels)]


def bits(arrs):
    return [np.ascontiguousarray(a).view(np.uint32).tolist() for a in arrs]


@pytest.mark.parametrize("channels", [1, 2])
def test_reverse_of_reverse_is_the_identity(channels):
    src = planes(channels, 333, 1)
    once = M.derive(src, 5, 300, reverse=True)
    twice = M.derive(once, 0, 300, reverse=True)
    assert bits(twice) == bits([p[5:305] for p in src])


@pytest.mark.parametrize("shape", [M.LINEAR, M.SQUARE, M.SMOOTH])
@pytest.mark.parametrize("fade", [1, 9, 300])
def test_reversed_fade_in_is_the_reverse_of_forward_fade_out(shape, fade):
    src = planes(2, 333, 2)
    a = M.derive(src, 3, 300, reverse=True, gain=0.5, fade_in=fade, shape_in=shape)
    b = M.derive(src, 3, 300, gain=0.5, fade_out=fade, shape_out=shape)
    assert bits(a) == bits([p[::-1] for p in b])


@pytest.mark.parametrize("shape", [M.LINEAR, M.SQUARE, M.SMOOTH])
def test_weights_start_at_zero_and_stay_within_one(shape):
    for length in (1, 2, 9, 1000, 65537):
        w = M.fade_weights(np.arange(length), length, shape)
        assert w.dtype == np.float32 and w[0] == 0 and np.all(w >= 0) and np.all(w <= 1)
    one = np.ones((1, 10), dtype=np.float32)
    faded = M.derive(one, 0, 10, fade_in=4, fade_out=4, shape_in=shape, shape_out=shape)[0]
    assert faded[0] == 0 and faded[9] == 0 and np.all(faded[4:6] == 1)


def test_peak_is_the_oracles_abs_max():
    L = O.lib()
    for seed, n in ((3, 1), (4, 511), (5, 5003)):
        x = planes(1, n, seed)[0]
        st = M.measure([x])
        assert np.float32(L.wbo_abs_max(x.ctypes.data_as(O.c_f32p), n)).tobytes() == np.float32(st["peak"][0]).tobytes()
        assert abs(x[st["peak_frame"][0]]) == st["peak"][0] and not np.any(np.abs(x[:st["peak_frame"][0]]) == st["peak"][0])


def test_measure_special_values():
    x = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-40, 2.0, np.inf], dtype=np.float32)
    st = M.measure([x, np.array([np.nan, np.nan], dtype=np.float32), np.array([0.0, -0.0], dtype=np.float32)])
    assert st["peak"][0] == np.inf and st["peak_frame"][0] == 3 and st["nans"][0] == 1 and st["over"][0] == 4
    assert st["min"][0] == -np.inf and st["max"][0] == np.inf
    assert (st["peak"][1], st["peak_frame"][1], st["nans"][1]) == (0, 0, 2)
    assert np.float32(st["min"][1]).tobytes() == np.float32(0.0).tobytes() == np.float32(st["max"][1]).tobytes()
    assert np.float32(st["min"][2]).tobytes() == np.float32(-0.0).tobytes() and np.float32(st["max"][2]).tobytes() == np.float32(0.0).tobytes()
    nan_out = M.derive([x], 0, 8, fade_in=8)[0].view(np.uint32)
    assert nan_out[0] == 0x7FC00000 and nan_out[1] == 0x80000000   # inf * 0 would be frame 3 only with a fade of weight 0 there


def test_normalize_gain_is_one_fp32_division():
    for target, peak in ((0.5, 0.3), (1.0, 3.0), (0.891, 1e-30)):
        g = M.normalize_gain(target, peak)
        assert g.dtype == np.float32 and g == np.float32(target) / np.float32(peak)
        assert g == np.float32(np.float64(np.float32(target)) / np.float64(np.float32(peak)))   # (fp64 then fp32: the same rounding)


def test_the_models_exact_sums_are_math_fsum():
    """measure()'s sum, sum_sq and abs_sum go through exact_sum (binade by binade, for clips of 10^7 frames); it must give
    math.fsum's correctly rounded value whatever the range of the samples: denormals, 10^-30 beside 10^30, cancellation"""
    import math
    rng = np.random.default_rng(0xE5AC7)
    for t in range(120):
        n = int(rng.integers(0, 3000))
        x = [rng.uniform(-1.4, 1.4, n), rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n), rng.integers(-2 ** 24, 2 ** 24, n) * 2.0 ** -149,
             np.where(rng.random(n) < 0.5, 3e38, -3e38) * rng.random(n), np.concatenate([rng.uniform(-1, 1, n), [1e30, -1e30, 1e-30, -0.0, 0.0]]),
             rng.uniform(-1e-20, 1e-20, n)][t % 6]
        d = np.asarray(x, dtype=np.float32).astype(np.float64)
        hi, lo = M.split26(d * d)
        assert np.array_equal(hi + lo, d * d) and np.all(np.frexp(hi)[0] * 2.0 ** 26 % 1 == 0) and np.all(np.frexp(lo)[0] * 2.0 ** 26 % 1 == 0)
        assert M.exact_sum(d, bits=24) == math.fsum(d) and M.exact_sum(np.abs(d), bits=24) == math.fsum(np.abs(d)), t
        assert M.exact_sum(hi, lo, bits=26) == math.fsum(d * d), t
