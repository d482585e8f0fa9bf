"""Export (wbx_clip_export, wbx_engine_export_sample, whitebox_amd/wav.py): everything that needs no device — byte counts,
argument refusals in front of any device call, the ctypes mirror of wbx_export_stats, the C++ adapter, and the WAVE
writer against the standard library's reader."""
import ctypes as C
import itertools
import os
import struct
import subprocess
import wave

import numpy as np
import pytest

import whitebox_amd as W
from whitebox_amd import _ffi, wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = {"i16": 2, "i24": 3, "i24_x8": 4, "i32": 4, "f32": 4}


@pytest.mark.parametrize("fmt,channels,n", list(itertools.product(BYTES, (1, 2), (0, 1, 7, 1000))))
def test_export_bytes(fmt, channels, n):
    assert W.lib().wbx_export_bytes(_ffi.OUT_FMT[fmt], channels, n) == BYTES[fmt] * channels * n


@pytest.mark.parametrize("fmt", [0, 1, 4, 8, 10, -1])
def test_export_bytes_of_an_unknown_format_is_zero(fmt):
    assert W.lib().wbx_export_bytes(fmt, 2, 1000) == 0


def test_export_bytes_beyond_32_bits():
    assert W.lib().wbx_export_bytes(_ffi.OUT_FMT["i24"], 2, (1 << 31) - 17) == 6 * ((1 << 31) - 17)


def test_null_and_invalid_arguments_are_rejected_without_a_device():
    L = W.lib()
    buf = (C.c_uint8 * 64)(*([0xA5] * 64))
    st = _ffi.ExportStats()
    assert L.wbx_clip_export(None, 0, 0, 8, _ffi.OUT_FMT["i16"], 0, buf, C.byref(st)) == -4
    assert L.wbx_clip_export(None, 0, 0, 8, _ffi.OUT_FMT["i16"], 0, None, None) == -4
    assert L.wbx_engine_export_sample(None, 0, 0, 8, _ffi.OUT_FMT["i16"], 1, buf, C.byref(st)) == -4
    assert L.wbx_set_export_chunk(None, 64) == -4
    assert L.wbx_set_export_chunk(None, 0) == -4
    assert bytes(buf) == b"\xA5" * 64


def test_export_stats_has_the_headers_size(tmp_path):
    """sizeof / offsetof as the C compiler lays wbx_export_stats out, against the ctypes mirror"""
    src = tmp_path / "stats_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wbx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(wbx_export_stats), offsetof(wbx_export_stats, peak),\n'
                   '         offsetof(wbx_export_stats, over), offsetof(wbx_export_stats, nans));\n'
                   '  return WBX_EXPORT_CLAMP == 1 ? 0 : 1;\n}\n')
    exe = str(tmp_path / "stats_size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _ffi.ExportStats
    assert got == [C.sizeof(S), S.peak.offset, S.over.offset, S.nans.offset] == [40, 0, 8, 24]
    assert _ffi.EXPORT_CLAMP == 1


def test_adapter_with_export_sample_compiles(tmp_path):
    """the compile step of test_abi.py::test_adapter_audio_buffer_host_semantics over a translation unit that uses
    Engine::export_sample (never run: it would need a device)"""
    src = tmp_path / "adapter_export.cpp"
    src.write_text('#include <vector>\n#include "wbx_adapter.hpp"\n'
                   'wbx_export_stats stem_to_i24(wbx::Engine& e, uint32_t sample, uint64_t n, std::vector<unsigned char>& out) {\n'
                   '  out.resize(wbx_export_bytes(WBX_OUT_I24, 2, n));\n'
                   '  return e.export_sample(sample, 0, n, WBX_OUT_I24, out.data(), true);\n}\n'
                   'int main() { return wbx_export_bytes(WBX_OUT_I16, 2, 8) == 32 ? 0 : 1; }\n')
    exe = str(tmp_path / "adapter_export")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-L" + os.path.join(ROOT, "whitebox_amd"), "-lwbx", "-Wl,-rpath," + os.path.join(ROOT, "whitebox_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert subprocess.call([exe]) == 0


@pytest.mark.parametrize("bits,channels", list(itertools.product((16, 24, 32), (1, 2))))
def test_wav_pcm_reads_back_with_the_standard_library(tmp_path, bits, channels):
    rng = np.random.default_rng(bits * 10 + channels)
    for n in (0, 1, 333):   # 333 frames of mono 24-bit: an odd number of bytes, the pad byte
        payload = rng.integers(0, 256, n * channels * bits // 8, dtype=np.uint8).tobytes()
        path = tmp_path / f"pcm_{bits}_{channels}_{n}.wav"
        with open(path, "wb") as f:
            wav.write_bytes(f, channels, 44100, bits, payload)
        assert os.path.getsize(path) == 44 + len(payload) + (len(payload) & 1)
        with wave.open(str(path), "rb") as r:
            assert (r.getnchannels(), r.getsampwidth(), r.getframerate(), r.getnframes(), r.getcomptype()) == \
                   (channels, bits // 8, 44100, n, "NONE")
            assert r.readframes(n) == payload


@pytest.mark.parametrize("channels", [1, 2])
def test_wav_float_header_fields(channels):
    n = 1000
    h = wav.header(channels, 48000, 32, n, float32=True)
    assert len(h) == 58
    riff, size, wave_id, fmt_id, fmt_len = struct.unpack_from("<4sI4s4sI", h, 0)
    assert (riff, wave_id, fmt_id, fmt_len) == (b"RIFF", b"WAVE", b"fmt ", 18)
    tag, ch, rate, byte_rate, align, bits, cb = struct.unpack_from("<HHIIHHH", h, 20)
    assert (tag, ch, rate, byte_rate, align, bits, cb) == (3, channels, 48000, 48000 * 4 * channels, 4 * channels, 32, 0)
    fact, fact_len, fact_frames, data_id, data_len = struct.unpack_from("<4sII4sI", h, 38)
    assert (fact, fact_len, fact_frames, data_id, data_len) == (b"fact", 4, n, b"data", n * 4 * channels)
    assert size == len(h) - 8 + data_len


def test_wav_refuses_what_it_cannot_write():
    with pytest.raises(ValueError):
        wav.header(2, 48000, 8, 10)
    with pytest.raises(ValueError):
        wav.header(2, 48000, 16, 10, float32=True)
    with pytest.raises(ValueError):
        wav.header(2, 48000, 32, 1 << 30)          # 8 GiB
    with pytest.raises(ValueError):
        wav.write_bytes(open(os.devnull, "wb"), 2, 48000, 24, b"\0" * 7)
