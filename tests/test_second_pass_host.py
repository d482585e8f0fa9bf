"""The matrix covers what it claims: every shape of tests/second_pass.py, which the GPU tests of clipfx_kernel, resample_kernel,
pitch_kernel and true_peak_kernel run, has more tiles than the launch has workgroups — by the library's own launch-shape
getters, without a device — and the seam tests that never claimed a second pass do not reach one.  A raised cap fails here."""
import ctypes as C

import pytest

import loudness_model as LM
import pitch_model as PM
import resample_model as RS
import second_pass as SP
import stretch_model as ST
import whitebox_amd as W
from whitebox_amd import _ffi

RESAMPLE_CASES = [(8000, 192000, "good"), (22050, 192000, "fast")]


def test_clipfx_shapes_pass_the_first_pass_of_the_grid():
    P = W.clipfx_pass_frames()
    n = SP.clipfx_frames()
    assert P > 0 and P % 512 == 0 and n > P                      # whole waves per pass
    assert n - 8 > P, "the ranges that start at first_frame 3, 5 and 8 of the same clip"
    assert (n - P) % 512 and (n - P) % 8 == 5                    # ends inside a wave; the last lane holds 5 frames
    assert SP.CLIPFX_SEAMS_FRAMES <= P and 1 << 21 <= P           # the seam test and the thread test stay in one pass
    assert 4096 * 2048 + 1037 > P                                # test_gpu_splice.py::test_grid_stride's stats reach a second


@pytest.mark.parametrize("rs,rd,q", RESAMPLE_CASES)
def test_resample_shapes_have_three_tiles_more_than_workgroups(rs, rd, q):
    n_in, n_out, sh, G = SP.resample_case(rs, rd, q)
    p = RS.plan(rs, rd, _ffi.SRC_QUALITY[q])
    assert sh["tile"] == 1024 == min(1024, ((4096 - p["T"]) * p["L"] // p["M"] + 1) & ~3)     # upsampling: the full tile
    assert sh["span"] == (p["L"] - 1 + (sh["tile"] - 1) * p["M"]) // p["L"] + p["T"] <= 4096
    assert sh["grid"] == G and sh["n_tiles"] == G + 3 == -(-n_out // sh["tile"])
    assert n_out % sh["tile"] and n_out == RS.out_frames(rs, rd, n_in) < SP.MAX_FRAMES
    assert (n_out % 4 != 0) == (p["L"] % 4 != 0 or p["M"] != 1), "a ragged last word wherever the ratio has one"


def test_one_of_the_resample_shapes_ends_inside_a_16_byte_word():
    assert any(SP.resample_case(*c)[1] % 4 for c in RESAMPLE_CASES)
    assert {RS.plan(rs, rd, _ffi.SRC_QUALITY[q])["L"] for rs, rd, q in RESAMPLE_CASES} == {24, 1280}    # both ends of the table


def test_the_seam_tests_of_resample_stay_inside_one_pass():
    for rs, rd in ((44100, 48000), (48000, 44100)):
        sh = W.resample_launch_shape(rs, rd, "good", W.resample_frames(rs, rd, SP.RESAMPLE_SEAMS_FRAMES))
        assert 1 < sh["n_tiles"] == sh["grid"]
    rs, rd, q, n = SP.RESAMPLE_LONGEST
    sh = W.resample_launch_shape(rs, rd, q, W.resample_frames(rs, rd, n))
    assert sh["tile"] < 1024 and sh["n_tiles"] == sh["grid"]
    # a downsampling tile below 1024 needs far more source than a test may hold to reach a second pass: the case is left out
    G = W.resample_launch_shape(rs, rd, q, SP.MAX_FRAMES - 1)["grid"]
    assert (G * sh["tile"] + 1) * 640 // 147 > 200_000_000


@pytest.mark.parametrize("source", SP.PITCH_RANGES)
def test_pitch_shape_has_three_tiles_more_than_workgroups(source):
    n, m, mid, sh, G = SP.pitch_case(source)
    k = SP.PITCH
    Hs = k["window"] // 2
    assert sh["tile"] == 1024 and sh["grid"] == G and sh["n_tiles"] == G + 3 == -(-m // 1024) and m % 4 == 1
    assert mid == PM.mid_frames(m, k["num"], k["den"]) == -(-m // 2) and n == (-(-mid // 8) + 5 if source == "eighth" else mid + mid // 16 + 5)
    # the frames the last step gives the intermediate: all inside the range from "longer", past its end after a few from "eighth"
    last = ST.steps(mid, k["window"]) - 1
    inside, needed = n - ST.anchor(last, n, mid, k["window"]), mid - last * Hs
    assert (inside >= needed) if source == "longer" else (0 < inside < needed // 4)
    assert last * Hs <= G * 1024 // 2, "the second pass's tiles lie in the last step"
    assert PM.check_args(n, m, k["num"], k["den"], _ffi.SRC_QUALITY[k["quality"]], k["window"], k["tolerance"]) == 0
    # the conversion's own getter gives the pitch call's shape: one formula
    assert sh == W.resample_launch_shape(k["num"], k["den"], k["quality"], m)


def test_true_peak_shape_has_three_tiles_more_than_workgroups():
    n_in, sh, G, tile_frames = SP.true_peak_case()
    assert sh["factor"] == 4 == LM.oversampling(SP.TRUE_PEAK_RATE) and tile_frames == 256
    assert sh["grid"] == G and sh["n_tiles"] == G + 3 and (4 * n_in) % 1024
    assert W.true_peak_launch_shape(SP.TRUE_PEAK_RATE, n_in - 3) == sh      # the range that starts at first_frame 3
    assert W.true_peak_launch_shape(SP.TRUE_PEAK_RATE, 1 << 20)["n_tiles"] <= G   # the thread test stays in one pass


def test_the_getters_refuse_what_the_calls_refuse():
    L = W.lib()
    v = [C.c_uint32(7) for _ in range(4)]
    ptr = [C.byref(x) for x in v]
    assert L.wbx_resample_launch_shape(48000, 48000, 1, 100, *ptr) == -4 and L.wbx_resample_launch_shape(11025, 192000, 1, 100, *ptr) == -3
    assert L.wbx_resample_launch_shape(44100, 48000, 1, 0, *ptr) == -4 and L.wbx_resample_launch_shape(44100, 48000, 1, SP.MAX_FRAMES, *ptr) == -4
    assert L.wbx_resample_launch_shape(44100, 48000, 1, 100, None, *ptr[1:]) == -4
    assert L.wbx_pitch_launch_shape(7, 7, 1, 100, *ptr) == -4 and L.wbx_pitch_launch_shape(0, 1, 1, 100, *ptr) == -4 and L.wbx_pitch_launch_shape(5, 1, 1, 100, *ptr) == -3
    assert L.wbx_pitch_launch_shape(3, 2, 9, 100, *ptr) == -4 and L.wbx_pitch_launch_shape(3, 2, 1, 0, *ptr) == -4
    assert L.wbx_true_peak_launch_shape(7999, 100, *ptr[:3]) == -3 and L.wbx_true_peak_launch_shape(48000, 0, *ptr[:3]) == -4
    assert L.wbx_true_peak_launch_shape(48000, 1 << 29, *ptr[:3]) == -3
    assert [x.value for x in v] == [7] * 4                       # nothing is written after a refusal
    assert W.true_peak_launch_shape(192000, 1000) == {"factor": 1, "n_tiles": 0, "grid": 0}
    assert W.resample_launch_shape(44100, 48000, "good", 5) == {"tile": 1024, "span": (159 + 1023 * 147) // 160 + 48, "n_tiles": 1, "grid": 1}
