"""The shapes at which the four capped clip kernels — clipfx_kernel, resample_kernel, pitch_kernel, true_peak_kernel — take a
SECOND pass over their grid (`for (...; x += gridDim.x * ...)`), computed from the library's host-only launch-shape getters
instead of restating the caps.  The GPU tests that run these shapes import them from here, and tests/test_second_pass_host.py
asserts, without a device, that each of them has more tiles than workgroups: raise a cap and that test fails instead of the
coverage silently vanishing.  Each shape is the smallest that reaches a second pass AND ends raggedly in it."""
import whitebox_amd as W
from whitebox_amd import synth

MAX_FRAMES = (1 << 31) - 16                                     # every pool clip is shorter

# the longest shapes of the seam tests that stay inside ONE pass (workgroup, wave and tile seams only)
CLIPFX_SEAMS_FRAMES = (1 << 20) + 3                             # test_gpu_clipfx.py::test_workgroup_and_wave_seams
RESAMPLE_SEAMS_FRAMES = (1 << 18) + 3                           # test_gpu_resample.py::test_tile_seams, 44100 <-> 48000 at GOOD
RESAMPLE_LONGEST = (192000, 44100, "fast", 29_300_000)          # test_gpu_resample.py::test_positions_past_2_to_the_32


class SynthPlane:
    """one channel of a wbx_clip_synth clip (whitebox_amd/synth.py's generator), sliced lazily: a model asks for the frames a
    window needs, and no test holds a plane of 10^7 frames on the host"""

    def __init__(self, seed, track, chan, frames, amp):
        self.seed, self.track, self.chan, self.frames, self.amp = seed, track, chan, frames, amp

    def __getitem__(self, s):
        assert s.step is None and 0 <= s.start <= s.stop <= self.frames
        return synth.clip_channel(self.seed, self.track, self.chan, s.stop - s.start, self.amp, first=s.start)


def clipfx_frames():
    """one pass and 1037 frames: the range ends inside a wave of the second pass, its last lane holding 5 frames"""
    return W.clipfx_pass_frames() + 1037


def resample_case(src_rate, dst_rate, quality):
    """(n_in, n_out, shape, G): the range whose result has G + 3 tiles, G the grid's cap, and a ragged last tile; n_out is no
    multiple of 4 where the ratio allows one (L = 24, M = 1 does not: every n_out is 24 n)"""
    cap = W.resample_launch_shape(src_rate, dst_rate, quality, MAX_FRAMES - 1)
    G, tile = cap["grid"], cap["tile"]
    p = W.resample_plan(src_rate, dst_rate, quality)
    n0 = (G + 2) * tile * p["M"] // p["L"] + 1                   # the first n_in whose n_out exceeds G + 2 tiles
    n_in = n0 + 12
    for n in range(n0 + 12, n0 + 76):
        if W.resample_frames(src_rate, dst_rate, n) % 4:
            n_in = n
            break
    n_out = W.resample_frames(src_rate, dst_rate, n_in)
    return n_in, n_out, W.resample_launch_shape(src_rate, dst_rate, quality, n_out), G


PITCH = dict(num=1, den=2, quality="fast", window=8192, tolerance=0)


PITCH_RANGES = ("eighth", "longer")


def pitch_case(source="eighth"):
    """(n, m, mid, shape, G): down an octave (L 2, M 1) to m = (G + 2) tiles + 301 frames.  "eighth": from the shortest range
    the stretch accepts for that intermediate (m' <= 8 n) and five frames more — the steps of the second pass's tiles then
    read past the range's end, and most of what these tiles store is silence.  "longer": from a range a sixteenth longer than
    the intermediate, so that every step is a blend (p_k - p_{k-1} = Hs + Hs / 16) of frames inside the range, to the end"""
    cap = W.pitch_launch_shape(PITCH["num"], PITCH["den"], PITCH["quality"], MAX_FRAMES - 1)
    G, tile = cap["grid"], cap["tile"]
    m = (G + 2) * tile + 301
    mid = W.pitch_mid_frames(m, PITCH["num"], PITCH["den"])
    n = -(-mid // 8) + 5 if source == "eighth" else mid + mid // 16 + 5
    return n, m, mid, W.pitch_launch_shape(PITCH["num"], PITCH["den"], PITCH["quality"], m), G


TRUE_PEAK_RATE = 48000


def true_peak_case():
    """(n_in, shape, G, tile_frames): at factor 4 a tile of 1024 oversampled frames is 256 source frames; G tiles and 767
    frames are three second-pass tiles whose last is ragged"""
    cap = W.true_peak_launch_shape(TRUE_PEAK_RATE, (MAX_FRAMES - 1) // 4)
    G, factor = cap["grid"], cap["factor"]
    assert factor == 4
    tile_frames = next(n for n in range(1, 1 << 16) if W.true_peak_launch_shape(TRUE_PEAK_RATE, n + 1)["n_tiles"] == 2)
    n_in = G * tile_frames + 767
    return n_in, W.true_peak_launch_shape(TRUE_PEAK_RATE, n_in), G, tile_frames
