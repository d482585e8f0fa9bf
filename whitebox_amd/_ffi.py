"""ctypes binding of include/wbx.h.  Loading fails loudly when libwbx.so has not been built."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("WBX_LIB") or os.path.join(_HERE, "libwbx.so")   # WBX_LIB: A/B another build of the library


class WbxError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: wbx_status {status}" + (f" ({detail})" if detail else ""))


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_tracks", C.c_uint32), ("max_blocks", C.c_uint32),
                ("block_frames", C.c_uint32), ("channels", C.c_uint32), ("sample_rate", C.c_uint32),
                ("group_size", C.c_uint32), ("max_segments", C.c_uint32), ("stream", C.c_void_p)]


class Segment(C.Structure):
    _fields_ = [("sample_offset", C.c_double), ("playback_speed", C.c_double), ("clip", C.c_uint32),
                ("buffer_offset", C.c_uint32), ("num_samples", C.c_uint32), ("gain", C.c_float)]


class ClipInfo(C.Structure):
    _fields_ = [("min_time", C.c_double), ("max_time", C.c_double), ("start_offset", C.c_double), ("speed", C.c_double),
                ("gain", C.c_float), ("sample", C.c_uint32)]


class PluginProcessInfo(C.Structure):
    _fields_ = [("sample_count", C.c_uint32), ("input_buffer_count", C.c_uint32), ("output_buffer_count", C.c_uint32),
                ("n_channels", C.c_uint32), ("input_buffer", C.POINTER(C.POINTER(C.c_float))),
                ("output_buffer", C.POINTER(C.POINTER(C.c_float))), ("input_event_list", C.c_void_p),
                ("sample_rate", C.c_double), ("tempo", C.c_double), ("project_time_in_ppq", C.c_double),
                ("project_time_in_samples", C.c_int64), ("playing", C.c_int32)]


class Plugin(C.Structure):
    _fields_ = [("userdata", C.c_void_p), ("process", C.c_void_p)]


class RecordInfo(C.Structure):
    _fields_ = [("recording", C.c_int32), ("armed", C.c_int32), ("input_type", C.c_int32), ("input_index", C.c_uint32),
                ("min_time", C.c_double), ("max_time", C.c_double), ("frames", C.c_uint64), ("status", C.c_uint32),
                ("_pad", C.c_uint32)]


class BounceSource(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint32), ("tap", C.c_int32), ("_pad", C.c_uint32)]


class ExportStats(C.Structure):
    _fields_ = [("peak", C.c_float * 2), ("over", C.c_uint64 * 2), ("nans", C.c_uint64 * 2)]


class ClipStats(C.Structure):          # wbx_clip_stats, 104 bytes
    _fields_ = [("peak", C.c_float * 2), ("min", C.c_float * 2), ("max", C.c_float * 2), ("peak_frame", C.c_uint64 * 2),
                ("over", C.c_uint64 * 2), ("nans", C.c_uint64 * 2), ("sum", C.c_double * 2), ("sum_sq", C.c_double * 2)]


class ClipEditDesc(C.Structure):       # wbx_clip_edit_desc, 56 bytes
    _fields_ = [("first_frame", C.c_uint64), ("n_frames", C.c_uint64), ("flags", C.c_uint32), ("channel_mode", C.c_int32),
                ("gain", C.c_float), ("_pad", C.c_uint32), ("fade_in", C.c_uint64), ("fade_out", C.c_uint64),
                ("fade_in_shape", C.c_int32), ("fade_out_shape", C.c_int32)]


class ResampleInfo(C.Structure):       # wbx_resample_info, 24 bytes
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("half_width", C.c_uint32), ("taps", C.c_uint32),
                ("table_floats", C.c_uint64)]


class Loudness(C.Structure):           # wbx_loudness, 80 bytes
    _fields_ = [("integrated", C.c_double), ("gated_power", C.c_double), ("momentary_max", C.c_double),
                ("short_term_max", C.c_double), ("range_lu", C.c_double), ("true_peak", C.c_float * 2), ("hops", C.c_uint64),
                ("blocks", C.c_uint64), ("blocks_gated", C.c_uint64), ("hop_frames", C.c_uint32), ("oversampling", C.c_uint32)]


class LimitStats(C.Structure):         # wbx_limit_stats, 32 bytes
    _fields_ = [("peak_in", C.c_double), ("min_gain", C.c_double), ("min_gain_frame", C.c_uint64), ("limited_frames", C.c_uint64)]


class DynamicsStats(C.Structure):      # wbx_dynamics_stats, 24 bytes
    _fields_ = [("min_gain", C.c_double), ("min_gain_frame", C.c_uint64), ("reduced_frames", C.c_uint64)]


class SaturateStats(C.Structure):      # wbx_saturate_stats, 24 bytes
    _fields_ = [("peak_drive", C.c_double), ("peak_index", C.c_uint64), ("beyond", C.c_uint64)]


class VarispeedInfo(C.Structure):      # wbx_varispeed_info, 32 bytes
    _fields_ = [("half_width", C.c_uint32), ("taps", C.c_uint32), ("phases", C.c_uint32), ("reserved", C.c_uint32),
                ("cutoff", C.c_double), ("beta", C.c_double)]


class VarispeedTile(C.Structure):      # wbx_varispeed_tile, 24 bytes
    _fields_ = [("first_out", C.c_uint32), ("n_out", C.c_uint32), ("lo_frame", C.c_int64), ("span", C.c_uint32),
                ("reserved", C.c_uint32)]


class DenoiseStats(C.Structure):       # wbx_denoise_stats, 32 bytes
    _fields_ = [("hops", C.c_uint64), ("cells", C.c_uint64), ("open_cells", C.c_uint64), ("bands", C.c_uint32),
                ("reserved", C.c_uint32)]


class StretchInfo(C.Structure):        # wbx_stretch_info, 32 bytes
    _fields_ = [("steps", C.c_uint64), ("searched_steps", C.c_uint64), ("candidates", C.c_uint64), ("max_shift", C.c_uint32),
                ("launches", C.c_uint32)]


class WarpMarker(C.Structure):         # wbx_warp_marker, 16 bytes
    _fields_ = [("src_frame", C.c_uint64), ("out_frame", C.c_uint64)]


class WarpInfo(C.Structure):           # wbx_warp_info, 40 bytes
    _fields_ = [("steps", C.c_uint64), ("searched_steps", C.c_uint64), ("candidates", C.c_uint64), ("max_shift", C.c_uint32),
                ("launches", C.c_uint32), ("segments", C.c_uint32), ("longest_segment_steps", C.c_uint32)]


class WarpSegment(C.Structure):        # wbx_warp_segment, 32 bytes
    _fields_ = [("src_frame", C.c_uint64), ("out_frame", C.c_uint64), ("first_step", C.c_uint64), ("steps", C.c_uint64)]


class PitchInfo(C.Structure):          # wbx_pitch_info, 48 bytes
    _fields_ = [("steps", C.c_uint64), ("searched_steps", C.c_uint64), ("candidates", C.c_uint64), ("mid_frames", C.c_uint64),
                ("max_shift", C.c_uint32), ("launches", C.c_uint32), ("L", C.c_uint32), ("M", C.c_uint32)]


class F0Frame(C.Structure):            # wbx_f0_frame, 32 bytes
    _fields_ = [("period", C.c_double), ("dip", C.c_double), ("energy", C.c_double), ("lag", C.c_uint32), ("voiced", C.c_uint32)]


class F0Info(C.Structure):             # wbx_f0_info, 32 bytes
    _fields_ = [("hops", C.c_uint64), ("voiced_hops", C.c_uint64), ("terms", C.c_uint64), ("launches", C.c_uint32),
                ("_pad", C.c_uint32)]


class AlignInfo(C.Structure):          # wbx_align_info, 80 bytes
    _fields_ = [("lag", C.c_int32), ("inverted", C.c_uint32), ("offset", C.c_double), ("score", C.c_double), ("r", C.c_double),
                ("energy", C.c_double), ("ref_energy", C.c_double), ("confidence", C.c_double), ("lags", C.c_uint32),
                ("chunks", C.c_uint32), ("terms", C.c_uint64), ("launches", C.c_uint32), ("_pad", C.c_uint32)]


class AlignPoint(C.Structure):         # wbx_align_point, 16 bytes
    _fields_ = [("r", C.c_double), ("energy", C.c_double)]


ALIGN_EITHER_POLARITY = 1


class OnsetFrame(C.Structure):         # wbx_onset_frame, 32 bytes
    _fields_ = [("energy", C.c_double), ("edge_energy", C.c_double), ("novelty", C.c_double), ("onset", C.c_uint32),
                ("_pad", C.c_uint32)]


class OnsetInfo(C.Structure):          # wbx_onset_info, 24 bytes
    _fields_ = [("hops", C.c_uint64), ("onsets", C.c_uint64), ("launches", C.c_uint32), ("_pad", C.c_uint32)]


class SpectrumInfo(C.Structure):       # wbx_spectrum_info, 16 bytes
    _fields_ = [("hops", C.c_uint64), ("bins", C.c_uint32), ("launches", C.c_uint32)]


SPECTRUM_MID = 2
WINDOW_KIND = {"rect": 0, "hann": 1, "kaiser": 2}


class SplicePart(C.Structure):         # wbx_splice_part, 64 bytes
    _fields_ = [("src_clip", C.c_uint32), ("flags", C.c_uint32), ("first_frame", C.c_uint64), ("n_frames", C.c_uint64),
                ("at", C.c_uint64), ("channel_mode", C.c_int32), ("gain", C.c_float), ("fade_in", C.c_uint64),
                ("fade_out", C.c_uint64), ("fade_in_shape", C.c_int32), ("fade_out_shape", C.c_int32)]


class SpliceSource(C.Structure):       # wbx_splice_source, 24 bytes
    _fields_ = [("channels", C.c_uint32), ("sample_rate", C.c_uint32), ("frames", C.c_uint64), ("format", C.c_int32),
                ("_pad", C.c_uint32)]


class PlanRecord(C.Structure):
    _fields_ = [("block", C.c_uint32), ("track", C.c_uint32), ("buffer_offset", C.c_uint32),
                ("num_samples", C.c_uint32), ("num_actual", C.c_uint32), ("sample", C.c_uint32),
                ("sample_offset", C.c_double), ("playback_speed", C.c_double), ("gain", C.c_float),
                ("flags", C.c_uint32)]


FMT = {"i16": 3, "i24": 5, "i32": 7, "f32": 9}
# TrackInputType (track_input.h:10-15) -> WBX_INPUT_*
INPUT_TYPE = {"none": 0, "midi": 1, "external_stereo": 2, "external_mono": 3}
BOUNCE_KIND = {"track": 0, "bus": 1, "master": 2}     # WBX_BOUNCE_*
BOUNCE_TAP = {"post": 0, "pre": 1}                      # WBX_TAP_*
OUT_FMT = {"i16": 3, "i24": 5, "i24_x8": 6, "i32": 7, "f32": 9}
OUT_DTYPE = {"i16": "<i2", "i24": "u1", "i24_x8": "<i4", "i32": "<i4", "f32": "<f4"}   # numpy element of an exported buffer
EXPORT_CLAMP = 1                                        # WBX_EXPORT_CLAMP
EDIT_REVERSE = 1                                        # WBX_EDIT_REVERSE
CH_MODE = {"keep": 0, "swap": 1, "left": 2, "right": 3, "mono_mix": 4, "dual_mono": 5}   # WBX_CH_*
CH_MODE_OUT = {"swap": 2, "left": 1, "right": 1, "mono_mix": 1, "dual_mono": 2}          # channels of the result ("keep": the source's)
FADE_SHAPE = {"linear": 0, "square": 1, "smooth": 2}    # WBX_FADE_*
SRC_QUALITY = {"fast": 0, "good": 1, "best": 2}         # WBX_SRC_*
LOUD_TRUE_PEAK = 1                                      # WBX_LOUD_TRUE_PEAK
FILTER_KIND = {"lowpass": 0, "highpass": 1, "bandpass": 2, "notch": 3, "allpass": 4, "peak": 5, "lowshelf": 6,
               "highshelf": 7}                          # WBX_FILT_*
DYN_SENSE = {"compress": 0, "gate": 1}                    # WBX_DYN_COMPRESS / WBX_DYN_GATE (a table's kind, a call's sense)
DYN_TABLE, DYN_NO_KEY = 3073, 0xFFFFFFFF                # WBX_DYN_TABLE, WBX_DYN_NO_KEY
SAT_KIND = {"hard": 0, "cubic": 1, "tanh": 2}             # WBX_SAT_HARD / CUBIC / TANH
SAT_TABLE = 16385                                       # WBX_SAT_TABLE
FIR_KIND = {"lowpass": 0, "highpass": 1, "bandpass": 2, "bandstop": 3}   # WBX_FIR_*

# every symbol include/wbx.h declares: name -> (restype, argtypes)
_vp, _u32, _i32, _f, _d, _sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_double, C.c_size_t
_pp = C.POINTER(C.c_void_p)
_fpp = C.POINTER(C.POINTER(C.c_float))
SYMBOLS = {
    "wbx_version": (C.c_char_p, []),
    "wbx_device_count": (C.c_int, []),
    "wbx_status_string": (C.c_char_p, [C.c_int]),
    "wbx_create": (C.c_int, [C.POINTER(Config), _pp]),
    "wbx_destroy": (None, [_vp]),
    "wbx_last_error": (C.c_char_p, [_vp]),
    "wbx_clip_upload": (C.c_int, [_vp, _u32, C.c_int, _u32, _u32, C.c_uint64, _pp]),
    "wbx_clip_synth": (C.c_int, [_vp, _u32, C.c_int, _u32, _u32, C.c_uint64, C.c_uint64, _u32, _f]),
    "wbx_clip_free": (C.c_int, [_vp, _u32]),
    "wbx_clip_pool_stats": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "wbx_clip_upload_interleaved": (C.c_int, [_vp, _u32, C.c_int, _u32, _u32, C.c_uint64, _vp]),
    "wbx_clip_ingest_device": (C.c_int, [_vp, _u32, C.c_int, _u32, _u32, C.c_uint64, _vp]),
    "wbx_clip_download": (C.c_int, [_vp, _u32, _u32, _vp]),
    "wbx_export_bytes": (C.c_uint64, [C.c_int, _u32, C.c_uint64]),
    "wbx_clip_export": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_int, _u32, _vp, C.POINTER(ExportStats)]),
    "wbx_set_export_chunk": (C.c_int, [_vp, _u32]),
    "wbx_clipfx_pass_frames": (C.c_uint64, []),
    "wbx_clip_measure": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.POINTER(ClipStats)]),
    "wbx_clip_derive": (C.c_int, [_vp, _u32, _u32, C.POINTER(ClipEditDesc), C.POINTER(ClipStats)]),
    "wbx_resample_plan": (C.c_int, [_u32, _u32, C.c_int, C.POINTER(ResampleInfo)]),
    "wbx_resample_frames": (C.c_uint64, [_u32, _u32, C.c_uint64]),
    "wbx_resample_table": (C.c_int, [_u32, _u32, C.c_int, _vp, _sz]),
    "wbx_resample_launch_shape": (C.c_int, [_u32, _u32, C.c_int, C.c_uint64] + [C.POINTER(_u32)] * 4),
    "wbx_clip_resample": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, _u32, C.c_int, C.POINTER(ClipStats)]),
    "wbx_splice_plan": (C.c_int, [_u32, C.c_uint64, C.POINTER(SplicePart), _u32, C.POINTER(SpliceSource), _u32,
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _vp, _sz, _vp, _sz]),
    "wbx_clip_splice": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.POINTER(SplicePart), _u32, C.POINTER(ClipStats)]),
    "wbx_loudness_hop_frames": (_u32, [_u32]),
    "wbx_loudness_hops": (C.c_uint64, [_u32, C.c_uint64]),
    "wbx_loudness_coefficients": (C.c_int, [_u32, _vp]),
    "wbx_true_peak_launch_shape": (C.c_int, [_u32, C.c_uint64] + [C.POINTER(_u32)] * 3),
    "wbx_loudness_gate": (C.c_int, [_u32, C.c_uint64, _u32, _vp, C.POINTER(Loudness)]),
    "wbx_f0_hops": (C.c_uint64, [C.c_uint64, _u32, _u32, _u32]),
    "wbx_f0_check": (C.c_int, [C.c_uint64, _u32, _u32, _u32, _u32, _d, C.c_int, _sz]),
    "wbx_f0_max_hops": (C.c_uint64, []),
    "wbx_f0_launch_terms": (C.c_uint64, []),
    "wbx_f0_launch_hops": (_u32, [_u32, _u32]),
    "wbx_f0_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_f0": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _u32, _d, _vp, _sz, C.POINTER(F0Info)]),
    "wbx_align_check": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, _u32, C.c_int, C.c_int, _sz]),
    "wbx_align_chunks": (_u32, [C.c_uint64]),
    "wbx_align_max_lags": (C.c_uint64, []),
    "wbx_align_chunk_frames": (_u32, []),
    "wbx_align_band_chunks": (_u32, [C.c_uint64]),
    "wbx_align_launches": (_u32, [C.c_uint64, C.c_uint64]),
    "wbx_align_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_align": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, _u32,
                                 C.POINTER(AlignInfo), _vp, _sz]),
    "wbx_spectrum_hops": (C.c_uint64, [C.c_uint64, _u32, _u32]),
    "wbx_spectrum_check": (C.c_int, [C.c_uint64, _u32, _u32, _u32, _u32, C.c_int, _sz]),
    "wbx_spectrum_max_cells": (C.c_uint64, []),
    "wbx_spectrum_launch_terms": (C.c_uint64, []),
    "wbx_spectrum_launch_hops": (_u32, [_u32, _u32]),
    "wbx_spectrum_basis_frames": (C.c_uint64, [_u32, _u32]),
    "wbx_spectrum_basis": (C.c_int, [_u32, _u32, _vp, _vp, C.c_int, _d, _vp]),
    "wbx_spectrum_log_freqs": (C.c_int, [_d, _d, _u32, _vp, C.POINTER(_u32)]),
    "wbx_spectrum_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_spectrum": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _u32, _u32, _vp, _sz, C.POINTER(SpectrumInfo)]),
    "wbx_onset_hops": (C.c_uint64, [C.c_uint64, _u32]),
    "wbx_onset_check": (C.c_int, [C.c_uint64, _u32, _d, _d, _d, _u32, _u32, C.c_int, _sz]),
    "wbx_onset_max_hops": (C.c_uint64, []),
    "wbx_onset_pick": (C.c_int, [_vp, C.c_uint64, _d, _d, _u32, _u32, C.POINTER(C.c_uint64)]),
    "wbx_onset_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_onsets": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _d, _d, _d, _u32, _u32, _vp, _sz, C.POINTER(OnsetInfo)]),
    "wbx_clip_tempo": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _d, _u32, _u32, _u32, _u32, _d, _vp, _sz, C.POINTER(F0Info)]),
    "wbx_clip_loudness": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.POINTER(Loudness), _vp, _sz]),
    "wbx_filter_design": (C.c_int, [_u32, C.c_int, _d, _d, _d, _vp]),
    "wbx_filter_check": (C.c_int, [_vp, _u32]),
    "wbx_filter_transition": (C.c_int, [_vp, _u32, _vp, _sz]),
    "wbx_filter_chunk_frames": (_u32, []),
    "wbx_filter_phase_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_filter": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _u32, C.POINTER(ClipStats)]),
    "wbx_fir_design": (C.c_int, [_u32, C.c_int, _d, _d, _u32, _d, _vp, _sz]),
    "wbx_convolve_frames": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "wbx_convolve_tile_frames": (_u32, []),
    "wbx_convolve_segment_taps": (_u32, []),
    "wbx_convolve_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_convolve": (C.c_int, [_vp, _u32, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                    _d, C.POINTER(ClipStats)]),
    "wbx_limit_ramp": (C.c_int, [_u32, _u32, _u32, _vp, _sz]),
    "wbx_limit_tile_frames": (_u32, []),
    "wbx_limit_segment_terms": (_u32, []),
    "wbx_limit_band_frames": (_u32, []),
    "wbx_limit_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_limit": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, _f, _d, _u32, _u32, _u32, C.POINTER(LimitStats),
                                 C.POINTER(ClipStats)]),
    "wbx_dynamics_table": (C.c_int, [C.c_int, _d, _d, _d, _d, _vp, _sz]),
    "wbx_dynamics_check": (C.c_int, [_vp, C.c_int, C.POINTER(_d)]),
    "wbx_dynamics_lookup": (C.c_int, [_vp, _d, C.POINTER(_d)]),
    "wbx_dynamics_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_dynamics": (C.c_int, [_vp, _u32, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp, _d, _d, _d, _u32,
                                    _u32, _u32, C.POINTER(DynamicsStats), C.POINTER(ClipStats)]),
    "wbx_saturate_table": (C.c_int, [C.c_int, _d, _vp, _sz]),
    "wbx_saturate_check": (C.c_int, [_vp]),
    "wbx_saturate_lookup": (C.c_int, [_vp, _d, C.POINTER(_d)]),
    "wbx_saturate_launch_shape": (C.c_int, [_u32, C.c_int, _u32, C.c_uint64, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32),
                                            C.POINTER(_u32), C.POINTER(_u32)]),
    "wbx_saturate_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_saturate": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, _u32, C.c_int, _vp, _d, _d, C.POINTER(SaturateStats),
                                    C.POINTER(ClipStats)]),
    "wbx_varispeed_plan": (C.c_int, [C.c_int, _u32, _u32, C.POINTER(VarispeedInfo)]),
    "wbx_varispeed_table": (C.c_int, [C.c_int, _u32, _u32, _vp, _vp, _sz]),
    "wbx_varispeed_position": (C.c_int, [_vp, C.c_uint64, _u32, C.c_uint64, C.POINTER(C.c_int64)]),
    "wbx_varispeed_check": (C.c_int, [_vp, C.c_uint64, _u32, C.c_uint64, C.c_uint64, C.c_int, _u32, _u32]),
    "wbx_varispeed_tiles": (C.c_int, [_vp, C.c_uint64, _u32, C.c_uint64, C.c_uint64, C.c_int, _u32, _u32, _vp, C.c_uint64,
                                      C.POINTER(C.c_uint64)]),
    "wbx_varispeed_max_knots": (C.c_uint64, []),
    "wbx_varispeed_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_varispeed": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u32, C.c_int, _u32,
                                     _u32, C.POINTER(ClipStats)]),
    "wbx_denoise_tables": (C.c_int, [_u32, _vp, _vp]),
    "wbx_denoise_threshold": (C.c_int, [_vp, C.c_uint64, _sz, _d, _vp]),
    "wbx_denoise_hops": (C.c_uint64, [C.c_uint64, _u32]),
    "wbx_denoise_profile_hops": (C.c_uint64, [C.c_uint64, _u32]),
    "wbx_denoise_band_hops": (_u32, [_u32, _u32]),
    "wbx_denoise_launches": (C.c_uint64, [C.c_uint64, _u32, _u32]),
    "wbx_denoise_check": (C.c_int, [C.c_uint64, _u32, _u32, _u32, _vp, _u32, _d]),
    "wbx_denoise_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_denoise_profile": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _vp, C.POINTER(C.c_uint64)]),
    "wbx_clip_denoise": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _vp, _d, _u32, C.POINTER(DenoiseStats)]),
    "wbx_stretch_steps": (C.c_uint64, [C.c_uint64, _u32]),
    "wbx_stretch_anchor": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, _u32]),
    "wbx_stretch_window": (C.c_int, [_u32, _vp, _sz]),
    "wbx_stretch_band_steps": (_u32, []),
    "wbx_stretch_launch_terms": (C.c_uint64, []),
    "wbx_stretch_step_terms": (C.c_uint64, []),
    "wbx_stretch_launch_steps": (_u32, [C.c_uint64, _u32, _u32]),
    "wbx_stretch_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_stretch": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _u32, _u32, _vp, _sz, C.POINTER(StretchInfo),
                                   C.POINTER(ClipStats)]),
    "wbx_warp_check": (C.c_int, [C.c_uint64, C.c_uint64, _vp, _u32, _u32, _u32]),
    "wbx_warp_steps": (C.c_uint64, [C.c_uint64, C.c_uint64, _vp, _u32, _u32]),
    "wbx_warp_segments": (C.c_int, [C.c_uint64, C.c_uint64, _vp, _u32, _u32, _vp, _sz]),
    "wbx_warp_max_markers": (_u32, []),
    "wbx_warp_max_steps": (C.c_uint64, []),
    "wbx_warp_launch_segments": (_u32, []),
    "wbx_warp_launches": (C.c_uint64, [C.c_uint64, C.c_uint64, _vp, _u32, _u32, _u32]),
    "wbx_warp_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_warp": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _u32, _u32, _u32, _vp, _sz,
                                C.POINTER(WarpInfo), C.POINTER(ClipStats)]),
    "wbx_pitch_mid_frames": (C.c_uint64, [C.c_uint64, _u32, _u32]),
    "wbx_pitch_max_steps": (_u32, []),
    "wbx_pitch_launch_shape": (C.c_int, [_u32, _u32, C.c_int, C.c_uint64] + [C.POINTER(_u32)] * 4),
    "wbx_pitch_ms": (C.c_int, [_vp, _vp]),
    "wbx_clip_pitch": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _u32, _u32, C.c_int, _u32, _u32, _vp, _sz,
                                 C.POINTER(PitchInfo), C.POINTER(ClipStats)]),
    "wbx_mip_levels": (_u32, [C.c_uint64]),
    "wbx_mip_data_count": (C.c_uint64, [C.c_uint64, _u32]),
    "wbx_clip_build_mipmaps": (C.c_int, [_vp, _u32, C.c_int]),
    "wbx_clip_fetch_mipmap": (C.c_int, [_vp, _u32, _u32, _vp]),
    "wbx_clip_mipmap_device": (C.c_int, [_vp, _u32, _u32, _pp, C.POINTER(C.c_uint64)]),
    "wbx_render_order": (C.c_int, [_vp, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int)]),
    "wbx_device_info": (C.c_int, [_vp, C.c_char_p, _sz, C.c_char_p, _sz]),
    "wbx_set_routing": (C.c_int, [_vp, _u32, C.POINTER(_i32), _u32]),
    "wbx_submit": (C.c_int, [_vp, _u32, _u32, C.POINTER(Segment), C.POINTER(_u32), C.POINTER(_f)]),
    "wbx_fetch": (C.c_int, [_vp, _fpp, C.POINTER(_f), C.POINTER(_f)]),
    "wbx_fetch_interleaved": (C.c_int, [_vp, C.c_int, _vp]),
    "wbx_set_master_format": (C.c_int, [_vp, C.c_int]),
    "wbx_sync": (C.c_int, [_vp]),
    "wbx_render_status": (C.c_int, [_vp]),
    "wbx_master_ready": (C.c_int, [_vp, _vp]),
    "wbx_partial_master": (C.c_int, [_vp, _pp, C.POINTER(_sz)]),
    "wbx_finalize_master": (C.c_int, [_vp, _vp, _u32, C.c_int, _vp]),
    "wbx_finalize_master_into": (C.c_int, [_vp, _vp, _vp, _u32, C.c_int, _vp]),
    "wbx_set_clamp": (C.c_int, [_vp, C.c_int]),
    "wbx_set_master_target": (C.c_int, [_vp, _vp]),
    "wbx_set_master_init": (C.c_int, [_vp, _vp]),
    "wbx_shard_tracks": (None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "wbx_dist_new_id": (C.c_int, [_vp]),
    "wbx_dist_init": (C.c_int, [_vp, _vp, _u32, _u32, C.c_int]),
    "wbx_dist_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int)]),
    "wbx_dist_result_rank": (C.c_int, [_vp, C.POINTER(_u32)]),
    "wbx_dist_exchange": (C.c_int, [_vp, _vp]),
    "wbx_dist_exchange_time": (C.c_int, [_vp, C.POINTER(_d), C.POINTER(C.c_uint64)]),
    "wbx_dist_allgather": (C.c_int, [_vp, _vp, _vp, _sz]),
    "wbx_dist_sync": (C.c_int, [_vp]),
    "wbx_dist_barrier": (C.c_int, [_vp]),
    "wbx_dist_max": (C.c_int, [_vp, C.POINTER(_d)]),
    "wbx_dist_shutdown": (C.c_int, [_vp]),
    "wbx_pace": (C.c_int, [_vp, _u32]),
    "wbx_host_alloc": (C.c_int, [_sz, _pp]),
    "wbx_host_free": (C.c_int, [_vp]),
    "wbx_kernel_time": (C.c_int, [_vp, C.c_int, C.POINTER(_d), C.POINTER(C.c_uint64)]),
    "wbx_kernel_name": (C.c_char_p, [_vp]),
    "wbx_render_uniform_speed": (C.c_double, [_vp]),
    "wbx_xcd_count": (_u32, [_vp]),
    "wbx_tail_time": (C.c_int, [_vp, C.POINTER(_d)]),
    "wbx_gap_time": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "wbx_engine_create": (C.c_int, [C.POINTER(Config), _pp]),
    "wbx_engine_destroy": (None, [_vp]),
    "wbx_engine_set_audio_channel_config": (C.c_int, [_vp, _u32, _u32, _u32]),
    "wbx_engine_last_error": (C.c_char_p, [_vp]),
    "wbx_engine_ctx": (_vp, [_vp]),
    "wbx_engine_set_bpm": (C.c_int, [_vp, _d]),
    "wbx_engine_set_playhead_position": (C.c_int, [_vp, _d]),
    "wbx_engine_add_track": (C.c_int, [_vp, C.POINTER(_u32)]),
    "wbx_engine_set_buses": (C.c_int, [_vp, _u32]),
    "wbx_track_set_volume": (C.c_int, [_vp, _u32, _f]),
    "wbx_track_set_pan": (C.c_int, [_vp, _u32, _f]),
    "wbx_track_set_mute": (C.c_int, [_vp, _u32, C.c_int]),
    "wbx_track_set_bus": (C.c_int, [_vp, _u32, _i32]),
    "wbx_engine_add_plugin_to_track": (C.c_int, [_vp, _u32, _vp]),
    "wbx_engine_delete_plugin_from_track": (C.c_int, [_vp, _u32]),
    "wbx_track_get_plugin": (C.c_int, [_vp, _u32, _pp]),
    "wbx_engine_delete_track": (C.c_int, [_vp, _u32]),
    "wbx_engine_clear_all": (C.c_int, [_vp]),
    "wbx_engine_move_track": (C.c_int, [_vp, _u32, _u32]),
    "wbx_engine_solo_track": (C.c_int, [_vp, _u32]),
    "wbx_engine_add_sample": (C.c_int, [_vp, C.c_int, _u32, _u32, C.c_uint64, _pp, C.POINTER(_u32)]),
    "wbx_engine_add_sample_interleaved": (C.c_int, [_vp, C.c_int, _u32, _u32, C.c_uint64, _vp, C.POINTER(_u32)]),
    "wbx_engine_add_sample_synth": (C.c_int, [_vp, C.c_int, _u32, _u32, C.c_uint64, C.c_uint64, _u32, _f,
                                              C.POINTER(_u32)]),
    "wbx_engine_delete_sample": (C.c_int, [_vp, _u32]),
    "wbx_engine_add_audio_clip": (C.c_int, [_vp, _u32, _d, _d, _d, _u32, _d, _f]),
    "wbx_engine_move_clip": (C.c_int, [_vp, _u32, _u32, _d]),
    "wbx_engine_resize_clip": (C.c_int, [_vp, _u32, _u32, _d, _d, _d, C.c_int, C.c_int, C.c_int]),
    "wbx_engine_delete_clip": (C.c_int, [_vp, _u32, _u32]),
    "wbx_engine_delete_region": (C.c_int, [_vp, _u32, _d, _d]),
    "wbx_engine_set_clip_gain": (C.c_int, [_vp, _u32, _u32, _f]),
    "wbx_engine_clip_count": (C.c_int, [_vp, _u32, C.POINTER(_u32)]),
    "wbx_engine_get_clip": (C.c_int, [_vp, _u32, _u32, C.POINTER(ClipInfo)]),
    "wbx_calc_move_clip": (None, [_d] * 4 + [C.POINTER(_d)] * 2),
    "wbx_calc_resize_clip": (None, [_d] * 11 + [C.c_int] * 4 + [C.POINTER(_d)] * 4),
    "wbx_calc_clip_shift": (_d, [_d] * 4),
    "wbx_shift_clip_content": (_d, [_d] * 5),
    "wbx_engine_play": (C.c_int, [_vp]),
    "wbx_engine_stop": (C.c_int, [_vp]),
    "wbx_engine_process": (C.c_int, [_vp, _fpp]),
    "wbx_engine_process_interleaved": (C.c_int, [_vp, C.c_int, _vp]),
    "wbx_engine_process_in": (C.c_int, [_vp, _fpp, _u32, _fpp]),
    "wbx_engine_process_interleaved_in": (C.c_int, [_vp, _fpp, _u32, C.c_int, _vp]),
    "wbx_engine_render": (C.c_int, [_vp, _u32]),
    "wbx_engine_bounce": (C.c_int, [_vp, _d, _d, C.POINTER(BounceSource), _u32, C.POINTER(_u32), C.POINTER(C.c_uint64)]),
    "wbx_engine_export_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_int, _u32, _vp, C.POINTER(ExportStats)]),
    "wbx_engine_measure_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.POINTER(ClipStats)]),
    "wbx_engine_derive_sample": (C.c_int, [_vp, _u32, C.POINTER(ClipEditDesc), C.POINTER(_u32)]),
    "wbx_engine_normalize_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _f, C.POINTER(_u32), C.POINTER(_f)]),
    "wbx_engine_resample_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.c_int, C.POINTER(_u32)]),
    "wbx_engine_filter_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _u32, C.POINTER(_u32)]),
    "wbx_engine_convolve_sample": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                             C.c_uint64, _d, C.POINTER(_u32), C.POINTER(ClipStats)]),
    "wbx_engine_limit_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _f, _d, _u32, _u32, _u32, C.POINTER(_u32),
                                          C.POINTER(LimitStats), C.POINTER(ClipStats)]),
    "wbx_engine_dynamics_sample": (C.c_int, [_vp, _u32, _u32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp, _d, _d, _d, _u32,
                                             _u32, _u32, C.POINTER(_u32), C.POINTER(DynamicsStats), C.POINTER(ClipStats)]),
    "wbx_engine_saturate_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.c_int, _vp, _d, _d, C.POINTER(_u32),
                                             C.POINTER(SaturateStats), C.POINTER(ClipStats)]),
    "wbx_engine_varispeed_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u32, C.c_int, _u32,
                                              _u32, C.POINTER(_u32), C.POINTER(ClipStats)]),
    "wbx_engine_denoise_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _vp, _d, C.POINTER(_u32),
                                            C.POINTER(DenoiseStats)]),
    "wbx_engine_denoise_profile_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _vp, C.POINTER(C.c_uint64)]),
    "wbx_engine_stretch_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _u32, _u32, C.POINTER(StretchInfo),
                                            C.POINTER(_u32)]),
    "wbx_engine_warp_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _u32, _u32, _u32, C.POINTER(WarpInfo),
                                         C.POINTER(_u32)]),
    "wbx_engine_pitch_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, C.c_uint64, _u32, _u32, C.c_int, _u32, _u32,
                                          C.POINTER(PitchInfo), C.POINTER(_u32)]),
    "wbx_engine_f0_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _u32, _d, _vp, _sz, C.POINTER(F0Info)]),
    "wbx_engine_spectrum_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _u32, _u32, _u32, _u32, _vp, _sz,
                                             C.POINTER(SpectrumInfo)]),
    "wbx_engine_align_samples": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64,
                                           _u32, C.POINTER(AlignInfo), _vp, _sz]),
    "wbx_engine_onsets_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _d, _d, _d, _u32, _u32, _vp, _sz,
                                           C.POINTER(OnsetInfo)]),
    "wbx_engine_tempo_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, _d, _u32, _u32, _u32, _u32, _d, _vp, _sz,
                                          C.POINTER(F0Info)]),
    "wbx_engine_loudness_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _u32, C.POINTER(Loudness), _vp, _sz]),
    "wbx_engine_normalize_loudness_sample": (C.c_int, [_vp, _u32, C.c_uint64, C.c_uint64, _d, _f, C.POINTER(_u32),
                                                       C.POINTER(_f)]),
    "wbx_engine_splice_samples": (C.c_int, [_vp, _u32, C.c_uint64, C.POINTER(SplicePart), _u32, C.POINTER(_u32)]),
    "wbx_clip_pool_limit": (C.c_int, [_vp, C.c_uint64]),
    "wbx_engine_set_input_channels": (C.c_int, [_vp, _u32]),
    "wbx_track_set_input": (C.c_int, [_vp, _u32, C.c_int, _u32, C.c_int]),
    "wbx_engine_arm_track_recording": (C.c_int, [_vp, _u32, C.c_int]),
    "wbx_engine_record": (C.c_int, [_vp]),
    "wbx_engine_stop_record": (C.c_int, [_vp]),
    "wbx_engine_is_recording": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "wbx_engine_record_info": (C.c_int, [_vp, _u32, C.POINTER(RecordInfo)]),
    "wbx_engine_set_record_chunk": (C.c_int, [_vp, _u32, _u32]),
    "wbx_engine_transport": (C.c_int, [_vp, C.POINTER(_d), C.POINTER(_d), C.POINTER(C.c_int)]),
    "wbx_engine_levels": (C.c_int, [_vp, C.POINTER(_f), _u32]),
    "wbx_engine_thread_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _u32]),
    "wbx_engine_sequencer_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "wbx_engine_callback_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "wbx_engine_perf_usage": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wbx_calc_perf_update": (C.c_double, [C.c_double] * 3),
    "wbx_calc_perf_usage": (C.c_double, [C.c_double]),
    "wbx_calc_buffer_period_ms": (C.c_double, [_u32, _u32]),
    "wbx_engine_fetch_plan": (C.c_int, [_vp, C.POINTER(PlanRecord), _sz, C.POINTER(_sz)]),
}

_lib = None


def lib_path() -> str:
    return _LIB


def lib() -> C.CDLL:
    """The HIP library.  No fallback: a missing build is an error, not a slower path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise ImportError(f"{_LIB} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); whitebox_amd has no CPU implementation")
        L = C.CDLL(_LIB)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib
