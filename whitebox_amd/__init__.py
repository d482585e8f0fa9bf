"""whitebox_amd — MI355X-native (gfx950) implementation of the whitebox per-block multitrack mix.

The product is the C-ABI shared library `libwbx.so` (include/wbx.h; sources in whitebox_amd/csrc);
this package is the thin Python binding used by tests and bench.py.  It never computes audio on the
CPU: `whitebox_amd.lib()` raises if the HIP library is missing, and engines cannot be created
without a gfx950 device.
"""
from ._ffi import WbxError, lib, lib_path  # noqa: F401
from .engine import AudioBuffer, Engine, MixContext, Track, edit_desc  # noqa: F401
from .engine import resample_frames, resample_plan, resample_table  # noqa: F401
from .engine import clipfx_pass_frames, pitch_launch_shape, resample_launch_shape, true_peak_launch_shape  # noqa: F401
from .engine import loudness_coefficients, loudness_gate, loudness_hops  # noqa: F401
from .engine import filter_design, filter_transition  # noqa: F401
from .engine import convolve_frames, fir_design  # noqa: F401
from .engine import limit_frames, limit_ramp  # noqa: F401
from .engine import dynamics_check, dynamics_lookup, dynamics_table  # noqa: F401
from .engine import saturate_check, saturate_launch_shape, saturate_lookup, saturate_table  # noqa: F401
from .engine import varispeed_check, varispeed_knots, varispeed_plan, varispeed_position, varispeed_table, varispeed_tiles  # noqa: F401
from .engine import denoise_band_hops, denoise_hops, denoise_tables, denoise_threshold  # noqa: F401
from .engine import stretch_anchor, stretch_steps, stretch_window  # noqa: F401
from .engine import warp_check, warp_launches, warp_segments, warp_steps  # noqa: F401
from .engine import pitch_mid_frames, pitch_ratio  # noqa: F401
from .engine import F0_DTYPE, f0_hops  # noqa: F401
from .engine import ALIGN_CURVE_DTYPE, ALIGN_EITHER_POLARITY, align_check, align_chunks  # noqa: F401
from .engine import SPECTRUM_MID, spectrum_basis, spectrum_hops, spectrum_log_freqs  # noqa: F401
from .engine import ONSET_DTYPE, onset_hops  # noqa: F401
from .engine import splice_part, splice_plan  # noqa: F401
