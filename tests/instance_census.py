"""Every compiled instance of the library's hot-path kernel templates, and how a session reaches it.

tests/test_instance_census.py holds this table against the symbol table of whitebox_amd/libwbx.so (a missing or a stale entry
fails) and, on a GPU, renders each entry's session: the launched instance must be the entry, and master, per-track peaks,
bus sums, stream-call log and transport must be what the oracle (one group) or tests/grouped_order.py (several) gives.

A recipe is built where kernels go wrong: N leaves a partial last pipeline batch and unequal groups, the clips hold NaN,
+-Inf, -0.0, subnormals, values the gains push past +-1 and the integer extremes, one track is muted, one hard-panned, one
has no clips; `cut` sessions put clip boundaries at frames 1, F/2+1 and F-1 of their blocks.

`env`: per-context switches (read by wbx_create: set before the engine is built).  `proc_env`: process-wide statics (read
once per process: the entry runs in a child process of its own).
"""
import dataclasses
from typing import Dict, Optional, Tuple


@dataclasses.dataclass(frozen=True)
class Entry:
    name: str                      # as nm -C and wbx_kernel_name spell it
    fmt: str = "f32"               # storage format of the clips
    fmts: Tuple[str, ...] = ()     # ... or of track t's clip: fmts[t % len(fmts)] (every format the family streams)
    src_rate: int = 48000          # their sample rate (48 kHz: the session rate)
    block: int = 512
    channels: int = 2
    n_tracks: int = 37
    n_blocks: int = 8              # K: blocks per render (callback: blocks rendered one per call)
    cut: bool = False              # tracks cut into clips, boundaries inside blocks (masked rows)
    group_size: int = 16           # 0: the library's choice
    n_buses: int = 0
    callback: bool = False         # max_blocks = 1 engine, one Engine::process per block
    master_formats: Tuple[str, ...] = ()   # renders again with the master in these interleaved device formats
    mix: str = ""                  # sum entries: the mix instance the session takes
    env: Dict[str, str] = dataclasses.field(default_factory=dict)
    proc_env: Dict[str, str] = dataclasses.field(default_factory=dict)
    shared_samples: int = 0        # > 0: the tracks play that many samples (long renders: the clip data stays small)
    note: str = ""


def _e(name, **kw):
    return Entry(name=name, **kw)


M = "wbx::mix_kernel<"
X = "wbx::mix_kernel_x<"
CB = "wbx::callback_kernel<"
S = "wbx::sum_kernel<"

CENSUS = [
    # ---- family 0: fp32 rows, integer PCM at unity speed
    _e(M + "4, true, 3, 0, 1, 1, 1, 256>", note="fp32 at the session rate, one clip per track"),
    _e(M + "2, true, 4, 0, 1, 1, 1, 256>", src_rate=44100, note="fp32 resampled, one clip per track"),
    _e(M + "8, true, 2, 0, 1, 1, 1, 256>", fmts=("f32", "i16", "i24", "i32"), env={"WBX_MIX_VARIANT": "82"}, note="A/B variant 82"),
    _e(M + "2, true, 3, 0, 1, 1, 2, 128>", src_rate=44100, cut=True, note="fp32 resampled, cut: both channels per lane"),
    _e(M + "1, true, 3, 0, 1, 1, 2, 128>", src_rate=44100, n_tracks=131, n_blocks=2048, group_size=0, shared_samples=4,
       env={"WBX_EXACT_MIN_BLOCKS": "4"}, note="c3 in chained renders of >= 2048 blocks (mix_long_chained_window_render)"),
    _e(M + "4, true, 2, 0, 1, 1, 2, 128>", fmts=("i16", "i24", "i32", "f32"), env={"WBX_MIX_VARIANT": "1042"}, note="A/B variant 1042"),
    _e(M + "2, true, 3, 0, 1, 1, 2, 256>", fmts=("i16", "i24", "i32", "f32"), block=1024, cut=True, note="1024-frame stereo, integer PCM"),
    _e(M + "2, true, 3, 0, 1, 1, 2, 64>", src_rate=44100, block=256, cut=True, note="256-frame stereo, cut: one wave = one block"),
    _e(M + "2, true, 3, 0, 1, 2, 1, 64>", block=128, fmts=("f32", "i16", "i24", "i32"), cut=True, n_blocks=5, note="128-frame stereo, cut, < 8 blocks: one wave"),
    _e(M + "2, true, 3, 0, 1, 1, 1, 128>", block=512, fmts=("f32", "i16", "i24", "i32"), channels=1, cut=True, n_blocks=5, note="512-frame mono, cut"),
    _e(M + "2, true, 3, 0, 1, 1, 1, 64>", block=256, fmts=("f32", "i16", "i24", "i32"), channels=1, cut=True, n_blocks=5, note="256-frame mono, cut"),
    _e(M + "2, true, 4, 0, 4, 2, 1, 256>", block=128, fmts=("f32", "i16", "i24", "i32"), n_blocks=9, note="128-frame stereo: four blocks per workgroup"),
    _e(M + "2, true, 4, 0, 2, 1, 1, 256>", src_rate=44100, block=256, n_blocks=9, note="256-frame stereo: two blocks per workgroup"),
    _e(M + "2, true, 4, 0, 4, 1, 1, 256>", block=256, fmts=("f32", "i16", "i24", "i32"), channels=1, n_blocks=9, note="256-frame mono: four blocks per workgroup"),
    _e(X + "2, 4, 0, 4, 2, 1>", block=128, fmts=("f32", "i16", "i24", "i32"), cut=True, n_blocks=11, note="128-frame stereo, cut, >= 8 blocks: packed masked rows"),
    _e(X + "2, 4, 0, 2, 1, 1>", block=512, fmts=("f32", "i16", "i24", "i32"), channels=1, cut=True, n_blocks=9, env={"WBX_PACKED_X": "1"}),
    _e(X + "2, 4, 0, 4, 1, 1>", block=256, fmts=("f32", "i16", "i24", "i32"), channels=1, cut=True, n_blocks=9, env={"WBX_PACKED_X": "1"}),
    # ---- family 1, everything: per-frame taps (fp32 played faster than recorded), window rows of every format
    _e(M + "2, true, 4, 1, 1, 1, 1, 256>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), note="per-frame taps"),
    _e(M + "2, false, 1, 1, 1, 1, 1, 256>", block=96, fmts=("f32", "i16", "i24", "i32"), n_blocks=3, env={"WBX_RAGGED": "0"},
       note="a block shape no lean instance has, without the rounding up to one (WBX_RAGGED=0)"),
    _e(M + "2, true, 3, 1, 1, 2, 1, 64>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=128, cut=True, n_blocks=5),
    _e(M + "2, true, 3, 1, 1, 1, 1, 128>", fmts=("i24", "i16", "i32", "f32"), src_rate=44100, block=256, cut=True),
    _e(M + "2, true, 3, 1, 1, 1, 1, 64>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=256, channels=1, cut=True, n_blocks=5),
    _e(M + "2, true, 4, 1, 4, 2, 1, 256>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=128, n_blocks=9),
    _e(M + "2, true, 4, 1, 2, 1, 1, 256>", fmts=("i24", "i16", "i32", "f32"), src_rate=44100, block=256, n_blocks=9),
    _e(M + "2, true, 4, 1, 4, 1, 1, 256>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=256, channels=1, n_blocks=9),
    _e(X + "2, 4, 1, 4, 2, 1>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=128, cut=True, n_blocks=11),
    _e(X + "2, 4, 1, 2, 1, 1>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=512, channels=1, cut=True, n_blocks=9, env={"WBX_PACKED_X": "1"}),
    _e(X + "2, 4, 1, 4, 1, 1>", src_rate=96000, fmts=("f32", "i16", "i24", "i32"), block=256, channels=1, cut=True, n_blocks=9, env={"WBX_PACKED_X": "1"}),
    # ---- family 2: 16-bit PCM only, resampled at speeds up to 0.999
    _e(M + "2, true, 4, 2, 1, 1, 1, 256>", fmt="i16", src_rate=44100, block=1024, channels=1, note="one channel per wave"),
    _e(M + "2, true, 3, 2, 1, 1, 2, 128>", fmt="i16", src_rate=44100),
    _e(M + "2, true, 3, 2, 1, 1, 2, 64>", fmt="i16", src_rate=44100, block=256, cut=True),
    _e(M + "2, true, 3, 2, 1, 1, 2, 256>", fmt="i16", src_rate=44100, block=1024, cut=True),
    _e(M + "4, true, 2, 2, 1, 1, 2, 128>", fmt="i16", src_rate=44100, env={"WBX_MIX_VARIANT": "1042"}),
    _e(M + "1, true, 3, 2, 1, 1, 2, 128>", fmt="i16", src_rate=44100, env={"WBX_MIX_VARIANT": "1013"}),
    # ---- family 3: family 1 without the per-frame taps
    _e(M + "1, true, 3, 3, 1, 1, 2, 128>", fmts=("i24", "i16", "i32", "f32"), src_rate=44100),
    _e(M + "2, true, 3, 3, 1, 1, 2, 128>", fmts=("i24", "i16", "i32", "f32"), src_rate=44100, env={"WBX_MIX_VARIANT": "1022"}),
    # ---- the one-launch callback (sequencer + mix + spread sum); each runs at 128-, 256- and 512-frame stereo
    _e(CB + "2, 0>", callback=True, fmts=("f32", "i16", "i24", "i32"), n_tracks=71, n_blocks=3, group_size=0, note="fp32"),
    _e(CB + "2, 1>", callback=True, fmts=("i24", "i16", "i32", "f32"), src_rate=44100, n_tracks=71, n_blocks=3, group_size=0, note="24-bit resampled"),
    _e(CB + "2, 2>", callback=True, fmt="i16", src_rate=44100, n_tracks=71, n_blocks=3, group_size=0, note="16-bit resampled"),
    _e(CB + "4, 0>", callback=True, fmts=("f32", "i16", "i24", "i32"), n_tracks=71, n_blocks=3, group_size=0, proc_env={"WBX_CB_U": "4"}),
    _e(CB + "8, 0>", callback=True, fmts=("f32", "i16", "i24", "i32"), n_tracks=71, n_blocks=3, group_size=0, proc_env={"WBX_CB_U": "8"}),
    # ---- the sum (no name API: launch_sum's condition is asserted instead)
    _e(S + "16, false, false>", src_rate=44100, mix=M + "2, true, 4, 0, 1, 1, 1, 256>", note="K >= 8 or <= 16 groups, no buses, planar"),
    _e(S + "32, false, false>", src_rate=44100, n_tracks=150, group_size=8, n_blocks=4, mix=M + "2, true, 4, 0, 1, 1, 1, 256>",
       note="K < 8 and > 16 groups"),
    _e(S + "16, true, false>", src_rate=44100, n_tracks=45, n_buses=3, mix=M + "2, true, 4, 0, 1, 1, 1, 256>", note="sub-buses, planar"),
    _e(S + "16, false, true>", src_rate=44100, master_formats=("i16", "i24", "i24_x8", "i32", "f32"), mix=M + "2, true, 4, 0, 1, 1, 1, 256>",
       note="interleaved device formats"),
    _e(S + "16, true, true>", src_rate=44100, n_tracks=45, n_buses=3, master_formats=("i16", "i24", "i24_x8", "i32", "f32"),
       mix=M + "2, true, 4, 0, 1, 1, 1, 256>", note="sub-buses, interleaved"),
]

# template __global__ functions of the library that are not part of the census, and why
EXCLUDED = {
    "wbx::deinterleave_kernel<": "clip ingest (wbx_media.hip): checked against the reference's Sample::load_file by test_gpu_media.py",
    "wbx::mip_tile_kernel<": "waveform mip-maps (wbx_media.hip): checked against the reference's summariser by test_gpu_media.py",
    "wbx::mip_upper_kernel<": "waveform mip-maps, upper levels (wbx_media.hip): test_gpu_media.py",
}

KINDS = (M, X, CB, S)


# ---- an entry's session
def _salted(spec_cls):
    class Salted(spec_cls):
        """clip audio with NaN, +-Inf, -0.0, a subnormal and values past +-1 (fp32), the integer extremes (PCM)"""
        def sample_data(self, i):
            import numpy as np
            out = super().sample_data(i)
            fmt = self.samples[i].fmt
            for c, a in enumerate(out):
                n = len(a) - 16
                if n < 8:
                    continue
                if fmt == "f32":
                    vals = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, 3.0, -2.5], np.float32)
                    vals = vals if i % 5 == 1 else vals[3:]          # (non-finite values on a few tracks only)
                else:
                    lo = {"i16": -32768, "i24": -(1 << 23), "i32": -(1 << 31)}[fmt]
                    vals = np.array([lo, -lo - 1, lo], a.dtype)
                idx = (np.arange(0, n, 211) + 13 * i + 3 * c) % n
                a[idx] = vals[(np.arange(len(idx)) + i) % len(vals)]
            return out
    return Salted


def build_spec(entry: Entry, n_blocks: Optional[int] = None, salt: bool = True):
    """the entry's session (n_blocks: how many blocks its clips must cover, default the entry's own)"""
    import numpy as np
    from whitebox_amd import synth

    K = n_blocks or entry.n_blocks
    spec = synth.make_session("census", entry.n_tracks, n_blocks=K, block=entry.block, src_rate=entry.src_rate, fmt=entry.fmt,
                              n_buses=entry.n_buses, seed=0xCE45 + entry.block + entry.src_rate)
    spec.channels = entry.channels
    N, F = entry.n_tracks, entry.block
    if entry.fmts:
        for t, smp in enumerate(spec.samples):
            smp.fmt = entry.fmts[t % len(entry.fmts)]
            smp.amp = synth.default_amp(N) if smp.fmt == "f32" else 1.0
    beat_frames = spec.sample_rate * 60.0 / spec.bpm
    ratio = entry.src_rate / spec.sample_rate
    if entry.cut:
        # boundaries at frames 1, F/2 + 1 and F - 1 of their blocks; clips of 1-2 blocks, each reading on where the last one
        # stopped; the one that ends at frame 1 ends one frame into its block
        spec.clips = []
        offs = (1, F // 2 + 1, F - 1)
        for t in range(N):
            pos, k = 0.0, 0
            while pos < (K + 1) * F:
                end = (int(pos) // F + 1 + (t + k) % 2) * F + offs[(t + k) % 3]
                spec.clips.append(synth.ClipSpec(t, pos / beat_frames, end / beat_frames, start_offset=float(pos * ratio),
                                                 gain=[1.0, 0.5, 1.7][k % 3]))
                pos, k = float(end), k + 1
    if entry.shared_samples:    # a few samples, each track reading its own stretch of one
        for s in spec.samples:
            s.frames += 1024
        spec.samples = spec.samples[:entry.shared_samples]
        for c in spec.clips:
            c.sample, c.start_offset = c.track % entry.shared_samples, float((c.track * 37) % 1000)
    for t in range(N):          # integer clips are full scale: the session level goes into the faders, as bench.py does
        if spec.samples[t % len(spec.samples)].fmt != "f32":
            spec.volumes_db[t] += 20.0 * float(np.log10(0.25 / np.sqrt(N)))
    spec.volumes_db[1] = 6.0                     # pushes its samples past +-1
    spec.mutes[2] = True
    spec.pans[3], spec.pans[4 % N] = -1.0, 1.0   # hard pans: exact-zero gains
    spec.clips = [c for c in spec.clips if c.track != 5]   # a track with no clips
    if entry.n_buses:                            # buses with direct tracks between their members
        spec.track_bus = [t % (entry.n_buses + 1) - 1 for t in range(N)]
    if salt:
        cls = _salted(type(spec))
        spec = cls(**{f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)})
    return spec
