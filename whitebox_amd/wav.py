"""RIFF/WAVE writer for exported samples — a convenience of the Python mirror, not of libwbx.so.

The C library ends at interleaved device-format samples in host memory (wbx_clip_export, wbx_engine_export_sample);
this file puts a 44-byte (PCM) or 58-byte (IEEE float) header in front of them and streams a sample into the file in
calls of bounded size, so that the host never holds more than one piece of a long take.

    from whitebox_amd import wav
    wav.write_sample(engine, sample, "take.wav", bits=24, frames=n)          # PCM 16 / 24 / 32
    wav.write_sample(engine, sample, "stem.wav", bits=32, float32=True, frames=n)
"""
from __future__ import annotations

import struct
from typing import BinaryIO, Optional

WAVE_FORMAT_PCM = 1
WAVE_FORMAT_IEEE_FLOAT = 3

# (bits, float) -> export format of whitebox_amd ("i24": true packed interleave)
EXPORT_FORMAT = {(16, False): "i16", (24, False): "i24", (32, False): "i32", (32, True): "f32"}


def header(channels: int, sample_rate: int, bits: int, n_frames: int, float32: bool = False) -> bytes:
    """The bytes in front of the audio: RIFF, "fmt " (and, for IEEE float, the cbSize field and the "fact" chunk the
    format asks of non-PCM data), "data".  PCM 16, 24, 32 bit; IEEE float 32 bit."""
    if (bits, bool(float32)) not in EXPORT_FORMAT:
        raise ValueError(f"wav: {bits}-bit {'float' if float32 else 'PCM'} is not supported")
    if channels < 1 or sample_rate < 1 or n_frames < 0:
        raise ValueError("wav: channels, sample_rate and n_frames must be positive")
    block_align = channels * bits // 8
    data_bytes = n_frames * block_align
    pad = data_bytes & 1   # chunks are word aligned
    if data_bytes + pad + 64 > 0xFFFFFFFF:
        raise ValueError("wav: more than 4 GiB of audio does not fit a RIFF file")
    tag = WAVE_FORMAT_IEEE_FLOAT if float32 else WAVE_FORMAT_PCM
    fmt = struct.pack("<HHIIHH", tag, channels, sample_rate, sample_rate * block_align, block_align, bits)
    extra = b""
    if float32:
        fmt += struct.pack("<H", 0)                                   # cbSize
        extra = b"fact" + struct.pack("<II", 4, n_frames)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + b"data" + struct.pack("<I", data_bytes)
    return b"RIFF" + struct.pack("<I", len(body) + data_bytes + pad) + body


def write_bytes(f: BinaryIO, channels: int, sample_rate: int, bits: int, payload: bytes, float32: bool = False) -> None:
    """header + an interleaved payload that is already in memory"""
    block_align = channels * bits // 8
    if len(payload) % block_align:
        raise ValueError("wav: the payload is not a whole number of frames")
    f.write(header(channels, sample_rate, bits, len(payload) // block_align, float32))
    f.write(payload)
    if len(payload) & 1:
        f.write(b"\0")


def write_sample(engine, sample: int, path: str, bits: int = 16, float32: bool = False, frames: Optional[int] = None,
                 channels: Optional[int] = None, clamp: bool = True, piece_frames: int = 1 << 20) -> dict:
    """Stream an engine sample into a WAVE file: the header, then engine.export_sample calls of at most `piece_frames`
    frames each.  Returns the statistics of the whole sample ({"peak", "over", "nans"} per channel)."""
    fmt = EXPORT_FORMAT.get((bits, bool(float32)))
    if fmt is None:
        raise ValueError(f"wav: {bits}-bit {'float' if float32 else 'PCM'} is not supported")
    known = getattr(engine, "_sample_shape", {}).get(sample, (None, engine.num_output_channels))
    frames = known[0] if frames is None else frames
    channels = known[1] if channels is None else channels
    if frames is None:
        raise ValueError("wav: give frames, the sample's length")
    total = {"peak": [0.0] * channels, "over": [0] * channels, "nans": [0] * channels}
    with open(path, "wb") as f:
        # the sample's own rate where the engine object knows it (an imported file, a converted sample), else the session's
        rate = getattr(engine, "_sample_rate", {}).get(sample, engine.audio_sample_rate)
        f.write(header(channels, rate, bits, frames, float32))
        done = 0
        while done < frames:
            n = min(piece_frames, frames - done)
            data, st = engine.export_sample(sample, fmt, done, n, clamp=clamp, channels=channels)
            f.write(data.tobytes())
            for c in range(channels):
                total["peak"][c] = max(total["peak"][c], st["peak"][c])
                total["over"][c] += st["over"][c]
                total["nans"][c] += st["nans"][c]
            done += n
        if (frames * channels * bits // 8) & 1:
            f.write(b"\0")
    return total
