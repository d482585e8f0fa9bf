"""Host model of wbx_clip_splice (include/wbx.h "Splicing clips"): numpy, the header's rule operation for operation.  A part's
value is tests/clipfx_model.py's derive of its edit; an output frame walks the parts that cover it in LIST order — the first
assigns, every later one is one float32 addition; a frame no part covers is +0.0; a NaN result is the quiet NaN 0x7FC00000.
There is no libm call and no tolerance: the device must reproduce every bit."""
from collections import namedtuple

import numpy as np

import clipfx_model as M

F32 = np.float32
TILE = 512

Part = namedtuple("Part", "src first n at reverse mode gain fade_in fade_out shape_in shape_out",
                  defaults=(0, False, M.KEEP, 1.0, 0, 0, M.LINEAR, M.LINEAR))


def part_value(sources, p):
    """[C'] float32 arrays of p.n frames: what wbx_clip_derive would store for the part's edit"""
    return M.derive(sources[p.src], p.first, p.n, bool(p.reverse), p.mode, p.gain, p.fade_in, p.fade_out, p.shape_in, p.shape_out)


def splice(sources, channels, n_frames, parts):
    """sources: {clip id: [C] float32 arrays of the whole clip}; parts: Part tuples -> [channels] float32 arrays of n_frames"""
    out = [np.zeros(n_frames, dtype=F32) for _ in range(channels)]
    have = np.zeros(n_frames, dtype=bool)
    with np.errstate(all="ignore"):
        for p in parts:
            v = part_value(sources, p)
            assert len(v) == channels and 0 < p.n and p.at + p.n <= n_frames
            seg = slice(p.at, p.at + p.n)
            for c in range(channels):
                out[c][seg] = np.where(have[seg], (out[c][seg] + v[c]).astype(F32), v[c])   # assign, or ONE fp32 addition
            have[seg] = True
    for y in out:
        y.view(np.uint32)[np.isnan(y)] = M.CANON_NAN
    return out


def tile_table(n_frames, parts):
    """the kernel's table by brute force: for every tile of 512 output frames the indices of the parts that touch it,
    ascending -> (tile_off [n_tiles + 1], tile_parts)"""
    n_tiles = (n_frames + TILE - 1) // TILE
    off, ent = [0], []
    for t in range(n_tiles):
        lo, hi = t * TILE, (t + 1) * TILE
        ent += [i for i, p in enumerate(parts) if p.at < hi and p.at + p.n > lo]
        off.append(len(ent))
    return np.array(off, dtype=np.uint32), np.array(ent, dtype=np.uint32)


def to_ffi(W, p):
    """a Part as the binding's wbx_splice_part"""
    return W.splice_part(p.src, p.first, p.n, p.at, bool(p.reverse), p.mode, p.gain, p.fade_in, p.fade_out, p.shape_in, p.shape_out)
