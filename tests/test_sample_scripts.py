"""The census of the sample life scripts (tests/sample_scripts.py) that tests/test_gpu_sample_scripts.py runs on the
device: what the seeds cover is asserted here, without a device, so that a script set which lost a case cannot pass for
want of it."""
import numpy as np

import sample_scripts as SS


def test_the_scripts_cover_what_they_are_for():
    c = SS.census()
    for kind in SS.KINDS:
        assert c["op:" + kind] >= 8, (kind, c["op:" + kind])
    for producer in SS.PRODUCERS:                       # everybody's result is somebody's source
        assert c["as_source:" + producer] >= 3, producer
    for chain in ("take->resample", "bounce->derive", "resample->derive->resample"):
        assert c["source:" + chain] >= 3, chain
    assert c["hole_refilled"] >= 10                     # a delete that was not the newest sample, then a producer no larger
    assert c["play_through_the_end_off_rate"] >= 5      # the first padding frame is read
    assert c["refused_delete"] >= 3
    assert c["worst_total_bytes"] <= SS.BUDGET


def test_every_producing_op_is_drawn_valid():
    """SS.census() validates every script on shapes (ranges, channel modes, fades, rates, lengths); here the contents model
    accepts every op of a script it can compute alone, and stays in audio range without a NaN"""
    for seed in SS.SEEDS[:3]:
        ops, _ = SS.make_script(seed)
        SS.validate(ops)
        m, skipped = SS.Contents(), set()
        for op in ops:
            src = op[2] if op[0] in ("derive", "normalize", "resample") else None
            if op[0] in ("take", "bounce"):
                skipped.update([op[1]] if op[0] == "take" else op[1])
            elif src in skipped:
                skipped.add(op[1])
            elif op[0] == "delete" and op[1] in skipped:
                continue
            else:
                key = m.apply(op)
                if key is not None and m.s[key][0] == "f32":
                    x = np.stack(m.s[key][2])
                    assert np.isfinite(x).all() and np.abs(x).max() <= 1.2, (seed, op)


def test_the_length_menu_holds_the_edges():
    L = set(SS.LENGTHS)
    assert {1, 7, 37} <= L
    assert any(SS.row_bytes(n) == (n + 16) * 4 and n + 1 in L for n in L)                       # a full row, and one frame more
    assert any(2 * SS.row_bytes(n) % SS.G == 0 and 2 * (n + 16) * 4 % SS.G == 0 and n + 1 in L for n in L)   # full granules
    assert sum(SS.body_bytes(n, 2) >= 8 * SS.G for n in L) >= 2 and SS.body_bytes(max(L), 2) <= 24 * SS.G
