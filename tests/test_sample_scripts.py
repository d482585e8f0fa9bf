"""The census of the sample life scripts (tests/sample_scripts.py) that tests/test_gpu_sample_scripts.py runs on the
device: what the seeds cover is asserted here, without a device, so that a script set which lost a case cannot pass for
want of it — every kind of op, splices and loudness normalizations among them, every producer's result as somebody's
source, the chains that run a splice over takes, bounces and earlier splices, the shapes of a splice (both channel counts,
a crossfade, an uncovered gap, 8 granules), the newcomers in freed extents and played through their end at another rate,
loudness measurements of no hop and with a true peak at 96 / 32 kHz, and refused producers with a delete behind them."""
import numpy as np

import sample_scripts as SS

# the seeds whose contents test_every_producing_op_is_drawn_valid computes (the numpy twin of a loudness measurement with
# its 4x rendering takes up to a second): the three that were computed before the loudness ops joined, which hold a
# loudness normalization under a binding ceiling AND one whose LUFS target binds, both asserted there
MODEL_SEEDS = SS.SEEDS[:3]


def test_the_scripts_cover_what_they_are_for():
    c = SS.census()
    for kind in SS.KINDS:
        assert c["op:" + kind] >= 8, (kind, c["op:" + kind])
    for producer in SS.PRODUCERS:                       # everybody's result is somebody's source
        assert c["as_source:" + producer] >= 3, producer
    for chain in ("take->resample", "bounce->derive", "resample->derive->resample",
                  "take->splice", "bounce->splice", "splice->splice", "splice->resample", "resample->loudnorm",
                  "splice->loudnorm", "derive->loudnorm", "normalize->loudnorm"):
        assert c["source:" + chain] >= 3, chain
    assert c["hole_refilled"] >= 10                     # a delete that was not the newest sample, then a producer no larger
    assert c["play_through_the_end_off_rate"] >= 5      # the first padding frame is read
    assert c["refused_delete"] >= 3
    assert c["worst_total_bytes"] <= SS.BUDGET
    # the shapes of a splice
    for fact in ("splice_both_channel_counts", "splice_crossfade", "splice_gap", "splice_8_granules", "splice_part_at_0",
                 "splice_part_to_the_end", "splice_part_straddles_a_tile"):
        assert c[fact] >= 3, (fact, c[fact])
    for n in SS.SPLICE_LENGTHS:
        assert c["splice_frames:%d" % n] >= 3, n
    # the two newest producers among the others: in a freed extent, and with the padding behind them read
    for producer in ("splice", "loudnorm"):
        assert c["hole_refilled:" + producer] >= 3, producer
        assert c["play_through_the_end_off_rate:" + producer] >= 3, producer
    assert c["splice_sounding_4_hops"] >= 3             # loud all over and long enough: a source for loudness ops
    # the measurement beside the pool: no hop is the edge, the others have hop energies to compare and most have blocks to
    # gate, on results of the device's own producers and at every rate but the session's
    assert c["loudness_no_hop"] >= 3 and c["loudness_to_the_last_frame"] >= 3
    assert c["loudness_true_peak_at_96000_or_32000"] >= 3
    assert c["loudness_hops"] >= 2 * c["loudness_no_hop"] and c["loudness_blocks"] >= 8
    for producer in ("splice", "derive", "resample"):
        assert c["loudness_hops:" + producer] >= 3 and c["loudness_blocks:" + producer] >= 3, producer
    for rate in SS.RATES:
        assert c["loudness_hops:%d" % rate] >= 3, rate
    # refused producers in a busy pool, and the delete that shows a pin left behind
    assert c["refused_splice:%d" % SS.REFUSED_I16] >= 3 and c["refused_splice:%d" % SS.REFUSED_RATES] >= 3
    assert c["refused_loudnorm"] >= 3
    assert c["refused_splice_then_delete"] >= 3 and c["refused_loudnorm_then_delete"] >= 3


def test_every_producing_op_is_drawn_valid():
    """SS.census() validates every script on shapes (ranges, channel modes, fades, rates, lengths, the hop minimum, the
    oversampling cap); here the contents model accepts every op of a script it can compute alone — splices and loudness
    normalizations with no take or bounce behind them included — and stays in audio range without a NaN.  Only
    MODEL_SEEDS are computed (see there)."""
    binds = {"ceiling": 0, "target": 0}
    for seed in MODEL_SEEDS:
        ops, _ = SS.make_script(seed)
        SS.validate(ops)
        m, skipped = SS.Contents(), set()
        for op in ops:
            if op[0] == "splice":
                srcs = {p[0] for p in op[4]}
            else:
                srcs = {op[2]} if op[0] in ("derive", "normalize", "resample", "loudnorm") else set()
            if op[0] in ("take", "bounce"):
                skipped.update([op[1]] if op[0] == "take" else op[1])
            elif srcs & skipped:
                skipped.add(op[1])
            elif op[0] == "delete" and op[1] in skipped:
                continue
            else:
                if op[0] == "loudnorm" and op[-1] == 0:
                    gain, free, top = m.loudnorm_gains(op)
                    assert np.isfinite(free) and gain == min(free, top) and gain > 0, (seed, op)
                    binds["ceiling" if top < free else "target"] += 1
                    m.apply_loudnorm(op, gain)
                    key = op[1]
                else:
                    key = m.apply(op)
                if key is not None and m.s[key][0] == "f32":
                    x = np.stack(m.s[key][2])
                    assert np.isfinite(x).all() and np.abs(x).max() <= 1.2, (seed, op)
    assert binds["ceiling"] >= 1 and binds["target"] >= 1, binds


def test_the_length_menu_holds_the_edges():
    L = set(SS.LENGTHS)
    assert {1, 7, 37} <= L
    assert any(SS.row_bytes(n) == (n + 16) * 4 and n + 1 in L for n in L)                       # a full row, and one frame more
    assert any(2 * SS.row_bytes(n) % SS.G == 0 and 2 * (n + 16) * 4 % SS.G == 0 and n + 1 in L for n in L)   # full granules
    assert sum(SS.body_bytes(n, 2) >= 8 * SS.G for n in L) >= 2 and SS.body_bytes(max(L), 2) <= 24 * SS.G
    S = set(SS.SPLICE_LENGTHS)                                                                  # the splice's tile of 512 frames
    assert {1, 511, 512, 513, 2573} <= S and any(n >= 70001 and n in L and SS.body_bytes(n, 2) >= 8 * SS.G for n in S)
