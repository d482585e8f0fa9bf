"""The census of the sample life scripts (tests/sample_scripts.py) that tests/test_gpu_sample_scripts.py runs on the
device: what the seeds cover is asserted here, without a device, so that a script set which lost a case cannot pass for
want of it — every kind of op, splices and loudness normalizations among them, every producer's result as somebody's
source, the chains that run a splice over takes, bounces and earlier splices, the shapes of a splice (both channel counts,
a crossfade, an uncovered gap, 8 granules), the newcomers in freed extents and played through their end at another rate,
loudness measurements of no hop and with a true peak at 96 / 32 kHz, and refused producers with a delete behind them;
for filter, convolve, limit, dynamics, stretch and pitch the chains among each other and the older producers, every edge of
their size menus, the channel pairings of a convolution, mono and stereo keys, the limiter working and idling, every
documented refusal; for f0, onsets and tempo ranges of no hop, with hops and to the last frame.  The contents model is
held against the bounds the generator keeps on shapes alone (the stretch's convex combination among them), and must
hear voiced f0 hops and onsets in the tone and click uploads."""
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


def test_the_scripts_cover_the_newer_producers_and_the_consumers():
    """filter, convolve, limit, dynamics, stretch and pitch among the others, f0, onsets and tempo beside them: the chains,
    the freed extents, the padding read at another rate, every edge of the size menus, and every documented refusal with a
    delete behind it"""
    c = SS.census()
    for chain in ("take->filter", "bounce->limit", "splice->convolve", "resample->stretch", "stretch->pitch", "limit->dynamics",
                  "dynamics->limit", "filter->loudnorm", "pitch->splice"):
        assert c["source:" + chain] >= 3, (chain, c["source:" + chain])
    for producer in SS.NEW_PRODUCERS:
        assert c["op:" + producer] >= 8 and c["as_source:" + producer] >= 3, producer
        assert c["hole_refilled:" + producer] >= 3, (producer, c["hole_refilled:" + producer])
        assert c["play_through_the_end_off_rate:" + producer] >= 3, (producer, c["play_through_the_end_off_rate:" + producer])
    # every edge of the size menus, counted as the splice's lengths are
    edges = [("filter_total", SS.FILTER_TOTALS), ("filter_tail", SS.FILTER_TAILS), ("filter_cascade", range(8)),
             ("convolve_taps", SS.CONV_TAPS), ("convolve_out", SS.CONV_OUT + ("full",)), ("convolve_out_first", (0, 1, "mid")),
             ("limit_frames", SS.CURVE_SIZES + ("long",)), ("limit_terms", SS.CURVE_TERMS),
             ("dynamics_frames", SS.CURVE_SIZES + ("long",)), ("dynamics_terms", SS.CURVE_TERMS),
             ("dynamics_sense", (SS.DYN.COMPRESS, SS.DYN.GATE)),
             ("stretch_window", SS.STRETCH_WINDOWS), ("stretch_tolerance", SS.STRETCH_TOLERANCES),
             ("pitch_window", SS.STRETCH_WINDOWS), ("pitch_tolerance", SS.STRETCH_TOLERANCES),
             ("pitch_ratio", ["%d/%d" % r for r in SS.PITCH_RATIOS]), ("pitch_quality", SS.QUALITIES),
             ("f0_window", SS.F0_WINDOWS), ("f0_hop", SS.F0_HOPS), ("f0_tau_max", SS.F0_TAU_MAX),
             ("onsets_hop", SS.ONSET_HOPS), ("tempo_hop", SS.ONSET_HOPS)]
    for menu, entries in edges:
        for e in entries:
            assert c["%s:%s" % (menu, e)] >= 3, (menu, e, c["%s:%s" % (menu, e)])
    assert max(L for _, L in (SS.PM.ratio(*r) for r in SS.PITCH_RATIOS)) > 1000     # the conversion's large table
    for fact in ("stretch_shorter_than_a_window", "stretch_ends_inside_a_word_and_a_step", "stretch_longer", "stretch_shorter",
                 "pitch_own_length", "pitch_another_length"):
        assert c[fact] >= 3, (fact, c[fact])
    for pairing in ("1*1", "1*2", "2*1", "2*2"):        # source x response: every channel pairing of a convolution
        assert c["convolve_channels:" + pairing] >= 3, pairing
    assert c["dynamics_key_channels:1"] >= 3 and c["dynamics_key_channels:2"] >= 3 and c["dynamics_keyed_by_itself"] >= 3
    assert c["dynamics_key_to_the_last_frame"] >= 3
    assert c["limit_works"] >= 3 and c["limit_idles"] >= 3            # decided on the bounds: drive x amp against the ceiling
    # every documented refusal in a busy pool, and the delete that shows a pin left behind (of both sources where there are two)
    for refusal in ("filter:%d" % SS.REFUSED_I16, "limit:%d" % SS.REFUSED_I16, "stretch:%d" % SS.REFUSED_I16,
                    "convolve:%d" % SS.REFUSED_RATES, "convolve:%d" % SS.REFUSED_I16, "dynamics:%d" % SS.REFUSED_RATES,
                    "dynamics:%d" % SS.REFUSED_I16, "stretch_beyond_8:%d" % SS.REFUSED_RATIO, "pitch:%d" % SS.REFUSED_ONE,
                    "pitch:%d" % SS.REFUSED_RATIO):
        assert c["refused_" + refusal] >= 3, (refusal, c["refused_" + refusal])
    for producer in SS.NEW_PRODUCERS:
        assert c["refused_%s_then_delete" % producer] >= 3, producer
    assert c["refused_convolve_then_delete_of_both"] >= 3 and c["refused_dynamics_then_delete_of_both"] >= 3
    # the consumers: the edge of no hop, hops to compare, and the source's last frame
    for consumer in SS.CONSUMERS:
        assert c["op:" + consumer] >= 8, consumer
        for fact in ("_no_hop", "_hops", "_to_the_last_frame"):
            assert c[consumer + fact] >= 3, (consumer + fact, c[consumer + fact])


def test_every_producing_op_is_drawn_valid():
    """SS.census() validates every script on shapes (ranges, channel modes, fades, rates, lengths, the hop minimum, the
    oversampling cap); here the contents model accepts every op of a script it can compute alone — splices and loudness
    normalizations with no take or bounce behind them included — and stays in audio range without a NaN.  Only
    MODEL_SEEDS are computed (see there)."""
    binds = {"ceiling": 0, "target": 0}
    seen = {"voiced f0 hops": 0, "onsets": 0, "tempo windows": 0, "limited frames": 0, "reduced frames": 0, "searched steps": 0}
    computed, bounds = dict.fromkeys(SS.NEW_PRODUCERS + SS.CONSUMERS, 0), {}
    for seed in MODEL_SEEDS:
        ops, _ = SS.make_script(seed)
        SS.validate(ops)
        m, skipped = SS.Contents(), set()
        for op in ops:
            srcs = SS.sources_of(op)
            if op[0] in ("take", "bounce"):
                skipped.update([op[1]] if op[0] == "take" else op[1])
            elif srcs & skipped:
                if op[0] in SS.PRODUCERS and op[1] is not None:
                    skipped.add(op[1])
            elif op[0] == "delete" and op[1] in skipped:
                continue
            elif op[0] in SS.CONSUMERS:
                rec, info = m.analyse(op)
                computed[op[0]] += 1
                assert len(rec) == info["hops"] and all(np.isfinite(rec[f]).all() for f in rec.dtype.names if f != "_pad"), (seed, op)
                seen["voiced f0 hops"] += info["voiced_hops"] if op[0] == "f0" else 0
                seen["tempo windows"] += info["hops"] if op[0] == "tempo" else 0
                seen["onsets"] += info["onsets"] if op[0] == "onsets" else 0
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
                if key is not None and op[0] in SS.NEW_PRODUCERS:
                    computed[op[0]] += 1
                    bounds.setdefault(op[0], []).append((float(np.abs(x).max()), seed, op))
                    seen["limited frames"] += m.info["limited_frames"] if op[0] == "limit" else 0
                    seen["reduced frames"] += m.info["reduced_frames"] if op[0] == "dynamics" else 0
                    seen["searched steps"] += m.info["searched_steps"] if op[0] in ("stretch", "pitch") else 0
    assert binds["ceiling"] >= 1 and binds["target"] >= 1, binds
    assert all(n >= 3 for n in computed.values()), computed       # (the others have a take or a bounce behind them)
    assert all(n >= 1 for n in seen.values()), seen                # the tone and the clicks do their job, the curves move
    # the bounds the generator keeps on shapes alone hold on the contents: a stretch is a convex combination of two source
    # frames, a limit stays under its ceiling, a convolution under amp x amp x L x gain, ... (Meta.amp, replayed here)
    for kind, peaks in bounds.items():
        for peak, seed, op in peaks:
            assert peak <= SS.AMP[seed, op[1]], (kind, peak, SS.AMP[seed, op[1]], seed, op)


def test_the_length_menu_holds_the_edges():
    L = set(SS.LENGTHS)
    assert {1, 7, 37} <= L
    assert any(SS.row_bytes(n) == (n + 16) * 4 and n + 1 in L for n in L)                       # a full row, and one frame more
    assert any(2 * SS.row_bytes(n) % SS.G == 0 and 2 * (n + 16) * 4 % SS.G == 0 and n + 1 in L for n in L)   # full granules
    assert sum(SS.body_bytes(n, 2) >= 8 * SS.G for n in L) >= 2 and SS.body_bytes(max(L), 2) <= 24 * SS.G
    S = set(SS.SPLICE_LENGTHS)                                                                  # the splice's tile of 512 frames
    assert {1, 511, 512, 513, 2573} <= S and any(n >= 70001 and n in L and SS.body_bytes(n, 2) >= 8 * SS.G for n in S)
