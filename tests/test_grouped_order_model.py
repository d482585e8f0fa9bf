"""CPU checks of tests/grouped_order.py, the plain restatement of the library's grouped summation order that the GPU tests
hold every grouped-order render against bit for bit: with one group per member list it must BE the reference's order (the
oracle's master and bus sums, bit for bit), and it must see what the 1e-6 RMS gate cannot."""
import dataclasses

import numpy as np
import pytest

import fuzz_util as FZ
import golden_util as G
import grouped_order as GO
from whitebox_amd import synth


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


class _SpecialValuesSpec(synth.SessionSpec):
    """fp32 clips salted with special values (as tests/test_gpu_parity.py salts its sessions)"""
    SALTS = {"denormals_and_zeros": [1e-40, -1e-45, -0.0, 0.0, 1.17549435e-38, -1e-39],
             "huge": [3e38, -3e38, 1e-40, -0.0, 2.5e37],
             "nonfinite": [np.inf, -np.inf, np.nan, 3e38, -0.0, 1e-40]}

    def sample_data(self, i):
        out = super().sample_data(i)
        specials = np.array(self.SALTS[self.salt], np.float32)
        for c, a in enumerate(out):
            n = len(a) - 16
            idx = (np.arange(0, n, 37) + 5 * i + c) % max(n, 1)
            a[idx] = specials[(np.arange(len(idx)) + i) % len(specials)]
        return out


def check_reference_order(spec, n_blocks):
    om, obus, tracks = GO.oracle_tracks(spec, n_blocks)
    assert tracks.shape == (n_blocks, spec.n_tracks, spec.channels, spec.block)
    for g in (GO.WHOLE, max(spec.n_tracks, 1)):
        m, bus = GO.model_for(spec, tracks, g)
        GO.assert_model(m, om, bus if spec.n_buses else None, obus, what=(spec.name, g))
    return om, obus, tracks


@pytest.mark.parametrize("name", G.session_names())
def test_model_is_the_reference_order_on_the_golden_sessions(name):
    """one group per member list: the golden master and bus sums (the reference's own engine) bit for bit"""
    spec, n_blocks, g = G.load_session(name)
    om, obus, tracks = check_reference_order(spec, n_blocks)
    assert np.array_equal(GO.bits(om), GO.bits(g["master"]))
    if spec.n_buses:
        m, bus = GO.model_for(spec, tracks, GO.WHOLE)
        assert np.array_equal(GO.bits(bus), GO.bits(g["buses"]))


@pytest.mark.parametrize("seed", range(40))
def test_model_is_the_reference_order_on_random_sessions(seed):
    """fuzz_util's sessions: sub-buses with tracks routed straight to the master between them, mutes, every storage
    format, mono and stereo, odd block sizes"""
    spec, n_blocks = FZ.random_session(seed)
    check_reference_order(spec, n_blocks)


@pytest.mark.parametrize("salt", ["denormals_and_zeros", "huge", "nonfinite"])
def test_model_is_the_reference_order_with_special_values(salt):
    """NaN, infinities, signed zeros, subnormals and values near FLT_MAX in the clips; a muted track, hard pans (exact-zero
    gains: -0.0 products) and sub-buses"""
    base = synth.make_session("spv", 20, seek=True, n_blocks=4, seed=0x5F0, src_rate=44100, amp=1e-3, n_buses=3)
    spec = _SpecialValuesSpec(**{f.name: getattr(base, f.name) for f in dataclasses.fields(base)})
    spec.salt = salt
    spec.mutes[3] = True
    spec.pans[5], spec.pans[6] = -1.0, 1.0
    spec.track_bus = [[-1, 0, 1, 2][t % 4] for t in range(spec.n_tracks)]
    om, _, tracks = check_reference_order(spec, 4)
    if salt == "nonfinite":
        assert np.isnan(om).any() and np.isnan(tracks).any()


def test_partition_restates_build_routing():
    """direct tracks first, then each bus's tracks, every list cut into pieces of G (the last piece short)"""
    bus = [-1, 0, 1, -1, 0, 7, 1, 0, -1, 0]          # (bus 7 of 2: straight to the master)
    parts = GO.partition(10, 2, 2, bus)
    assert parts == [(-1, [0, 3]), (-1, [5, 8]), (0, [1, 4]), (0, [7, 9]), (1, [2, 6])]
    assert GO.partition(10, 3, 2, bus) == [(-1, [0, 3, 5]), (-1, [8]), (0, [1, 4, 7]), (0, [9]), (1, [2, 6])]
    assert GO.shape_of(GO.partition(300, 128)) == (3, 128)
    assert GO.partition(5, 4, 3, [2, 2, 2, 2, 2]) == [(2, [0, 1, 2, 3]), (2, [4])]
    assert [GO.group_size_of(n, 0, 1) for n in (1, 16, 17, 64, 65, 256, 257, 512, 513, 4096)] == [64, 64, 1, 1, 4, 4, 8, 8, 16, 16]
    assert GO.group_size_of(4096, 0, 8) == 128 and GO.group_size_of(4096, 24, 1) == 24


def _mix_bus_level(n_tracks=1024, n_blocks=2):
    """BASELINE config 3's session at mix-bus level (amp = 1/sqrt(N): the master around full scale, part of it clamped)"""
    return synth.make_session("c3", n_tracks, n_blocks=n_blocks, seed=0x5EED0003, src_rate=44100,
                              amp=float(np.float32(1.0 / np.sqrt(n_tracks))))


def test_rms_gate_misses_what_the_model_sees():
    """At mix-bus level, three wrong renders that the 1e-6 RMS gate against the reference order passes: two group sums added
    in the wrong order, one 4-frame lane of one block summed in the reference's order instead of the grouped one, one
    sample one ulp off.  The model tells each of them from the right grouped-order render."""
    spec = _mix_bus_level()
    om, _, tracks = GO.oracle_tracks(spec, 2)
    groups = GO.spec_partition(spec, GO.DEFAULT_GROUP)
    right, _ = GO.grouped_sum(tracks, groups)
    assert rms(right, om) <= 1e-6 and not np.array_equal(GO.bits(right), GO.bits(om))   # (the grouped order is not the reference's)

    swapped = list(groups)
    swapped[2], swapped[5] = swapped[5], swapped[2]
    wrong_order, _ = GO.grouped_sum(tracks, swapped)

    lane = right.copy()
    diff = np.argwhere(GO.bits(right[1, 1]) != GO.bits(om[1, 1]))
    f0 = int(diff[len(diff) // 2][0]) & ~3
    lane[1, 1, f0:f0 + 4] = om[1, 1, f0:f0 + 4]

    ulp = right.copy()
    k = np.argwhere(np.abs(right[0, 0]) < 0.5)[0][0]
    ulp[0, 0, k] = np.nextafter(ulp[0, 0, k], np.float32(1.0))

    for what, wrong in (("groups swapped", wrong_order), ("one lane", lane), ("one ulp", ulp)):
        assert rms(wrong, om) <= 1e-6, what
        assert not GO.same_bits(wrong, right).all(), what
        with pytest.raises(AssertionError):
            GO.assert_model(wrong, right, what=what)
