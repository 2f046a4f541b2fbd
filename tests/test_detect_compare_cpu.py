"""CPU: the comparison that test_gpu_detect_instances.py holds every kernel instance to must be able to fail. The oracle's own
result for the SF11 inputs, wrapped as the device result is (torch tensors, sym as int16), passes test_gpu_scan_keys.compare;
a copy that is wrong in one window, in each of the ways a tie-break, a neighbour pick or a reduction goes wrong, does not."""
import numpy as np
import pytest
import torch

from detect_edge_inputs import TWIN_AT, W, check_inputs, clean_windows, expected, inputs, twin_pairs
from test_gpu_scan_keys import compare

SF = 11
KEYS = ("sym", "power", "powerAvg", "fIndex")


def as_device_result(o):
    return {k: torch.from_numpy(o[k].view(np.int16) if k == "sym" else o[k]) for k in KEYS}


def mutated(o, key, w, value):
    m = {k: o[k].copy() for k in KEYS}
    m[key][w] = value
    return m


@pytest.fixture(scope="module")
def outs(oracle):
    res = expected(oracle, SF, "UNI")
    check_inputs(oracle, SF, "UNI", res)
    return {i.name: o for i, o in zip(inputs(SF), res)}


def rejected(m, o):
    with pytest.raises(AssertionError):
        compare(as_device_result(m), o, "mutated")
    return True


def test_the_unmutated_result_is_accepted(outs):
    for name, o in outs.items():
        compare(as_device_result(o), o, name)


def test_a_tie_broken_to_the_higher_bin_is_rejected(outs):
    o = outs["twin tones"]
    for w, (a, b) in zip(TWIN_AT, twin_pairs(SF)):
        assert o["sym"][w] == a
        assert rejected(mutated(o, "sym", w, b), o)


def test_swapped_neighbours_are_rejected(outs):
    """left and right bin exchanged: fIndex = 0.5 (right - left) / (2 peak - right - left) changes its sign and nothing else"""
    o = outs["sweep"]
    for w in (1, 2, 2047):                               # +0.3, -0.3, and the peak in the last bin (right neighbour: bin 0)
        assert abs(o["fIndex"][w]) > 0.01
        assert rejected(mutated(o, "fIndex", w, -o["fIndex"][w]), o)


def test_a_nan_window_with_an_index_is_rejected(outs):
    o = outs["NaN sample"]
    w = 1                                                # cases(): windows 1, 4, 7, ... hold the NaN
    assert np.isnan(inputs(SF)[[i.name for i in inputs(SF)].index("NaN sample")].iq[w]).any()
    assert o["sym"][w] == 0 and np.isneginf(o["power"][w]) and np.isnan(o["powerAvg"][w])     # no bin exceeds 0; the total is NaN
    assert rejected(mutated(o, "sym", w, 1), o)


def test_power_avg_off_by_1e_4_db_is_rejected(outs):
    o = outs["noise"]
    w = 3
    assert not clean_windows(o)[w] and abs(o["powerAvg"][w]) < 128     # two float ulps are below 1.6e-5 dB here
    for d in (1e-4, -1e-4):
        assert rejected(mutated(o, "powerAvg", w, np.float32(np.float64(o["powerAvg"][w]) + d)), o)


def test_a_finite_number_for_minus_inf_power_is_rejected(outs):
    o = outs["all-zero"]
    w = W - 1
    assert w % 8 != 0 and np.isneginf(o["power"][w])
    for k in ("power", "powerAvg"):
        assert rejected(mutated(o, k, w, np.float32(-3e38)), o)
