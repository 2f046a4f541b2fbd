"""CPU: the streams of stream_edge_inputs.py are what they claim to be -- asserted on the ORACLE's output (the restated LoRaDemod
block, pinned to the verbatim one), never on the device's: every data bin won once (set A), the first signal-bearing FRAMESYNC
window peaking in the chosen bin with a fIndex that cannot hide inside the comparison's tolerance (set B), non-finite values in
the calls but in no FRAMESYNC call (set C). test_gpu_stream_instances.py runs the same streams through every streaming instance."""
import numpy as np
import pytest

from stream_edge_inputs import EXTRA_A, SFS, expected, inputs, rows, symbols_per_frame, sync_targets

FRAMESYNC, DOWNCHIRP0, DOWNCHIRP1, QUARTERCHIRP, DATASYMBOLS = range(5)


def posted_one_packet(r, want=None, length=None):
    if len(r["packets"]) != 1:
        return False
    p = r["packets"][0][1]
    return (want is None or np.array_equal(p, want.astype(np.int16))) and (length is None or len(p) == length)


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("sf", SFS)
def test_the_streams_are_built_as_described(sf, name):
    N = 1 << sf
    s = inputs(sf, name)
    assert inputs(sf, name) is s                                        # built once
    n_ch = {"A": N // symbols_per_frame(sf) + EXTRA_A, "B": len(sync_targets(sf)), "C": 7}[name]
    assert len(s.streams) == len(s.syms) == len(s.leads) == n_ch
    frame = (10 + 2 + 2) * N + N // 4 + (s.mtu + 1) * N                 # preamble, sync, down-chirps, quarter chirp, symbols, padding = 1
    for st, sy, k in zip(s.streams, s.syms, s.leads):
        assert st.dtype == np.complex64 and not st.flags.writeable and 0 <= k < N
        assert st.size == N + k + frame + 2 * N and len(sy) == s.mtu
        assert not st[:N + k].any() and not st[N + k + frame:].any()    # exact zeros around the frame
        assert st[N + k] != 0
    if name == "A":
        S, B = s.mtu, N // s.mtu
        assert S == (64 if sf == 12 else 32)
        assert sorted(int(v) for sy in s.syms[:B] for v in sy) == list(range(N))
        assert s.leads[:B] == [(c * S + 5) % N for c in range(B)]
    if name == "B":
        assert s.mtu == 2 and s.leads == [(1 - b) % N for b in s.targets] and len(set(s.targets)) == len(s.targets)
        assert {0, 1, 2, N - 2, N - 1, N // 2 - 1, N // 2, N // 2 + 1} <= set(s.targets)
        assert set(s.targets) == set(range(N)) if sf <= 10 else {j * (N // 256 + 1) % N for j in range(256)} <= set(s.targets)
    if name == "C":
        bad = [int((~np.isfinite(st.view(np.float32))).sum()) for st in s.streams]
        assert bad == [2, 1, 3, 0, 0, 0, 0]
        assert np.abs(s.streams[3]).max() > 1e19 and np.abs(s.streams[4]).max() > 1e38 and 0 < np.abs(s.streams[5]).max() < 1e-20
    r = rows(sf, name)
    assert r.shape[0] == n_ch and r.shape[1] % 16 == 0 and not r.flags.writeable
    for c, st in enumerate(s.streams):
        assert np.array_equal(r[c, :st.size].view(np.uint32), st.view(np.uint32)) and not r[c, st.size:].any()


@pytest.mark.parametrize("sf", SFS)
def test_data_sweep_every_bin_wins_a_data_symbol_once(oracle, sf):
    N = 1 << sf
    s = inputs(sf, "A")
    res = expected(oracle, sf, "A")
    assert expected(oracle, sf, "A") is res                             # computed once
    B = N // s.mtu
    for c, (r, sy) in enumerate(zip(res, s.syms)):
        assert posted_one_packet(r, want=sy), "sf%d channel %d" % (sf, c)
    values = sorted(k["value"] for r in res[:B] for k in r["calls"] if k["state"] == DATASYMBOLS)
    assert values == list(range(N))
    # the padded rows the resident receiver takes: the same packets
    for c, (r, sy) in enumerate(zip(expected(oracle, sf, "A", padded=True), s.syms)):
        assert posted_one_packet(r, want=sy), "sf%d channel %d, padded" % (sf, c)


@pytest.mark.parametrize("sf", SFS)
def test_sync_sweep_first_framesync_window_peaks_in_the_target_bins(oracle, sf):
    N = 1 << sf
    s = inputs(sf, "B")
    res = expected(oracle, sf, "B")
    for c, (r, sy) in enumerate(zip(res, s.syms)):
        assert posted_one_packet(r, want=sy), "sf%d channel %d (bin %d)" % (sf, c, s.targets[c])
    first = [next(k for k in r["calls"] if k["state"] == FRAMESYNC and np.isfinite(k["snr"])) for r in res]
    reached = {k["value"] for k in first}
    assert len(reached & set(s.targets)) >= 0.95 * len(s.targets)
    assert {0, 1, N - 1} <= reached
    if sf >= 11:
        assert {v // (N // 16) for v in reached} == set(range(16))
    for c, k in enumerate(first):
        if c % 3:
            assert abs(k["fIndex"]) > 0.01, "sf%d channel %d (bin %d): fIndex %r" % (sf, c, s.targets[c], k["fIndex"])


@pytest.mark.parametrize("sf", SFS)
def test_non_finite_samples_stay_out_of_framesync(oracle, sf):
    for padded in (False, True):
        res = expected(oracle, sf, "C", padded=padded)
        assert len(res) == 7
        for c, r in enumerate(res):
            assert posted_one_packet(r, length=8), "sf%d channel %d" % (sf, c)
        calls = [k for r in res for k in r["calls"]]
        assert sum(1 for k in calls if not np.isfinite(k["power"]) or not np.isfinite(k["fIndex"])) >= 8
        assert all(np.isfinite(k["fIndex"]) for k in calls if k["state"] == FRAMESYNC)
