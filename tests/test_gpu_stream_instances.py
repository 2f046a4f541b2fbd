"""GPU: the edge streams of stream_edge_inputs.py through every shipped instance of the streaming demodulator (mode 1, the frame
machine on the device) -- the counterpart of test_gpu_detect_instances.py for the path a receiver runs.

The streaming kernels do not reuse the batch scan: demodStream (lorahip_streamkernel.h) and demodStreamWide (lorahip_stream_wide.hip)
carry their own FFT phases, scans, neighbour fetch and -- without a trace -- a quick path of their own (scanQuick, squelchQuickF,
neighbours by register select, fIndexPaired). The instances, by the selection that reaches them:

  SF6, SF10      set_stream_lanes(-1)                       Stream6, Stream10
  SF7            lanes -1, 4, 5, 16|3, 16|4, 16|5           Stream7, Stream7L4, Stream7L5 and the three look-ahead (AHEAD) instances
  SF8            lanes -1, 5, 6, 16|4, 16|5                 Stream8, Stream8L5, Stream8L6, two AHEAD
  SF9            lanes -1, 6, 16|5                          Stream9, Stream9L6, one AHEAD
  SF11, SF12     set_stream_grid(-1) / set_stream_grid(3)   StreamWide11 / 12 plain and PERSIST (more than 3 channels)
  SF7 to SF12    receive(async_=3, depth=1)                 the resident (RES) instances

What goes through each: set A (every bin wins a data symbol once), set B (the first signal-bearing FRAMESYNC window peaks in
every bin / 264 chosen bins: the window whose fIndex enters the fine-tune state) and set C (NaN, Inf, overflow, subnormals outside
FRAMESYNC). Per non-resident instance and set: (a) a traced run against the oracle call by call, (b) an untraced run -- packets,
read positions, call count, signals -- against the oracle and the traced run, (c) for set B the quick path's fIndex, visible only
through the fine-tune state: an untraced prefix up to the middle of the preamble, traced from there, must continue as the fully
traced run does, and (d) the integer fields of the traces and the packets identical across the instances of one SF. The resident
instances have no trace: (e) sets A and C in receiver steps of 5 N to 9 N samples against the oracle.

What it found when written (profiles/r15/README.md): sets A and B nothing; set C, channel 4 -- the finite sample (3e38, -3e38) at
N / 2 + 1 of a DATASYMBOLS window -- value 1 against the oracle's 0 in every instance at SF 6, 7, 8, 10 and 12: the dechirp leaves
(y, -Inf) without a NaN, kissfft's leaf product by twiddle(0) = (1, -0) makes it NaN (no bin wins: index 0), the kernels' skipped
product left bins of a clean Inf. The streaming kernels now repeat a window whose total is not finite with the products carried out."""
import numpy as np
import pytest

from stream_edge_inputs import expected, inputs, rows
from test_gpu_demod import TOL_DB, compare_channel, compare_channel_by_class

pytestmark = pytest.mark.gpu

AHEAD = 16                                                  # lorahip.h: LORAHIP_LANES_AHEAD | log2 lanes of one window
LANES = {6: [-1], 7: [-1, 4, 5, AHEAD | 3, AHEAD | 4, AHEAD | 5], 8: [-1, 5, 6, AHEAD | 4, AHEAD | 5], 9: [-1, 6, AHEAD | 5], 10: [-1]}
GRIDS = {11: [-1, 3], 12: [-1, 3]}                          # < 0: one workgroup per channel; 3: PERSIST, three workgroups walk the channels
INSTANCES = [(sf, "lanes", v) for sf, vs in LANES.items() for v in vs] + [(sf, "grid", v) for sf, vs in GRIDS.items() for v in vs]
RESIDENT_SFS = [7, 8, 9, 10, 11, 12]

INT_FIELDS = ("consumed", "state_before", "value", "worked", "packet_len", "signals", "sig_error", "fine_idx_before", "fine_idx_after")
STATE_FIELDS = ("consumed", "state_before", "value", "fine_idx_before", "fine_idx_after", "packet_len")


def instance_id(inst):
    sf, kind, v = inst
    if kind == "grid":
        return "sf%d-%s" % (sf, "plain" if v < 0 else "persist")
    return "sf%d-%s" % (sf, "base" if v < 0 else ("ahead%d" % (v & 15) if v & AHEAD else "lanes%d" % v))


def make(L, inst, n_channels, mtu):
    """a mode-1 demodulator forced onto one instance; the selection is asserted"""
    sf, kind, v = inst
    d = L.LoRaDemod(sf, n_channels=n_channels)
    d.set_mode(1)
    d.setMTU(mtu)
    if kind == "lanes":
        d.set_stream_lanes(v)
        assert d.stream_lanes() == (sf - 4 if v < 0 else v), "%s: the build does not hold the instance" % instance_id(inst)
    else:
        d.set_stream_grid(v)
        assert d.stream_lanes() == sf - 4
        assert v < 0 or n_channels > v                      # the persistent grid is taken with more channels than workgroups only
    return d


def first_difference(tr, calls):
    """where a trace leaves the oracle's calls, for the message of a failed comparison: "call i field: got / expected" """
    if len(tr) != len(calls):
        return "%d calls, expected %d" % (len(tr), len(calls))
    for i, (a, b) in enumerate(zip(tr, calls)):
        for ka, kb, tol in (("consumed", "consumed", 0), ("state_before", "state", 0), ("value", "value", 0), ("f_index", "fIndex", 2e-6), ("power", "power", TOL_DB)):
            va, vb = float(a[ka]), float(b[kb])
            if va != vb and not (np.isnan(va) and np.isnan(vb)) and not abs(va - vb) <= tol:
                return "call %d %s: %r, expected %r" % (i, ka, a[ka], b[kb])
    return "no difference found"


def check_packets(pk, c, ref, where):
    mine = [p[2] for p in pk if p[0] == c]
    assert len(mine) == len(ref["packets"]), "%s: %d packets, expected %d" % (where, len(mine), len(ref["packets"]))
    for j, (a, (_, b)) in enumerate(zip(mine, ref["packets"])):
        assert np.array_equal(a, b), "%s packet %d: %r, expected %r" % (where, j, a.tolist(), b.tolist())


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


_ACROSS = {}        # (sf, set) -> (instance id, per channel the integer fields of the trace, the packets): the first instance that ran


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_edge_streams_through_every_instance(gpu, oracle, inst, name):
    import lora_sdr_amd as L
    sf = inst[0]
    N = 1 << sf
    s = inputs(sf, name)
    refs = expected(oracle, sf, name)
    B = len(s.streams)
    tag = "%s set %s" % (instance_id(inst), name)
    total_calls = sum(len(r["calls"]) for r in refs)
    used = [int(sum(k["consumed"] for k in r["calls"])) for r in refs]

    # (a) traced
    d = make(L, inst, B, s.mtu)
    try:
        d.set_trace(True)
        d.work(s.streams)
        pk = d.packets()
        traces = [d.trace_array(c) for c in range(B)]
        for c in range(B):
            where = "%s traced channel %d" % (tag, c)
            try:
                if name == "C":
                    compare_channel_by_class(traces[c], refs[c]["calls"], where)
                else:
                    compare_channel(traces[c], refs[c]["calls"])
            except AssertionError as e:
                raise AssertionError("%s %s\n%s" % (where, first_difference(traces[c], refs[c]["calls"]), e)) from e
            check_packets(pk, c, refs[c], where)
            assert d.consumed(c) == used[c], "%s consumed: %d, expected %d" % (where, d.consumed(c), used[c])
        assert d.work_calls() == total_calls, "%s traced work_calls" % tag
    finally:
        d.close()

    # (d) across the instances of the SF: integer fields and packets identical
    ints = [np.stack([t[f].astype(np.int64) for f in INT_FIELDS]) for t in traces]
    packets = [(p[0], p[2].tolist()) for p in sorted(pk, key=lambda p: (p[0], p[1]))]
    other, ints0, packets0 = _ACROSS.setdefault((sf, name), (instance_id(inst), ints, packets))
    for c in range(B):
        if not np.array_equal(ints[c], ints0[c]):
            f, i = np.argwhere(ints[c] != ints0[c])[0] if ints[c].shape == ints0[c].shape else (0, -1)
            raise AssertionError("%s channel %d call %d %s: differs from instance %s" % (tag, c, i, INT_FIELDS[f], other))
    assert packets == packets0, "%s: packets differ from instance %s" % (tag, other)

    # (b) untraced, signals kept: the quick squelch estimate, fIndex only where the frame machine consumes it
    d = make(L, inst, B, s.mtu)
    try:
        d.set_signals(True)
        d.work(s.streams)
        pk2 = d.packets(clear=False)
        ch, _rd, er, pw, sn = d.signals()
        for c in range(B):
            where = "%s untraced channel %d" % (tag, c)
            check_packets(pk2, c, refs[c], where)
            assert d.consumed(c) == used[c], "%s consumed: %d, expected %d" % (where, d.consumed(c), used[c])
            mine, want = ch == c, traces[c][traces[c]["signals"] != 0]
            assert er[mine].tolist() == [int(g[0]) for g in refs[c]["signals"]], "%s sig_error" % where
            assert mine.sum() == want.size, "%s signals" % where
            assert np.array_equal(bits(pw[mine]), bits(want["sig_power"])), "%s sig_power: %r, traced %r" % (where, pw[mine], want["sig_power"])
            assert np.array_equal(bits(sn[mine]), bits(want["sig_snr"])), "%s sig_snr: %r, traced %r" % (where, sn[mine], want["sig_snr"])
        assert d.work_calls() == total_calls, "%s untraced work_calls: %d, expected %d" % (tag, d.work_calls(), total_calls)
    finally:
        d.close()
    if name != "B":
        return

    # (c) the quick path's fIndex through the state it leaves: untraced up to f0 + 6 N (inside the preamble, after the FRAMESYNC calls
    # that add fIndex to the fine-tune error), traced from there -- the tail of the fully traced run, fine_err_before bit for bit
    d = make(L, inst, B, s.mtu)
    try:
        d.work([st[:N + k + 6 * N] for st, k in zip(s.streams, s.leads)])
        stopped = [d.consumed(c) for c in range(B)]
        n_before = []
        for c in range(B):
            ends = np.cumsum(traces[c]["consumed"])
            i = int(np.searchsorted(ends, stopped[c]))
            assert i < len(ends) and ends[i] == stopped[c], "%s channel %d: the untraced prefix stopped inside a call of the traced run (%d)" % (tag, c, stopped[c])
            n_before.append(i + 1)
        d.clear_packets()
        d.set_trace(True)
        d.work([st[u:] for st, u in zip(s.streams, stopped)])
        for c in range(B):
            got, want = d.trace_array(c), traces[c][n_before[c]:]
            where = "%s continuation channel %d (bin %d)" % (tag, c, s.targets[c])
            assert len(got) == len(want) > 0, "%s: %d calls, expected %d" % (where, len(got), len(want))
            for f in STATE_FIELDS:
                if not np.array_equal(got[f], want[f]):
                    i = int(np.argmax(got[f] != want[f]))
                    raise AssertionError("%s call %d %s: %r, traced run %r" % (where, n_before[c] + i, f, got[f][i], want[f][i]))
            if not np.array_equal(bits(got["fine_err_before"]), bits(want["fine_err_before"])):
                i = int(np.argmax(bits(got["fine_err_before"]) != bits(want["fine_err_before"])))
                raise AssertionError("%s call %d fine_err_before: %r, traced run %r" % (where, n_before[c] + i, got["fine_err_before"][i], want["fine_err_before"][i]))
    finally:
        d.close()


@pytest.mark.parametrize("name", ["A", "C"])
@pytest.mark.parametrize("sf", RESIDENT_SFS)
def test_edge_streams_through_the_resident_instances(gpu, oracle, sf, name):
    """(e) receive(async_=3): one kernel stays on the device and takes the steps as messages (test_gpu_receiver.py::
    test_resident_receiver_equals_the_reference, cut down): all steps together give the oracle's packets, read positions, call
    total and signals"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(1700 + sf)
    N = 1 << sf
    s = inputs(sf, name)
    host = rows(sf, name)
    refs = expected(oracle, sf, name, padded=True)
    B, cap = host.shape
    tag = "sf%d-resident set %s" % (sf, name)
    iq = gpu.tensor(host).cuda()
    gpu.cuda.synchronize()
    d = L.LoRaDemod(sf, n_channels=B)
    try:
        d.set_mode(1); d.setMTU(s.mtu); d.set_signals(True)
        prows = [d.receiver_rows(cap_packets=4 * B, stride=64) for _ in range(2)]
        sigs = [d.receiver_signal_rows(8 * B, pinned_host=True) for _ in range(2)]
        got, got_sig, calls, w, k, resident_steps = [[] for _ in range(B)], [[] for _ in range(B)], 0, 0, 0, 0
        pending = []                                                 # row sets of the resident steps rung and not yet reported, oldest first

        def take(n, r, sig, nsig):
            sy, ns, chn = r[0][:n].cpu().numpy(), r[1][:n].cpu().numpy(), r[2][:n].cpu().numpy()
            for i in range(n):
                got[int(chn[i])].append(sy[i, :ns[i]].copy())
            for i in range(nsig):
                got_sig[int(sig[0][i])].append((int(sig[1][i]), float(sig[2][i]), float(sig[3][i])))
        while w < cap:
            w = min(cap, w + int(rng.integers(5 * N, 9 * N + 1)))
            j = k % 2
            d.register_signal_rows(sigs[j])
            n, c_ = d.receive(iq, w, prows[j], async_=3, depth=1)
            calls += c_
            if d.resident_active():
                resident_steps += 1
                pending.append(j)                                    # this call rang a step into prows[j] ...
                for pk_, sg_ in d.last_steps():                      # ... and reported the one rung a call ago
                    jj = pending.pop(0)
                    take(pk_, prows[jj], sigs[jj], sg_)
            else:
                take(n, prows[j], sigs[j], d.last_signals())        # an ordinary step (the first): its own rows, at once
            k += 1
        n, c_ = d.receive_flush(prows[k % 2])
        calls += c_
        steps = d.last_steps()
        assert len(steps) == len(pending) and not d.resident_active(), tag
        for pk_, sg_ in steps:
            jj = pending.pop(0)
            take(pk_, prows[jj], sigs[jj], sg_)
        take(n - sum(p for p, _ in steps), prows[k % 2], sigs[k % 2], 0)
        assert resident_steps >= 2, "%s: the resident kernel did not run" % tag
        for c in range(B):
            r = refs[c]
            where = "%s channel %d" % (tag, c)
            assert len(got[c]) == len(r["packets"]), "%s: %d packets, expected %d" % (where, len(got[c]), len(r["packets"]))
            for j, (a, (_, b)) in enumerate(zip(got[c], r["packets"])):
                assert np.array_equal(a, b), "%s packet %d: %r, expected %r" % (where, j, a.tolist(), b.tolist())
            want = int(sum(q["consumed"] for q in r["calls"]))
            assert d.consumed(c) == want, "%s consumed: %d, expected %d" % (where, d.consumed(c), want)
            assert [g[0] for g in got_sig[c]] == [int(q[0]) for q in r["signals"]], "%s sig_error" % where
            assert np.allclose([g[1:] for g in got_sig[c]], [q[1:] for q in r["signals"]], rtol=0, atol=2e-5, equal_nan=True), "%s sig_power / sig_snr" % where
        assert calls == sum(len(r["calls"]) for r in refs) == d.work_calls(), "%s work_calls" % tag
    finally:
        d.close()
