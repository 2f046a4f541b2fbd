"""GPU: ONE level-3 receiver walked through every way its frame state and open packets change hands (lorahip_demod_home.h) -- append
runs on the streaming kernels, the pipelined receiver, host-driven rounds, a deferred activate(), a resumed run, carry rows regrown,
the resident receiver, records dropped on the device -- with a packet open across each hand-over, beside the oracle's restated block
fed the same chunks, re-activated and given the new MTU at the same places.

Where a chunk ends is chosen from the oracle's own per-call states: at every hand-over at least one channel stands in DATASYMBOLS
with a symbol stored (the call before the boundary and the one after it both begin in DATASYMBOLS). After every step the read
positions are the oracle's -- except between resident steps, where lorahip_demod_consumed_all is refused by design (checked at their
flush) -- and the packets of all steps together are the oracle's, per channel, in order.

One hand-over has no packet open, on purpose: the one at which the MTU is raised (see there)."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import WorkResult, _i16p, _ptr
from test_gpu_demod import frames

pytestmark = pytest.mark.gpu
DATASYMBOLS = 4


class Block:
    """the oracle's LoRaDemod blocks, one per channel: `ops` is what happened to them so far; run() replays it from the start and then
    looks ahead to the end of the streams under the settings in force"""

    def __init__(self, orc, sf, host, mtu):
        self.orc, self.sf, self.host, self.ops, self.mtu0 = orc, sf, np.ascontiguousarray(host), [], mtu

    def run(self):
        L, N = self.orc.L, 1 << self.sf
        out = []
        for iq in self.host:
            d = L.lo_demod_new(self.sf)
            L.lo_demod_set_sync(d, 0x12); L.lo_demod_set_threshold(d, -30.0); L.lo_demod_set_mtu(d, self.mtu0)
            res, pkt, pos, packets, last, ahead = WorkResult(), np.zeros(256, np.int16), 0, [], None, []
            for op, v in self.ops + [("ahead", iq.size)]:
                if op == "activate":
                    L.lo_demod_activate(d)
                elif op == "mtu":
                    L.lo_demod_set_mtu(d, v)
                else:
                    if op == "ahead":
                        at = pos
                    while L.lo_demod_work(d, iq.ctypes.data + 8 * pos, v - pos, C.byref(res), None, None, _ptr(pkt, _i16p)) and res.consumed:
                        call = (pos, int(res.stateBefore), bool(res.packetPosted))
                        if op == "ahead":
                            ahead.append(call)
                        else:
                            last = call
                            if res.packetPosted:
                                packets.append(pkt[:res.packetLen].copy())
                        pos += res.consumed
            L.lo_demod_free(d)
            out.append(dict(pos=at, packets=packets, last=last, ahead=ahead))
        return out

    def boundary(self, w0, lo, hi, no_packets=False, outside=False):
        """the first fill level in [w0 + lo, w0 + hi] windows at which a channel is inside a packet with symbols stored (and, if asked,
        before which no channel completes a packet), and the channels that are. outside: at which NO channel has a packet's buffer (QUARTERCHIRP, DATASYMBOLS)."""
        N = 1 << self.sf
        now = self.run()
        for w in range(w0 + lo * N, min(w0 + hi * N, self.host.shape[1]) + 1, N // 2 + 5):
            inside, data, posted = [], 0, False
            for c, o in enumerate(now):
                calls = ([o["last"]] if o["last"] else []) + o["ahead"]
                i = 1 if o["last"] else 0
                while i < len(calls) and w - calls[i][0] >= 2 * N:       # LoRaDemod.cpp:148: the calls this fill level allows
                    posted = posted or calls[i][2]
                    i += 1
                data += i == len(calls) or calls[i][1] >= DATASYMBOLS - 1   # (QUARTERCHIRP: the packet's buffer exists already; behind the last call: not known)
                if 1 <= i < len(calls) and calls[i - 1][1] == DATASYMBOLS and not calls[i - 1][2] and calls[i][1] == DATASYMBOLS:
                    inside.append(c)
            if (data == 0) if outside else (inside and not (no_packets and posted)):
                return w, inside
        raise AssertionError("no fill level in [%d, %d] windows behind %d leaves a channel inside a packet (or, outside: none)" % (lo, hi, w0))


@pytest.mark.parametrize("sf,B", [(7, 5), (11, 3)])
def test_one_receiver_through_every_hand_over_with_a_packet_open(gpu, oracle, sf, B):
    import lora_sdr_amd as L
    rng = np.random.default_rng(1600 + sf)
    N = 1 << sf
    streams = [frames(oracle, rng, sf, 4, 18 + c, off=rng.uniform(-0.4, 0.4), noise=0.05, lead=N // 2 + 7 * N * c + int(rng.integers(0, N)))[0] for c in range(B)]
    cap = -(-max(s.size for s in streams) // 16) * 16              # rows of whole 128-byte lines: what the resident receiver asks for
    host = np.zeros((B, cap), np.complex64)
    for c, s in enumerate(streams):
        host[c, :s.size] = s
    iq = gpu.from_numpy(host).cuda()
    gpu.cuda.synchronize()
    blk = Block(oracle, sf, host, 6)
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(1); d.setMTU(6)
    rows = [d.receiver_rows(cap_packets=8 * B, stride=80) for _ in range(2)]
    got, w, walk = [[] for _ in range(B)], 0, []

    def take_rows(n, r, sync=True):
        if sync:
            gpu.cuda.synchronize()
        sy, ns, chn = r[0][:n].cpu().numpy(), r[1][:n].cpu().numpy(), r[2][:n].cpu().numpy()
        for i in range(n):
            got[int(chn[i])].append(sy[i, :ns[i]].copy())

    def take_queue():
        for c, _, s in d.packets():
            got[c].append(s)

    def advance(lo=2, hi=45, **kw):
        nonlocal w
        w, inside = blk.boundary(w, lo, hi, **kw)
        blk.ops.append(("feed", w))
        return inside

    def positions(step):
        want = [o["pos"] for o in blk.run()]
        assert d.consumed_all().tolist() == want, step
        walk.append(step)

    # 1. an append run on the streaming kernel; its records stay on the device, the open packets in the carry rows
    advance(); d.work_append(iq, w); positions("append run, mode 1")
    # 2. the pipelined receiver: the first call finds the records of (1) pending and takes an ordinary step, the next two are pipelined
    for k in range(3):
        advance()
        n, _ = d.receive(iq, w, rows[k & 1], async_=2)
        take_rows(n, rows[k & 1])
        positions("receive, async 2, call %d" % k)
    with pytest.raises(L.LoraHipError):
        d.packets()                                                 # steps are in flight
    # 3. flush
    n, _ = d.receive_flush(rows[1]); take_rows(n, rows[1]); positions("flush of the pipeline")
    # 4. host-driven rounds continue the streams: the mirrors are synced, the open packets fetched from the carry rows
    d.set_mode(2); advance(); d.work_append(iq, w); take_queue(); positions("append run, mode 2")
    # 5. activate() with a packet open: the reference block forgets the frame, not its fine-tune state
    d.activate(); blk.ops.append(("activate", None))
    # 6. the streaming kernel again, its record capacity so small that the run is resumed: the symbols pass through the mirrors
    d.set_mode(1); d.set_record_capacity(6)
    advance(lo=12); d.work_append(iq, w)
    assert d.last_launches() > 1
    take_queue(); positions("resumed append run, mode 1")
    d.set_record_capacity(0)
    # ... whose open packets, now in the mirrors alone, go up to the carry rows for an ordinary run. It ends where the oracle shows no
    # channel with a packet begun: the reference block sizes a packet's buffer by the MTU at DOWNCHIRP1 (LoRaDemod.cpp:260), so
    # raising the MTU under an open packet is a buffer overrun there, not a behaviour to compare with
    assert advance(outside=True) == []
    d.work_append(iq, w); take_queue(); positions("append run that ends outside every packet")
    # 7. packets longer than the 64 carry rows: the rows are regrown by the next run
    d.setMTU(70); blk.ops.append(("mtu", 70))
    # 8. the resident receiver: an ordinary step first (it regrows the rows), then steps the kernel takes
    pending, resident = [], []
    for k in range(4):
        advance()
        n, _ = d.receive(iq, w, rows[k & 1], async_=3)
        resident.append(d.resident_active())
        if resident[-1]:
            pending.append(k & 1)
            for pk_, _ in d.last_steps():
                take_rows(pk_, rows[pending.pop(0)], sync=False)    # (no device-wide wait while the kernel is resident)
        else:
            take_rows(n, rows[k & 1], sync=False)
            positions("receive, async 3, call %d (ordinary)" % k)
    assert resident == [False, True, True, True]
    # 9. flush
    n, _ = d.receive_flush(rows[0])
    steps = d.last_steps()
    assert not d.resident_active() and len(steps) == len(pending) == 1
    take_rows(steps[0][0], rows[pending.pop(0)]); take_rows(n - steps[0][0], rows[0])
    positions("flush of the resident receiver")
    # 10. a run that completes no packet, and its records dropped where they are: the open packets are in the carry rows
    inside = advance(no_packets=True); d.work_append(iq, w); positions("append run before clear_packets")
    d.clear_packets(); positions("clear_packets with records on the device")
    # 11. to the end of the streams
    w = cap; blk.ops.append(("feed", w)); d.work_append(iq, w); take_queue(); positions("last run")
    want = blk.run()
    for c in range(B):
        assert len(got[c]) == len(want[c]["packets"]) >= 1, "channel %d" % c      # (few: at MTU 70 and the default threshold a packet spans frames)
        assert all(np.array_equal(a, b) for a, b in zip(got[c], want[c]["packets"])), "channel %d" % c
    assert len(walk) == 13 and inside
    d.close()
