"""GPU: the packet hand-off of a mixed-SF handle (lorahip_demod_create_mixed -> lorahip_demod_packets_to_device) and the device-resident
chain it opens: mixed receiver -> packets_device -> LoRaDecoderSet.decode_batch(index=channels, table=decoder of channel) -> bytes.
Everything compared is integer and exact: symbols, lengths, channel numbers, bytes."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_demod import frames

pytestmark = pytest.mark.gpu


def rows_by_channel(syms, nsyms, chan):
    """device rows -> {channel: [symbols of its rows, in row order]}"""
    syms, nsyms, chan = syms.cpu().numpy(), nsyms.cpu().numpy(), chan.cpu().numpy()
    out = {}
    for r in range(chan.size):
        assert 0 < nsyms[r] <= syms.shape[1] and not syms[r, nsyms[r]:].any()           # (zero padded behind the packet)
        out.setdefault(int(chan[r]), []).append(syms[r, :nsyms[r]].tolist())
    return out


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_handoff_lists_the_parts_in_queue_order_with_global_channels(gpu, oracle, devices):
    """19 channels with SF = 7 + c mod 6, two frames each, on one device slot and on two slots naming the same device: straight after the
    run (every part packs its rows on the device) and again after packets() has drained the records to the host (the host-queue path), the
    rows that carry a global channel are that channel's packets in order -- the host queue's and the reference's --, and the parts follow
    each other in the queue's order. Too few rows: LORAHIP_E_INVALID with the total in *n_packets."""
    import lora_sdr_amd as L
    rng = np.random.default_rng(1900 + len(devices))
    B = 19
    sfs = 7 + np.arange(B) % 6
    streams, want = [], []
    for c in range(B):
        sf = int(sfs[c])
        st, _ = frames(oracle, rng, sf, 2, 6 + c % 3, off=rng.uniform(-0.4, 0.4), noise=0.05, lead=int(rng.integers(0, 2 << sf)))
        streams.append(st)
        want.append([q.tolist() for _, q in oracle.demod_run(sf, st, mtu=7)["packets"]])
        assert len(want[-1]) == 2
    m = L.LoRaDemod(channel_sf=sfs, devices=devices)
    m.setMTU(7)
    slot = m.device_slot_of()
    bufs, first, cnt = [], np.zeros(B, np.int64), np.zeros(B, np.uint64)
    for s in range(len(devices)):
        at, parts = 5, [np.zeros(5, np.complex64)]
        for c in np.nonzero(slot == s)[0]:
            first[c], cnt[c] = at, streams[c].size
            parts.append(streams[c]); at += streams[c].size
        bufs.append(gpu.from_numpy(np.concatenate(parts)).cuda())
    if len(devices) == 1:
        m.work_segments(bufs[0], first, cnt)
    else:
        m.work_segments_multi(bufs, first, cnt)
    part_of = np.asarray(m.part_of)
    for path in ("device", "host queue"):
        ps, pn, pc = m.packets_device(clear=False)
        assert ps.shape == (2 * B, 8) and ps.device.index == 0
        got = rows_by_channel(ps, pn, pc)
        host = m.packets(clear=False)                               # (the first pass ends here: the records are on the host from now on)
        assert len(host) == 2 * B
        for c in range(B):
            assert got.get(c) == [q.tolist() for cc, _, q in host if cc == c] == want[c], (path, "channel", c)
        rows_part = part_of[pc.cpu().numpy()]
        assert (np.diff(rows_part) >= 0).all() and np.unique(rows_part).size == len(m.parts), path
        if path == "host queue":
            assert pc.cpu().tolist() == [cc for cc, _, _ in host]    # row for row the queue's own order
    # too few rows through the C entry point: refused, the total reported, nothing cleared
    n = 2 * B
    syms = gpu.zeros((n, 8), dtype=gpu.int16, device="cuda")
    ns, ch = gpu.zeros(n, dtype=gpu.int32, device="cuda"), gpu.zeros(n, dtype=gpu.int32, device="cuda")
    got_n = C.c_size_t(0)
    rc = m._lib.lorahip_demod_packets_to_device(m._h, C.c_void_p(syms.data_ptr()), 8, C.c_void_p(ns.data_ptr()), C.c_void_p(ch.data_ptr()), n - 1, C.byref(got_n))
    assert rc == -1 and got_n.value == n
    rc = m._lib.lorahip_demod_packets_to_device(m._h, C.c_void_p(syms.data_ptr()), 8, C.c_void_p(ns.data_ptr()), None, n, C.byref(got_n))
    assert rc == 0 and got_n.value == n                              # (channel_dev is optional, as on a plain handle)
    ps, pn, pc = m.packets_device()
    assert np.array_equal(ps.cpu().numpy(), syms.cpu().numpy()) and np.array_equal(pn.cpu().numpy(), ns.cpu().numpy())
    assert m.packets() == [] and m.packets_device()[0].shape[0] == 0
    m.close()


MTU = 64


def gateway_traffic(torch, rng):
    """12 channels, SF 7..12 x coding rate 4/5 and 4/8, two payloads of 5..20 bytes each: transmit() per channel at the noise of
    test_receive_chain_bytes_in_bytes_out (sigma 0.3), the two frames MTU + 4 silent symbols apart -> (channel_sf, coding rates, payloads, streams)"""
    import lora_sdr_amd as L
    sfs, crs, payloads, streams = [], [], [], []
    for sf in range(7, 13):
        for cr in ("4/5", "4/8"):
            N = 1 << sf
            sent = [rng.integers(0, 256, int(rng.integers(5, 21))).astype(np.uint8) for _ in range(2)]
            iq, nsyms = L.transmit(sent, sf=sf, cr=cr, padding=2, sigma=0.3, seed=5 + len(sfs), lead=N // 2 + 3, tail=(MTU + 4) * N)
            assert int(nsyms.max()) <= MTU and int(nsyms.min()) >= 8
            sfs.append(sf); crs.append(cr); payloads.append(sent); streams.append(iq.reshape(-1).contiguous())
    return np.array(sfs), crs, payloads, streams


def test_mixed_gateway_bytes_in_bytes_out(gpu, oracle):
    """bytes -> transmit() per (SF, rate) -> ONE mixed handle -> packets_device -> ONE LoRaDecoderSet launch whose table says "decoder of
    channel" -> every channel's payloads, all of them, in order. Nothing of the packets visits the host between the receiver and the bytes.
    Before that the reference alone (the oracle's demodulator and decoder on the CPU) must recover every payload from the same samples."""
    import lora_sdr_amd as L
    sfs, crs, payloads, streams = gateway_traffic(gpu, np.random.default_rng(2024))
    B = len(streams)
    for c in range(B):
        pk = oracle.demod_run(int(sfs[c]), streams[c].cpu().numpy(), mtu=MTU)["packets"]
        dec = [oracle.decode(int(sfs[c]), np.asarray(q).astype(np.uint16), cr=crs[c], crcc=True, error_check=True) for _, q in pk]
        assert [None if o is None else o.tolist() for o, _ in dec] == [p.tolist() for p in payloads[c]], ("the reference at this noise", c)
    buf = gpu.cat(streams)
    cnt = np.array([s.numel() for s in streams], np.uint64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    m = L.LoRaDemod(channel_sf=sfs, devices=[0])
    m.setMTU(MTU)
    m.work_segments(buf, first, cnt)
    syms, nsyms, chan = m.packets_device(stride=MTU)
    assert syms.shape == (2 * B, MTU)
    decoders = []
    for sf in range(7, 13):
        for cr in ("4/5", "4/8"):
            d = L.LoRaDecoder(); d.setSpreadFactor(sf); d.setCodingRate(cr); d.enableCrcc(True); d.enableErrorCheck(True)
            decoders.append(d)
    decoder_of_channel = gpu.arange(B, dtype=gpu.int32, device="cuda")      # channel c was sent at decoders[c]'s settings
    out, out_len, dropped = L.LoRaDecoderSet(decoders).decode_batch(syms, nsyms, index=chan, table=decoder_of_channel)
    out, out_len, dropped, chan = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy(), chan.cpu().numpy()
    assert int(dropped.sum()) == 0 and (out_len >= 5).all()
    for c in range(B):
        got = [out[r, :out_len[r]].tolist() for r in np.flatnonzero(chan == c)]
        assert got == [p.tolist() for p in payloads[c]], ("channel", c, "SF%d" % sfs[c], crs[c])
    m.close()


def test_a_refused_device_leaves_no_hip_error_behind(gpu):
    """a mixed handle over a device that does not exist is refused, and the parts made up to then are taken down without a HIP call on that
    device: the next launch of this thread reports its own outcome, not a stale 'invalid device'"""
    import lora_sdr_amd as L
    with pytest.raises(L.LoraHipError):
        L.LoRaDemod(channel_sf=[7, 8], devices=[99])
    dec = L.LoRaDecoder()
    dec.setSpreadFactor(7)
    assert dec.work([np.zeros(8, np.uint16)]) is not None
    d = L.LoRaDemod(7, n_channels=2)
    d.work(gpu.zeros((2, 1024), dtype=gpu.complex64, device="cuda"))
    assert d.packets() == []
    d.close()


def test_handoff_over_two_devices_is_refused(gpu):
    import lora_sdr_amd as L
    if L.device_count() < 2:
        pytest.skip("needs two GPUs: the rows of one decoder launch live on one device")
    m = L.LoRaDemod(channel_sf=[7, 8, 9, 10], devices=[0, 1])
    assert len(set(p[0] for p in m.parts)) == 2
    got = C.c_size_t(0)
    p = C.c_void_p(256)
    assert m._lib.lorahip_demod_packets_to_device(m._h, p, 8, p, p, 4, C.byref(got)) == -1
    assert b"one device" in m._lib.lorahip_last_error()
    m.close()
