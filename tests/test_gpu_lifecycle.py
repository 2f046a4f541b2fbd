"""Create / use / destroy cycles of every owner of device memory in the library: what a cycle allocates, it gives back."""
import numpy as np
import pytest

from test_gpu_demod import frames

pytestmark = pytest.mark.gpu

MIB = 1 << 20
WARMUP, CYCLES = 3, 20
# Free device memory lost over CYCLES cycles by the library as it was BEFORE the owning handles (lorahip_own.h), measured with this
# test on one MI355X: 0 bytes (never negative either: the runtime keeps what the warm-up cycles made it reserve). The bound is that
# figure plus two 2 MiB allocation granules for the runtime's own bookkeeping.
PARENT_DRIFT = 0
BOUND = PARENT_DRIFT + 4 * MIB


def _cycle(L, torch, x_host, iq, host, wide, mixed_iq, expected):
    B, cap = iq.shape
    N = 128
    # Context: the host-pointer entry point (staging pair, the double-buffered upload)
    ctx = L.Context(7)
    out = ctx.detect_batch(x_host)
    assert len(out["sym"]) == x_host.shape[0]
    # Channelizer (borrows the context)
    ch = L.Channelizer(ctx, np.linspace(-0.4, 0.4, 64), 8, L.design_lowpass(8, 64))
    assert ch.run(wide).shape == (64, wide.numel() // 8)
    assert ch.run(wide).shape == (64, wide.numel() // 8)
    torch.cuda.synchronize()
    ch.close()
    ctx.close()
    # LoRaDetector (level 1: the mapped staging block)
    det = L.LoRaDetector(N)
    for i in range(N):
        det.feed(i, x_host[0, i])
    assert 0 <= det.detect()[0] < N
    det.close()
    # MixedDetector: a context, an offsets table and an event per bucket
    md = L.MixedDetector([7] * 2048 + [8] * 1024 + [9] * 512)
    md.plan(np.zeros(md.n_channels, np.int64), 32)
    md.detect(mixed_iq)
    md.plan(np.zeros(md.n_channels, np.int64), 64)                          # a second plan replaces the tables
    md.detect(mixed_iq)
    md.close()
    # LoRaDemod with the debug ports (few channels: the ports triple the traffic)
    dp = L.LoRaDemod(7, n_channels=8); dp.set_mode(1); dp.setMTU(9)
    dp.set_ports(fft_frames=96, dec_samples=cap, raw_samples=cap)
    dp.work(iq[:8].contiguous())
    assert dp.ports(0)["produced"]["fft"] > 0
    dp.close()
    # LoRaDemod, every way of running it
    d = L.LoRaDemod(7, n_channels=B); d.set_mode(1); d.setMTU(9)
    d.set_signals(True)
    d.work(iq)                                                              # a streaming run, with signals
    assert len(d.signals()[0]) >= expected                                  # (read first: the signals are cleared with the packets)
    assert len(d.packets()) == expected
    d.work(host)                                                            # from host streams: the owned upload buffer
    assert len(d.packets()) == expected
    d.set_signals(False)
    small, big = d.receiver_rows(cap_packets=2, stride=16), d.receiver_rows(cap_packets=expected + 64, stride=16)
    # pipelined steps (async = 2); refused calls on the way leave the object working
    d.rewind(); d.activate()
    got = refused = 0
    for k in range(1, 6):
        w = cap * k // 5
        try:
            n, _ = d.receive(iq, w, small, async_=2)                        # rows too small for what is due: refused, nothing lost
        except L.LoraHipError:
            refused += 1
            n, _ = d.receive(iq, w, big, async_=2)
        got += n
        if k == 3:
            with pytest.raises(L.LoraHipError):                             # a step is in flight
                d.work(iq)
            d.set_mode(2)
            with pytest.raises(L.LoraHipError):                             # a setting changed under the running pipeline
                d.receive(iq, w, big, async_=2)
            d.set_mode(1)
    try:
        n, _ = d.receive_flush(small)
    except L.LoraHipError:
        refused += 1
        n, _ = d.receive_flush(big)
    got += n
    assert got == expected and refused >= 1
    # resident steps (async = 3)
    rows = [big, d.receiver_rows(cap_packets=expected + 64, stride=16)]
    d.rewind(); d.activate()
    got = 0
    for k in range(1, 6):
        n, _ = d.receive(iq, cap * k // 5 & ~15, rows[k & 1], async_=3)
        got += n
        assert k == 1 or d.resident_active()                                # (the first call is an ordinary step)
    with pytest.raises(L.LoraHipError):                                     # the kernel is on the device
        d.work(iq)
    n, _ = d.receive_flush(rows[0])
    assert got + n == expected and not d.resident_active()
    d.rewind(); d.activate()
    d.work_append(iq, cap)                                                  # the flushed object is an ordinary one
    assert len(d.packets()) == expected
    torch.cuda.synchronize()
    held = torch.cuda.mem_get_info()[0]                                     # free memory with the large object still alive
    d.close()
    torch.cuda.synchronize()
    return held


def test_cycles_give_back_the_device_memory_they_take(gpu, oracle):
    """Every owner -- Context (host-pointer detect_batch), Channelizer, LoRaDetector, MixedDetector, LoRaDemod (streaming run with
    signals, run from host streams, debug ports, pipelined steps + flush, resident steps + flush; 4096 SF7 channels) -- is created, used
    until every lazily made resource exists, and destroyed; the large LoRaDemod alone must show as tens of MiB less free memory while it lives (measured: 248 MiB). After 3 warm-up cycles the free
    device memory (torch.cuda.mem_get_info) is read, 20 more cycles run, and it is read again: the loss may not exceed what the
    library lost before its buffers, events and streams were owned by handles (measured with this test: 0 bytes) plus 4 MiB. Measured
    with the handles: 0 bytes. One leaked buffer per cycle would show as 20 times its size.
    The test does not see leaked events, streams or a few bytes of pinned memory: those are covered by construction (no release call
    is left outside the handles). Calls that are refused on the way -- rows too small, a run or a changed setting while a pipelined or
    resident step is in flight -- leave the object working: every cycle still delivers every packet."""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(77)
    B, N = 4096, 128
    st, _ = frames(oracle, rng, 7, 2, 8)
    st = np.pad(st, (0, -st.size % 16))                                     # rows of whole 128-byte lines: what the resident mode asks for
    expected = len(oracle.demod_run(7, st, mtu=9)["packets"]) * B
    assert expected == 2 * B
    host = np.ascontiguousarray(np.broadcast_to(st, (B, st.size)))
    iq = torch.from_numpy(host).cuda()
    x_host = (rng.standard_normal((16384, N)) + 1j * rng.standard_normal((16384, N))).astype(np.complex64)
    wide = torch.from_numpy(x_host[:512].reshape(-1).copy()).cuda()
    mixed_iq = torch.from_numpy(x_host[:256].reshape(-1).copy()).cuda()     # 64 windows of SF9 from sample 0
    args = (L, torch, x_host, iq, host, wide, mixed_iq, expected)
    for _ in range(WARMUP):
        _cycle(*args)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    low = min(_cycle(*args) for _ in range(CYCLES))
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print("free device memory: %d -> %d bytes over %d cycles: lost %d bytes (%.2f MiB); bound %.2f MiB; the large object alone holds %.1f MiB"
          % (free0, free1, CYCLES, free0 - free1, (free0 - free1) / MIB, BOUND / MIB, (free0 - low) / MIB))
    assert free0 - low >= 32 * MIB, "the measurement would not see a leak: a live object does not show in the free memory"
    assert free0 - free1 <= BOUND
