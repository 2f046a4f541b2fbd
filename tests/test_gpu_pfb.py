"""GPU: the polyphase filter-bank channeliser (lorahip_pfb_*). Its rows are by definition the direct-form
channeliser's for freq = bin / M, so the fp32 kernel is held to the same float64 definition (oracle/channelizer.py) within the same
tolerance, to the direct form on the device, to bit-exact chunk invariance, and to the property that matters: bytes sent through a
synthesised wideband stream of a uniform channel plan come back from every channel, with the packets the direct form yields."""
import ctypes as C

import numpy as np
import pytest

import synthesizer_def as sd

pytestmark = pytest.mark.gpu

# the project's channeliser tolerance (tests/test_gpu_channelizer.py): error <= TOL * sum|h| * max|x|. An fp32 simulation of this
# evaluation (serial fp32 branch sums, complex64 FFT) stays at 1e-9 .. 3e-8 of that scale for M = 8 .. 1024.
TOL = 4e-6


def _stream(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _tile(M):
    return max(16, min(256, 4096 // M))            # output times per workgroup: the streams below span more than two


def _taps(rng, D, L):
    from oracle import channelizer as oc
    h = oc.design_lowpass(D, L) if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)       # not symmetric: the tap order matters


def _bins(rng, M):
    if M <= 64:
        return None
    return np.concatenate([rng.permutation(M)[:16], [0, M // 2, M - 1]]).astype(np.int32)


def _shapes():
    out = []
    for log2m in range(3, 11):
        M = 1 << log2m
        for D in (M, 5 * M // 4, {8: 5, 16: 11, 32: 27, 64: 45, 128: 77, 256: 199, 512: 333, 1024: 1001}[M]):
            for L in (M // 2, 8 * M, 8 * M + 3):
                out.append((M, D, L))
    return out


@pytest.mark.parametrize("M,D,L", _shapes())
def test_against_float64_definition(gpu, M, D, L):
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    rng = np.random.default_rng(M * 10000 + D * 10 + L % 10)
    T = _tile(M)
    n = (2 * T + T // 3 + 1) * D + 7
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    bins = _bins(rng, M)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        got = pf.run(torch.from_numpy(x).cuda()).cpu().numpy()
        freqs = pf.freqs.copy()
        pf.close()
    assert np.array_equal(freqs, (np.arange(M) if bins is None else bins) / M)
    want = oc.channelize(x, freqs, D, h)
    assert got.shape == want.shape == (freqs.size, n // D)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(got - want).max())
    print("PFB accuracy M %d D %d L %d: err / scale %.3g" % (M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)
    # and it is not trivially small: the outputs carry signal
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(L))


@pytest.mark.parametrize("M,D,L,bins", [(16, 16, 128, None), (64, 64, 512, None), (32, 40, 256, [3, -3, 16, 0, 31, 7]), (128, 72, 600, [0, 1, 64, -1, 77])])
def test_against_the_direct_form_on_the_device(gpu, M, D, L, bins):
    """both are within TOL of one definition, so within 2 TOL of each other"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M + D)
    n = 5 * _tile(M) * D // 2 + 3
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        ch = Lh.Channelizer(ctx, pf.freqs, D, h)
        a = pf.run(xd).cpu().numpy()
        b = ch.run(xd).cpu().numpy()
        pf.close(); ch.close()
    assert a.shape == b.shape == (pf.n_channels, n // D)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(a - b).max())
    print("PFB vs direct form M %d D %d L %d: diff / scale %.3g" % (M, D, L, err / scale))
    assert err <= 2 * TOL * scale
    assert float(np.abs(b).max()) > 0.05 * scale / np.sqrt(L)


@pytest.mark.parametrize("M,D,L,n", [(32, 12, 100, 50000), (512, 640, 1000, 150000), (8, 3000, 70, 400000)])
def test_chunked_stream_is_bit_identical(gpu, M, D, L, n):
    """the ragged chunk list of tests/test_gpu_channelizer.py (pieces shorter than D, than the history, empty, long), with the input
    taken from the LDS copy (the first shape) and straight from memory (the others)"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(5)
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    bins = rng.integers(-M, 2 * M, 11).astype(np.int32)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        whole = pf.run(x).cpu().numpy()
        pf.reset()
        parts, pos = [], 0
        sizes = [1, 3, 0, 11, 12, 13, 1, 1, 1, 200, 5, 4096, 7, 111, 2, 10000]     # shorter than D, than the history, empty, long
        while pos < n:
            s = min(sizes[len(parts) % len(sizes)], n - pos)
            assert pf.out_count(s) == (pos + s) // D - pos // D
            parts.append(pf.run(x[pos:pos + s]).cpu().numpy())
            pos += s
        again = pf.run(x[:0])
        assert again.shape == (bins.size, 0)
        pf.reset()                                          # starts over, bit-identically
        once_more = pf.run(x).cpu().numpy()
        pf.close()
    glued = np.concatenate(parts, axis=1)
    assert glued.shape == whole.shape == (bins.size, n // D)
    assert np.array_equal(glued.view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(once_more.view(np.uint32), whole.view(np.uint32))
    assert float(np.abs(whole).max()) > 0.0


def test_layout_and_selection(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(11)
    M, D, L, n = 64, 80, 512, 40000
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    with Lh.Context(7) as ctx:
        full = Lh.PolyphaseChannelizer(ctx, M, D, h)
        assert full.n_channels == M and np.array_equal(full.freqs, np.arange(M) / M)
        tight = full.run(x)
        assert tight.shape == (M, n // D)
        # a column slice of a wider buffer: loose row stride, the columns outside stay as they were
        ring = torch.full((M, n // D + 37), 7.0 + 0j, dtype=torch.complex64, device="cuda")
        full.reset()
        got = full.run(x, out=ring[:, 5:])
        assert got.shape == tight.shape and got.data_ptr() == ring[:, 5:].data_ptr()
        assert torch.equal(ring[:, 5:5 + n // D], tight)
        assert bool((ring[:, :5] == 7.0).all()) and bool((ring[:, 5 + n // D:] == 7.0).all())
        full.close()
        # permuted, duplicate and negative bins; a subset equals the same rows of the full bank bit for bit
        bins = np.array([5, 63, -1, 0, 5, -64, 64 + 9, -32, 32, 17, -3 * 64 - 2], np.int32)
        sub = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        assert sub.n_channels == bins.size and np.array_equal(sub.freqs, bins / M)
        rows = sub.run(x)
        sub.close()
        assert torch.equal(rows, tight[torch.from_numpy(bins.astype(np.int64) % M).cuda()])
        assert torch.equal(rows[0], rows[4]) and torch.equal(rows[1], rows[2])
    assert float(tight.abs().max()) > 0.0


def test_phase_never_drifts(gpu):
    """a tone at a bin's centre comes out as DC of gain sum(h), also two billion samples into the stream: the phase is the stream
    position modulo M"""
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    M, D, L, b = 16, 8, 64, 3
    h = oc.design_lowpass(D, L)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, [b, b + 4])
        zeros = torch.zeros(1 << 24, dtype=torch.complex64, device="cuda")
        scratch = torch.empty((2, (1 << 24) // D), dtype=torch.complex64, device="cuda")
        n0 = 0
        for _ in range(128):
            pf.run(zeros, out=scratch)
            n0 += zeros.numel()
        assert n0 == 1 << 31
        n = 4096
        idx = np.arange(n, dtype=np.int64) + n0
        tone = np.exp(2j * np.pi * ((b * idx) % M) / M).astype(np.complex64)
        y = pf.run(torch.from_numpy(tone).cuda()).cpu().numpy()
        pf.close()
    settled = y[0, L // D + 1:]
    assert np.abs(settled - 1.0).max() < 2e-6            # sum(h) = 1, phase 0
    assert np.abs(y[1, L // D + 1:]).max() < 1e-3        # the bin a quarter of the band away sees only the stop band


def test_argument_checks_leave_the_stream_alone(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(3)
    h8 = np.ones(8, np.float32)
    M, D, L, n = 16, 20, 100, 9000
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    with Lh.Context(7) as ctx:
        for args in [(12, 4, h8), (4, 4, h8), (2048, 4, h8), (40, 4, h8), (16, 0, h8), (16, 4097, h8), (16, 4, np.zeros(0, np.float32)),
                     (16, 4, np.ones(65537, np.float32))]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseChannelizer(ctx, *args)
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseChannelizer(ctx, 16, 4, h8, bins=[])
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, [1, -2, 9])
        want = pf.run(x).cpu().numpy()
        pf.reset()
        cut = 3333
        first = pf.run(x[:cut]).cpu().numpy()
        lib = Lh.load()
        got = C.c_size_t()
        n_next = pf.out_count(n - cut)
        buf = torch.empty((3, n_next), dtype=torch.complex64, device="cuda")
        rest = x[cut:].contiguous()
        # no rows, rows too short, no input: each is refused with a reason, consumes nothing and leaves position and history alone
        for wide_p, out_p, stride in [(rest.data_ptr(), None, n_next), (rest.data_ptr(), buf.data_ptr(), n_next - 1), (None, buf.data_ptr(), n_next)]:
            rc = lib.lorahip_pfb_run(pf._h, C.c_void_p(wide_p) if wide_p else None, rest.numel(), C.c_void_p(out_p) if out_p else None, stride, C.byref(got))
            assert rc == -1
            assert lib.lorahip_last_error().decode().startswith("polyphase channeliser")
            assert pf.out_count(n - cut) == n_next
        with pytest.raises(ValueError):
            pf.run(rest, out=buf[:, :n_next - 1])
        with pytest.raises(ValueError):
            pf.run(rest.to(torch.complex128))
        second = pf.run(rest, out=buf).cpu().numpy()
        pf.close()
    glued = np.concatenate([first, second], axis=1)
    assert np.array_equal(glued.view(np.uint32), want.view(np.uint32))


def _receive(Lh, narrow, sf, mtu):
    d = Lh.LoRaDemod(sf, n_channels=narrow.shape[0]); d.set_mode(1); d.setMTU(mtu)
    d.work(narrow.contiguous())                                  # no host sync: the whole chain shares torch's stream
    pk = sorted(d.packets(), key=lambda p: p[0])
    d.close()
    return pk


def _decode(Lh, sf, cr, pk):
    dec = Lh.LoRaDecoder()
    dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True)
    out = dec.work([p[2] for p in pk])
    return out, dec.getDropped()


def _same_packets(a, b):
    return [(c, s.tolist()) for c, _, s in a] == [(c, s.tolist()) for c, _, s in b]


@pytest.mark.parametrize("sf,cr", [(7, "4/5"), (9, "4/8")])
def test_device_loopback_bytes_to_bytes(gpu, sf, cr):
    """Case A: the 8 even bins of M = 16 at D = 16 (channels two bandwidths apart), messages and near/far of the synthesiser's loopback:
    transmit -> Synthesizer(pf.freqs) -> AWGN -> PolyphaseChannelizer -> LoRaDemod -> LoRaDecoder (crc check and error check on) returns
    every channel's bytes and the packets the direct-form Channelizer yields from the same wideband stream; then the running form:
    ragged wideband pieces into a (K, capacity) buffer and work_segments."""
    import torch
    import lora_sdr_amd as Lh
    msgs, _, gains = sd.loopback_case(sf)
    M, K, U, L, N = 16, 8, 16, 128, 1 << sf
    bins = np.arange(-8, 8, 2)
    h = Lh.design_lowpass(U, L, cutoff=0.6 / U)
    rng = np.random.default_rng(200 + sf)
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        T = rows.shape[1]
        pf = Lh.PolyphaseChannelizer(ctx, M, U, h, bins)
        assert np.array_equal(pf.freqs, bins / 16.0)
        sy = Lh.Synthesizer(ctx, pf.freqs, U, U * h, gains)
        wide = sy.run(rows)
        sy.close()
        ctx.add_awgn(wide, 0.2, seed=3)
        narrow = pf.run(wide)
        assert narrow.shape == (K, T)
        pk = _receive(Lh, narrow, sf, mtu)
        assert [p[0] for p in pk] == list(range(K))
        out, dropped = _decode(Lh, sf, cr, pk)
        bad = [k for k, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
        assert not bad, "channels whose bytes did not come back: %s" % bad
        assert dropped == 0
        ch = Lh.Channelizer(ctx, pf.freqs, U, h)
        assert _same_packets(pk, _receive(Lh, ch.run(wide), sf, mtu))
        ch.close()
        # running
        pf.reset()
        cap = T + 8
        ring = torch.zeros((K, cap), dtype=torch.complex64, device="cuda")
        d = Lh.LoRaDemod(sf, n_channels=K); d.set_mode(1); d.setMTU(mtu)
        read = np.zeros(K, np.int64)
        w, fed, got = 0, 0, []
        while fed < wide.numel():
            n_in = min(wide.numel() - fed, int(rng.integers(U * N // 3, 5 * U * N)))
            o = pf.run(wide[fed:fed + n_in], out=ring[:, w:])
            fed += n_in
            w += o.shape[1]
            d.work_segments(ring, np.arange(K) * cap + read, w - read)
            got += d.packets()
            read += d.consumed_all()
        d.close(); pf.close()
        assert w == T
        assert torch.equal(ring[:, :w], narrow)
        assert _same_packets(sorted(got, key=lambda p: p[0]), pk)


def test_full_bank_loopback(gpu):
    """Case B: every bin of M = 32 carries a channel, 1.25 bandwidths apart (D = 40; D = 48 if the direct form does not return all 32
    messages at 40 -- the direct-form Channelizer on the same stream is the yardstick and decides whether the shape is a valid one). The
    filter bank's packets equal the direct form's, channel by channel, and decode to the bytes that were sent."""
    import lora_sdr_amd as Lh
    sf, cr, M, L = 7, "4/5", 32, 1024
    N = 1 << sf
    rng = np.random.default_rng(32)
    msgs = [rng.integers(0, 256, int(rng.integers(4, 25))).astype(np.uint8) for _ in range(M)]
    gains = 10.0 ** (-2.0 * (np.arange(M) % 4) / 20.0)          # 0 .. -6 dB between neighbours
    bins = np.arange(M) - M // 2
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        valid = None
        for D in (40, 48):
            h = Lh.design_lowpass(D, L, cutoff=0.5 / M)          # half way between a channel's edge and its neighbour's
            pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
            sy = Lh.Synthesizer(ctx, pf.freqs, D, D * h, gains)
            wide = sy.run(rows)
            sy.close()
            ctx.add_awgn(wide, 0.2, seed=3)
            ch = Lh.Channelizer(ctx, pf.freqs, D, h)
            ref_pk = _receive(Lh, ch.run(wide), sf, mtu)
            ch.close()
            out, dropped = _decode(Lh, sf, cr, ref_pk)
            ok = ([p[0] for p in ref_pk] == list(range(M)) and dropped == 0
                  and all(o is not None and np.array_equal(o, m) for o, m in zip(out, msgs)))
            print("full bank M 32, D %d: the direct form returns %s" % (D, "all 32 messages" if ok else "%d packets, not all messages" % len(ref_pk)))
            if ok:
                valid = D
                pk = _receive(Lh, pf.run(wide), sf, mtu)
                pf.close()
                break
            pf.close()
        assert valid is not None, "the direct form does not return all 32 messages at D = 40 or 48: not a valid shape"
        assert _same_packets(pk, ref_pk)
        out, dropped = _decode(Lh, sf, cr, pk)
        assert dropped == 0 and all(o is not None and np.array_equal(o, m) for o, m in zip(out, msgs))
