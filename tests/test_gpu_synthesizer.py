"""GPU: the front-end synthesiser (lorahip_synthesizer_*), the channeliser's mirror image on the transmit side. Like the channeliser it
is not a reference component: the fp32 kernel is held to the float64 restatement of its definition (tests/synthesizer_def.py) within
a derived worst-case bound, to bit-exact chunk invariance (a stream cut into ragged pieces == one call, also two billion outputs into
the stream), and to the property that matters: bytes -> transmit -> synthesiser -> noise -> channeliser -> demodulator -> decoder ->
the same bytes, every step on the device, through ONE wideband stream."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

import synthesizer_def as sd

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _rows(rng, K, n):
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def bound(K, U, L, scale):
    """Worst-case forward bound of the fp32 evaluation: T = K * ceil(L/U) accumulated terms, one rounding per accumulation, plus per term
    the rounding of the coefficient, of the rotated input, of the mixer (~1e-7) and of the product: (T + 8) * 2^-24 * scale."""
    return (K * (-(-L // U)) + 8) * U24 * scale


@pytest.mark.parametrize("K,U,L", [(8, 8, 64), (3, 5, 37), (19, 16, 128), (1, 1, 1), (2, 1, 9), (9, 64, 256), (5, 72, 300), (4, 10, 3)])
def test_against_float64_definition(gpu, K, U, L):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(K * 1000 + U)
    n = max(2507, 20007 // U)
    x = _rows(rng, K, n)
    freqs = rng.uniform(-0.5, 0.5, K)
    freqs[0] = 0.0
    h = Lh.design_lowpass(U, L) * U if L > 1 else np.ones(1, np.float32)
    h = (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)          # not symmetric: the tap order matters
    gains = rng.uniform(0.25, 2.0, K).astype(np.float32)
    with Lh.Context(7) as ctx:
        for g in (gains, None):
            want = sd.synthesize(x, freqs, U, h, g)
            sy = Lh.Synthesizer(ctx, freqs, U, h, g)
            assert sy.out_count(n) == n * U
            got = sy.run(torch.from_numpy(x).cuda()).cpu().numpy()
            sy.close()
            assert got.shape == want.shape == (n * U,)
            scale = sd.error_scale(x, h, U, g)
            err = float(np.abs(got - want).max())
            print("synthesiser K=%d U=%d L=%d gains=%s: err/scale = %.3g (bound %.3g)" % (K, U, L, "yes" if g is not None else "none",
                                                                                            err / scale, bound(K, U, L, 1.0)))
            assert err <= bound(K, U, L, scale), (err, scale)
            # and it is not trivially small: the outputs carry signal
            assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(K * (-(-L // U))))
            if L < U:
                assert np.all(got.reshape(n, U)[:, L:] == 0)       # phases without a tap: exact zeros


def test_chunked_stream_is_bit_identical_and_reset_starts_over(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(5)
    K, U, L, n = 11, 12, 100, 6000
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    freqs = rng.uniform(-0.5, 0.5, K)
    h = Lh.design_lowpass(U, L) * U
    gains = rng.uniform(0.25, 2.0, K)
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h, gains)
        whole = sy.run(x).cpu().numpy()
        sy.reset()
        parts, pos = [], 0
        sizes = [1, 3, 0, 7, 8, 9, 1, 1, 1, 200, 5, 1023, 7, 111, 2, 2500]     # shorter than the history, empty, across tiles, long
        while pos < n:
            s = min(sizes[len(parts) % len(sizes)], n - pos)
            assert sy.out_count(s) == s * U
            parts.append(sy.run(x[:, pos:pos + s]).cpu().numpy())             # a column slice: the row stride stays n
            pos += s
        again = sy.run(x[:, :0])
        assert again.shape == (0,)
        glued = np.concatenate(parts)
        assert glued.shape == whole.shape
        assert np.array_equal(bits(glued), bits(whole))
        sy.reset()                                                             # starts over: the first outputs again
        assert np.array_equal(bits(sy.run(x[:, :777]).cpu().numpy()), bits(whole[:777 * U]))
        sy.close()


def test_loose_row_stride_equals_tight(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(6)
    K, U, L, n = 5, 16, 128, 3001
    x = torch.from_numpy(_rows(rng, K, n + 150)).cuda()
    freqs = rng.uniform(-0.5, 0.5, K)
    h = Lh.design_lowpass(U, L) * U
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h)
        loose_rows = x[:, 13:13 + n]
        assert loose_rows.stride(0) == n + 150
        loose = sy.run(loose_rows).cpu().numpy()
        sy.reset()
        tight = sy.run(loose_rows.contiguous()).cpu().numpy()
        sy.reset()
        out = torch.full((n * U + 5,), 7.0, dtype=torch.complex64, device="cuda")
        given = sy.run(loose_rows, out=out[1:])                                # an 8-byte aligned output: the narrow store path
        assert given.data_ptr() == out.data_ptr() + 8 and given.numel() == n * U
        assert out[0].item() == 7.0 and bool((out[n * U + 1:] == 7.0).all())
        sy.close()
    assert np.array_equal(bits(loose), bits(tight))
    assert np.array_equal(bits(given.cpu().numpy()), bits(tight))


def test_no_drift_two_billion_outputs_in(gpu):
    """zero rows in large chunks until the stream position passes 2^31 outputs, then a short block against the definition evaluated at
    absolute indices, under the same bound (a float phase accumulator would have lost the carriers long before)"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(8)
    K, U, L, n = 2, 16, 128, 300
    freqs = np.array([0.1234567, -0.3141592])
    h = (Lh.design_lowpass(U, L) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    gains = np.array([1.5, 0.5], np.float32)
    x = _rows(rng, K, n)
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h, gains)
        zeros = torch.zeros((K, 1 << 22), dtype=torch.complex64, device="cuda")
        out = torch.empty((1 << 22) * U, dtype=torch.complex64, device="cuda")
        n0 = 0
        for _ in range(33):
            sy.run(zeros, out=out)
            n0 += zeros.shape[1]
        assert n0 * U > 2 ** 31
        assert float(out.abs().max()) == 0.0                                   # zeros in, exact zeros out
        del out
        got = sy.run(torch.from_numpy(x).cuda()).cpu().numpy()
        sy.close()
    want = sd.synthesize(x, freqs, U, h, gains, n0=n0)
    scale = sd.error_scale(x, h, U, gains)
    err = float(np.abs(got - want).max())
    print("synthesiser no-drift at output %d: err/scale = %.3g (bound %.3g)" % (n0 * U, err / scale, bound(K, U, L, 1.0)))
    assert err <= bound(K, U, L, scale), (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(K * (L // U))


def test_argument_checks_leave_the_stream_untouched(gpu):
    import torch
    import lora_sdr_amd as Lh
    lib = Lh.load()
    rng = np.random.default_rng(9)
    h8 = np.ones(8, np.float32)
    K, U, L, n = 3, 8, 64, 2000
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    freqs = [0.0, 0.2, -0.3]
    h = Lh.design_lowpass(U, L) * U
    with Lh.Context(7) as ctx:
        for bad in (dict(interp=0), dict(interp=257), dict(freqs=[]), dict(taps=np.zeros(0, np.float32)),
                    dict(interp=1, taps=np.ones(65536, np.float32)),          # the tile does not fit the LDS
                    dict(gains=[float("nan")]), dict(gains=[float("inf")])):
            kw = dict(freqs=[0.0], interp=4, taps=h8, gains=None); kw.update(bad)
            with pytest.raises(Lh.LoraHipError):
                Lh.Synthesizer(ctx, kw["freqs"], kw["interp"], kw["taps"], kw["gains"])
        Lh.Synthesizer(ctx, [float("nan")], 4, h8).close()                     # a non-finite frequency counts as 0, as in phase_inc
        with pytest.raises(ValueError):
            Lh.Synthesizer(ctx, [0.0, 0.1], 4, h8, gains=[1.0])
        sy = Lh.Synthesizer(ctx, freqs, U, h)
        whole = sy.run(x).cpu().numpy()
        sy.reset()
        first = sy.run(x[:, :700]).cpu().numpy()
        out = torch.empty(n * U, dtype=torch.complex64, device="cuda")
        got = C.c_size_t(123)
        # a row stride shorter than the row, a missing pointer, more than 2^30 outputs: refused, nothing consumed
        assert lib.lorahip_synthesizer_run(sy._h, C.c_void_p(x.data_ptr()), 10, 11, C.c_void_p(out.data_ptr()), C.byref(got)) == -1
        assert got.value == 0
        assert lib.lorahip_synthesizer_run(sy._h, None, n, 5, C.c_void_p(out.data_ptr()), C.byref(got)) == -1
        assert lib.lorahip_synthesizer_run(sy._h, C.c_void_p(x.data_ptr()), n, 5, None, C.byref(got)) == -1
        too_many = (1 << 30) // U + 1
        assert lib.lorahip_synthesizer_run(sy._h, C.c_void_p(x.data_ptr()), too_many, too_many, C.c_void_p(out.data_ptr()), C.byref(got)) == -1
        assert b"2^30" in lib.lorahip_last_error()
        with pytest.raises(ValueError):
            sy.run(x[:2])                                                      # not K rows
        with pytest.raises(ValueError):
            sy.run(x.real)
        rest = sy.run(x[:, 700:]).cpu().numpy()
        sy.close()
    assert np.array_equal(bits(np.concatenate([first, rest])), bits(whole))


def _receive(Lh, ctx, narrow, sf, cr, mtu):
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


@pytest.mark.parametrize("sf,cr", [(7, "4/5"), (9, "4/8")])
def test_device_loopback_bytes_to_bytes(gpu, sf, cr):
    """8 channels, one message of 4..24 random bytes each, 0 .. -14 dB of near/far, frames starting 37 samples apart: transmit ->
    Synthesizer (16x) -> AWGN on the wideband stream -> Channelizer -> LoRaDemod -> LoRaDecoder (crc check and error check on) returns
    every channel's bytes; then the same with the wideband stream produced and consumed in ragged chunks (the running chain)."""
    import torch
    import lora_sdr_amd as Lh
    msgs, freqs, gains = sd.loopback_case(sf)
    K, U, L, N = 8, 16, 128, 1 << sf
    h = Lh.design_lowpass(U, L, cutoff=0.6 / U)
    rng = np.random.default_rng(100 + sf)
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        T = rows.shape[1]
        # one shot
        sy = Lh.Synthesizer(ctx, freqs, U, U * h, gains)
        wide = sy.run(rows)
        assert wide.shape == (T * U,)
        clean = wide.clone()
        ctx.add_awgn(wide, 0.2, seed=3)
        ch = Lh.Channelizer(ctx, freqs, U, h)
        narrow = ch.run(wide)
        assert narrow.shape == (K, T)
        pk = _receive(Lh, ctx, narrow, sf, cr, mtu)
        assert [p[0] for p in pk] == list(range(K))
        out, dropped = _decode(Lh, sf, cr, pk)
        bad = [k for k, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
        assert not bad, "channels whose bytes did not come back: %s" % bad
        assert dropped == 0
        # running: the rows go in in ragged pieces and make the same wideband stream, bit for bit; it gets the same noise; then it is
        # consumed in ragged pieces: the channeliser appends each piece's output to the columns of one (K, capacity) buffer and the
        # demodulator reads, per channel, what it has not consumed yet
        sy.reset(); ch.reset()
        wide2 = torch.empty(T * U, dtype=torch.complex64, device="cuda")
        fed = 0
        while fed < T:
            n_in = min(T - fed, int(rng.integers(N // 3, 5 * N)))
            piece = sy.run(rows[:, fed:fed + n_in], out=wide2[fed * U:])
            assert piece.numel() == n_in * U
            fed += n_in
        assert torch.equal(wide2, clean)                             # the chunked synthesiser is bit-identical (tested above too)
        ctx.add_awgn(wide2, 0.2, seed=3)
        cap = T + 8
        ring = torch.zeros((K, cap), dtype=torch.complex64, device="cuda")
        d = Lh.LoRaDemod(sf, n_channels=K); d.set_mode(1); d.setMTU(mtu)
        read = np.zeros(K, np.int64)
        w, fed, got = 0, 0, []
        while fed < wide2.numel():
            n_in = min(wide2.numel() - fed, int(rng.integers(U * N // 3, 5 * U * N)))
            o = ch.run(wide2[fed:fed + n_in], out=ring[:, w:])
            fed += n_in
            w += o.shape[1]
            d.work_segments(ring, np.arange(K) * cap + read, w - read)
            got += d.packets()
            read += d.consumed_all()
        d.close()
        assert w == T
        got = sorted(got, key=lambda p: p[0])
        assert [(c, s_.tolist()) for c, _, s_ in got] == [(c, s_.tolist()) for c, _, s_ in pk]     # the same packets
        out2, dropped2 = _decode(Lh, sf, cr, got)
        assert dropped2 == 0 and all(o is not None and np.array_equal(o, m) for o, m in zip(out2, msgs))
        sy.close(); ch.close()


def test_two_spreading_factors_in_one_stream(gpu):
    """rows 0-3 carry SF7 frames, rows 4-7 SF9 frames: one Synthesizer (it knows nothing about SFs), one Channelizer, two LoRaDemod
    objects on the row halves; all bytes come back"""
    import torch
    import lora_sdr_amd as Lh
    K, U, L, cr = 8, 16, 128, "4/8"
    rng = np.random.default_rng(79)
    msgs = [rng.integers(0, 256, int(rng.integers(4, 25))).astype(np.uint8) for _ in range(K)]
    freqs = (np.arange(K) - 3.5) * 0.1
    h = Lh.design_lowpass(U, L, cutoff=0.6 / U)
    halves, mtus = [], []
    ctxs = [Lh.Context(7), Lh.Context(9)]
    try:
        for ctx, sf, part in ((ctxs[0], 7, msgs[:4]), (ctxs[1], 9, msgs[4:])):
            N = 1 << sf
            enc = Lh.LoRaEncoder(ctx=ctx)
            enc.setSpreadFactor(sf); enc.setCodingRate(cr)
            mtus.append(enc.num_symbols(max(len(m) for m in part)))
            iq, _ = Lh.transmit([bytes(m) for m in part], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
            halves.append(iq)
        T = max(int(a.shape[1]) for a in halves)
        rows = torch.zeros((K, T), dtype=torch.complex64, device="cuda")
        rows[:4, :halves[0].shape[1]] = halves[0]
        rows[4:, :halves[1].shape[1]] = halves[1]
        ctx = ctxs[0]
        sy = Lh.Synthesizer(ctx, freqs, U, U * h)
        wide = sy.run(rows)
        ctx.add_awgn(wide, 0.2, seed=4)
        ch = Lh.Channelizer(ctx, freqs, U, h)
        narrow = ch.run(wide)
        sy.close(); ch.close()
        for sf, lo, mtu in ((7, 0, mtus[0]), (9, 4, mtus[1])):
            pk = _receive(Lh, ctx, narrow[lo:lo + 4], sf, cr, mtu)
            assert [p[0] for p in pk] == [0, 1, 2, 3], (sf, [p[0] for p in pk])
            out, dropped = _decode(Lh, sf, cr, pk)
            assert dropped == 0 and all(o is not None and np.array_equal(o, m) for o, m in zip(out, msgs[lo:lo + 4])), sf
    finally:
        for c in ctxs:
            c.close()
