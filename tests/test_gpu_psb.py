"""GPU: the polyphase synthesis filter bank (lorahip_psb_*). Its output is by definition the direct-form
synthesiser's for freq = bin / M, so the fp32 kernels are held to the same float64 definition (tests/synthesizer_def.py) within the
front ends' tolerance, to the direct form on the device, to bit-exact chunk invariance, to the definition's reach of a non-finite
sample, and to the property that matters: bytes sent through the bank come back from every channel of a polyphase receive bank, with
the packets the direct-form synthesiser yields.

err / error_scale as printed (`-s`) on an MI355X is tabulated in DESIGN.md section 8d."""
import ctypes as C

import numpy as np
import pytest

import synthesizer_def as sd

pytestmark = pytest.mark.gpu

# the project's front-end tolerance (tests/test_gpu_channelizer.py, tests/test_gpu_pfb.py), here relative to
# synthesizer_def.error_scale = max|x| sum|g| max_p sum_i |h[p + iU]|. A complex64 / float32 simulation of this evaluation stays at
# 2e-9 .. 4e-8 of that scale for M = 8 .. 1024.
TOL = 4e-6
ODD_U = {8: 5, 16: 11, 32: 27, 64: 45, 128: 77, 256: 199, 512: 333, 1024: 1001}
RAGGED = [1, 3, 0, 11, 12, 13, 1, 1, 1, 200, 5, 4096, 7, 111, 2, 10000]     # the size list of tests/test_gpu_pfb.py


def _rows(rng, K, n):
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def _tile(M):
    return max(8, min(256, 4096 // M))             # input times per workgroup of the transform: the streams below span more than two


def _taps(rng, U, L):
    import lora_sdr_amd as Lh
    h = Lh.design_lowpass(U, L, cutoff=0.37 / U) * U if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)       # not symmetric: the tap order matters


def _bins(rng, M):
    if M <= 64:
        return None
    return np.concatenate([rng.permutation(M)[:16], [0, M // 2, M - 1]]).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _err(got, x, freqs, U, h, gains, idx=None):
    """max|got - definition| / error_scale over the outputs idx (None: all), and max|definition| / error_scale"""
    idx = np.arange(x.shape[1] * U, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    want = sd.synthesize_at(x, freqs, U, h, gains, n=idx)
    scale = sd.error_scale(x, h, U, gains)
    return float(np.abs(got[idx] - want).max()) / scale, float(np.abs(want).max()) / scale


def _shapes():
    out = []
    for log2m in range(3, 11):
        M = 1 << log2m
        for U in (M, 5 * M // 4, ODD_U[M]):
            for L in ((U + 1) // 2, 8 * U, 8 * U + 3):
                out.append((M, U, L))
    return out


@pytest.mark.parametrize("M,U,L", _shapes())
def test_against_float64_definition(gpu, M, U, L):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M * 10000 + U * 10 + L % 10)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    bins = _bins(rng, M)
    K = M if bins is None else bins.size
    x = _rows(rng, K, n)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    I = -(-L // U)
    # every output where that is cheap; otherwise every phase of the first and last input times and of seeded others
    if n * U * I * K <= 1e7:
        idx = None
    else:
        m = np.unique(np.concatenate([np.arange(I + 2), np.arange(n - 3, n), rng.choice(n, max(8, int(1e7 / (U * I * K))), replace=False)]))
        idx = (m[m < n][:, None] * U + np.arange(U)[None, :]).reshape(-1)
    with Lh.Context(7) as ctx:
        for gains in (g, None):
            ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, gains)
            got = ps.run(xd).cpu().numpy()
            freqs = ps.freqs.copy()
            assert ps.n_channels == K and ps.out_count(n) == n * U
            ps.close()
            assert np.array_equal(freqs, (np.arange(M) if bins is None else bins) / M)
            assert got.shape == (n * U,)
            err, level = _err(got, x, freqs, U, h, gains, idx)
            print("PSB accuracy M %d U %d L %d %s: err / scale %.3g" % (M, U, L, "gains" if gains is not None else "no gains", err))
            assert err <= TOL, err
            assert level > 0.05 / max(1.0, np.sqrt(K * I))              # the outputs carry signal
            if L < U:
                assert np.all(_bits(got.reshape(n, U)[:, L:]) == 0)     # phases without a tap: exact (positive) zeros


@pytest.mark.parametrize("M,U,L,bins", [(16, 16, 128, None), (64, 64, 512, None), (32, 40, 256, [3, -3, 16, 0, 31, 7, 3 + 32]),
                                        (128, 72, 600, [0, 1, 64, -1, 77, 127])])
def test_against_the_direct_form_on_the_device(gpu, M, U, L, bins):
    """both are within TOL of one definition, so within 2 TOL of each other"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M + U)
    K = M if bins is None else len(bins)
    n = 5 * _tile(M) // 2 + 3
    x = _rows(rng, K, n)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        sy = Lh.Synthesizer(ctx, ps.freqs, U, h, g)
        a = ps.run(xd).cpu().numpy()
        b = sy.run(xd).cpu().numpy()
        ps.close(); sy.close()
    assert a.shape == b.shape == (n * U,)
    scale = sd.error_scale(x, h, U, g)
    err = float(np.abs(a - b).max())
    print("PSB vs direct form M %d U %d L %d: diff / scale %.3g" % (M, U, L, err / scale))
    assert err <= 2 * TOL * scale
    assert float(np.abs(b).max()) > 0.05 * scale / np.sqrt(K * (L // U))


# a small U; a history longer than a tile (ceil(L/U) - 1 = 199 > T = 8); a large U; calls longer than one segment of the workspace
# (4096 input times at M = 1024)
@pytest.mark.parametrize("M,U,L,n", [(32, 12, 100, 5000), (512, 5, 1000, 3000), (8, 3000, 7000, 500), (1024, 3, 20, 15000)])
def test_chunked_stream_is_bit_identical(gpu, M, U, L, n):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(5)
    bins = rng.integers(-M, 2 * M, 11).astype(np.int32)
    x = torch.from_numpy(_rows(rng, bins.size, n)).cuda()
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, bins.size).astype(np.float32)
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        whole = ps.run(x).cpu().numpy()
        ps.reset()
        parts, pos = [], 0
        while pos < n:
            s = min(RAGGED[len(parts) % len(RAGGED)], n - pos)
            assert ps.out_count(s) == s * U
            parts.append(ps.run(x[:, pos:pos + s]).cpu().numpy())
            assert parts[-1].shape == (s * U,)
            pos += s
        assert ps.run(x[:, :0]).shape == (0,)
        ps.reset()                                          # starts over, bit-identically
        once_more = ps.run(x).cpu().numpy()
        ps.close()
    glued = np.concatenate(parts)
    assert glued.shape == whole.shape == (n * U,)
    assert np.array_equal(_bits(glued), _bits(whole))
    assert np.array_equal(_bits(once_more), _bits(whole))
    idx = np.unique(np.concatenate([np.arange(min(n * U, 2000)), rng.choice(n * U, 2000), np.arange(n * U - 2000, n * U)]))
    err, level = _err(whole, x.cpu().numpy(), bins / M, U, h, g, idx)
    print("PSB chunks M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
    assert err <= TOL and level > 0.0


def test_one_channel_many_rows_and_the_interp_edges(gpu):
    """K = 1; 5000 rows on 16 bins (every bin sums some 300 rows: the float64 sum); U = 1; U = 4096 at the smallest and the largest
    M; L = 1; L = 65536 at a small U and at U = 4096"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(77)
    #        M     U     L      K     n      outputs compared
    cases = [(8, 8, 64, 1, 600, None),
             (16, 4, 32, 5000, 40, None),
             (128, 1, 9, 7, 300, None),
             (8, 4096, 8197, 8, 40, 6000),
             (1024, 4096, 8197, 19, 20, 6000),
             (16, 4, 1, 16, 100, None),
             (8, 3, 65536, 2, 22000, 150),
             (8, 4096, 65536, 3, 40, 6000)]
    with Lh.Context(7) as ctx:
        for M, U, L, K, n, pick in cases:
            bins = np.array([3]) if K == 1 else (None if K == M else rng.integers(-M, 2 * M, K))
            x = _rows(rng, K, n)
            h = _taps(rng, U, L) if L <= 8197 else (rng.uniform(-1.0, 1.0, L) * np.exp(-np.arange(L) / 2e4)).astype(np.float32)
            g = rng.uniform(0.25, 2.0, K).astype(np.float32)
            ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
            got = ps.run(torch.from_numpy(x).cuda()).cpu().numpy()
            ps.reset()
            cut = n // 3
            two = np.concatenate([ps.run(torch.from_numpy(x[:, :cut]).cuda()).cpu().numpy(), ps.run(torch.from_numpy(x[:, cut:]).cuda()).cpu().numpy()])
            freqs = ps.freqs.copy()
            ps.close()
            assert got.shape == (n * U,)
            assert np.array_equal(_bits(got), _bits(two))
            idx = None
            if pick is not None:                            # the first outputs, the last ones (the whole filter is in them) and seeded others
                idx = np.unique(np.concatenate([np.arange(pick // 3), np.arange(n * U - pick // 3, n * U), rng.choice(n * U, pick // 3)]))
            err, level = _err(got, x, freqs, U, h, g, idx)
            print("PSB edges M %d U %d L %d K %d: err / scale %.3g" % (M, U, L, K, err))
            assert err <= TOL, (M, U, L, K, err)
            assert level > 0.0


def test_layout_strides_and_calls_inside_a_tile(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(11)
    M, U, L, n = 64, 80, 512, 700
    bins = np.array([5, 63, -1, 0, 5, -64, 64 + 9, -32, 32, 17, -3 * 64 - 2], np.int32)
    K = bins.size
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    h = _taps(rng, U, L)
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins)
        assert ps.n_channels == K and np.array_equal(ps.freqs, bins / M) and np.array_equal(ps.bins, bins)
        tight = ps.run(x)
        assert tight.shape == (n * U,)
        # a column slice of a wider buffer (row stride larger than n_in), the output into a longer buffer that stays as it was behind
        ring = torch.full((K, n + 37), 7.0 + 0j, dtype=torch.complex64, device="cuda")
        ring[:, 5:5 + n] = x
        sink = torch.full((n * U + 9,), 3.0 + 0j, dtype=torch.complex64, device="cuda")
        ps.reset()
        got = ps.run(ring[:, 5:5 + n], out=sink)
        assert got.data_ptr() == sink.data_ptr() and torch.equal(got, tight) and bool((sink[n * U:] == 3.0).all())
        # calls that start and end inside a tile of 64 input times
        ps.reset()
        cuts = [0, 5, 7, 64, 65, 130, 190, 191, n]
        parts = [ps.run(x[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert torch.equal(torch.cat(parts), tight)
        ps.close()
        # rows that share a bin are summed: the same stream from the summed rows on distinct bins
        uniq = np.unique(bins % M)
        summed = torch.stack([x[torch.from_numpy(np.nonzero(bins % M == b)[0]).cuda()].sum(0) for b in uniq])
        one = Lh.PolyphaseSynthesizer(ctx, M, U, h, uniq)
        ref = one.run(summed).cpu().numpy()
        one.close()
    t = tight.cpu().numpy()
    scale = sd.error_scale(x.cpu().numpy(), h, U)
    assert float(np.abs(t - ref).max()) <= 2 * TOL * scale and float(np.abs(t).max()) > 0.0


def test_argument_checks_leave_the_stream_alone(gpu):
    """one step outside each limit is refused with a reason; a refused call consumes nothing and leaves position and history alone"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(3)
    h8 = np.ones(8, np.float32)
    M, U, L, n = 16, 20, 100, 900
    bins = [1, -2, 9]
    x = torch.from_numpy(_rows(rng, 3, n)).cuda()
    h = _taps(rng, U, L)
    lib = Lh.load()
    with Lh.Context(7) as ctx:
        for args in [(12, 4, h8), (4, 4, h8), (2048, 4, h8), (40, 4, h8), (16, 0, h8), (16, 4097, h8), (16, 4, np.zeros(0, np.float32)),
                     (16, 4, np.ones(65537, np.float32))]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseSynthesizer(ctx, *args)
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        for kw in [dict(bins=[]), dict(bins=[1, 2], gains=[1.0, np.inf]), dict(bins=[1, 2], gains=[np.nan, 1.0])]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseSynthesizer(ctx, 16, 4, h8, **kw)
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        Lh.PolyphaseSynthesizer(ctx, 8, 4096, np.ones(65536, np.float32), bins=[0]).close()      # the limits themselves are accepted
        Lh.PolyphaseSynthesizer(ctx, 1024, 1, np.ones(1, np.float32), bins=[0]).close()
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins)
        want = ps.run(x).cpu().numpy()
        ps.reset()
        cut = 333
        first = ps.run(x[:, :cut]).cpu().numpy()
        rest = x[:, cut:].contiguous()
        n_next = n - cut
        buf = torch.empty(n_next * U, dtype=torch.complex64, device="cuda")
        got = C.c_size_t(5)
        # no rows, no output, a row stride below n_in: each refused with a reason
        for in_p, out_p, stride in [(None, buf.data_ptr(), n_next), (rest.data_ptr(), None, n_next), (rest.data_ptr(), buf.data_ptr(), n_next - 1)]:
            rc = lib.lorahip_psb_run(ps._h, C.c_void_p(in_p) if in_p else None, stride, n_next, C.c_void_p(out_p) if out_p else None, C.byref(got))
            assert rc == -1 and got.value == 0
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        with pytest.raises(ValueError):
            ps.run(rest, out=buf[:n_next * U - 1])
        with pytest.raises(ValueError):
            ps.run(rest.to(torch.complex128))
        with pytest.raises(ValueError):
            ps.run(rest[:2])
        second = ps.run(rest, out=buf).cpu().numpy()
        ps.close()
        assert np.array_equal(_bits(np.concatenate([first, second])), _bits(want))
        # one input time beyond 2^30 outputs in one call: refused; 2^30 itself is a call's limit, not the stream's
        big = Lh.PolyphaseSynthesizer(ctx, 8, 4096, h8, bins=[0])
        rows = torch.zeros((1, (1 << 18) + 1), dtype=torch.complex64, device="cuda")
        rows[0, :4] = 1.0
        with pytest.raises(Lh.LoraHipError):
            big.run(rows)
        assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser: more than 2^30 outputs")
        y = big.run(rows[:, :4]).cpu().numpy()              # ... and the stream still starts at 0
        big.close()
    assert np.array_equal(y.reshape(4, 4096)[:, :8], np.ones((4, 8), np.complex64)) and not y.reshape(4, 4096)[:, 8:].any()


@pytest.mark.parametrize("M,U,L", [(16, 8, 61), (16, 8, 64)])
def test_non_finite_samples_reach_exactly_the_definitions_span(gpu, M, U, L):
    """a NaN, a +Inf and a -Inf in three rows, all taps non-zero: output n is non-finite exactly when m U <= n < m U + L for one of
    the bad input times m -- the definition's L outputs, not whole rounds of U --, and every other output is, bit for bit, what the
    stream gives with those three samples replaced by zeros. In one call, and with the NaN in the history of a later call."""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(6 + L)
    bins = np.array([0, 4, 7], np.int32)
    T = _tile(M)
    n = 3 * T + 11
    cut = T + 45
    x = _rows(rng, 3, n)
    clean = x.copy()
    at_nan, at_pinf, at_ninf = cut - 3, 2 * T - 1, 2 * T + 9       # in the second call's history; the last time of a tile; elsewhere
    x[0, at_nan] = np.float32("nan")
    x[1, at_pinf] = complex(np.float32("inf"), 1.0)
    x[2, at_ninf] = complex(0.5, -np.float32("inf"))
    for m in (at_nan, at_pinf, at_ninf):
        clean[:, m] = 0
    h = (Lh.design_lowpass(U, L) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    assert np.all(h != 0)
    nn = np.arange(n * U, dtype=np.int64)
    hit = np.zeros(n * U, bool)
    for m in (at_nan, at_pinf, at_ninf):
        hit |= (nn >= m * U) & (nn < m * U + L)
    want = sd.synthesize_at(x, bins / M, U, h, None, n=nn)
    assert np.array_equal(~np.isfinite(want), hit) and hit.sum() == 3 * L      # the definition itself: L outputs per sample
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins)
        whole = ps.run(xd).cpu().numpy()
        ps.reset()
        two = np.concatenate([ps.run(xd[:, :cut]).cpu().numpy(), ps.run(xd[:, cut:]).cpu().numpy()])
        ps.reset()
        base = ps.run(torch.from_numpy(clean).cuda()).cpu().numpy()
        ps.close()
    assert np.isfinite(base).all()
    # (the clean stream differs from the bad one in ALL rows of the three times, so away from them it is the same sum of the same terms)
    for y in (whole, two):
        bad = ~np.isfinite(y)
        print("PSB non-finite U=%d L=%d: %d non-finite outputs, %d by the definition" % (U, L, bad.sum(), hit.sum()))
        assert np.array_equal(bad, hit), (np.nonzero(bad != hit)[0][:10].tolist(), int(bad.sum()), int(hit.sum()))
        assert np.array_equal(_bits(y[~hit]), _bits(base[~hit]))
    err, _ = _err(base, clean, bins / M, U, h, None)
    assert err <= TOL


def _receive(Lh, narrow, sf, mtu):
    d = Lh.LoRaDemod(sf, n_channels=narrow.shape[0]); d.set_mode(1); d.setMTU(mtu)
    d.work(narrow.contiguous())
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


def _loopback(Lh, ctx, sf, cr, msgs, gains, M, U, L, bins, cutoff):
    """transmit rows -> PolyphaseSynthesizer -> AWGN -> PolyphaseChannelizer -> LoRaDemod -> LoRaDecoder: every channel's bytes come
    back, and the packets are those the direct-form Synthesizer yields on the same plan"""
    N = 1 << sf
    K = len(msgs)
    h = Lh.design_lowpass(U, L, cutoff=cutoff)
    enc = Lh.LoRaEncoder(ctx=ctx)
    enc.setSpreadFactor(sf); enc.setCodingRate(cr)
    mtu = enc.num_symbols(max(len(m) for m in msgs))
    iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
    rows = sd.stagger(iq)
    pf = Lh.PolyphaseChannelizer(ctx, M, U, h, bins)
    ps = Lh.PolyphaseSynthesizer(ctx, M, U, U * h, bins, gains)
    assert np.array_equal(ps.freqs, pf.freqs)
    sy = Lh.Synthesizer(ctx, pf.freqs, U, U * h, gains)
    packets = []
    for front in (ps, sy):
        wide = front.run(rows)
        assert wide.shape == (rows.shape[1] * U,)
        ctx.add_awgn(wide, 0.2, seed=3)
        pf.reset()
        packets.append(_receive(Lh, pf.run(wide), sf, mtu))
    ps.close(); sy.close(); pf.close()
    pk, ref_pk = packets
    assert [p[0] for p in pk] == list(range(K))
    out, dropped = _decode(Lh, sf, cr, pk)
    bad = [k for k, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
    assert not bad, "channels whose bytes did not come back: %s" % bad
    assert dropped == 0
    assert _same_packets(pk, ref_pk)


@pytest.mark.parametrize("sf,cr", [(7, "4/5"), (9, "4/8")])
def test_device_loopback_bytes_to_bytes(gpu, sf, cr):
    """Case A of DESIGN.md section 8c: the 8 even bins of M = 16 at U = D = 16 (channels two bandwidths apart), 0 .. -14 dB of near/far"""
    import lora_sdr_amd as Lh
    msgs, _, gains = sd.loopback_case(sf)
    with Lh.Context(sf) as ctx:
        _loopback(Lh, ctx, sf, cr, msgs, gains, 16, 16, 128, np.arange(-8, 8, 2), 0.6 / 16)


def test_full_bank_loopback(gpu):
    """Case B of DESIGN.md section 8c: every bin of M = 32 carries a channel, 1.5 bandwidths apart (U = D = 48, L = 1024), 0 .. -6 dB
    between neighbours"""
    import lora_sdr_amd as Lh
    sf, cr, M = 7, "4/5", 32
    rng = np.random.default_rng(32)
    msgs = [rng.integers(0, 256, int(rng.integers(4, 25))).astype(np.uint8) for _ in range(M)]
    gains = 10.0 ** (-2.0 * (np.arange(M) % 4) / 20.0)
    with Lh.Context(sf) as ctx:
        _loopback(Lh, ctx, sf, cr, msgs, gains, M, 48, 1024, np.arange(M) - M // 2, 0.5 / M)
