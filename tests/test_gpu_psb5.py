"""GPU: the polyphase synthesis filter bank on 5 * 2^a bins (lorahip_psb_create_radix5, PolyphaseSynthesizer.radix5 / .for_plan;
DESIGN.md section 8d.1), the transmit side of the LoRaWAN plans with 125 kHz channels 200 kHz apart (interp / n_bins = 8 / 5).

The output is defined by the exact phase b (n mod M) / M (include/lorahip.h); tests/test_psb5_cpu.py holds that evaluation to
tests/synthesizer_def.py for these M to 1e-9 of the scale, so the yardstick here is synthesizer_def.synthesize_at(x, bins / M, U, h, g),
as in tests/test_gpu_psb.py, and the tolerance is the front ends' TOL = 4e-6 of synthesizer_def.error_scale. The power-of-two bank
measures 1e-8 .. 4e-8 of that scale; a case above 1e-6 would be a defect to look into, not something the tolerance is there to absorb.
err / scale of every accuracy case is printed (`-s`) and tabulated in DESIGN.md section 8d.1.

    what                                                                test
    7 bin counts x U = 8M/5, M, odd < M x L = ceil(U/2), 8U, 8U + 3,    test_against_float64_definition
    more than two tiles from the start of the stream, gains and none
    the direct form on the device, negative bins and bins beyond +-M    test_against_the_direct_form_on_the_device
    ragged calls, reset and again: L = 1, a history longer than a       test_chunked_stream_is_bit_identical
    tile, U = 3000 at M = 5, a call longer than a workspace segment
    column slice, out=, duplicate bins, n_sel = 1 and 5000              test_layout_and_selection
    a NaN and an Inf reach the definition's L outputs and no other      test_non_finite_samples_reach_exactly_the_definitions_span
    the two constructors are disjoint; refused runs leave the stream    test_refusals_leave_the_stream_alone
    bytes -> transmit -> for_plan -> AWGN -> PolyphaseChannelizer       test_lorawan_plan_bytes_to_bytes
    .for_plan -> LoRaDemod -> LoRaDecoder at M = 5, 40 and 320
"""
import ctypes as C

import numpy as np
import pytest

import synthesizer_def as sd
import test_gpu_psb as base                 # its helpers, tolerance and ragged size list; none of its tests

pytestmark = pytest.mark.gpu

TOL = base.TOL                              # 4e-6 of synthesizer_def.error_scale
RAGGED = base.RAGGED
RADIX5 = (5, 10, 20, 40, 80, 160, 320)
ODD_U = {5: 3, 10: 7, 20: 13, 40: 27, 80: 51, 160: 119, 320: 273}      # odd, coprime to M, below it
_rows, _taps, _bits, _err = base._rows, base._taps, base._bits, base._err


def _tile(M):
    """input times per workgroup of the transform (tests/test_psb5_cpu.py restates the constructor's rule)"""
    return max(8, min(256, 1 << ((4096 // M).bit_length() - 1)))


def _bins(rng, M):
    if M <= 80:
        return None
    return np.concatenate([rng.permutation(M)[:16], [0, M // 2, M - 1]]).astype(np.int32)


@pytest.mark.parametrize("M,U,L", [(M, U, L) for M in RADIX5 for U in (8 * M // 5, M, ODD_U[M]) for L in ((U + 1) // 2, 8 * U, 8 * U + 3)])
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
            ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, gains)
            got = ps.run(xd).cpu().numpy()
            freqs = ps.freqs.copy()
            assert (ps.n_bins, ps.interp, ps.n_taps, ps.n_channels) == (M, U, L, K) and ps.out_count(n) == n * U
            ps.close()
            assert np.array_equal(freqs, (np.arange(M) if bins is None else bins) / M)
            assert got.shape == (n * U,)
            err, level = _err(got, x, freqs, U, h, gains, idx)
            print("PSB5 accuracy M %d U %d L %d %s: err / scale %.3g" % (M, U, L, "gains" if gains is not None else "no gains", err))
            assert err <= TOL, err
            assert level > 0.05 / max(1.0, np.sqrt(K * I))              # the outputs carry signal
            if L < U:
                assert np.all(_bits(got.reshape(n, U)[:, L:]) == 0)     # phases without a tap: exact (positive) zeros


@pytest.mark.parametrize("M,U,L,bins", [(10, 16, 128, [3, -3, 5, 0, 9, -10, 17, -21]), (40, 64, 512, None),
                                        (160, 100, 700, [0, 1, 80, -1, 77, 165, -482])])
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
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        sy = Lh.Synthesizer(ctx, ps.freqs, U, h, g)
        a = ps.run(xd).cpu().numpy()
        b = sy.run(xd).cpu().numpy()
        ps.close(); sy.close()
    assert a.shape == b.shape == (n * U,)
    scale = sd.error_scale(x, h, U, g)
    err = float(np.abs(a - b).max())
    print("PSB5 vs direct form M %d U %d L %d: diff / scale %.3g" % (M, U, L, err / scale))
    assert err <= 2 * TOL * scale
    assert float(np.abs(b).max()) > 0.05 * scale / np.sqrt(K * (L // U))


# L = 1; a staged LoRaWAN shape; a history longer than a tile (ceil(L/U) - 1 = 199 > T = 8); a large U and no radix-2 stage; a call
# longer than one segment of the workspace (13107 input times at M = 320)
@pytest.mark.parametrize("M,U,L,n", [(20, 7, 1, 5000), (40, 64, 323, 3000), (320, 5, 1000, 3000), (5, 3000, 7000, 500), (320, 3, 20, 15000)])
def test_chunked_stream_is_bit_identical(gpu, M, U, L, n):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(5 + M)
    bins = rng.integers(-M, 2 * M, 11).astype(np.int32)
    x = torch.from_numpy(_rows(rng, bins.size, n)).cuda()
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, bins.size).astype(np.float32)
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        whole = ps.run(x).cpu().numpy()
        glued = []
        for _ in range(2):                                      # reset, and the same again
            ps.reset()
            parts, pos = [], 0
            while pos < n:
                s = min(RAGGED[len(parts) % len(RAGGED)], n - pos)
                assert ps.out_count(s) == s * U
                parts.append(ps.run(x[:, pos:pos + s]).cpu().numpy())
                assert parts[-1].shape == (s * U,)
                pos += s
            assert ps.run(x[:, :0]).shape == (0,)
            glued.append(np.concatenate(parts))
        ps.close()
    for y in glued:
        assert y.shape == whole.shape == (n * U,)
        assert np.array_equal(_bits(y), _bits(whole))
    idx = np.unique(np.concatenate([np.arange(min(n * U, 2000)), rng.choice(n * U, 2000), np.arange(n * U - 2000, n * U)]))
    err, level = _err(whole, x.cpu().numpy(), bins / M, U, h, g, idx)
    print("PSB5 chunks M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
    assert err <= TOL and level > 0.0


def test_layout_and_selection(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(11)
    M, U, L, n = 40, 64, 323, 300
    bins = np.array([5, 39, -1, 0, 5, -40, 40 + 9, -20, 20, 17, -3 * 40 - 2], np.int32)      # duplicate, negative, beyond +-M
    K = bins.size
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    h = _taps(rng, U, L)
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins)
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
        ps.close()
        err, level = _err(tight.cpu().numpy(), x.cpu().numpy(), bins / M, U, h, None)
        print("PSB5 duplicate, negative and far bins M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
        assert err <= TOL and level > 0.0
        # rows that share a bin are summed: [x, 0] and [0, x] on one bin are, bit for bit, the one row x (gains 1)
        one = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, [M - 27])
        assert one.n_channels == 1
        alone = one.run(x[:1])
        one.close()
        err, level = _err(alone.cpu().numpy(), x[:1].cpu().numpy(), np.array([M - 27]) / M, U, h, None)
        print("PSB5 one row M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
        assert err <= TOL and level > 0.0
        two = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, [M - 27, -27])
        zero = torch.zeros_like(x[:1])
        first = two.run(torch.cat([x[:1], zero]))
        two.reset()
        second = two.run(torch.cat([zero, x[:1]]))
        two.close()
        assert np.array_equal(_bits(first.cpu().numpy()), _bits(alone.cpu().numpy()))
        assert np.array_equal(_bits(second.cpu().numpy()), _bits(alone.cpu().numpy()))
        # 5000 seeded rows at M = 20 (every bin sums some 250 rows)
        M2, U2, L2, n2 = 20, 32, 100, 40
        many = rng.integers(-3 * M2, 3 * M2, 5000).astype(np.int32)
        x2 = _rows(rng, 5000, n2)
        h2 = _taps(rng, U2, L2)
        g2 = rng.uniform(0.25, 2.0, 5000).astype(np.float32)
        big = Lh.PolyphaseSynthesizer.radix5(ctx, M2, U2, h2, many, g2)
        y2 = big.run(torch.from_numpy(x2).cuda()).cpu().numpy()
        big.close()
        assert y2.shape == (n2 * U2,)
        err, level = _err(y2, x2, many / M2, U2, h2, g2)
        print("PSB5 5000 rows M %d U %d L %d: err / scale %.3g" % (M2, U2, L2, err))
        assert err <= TOL and level > 0.0


@pytest.mark.parametrize("M,U,L", [(5, 8, 67), (40, 64, 323)])
def test_non_finite_samples_reach_exactly_the_definitions_span(gpu, M, U, L):
    """one NaN and, in a second run, one Inf at x_k[m], m inside the second tile: the outputs m U .. m U + L - 1 are non-finite -- the
    definition's L outputs, not whole rounds of U --, and every other output is, bit for bit, that of the run without it (no other
    output has a term from input time m)"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(6 + L)
    bins = np.array([0, 2, -1], np.int32)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    m, k = T + 45, 1
    assert T < m < 2 * T and m * U + L < n * U
    x = _rows(rng, 3, n)
    h = _taps(rng, U, L)
    nn = np.arange(n * U, dtype=np.int64)
    hit = (nn >= m * U) & (nn < m * U + L)
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins)
        base_run = ps.run(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.isfinite(base_run).all()
        for bad_value in (complex(np.float32("nan"), 0.25), complex(1.0, -np.float32("inf"))):
            xb = x.copy()
            xb[k, m] = bad_value
            want = sd.synthesize_at(xb, bins / M, U, h, None, n=nn)
            assert np.array_equal(~np.isfinite(want), hit) and hit.sum() == L      # the definition itself: L outputs
            ps.reset()
            y = ps.run(torch.from_numpy(xb).cuda()).cpu().numpy()
            bad = ~np.isfinite(y)
            print("PSB5 non-finite M=%d U=%d L=%d: %d non-finite outputs, %d by the definition" % (M, U, L, bad.sum(), hit.sum()))
            assert np.array_equal(bad, hit), (np.nonzero(bad != hit)[0][:10].tolist(), int(bad.sum()), int(hit.sum()))
            assert np.array_equal(_bits(y[~hit]), _bits(base_run[~hit]))
        ps.close()
    err, _ = _err(base_run, x, bins / M, U, h, None)
    assert err <= TOL


def test_refusals_leave_the_stream_alone(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(3)
    h8 = np.ones(8, np.float32)
    M, U, L, n = 20, 32, 100, 900
    bins = [1, -2, 9]
    x = torch.from_numpy(_rows(rng, 3, n)).cuda()
    h = _taps(rng, U, L)
    lib = Lh.load()
    with Lh.Context(7) as ctx:
        # the two constructors are disjoint, and the limits are those of lorahip_psb_check_radix5
        for args in [(64, 4, h8), (8, 4, h8), (15, 4, h8), (640, 4, h8), (0, 4, h8), (40, 0, h8), (40, 4097, h8), (40, 4, np.zeros(0, np.float32)),
                     (40, 4, np.ones(65537, np.float32))]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseSynthesizer.radix5(ctx, *args)
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        for M_old in RADIX5 + (24,):
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseSynthesizer(ctx, M_old, 4, h8)
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseSynthesizer.for_plan(ctx, (24, 4, [0]), h8)
        for kw in [dict(bins=[]), dict(bins=[1, 2], gains=[1.0, np.inf]), dict(bins=[1, 2], gains=[np.nan, 1.0])]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseSynthesizer.radix5(ctx, 40, 4, h8, **kw)
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
        Lh.PolyphaseSynthesizer.radix5(ctx, 5, 4096, np.ones(65536, np.float32), bins=[0]).close()      # the limits themselves are accepted
        Lh.PolyphaseSynthesizer.for_plan(ctx, (320, 1, [0]), np.ones(1, np.float32)).close()
        undisturbed = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins)
        want = undisturbed.run(x).cpu().numpy()
        undisturbed.close()
        ps = Lh.PolyphaseSynthesizer.for_plan(ctx, (M, U, bins), h)
        cut = 333
        first = ps.run(x[:, :cut]).cpu().numpy()
        rest = x[:, cut:].contiguous()
        n_next = n - cut
        buf = torch.empty(n_next * U, dtype=torch.complex64, device="cuda")
        got = C.c_size_t(5)
        too_many = (1 << 30) // U + 1
        # no rows, no output, a row stride below n_in, and more than 2^30 outputs (by count only: refused before anything is launched or read)
        for in_p, out_p, stride, n_in, reason in [(None, buf.data_ptr(), n_next, n_next, "pointer is NULL"),
                                                  (rest.data_ptr(), None, n_next, n_next, "pointer is NULL"),
                                                  (rest.data_ptr(), buf.data_ptr(), n_next - 1, n_next, "in_stride"),
                                                  (rest.data_ptr(), buf.data_ptr(), too_many, too_many, "more than 2^30 outputs")]:
            rc = lib.lorahip_psb_run(ps._h, C.c_void_p(in_p) if in_p else None, stride, n_in, C.c_void_p(out_p) if out_p else None, C.byref(got))
            assert rc == -1 and got.value == 0
            text = lib.lorahip_last_error().decode()
            assert text.startswith("polyphase synthesiser") and reason in text, text
        with pytest.raises(ValueError):
            ps.run(rest, out=buf[:n_next * U - 1])
        second = ps.run(rest, out=buf).cpu().numpy()
        ps.close()
    assert np.array_equal(_bits(np.concatenate([first, second])), _bits(want))


PLANS = [(1e6, 868.3e6, 868.1e6 + 0.2e6 * np.arange(3), 5, 8), (8e6, 867.9e6, 867.1e6 + 0.2e6 * np.arange(8), 40, 64),
         (64e6, 867.9e6, 867.1e6 + 0.2e6 * np.arange(8), 320, 512)]


@pytest.mark.parametrize("fs,centre,channels,M,U", PLANS, ids=["EU868-1MHz-M5", "8-channels-8MHz-M40", "8-channels-64MHz-M320"])
def test_lorawan_plan_bytes_to_bytes(gpu, fs, centre, channels, M, U):
    """125 kHz channels 200 kHz apart, SF7, coding rate 4/5, the messages and near/far of synthesizer_def.loopback_case, taps and noise
    of tests/test_gpu_pfb5.py: uniform_plan -> transmit -> PolyphaseSynthesizer.for_plan -> AWGN -> PolyphaseChannelizer.for_plan ->
    LoRaDemod -> LoRaDecoder (crc check and error check on) returns every channel's bytes, and the packets are those the direct-form
    Synthesizer yields from the same rows -- where it takes the plan: interp = 512 (64 MHz) it refuses"""
    import lora_sdr_amd as Lh
    sf, cr = 7, "4/5"
    N = 1 << sf
    plan = Lh.uniform_plan(fs, centre, channels)
    n_bins, D, bins = plan
    K = bins.size
    assert (n_bins, D) == (M, U) and bins.tolist() == list(range(-(K // 2), K - K // 2))
    msgs, _, gains = sd.loopback_case(sf)
    msgs, gains = msgs[:K], gains[:K]
    h = Lh.design_lowpass(D, 16 * D, cutoff=0.6 / D)
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        pf = Lh.PolyphaseChannelizer.for_plan(ctx, plan, h)
        ps = Lh.PolyphaseSynthesizer.for_plan(ctx, plan, D * h, gains)
        assert np.array_equal(ps.freqs, pf.freqs) and np.array_equal(ps.freqs, bins / float(M)) and (ps.n_bins, ps.interp) == (M, U)
        fronts = [ps]
        if U <= 256:
            fronts.append(Lh.Synthesizer(ctx, pf.freqs, D, D * h, gains))
        else:
            with pytest.raises(Lh.LoraHipError):
                Lh.Synthesizer(ctx, pf.freqs, D, D * h, gains)
        packets = []
        for front in fronts:
            wide = front.run(rows)
            assert wide.shape == (rows.shape[1] * U,)
            ctx.add_awgn(wide, 0.2, seed=3)
            pf.reset()
            packets.append(base._receive(Lh, pf.run(wide), sf, mtu))
            front.close()
        pf.close()
        pk = packets[0]
        assert [p[0] for p in pk] == list(range(K))
        out, dropped = base._decode(Lh, sf, cr, pk)
        bad = [k for k, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
        assert not bad, "channels whose bytes did not come back: %s" % bad
        assert dropped == 0
        if len(packets) == 2:
            assert base._same_packets(pk, packets[1])
