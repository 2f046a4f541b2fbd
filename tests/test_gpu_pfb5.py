"""GPU: the polyphase filter-bank channeliser on 5 * 2^a bins (lorahip_pfb_create_radix5, PolyphaseChannelizer.radix5 / .for_plan;
DESIGN.md section 8c), the bin counts of the LoRaWAN plans with 125 kHz channels 200 kHz apart (decim / n_bins = 8 / 5).

The rows are defined by the folded formula of include/lorahip.h with the exact phase b (n mod M) / M; tests/pfb_def.py restates it in
float64 and tests/test_pfb5_cpu.py holds that to oracle/channelizer.py for these M. Everything here is held to TOL = 4e-6 of
sum|h| max|x|, the project's channeliser tolerance (tests/test_gpu_pfb.py); an fp32 simulation of the evaluation stays at 6e-9 .. 1.1e-7
of that scale, so a case above 1e-6 would be a finding. err / scale of every accuracy case is printed (`-s`).

    what                                                                test
    7 bin counts x D = 8M/5, M, odd < M x L = M/2, 8M, 8M + 3, from     test_against_float64_definition
    the start of the stream (n - s < 0 in the first outputs)
    the direct form on the device, negative bins and bins beyond +-M    test_against_the_direct_form_on_the_device
    one call = cuts of 1 sample, less than the history, a ragged        test_chunked_stream_is_bit_identical
    length, the rest; reset and again; calls inside one tile
    column slice, duplicates, n_sel = 1 and 5000                        test_layout_and_selection
    both sides of the 80 KiB staging line (M = 40, 320), D = 1 and      test_shape_edges_against_float64_definition
    4096, L = 65536 (M = 5: 13108 rounds; M = 320)
    refusals leave the stream alone; the two constructors are disjoint  test_refusals_leave_the_stream_alone
    bytes -> transmit -> Synthesizer -> AWGN -> for_plan -> LoRaDemod   test_lorawan_plan_bytes_to_bytes
    -> LoRaDecoder on EU868 at 1 MHz (M = 5) and 8 channels at M = 40

The direct-form Channelizer takes no decim = 100 with 700 taps in one step (its tile of decim * (256 + n_taps / decim) samples,
210 400 bytes, does not fit the 160 KiB of a workgroup). Its outputs sit at n_m = (m + 1) D - 1 with the phase counted in input samples,
so the direct form at D = 100 is, by the definition in include/lorahip.h, every second output of the same object at decim = 50 (which
fits): _direct_form runs it that way for (160, 100, 700). The same shape is also held to the float64 definition in
test_shape_edges_against_float64_definition (the M = 160 row there).
"""
import ctypes as C

import numpy as np
import pytest

import pfb_def as pd
import synthesizer_def as sd
from test_gpu_channelizer_edges import definition_at, instance      # the float64 definition at chosen outputs; the direct form's rule
from test_gpu_pfb_edges import _compared                            # which outputs an edge shape compares

TOL = 4e-6              # of sum|h| * max|x|: the tolerance of tests/test_gpu_pfb.py
STAGE_LDS = 80 << 10
RADIX5 = (5, 10, 20, 40, 80, 160, 320)
ODD_D = {5: 3, 10: 7, 20: 13, 40: 27, 80: 51, 160: 119, 320: 273}      # odd, coprime to M, below it


def _stream(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def plan(M, D, L):
    """what lorahip_pfb_create_radix5 derives from a shape: T = the largest power of two with T M <= 4096 (16 at least, 256 at most),
    fold rounds Q, padded length Lp, the tile's input span, and whether that span is copied to the LDS: it is when it fits beside
    the sums (rows M + 1 apart) and the twiddles (M / 10 of the radix-2 part, M of the radix-5 stage) within 80 KiB"""
    M, D, L = int(M), int(D), int(L)
    T = max(16, min(256, 1 << ((4096 // M).bit_length() - 1)))
    Q = -(-L // M)
    Lp = Q * M
    fixed = (T * (M + 1) + M // 10 + M) * 8
    span = (T - 1) * D + Lp
    return dict(T=T, Q=Q, Lp=Lp, span=span, lds=fixed + 8 * span, staged=fixed + 8 * span <= STAGE_LDS)


def _last_staged_decim(M, L):
    return max(D for D in range(1, 4097) if plan(M, D, L)["staged"])


def _taps(rng, D, L):
    from oracle import channelizer as oc
    h = oc.design_lowpass(D, L) if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)       # not symmetric: the tap order matters


def _bins(rng, M):
    if M <= 80:
        return None
    return np.concatenate([rng.permutation(M)[:16], [0, M // 2, M - 1]]).astype(np.int32)


def test_tiles_and_the_staging_line_by_the_constructors_rule():
    assert [plan(M, 1, 1)["T"] for M in RADIX5] == [256, 256, 128, 64, 32, 16, 16]
    for M, L in ((40, 320), (320, 640)):
        D = _last_staged_decim(M, L)
        assert 1 < D < 4096
        assert plan(M, D, L)["lds"] <= STAGE_LDS < plan(M, D + 1, L)["lds"]
        assert plan(M, D, L)["staged"] and not plan(M, D + 1, L)["staged"]
    assert plan(5, 1, 37)["staged"] and not plan(5, 4096, 37)["staged"] and not plan(320, 4096, 700)["staged"]
    assert plan(5, 8, 65536)["Q"] == 13108 and plan(320, 320, 65536)["Q"] == 205


# ---------------------------------------------------------------------------------------------------------------------------
# against the float64 definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(M, D, L) for M in RADIX5 for D in (8 * M // 5, M, ODD_D[M]) for L in (max(1, M // 2), 8 * M, 8 * M + 3)])
def test_against_float64_definition(gpu, M, D, L):
    """two tiles and a third from the start of the stream: with D < M the first outputs have n_m - s < 0, L = M // 2 leaves residues
    without a tap, 8 M + 3 is no multiple of M, and M = 5 has no radix-2 stage"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M * 10000 + D * 10 + L % 10)
    T = plan(M, D, L)["T"]
    n = (2 * T + T // 3 + 1) * D + 7
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    bins = _bins(rng, M)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        got = pf.run(torch.from_numpy(x).cuda()).cpu().numpy()
        freqs = pf.freqs.copy()
        assert (pf.n_bins, pf.decim, pf.n_taps, pf.n_channels) == (M, D, L, M if bins is None else bins.size)
        pf.close()
    assert np.array_equal(freqs, (np.arange(M) if bins is None else bins) / M)
    want = pd.channelize(x, M, D, h, bins)
    assert got.shape == want.shape == (freqs.size, n // D)
    scale = pd.scale(x, h)
    err = float(np.abs(got - want).max())
    print("PFB5 accuracy M %d D %d L %d: err / scale %.3g" % (M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)
    # and it is not trivially small: the outputs carry signal
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(L))


def _direct_form_decim(D, L):
    """the decimation to give the direct-form Channelizer for outputs every D samples: D itself where its tile fits the LDS (the
    constructor's rule, `instance` of tests/test_gpu_channelizer_edges.py), otherwise D / f for the smallest f that divides D and
    fits. Output m' of decim = D / f sits at sample (m' + 1) D / f - 1 with the same taps and the same 64-bit phase, so the outputs
    m' = f m + f - 1 ARE the outputs m of decim = D: nothing is approximated. Returns (decim, f)."""
    for f in range(1, D + 1):
        if D % f == 0 and instance(D // f, L):
            return D // f, f
    raise ValueError("no divisor of decim = %d fits the direct form with %d taps" % (D, L))


def test_direct_form_decimation_by_the_constructors_rule():
    """the three shapes of test_against_the_direct_form_on_the_device: two run in one step, (100, 700) at decim = 50 keeping every
    second output; and the identity itself on the float64 oracle"""
    from oracle import channelizer as oc
    assert _direct_form_decim(16, 80) == (16, 1) and _direct_form_decim(64, 323) == (64, 1)
    assert instance(100, 700) == 0 and _direct_form_decim(100, 700) == (50, 2)
    rng = np.random.default_rng(2)
    x = _stream(rng, 100 * 9 + 57)
    h = _taps(rng, 100, 700)
    f = np.array([0.0, 1 / 160, -3 / 160, 0.5])
    assert np.array_equal(oc.channelize(x, f, 50, h)[:, 1::2], oc.channelize(x, f, 100, h))


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L,bins", [(10, 16, 80, [3, -3, 5, 0, 9, -10, 17, -21]), (40, 64, 323, [0, 1, 20, -1, -20, 39, 40 + 7, -2 * 40 - 3]),
                                        (160, 100, 700, [0, 1, 80, -1, 77, 160 + 5, -3 * 160 - 2])])
def test_against_the_direct_form_on_the_device(gpu, M, D, L, bins):
    """both are within TOL of one definition, so within 2 TOL of each other. Channelizer takes (100, 700) as decim = 50, of which
    every second output is the direct form at D = 100 (_direct_form_decim; the module's docstring)."""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M + D)
    n = 5 * plan(M, D, L)["T"] * D // 2 + 3
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        Dd, f = _direct_form_decim(D, L)
        ch = Lh.Channelizer(ctx, pf.freqs, Dd, h)
        a = pf.run(xd).cpu().numpy()
        b = ch.run(xd).cpu().numpy()[:, f - 1::f]
        pf.close(); ch.close()
    assert a.shape == b.shape == (len(bins), n // D)
    scale = pd.scale(x, h)
    err = float(np.abs(a - b).max())
    print("PFB5 vs direct form M %d D %d L %d: diff / scale %.3g" % (M, D, L, err / scale))
    assert err <= 2 * TOL * scale
    assert float(np.abs(b).max()) > 0.05 * scale / np.sqrt(L)


# ---------------------------------------------------------------------------------------------------------------------------
# chunk invariance, layout, selection
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(20, 7, 1), (40, 64, 323), (320, 512, 2560)])
def test_chunked_stream_is_bit_identical(gpu, M, D, L):
    """one call against cuts at 1 sample, fewer samples than the history, a length that is a multiple of neither M nor D nor T D, a
    run of short calls that start and end inside one tile, and the rest; reset() and the same again. Staged (the first two shapes)
    and from memory (the third)"""
    import torch
    import lora_sdr_amd as Lh
    pl = plan(M, D, L)
    assert pl["staged"] == (M != 320)
    T = pl["T"]
    rng = np.random.default_rng(5 + M)
    n = (3 * T + T // 3 + 1) * D + 7
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    bins = rng.integers(-M, 2 * M, 11).astype(np.int32)
    short = max(1, (pl["Lp"] - 1) // 2)                          # fewer than the Lp - 1 samples of history (1 where there are 19)
    ragged = T * D + D // 2 + 3
    while ragged % M == 0 or ragged % D == 0:
        ragged += 1
    sizes = [1, short, ragged, 0] + [2 * D + 1] * 3               # ... then three calls inside the second tile
    assert short < pl["Lp"] and ragged % (T * D) and sum(sizes) < n - T * D
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        whole = pf.run(x).cpu().numpy()
        for _ in range(2):
            pf.reset()
            parts, pos = [], 0
            for s in sizes + [n]:
                s = min(s, n - pos)
                assert pf.out_count(s) == (pos + s) // D - pos // D
                parts.append(pf.run(x[pos:pos + s]).cpu().numpy())
                pos += s
            assert pos == n
            glued = np.concatenate(parts, axis=1)
            assert glued.shape == whole.shape == (bins.size, n // D)
            assert np.array_equal(_bits(glued), _bits(whole))
        pf.close()
    assert float(np.abs(whole).max()) > 0.0


@pytest.mark.gpu
def test_layout_and_selection(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(11)
    M, D, L, n = 40, 64, 323, 20000
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    with Lh.Context(7) as ctx:
        full = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h)
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
        # permuted, duplicate and negative bins equal the same rows of the full bank bit for bit
        bins = np.array([5, 39, -1, 0, 5, -40, 40 + 9, -20, 20, 17, -3 * 40 - 2], np.int32)
        sub = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        assert sub.n_channels == bins.size and np.array_equal(sub.freqs, bins / M)
        rows = sub.run(x)
        sub.close()
        assert torch.equal(rows, tight[torch.from_numpy(bins.astype(np.int64) % M).cuda()])
        assert torch.equal(rows[0], rows[4]) and torch.equal(rows[1], rows[2])
        three = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, [-1, M - 1, 2 * M - 1])
        same = three.run(x)
        three.close()
        assert torch.equal(same[0], tight[M - 1]) and torch.equal(same[1], same[0]) and torch.equal(same[2], same[0])
        one = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, [M - 27])
        assert one.n_channels == 1
        assert torch.equal(one.run(x)[0], tight[M - 27])
        one.close()
        # 5000 seeded rows at M = 20: the store loop over many duplicate rows
        M2, D2, L2, n2 = 20, 32, 100, 32 * 300 + 5
        x2 = torch.from_numpy(_stream(rng, n2)).cuda()
        h2 = _taps(rng, D2, L2)
        full2 = Lh.PolyphaseChannelizer.radix5(ctx, M2, D2, h2)
        tight2 = full2.run(x2)
        full2.close()
        many = rng.integers(-3 * M2, 3 * M2, 5000).astype(np.int32)
        big = Lh.PolyphaseChannelizer.radix5(ctx, M2, D2, h2, many)
        rows2 = big.run(x2)
        big.close()
        assert rows2.shape == (5000, n2 // D2)
        assert torch.equal(rows2, tight2[torch.from_numpy(many.astype(np.int64) % M2).cuda()])
    assert float(tight.abs().max()) > 0.0 and float(tight2.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# edges of the shape limits
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_shapes():
    out = []
    for M, L in ((40, 320), (320, 640)):
        D = _last_staged_decim(M, L)
        out += [(M, D, L), (M, D + 1, L)]                         # the last D with the LDS copy, the first without
    out += [(5, 1, 37), (320, 1, 700), (5, 4096, 37), (320, 4096, 700)]
    out += [(5, 8, 65536), (320, 320, 65536)]                    # 13108 rounds; the longest filter at the largest M
    out += [(160, 100, 700)]                                     # the shape the direct form on the device refuses
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", _edge_shapes())
def test_shape_edges_against_float64_definition(gpu, M, D, L):
    """the first, the last, the tile-boundary and seeded other outputs (all where that is cheap) against the float64 definition at
    absolute indices with freqs = bins / M, and the stream in two calls, the first shorter than the history, bit for bit"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M * 100003 + D * 101 + L)
    pl = plan(M, D, L)
    T = pl["T"]
    n = max((2 * T + T // 3 + 1) * D + 7, L + (T + T // 3) * D + 7)
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    bins = np.arange(M, dtype=np.int32) if M == 5 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:5]]).astype(np.int32)
    xd = torch.from_numpy(x).cuda()
    first = max(1, min(pl["Lp"] // 2, n // 4))
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        whole = pf.run(xd).cpu().numpy()
        pf.reset()
        parts = [pf.run(xd[:first]).cpu().numpy(), pf.run(xd[first:]).cpu().numpy()]
        pf.close()
    assert whole.shape == (bins.size, n // D)
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    m = _compared(rng, n // D, T, L, bins.size)
    want = definition_at(x, 0, bins / float(M), D, h, m)
    scale = pd.scale(x, h)
    err = float(np.abs(whole[:, m] - want).max())
    print("PFB5 edges M %d D %d L %d (%s, %d rounds): err / scale %.3g, %d outputs x %d bins compared"
          % (M, D, L, "LDS copy" if pl["staged"] else "from memory", pl["Q"], err / scale, m.size, bins.size))
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(L))
    assert m[0] == 0 and m[-1] == n // D - 1 and (m[-1] + 1) * D - 1 >= L      # the start of the stream and a full filter are compared


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_stream_alone(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(3)
    h8 = np.ones(8, np.float32)
    M, D, L, n = 20, 32, 100, 9000
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    lib = Lh.load()
    with Lh.Context(7) as ctx:
        # the two constructors are disjoint, and the limits are those of lorahip_pfb_check_radix5
        for args in [(64, 4, h8), (8, 4, h8), (15, 4, h8), (640, 4, h8), (0, 4, h8), (40, 0, h8), (40, 4097, h8), (40, 4, np.zeros(0, np.float32)),
                     (40, 4, np.ones(65537, np.float32))]:
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseChannelizer.radix5(ctx, *args)
            assert lib.lorahip_last_error().decode().startswith("polyphase channeliser")
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseChannelizer.radix5(ctx, 40, 4, h8, bins=[])
        for M_old in (40, 24):
            with pytest.raises(Lh.LoraHipError):
                Lh.PolyphaseChannelizer(ctx, M_old, 4, h8)
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseChannelizer.for_plan(ctx, (24, 4, [0]), h8)
        undisturbed = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, [1, -2, 9])
        want = undisturbed.run(x).cpu().numpy()
        undisturbed.close()
        pf = Lh.PolyphaseChannelizer.for_plan(ctx, (M, D, [1, -2, 9]), h)
        cut = 3333
        first = pf.run(x[:cut]).cpu().numpy()
        got = C.c_size_t()
        n_next = pf.out_count(n - cut)
        buf = torch.empty((3, n_next), dtype=torch.complex64, device="cuda")
        rest = x[cut:].contiguous()
        # no rows, rows too short, no input, and more than 2^30 outputs (by count only: refused before anything is launched or read)
        for wide_p, n_in, out_p, stride, reason in [(rest.data_ptr(), rest.numel(), None, n_next, "no output rows"),
                                                    (rest.data_ptr(), rest.numel(), buf.data_ptr(), n_next - 1, "out_stride below"),
                                                    (None, rest.numel(), buf.data_ptr(), n_next, "no input"),
                                                    (rest.data_ptr(), ((1 << 30) + 2) * D, buf.data_ptr(), 1 << 31, "more than 2^30 outputs")]:
            rc = lib.lorahip_pfb_run(pf._h, C.c_void_p(wide_p) if wide_p else None, n_in, C.c_void_p(out_p) if out_p else None, stride, C.byref(got))
            assert rc == -1
            text = lib.lorahip_last_error().decode()
            assert text.startswith("polyphase channeliser") and reason in text, text
            assert pf.out_count(n - cut) == n_next
        with pytest.raises(ValueError):
            pf.run(rest, out=buf[:, :n_next - 1])
        second = pf.run(rest, out=buf).cpu().numpy()
        pf.close()
    glued = np.concatenate([first, second], axis=1)
    assert np.array_equal(_bits(glued), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: a LoRaWAN band plan, bytes to bytes
# ---------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.gpu
@pytest.mark.parametrize("fs,centre,channels", [(1e6, 868.3e6, 868.1e6 + 0.2e6 * np.arange(3)), (8e6, 867.9e6, 867.1e6 + 0.2e6 * np.arange(8))],
                         ids=["EU868-1MHz-M5", "8-channels-8MHz-M40"])
def test_lorawan_plan_bytes_to_bytes(gpu, fs, centre, channels):
    """125 kHz channels 200 kHz apart, SF7, coding rate 4/5, messages, near/far and noise of test_device_loopback_bytes_to_bytes in
    tests/test_gpu_pfb.py: transmit -> Synthesizer(bins / M, interp = D) -> AWGN -> PolyphaseChannelizer.for_plan -> LoRaDemod ->
    LoRaDecoder (crc check and error check on) returns every channel's bytes and the packets the direct-form Channelizer yields from
    the same wideband stream; then the running form: ragged wideband pieces into a (K, capacity) buffer and work_segments."""
    import torch
    import lora_sdr_amd as Lh
    sf, cr = 7, "4/5"
    N = 1 << sf
    plan_ = Lh.uniform_plan(fs, centre, channels)
    M, D, bins = plan_
    K = bins.size
    assert (M, D) == ((5, 8) if K == 3 else (40, 64)) and bins.tolist() == list(range(-(K // 2), K - K // 2))
    msgs, _, gains = sd.loopback_case(sf)
    msgs, gains = msgs[:K], gains[:K]
    Lt = 16 * D
    h = Lh.design_lowpass(D, Lt, cutoff=0.6 / D)
    rng = np.random.default_rng(200 + M)
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        T = rows.shape[1]
        pf = Lh.PolyphaseChannelizer.for_plan(ctx, plan_, h)
        assert np.array_equal(pf.freqs, bins / float(M)) and pf.n_bins == M and pf.decim == D
        sy = Lh.Synthesizer(ctx, pf.freqs, D, D * h, gains)
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
        ch = Lh.Channelizer(ctx, pf.freqs, D, h)
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
            n_in = min(wide.numel() - fed, int(rng.integers(D * N // 3, 5 * D * N)))
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
