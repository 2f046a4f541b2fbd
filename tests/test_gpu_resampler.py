"""GPU: the rational-rate resampler (lorahip_resampler_*). Not a reference component: the fp32 kernel is held to the float64
restatement of its definition (tests/resampler_def.py, itself held to scipy and to the synthesiser's and channeliser's definitions in
tests/test_resampler_cpu.py) within a derived bound, to bit-exact chunk invariance, to the definition at stream positions beyond 2^33
and 2^40, to its layout and refusal rules, to the integer-input and non-finite rules, and to the property that matters: bytes ->
transmit -> synthesiser -> 6/5 -> noise -> 5/6 -> channeliser -> demodulator -> decoder -> the same bytes, every step on the device."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

import resampler_def as rd
import synthesizer_def as sd

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _rows(rng, K, n):
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def _taps(Lh, rng, U, D, L):
    """a low-pass made asymmetric by random factors: the tap order matters"""
    h = Lh.Resampler.design(U, D, L) if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)


def bound(U, L, scale):
    """T = ceil(L/U) fused multiply-adds per component, each ONE rounding of a partial sum that error_scale bounds; taps and inputs are
    exact in fp32: (T + 2) * 2^-24 * scale"""
    return (-(-L // U) + 2) * U24 * scale


def _all_outputs(x, U, D, h, n0=0):
    """the definition for every output of the samples n0 .. n0 + n - 1 (the selected-output form: no zero-stuffed convolution)"""
    n = x.shape[1]
    return rd.resample_at(x, U, D, h, m=range(n0 * U // D, (n0 + n) * U // D), n0=n0)


@pytest.mark.parametrize("K,U,D,L", [(1, 1, 1, 1), (1, 5, 6, 120), (3, 6, 5, 96), (9, 25, 24, 400), (2, 24, 25, 400), (1, 25, 256, 1000),
                                     (4, 128, 125, 640), (2, 4, 6, 48), (3, 7, 3, 4), (1, 1, 8, 64), (1, 8, 1, 64)])
def test_against_float64_definition(gpu, K, U, D, L):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(K * 1000 + U * 7 + D)
    n = int(20000 / max(1.0, U / D)) + 7
    x = _rows(rng, K, n)
    h = _taps(Lh, rng, U, D, L)
    want = _all_outputs(x, U, D, h)
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        assert rs.out_count(n) == rd.out_count(0, n, U, D) == n * U // D
        got = rs.run(torch.from_numpy(x).cuda()).cpu().numpy()
        rs.close()
    assert got.shape == want.shape == (K, n * U // D)
    scale = rd.error_scale(x, h, U)
    err = float(np.abs(got - want).max())
    print("resampler K=%d %d/%d L=%d: err/scale = %.3g (bound %.3g)" % (K, U, D, L, err / scale, bound(U, L, 1.0)))
    assert err <= bound(U, L, scale), (err, scale)
    # and it is not trivially small: the outputs carry signal
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(-(-L // U)))
    if L < U:
        p = ((np.arange(want.shape[1]) + 1) * D - 1) % U
        assert np.any(p >= L) and np.all(got[:, p >= L] == 0)          # phases without a tap: exact zeros
        assert np.all(got[:, p < L] != 0)


def test_one_row_takes_and_returns_1d(gpu):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(4)
    x = torch.from_numpy(_rows(rng, 1, 3000)).cuda()
    h = Lh.Resampler.design(5, 6, 120)
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, 5, 6, h)
        two = rs.run(x)
        rs.reset()
        one = rs.run(x[0])
        assert two.shape == (1, 2500) and one.shape == (2500,)
        assert torch.equal(one, two[0])
        with pytest.raises(ValueError):
            rs.run(x.real)
        rs.close()
        rs = Lh.Resampler(ctx, 5, 6, h, n_rows=2)
        with pytest.raises(ValueError):
            rs.run(x)                                                    # not n_rows rows
        rs.close()


SIZES = [1, 3, 0, 7, 8, 9, 1, 1, 1, 200, 5, 1023, 7, 111, 2, 2500]            # shorter than the history, empty, across tiles, long


@pytest.mark.parametrize("K,U,D,L,n,sizes", [(5, 25, 24, 400, 6000, SIZES), (2, 3, 7, 40, 700, [1, 2])])
def test_chunked_stream_is_bit_identical_and_reset_starts_over(gpu, K, U, D, L, n, sizes):
    """3/7 in pieces of 1 and 2 samples: most calls give 0 or 1 outputs"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(5)
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    h = _taps(Lh, rng, U, D, L)
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        whole = rs.run(x).cpu().numpy()
        assert whole.shape == (K, n * U // D)
        rs.reset()
        parts, pos, i, empty = [], 0, 0, 0
        while pos < n:
            s = min(sizes[i % len(sizes)], n - pos)
            i += 1
            count = rd.out_count(pos, s, U, D)
            assert rs.out_count(s) == count                                # right before every call
            part = rs.run(x[:, pos:pos + s])                               # a column slice: the row stride stays n
            assert part.shape == (K, count)
            empty += count == 0
            parts.append(part)
            pos += s
        assert empty > 0
        glued = torch.cat(parts, dim=1).cpu().numpy()
        assert glued.shape == whole.shape
        assert np.array_equal(bits(glued), bits(whole))
        rs.reset()                                                         # starts over: the first outputs again
        assert np.array_equal(bits(rs.run(x[:, :577]).cpu().numpy()), bits(whole[:, :577 * U // D]))
        rs.close()


@pytest.mark.parametrize("K,U,D,L,position", [(2, 25, 24, 400, 2 ** 33 + 3), (2, 125, 128, 1000, 2 ** 40 + 1), (1, 5, 6, 120, 2 ** 33 + 3)])
def test_deep_stream_position(gpu, K, U, D, L, position):
    """reset(position): the samples before it are zeros, the outputs and their count are the definition's at that n0 -- in two calls,
    so that the carried history is read at a deep position too"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(8)
    n = 5000
    x = _rows(rng, K, n)
    h = _taps(Lh, rng, U, D, L)
    want = _all_outputs(x, U, D, h, n0=position)
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        rs.run(torch.from_numpy(_rows(rng, K, 300)).cuda())                # something to forget
        rs.reset(position=position)
        xd = torch.from_numpy(x).cuda()
        assert rs.out_count(n) == rd.out_count(position, n, U, D)
        assert rs.out_count(1777) == rd.out_count(position, 1777, U, D)
        a = rs.run(xd[:, :1777])
        assert rs.out_count(n - 1777) == rd.out_count(position + 1777, n - 1777, U, D)
        b = rs.run(xd[:, 1777:])
        got = torch.cat([a, b], dim=1).cpu().numpy()
        rs.close()
    assert got.shape == want.shape == (K, rd.out_count(position, n, U, D))
    scale = rd.error_scale(x, h, U)
    err = float(np.abs(got - want).max())
    print("resampler %d/%d at position %d: err/scale = %.3g (bound %.3g)" % (U, D, position, err / scale, bound(U, L, 1.0)))
    assert err <= bound(U, L, scale), (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(-(-L // U))


@pytest.mark.parametrize("K", [1, 8, 9, 17])
def test_loose_strides_and_nothing_written_outside(gpu, K):
    """rows a column slice of a wider buffer, outputs into a column slice of a buffer filled with a pattern: the same bits as the tight
    run, and the pattern is intact behind n_out in every row, between the rows and behind the last row (5/6 with 120 taps groups
    8 rows a workgroup: K = 1, 8, 9, 17 stand on both sides of a group)"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(6 + K)
    U, D, L, n = 5, 6, 120, 3001
    x = torch.from_numpy(_rows(rng, K, n + 150)).cuda()
    h = _taps(Lh, rng, U, D, L)
    n_out = n * U // D
    stride = n_out + 40
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        loose_rows = x[:, 13:13 + n]
        assert K == 1 or loose_rows.stride(0) == n + 150
        tight = rs.run(loose_rows.contiguous())
        assert tight.shape == (K, n_out)
        rs.reset()
        flat = torch.full((K * stride + 100,), 7.0, dtype=torch.complex64, device="cuda")
        buf = flat[:K * stride].view(K, stride)
        given = rs.run(loose_rows, out=buf[:, 3:3 + n_out + 5])            # 5 columns of room behind n_out
        rs.close()
    assert given.shape == (K, n_out) and given.data_ptr() == flat.data_ptr() + 3 * 8
    assert torch.equal(given, tight)
    assert torch.equal(buf[:, 3:3 + n_out], tight)
    assert bool((buf[:, :3] == 7.0).all()) and bool((buf[:, 3 + n_out:] == 7.0).all()) and bool((flat[K * stride:] == 7.0).all())


@pytest.mark.parametrize("dtype,K,U,D,L", [("int16", 3, 25, 24, 400), ("int8", 2, 5, 6, 120), ("int16", 1, 1, 8, 64)])
def test_integer_rows_are_bit_identical_to_their_cf32_conversion(gpu, dtype, K, U, D, L):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(11)
    n = 4000
    info = np.iinfo(dtype)
    ints = rng.integers(info.min, info.max + 1, (K, n + 9, 2)).astype(dtype)
    h = _taps(Lh, rng, U, D, L)
    for scale in (None, 3.0e-3):
        s32 = np.float32(scale if scale is not None else (2.0 ** -15 if dtype == "int16" else 2.0 ** -7))
        conv = (s32 * ints.astype(np.float32)).astype(np.float32)          # one fp32 multiply per component
        x = torch.from_numpy(np.ascontiguousarray(conv).view(np.complex64)[..., 0]).cuda()
        di = torch.from_numpy(ints).cuda()
        with Lh.Context(7) as ctx:
            rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
            want = rs.run(x[:, 4:4 + n])
            rs.reset()
            parts, pos = [], 0
            for s in [5, 1, 0, 700, 33, 2000, n]:
                s = min(s, n - pos)
                parts.append(rs.run_int(di[:, 4 + pos:4 + pos + s], scale=scale))   # rows a slice: stride n + 9 samples
                pos += s
            assert pos == n
            got = torch.cat(parts, dim=1)
            # and the two kinds of call alternate freely on one stream
            rs.reset()
            mixed = torch.cat([rs.run_int(di[:, 4:4 + 1234], scale=scale), rs.run(x[:, 4 + 1234:4 + n])], dim=1)
            if K == 1:
                rs.reset()
                flat = rs.run_int(di[0, 4:4 + n], scale=scale)
                assert flat.shape == (n * U // D,) and torch.equal(flat, want[0])
            rs.close()
        assert got.shape == want.shape == (K, n * U // D)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
        assert np.array_equal(bits(mixed.cpu().numpy()), bits(want.cpu().numpy()))


def test_integer_argument_checks(gpu):
    import torch
    import lora_sdr_amd as Lh
    from lora_sdr_amd import _lib
    lib = Lh.load()
    rng = np.random.default_rng(12)
    n = 1000
    di = torch.from_numpy(rng.integers(-1000, 1000, (1, n, 2)).astype(np.int16)).cuda()
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, 5, 6, Lh.Resampler.design(5, 6, 120))
        first = rs.run_int(di[:, :400]).clone()
        got = C.c_size_t(123)

        def call(ptr, fmt, scale):
            return lib.lorahip_resampler_run_iq(rs._h, C.c_void_p(ptr), fmt, C.c_float(scale), n, 100, C.c_void_p(out.data_ptr()), n, C.byref(got))
        ptr = di.data_ptr() + 400 * 4
        for args, word in [((ptr + 2, _lib.IQ_SC16, 1.0), b"aligned"), ((ptr, 7, 1.0), b"format"), ((ptr, _lib.IQ_SC16, float("nan")), b"finite"),
                           ((ptr, _lib.IQ_SC16, float("inf")), b"finite"), ((ptr, _lib.IQ_CF32, 0.5), b"scale 1")]:
            assert call(*args) == -1, args
            assert got.value == 0
            text = lib.lorahip_last_error()
            assert text.startswith(b"resampler: ") and word in text, text
        with pytest.raises(ValueError):
            rs.run_int(di.float())
        with pytest.raises(ValueError):
            rs.run_int(di[:, :10], scale=float("nan"))
        assert rs.out_count(600) == rd.out_count(400, 600, 5, 6)           # nothing was consumed
        rest = rs.run_int(di[:, 400:])
        rs.reset()
        whole = rs.run_int(di)
        rs.close()
    assert np.array_equal(bits(torch.cat([first, rest], dim=1).cpu().numpy()), bits(whole.cpu().numpy()))


@pytest.mark.parametrize("K,U,D,L", [(3, 25, 24, 400), (2, 6, 5, 100), (2, 5, 16, 37), (2, 7, 3, 4)])
def test_nonfinite_samples_reach_exactly_the_outputs_of_the_rule(gpu, K, U, D, L):
    """a NaN and an Inf in row 1: the outputs m of row 1 with floor(t_m / U) - ceil(L / U) < c <= floor(t_m / U) are non-finite (the
    products with the zero padding of the taps are formed), every other output and every other row is bit-identical to the clean run,
    in one call and cut into pieces (one cut right behind the NaN: it then comes from the carried history)"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(13)
    n, c_nan, c_inf = 3000, 1501, 2222
    x = _rows(rng, K, n)
    h = _taps(Lh, rng, U, D, L)
    dirty = x.copy()
    dirty[1, c_nan] = np.nan
    dirty[1, c_inf] = np.inf
    hit = sorted(set(rd.nonfinite_outputs(c_nan, U, D, L, 0, n)) | set(rd.nonfinite_outputs(c_inf, U, D, L, 0, n)))
    assert hit
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        clean = rs.run(torch.from_numpy(x).cuda()).cpu().numpy()
        rs.reset()
        xd = torch.from_numpy(dirty).cuda()
        one = rs.run(xd).cpu().numpy()
        rs.reset()
        cut = torch.cat([rs.run(xd[:, :c_nan + 1]), rs.run(xd[:, c_nan + 1:c_inf]), rs.run(xd[:, c_inf:])], dim=1).cpu().numpy()
        rs.close()
    for got in (one, cut):
        bad = ~np.isfinite(got)
        assert not bad[0].any() and not bad[2:].any()
        p = ((np.array(hit) + 1) * D - 1) % U
        reached = np.array(hit)[p < L]                                     # a phase without a tap stays an exact zero
        assert sorted(np.flatnonzero(bad[1])) == sorted(reached)
        assert np.all(got[1, np.array(hit)[p >= L]] == 0)
        assert np.array_equal(bits(got[~bad]), bits(clean[~bad]))
    assert np.array_equal(bits(one), bits(cut))


def test_refusals_leave_the_stream_untouched(gpu):
    import torch
    import lora_sdr_amd as Lh
    lib = Lh.load()
    rng = np.random.default_rng(9)
    K, U, D, L, n = 3, 6, 5, 96, 2000
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    h = Lh.Resampler.design(U, D, L)
    with Lh.Context(7) as ctx:
        for bad in (dict(up=0), dict(down=0), dict(up=1025), dict(down=1025), dict(taps=np.zeros(0, np.float32)), dict(n_rows=0),
                    dict(up=1, down=1, taps=np.ones(65536, np.float32))):     # 65535 samples of history do not fit the LDS
            kw = dict(up=U, down=D, taps=h, n_rows=K); kw.update(bad)
            with pytest.raises(Lh.LoraHipError):
                Lh.Resampler(ctx, kw["up"], kw["down"], kw["taps"], kw["n_rows"])
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        whole = rs.run(x).cpu().numpy()
        rs.reset()
        first = rs.run(x[:, :701]).cpu().numpy()
        count = rs.out_count(500)
        out = torch.empty((K, n * 2), dtype=torch.complex64, device="cuda")
        got = C.c_size_t(123)
        xp, op = C.c_void_p(x.data_ptr() + 701 * 8), C.c_void_p(out.data_ptr())
        # a row stride shorter than the row, an output stride shorter than the count, missing pointers, more than 2^30 outputs
        # (by its arguments alone: the kernel is never launched): refused with a text, nothing consumed
        too_many = ((1 << 30) + 2) * D // U + 1
        for args, word in [((xp, 10, 11, op, n * 2), b"in_stride"), ((xp, n, 500, op, count - 1), b"out_stride"), ((None, n, 500, op, n * 2), b"NULL"),
                           ((xp, n, 500, None, n * 2), b"NULL"), ((xp, too_many, too_many, op, 1 << 31), b"2^30")]:
            assert lib.lorahip_resampler_run(rs._h, *args, C.byref(got)) == -1, word
            assert got.value == 0
            text = lib.lorahip_last_error()
            assert text.startswith(b"resampler: ") and word in text, text
            assert rs.out_count(500) == count
        with pytest.raises(Lh.LoraHipError):
            rs.reset(position=2 ** 52 + 1)
        assert rs.out_count(500) == count
        rest = rs.run(x[:, 701:]).cpu().numpy()
        rs.close()
    assert np.array_equal(bits(np.concatenate([first, rest], axis=1)), bits(whole))


def _receive(Lh, narrow, sf, mtu):
    d = Lh.LoRaDemod(sf, n_channels=narrow.shape[0]); d.set_mode(1); d.setMTU(mtu)
    d.work(narrow.contiguous())                                  # no host sync: the whole chain shares torch's stream
    pk = sorted(d.packets(), key=lambda p: p[0])
    d.close()
    return pk


def test_device_loopback_at_a_rate_off_the_grid(gpu):
    """SF7, 8 channels, one message of 4..24 random bytes each, frames starting 37 samples apart: transmit -> Synthesizer (16x) ->
    Resampler 6/5 (the "2.4 Msps" stream of a radio whose grid runs at 2 Msps) -> AWGN -> Resampler 5/6 -> Channelizer -> LoRaDemod ->
    LoRaDecoder (crc check and error check on) returns every channel's bytes. tests/test_resampler_cpu.py runs the same inputs through
    the float64 definitions."""
    import lora_sdr_amd as Lh
    sf, cr = 7, "4/5"
    msgs, freqs = rd.loopback_messages(sf), rd.LOOPBACK_FREQS
    K, U, N = 8, rd.LOOPBACK_INTERP, 1 << sf
    h = Lh.design_lowpass(U, rd.LOOPBACK_CHANNEL_TAPS, cutoff=0.6 / U)
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit([bytes(m) for m in msgs], sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        T = rows.shape[1]
        sy = Lh.Synthesizer(ctx, freqs, U, U * h)
        up = Lh.Resampler(ctx, 6, 5, Lh.Resampler.design(6, 5, rd.LOOPBACK_RESAMPLER_TAPS))
        down = Lh.Resampler(ctx, 5, 6, Lh.Resampler.design(5, 6, rd.LOOPBACK_RESAMPLER_TAPS))
        ch = Lh.Channelizer(ctx, freqs, U, h)
        wide = sy.run(rows)
        radio = up.run(wide)                                               # 1-D in, 1-D out
        assert radio.shape == (T * U * 6 // 5,)
        ctx.add_awgn(radio, rd.LOOPBACK_SIGMA, seed=3)
        back = down.run(radio)
        assert back.shape == (radio.numel() * 5 // 6,)
        narrow = ch.run(back)
        pk = _receive(Lh, narrow, sf, mtu)
        assert [p[0] for p in pk] == list(range(K))
        dec = Lh.LoRaDecoder()
        dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True)
        out = dec.work([p[2] for p in pk])
        bad = [k for k, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
        assert not bad, "channels whose bytes did not come back: %s" % bad
        assert dec.getDropped() == 0
        for o in (sy, up, down, ch):
            o.close()
