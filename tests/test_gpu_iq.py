"""GPU: integer IQ input (sc16, sc8) of the receive front ends -- Channelizer.run_int / run_captures_int, PolyphaseChannelizer.run_int,
the *_run_iq entry points (include/lorahip.h). The definition is x[n] = scale * (float)(I[n], Q[n]) with one fp32
multiply per component and the cf32 definition after that, so there is no tolerance here: run_int(ints, scale) must give, bit for bit,
what the same object's run() gives on torch.view_as_complex(ints.float() * scale) -- for every kernel instance, chunking, alignment,
scale and mixture of formats on one stream. run() itself is held to its float64 definition by the tests of each front end. All
comparisons are on int32 views: identity means bits."""
import ctypes as C

import numpy as np
import pytest

import synthesizer_def as sd

pytestmark = pytest.mark.gpu

STAGE_LDS = 80 << 10
FORMATS = {"sc16": dict(dtype="int16", lo=-32768, hi=32767, scale=2.0 ** -15, code=1, bytes=4),
           "sc8": dict(dtype="int8", lo=-128, hi=127, scale=2.0 ** -7, code=2, bytes=2)}
# one shape per kernel instance: the direct form with two outputs a lane and with one (odd filter: the pad tap is in play), both radices
# of the polyphase bank with the tile's input staged in the LDS and read from memory (tests/test_gpu_pfb_edges.py pins D = 22 / 23 as
# the two sides of the 80 KiB line for M = 16, L = 128)
CASES = {"direct-rm2": dict(kind="direct", D=8, L=64, RM=2),
         "direct-rm1": dict(kind="direct", D=32, L=255, RM=1),
         "pfb-staged": dict(kind="pfb", M=16, D=16, L=128, staged=True),
         "pfb-unstaged": dict(kind="pfb", M=16, D=23, L=128, staged=False),
         "pfb5-staged": dict(kind="pfb5", M=10, D=16, L=83, staged=True),
         "pfb5-unstaged": dict(kind="pfb5", M=10, D=40, L=83, staged=False)}
DIRECT_FREQS = [0.0, -0.21, 0.13, 0.37, -0.05, 0.5, 0.25, -0.4, 0.031, -0.3, 0.44]      # 0, negative ones, K = 11: no multiple of 8
BINS = {16: [3, -3, 0, 8, 3], 10: [1, -2, 0, 5, 1]}                                      # a negative bin and a duplicate


def direct_plan(D, L):
    """the direct form's rule restated (lorahip_channelizer_create): filters in tap pairs, two output times a lane when the tile's
    input, split by decimation phase, fits 64 KiB of LDS, one otherwise; tile = 256 * RM outputs"""
    L = (L + 1) & ~1
    for RM in (2, 1):
        QP = (256 * RM + (L - 1) // D + 1) | 1
        if D * QP * 8 <= ((64 << 10) if RM == 2 else (160 << 10)):
            return dict(RM=RM, tile=256 * RM, hist=L - 1 + D)
    raise AssertionError("no instance")


def pfb_plan(M, D, L):
    """the polyphase bank's rule restated (pfbCreate, as tests/test_gpu_pfb5.py does): T = the largest power of two with T M <= 4096
    (16 at least, 256 at most); the tile's input span is copied to the LDS when fixed + 8 * span <= 80 KiB, fixed = the sums (rows
    M + 1 apart) and the twiddles (M / 2; 5 * 2^a: M / 10 + M)"""
    T = max(16, min(256, 1 << ((4096 // M).bit_length() - 1)))
    Lp = -(-L // M) * M
    tw = M // 2 if M & (M - 1) == 0 else M // 10 + M
    fixed = (T * (M + 1) + tw) * 8
    span = (T - 1) * D + Lp
    return dict(tile=T, hist=Lp - 1, staged=fixed + 8 * span <= STAGE_LDS)


def _plan(name):
    c = CASES[name]
    return direct_plan(c["D"], c["L"]) if c["kind"] == "direct" else pfb_plan(c["M"], c["D"], c["L"])


def _assert_path(name):
    """a changed plan rule fails here instead of silently testing one path twice"""
    c, p = CASES[name], _plan(name)
    if c["kind"] == "direct":
        assert p["RM"] == c["RM"], name
    else:
        assert p["staged"] == c["staged"], name
    assert pfb_plan(16, 22, 128)["staged"] and not pfb_plan(16, 23, 128)["staged"]
    assert len(DIRECT_FREQS) % 8 and 0.0 in DIRECT_FREQS and min(DIRECT_FREQS) < 0


def _taps(D, L):
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(1000 * D + L)
    return (Lh.design_lowpass(D, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)       # not symmetric: the tap order matters


def _make(ctx, name):
    import lora_sdr_amd as Lh
    c = CASES[name]
    h = _taps(c["D"], c["L"])
    if c["kind"] == "direct":
        return Lh.Channelizer(ctx, DIRECT_FREQS, c["D"], h)
    make = Lh.PolyphaseChannelizer if c["kind"] == "pfb" else Lh.PolyphaseChannelizer.radix5
    return make(ctx, c["M"], c["D"], h, BINS[c["M"]])


def _entry(name):
    """(the *_run_iq entry point, the prefix of its refusal texts)"""
    return ("lorahip_channelizer_run_iq", "channeliser") if CASES[name]["kind"] == "direct" else ("lorahip_pfb_run_iq", "polyphase channeliser")


def _length(name):
    """three tiles plus a ragged remainder, and no whole number of outputs"""
    return (3 * _plan(name)["tile"] + 37) * CASES[name]["D"] + 5


def _ints(fmt, n, seed):
    """(n, 2) random integers over the format's full range with the extremes planted, on the device"""
    import torch
    f = FORMATS[fmt]
    rng = np.random.default_rng(seed)
    a = rng.integers(f["lo"], f["hi"] + 1, (n, 2)).astype(f["dtype"])
    a[0], a[7], a[n // 2], a[n - 1] = (f["lo"], f["hi"]), (f["hi"], f["hi"]), (f["hi"], f["lo"]), (f["lo"], f["lo"])
    return torch.from_numpy(a).cuda()


def _cf32(ints, scale):
    """the reference side's input: the definition, evaluated by torch in fp32"""
    import torch
    return torch.view_as_complex((ints.float() * float(np.float32(scale))).contiguous())


def _same(a, b):
    import torch
    i32 = lambda t: torch.view_as_real(t.contiguous()).view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(i32(a), i32(b)))


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as Lh
    with Lh.Context(7) as c:
        yield c


@pytest.fixture(scope="module")
def refs(ctx):
    """(ints, want) of a shape and a format at the default scale, computed once: want = run() on the converted array"""
    cache = {}

    def get(name, fmt):
        if (name, fmt) not in cache:
            ints = _ints(fmt, _length(name), sorted(CASES).index(name) * 2 + FORMATS[fmt]["code"])
            obj = _make(ctx, name)
            want = obj.run(_cf32(ints, FORMATS[fmt]["scale"])).clone()
            obj.close()
            assert want.shape == (obj.n_channels, _length(name) // CASES[name]["D"])
            assert float(want.abs().max()) > 0.0
            cache[(name, fmt)] = (ints, want)
        return cache[(name, fmt)]
    return get


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identity_per_instance(ctx, refs, name, fmt):
    _assert_path(name)
    ints, want = refs(name, fmt)
    obj = _make(ctx, name)
    got = obj.run_int(ints)
    obj.close()
    assert _same(got, want)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_chunked_stream_is_bit_identical(ctx, refs, name, fmt):
    """ragged pieces: of 1 sample, shorter than a decimation step, shorter than the carried history, empty, one that ends inside a
    tile, long ones"""
    ints, want = refs(name, fmt)
    n, D, p = ints.shape[0], CASES[name]["D"], _plan(name)
    inside = p["tile"] * D + p["tile"] * D // 3                   # a piece this long from a tile's start ends inside the next tile
    sizes = [1, 1, 3, 0, p["hist"] - 1, D - 1, 1, p["hist"] // 2, 200, 5, inside, 7, 111, 2, 2 * p["tile"] * D + 11]
    assert min(s for s in sizes if s) == 1 and 0 < p["hist"] - 1 < p["hist"] and inside % (p["tile"] * D)
    obj = _make(ctx, name)
    whole = obj.run_int(ints).clone()
    obj.reset()
    parts, pos = [], 0
    while pos < n:
        s = min(sizes[len(parts) % len(sizes)], n - pos)
        assert obj.out_count(s) == (pos + s) // D - pos // D
        parts.append(obj.run_int(ints[pos:pos + s]).clone())
        pos += s
    obj.close()
    import torch
    glued = torch.cat(parts, dim=1)
    assert _same(glued, whole)
    assert _same(glued, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_formats_mix_freely_on_one_stream(ctx, name):
    """pieces alternately as sc16, cf32 (run) and sc8: the carried history is cf32, so the stream is the all-cf32 stream. The sc16 values
    are 64 times the sc8 ones and the sc8 scale 64 times the sc16 one (a power of two: the same floats)."""
    import torch
    n, D, p = _length(name), CASES[name]["D"], _plan(name)
    i8 = _ints("sc8", n, 77)
    i16 = i8.to(torch.int16) * 64
    s16 = 0.0123 / 64
    s8 = float(np.float32(s16)) * 64
    x = _cf32(i8, s8)
    assert _same(x, _cf32(i16, s16))
    obj = _make(ctx, name)
    want = obj.run(x).clone()
    obj.reset()
    sizes = [p["hist"] // 2, 1, p["tile"] * D + 3, D - 1, 5, 333, 2 * D, 1, 1]
    parts, pos = [], 0
    while pos < n:
        s = min(sizes[len(parts) % len(sizes)], n - pos)
        how = len(parts) % 3
        if how == 0:
            parts.append(obj.run_int(i16[pos:pos + s], scale=s16).clone())
        elif how == 1:
            parts.append(obj.run(x[pos:pos + s]).clone())
        else:
            parts.append(obj.run_int(i8[pos:pos + s], scale=s8).clone())
        pos += s
    obj.close()
    assert len(parts) >= 9
    assert _same(torch.cat(parts, dim=1), want)


@pytest.mark.parametrize("fmt,skip", [("sc16", 1), ("sc8", 1), ("sc8", 3)])
@pytest.mark.parametrize("name", ["direct-rm2", "direct-rm1", "pfb-staged", "pfb-unstaged"])
def test_alignment_to_the_sample_size_is_enough(ctx, refs, name, fmt, skip):
    """wide = buf[skip:] of a larger tensor, as a ring buffer presents it: sc16 4-byte aligned but not 8, sc8 2-byte aligned but not 4"""
    import torch
    ints, want = refs(name, fmt)
    buf = torch.zeros((ints.shape[0] + 8, 2), dtype=ints.dtype, device="cuda")
    wide = buf[skip:skip + ints.shape[0]]
    wide.copy_(ints)
    size = FORMATS[fmt]["bytes"]
    assert buf.data_ptr() % 16 == 0 and wide.data_ptr() % size == 0 and wide.data_ptr() % (2 * size) == size
    obj = _make(ctx, name)
    aligned = obj.run_int(ints.clone()).clone()
    obj.reset()
    got = obj.run_int(wide)
    obj.close()
    assert _same(got, aligned)
    assert _same(got, want)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", ["direct-rm2", "pfb-unstaged", "pfb5-staged"])
def test_scales(ctx, refs, name, fmt):
    """the default, one that is no power of two, a negative one, and 0: the reference's output on that all-zero array, signed zeros
    included"""
    import torch
    ints, want = refs(name, fmt)
    obj = _make(ctx, name)
    assert _same(obj.run_int(ints, scale=None), want)
    for scale in (FORMATS[fmt]["scale"], 0.0123, 1.0 / 3.0, -0.75, -2.0 ** -15, 0.0):
        x = _cf32(ints, scale)
        obj.reset()
        ref = obj.run(x).clone()
        obj.reset()
        got = obj.run_int(ints, scale=scale)
        assert _same(got, ref), scale
        if scale == 0.0:
            assert bool(torch.signbit(torch.view_as_real(x)).any()) and float(ref.abs().max()) == 0.0      # -0.0 among the inputs
    obj.close()


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", ["direct-rm2", "direct-rm1"])
def test_captures(ctx, name, fmt):
    """S = 3 captures a capture_stride larger than n_in apart, bit-identical to run_captures on the converted array; the object's own
    stream goes on afterwards as if nothing had happened"""
    import torch
    import lora_sdr_amd as Lh
    D, tile = CASES[name]["D"], _plan(name)["tile"]
    S, n, gap = 3, (tile + 29) * D + 3, 5
    scale = 0.0123
    buf = _ints(fmt, S * (n + gap), 31).reshape(S, n + gap, 2)
    wide = buf[:, :n]
    assert wide.stride(0) // 2 == n + gap > n
    stream = _ints(fmt, 4 * n, 32)
    xs = _cf32(stream, scale)
    obj = _make(ctx, name)
    whole = obj.run(xs).clone()
    want = obj.run_captures(_cf32(wide, scale)).clone()
    obj.reset()
    cut = n + D // 2
    first = obj.run(xs[:cut]).clone()
    before = obj.out_count(4 * n - cut)
    got = obj.run_captures_int(wide, scale=scale)
    assert got.shape == (S, obj.n_channels, n // D)
    assert _same(got, want)
    assert float(got.abs().max()) > 0.0
    # the C call itself, the captures further apart still, into rows with a stride of their own
    lib = Lh.load()
    out = torch.zeros((S, obj.n_channels, n // D + 3), dtype=torch.complex64, device="cuda")
    cnt = C.c_size_t()
    rc = lib.lorahip_channelizer_run_captures_iq(obj._h, C.c_void_p(buf.data_ptr()), FORMATS[fmt]["code"], C.c_float(scale), 2, 2 * (n + gap), n,
                                                 C.c_void_p(out.data_ptr()), n // D + 3, C.byref(cnt))
    assert rc == 0 and cnt.value == n // D
    assert _same(out[0, :, :n // D], want[0]) and _same(out[1, :, :n // D], want[2]) and float(out[2].abs().max()) == 0.0
    assert obj.out_count(4 * n - cut) == before
    second = obj.run(xs[cut:])
    obj.close()
    assert _same(torch.cat([first, second], dim=1), whole)


@pytest.mark.parametrize("name", ["direct-rm2", "pfb-staged", "pfb5-unstaged"])
def test_refusals_leave_the_stream_alone(ctx, refs, name):
    import torch
    import lora_sdr_amd as Lh
    lib = Lh.load()
    run_iq, prefix = _entry(name)
    ints, want = refs(name, "sc16")
    n, D = ints.shape[0], CASES[name]["D"]
    cut = n // 3 + 1
    obj = _make(ctx, name)
    first = obj.run_int(ints[:cut]).clone()
    rest = ints[cut:]
    n_next = obj.out_count(n - cut)
    assert n_next > 0
    out = torch.zeros((obj.n_channels, n_next), dtype=torch.complex64, device="cuda")
    cf = _cf32(rest, 2.0 ** -15)
    i8 = torch.zeros((n - cut + 1, 2), dtype=torch.int8, device="cuda")
    cnt = C.c_size_t()
    s16 = 2.0 ** -15
    p16, p8, pcf = rest.data_ptr(), i8.data_ptr(), cf.data_ptr()
    assert p16 % 4 == 0 and p8 % 2 == 0 and pcf % 8 == 0
    refused = [("format 3", p16, 3, s16), ("format -1", p16, -1, s16), ("format 256", p16, 256, s16),
               ("NaN scale", p16, 1, float("nan")), ("Inf scale", p16, 1, float("inf")), ("-Inf scale", p8, 2, float("-inf")),
               ("cf32 with scale 2", pcf, 0, 2.0),
               ("sc16 at an odd address", p16 + 1, 1, s16), ("sc16 at 2 bytes", p16 + 2, 1, s16), ("sc8 at an odd address", p8 + 1, 2, s16),
               ("cf32 at 4 bytes", pcf + 4, 0, 1.0)]
    for what, ptr, fmt, scale in refused:
        rc = getattr(lib, run_iq)(obj._h, C.c_void_p(ptr), fmt, C.c_float(scale), n - cut, C.c_void_p(out.data_ptr()), n_next, C.byref(cnt))
        assert rc == -1, what
        assert lib.lorahip_last_error().decode().startswith(prefix + ":"), (what, lib.lorahip_last_error())
        assert obj.out_count(n - cut) == n_next, what
    # rows too short: the refusal of the plain run
    rc = getattr(lib, run_iq)(obj._h, C.c_void_p(p16), 1, C.c_float(s16), n - cut, C.c_void_p(out.data_ptr()), n_next - 1, C.byref(cnt))
    assert rc == -1 and obj.out_count(n - cut) == n_next
    if CASES[name]["kind"] == "direct":
        rc = lib.lorahip_channelizer_run_captures_iq(obj._h, C.c_void_p(p16), 3, C.c_float(s16), 1, n - cut, n - cut, C.c_void_p(out.data_ptr()), n_next, C.byref(cnt))
        assert rc == -1 and lib.lorahip_last_error().decode().startswith(prefix + ":")
        with pytest.raises(ValueError):
            obj.run_captures_int(rest)                                      # (n, 2) is no (S, n, 2)
    # Python: wrong dtype, wrong shape, strides other than (2, 1), a scale that is no finite number, an out too small
    for bad in (rest.to(torch.int32), rest.float(), cf, rest[:, 0], rest.reshape(-1), torch.zeros((n - cut, 3), dtype=torch.int16, device="cuda"),
                rest[::2], rest.t().contiguous().t(), rest.reshape(1, -1, 2), rest.cpu()):
        with pytest.raises(ValueError, match="int16 or int8"):
            obj.run_int(bad)
    for bad in (float("nan"), float("inf"), 1e60, "x"):
        with pytest.raises(ValueError, match="scale"):
            obj.run_int(rest, scale=bad)
    with pytest.raises(ValueError, match="out must be"):
        obj.run_int(rest, out=out[:, :n_next - 1])
    assert obj.out_count(n - cut) == n_next
    second = obj.run_int(rest, out=out)
    assert second.data_ptr() == out.data_ptr()
    assert _same(torch.cat([first, second], dim=1), want)
    # LORAHIP_IQ_CF32 with scale 1 is the plain run
    obj.reset()
    full = _cf32(ints, s16)
    out_all = torch.zeros_like(want)
    rc = getattr(lib, run_iq)(obj._h, C.c_void_p(full.data_ptr()), 0, C.c_float(1.0), n, C.c_void_p(out_all.data_ptr()), want.shape[1], C.byref(cnt))
    obj.close()
    assert rc == 0 and cnt.value == want.shape[1] == n // D
    assert _same(out_all, want)


def _bytes_back(Lh, narrow, sf, cr, mtu):
    d = Lh.LoRaDemod(sf, n_channels=narrow.shape[0]); d.set_mode(1); d.setMTU(mtu)
    d.work(narrow.contiguous())
    pk = sorted(d.packets(), key=lambda p: p[0])
    d.close()
    dec = Lh.LoRaDecoder()
    dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True)
    out = dec.work([p[2] for p in pk])
    return [p[0] for p in pk], [None if o is None else bytes(o) for o in out], dec.getDropped()


def test_loopback_bytes_to_bytes_through_integers(gpu):
    """Case A of tests/test_gpu_pfb.py (the 8 even bins of M = 16 at D = 16, SF7, its messages and near/far): transmit ->
    PolyphaseSynthesizer -> quantised here to sc16 and to sc8 with the peak at full scale -> PolyphaseChannelizer.run_int -> LoRaDemod ->
    LoRaDecoder returns every channel's bytes. The cf32 chain comes first: that it returns the bytes is what makes the shape a valid
    one. 8 bits under 8 summed channels leave about 30 dB a channel before the decimation gain, far more than SF7 needs."""
    import torch
    import lora_sdr_amd as Lh
    sf, cr = 7, "4/5"
    msgs, _, gains = sd.loopback_case(sf)
    M, K, U, L, N = 16, 8, 16, 128, 1 << sf
    bins = np.arange(-8, 8, 2)
    h = Lh.design_lowpass(U, L, cutoff=0.6 / U)
    sent = [bytes(m) for m in msgs]
    with Lh.Context(sf) as ctx:
        enc = Lh.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate(cr)
        mtu = enc.num_symbols(max(len(m) for m in msgs))
        iq, _ = Lh.transmit(sent, sf=sf, cr=cr, padding=2, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
        rows = sd.stagger(iq)
        sy = Lh.PolyphaseSynthesizer(ctx, M, U, U * h, bins, gains)
        wide = sy.run(rows).clone()
        sy.close()
        pf = Lh.PolyphaseChannelizer(ctx, M, U, h, bins)
        chans, got, dropped = _bytes_back(Lh, pf.run(wide), sf, cr, mtu)
        assert chans == list(range(K)) and got == sent and dropped == 0, "the cf32 chain does not return the bytes: the shape is not valid"
        comp = torch.view_as_real(wide)
        peak = float(comp.abs().max())
        for dtype, qmax in ((torch.int16, 32767), (torch.int8, 127)):
            g = qmax / peak
            q = torch.clamp(torch.round(comp * g), -qmax - 1, qmax).to(dtype)
            assert int(q.abs().max()) == qmax
            pf.reset()
            narrow = pf.run_int(q, scale=1.0 / g)
            assert narrow.shape == (K, rows.shape[1])
            chans, got, dropped = _bytes_back(Lh, narrow, sf, cr, mtu)
            assert chans == list(range(K)) and got == sent and dropped == 0, dtype
        pf.close()
