"""GPU: integer IQ output (sc16, sc8) of the two synthesisers -- Synthesizer.run_int, PolyphaseSynthesizer.run_int, clipped(), the
*_run_iq / *_clipped entry points (include/lorahip.h "Integer IQ output"). The definition quantises the cf32 output
sample of the object's own definition -- t = scale * c in fp32, r = rint(t), NaN -> 0, saturate, count what clipped -- so there is no
tolerance here: run_int(rows, dtype, scale) must store, bit for bit, the same object's run(rows) quantised by the torch expression of
that definition on the device, for every store path, chunking, alignment, scale and mixture of formats on one stream, and clipped()
must be the torch count. run() itself is held to its float64 definition by the tests of each synthesiser. tests/test_iq_out_cpu.py
holds the torch expression to the numpy definition (tests/iq_out_def.py) and that to hand-written cases."""
import ctypes as C
import math

import numpy as np
import pytest

import iq_out_def as qd
import synthesizer_def as sd

pytestmark = pytest.mark.gpu

FORMATS = {"sc16": dict(dtype="int16", code=1, bytes=4), "sc8": dict(dtype="int8", code=2, bytes=2)}
DIRECT_FREQS = [0.0, -0.21, 0.13, 0.37, -0.05, 0.5, 0.25, -0.4, 0.031, -0.3, 0.44]      # 0, negative ones, K = 11: no multiple of 8
BINS = {16: [3, -3, 0, 8, 3], 32: [5, -7, 0, 16, 5], 10: [1, -2, 0, 5, 1], 1024: [3, -300, 0, 512, 3]}     # a negative bin and a duplicate
# the smallest shapes that reach each store path. Direct form: a lane holds 8 output phases; a full phase block is written in 16-byte
# stores when vec16 holds, everything else one sample at a time. Polyphase: one output a lane; (1024, 3, 20) with 9000 input times spans
# three workspace segments of 4096.
CASES = {"direct-8x64": dict(kind="direct", U=8, L=64),            # vec16 for sc16 and sc8
         "direct-12x100": dict(kind="direct", U=12, L=100),        # the second phase block is partial; vec16 for sc16 only
         "direct-3x20": dict(kind="direct", U=3, L=20),            # U < 8, odd: one sample at a time
         "direct-16x5": dict(kind="direct", U=16, L=5),            # phases without a tap: exact zeros that count nothing
         "psb-16": dict(kind="psb", M=16, U=16, L=128),
         "psb-32": dict(kind="psb", M=32, U=12, L=100),
         "psb5-10": dict(kind="psb5", M=10, U=16, L=83),
         "psb-1024": dict(kind="psb", M=1024, U=3, L=20, n=9000)}
PSB_WS_POINTS = 1 << 22


def vec16(U, fmt, ptr):
    """the direct form's rule of the wide store path restated (lorahip_synth.hip): lanes lie U samples apart, so every lane's first
    output is 16-byte aligned when U * sizeof(sample) is a multiple of 16 and the buffer is"""
    return (U * FORMATS[fmt]["bytes"]) % 16 == 0 and ptr % 16 == 0


def bank_tile(M):
    """psbCreate's T restated: the largest power of two with T M <= 4096, 8 at least, 256 at most"""
    return max(8, min(256, 1 << ((4096 // M).bit_length() - 1)))


def _n_in(name):
    """two tiles plus a ragged rest"""
    c = CASES[name]
    if "n" in c:
        return c["n"]
    return 2 * (256 if c["kind"] == "direct" else bank_tile(c["M"])) + 37


def _taps(U, L):
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(1000 * U + L)
    return (U * Lh.design_lowpass(U, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)     # not symmetric: the tap order matters


def _gains(name):
    K = len(DIRECT_FREQS) if CASES[name]["kind"] == "direct" else len(BINS[CASES[name]["M"]])
    return np.linspace(0.6, 1.4, K).astype(np.float32)


def _make(ctx, name):
    import lora_sdr_amd as Lh
    c = CASES[name]
    h = _taps(c["U"], c["L"])
    if c["kind"] == "direct":
        return Lh.Synthesizer(ctx, DIRECT_FREQS, c["U"], h, _gains(name))
    make = Lh.PolyphaseSynthesizer if c["kind"] == "psb" else Lh.PolyphaseSynthesizer.radix5
    return make(ctx, c["M"], c["U"], h, BINS[c["M"]], _gains(name))


def _entry(kind):
    """(the *_run_iq entry point, the *_clipped one, the prefix of the refusal texts)"""
    if kind == "direct":
        return "lorahip_synthesizer_run_iq", "lorahip_synthesizer_clipped", "synthesiser"
    return "lorahip_psb_run_iq", "lorahip_psb_clipped", "polyphase synthesiser"


def _amplitude(name):
    """The rows are complex Gaussians, each component of standard deviation a. Output phase p is then Gaussian with component variance
    a^2 sum_k g_k^2 sum_i h[p + i U]^2 (independent rows, unit-modulus mixers), 0 for a phase without a tap, and a component clips at
    the default scales when it exceeds 1 (+ half a step). a is the value at which 5 % of all components do: inside the 1 % .. 10 % the
    tests assert from the cf32 output."""
    c = CASES[name]
    h = _taps(c["U"], c["L"]).astype(np.float64)
    g2 = float((_gains(name).astype(np.float64) ** 2).sum())
    var = np.array([g2 * (h[p::c["U"]] ** 2).sum() for p in range(c["U"])])
    share = lambda a: float(np.mean([math.erfc(1.0 / (a * math.sqrt(2.0 * v))) if v > 0 else 0.0 for v in var]))
    lo, hi = 1e-3, 1e3
    for _ in range(60):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if share(mid) < 0.05 else (lo, mid)
    return lo


def _rows(name, n=None):
    import torch
    c = CASES[name]
    K = len(_gains(name))
    n = _n_in(name) if n is None else n
    rng = np.random.default_rng(sorted(CASES).index(name) + 10)
    x = (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))) * _amplitude(name)
    return torch.from_numpy(x.astype(np.complex64)).cuda()


def _quantise(y, fmt, scale):
    """the torch expression of the definition on the device: (the (n, 2) integer tensor, the number of clipped components) of the cf32
    stream y"""
    import torch
    lo, hi = qd.BOUNDS[fmt]
    r = torch.round(torch.view_as_real(y) * float(np.float32(scale)))
    q = torch.nan_to_num(r, nan=0.0, posinf=float(hi), neginf=float(lo)).clamp(lo, hi).to(getattr(torch, FORMATS[fmt]["dtype"]))
    return q, int((torch.isnan(r) | (r < lo) | (r > hi)).sum())


def _dtype(fmt):
    import torch
    return getattr(torch, FORMATS[fmt]["dtype"])


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as Lh
    with Lh.Context(7) as c:
        yield c


@pytest.fixture(scope="module")
def refs(ctx):
    """(rows, the cf32 output of one run() call) of a shape, computed once and left alone"""
    cache = {}

    def get(name):
        if name not in cache:
            rows = _rows(name)
            obj = _make(ctx, name)
            want = obj.run(rows).clone()
            assert obj.clipped() == 0                      # the cf32 run counts nothing
            obj.close()
            assert want.shape == (_n_in(name) * CASES[name]["U"],)
            cache[name] = (rows, want)
        return cache[name]
    return get


def _assert_paths(name, fmt, ptr):
    """a changed rule fails here instead of silently testing one path twice"""
    c = CASES[name]
    if name == "direct-8x64":
        assert vec16(c["U"], fmt, ptr) and c["U"] % 8 == 0
    elif name == "direct-12x100":
        assert vec16(c["U"], fmt, ptr) == (fmt == "sc16") and c["U"] % 8 and c["U"] > 8
    elif name == "direct-3x20":
        assert not vec16(c["U"], fmt, ptr) and c["U"] < 8 and c["U"] % 2
    elif name == "direct-16x5":
        assert c["L"] < c["U"]
    elif name == "psb-1024":
        assert -(-c["n"] // (PSB_WS_POINTS // c["M"])) == 3
    if c["kind"] == "direct":
        assert len(DIRECT_FREQS) % 8 and 0.0 in DIRECT_FREQS and min(DIRECT_FREQS) < 0
    else:
        b = BINS[c["M"]]
        assert min(b) < 0 and len(set(b)) < len(b)
        assert "n" in c or (_n_in(name) > 2 * bank_tile(c["M"]) and _n_in(name) % bank_tile(c["M"]))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_identity_and_count(ctx, refs, name, fmt):
    """run_int == quantised run() and clipped() == the torch count, at the default scale with 1 % .. 10 % of the components clipping;
    nothing clips at a small scale; reset() clears the count; the cf32 runs add nothing"""
    import torch
    rows, want = refs(name)
    c = CASES[name]
    scale = qd.DEFAULT_SCALE[fmt]
    q, n_clip = _quantise(want, fmt, scale)
    share = n_clip / float(q.numel())
    print("IQ out %s %s: %d of %d components clip (%.2f %%)" % (name, fmt, n_clip, q.numel(), 100 * share))
    assert 0.01 <= share <= 0.10
    obj = _make(ctx, name)
    got = obj.run_int(rows, dtype=_dtype(fmt))
    _assert_paths(name, fmt, got.data_ptr())
    assert got.dtype == _dtype(fmt) and got.shape == (want.numel(), 2)
    assert torch.equal(got, q)
    assert obj.clipped() == n_clip
    assert obj.clipped() == n_clip                         # reading does not clear
    if name == "direct-16x5":                              # phases without a tap are exact zeros
        zero = got.reshape(-1, c["U"], 2)[:, c["L"]:]
        assert zero.numel() and not bool(zero.any())
    # the cf32 run and LORAHIP_IQ_CF32 with scale 1 add nothing, and are the plain run
    obj.reset()
    assert obj.clipped() == 0
    assert torch.equal(torch.view_as_real(obj.run(rows)).view(torch.int32), torch.view_as_real(want).view(torch.int32))
    obj.reset()
    out = torch.zeros_like(want)
    cnt = C.c_size_t()
    run_iq = _entry(c["kind"])[0]
    rc = getattr(obj._lib, run_iq)(obj._h, C.c_void_p(rows.data_ptr()), int(rows.stride(0)), int(rows.shape[1]), C.c_void_p(out.data_ptr()), 0,
                                   C.c_float(1.0), C.byref(cnt))
    assert rc == 0 and cnt.value == want.numel()
    assert torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(want).view(torch.int32))
    assert obj.clipped() == 0
    # a scale at which nothing clips: the largest component lands inside the range
    obj.reset()
    small = 0.5 * qd.DEFAULT_SCALE[fmt] / float(torch.view_as_real(want).abs().max())
    q_small, none = _quantise(want, fmt, small)
    assert none == 0 and int(q_small.abs().max()) > 0
    assert torch.equal(obj.run_int(rows, dtype=_dtype(fmt), scale=small), q_small)
    assert obj.clipped() == 0
    # the count adds up over runs, and reset() clears it
    obj.reset()
    obj.run_int(rows, dtype=_dtype(fmt))
    obj.reset()
    obj.run_int(rows, dtype=_dtype(fmt))
    assert obj.clipped() == n_clip
    obj.run_int(rows[:, :1], dtype=_dtype(fmt))
    obj.reset()
    assert obj.clipped() == 0
    obj.close()


def _planted(fmt, scale):
    """float32 values that scale * v (one fp32 multiply) turns into every case of the definition: exact ties of both parities, values
    just inside and beyond both ends, +-3e38, a denormal, -0.0. Built by dividing the targets by the scale and kept only where the
    fp32 product gives the target back exactly, so a scale that is no power of two keeps the ties it can reach (1.5 v is exact for
    every v = 2 t / 3 with few bits: t = 1.5, 4.5, ... and hi + 0.5 = 65535 / 2 among them)."""
    lo, hi = qd.BOUNDS[fmt]
    f32 = np.float32
    targets = [k + 0.5 for k in range(-12, 12)] + [100.5, 101.5, 102.5, -100.5, -101.5, -102.5, hi - 0.5, hi + 0.5, lo - 0.5, lo + 0.5,
                                                   hi, lo, hi + 1.0, lo - 1.0, hi - 1.0, lo + 1.0, 3.0e5, -3.0e5, 7.0, -7.0, 0.25, -0.25]
    vals = []
    for t in targets:
        v = f32(f32(t) / f32(scale))
        if f32(v * f32(scale)) == f32(t):
            vals.append(v)
    # inside (hi, hi + 0.5) and (lo - 0.5, lo): they round to the end without clipping; a quarter step leaves room for the division
    vals += [f32(f32(hi + 0.25) / f32(scale)), f32(f32(lo - 0.25) / f32(scale))]
    vals += [f32(3e38), f32(-3e38), f32(1e-45), f32(-0.0), f32(0.0)]
    return np.array(vals, f32)


def _identity(ctx, kind):
    """y == x: one channel at frequency 0 (bin 0 alone), no interpolation, one tap of 1, gain 1"""
    import lora_sdr_amd as Lh
    one = np.ones(1, np.float32)
    if kind == "direct":
        return Lh.Synthesizer(ctx, [0.0], 1, one, one)
    return Lh.PolyphaseSynthesizer(ctx, 8, 1, one, [0], one)


@pytest.mark.parametrize("scale", [1.0, 1.5])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("kind", ["direct", "psb"])
def test_planted_values(ctx, kind, fmt, scale):
    """An identity plan carries planted values to the store: ties of both parities, both ends, NaN, +-Inf, +-3e38, a denormal, -0.0, at
    scale 1 and at 1.5 (no power of two). The categories are asserted on the cf32 run() output first, then bit identity and the count.

    What an identity plan does with a NON-FINITE sample is the object's own definition, not this feature's. The direct form rotates
    every input by its mixer phase, here (1, 0), and multiplies by the tap (1, 0), and 0 * Inf = NaN: an Inf in a row arrives as NaN
    (include/lorahip.h describes the same for the padding taps), so no row value puts an Inf into the direct form's cf32 output. The
    bank's transform multiplies by twiddles (1, 0) on every path but the one to residue 0, which only adds: the non-finite samples
    stand at stream positions that are multiples of 8, so in the bank they reach the store as they are, and there +Inf and -Inf are
    asserted on the cf32 output. In both objects the +-Inf branch of the definition is also reached through the product: t = 1.5 *
    +-3e38 overflows, asserted on t. The finite rows come back through the direct form value for value (-0.0 as +0.0: 0 + 1 * -0.0 =
    +0.0), asserted by value."""
    import torch
    lo, hi = qd.BOUNDS[fmt]
    v = _planted(fmt, scale)
    n = v.size
    # I carries the planted values against a plain Q, then Q against a plain I; then the non-finite samples, each at a multiple of 8
    special = [complex(np.nan, 1.0), complex(1.0, np.nan), complex(np.inf, 1.0), complex(1.0, -np.inf), complex(-np.inf, np.inf)]
    tail = np.full((-2 * n) % 8 + 8 * len(special), 1 + 1j, np.complex64)
    tail[(-2 * n) % 8::8] = special
    x = np.concatenate([v + 1j * np.float32(3.0), np.float32(-2.0) + 1j * v, tail]).astype(np.complex64)
    assert all(i % 8 == 0 for i in np.nonzero(~np.isfinite(x))[0]) and (~np.isfinite(x)).sum() == len(special)
    rows = torch.from_numpy(x[None, :]).cuda()
    obj = _identity(ctx, kind)
    y = obj.run(rows).clone()
    comp = torch.view_as_real(y)
    finite = torch.isfinite(torch.view_as_real(rows[0])).all(dim=1)
    assert int(finite.sum()) == x.size - len(special)
    if kind == "direct":
        assert torch.equal(comp[finite], torch.view_as_real(rows[0])[finite])          # by value: -0.0 == +0.0
    t = comp * float(np.float32(scale))
    fl = torch.floor(t)
    tie = torch.isfinite(t) & (t - fl == 0.5) & (t.abs() < 1000)
    cats = {"nan": torch.isnan(comp), "tie, even floor": tie & (fl % 2 == 0), "tie, odd floor": tie & (fl % 2 != 0),
            "beyond hi": torch.isfinite(t) & (t > hi + 0.5), "below lo": torch.isfinite(t) & (t < lo - 0.5),
            "just inside hi": (t > hi) & (t < hi + 0.5), "just inside lo": (t < lo) & (t > lo - 0.5),
            "denormal": (comp != 0) & (comp.abs() < 1e-38), "3e38": comp.abs() > 2.9e38, "zero": comp == 0}
    if scale == 1.0:
        cats["tie at hi"], cats["tie at lo"] = t == hi + 0.5, t == lo - 0.5
    else:
        cats["+inf of t"], cats["-inf of t"] = torch.isposinf(t) & torch.isfinite(comp), torch.isneginf(t) & torch.isfinite(comp)
    if kind == "psb":
        cats["+inf"], cats["-inf"] = torch.isposinf(comp), torch.isneginf(comp)
    print("IQ out planted %s %s scale %g: %s" % (kind, fmt, scale, {k: int(m.sum()) for k, m in cats.items()}))
    for what, mask in cats.items():
        assert bool(mask.any()), what
    q, n_clip = _quantise(y, fmt, scale)
    assert n_clip > 0
    obj.reset()
    got = obj.run_int(rows, dtype=_dtype(fmt), scale=scale)
    assert torch.equal(got, q)
    assert obj.clipped() == n_clip
    obj.close()


@pytest.mark.parametrize("name", ["direct-12x100", "direct-3x20", "psb-32", "psb5-10"])
def test_chunking_and_mixed_formats(ctx, refs, name):
    """the same stream in ragged pieces -- 1 sample, shorter than the history, ending inside a tile -- that alternate sc16, the cf32
    run and sc8 with different scales: each piece is the quantisation of its slice of the one-call cf32 output, and the counts add up"""
    import torch
    rows, want = refs(name)
    c = CASES[name]
    n, U = _n_in(name), c["U"]
    hist = -(-c["L"] // U) - 1
    tile = 256 if c["kind"] == "direct" else bank_tile(c["M"])
    assert hist >= 2
    cuts = [0, 1, 1 + (hist - 1), tile - 3, tile - 2, tile + 5, 2 * tile, n]
    assert cuts == sorted(set(cuts)) and cuts[2] - cuts[1] < hist and cuts[3] % tile and cuts[5] % tile
    kinds = ["sc16", "cf32", "sc8"]
    scales = {"sc16": qd.DEFAULT_SCALE["sc16"], "sc8": 0.83 * qd.DEFAULT_SCALE["sc8"]}
    obj = _make(ctx, name)
    total = 0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        kind = kinds[i % 3]
        piece = want[a * U:b * U]
        if kind == "cf32":
            got = obj.run(rows[:, a:b])
            assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(piece.contiguous()).view(torch.int32)), (i, a, b)
        else:
            q, n_clip = _quantise(piece, kind, scales[kind])
            total += n_clip
            assert torch.equal(obj.run_int(rows[:, a:b], dtype=_dtype(kind), scale=scales[kind]), q), (i, a, b, kind)
        assert obj.clipped() == total, (i, a, b, kind)
    assert total > 0
    obj.close()


@pytest.mark.parametrize("name", ["direct-8x64", "direct-12x100", "direct-3x20", "psb-32", "psb-1024"])
def test_alignment_and_overrun(ctx, refs, name):
    """outputs into buf[1:] (sc16, sc8) and buf[3:] (sc8) of a buffer filled with a canary: the same samples as the aligned run, and
    every canary before the first and after the last of the n_out samples untouched"""
    import torch
    rows, want = refs(name)
    n_out = want.numel()
    obj = _make(ctx, name)
    for fmt, lead in (("sc16", 1), ("sc8", 1), ("sc8", 3)):
        q, n_clip = _quantise(want, fmt, qd.DEFAULT_SCALE[fmt])
        canary = 0x5a
        buf = torch.full((n_out + lead + 9, 2), canary, dtype=_dtype(fmt), device="cuda")
        assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + lead * FORMATS[fmt]["bytes"]) % 16
        assert not vec16(CASES[name]["U"], fmt, buf[lead:].data_ptr())
        obj.reset()
        got = obj.run_int(rows, dtype=_dtype(fmt), out=buf[lead:])
        assert got.data_ptr() == buf[lead:].data_ptr() and got.shape == (n_out, 2)
        assert torch.equal(got, q), (fmt, lead)
        assert obj.clipped() == n_clip
        assert bool((buf[:lead] == canary).all()) and bool((buf[lead + n_out:] == canary).all()), (fmt, lead)
        # room for exactly n_out samples will do
        obj.reset()
        exact = torch.full((n_out + lead, 2), canary, dtype=_dtype(fmt), device="cuda")
        assert torch.equal(obj.run_int(rows, dtype=_dtype(fmt), out=exact[lead:]), q)
        assert bool((exact[:lead] == canary).all())
    obj.close()


@pytest.mark.parametrize("name", ["direct-12x100", "psb-32", "psb5-10"])
def test_refusals(ctx, refs, name):
    """what *_run_iq refuses, through ctypes: LORAHIP_E_INVALID, the object's prefix in lorahip_last_error(), *n_out == 0, the count and
    the stream untouched -- the good call afterwards gives what it gives on a stream that never saw a refusal"""
    import torch
    rows, want = refs(name)
    c = CASES[name]
    U = c["U"]
    run_iq, clipped, prefix = _entry(c["kind"])
    obj = _make(ctx, name)
    lib = obj._lib
    cut = _n_in(name) // 3 + 1
    s16 = qd.DEFAULT_SCALE["sc16"]
    q_first, clip_first = _quantise(want[:cut * U], "sc16", s16)
    assert torch.equal(obj.run_int(rows[:, :cut]), q_first)
    assert obj.clipped() == clip_first and clip_first > 0
    rest = rows[:, cut:]
    n_rest = rest.shape[1]
    out16 = torch.zeros((n_rest * U + 1, 2), dtype=torch.int16, device="cuda")
    out8 = torch.zeros((n_rest * U + 1, 2), dtype=torch.int8, device="cuda")
    outcf = torch.zeros(n_rest * U + 1, dtype=torch.complex64, device="cuda")
    p16, p8, pcf, pin = out16.data_ptr(), out8.data_ptr(), outcf.data_ptr(), rest.data_ptr()
    assert p16 % 4 == 0 and p8 % 2 == 0 and pcf % 8 == 0
    refused = [("format 3", pin, p16, 3, s16), ("format -1", pin, p16, -1, s16), ("format 256", pin, p16, 256, s16),
               ("NaN scale", pin, p16, 1, float("nan")), ("Inf scale", pin, p16, 1, float("inf")), ("-Inf scale", pin, p8, 2, float("-inf")),
               ("cf32 with scale 0.5", pin, pcf, 0, 0.5),
               ("sc16 at an odd address", pin, p16 + 1, 1, s16), ("sc16 at 2 bytes", pin, p16 + 2, 1, s16), ("sc8 at an odd address", pin, p8 + 1, 2, 1.0),
               ("cf32 at 4 bytes", pin, pcf + 4, 0, 1.0),
               ("no output", pin, None, 1, s16), ("no input", None, p16, 1, s16), ("no input, cf32", None, pcf, 0, 1.0)]
    count = C.c_ulonglong()
    for what, src, dst, fmt, scale in refused:
        cnt = C.c_size_t(77)
        rc = getattr(lib, run_iq)(obj._h, C.c_void_p(src), int(rest.stride(0)), n_rest, C.c_void_p(dst), fmt, C.c_float(scale), C.byref(cnt))
        assert rc == -1, what
        assert lib.lorahip_last_error().decode().startswith(prefix + ":"), (what, lib.lorahip_last_error())
        assert cnt.value == 0, what
        assert getattr(lib, clipped)(obj._h, C.byref(count)) == 0 and count.value == clip_first, what
    assert getattr(lib, clipped)(obj._h, None) == -1
    assert not bool(out16.any()) and not bool(out8.any()) and not bool(torch.view_as_real(outcf).any())
    # Python: what _iq_out_args and _iq_out_buffer refuse, through the methods
    for bad in (rest.cpu(), rest.to(torch.complex128), rest[:-1], torch.view_as_real(rest)):
        with pytest.raises(ValueError, match="rows must be"):
            obj.run_int(bad)
    for bad in (torch.int32, torch.float32, "int16"):
        with pytest.raises(ValueError, match="torch.int16 or torch.int8"):
            obj.run_int(rest, dtype=bad)
    for bad in (float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError, match="scale"):
            obj.run_int(rest, scale=bad)
    for bad in (out8, out16[:n_rest * U - 1], out16[::2], out16.reshape(-1), out16.cpu(), out16.t().contiguous().t()):
        with pytest.raises(ValueError, match="out must be"):
            obj.run_int(rest, out=bad)
    assert obj.clipped() == clip_first
    # the good call afterwards continues the stream
    q_rest, clip_rest = _quantise(want[cut * U:], "sc8", 90.0)
    second = obj.run_int(rest, dtype=torch.int8, scale=90.0, out=out8)
    assert second.data_ptr() == out8.data_ptr()
    assert torch.equal(second, q_rest)
    assert obj.clipped() == clip_first + clip_rest
    obj.close()


def _bytes_back(Lh, narrow, sf, cr, mtu):
    d = Lh.LoRaDemod(sf, n_channels=narrow.shape[0]); d.set_mode(1); d.setMTU(mtu)
    d.work(narrow.contiguous())
    pk = sorted(d.packets(), key=lambda p: p[0])
    d.close()
    dec = Lh.LoRaDecoder()
    dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True)
    out = dec.work([p[2] for p in pk])
    return [p[0] for p in pk], [None if o is None else bytes(o) for o in out], dec.getDropped()


def test_loopback_bytes_to_bytes_through_integers_on_both_sides(gpu):
    """Case A of DESIGN.md section 8c (the 8 even bins of M = 16 at U = D = 16, L = 128, SF7 4/5, its messages and near/far): transmit ->
    PolyphaseSynthesizer.run_int -> PolyphaseChannelizer.run_int -> LoRaDemod -> LoRaDecoder returns every channel's bytes, as sc16 and
    as sc8, with the peak at full scale (nothing clips) and the receive scale the inverse of the transmit scale; the same through the
    direct-form Synthesizer.run_int. 8 bits under 8 summed channels leave about 30 dB a channel before the decimation gain."""
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
        pf = Lh.PolyphaseChannelizer(ctx, M, U, h, bins)
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, U * h, bins, gains)
        sy = Lh.Synthesizer(ctx, pf.freqs, U, U * h, gains)
        for front in (ps, sy):
            peak = float(torch.view_as_real(front.run(rows)).abs().max())
            assert peak > 0
            for dtype, qmax in ((torch.int16, 32767), (torch.int8, 127)):
                g = qmax / peak
                front.reset()
                q = front.run_int(rows, dtype=dtype, scale=g)
                assert front.clipped() == 0
                assert q.shape == (rows.shape[1] * U, 2) and int(q.abs().max()) >= qmax - 1
                pf.reset()
                narrow = pf.run_int(q, scale=1.0 / g)
                chans, got, dropped = _bytes_back(Lh, narrow, sf, cr, mtu)
                assert chans == list(range(K)) and got == sent and dropped == 0, (type(front).__name__, dtype)
        ps.close(); sy.close(); pf.close()
