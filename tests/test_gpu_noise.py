"""GPU: the synthetic-input noise (addAwgn and the noise term of synthSymbols, lora_sdr_amd/csrc/lorahip_tx.hip) is noise.

Every symbol-error figure of the project (BASELINE config 5, the loopback test, the channeliser chain tests) is drawn from this
generator, and nothing bit-exact exists to hold it to. So it is held to closed-form statistics of independent N(0, sigma^2)
components, to its own description (splitmix64 of a counter, Box-Muller in double, restated on the host) and to the claim that
both kernels run the same generator.

The bounds are derived, not measured: five standard errors of each estimator under the null hypothesis (independent unit
normals, n samples): mean 1/sqrt(n), variance sqrt(2/n), a correlation of two independent unit sequences over n' products
1/sqrt(n'), excess kurtosis sqrt(24/n). One stream gives 44 such statistics, about 2.5e-5 of false alarm at five standard
errors; the seeds are fixed, and the six configurations (two kernels, three sigmas) use the SAME seed and therefore the same
underlying normals, scaled: they are one trial, not six. test_bounds_hold_for_numpys_generator runs the same code over numpy's
generator without a GPU, so a bound cannot be the cause of a failure.

synth_symbols' noise is looked at as synth_symbols(noise_sigma) - synth_symbols(0): the sum was rounded to fp32 at the chirp's
magnitude, which adds a rounding term below 2^-24 (1 + 6.7 sigma) per component -- at most 4e-7 sigma, four orders below any bound here.
"""
import numpy as np
import pytest

N_SAMPLES = 1 << 24
SEED = 0x5EED0F00D
CUTOFF = float(np.sqrt(2.0 * np.log(2.0 ** 32)))           # Box-Muller on u1 >= 2^-32: no component beyond 6.66 sigma
LAGS = [1] + [1 << k for k in range(1, 13)]


def _corr(a, b):
    """mean of a * b and five standard errors of it for independent unit sequences"""
    return float(np.dot(a, b)) / a.size, 5.0 / np.sqrt(a.size)


def stream_statistics(I, Q, row_lag):
    """I, Q: float64 components of n samples in units of sigma. Returns [(name, value, low, high)]"""
    n = I.size
    out = []
    for name, c in (("I", I), ("Q", Q)):
        mean = float(c.mean())
        var = float(np.dot(c, c)) / n - mean * mean
        out.append(("mean " + name, mean, -5.0 / np.sqrt(n), 5.0 / np.sqrt(n)))
        out.append(("variance " + name, var, 1.0 - 5.0 * np.sqrt(2.0 / n), 1.0 + 5.0 * np.sqrt(2.0 / n)))
        d = c - mean
        d2 = d * d
        kurt = float(np.dot(d2, d2)) / n / (var * var) - 3.0
        out.append(("excess kurtosis " + name, kurt, -5.0 * np.sqrt(24.0 / n), 5.0 * np.sqrt(24.0 / n)))
        for lag in LAGS + [row_lag]:
            v, b = _corr(c[:-lag], c[lag:])
            out.append(("autocorrelation %s lag %d" % (name, lag), v, -b, b))
    v, b = _corr(I, Q)
    out.append(("correlation I Q", v, -b, b))
    peak = float(max(np.abs(I).max(), np.abs(Q).max()))
    out.append(("largest |component| / sigma", peak, 4.5, CUTOFF * (1.0 + 2.0 ** -20)))
    return out


def cross_statistics(what, Ia, Qa, Ib, Qb):
    """two streams that should be independent (two rows, two seeds)"""
    out = []
    for name, a, b_ in (("I I", Ia, Ib), ("Q Q", Qa, Qb), ("I Q", Ia, Qb)):
        v, b = _corr(a, b_)
        out.append(("correlation %s %s" % (what, name), v, -b, b))
    return out


def repeats(z64):
    """number of 64-bit samples (fp32 I and Q together) among the first 2^20 that occurred before"""
    w = np.ascontiguousarray(z64[:1 << 20]).view(np.uint64)
    return int(w.size - np.unique(w).size)


def check(stats):
    for name, value, low, high in stats:
        print("%-40s %+.4e   [%+.4e, %+.4e]" % (name, value, low, high))
    bad = [s for s in stats if not (s[2] <= s[1] <= s[3])]
    assert not bad, bad


def all_statistics(rows, other_seeds, sigma):
    """rows: (2, n) complex64, one generator stream of 2n samples (row 1 follows row 0); other_seeds: [(what, (n,) complex64)]"""
    s = float(np.float32(sigma))
    n = rows.shape[1]
    I0, Q0 = rows[0].real.astype(np.float64) / s, rows[0].imag.astype(np.float64) / s
    stats = stream_statistics(I0, Q0, n // 4)
    I1, Q1 = rows[1].real.astype(np.float64) / s, rows[1].imag.astype(np.float64) / s
    stats += cross_statistics("of two rows", I0, Q0, I1, Q1)
    del I1, Q1
    for what, z in other_seeds:
        stats += cross_statistics(what, I0, Q0, z.real.astype(np.float64) / s, z.imag.astype(np.float64) / s)
    return stats


def test_bounds_hold_for_numpys_generator():
    """the same statistics, the same bounds, numpy's normal generator in the place of the kernel. Its largest component is held to
    the lower bound only: the cut-off above is the kernel's own (a 32-bit uniform in Box-Muller), not a property of a normal."""
    rng = np.random.default_rng(2024)
    n = N_SAMPLES
    def draw(shape):
        z = np.empty(shape, np.complex64)
        z.real = rng.standard_normal(shape, np.float32)
        z.imag = rng.standard_normal(shape, np.float32)
        return z
    stats = all_statistics(draw((2, n)), [("of seeds one bit apart", draw(n)), ("of two seeds", draw(n))], 1.0)
    assert len(stats) == 45
    stats = [(nm, v, lo, (np.inf if nm.startswith("largest") else hi)) for nm, v, lo, hi in stats]
    check(stats)
    assert repeats(draw(1 << 20)) == 0


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def host_noise(n, seed, first=0):
    """the generator as lorahip_tx.hip (noiseSample) states it: sample e = Box-Muller in double of the two 32-bit halves of
    splitmix64(seed ^ (e * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019)), rounded to fp32"""
    e = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = splitmix64(np.uint64(seed) ^ (e * np.uint64(0xD1342543DE82EF95) + np.uint64(0x632BE59BD9B4E019)))
    u1 = ((r >> np.uint64(32)).astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = (r & np.uint64(0xffffffff)).astype(np.float64) * 2.0 ** -32
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(n, np.complex64)
    z.real = (rad * np.cos(6.283185307179586476925 * u2)).astype(np.float32)
    z.imag = (rad * np.sin(6.283185307179586476925 * u2)).astype(np.float32)
    return z


def test_host_restatement_is_noise_too():
    """the restated generator (no GPU) through the per-stream statistics on 2^20 samples, cut-off included: what the GPU test
    pins the kernel to is itself a normal generator"""
    z = host_noise(1 << 20, SEED)
    check(stream_statistics(z.real.astype(np.float64), z.imag.astype(np.float64), (1 << 20) // 4)[:-1])
    peak = np.abs(z.view(np.float32)).max()
    assert 4.0 < peak <= CUTOFF * (1.0 + 2.0 ** -20)         # 2^21 components: the largest is beyond 4 (expected 5.1)
    assert repeats(z) == 0


# ---------------------------------------------------------------------------------------------------------------------------
SF = 10


def _awgn(ctx, torch, shape, sigma, seed):
    return ctx.add_awgn(torch.zeros(shape, dtype=torch.complex64, device="cuda"), sigma, seed=seed)


def _synth_noise(ctx, torch, shape, sigma, seed):
    """synth_symbols(noise_sigma) - synth_symbols(0) over prod(shape) samples (rows = channels of shape[1] >> SF windows each)"""
    n = int(np.prod(shape))
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    sym = torch.randint(0, 1 << SF, (n >> SF,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    noisy = ctx.synth_symbols(sym, 1.0, sigma, seed)
    clean = ctx.synth_symbols(sym, 1.0, 0.0, seed)
    assert float(clean.abs().max()) < 1.0 + 1e-6             # the clean signal is the unit chirp
    return (noisy - clean).reshape(shape)                    # exact in fp32 up to the rounding the sum already has


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [0.2, 1.0, 4.0])
@pytest.mark.parametrize("source", ["add_awgn", "synth_symbols"])
def test_noise_statistics(gpu, source, sigma):
    import torch
    import lora_sdr_amd as Lh
    make = _awgn if source == "add_awgn" else _synth_noise
    n = N_SAMPLES
    with Lh.Context(SF) as ctx:
        rows = make(ctx, torch, (2, n), sigma, SEED).cpu().numpy()
        others = [("of seeds one bit apart", make(ctx, torch, (n,), sigma, SEED ^ 1).cpu().numpy()),
                  ("of two seeds", make(ctx, torch, (n,), sigma, 0xC0FFEE123456789).cpu().numpy())]
        # exact repeats: on the generator's own samples (for synth_symbols with a zero chirp: a sum rounded at the chirp's
        # magnitude keeps only some 2^22 values per component and repeats by rounding alone)
        if source == "add_awgn":
            raw = rows[0, :1 << 20]
        else:
            sym = torch.zeros((1 << 20) >> SF, dtype=torch.int16, device="cuda")
            raw = ctx.synth_symbols(sym, 0.0, sigma, SEED).cpu().numpy()
    stats = all_statistics(rows, others, sigma)
    assert len(stats) == 45
    check(stats)
    assert repeats(raw) == 0


@pytest.mark.gpu
def test_deterministic_and_neutral(gpu):
    """the same seed gives the same bits, another seed others; sigma = 0 and n = 0 leave the tensor untouched"""
    import torch
    import lora_sdr_amd as Lh
    n = 100003
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    base = torch.view_as_complex(torch.randn((n, 2), generator=g, device="cuda"))
    with Lh.Context(7) as ctx:
        a = ctx.add_awgn(base.clone(), 0.5, seed=11)
        b = ctx.add_awgn(base.clone(), 0.5, seed=11)
        c = ctx.add_awgn(base.clone(), 0.5, seed=12)
        assert torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32))
        assert not torch.equal(a, c) and not torch.equal(a, base)
        z = ctx.add_awgn(base.clone(), 0.0, seed=11)
        assert torch.equal(torch.view_as_real(z).view(torch.int32), torch.view_as_real(base).view(torch.int32))
        e = base.clone()
        ctx.add_awgn(e[5:5], 1.0, seed=11)
        assert torch.equal(torch.view_as_real(e).view(torch.int32), torch.view_as_real(base).view(torch.int32))
        sym = torch.arange(64, device="cuda", dtype=torch.int32).to(torch.int16)
        s1 = ctx.synth_symbols(sym, 1.0, 0.3, seed=5)
        s2 = ctx.synth_symbols(sym, 1.0, 0.3, seed=5)
        assert torch.equal(torch.view_as_real(s1).view(torch.int32), torch.view_as_real(s2).view(torch.int32))
        assert not torch.equal(s1, ctx.synth_symbols(sym, 1.0, 0.3, seed=6))


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [0.2, 1.0, 4.0])
@pytest.mark.parametrize("sf", [7, 10, 12])
def test_synth_noise_is_add_awgn(gpu, sf, sigma):
    """synth_symbols(sym, noise_sigma = s, seed) == synth_symbols(sym, 0) followed by add_awgn(s, seed), bit for bit: both add
    sigma * (float)(...) in fp32 to the already rounded chirp sample, with the same counter (the library is built without FMA
    contraction, so neither sum is fused)"""
    import torch
    import lora_sdr_amd as Lh
    g = torch.Generator(device="cuda"); g.manual_seed(sf)
    with Lh.Context(sf) as ctx:
        sym = torch.randint(0, 1 << sf, ((1 << 21) >> sf,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        one = ctx.synth_symbols(sym, 0.7, sigma, seed=99)
        two = ctx.add_awgn(ctx.synth_symbols(sym, 0.7, 0.0, seed=1), sigma, seed=99)
        assert one.shape == two.shape == (1 << 21,)
        assert torch.equal(torch.view_as_real(one).view(torch.int32), torch.view_as_real(two).view(torch.int32))
        assert not torch.equal(one, ctx.synth_symbols(sym, 0.7, 0.0))


@pytest.mark.gpu
def test_generator_is_the_stated_one(gpu):
    """the first 2^16 samples against the host restatement of splitmix64 + Box-Muller, within one fp32 ulp: the device's log /
    sincos in double against numpy's differ by a double ulp or so, which moves an fp32 rounding once in some 10^8 values"""
    import torch
    import lora_sdr_amd as Lh
    with Lh.Context(7) as ctx:
        for seed in (0, SEED, 2 ** 64 - 1):
            got = _awgn(ctx, torch, (1 << 16,), 1.0, seed).cpu().numpy()
            want = host_noise(1 << 16, seed)
            ulp = np.spacing(np.abs(want.view(np.float32)))
            diff = np.abs(got.view(np.float32).astype(np.float64) - want.view(np.float32).astype(np.float64))
            assert np.all(diff <= ulp), (seed, int(np.argmax(diff / ulp)), float((diff / ulp).max()))
            assert np.mean(diff == 0) > 0.99                 # nearly all components agree to the bit
        # sigma scales in fp32
        got = _awgn(ctx, torch, (4096,), 0.2, SEED).cpu().numpy().view(np.float32)
        want = np.float32(0.2) * host_noise(4096, SEED).view(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2.0 * np.spacing(np.abs(want)))
