"""GPU: the front-end synthesiser at the edges its definition covers (lora_sdr_amd/csrc/lorahip_synth.hip against
tests/synthesizer_def.py).

The kernel has nothing to be bit-exact with, so every test here compares with the float64 definition

    y[n] = sum_k gain[k] exp(+2 pi i frac(w_k n / 2^64)) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]

-- through synthesizer_def.synthesize_at, which evaluates the same sum for SELECTED outputs at absolute indices and is held to
synthesizer_def.synthesize by the first test here (no gpu marker) -- under `bound(K, U, L, scale)` of tests/test_gpu_synthesizer.py.

    what                                                      test
    HC = ceil(L/U) - 1 = 255, 256, 257, 512, 513, 600 (three  test_shape_edges_against_float64_definition, every shape also in
    and four 256-blocks in the rotation, more than two        ragged chunks, bit for bit (pieces shorter than HC: the history
    staging passes), ceil(L/U) = 2295 (the LDS limit) with    is copied from the old history; pieces across a 256 boundary)
    one and two channel groups, U = 256 with and without a
    tap-less last phase, partial and single-phase blocks,
    K = 1 .. 17
    ceil(L/U) = 2296 refused, with its reason                 test_shapes_that_do_not_fit_are_refused
    dyadic frequencies, +-0.5, outside [-0.5, 0.5), 256-block test_mixer_accuracy_relative_to_each_channel
    phases on, below and above every quadrant edge of
    mixerPhase; accuracy relative to EACH channel, 0 .. -60 dB
    NaN, +Inf, -Inf reach exactly U ceil(L/U) outputs         test_non_finite_samples_reach_exactly_their_span
    1e-30 and 1e30                                            test_extreme_amplitudes_follow_the_definition
    K = 65535 + 9: the history kernel's third grid dimension  test_more_channels_than_one_grid_dimension
    a row 2^31 samples into the allocation                    test_rows_beyond_2_pow_31_samples

The negative first block (mb "wraps like the counter") is what every stream that starts at sample 0 runs: the samples it rotates
are the zeros before the stream, so all it has to deliver is a finite phasor -- the shape tests start at 0 and would see a NaN.

Mixer accuracy (test_mixer_accuracy_relative_to_each_channel): one unit tone in channel k, the other 23 rows zero, gains from 0 to
-60 dB; the error is max|y - definition| / max|y_k| for that channel, worst channel. "plain fp32" is the definition in numpy
float32 (sequential sum of h[j] x, times the correctly rounded phasor, times the gain), measured by the test on the host; the bound
is 4 x that, as in tests/test_gpu_channelizer_edges.py:

    shape             plain fp32 vs float64    bound (4 x)    kernel vs float64 (MI355X)
    U = 8,  L = 64    2.35e-7                  9.39e-7        4.14e-7
    U = 16, L = 128   2.45e-7                  9.78e-7        3.81e-7

err / scale of every other accuracy case is printed by the tests (`-s`). Measured on an MI355X: 5.5e-8 .. 4.9e-7 over the 23 shapes
(largest: K = 9, U = 2, L = 4589 at 4.9e-7 under a bound of 1.2e-3; K = 1, U = 1, L = 2295 at 3.8e-7), 7.3e-8 .. 8.8e-8 at 1e-30 and
1e30, 3.7e-8 at K = 65544. Non-finite samples: three bad samples make 192 outputs non-finite at (U, L) = (8, 64) and at (8, 61),
where the definition's L gives 183: the kernel multiplies the zero padding of its tap table, include/lorahip.h says so.
"""
import numpy as np
import pytest

import synthesizer_def as sd
from test_gpu_channelizer_edges import DYADIC, QUADRANT_EDGES, _bits
from test_gpu_synthesizer import bound

M64 = (1 << 64) - 1
TILE = 256


# ---------------------------------------------------------------------------------------------------------------------------
# host side: the constructor's rule, the shape list, which outputs are compared
# ---------------------------------------------------------------------------------------------------------------------------
def plan(U, L):
    """what lorahip_synthesizer_create derives from a shape: taps per phase I, history HC, 256-blocks a tile's rotation spans, LDS
    bytes (8 channels x (256 + HC) rotated samples and 8 x nBlk block phases), and whether the shape is accepted"""
    I = -(-int(L) // int(U))
    HC = I - 1
    nBlk = -(-HC // TILE) + 1
    lds = (8 * (TILE + HC) + 8 * nBlk) * 8
    return dict(I=I, HC=HC, nBlk=nBlk, lds=lds, ok=lds <= (160 << 10) and 8 * nBlk <= TILE)


#          K   U    L
SHAPES = [(2,  1,   256),          # HC = 255: the last history inside one 256-block
          (2,  1,   257),          # HC = 256: two whole blocks
          (2,  1,   258),          # HC = 257: the first with three blocks
          (2,  1,   513),          # HC = 512: three
          (2,  1,   514),          # HC = 513: four
          (2,  1,   601),          # HC = 600: more than two staging passes
          (3,  3,   3 * 257 + 1),  # HC = 257 at U > 1, the last phases one tap short
          (1,  1,   2295),         # I = 2295: the longest that fits the LDS, one channel
          (9,  2,   4589),         # the same with two channel groups and an odd filter
          (2,  256, 256),          # one tap per phase
          (2,  256, 255),          # the last phase without a tap
          (2,  256, 65536),        # the longest filter
          (3,  2,   16), (3, 4, 32), (3, 6, 50),       # even and below 8: 16-byte stores offered, the phase block partial
          (3,  9,   40), (3, 17, 70),                  # a phase block holding one phase
          (1,  8,   64), (7, 8, 64), (8, 8, 64), (9, 8, 64), (16, 8, 64), (17, 8, 64)]
REFUSED = [(1, 1, 2296), (1, 2, 4591)]


def _lowpass(U, L):
    from oracle import channelizer as oc
    return oc.design_lowpass(U, L)


def _rows(rng, K, n):
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def _length(U, L):
    """two to three tiles and a ragged tail, and long enough to fill the filter and cross a tile after that"""
    HC = plan(U, L)["HC"]
    return max(2 * TILE + TILE // 3 + 7, HC + TILE + 91)


def _compared(rng, n, U, L, K):
    """the absolute output indices a shape is compared at: all of them where that is cheap, otherwise all U phases of the first and
    last input times, of those around every 256 boundary and around the place where the filter is first full, and of seeded others"""
    I = plan(U, L)["I"]
    if n * U * I * K <= 1.5e7:
        return np.arange(n * U, dtype=np.int64)
    m = set(range(4)) | set(range(n - 4, n)) | set(range(I - 3, min(n, I + 2)))
    for b in range(TILE, n, TILE):
        m |= set(range(b - 3, min(n, b + 3)))
    want = max(len(m), int(1.5e7 / (U * I * K)))
    m |= set(int(v) for v in rng.choice(n, min(n, want) - len(m), replace=False)) if want > len(m) else set()
    m = np.array(sorted(m), np.int64)
    return (m[:, None] * U + np.arange(U, dtype=np.int64)[None, :]).reshape(-1)


def test_synthesize_at_equals_synthesize_and_the_shape_list_sits_on_every_boundary():
    """the helper against synthesizer_def.synthesize (all outputs, a scattered subset, a window of the stream with its absolute
    position); then the list above by the constructor's rule: neighbours on either side of HC = 256 and of HC = 512, the LDS limit
    from inside, the refused shapes the FIRST that do not fit"""
    rng = np.random.default_rng(1)
    for K, U, L, n, n0 in ((3, 5, 37, 200, 0), (2, 1, 9, 100, 7), (4, 10, 3, 50, 12345), (1, 1, 1, 30, 0), (9, 8, 61, 300, 1 << 29)):
        x = _rows(rng, K, n)
        f = rng.uniform(-1.5, 1.5, K)
        h = rng.uniform(0.5, 1.5, L).astype(np.float32)
        g = rng.uniform(0.25, 2.0, K)
        want = sd.synthesize(x, f, U, h, g, n0=n0)
        idx = n0 * U + np.arange(n * U, dtype=np.int64)
        got = sd.synthesize_at(x, f, U, h, g, n=idx, n0=n0)
        assert np.abs(got - want).max() <= 1e-13 * sd.error_scale(x, h, U, g)      # float64 both: only the order of the sum differs
        pick = rng.choice(n * U, min(40, n * U), replace=False)
        assert np.abs(sd.synthesize_at(x, f, U, h, g, n=idx[pick], n0=n0) - got[pick]).max() <= 1e-13 * sd.error_scale(x, h, U, g)
        # rows handed over as a window of a longer stream: the samples before it read as zero
        cut = n // 3
        tail = sd.synthesize_at(x[:, cut:], f, U, h, g, n=idx[(cut + L) * U:], n0=n0 + cut)
        assert np.abs(tail - want[(cut + L) * U:]).max() <= 1e-13 * sd.error_scale(x, h, U, g)
    p = {(U, L): plan(U, L) for _, U, L in SHAPES}
    assert all(v["ok"] for v in p.values())
    assert [p[(1, L)]["HC"] for L in (256, 257, 258, 513, 514, 601)] == [255, 256, 257, 512, 513, 600]
    assert [p[(1, L)]["nBlk"] for L in (256, 257, 258, 513, 514, 601)] == [2, 2, 3, 3, 4, 4]
    assert p[(3, 772)]["HC"] == 257 and p[(3, 772)]["nBlk"] == 3
    assert p[(1, 2295)]["I"] == p[(2, 4589)]["I"] == 2295 and p[(1, 2295)]["lds"] == 160 << 10
    assert all(plan(U, L)["I"] == 2296 and not plan(U, L)["ok"] for _, U, L in REFUSED)
    assert plan(2, 4590)["ok"] and all(plan(1, L)["ok"] for L in range(1, 2296))
    assert p[(256, 65536)]["HC"] == 255 and p[(256, 255)]["I"] == 1
    assert {K for K, _, _ in SHAPES} >= {1, 7, 8, 9, 16, 17}


# ---------------------------------------------------------------------------------------------------------------------------
# item 1: shapes on both sides of every boundary
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K,U,L", SHAPES, ids=["K%d-U%d-L%d" % s for s in SHAPES])
def test_shape_edges_against_float64_definition(gpu, K, U, L):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(K * 100003 + U * 101 + L)
    HC = plan(U, L)["HC"]
    n = _length(U, L)
    x = _rows(rng, K, n)
    freqs = rng.uniform(-0.5, 0.5, K)
    if K > 1:
        freqs[0] = 0.0
    # cutoff 0.37 / U, not the default 0.5 / U: at U = 1 the default is a full-band filter, a single non-zero tap for odd L
    h = (Lh.design_lowpass(U, L, cutoff=0.37 / U) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)   # not symmetric: the tap order matters
    assert np.count_nonzero(np.abs(h) > 1e-3 * np.abs(h).max()) >= min(L, 8)
    gains = rng.uniform(0.25, 2.0, K).astype(np.float32)
    idx = _compared(rng, n, U, L, K)
    want = sd.synthesize_at(x, freqs, U, h, gains, n=idx)
    xd = torch.from_numpy(x).cuda()
    # pieces shorter than the history (with HC > 256 the new history is copied from the old one), empty, across 256 boundaries
    sizes = [1, max(1, HC // 2), 7, 0, 250, HC + 5, 300, n]
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h, gains)
        whole = sy.run(xd).cpu().numpy()
        sy.reset()
        parts, pos = [], 0
        for s in sizes:
            s = min(s, n - pos)
            parts.append(sy.run(xd[:, pos:pos + s]).cpu().numpy())
            pos += s
        sy.close()
    assert pos == n and whole.shape == (n * U,)
    scale = sd.error_scale(x, h, U, gains)
    err = float(np.abs(whole[idx] - want).max())
    print("synthesiser edges K=%d U=%d L=%d (HC %d): err/scale = %.3g (bound %.3g), %d outputs compared"
          % (K, U, L, HC, err / scale, bound(K, U, L, 1.0), idx.size))
    assert err <= bound(K, U, L, scale), (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(K * (-(-L // U))))
    if L < U:
        assert np.all(whole.reshape(n, U)[:, L:] == 0)           # phases without a tap: exact zeros
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))


@pytest.mark.gpu
@pytest.mark.parametrize("K,U,L", REFUSED)
def test_shapes_that_do_not_fit_are_refused(gpu, K, U, L):
    import lora_sdr_amd as Lh
    with Lh.Context(7) as ctx:
        with pytest.raises(Lh.LoraHipError):
            Lh.Synthesizer(ctx, np.zeros(K), U, np.ones(L, np.float32))
        assert Lh.load().lorahip_last_error().decode().startswith("synthesiser:")
        Lh.Synthesizer(ctx, np.zeros(K), U, np.ones(L - 1, np.float32)).close()    # one tap less: accepted


# ---------------------------------------------------------------------------------------------------------------------------
# item 2: frequencies at their edges, accuracy relative to each channel
# ---------------------------------------------------------------------------------------------------------------------------
def _mixer_case(U, L):
    """24 channels: the 9 DYADIC frequencies, and 15 built in Python integers so that the 32-bit phase the kernel hands mixerPhase
    at the start of ONE 256-block -- the top 32 bits of (w_k U mod 2^64) * 256 B -- is exactly each quadrant edge, one unit (of
    2^-32 turn) below it and one above it, and three places inside the quadrants. B is chosen with 256 B U < 2^20, so that a
    frequency a double holds exactly (w a multiple of 2^11) can hit the unit. One unit tone per channel, inside the pass band; the
    stream starts at an odd place in block B - 1 behind zeros, so block B is rotated as a tile's own block and as the history of the
    next tile. Gains from 0 to -60 dB."""
    K = 24
    B = (1 << 20) // (TILE * U) - 3
    NB = TILE * B * U                                           # output index of the block's first sample
    assert NB << 11 <= 1 << 31
    targets = []
    for e in QUADRANT_EDGES:
        targets += [e - 1, e, e + 1]
    targets += [0x40000000, 0x80000000 - 5, 0xC0000000 + 123]
    rng = np.random.default_rng(U * 1000 + L)
    freqs = list(DYADIC)
    for k, tgt in enumerate(targets):
        w0 = (int(round(((k - 7.5) / 16.0) % 1.0 * (1 << 53))) << 11) & M64
        want = ((tgt & 0xffffffff) << 32) + (1 << 31)
        r = (want - w0 * NB) & M64                              # phase still to be made up at the block start
        dw = (r // (NB << 11)) << 11                            # a double holds 53 bits of the increment
        w = (w0 + dw) & M64
        f = w / float(1 << 64)                                  # exact
        assert sd.phase_inc(f) == w and dw < (1 << 45)
        freqs.append(f)
    assert len(freqs) == K
    # what the test is for, checked on the host with integers as the kernel forms them: (w U mod 2^64) * (256 B) >> 32
    ph = [(((sd.phase_inc(f) * U) & M64) * (TILE * B) & M64) >> 32 for f in freqs[len(DYADIC):]]
    assert ph == [t & 0xffffffff for t in targets]
    gains = (10.0 ** (-60.0 * np.arange(K) / (K - 1) / 20.0)).astype(np.float32)
    x0 = (B - 1) * TILE + 77                                    # input time of the first tone sample
    n = 3 * TILE + 5
    idx = np.arange(n, dtype=np.uint64) + np.uint64(x0)
    x = np.empty((K, n), np.complex64)
    for k in range(K):
        wt = int(rng.uniform(-0.3, 0.3) * (1 << 64)) & M64      # cycles per INPUT sample: inside the pass band of U h
        with np.errstate(over="ignore"):
            x[k] = np.exp(2j * np.pi * ((np.uint64(wt) * idx).astype(np.int64).astype(np.float64) * 2.0 ** -64))
    h = (_lowpass(U, L) * U).astype(np.float32)
    out = np.arange((x0 + L // U + 1) * U, (x0 + n) * U, dtype=np.int64)       # the filter holds tone samples only
    assert out[0] < NB and NB + TILE * U <= out[-1] + 1         # block B is compared whole, and what follows it reaches back into it
    return dict(K=K, U=U, L=L, B=B, x0=x0, x=x, h=h, freqs=np.array(freqs), gains=gains, out=out)


def _plain_fp32(c, k):
    """channel k alone, the definition in numpy float32: h[j] x summed in the order of j, times the correctly rounded phasor, times
    the gain"""
    U, L, h, out, x0 = c["U"], c["L"], c["h"], c["out"], c["x0"]
    xk = c["x"][k]
    acc = np.zeros(out.size, np.complex64)
    for j in range(L):
        sel = (out - j) % U == 0
        m = (out[sel] - j) // U - x0
        acc[sel] = acc[sel] + (h[j] * xk[m]).astype(np.complex64)
    with np.errstate(over="ignore"):
        ph = (np.uint64(sd.phase_inc(c["freqs"][k])) * out.astype(np.uint64)).astype(np.int64).astype(np.float64) * 2.0 ** -64
    return (acc * np.exp(2j * np.pi * ph).astype(np.complex64)) * c["gains"][k]


def test_mixer_case_is_what_it_says():
    """the frequency construction on the host (its own asserts), and the yardstick: the plain-fp32 error per channel is an fp32
    rounding figure -- at least a quarter ulp, at most a random walk of the roundings of ceil(L/U) terms and three products"""
    for U, L in ((8, 64), (16, 128)):
        c = _mixer_case(U, L)
        worst = 0.0
        for k in range(c["K"]):
            want = sd.synthesize_at(c["x"][k:k + 1], c["freqs"][k:k + 1], U, c["h"], c["gains"][k:k + 1], n=c["out"], n0=c["x0"])
            assert np.abs(want).max() > 0.5 * c["gains"][k]     # the channel carries its tone
            worst = max(worst, float(np.abs(_plain_fp32(c, k) - want).max() / np.abs(want).max()))
        print("synthesiser mixer case U=%d L=%d: plain fp32 vs float64, worst channel %.3e" % (U, L, worst))
        assert 2.0 ** -26 < worst < 2.0 ** -24 * (np.sqrt(L // U) + 3.0) * 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("U,L", [(8, 64), (16, 128)])
def test_mixer_accuracy_relative_to_each_channel(gpu, U, L):
    """see the table in the module docstring: kernel vs float64 within 4 x (plain fp32 vs float64), per channel relative to that
    channel's largest output, every channel alone in a 24-channel object (the other rows zero: by linearity, and exact zeros add
    nothing in fp32)"""
    import torch
    import lora_sdr_amd as Lh
    c = _mixer_case(U, L)
    K, x0, out = c["K"], c["x0"], c["out"]
    n = c["x"].shape[1]
    plain = np.empty(K)
    kern = np.empty(K)
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, c["freqs"], U, c["h"], c["gains"])
        zeros = torch.zeros((K, x0), dtype=torch.complex64, device="cuda")
        sink = torch.empty(x0 * U, dtype=torch.complex64, device="cuda")
        for k in range(K):
            want = sd.synthesize_at(c["x"][k:k + 1], c["freqs"][k:k + 1], U, c["h"], c["gains"][k:k + 1], n=out, n0=x0)
            plain[k] = np.abs(_plain_fp32(c, k) - want).max() / np.abs(want).max()
            rows = torch.zeros((K, n), dtype=torch.complex64, device="cuda")
            rows[k] = torch.from_numpy(c["x"][k]).cuda()
            sy.reset()
            sy.run(zeros, out=sink)
            y = sy.run(rows).cpu().numpy()
            kern[k] = np.abs(y[out - x0 * U] - want).max() / np.abs(want).max()
        sy.close()
    bound4 = 4.0 * plain.max()
    print("synthesiser mixer accuracy U=%d L=%d: plain fp32 %.3e, bound %.3e, kernel %.3e (worst channel %d)"
          % (U, L, plain.max(), bound4, kern.max(), int(kern.argmax())))
    print("  per channel: " + " ".join("%.2e" % v for v in kern))
    assert kern.max() <= bound4, (kern.max(), bound4, kern.tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# item 3: non-finite samples
# ---------------------------------------------------------------------------------------------------------------------------
def reach(U, L):
    """outputs one input sample takes part in, as include/lorahip.h states it: the taps are padded with zeros to ceil(L/U) whole
    rounds of U, and the kernel forms the products with the padding"""
    return U * (-(-L // U))


@pytest.mark.gpu
@pytest.mark.parametrize("U,L", [(8, 64), (8, 61)])
def test_non_finite_samples_reach_exactly_their_span(gpu, U, L):
    """a NaN, a +Inf and a -Inf in three rows, all taps non-zero: output n is non-finite exactly when m U <= n < m U + U ceil(L/U)
    for one of the bad input times m (include/lorahip.h; for L a multiple of U these are the definition's L outputs, for L = 61 the
    three outputs behind them as well); every other output is within the bound. In one call, and with the NaN in the history of a
    later call."""
    import torch
    import lora_sdr_amd as Lh
    K = 3
    rng = np.random.default_rng(6 + L)
    n = 3 * TILE + 11
    cut = TILE + 45
    x = _rows(rng, K, n)
    at_nan, at_pinf, at_ninf = cut - 3, 2 * TILE - 1, 2 * TILE + 9      # in the second call's history; the last lane of a tile; elsewhere
    x[0, at_nan] = np.float32("nan")
    x[1, at_pinf] = complex(np.float32("inf"), 1.0)
    x[2, at_ninf] = complex(0.5, -np.float32("inf"))
    freqs = np.array([0.0, 0.25, rng.uniform(-0.5, 0.5)])               # purely real and purely imaginary rotations included
    h = (Lh.design_lowpass(U, L) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    assert np.all(h != 0)
    nn = np.arange(n * U, dtype=np.int64)
    hit = np.zeros(n * U, bool)
    strict = np.zeros(n * U, bool)
    for m in (at_nan, at_pinf, at_ninf):
        hit |= (nn >= m * U) & (nn < m * U + reach(U, L))
        strict |= (nn >= m * U) & (nn < m * U + L)
    want = sd.synthesize_at(x, freqs, U, h, None, n=nn)
    assert np.array_equal(~np.isfinite(want), strict)                   # the definition itself: L outputs per sample
    assert hit.sum() == 3 * reach(U, L) and (L % U or np.array_equal(hit, strict))
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h)
        whole = sy.run(xd).cpu().numpy()
        sy.reset()
        two = np.concatenate([sy.run(xd[:, :cut]).cpu().numpy(), sy.run(xd[:, cut:]).cpu().numpy()])
        sy.close()
    scale = sd.error_scale(np.where(np.isfinite(x), x, 0), h, U)
    for y in (whole, two):
        bad = ~np.isfinite(y)
        print("synthesiser non-finite U=%d L=%d: %d non-finite outputs, %d by the definition (L), %d by the stated reach"
              % (U, L, bad.sum(), strict.sum(), hit.sum()))
        assert np.array_equal(bad, hit), (np.nonzero(bad != hit)[0][:10].tolist(), int(bad.sum()), int(hit.sum()))
        err = float(np.abs(y[~hit] - want[~hit]).max())
        assert err <= bound(K, U, L, scale), (err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# item 4: extreme amplitudes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("U,L", [(8, 64), (16, 128)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_follow_the_definition(gpu, U, L, amp):
    """inputs of the order of 1e-30 and of 1e30 on the 24-channel shapes: the same bound relative to the scale at that amplitude"""
    import torch
    import lora_sdr_amd as Lh
    K = 24
    rng = np.random.default_rng(60 + U)
    n = 2 * TILE + TILE // 3 + 7
    x = (_rows(rng, K, n) * np.float32(amp)).astype(np.complex64)
    freqs = np.concatenate([DYADIC, rng.uniform(-0.5, 0.5, K - len(DYADIC))])
    h = (Lh.design_lowpass(U, L) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    gains = rng.uniform(0.25, 2.0, K).astype(np.float32)
    want = sd.synthesize_at(x, freqs, U, h, gains, n=np.arange(n * U))
    scale = sd.error_scale(x, h, U, gains)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    # on the host first: normal numbers in, the definition finite with head room for every partial sum, and the bound far above
    # the smallest normal number times the number of terms, so flushing subnormal products cannot be what decides
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(parts).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < huge / 4 and bound(K, U, L, scale) > 1e2 * tiny * K * (L // U)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(K * (L // U))
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h, gains)
        y = sy.run(torch.from_numpy(x).cuda()).cpu().numpy()
        sy.close()
    assert np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max())
    print("synthesiser amplitude %g U=%d L=%d: err/scale = %.3g (bound %.3g)" % (amp, U, L, err / scale, bound(K, U, L, 1.0)))
    assert err <= bound(K, U, L, scale), (err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# item 5: more channels than one dimension of the history kernel's grid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_channels_than_one_grid_dimension(gpu):
    """K = 65535 + 9, U = 1, L = 3, two chunks: the history kernel walks the channels with its second AND third grid dimension. Six
    rows carry noise -- the first, the last of the first group, the two on either side of channel 65535, the last two -- and all
    others are zero, so that the bound counts six channels (exact zeros add nothing) and a history row that is lost or misplaced
    shows: the first two outputs of the second chunk are built from it."""
    import torch
    import lora_sdr_amd as Lh
    K, U, L, n, cut = 65535 + 9, 1, 3, 300, 131
    live = np.array([0, 7, 65534, 65535, 65536, K - 1])
    rng = np.random.default_rng(5)
    xl = _rows(rng, live.size, n)
    freqs = rng.uniform(-0.5, 0.5, K)
    h = np.array([0.75, -0.5, 0.625], np.float32)
    want = sd.synthesize_at(xl, freqs[live], U, h, None, n=np.arange(n))
    xd = torch.zeros((K, n), dtype=torch.complex64, device="cuda")
    xd[torch.from_numpy(live).cuda()] = torch.from_numpy(xl).cuda()
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h)
        whole = sy.run(xd).cpu().numpy()
        sy.reset()
        two = np.concatenate([sy.run(xd[:, :cut]).cpu().numpy(), sy.run(xd[:, cut:]).cpu().numpy()])
        sy.close()
    scale = sd.error_scale(xl, h, U)
    err = float(np.abs(two - want).max())
    print("synthesiser K=%d: err/scale = %.3g (bound for the 6 live rows %.3g)" % (K, err / scale, bound(live.size, U, L, 1.0)))
    assert err <= bound(live.size, U, L, scale), (err, scale)
    assert np.array_equal(_bits(two), _bits(whole))
    assert float(np.abs(want[cut:cut + 2]).min()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# item 6: 64-bit row addressing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_beyond_2_pow_31_samples(gpu):
    """in_stride = 2^28 + 5 and K = 9: row 8 starts 2^31 + 40 samples (16 GiB) into ONE uninitialised allocation of which only the
    columns used are filled; equal to the tight run bit for bit. Skipped only when less than that is free."""
    import torch
    import lora_sdr_amd as Lh
    K, U, L, n = 9, 8, 64, 2 * TILE + 37
    stride = (1 << 28) + 5
    need = 8 * ((K - 1) * stride + n) + (1 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    rng = np.random.default_rng(64)
    x = torch.from_numpy(_rows(rng, K, n)).cuda()
    freqs = rng.uniform(-0.5, 0.5, K)
    h = (Lh.design_lowpass(U, L) * U).astype(np.float32)
    big = torch.empty((K - 1) * stride + n, dtype=torch.complex64, device="cuda")
    rows = big.as_strided((K, n), (stride, 1))
    assert rows[8].data_ptr() - big.data_ptr() == 8 * ((1 << 31) + 40)
    rows.copy_(x)
    with Lh.Context(7) as ctx:
        sy = Lh.Synthesizer(ctx, freqs, U, h)
        tight = sy.run(x).cpu().numpy()
        sy.reset()
        cut = 100                                                # the history kernel reads the strided rows too
        loose = np.concatenate([sy.run(rows[:, :cut]).cpu().numpy(), sy.run(rows[:, cut:]).cpu().numpy()])
        sy.close()
    del big, rows
    assert np.array_equal(_bits(loose), _bits(tight))
    # row 8 is in the sum: without it the stream is another one
    assert float(np.abs(tight).max()) > 0.0 and np.isfinite(tight.view(np.float32)).all()
    want = sd.synthesize_at(x.cpu().numpy(), freqs, U, h, None, n=np.arange(n * U))
    scale = sd.error_scale(x.cpu().numpy(), h, U)
    assert float(np.abs(loose - want).max()) <= bound(K, U, L, scale)
