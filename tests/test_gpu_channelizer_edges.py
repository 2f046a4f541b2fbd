"""GPU: the channeliser at the edges its definition covers (lora_sdr_amd/csrc/lorahip_chan.hip against oracle/channelizer.py).

The kernel has nothing to be bit-exact with, so every test here compares with the float64 definition

    y_k[m] = sum_j h[j] x[n_m - j] exp(-2 pi i frac(w_k (n_m - j) / 2^64)),   n_m = (m + 1) D - 1

-- through oracle.channelizer.channelize for short streams from sample 0, and through `definition_at` below, which evaluates
the same sum for SELECTED outputs at absolute sample indices, for the calls of 2^29 outputs and the streams 2^31 samples deep
that nobody convolves on the host. `definition_at` itself is held to oracle.channelizer.channelize by the one test here without
the gpu marker.

Mixer accuracy (test_mixer_accuracy_relative_to_each_channel): a sum of unit tones, one per channel in its pass band; the
error is max|y - definition| / max|y_k| per channel, worst channel. "plain fp32" is the same definition in numpy float32
(product with the correctly rounded phasor, sequential accumulate) on the same inputs, measured by the test on the host; the
bound is 4 x that (the kernel sums pre-rotated taps in another order and composes the phasor from three fp32 factors):

    shape (instance)          plain fp32 vs float64    bound (4 x)    kernel vs float64 (MI355X)
    D = 8,  L = 64  (RM 2)    4.90e-7                  1.96e-6        7.05e-7
    D = 16, L = 128 (RM 1)    7.92e-7                  3.17e-6        1.16e-6

(the input is 24 unit tones, max|x| = 14.5 against max|y_k| between 1 and 4: the roundings scale with the input, which is why
these figures are a few times those of a single tone.) For scale: a build whose 2 pi / 2^32 constant in mixerPhase is off by
1e-5 -- a phase error of up to 8e-6 rad at the quadrant edges -- measures 8.1e-6 and 8.4e-6 here.
"""
import numpy as np
import pytest

TOL = 4e-6              # of sum|h| * max|x|: the tolerance of tests/test_gpu_channelizer.py
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# host side: the definition for selected outputs, the constructor's rule for the instance
# ---------------------------------------------------------------------------------------------------------------------------
def definition_at(x, x0, freqs, decim, taps, m):
    """float64 definition of the outputs with absolute indices m (int array) for every frequency: x[i] is the wideband sample of
    absolute index x0 + i, every sample outside x (and before the start of the stream) reads as 0. Returns (K, len(m)) complex128.
    The phase is the 64-bit integer product w_k * n read as signed, exactly as oracle/channelizer.py forms it."""
    from oracle import channelizer as oc
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    m = np.asarray(m, np.int64)
    D, L = int(decim), h.size
    out = np.empty((len(freqs), m.size), np.complex128)
    step = max(1, (1 << 20) // L)
    for a in range(0, m.size, step):
        n = ((m[a:a + step, None] + 1) * D - 1) - np.arange(L, dtype=np.int64)[None, :]        # absolute sample index per (m, j)
        i = n - int(x0)
        ok = (n >= 0) & (i >= 0) & (i < x.size)
        xs = np.where(ok, x[np.clip(i, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
        nu = n.astype(np.uint64)
        for k, f in enumerate(freqs):
            with np.errstate(over="ignore"):
                ph = (np.uint64(oc.phase_inc(f)) * nu).astype(np.int64)
            rot = np.exp(-2j * np.pi * (ph.astype(np.float64) * 2.0 ** -64))
            with np.errstate(invalid="ignore", over="ignore"):
                out[k, a:a + step] = np.sum(np.where(ok, h[None, :] * xs * rot, 0.0), axis=1)
    return out


def instance(decim, n_taps):
    """which kernel instance lorahip_channelizer_create selects: 2 output times per lane when the tile fits 64 KiB of LDS, 1 when it
    fits 160 KiB, 0 = refused. QP = (256 RM + (L - 1) / D + 1) | 1 slots per decimation phase, L = n_taps rounded up to even."""
    L = (int(n_taps) + 1) & ~1
    for rm, limit in ((2, 64 << 10), (1, 160 << 10)):
        qp = (256 * rm + (L - 1) // int(decim) + 1) | 1
        if int(decim) * qp * 8 <= limit:
            return rm
    return 0


def _stream(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_definition_at_equals_the_oracle_on_a_short_stream():
    """the helper against oracle.channelizer.channelize: all outputs, a scattered subset, a window of the stream given with its
    absolute position (samples before it zero), odd and even filter lengths, frequencies outside [-0.5, 0.5)"""
    from oracle import channelizer as oc
    rng = np.random.default_rng(1)
    for K, D, L, n in ((3, 5, 37, 2000), (2, 1, 2, 700), (9, 16, 128, 5000), (1, 7, 1, 300)):
        x = _stream(rng, n)
        freqs = rng.uniform(-1.5, 1.5, K)
        h = (rng.uniform(0.5, 1.5, L) * (oc.design_lowpass(D, L) if L > 1 else 1.0)).astype(np.float32)
        want = oc.channelize(x, freqs, D, h)
        got = definition_at(x, 0, freqs, D, h, np.arange(n // D))
        scale = np.abs(h).sum() * np.abs(x).max()
        assert np.abs(got - want).max() <= 1e-13 * scale            # float64 both: only the order of the sum differs
        pick = rng.choice(n // D, min(50, n // D), replace=False)
        assert np.array_equal(definition_at(x, 0, freqs, D, h, pick), got[:, pick])
        # the same stream preceded by zeros, handed over as a window with its absolute position
        off = 12345 * D + 3
        xz = np.concatenate([np.zeros(off, np.complex64), x])
        wantz = oc.channelize(xz, freqs, D, h)
        mz = np.arange(off // D, xz.size // D)
        assert np.abs(definition_at(x, off, freqs, D, h, mz) - wantz[:, mz]).max() <= 1e-13 * scale
    # instance(): the worked examples of the rule
    assert [instance(8, 64), instance(16, 128), instance(256, 65536)] == [2, 1, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# item 1: calls of more than 2^29 outputs per channel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K,D,n_out", [(1, 1, (1 << 29) + (1 << 20)), (9, 2, (1 << 29) + 4096)])
def test_one_call_beyond_2_pow_29_outputs(gpu, K, D, n_out):
    """one call may make up to 2^30 outputs per channel (8 GiB a row): every row is addressed with 64 bits. Compared with the
    definition: the first 4096 outputs, 4096 around m = 2^29, the last 4096 and 64 seeded blocks of 256 in between.
    Device memory: 8 bytes x (n_in + K n_out) for the two buffers plus one n_in-sized temporary while the input is made:
    about 15 GB for K = 1, D = 1 and 58 GB for K = 9, D = 2. Skipped only when less than that is free."""
    import torch
    import lora_sdr_amd as Lh
    n_in = n_out * D
    need = 8 * (2 * n_in + K * n_out) + (2 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GB of free device memory for a call of %d outputs x %d channels, %.1f GB free" % (need / 1e9, n_out, K, free / 1e9))
    rng = np.random.default_rng(K)
    h = np.array([0.75, -0.5], np.float32)
    freqs = np.concatenate([[0.0], rng.uniform(-0.5, 0.5, K - 1)])
    g = torch.Generator(device="cuda"); g.manual_seed(29 + K)
    x = torch.view_as_complex(torch.randn((n_in, 2), generator=g, device="cuda"))
    xmax = float(torch.view_as_real(x).abs().amax()) * np.sqrt(2.0)          # >= max|x|
    out = torch.full((K, n_out), float("nan"), dtype=torch.complex64, device="cuda")
    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, freqs, D, h)
        y = ch.run(x, out=out)
        assert y.shape == (K, n_out)
        torch.cuda.synchronize()
        ch.close()
    blocks = [(0, 4096), ((1 << 29) - 2048, 4096), (n_out - 4096, 4096)]
    blocks += [(int(s), 256) for s in np.sort(rng.integers(4096, n_out - 4096 - 256, 64))]
    tol = TOL * float(np.abs(h).sum()) * xmax
    bad = []
    for m0, cnt in blocks:
        lo = max(0, (m0 + 1) * D - 1 - (h.size - 1))
        hi = (m0 + cnt) * D
        want = definition_at(x[lo:hi].cpu().numpy(), lo, freqs, D, h, np.arange(m0, m0 + cnt))
        got = out[:, m0:m0 + cnt].cpu().numpy()
        wrong = ~(np.abs(got - want) <= tol)                                # a NaN left in place counts as wrong
        for k, i in zip(*np.nonzero(wrong)):
            bad.append((int(k), m0 + int(i)))
    assert not bad, "%d wrong outputs among the compared ones; the first (channel, m): %s; the last: %s" % (len(bad), bad[:6], bad[-3:])


# ---------------------------------------------------------------------------------------------------------------------------
# item 2: the mixer, relative to each channel's own output
# ---------------------------------------------------------------------------------------------------------------------------
QUADRANT_EDGES = (0x20000000, 0x60000000, 0xA0000000, 0xE0000000)       # where mixerPhase changes the quarter turn it takes out


def _mixer_case(D, L):
    """24 channels on a grid of 1/24, each nudged (by less than 1e-6 cycles per sample, in Python integers) so that the phase the
    kernel evaluates at the start of ONE tile -- the top 32 bits of w_k * ((mTile + 1) D - 1) -- lands where wanted: 16 units and
    2^11 units (of 2^-32 turn) on either side of each of the four quadrant edges, and eight places inside the quadrants. One unit
    tone per channel, delta_k off its centre inside the pass band; the stream starts at an odd absolute position behind zeros."""
    from oracle import channelizer as oc
    RM = instance(D, L)
    TM = 256 * RM
    K = 24
    x0 = 3 * (1 << 20) + 5 * D + 1                              # the zeros fed before the tones
    m_first = x0 // D
    m_tile = (m_first // TM + 2) * TM                           # the aimed tile: the third one the tones touch, filter long filled
    n_tile = (m_tile + 1) * D - 1
    targets = []
    for e in QUADRANT_EDGES:
        targets += [e - 16, e + 16]
    for e in QUADRANT_EDGES:
        targets += [e - (1 << 11), e + (1 << 11)]
    targets += [0x00000000 + 77, 0x40000000, 0x80000000 - 5, 0xC0000000 + 123, 0x10000000, 0x50000000, 0x90000000, 0xD0000000]
    assert len(targets) == K
    rng = np.random.default_rng(D * 1000 + L)
    freqs, tone_w = [], []
    for k in range(K):
        w0 = (int(round(((k - 11.5) / 24.0) % 1.0 * (1 << 53))) << 11) & M64
        want = ((targets[k] & 0xffffffff) << 32) + (1 << 31)
        r = (want - w0 * n_tile) & M64                          # phase still to be made up at n_tile
        dw = (r // (n_tile << 11)) << 11                        # a double holds 53 bits of the increment: w stays a multiple of 2^11
        w = (w0 + dw) & M64
        f = w / float(1 << 64)                                  # exact
        assert oc.phase_inc(f) == w and dw < (1 << 44)
        freqs.append(f)
        delta = int(rng.uniform(-0.3, 0.3) / D * (1 << 64))
        tone_w.append((w + delta) & M64)
    # what the test is for, checked on the host with integers: both sides of every edge within 2^-20 turn, and all four quadrants
    ph = [((w_ * n_tile) & M64) >> 32 for w_ in (oc.phase_inc(f) for f in freqs)]
    for e in QUADRANT_EDGES:
        assert any(e - (1 << 12) <= p < e for p in ph) and any(e <= p < e + (1 << 12) for p in ph), hex(e)
    assert {((p + 0x20000000) & 0xffffffff) >> 30 for p in ph} == {0, 1, 2, 3}
    n = 4 * TM * D + 3
    idx = np.arange(n, dtype=np.uint64) + np.uint64(x0)
    x = np.zeros(n, np.complex128)
    for wt in tone_w:
        with np.errstate(over="ignore"):
            x += np.exp(2j * np.pi * ((np.uint64(wt) * idx).astype(np.int64).astype(np.float64) * 2.0 ** -64))
    x = x.astype(np.complex64)
    h = oc.design_lowpass(D, L)
    m = np.arange(m_first + L // D + 1, (x0 + n) // D)         # the filter holds tone samples only
    assert m[0] <= m_tile and m_tile + TM <= m[-1] + 1          # lanes 0, 255, 256 (and 511) of the aimed tile are compared
    return dict(K=K, D=D, L=L, RM=RM, TM=TM, x0=x0, x=x, h=h, freqs=np.array(freqs), m=m, m_first=m_first)


def _plain_fp32(c):
    """the definition in numpy float32: h[j] * x[n - j] times the correctly rounded phasor, summed in the order of j"""
    from oracle import channelizer as oc
    x, h, D, L, x0, m = c["x"], c["h"], c["D"], c["L"], c["x0"], c["m"]
    out = np.empty((c["K"], m.size), np.complex64)
    n_m = (m + 1) * D - 1
    for k, f in enumerate(c["freqs"]):
        w = np.uint64(oc.phase_inc(f))
        acc = np.zeros(m.size, np.complex64)
        for j in range(L):
            n = n_m - j
            with np.errstate(over="ignore"):
                ph = (w * n.astype(np.uint64)).astype(np.int64).astype(np.float64) * 2.0 ** -64
            rot = np.exp(-2j * np.pi * ph).astype(np.complex64)
            acc = acc + (h[j] * x[n - x0]).astype(np.complex64) * rot
        out[k] = acc
    return out


def _rel_err(y, want):
    """max over channels of max|y_k - want_k| / max|want_k|"""
    return float((np.abs(y - want).max(axis=1) / np.abs(want).max(axis=1)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("D,L", [(8, 64), (16, 128)])
def test_mixer_accuracy_relative_to_each_channel(gpu, D, L):
    """see the table in the module docstring: kernel vs float64 within 4 x (plain fp32 vs float64), per channel relative to that
    channel's largest output, 24 channels whose tile-start phases sit on both sides of every quadrant edge of the sine/cosine"""
    import torch
    import lora_sdr_amd as Lh
    c = _mixer_case(D, L)
    assert c["RM"] == (2 if D == 8 else 1)
    want = definition_at(c["x"], c["x0"], c["freqs"], D, c["h"], c["m"])
    assert np.abs(want).max(axis=1).min() > 0.5                 # every channel carries its tone: |H(delta_k)| is of order 1
    plain = _rel_err(_plain_fp32(c), want)
    bound = 4.0 * plain
    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, c["freqs"], D, c["h"])
        ch.run(torch.zeros(c["x0"], dtype=torch.complex64, device="cuda"))
        y = ch.run(torch.from_numpy(c["x"]).cuda()).cpu().numpy()
        ch.close()
    got = y[:, c["m"] - c["m_first"]]
    per_channel = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    print("mixer accuracy D=%d L=%d RM=%d: plain fp32 %.3e, bound %.3e, kernel %.3e (worst channel %d)"
          % (D, L, c["RM"], plain, bound, per_channel.max(), int(per_channel.argmax())))
    # the yardstick itself is an fp32 rounding figure: at least half an ulp of one term, at most a random walk of L roundings of
    # the largest term
    ratio = float(np.abs(c["h"]).sum() * np.abs(c["x"]).max() / np.abs(want).max(axis=1).min())
    assert 2.0 ** -25 < plain < 2.0 ** -24 * np.sqrt(L) * ratio, (plain, ratio)
    assert per_channel.max() <= bound, (per_channel.max(), bound, per_channel.tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# item 3: 2^31 samples into a stream
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,L", [(8, 64), (16, 128)])
def test_noise_two_billion_samples_into_the_stream(gpu, D, L):
    """2^31 + 12345 zero samples, then three tiles' worth of noise in ragged chunks (the first shorter than the filter), 19
    channels (three groups, the last one partly filled): every output against the definition at absolute sample indices, and
    bit for bit against one call from the same stream position"""
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    K = 19
    TM = 256 * instance(D, L)
    rng = np.random.default_rng(31 + D)
    freqs = rng.uniform(-0.5, 0.5, K)
    h = (oc.design_lowpass(D, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    n = 3 * TM * D + 5
    x = _stream(rng, n)
    xd = torch.from_numpy(x).cuda()
    x0 = (1 << 31) + 12345
    zeros = torch.zeros(1 << 24, dtype=torch.complex64, device="cuda")
    sink = torch.empty((K, (1 << 24) // D + 1), dtype=torch.complex64, device="cuda")
    runs = []
    with Lh.Context(7) as ctx:
        for sizes in ([L // 2 - 1, 1, D - 1, TM * D + 3, 0, 7, n], [n]):
            ch = Lh.Channelizer(ctx, freqs, D, h)
            for _ in range(128):
                ch.run(zeros, out=sink)
            ch.run(zeros[:12345], out=sink)
            assert ch.out_count(D) == (x0 + D) // D - x0 // D
            parts, pos = [], 0
            for s in sizes:
                s = min(s, n - pos)
                parts.append(ch.run(xd[pos:pos + s]).cpu().numpy())
                pos += s
            assert pos == n
            runs.append(np.concatenate(parts, axis=1))
            ch.close()
    ragged, whole = runs
    m = np.arange(x0 // D, (x0 + n) // D)
    assert ragged.shape == whole.shape == (K, m.size)
    assert np.array_equal(_bits(ragged), _bits(whole))
    want = definition_at(x, x0, freqs, D, h, m)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(ragged - want).max())
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)


# ---------------------------------------------------------------------------------------------------------------------------
# item 4: row and capture strides wider than the data
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loose_strides_leave_the_padding_alone(gpu):
    """the raw entry points with out_stride = n_out + 37 and capture_stride = n_in + 101: the outputs are those of the tight
    layout bit for bit, every padding word of the output buffer keeps the NaN pattern it was filled with, and the NaN in the
    input padding reaches no output"""
    import ctypes as C
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    rng = np.random.default_rng(4)
    S, K, D, L, n_in = 3, 10, 8, 64, 7001
    n_out = n_in // D
    ostride, cstride = n_out + 37, n_in + 101
    PAT = np.uint32(0x7FC0BEEF)
    x = np.stack([_stream(rng, n_in) for _ in range(S)])
    freqs = rng.uniform(-0.5, 0.5, K)
    h = oc.design_lowpass(D, L)
    xd = torch.from_numpy(x).cuda()
    padded_in = torch.full((S, cstride), float("nan"), dtype=torch.complex64, device="cuda")
    padded_in[:, :n_in] = xd
    lib = Lh.load()

    def patterned(*shape):
        t = torch.from_numpy(np.full(shape + (2,), PAT, np.uint32).view(np.float32)).cuda()
        return torch.view_as_complex(t)

    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, freqs, D, h)
        tight_caps = ch.run_captures(xd).cpu().numpy()
        tight_run = ch.run(xd[1]).cpu().numpy()
        # run_captures, both strides loose
        out = patterned(S, K, ostride)
        got = C.c_size_t()
        ctx.use_torch_stream()
        Lh.api.check(lib.lorahip_channelizer_run_captures(ch._h, C.c_void_p(padded_in.data_ptr()), S, cstride, n_in,
                                                          C.c_void_p(out.data_ptr()), ostride, C.byref(got)), "run_captures")
        assert got.value == n_out
        caps = out.cpu().numpy()
        # run, loose row stride, from a fresh stream
        ch.reset()
        out1 = patterned(K, ostride)
        Lh.api.check(lib.lorahip_channelizer_run(ch._h, C.c_void_p(padded_in[1].data_ptr()), n_in, C.c_void_p(out1.data_ptr()), ostride,
                                                 C.byref(got)), "run")
        assert got.value == n_out
        one = out1.cpu().numpy()
        ch.close()
    assert np.array_equal(_bits(caps[:, :, :n_out]), _bits(tight_caps))
    assert np.all(_bits(caps[:, :, n_out:]) == PAT)
    assert np.isfinite(caps[:, :, :n_out].view(np.float32)).all()
    assert np.array_equal(_bits(one[:, :n_out]), _bits(tight_run))
    assert np.all(_bits(one[:, n_out:]) == PAT)
    assert np.array_equal(_bits(one[:, :n_out]), _bits(tight_caps[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# item 5: shapes on both sides of the instance choice, long filters, channel counts, frequencies
# ---------------------------------------------------------------------------------------------------------------------------
DYADIC = [0.375, 1.375, -0.625, 8.375, -0.5, 0.5, 3.0, -2.0, 0.49999999999999994]
#          K    D     L    frequencies (None: seeded in [-0.5, 0.5))
SHAPES = [(3,   15,   64,  None),          # 62040 B of LDS: the last D with two outputs per lane at 64 taps
          (3,   16,   64,  None),          # 66176 B: the first with one
          (3,   8,    4080, None),         # 65472 B: two
          (3,   8,    4096, None),         # 65600 B: one
          (2,   8,    4088, None),         # 65472 B still: the last length with two at D = 8
          (2,   8,    4090, None),         # 65600 B: the first with one
          (2,   79,   8,   None),          # 162424 B: the largest decimation a short filter fits with
          (2,   64,   4032, None),         # 163328 B: the longest filter at D = 64
          (2,   1,    4096, None),         # L = 16 x 256 D: the tile's input is nearly all filter span
          (3,   2,    3001, None),         # the same with an odd filter (padded to even on the old end)
          (5,   3,    2,   None),          # the shortest filter the inner loop takes whole
          (8,   8,    64,  None),          # one whole group
          (16,  8,    64,  None),          # two whole groups
          (17,  8,    64,  None),          # one channel over
          (300, 4,    16,  None),          # 38 groups
          (9,   8,    64,  DYADIC),        # outside [-0.5, 0.5), equal modulo 1, the ends of the interval
          (6,   16,   128, [-7.3, 2.6, 1e6 + 0.25, -1e6 - 0.125, 0.999999999, -0.999999999])]
REFUSED = [(2, 80, 8), (2, 64, 4034), (1, 256, 65536)]


def test_shape_list_sits_on_both_sides_of_both_boundaries():
    """a test of the list above: by the constructor's rule it holds neighbours on either side of the 64 KiB line (at fixed L and
    at fixed D) and of the 160 KiB line, and the refused shapes are the FIRST that do not fit"""
    inst = {(D, L): instance(D, L) for _, D, L, _ in SHAPES}
    assert inst[(15, 64)] == 2 and inst[(16, 64)] == 1
    assert inst[(8, 4080)] == 2 and inst[(8, 4096)] == 1 and inst[(8, 4088)] == 2 and instance(8, 4089) == inst[(8, 4090)] == 1
    assert inst[(79, 8)] == 1 and instance(80, 8) == 0 and all(instance(D, 8) for D in range(1, 80))
    assert inst[(64, 4032)] == 1 and instance(64, 4034) == 0 and instance(64, 4033) == 0
    assert all(instance(D, L) == 0 for _, D, L in REFUSED) and all(inst.values())
    assert {1, 2} <= set(inst.values())


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,L,freqs", SHAPES, ids=["K%d-D%d-L%d%s" % (s[0], s[1], s[2], "" if s[3] is None else "-f") for s in SHAPES])
def test_shape_edges_against_float64_definition(gpu, K, D, L, freqs):
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    rng = np.random.default_rng(K * 100003 + D * 101 + L)
    TM = 256 * instance(D, L)
    n = max(2 * TM * D, 2 * L) + TM * D // 2 + 7 * D + 3
    x = _stream(rng, n)
    f = rng.uniform(-0.5, 0.5, K) if freqs is None else np.array(freqs, np.float64)
    assert f.size == K
    h = (oc.design_lowpass(D, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    want = oc.channelize(x, f, D, h)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, f, D, h)
        whole = ch.run(xd).cpu().numpy()
        ch.reset()
        first = max(1, min(L // 2, n // 4))                     # shorter than the history (L - 1 + D samples), then one long chunk
        parts = [ch.run(xd[:first]).cpu().numpy(), ch.run(xd[first:]).cpu().numpy()]
        ch.close()
    assert whole.shape == want.shape == (K, n // D)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(whole - want).max())
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    if freqs is DYADIC:                                          # equal modulo 1 is the same channel, bit for bit
        for k in (1, 2, 3):
            assert np.array_equal(_bits(whole[k]), _bits(whole[0]))
        assert np.array_equal(_bits(whole[4]), _bits(whole[5])) and np.array_equal(_bits(whole[6]), _bits(whole[7]))


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,L", REFUSED)
def test_shapes_that_do_not_fit_are_refused(gpu, K, D, L):
    import lora_sdr_amd as Lh
    with Lh.Context(7) as ctx:
        with pytest.raises(Lh.LoraHipError):
            Lh.Channelizer(ctx, np.zeros(K), D, np.ones(L, np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# item 6: non-finite and extreme samples
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,L", [(8, 64), (16, 128)])
def test_non_finite_samples_reach_exactly_their_filter_span(gpu, D, L):
    """a NaN, a +Inf and a -Inf in the stream, all taps non-zero: output m is non-finite exactly when n_m - L < n_bad <= n_m for
    one of them, on every channel (the centre-frequency one with purely real taps included); every other output is within TOL"""
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    K = 11
    TM = 256 * instance(D, L)
    rng = np.random.default_rng(6 + D)
    n = 3 * TM * D + 11
    cut = TM * D + 5 * D + 2                                     # the stream is fed as [0, cut) and [cut, n)
    x = _stream(rng, n)
    at_nan = cut - 3                                             # inside what becomes the second call's history
    at_pinf = 2 * TM * D - 1                                     # the newest sample of the last output of a tile
    at_ninf = 2 * TM * D + 9 * D                                 # elsewhere; I and Q of different kinds
    x[at_nan] = np.float32("nan")
    x[at_pinf] = complex(np.float32("inf"), 1.0)
    x[at_ninf] = complex(0.5, -np.float32("inf"))
    freqs = np.concatenate([[0.0, 0.25], rng.uniform(-0.5, 0.5, K - 2)])
    h = (oc.design_lowpass(D, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    assert np.all(h != 0)
    n_m = (np.arange(n // D) + 1) * D - 1
    hit = np.zeros(n // D, bool)
    for b in (at_nan, at_pinf, at_ninf):
        hit |= (n_m - L < b) & (b <= n_m)
    assert 3 * (L // D) <= hit.sum() <= 3 * (L // D + 1) and hit[2 * TM - 1] and not hit[2 * TM - 2]
    want = definition_at(x, 0, freqs, D, h, np.arange(n // D))
    assert np.array_equal(~np.isfinite(want), np.broadcast_to(hit, want.shape))
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, freqs, D, h)
        y = np.concatenate([ch.run(xd[:cut]).cpu().numpy(), ch.run(xd[cut:]).cpu().numpy()], axis=1)
        ch.close()
    assert y.shape == want.shape
    assert np.array_equal(~np.isfinite(y), np.broadcast_to(hit, y.shape))
    scale = float(np.abs(h).sum() * np.abs(x[np.isfinite(x)]).max())
    err = float(np.abs(y[:, ~hit] - want[:, ~hit]).max())
    assert err <= TOL * scale, (err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("D,L", [(8, 64), (16, 128)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_follow_the_definition(gpu, D, L, amp):
    """inputs of the order of 1e-30 and of 1e30: the same tolerance relative to sum|h| max|x| at that scale"""
    import torch
    import lora_sdr_amd as Lh
    from oracle import channelizer as oc
    K = 9
    rng = np.random.default_rng(60 + D)
    n = 3 * 256 * instance(D, L) * D + 11
    x = (_stream(rng, n) * np.float32(amp)).astype(np.complex64)
    freqs = np.concatenate([[0.0], rng.uniform(-0.5, 0.5, K - 1)])
    h = (oc.design_lowpass(D, L) * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    want = oc.channelize(x, freqs, D, h)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    # on the host first: the inputs are normal numbers, the definition stays finite with head room for every partial sum, and
    # the tolerance itself is far above the smallest normal number, so flushing a subnormal product cannot be what decides
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(x.view(np.float32)).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < huge / 4 and TOL * scale > 1e2 * tiny
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)
    with Lh.Context(7) as ctx:
        ch = Lh.Channelizer(ctx, freqs, D, h)
        y = ch.run(torch.from_numpy(x).cuda()).cpu().numpy()
        ch.close()
    assert np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max())
    assert err <= TOL * scale, (err, scale)
