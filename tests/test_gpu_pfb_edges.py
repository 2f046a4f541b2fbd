"""GPU: the polyphase filter-bank channeliser at the edges its definition covers (lora_sdr_amd/csrc/lorahip_pfb.hip against
oracle/channelizer.py).

Row i of the bank is BY DEFINITION the direct-form channeliser's for freq = bins[i] / M, so every test here compares with

    y_b[m] = sum_{j<L} h[j] x[n_m - j] exp(-2 pi i b (n_m - j) / M),   n_m = (m + 1) D - 1

through `definition_at` of tests/test_gpu_channelizer_edges.py (the float64 definition for selected outputs at absolute sample
indices, held to oracle.channelizer.channelize there) with freqs = bins / M, within TOL = 4e-6 sum|h| max|x|.

    what                                                      test
    both sides of the 80 KiB line between the LDS copy of     test_shape_edges_against_float64_definition, every shape also in
    the input and reads from memory (M = 16, 64, 256, 512);   two chunks, bit for bit (the first shorter than the history: the
    D = 1, D = 4096; L = 1, M - 1, M, M + 1, 65536;           unstaged kernel then takes its bounds-checked loop, the staged
    n_sel = 1 and 5000                                         one its bounds-checked copy)
    one step outside each limit refused, with its reason      test_shapes_outside_the_limits_are_refused
    noise 2^31 samples into the stream, staged and unstaged   test_noise_two_billion_samples_into_the_stream
    NaN, +Inf, -Inf reach exactly the L outputs of the        test_non_finite_samples_reach_exactly_their_filter_span
    definition, also for L not a multiple of M
    1e-30 and 1e30                                            test_extreme_amplitudes_follow_the_definition
    a row 2^32 bytes and one 2^31 samples into the buffer     test_rows_beyond_2_pow_32_bytes

err / scale of every accuracy case is printed by the tests (`-s`). Measured on an MI355X, of sum|h| max|x| (TOL is 4e-6):

    22 shapes                      1.4e-9 .. 1.0e-7   (largest: M = 16, L = 1 at 1.0e-7; M = 8, L = 65536 at 8.1e-8)
    2^31 samples into the stream   3.3e-8 (16, 8, 64), 5.1e-9 (512, 640, 1000)
    1e-30 and 1e30                 2.8e-8 (16, 8, 64), 3.9e-9 .. 4.7e-9 (256, 320, 2048)

Non-finite samples: before every residue got its own number of fold rounds the kernel multiplied the zero padding of the tap table
and the test measured 30 non-finite output times instead of 24 at (16, 8, 67) and 6 instead of 4 at (512, 640, 1000).
"""
import numpy as np
import pytest

from test_gpu_channelizer_edges import definition_at, _bits, _stream

TOL = 4e-6              # of sum|h| * max|x|: the tolerance of tests/test_gpu_pfb.py
STAGE_LDS = 80 << 10


# ---------------------------------------------------------------------------------------------------------------------------
# host side: the constructor's rule, the shape list, which outputs are compared
# ---------------------------------------------------------------------------------------------------------------------------
def plan(M, D, L):
    """what lorahip_pfb_create derives from a shape: output times per tile T, fold rounds Q, padded length Lp, the tile's input span,
    and whether that span is copied to the LDS (it is when it fits beside the sums and the twiddles within 80 KiB)"""
    M, D, L = int(M), int(D), int(L)
    T = max(16, min(256, 4096 // M))
    Q = -(-L // M)
    Lp = Q * M
    fixed = (T * (M + 1) + M // 2) * 8
    span = (T - 1) * D + Lp
    return dict(T=T, Q=Q, Lp=Lp, span=span, lds=fixed + 8 * span, staged=fixed + 8 * span <= STAGE_LDS)


def check(M, D, L, n_sel):
    """lorahip_pfb_check restated"""
    return (8 <= M <= 1024 and M & (M - 1) == 0) and 1 <= D <= 4096 and 1 <= L <= 65536 and 1 <= n_sel <= 65535 * 8


#          M     D     L      rows (None: all bins; int: that many seeded bins, duplicates allowed)
SHAPES = [(16,   22,   128,   None),       # 81 792 B: the last D with the LDS copy at 128 taps
          (16,   23,   128,   None),       # 83 832 B: the first without
          (16,   16,   1792,  5),          # 81 856 B: the longest filter with the copy at D = 16
          (16,   16,   1793,  5),          # one tap more is one round more: 81 984 B, without
          (64,   87,   512,   None),       # 81 480 B: with
          (64,   88,   512,   None),       # 81 984 B: without
          (256,  263,  2048,  19),         # 81 864 B: with
          (256,  264,  2048,  19),         # 81 984 B: without
          (512,  84,   512,   19),         # 81 888 B: M = 512 with the copy
          (512,  85,   512,   19),         # 82 008 B: without
          (8,    1,    70,    None),       # the smallest D
          (1024, 1,    1500,  19),
          (8,    4096, 70,    None),       # the largest D, from memory
          (1024, 4096, 8192,  19),
          (16,   5,    1,     None),       # one tap: one round, Lp = M
          (32,   12,   31,    None), (32, 12, 32, None), (32, 12, 33, None),    # around one round
          (8,    8,    65536, 3),          # Q = 8192
          (1024, 1024, 65536, 2),          # the longest filter at the largest M
          (64,   48,   300,   1),          # the smallest selection
          (16,   16,   100,   5000)]       # the store loop over many duplicate rows
REFUSED = [(4, 4, 8, 4), (2048, 4, 8, 4), (24, 4, 8, 4), (16, 0, 8, 4), (16, 4097, 8, 4), (16, 4, 0, 4), (16, 4, 65537, 4),
           (16, 4, 8, 0), (16, 4, 8, 65535 * 8 + 1)]


def _taps(rng, D, L):
    from oracle import channelizer as oc
    h = oc.design_lowpass(D, L) if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)       # not symmetric: the tap order matters


def _bins(rng, M, rows):
    if rows is None:
        return None
    if rows <= 19:
        return np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:16]])[:rows].astype(np.int32) if rows > 1 else np.array([M - 27], np.int32)
    return rng.integers(-3 * M, 3 * M, rows).astype(np.int32)


def _length(M, D, L):
    """two tiles and a third of one plus a ragged tail, and long enough to fill the filter and cross a tile after that"""
    T = plan(M, D, L)["T"]
    return max((2 * T + T // 3 + 1) * D + 7, L + (T + T // 3) * D + 7)


def _compared(rng, n_out, T, L, K):
    """the output times a shape is compared at: all where that is cheap, otherwise the first and last, those around every tile
    boundary and seeded others"""
    if n_out * L * K <= 1.2e7:
        return np.arange(n_out, dtype=np.int64)
    m = set(range(3)) | set(range(n_out - 3, n_out))
    for b in range(T, n_out, T):
        m |= {b - 1, b}
    want = int(1.2e7 / (L * K))
    if want > len(m):
        m |= set(int(v) for v in rng.choice(n_out, min(n_out, want), replace=False)[:want - len(m)])
    else:
        m = set(sorted(m)[:: -(-len(m) // want)]) | {n_out - 1}
    return np.array(sorted(m), np.int64)


def test_shape_list_sits_on_both_sides_of_the_staging_line_and_inside_every_limit():
    """a test of the lists above by the constructor's rule: for M = 16, 64, 256 and 512 neighbours on either side of the 80 KiB
    line (in D, and in L for M = 16), every limit of lorahip_pfb_check reached from inside, and every refused shape one step
    outside exactly one limit"""
    p = {(M, D, L): plan(M, D, L) for M, D, L, _ in SHAPES}
    for M, D, L in ((16, 22, 128), (64, 87, 512), (256, 263, 2048), (512, 84, 512)):
        assert p[(M, D, L)]["staged"] and not p[(M, D + 1, L)]["staged"], (M, D, L)
        assert p[(M, D, L)]["lds"] <= STAGE_LDS < p[(M, D + 1, L)]["lds"]
    assert p[(16, 16, 1792)]["staged"] and not p[(16, 16, 1793)]["staged"]
    assert not p[(8, 4096, 70)]["staged"] and not p[(1024, 4096, 8192)]["staged"] and not p[(1024, 1, 1500)]["staged"]
    assert p[(8, 1, 70)]["staged"] and p[(16, 5, 1)]["Lp"] == 16 and p[(16, 5, 1)]["Q"] == 1
    assert [p[(32, 12, L)]["Q"] for L in (31, 32, 33)] == [1, 1, 2]
    assert p[(8, 8, 65536)]["Q"] == 8192 and p[(1024, 1024, 65536)]["Q"] == 64
    assert all(check(M, D, L, M if r is None else r) for M, D, L, r in SHAPES)
    assert {D for _, D, _, _ in SHAPES} >= {1, 4096} and {L for _, _, L, _ in SHAPES} >= {1, 65536}
    assert {r for _, _, _, r in SHAPES} >= {1, 5000}
    assert not any(check(*s) for s in REFUSED)
    inside = (16, 4, 8, 4)
    for s in REFUSED:                                            # one argument differs from an accepted shape
        assert sum(a != b for a, b in zip(s, inside)) == 1
    assert check(8, 1, 1, 1) and check(1024, 4096, 65536, 65535 * 8)


# ---------------------------------------------------------------------------------------------------------------------------
# item 1: shapes against the definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L,rows", SHAPES, ids=["M%d-D%d-L%d-%s" % (s[0], s[1], s[2], "all" if s[3] is None else "sel%d" % s[3]) for s in SHAPES])
def test_shape_edges_against_float64_definition(gpu, M, D, L, rows):
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M * 100003 + D * 101 + L)
    pl = plan(M, D, L)
    n = _length(M, D, L)
    x = _stream(rng, n)
    h = _taps(rng, D, L)
    bins = _bins(rng, M, rows)
    xd = torch.from_numpy(x).cuda()
    first = max(1, min(pl["Lp"] // 2, n // 4))                   # shorter than the history (Lp - 1 samples), then the rest
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        whole = pf.run(xd).cpu().numpy()
        pf.reset()
        parts = [pf.run(xd[:first]).cpu().numpy(), pf.run(xd[first:]).cpu().numpy()]
        b = pf.bins.astype(np.int64) % M
        pf.close()
    assert whole.shape == (b.size, n // D)
    assert np.array_equal(_bits(np.concatenate(parts, axis=1)), _bits(whole))
    uniq, where, inverse = np.unique(b, return_index=True, return_inverse=True)
    if uniq.size < b.size:                                       # duplicates equal their originals bit for bit
        assert np.array_equal(_bits(whole), _bits(whole[where][inverse]))
    m = _compared(rng, n // D, pl["T"], L, uniq.size)
    want = definition_at(x, 0, uniq / float(M), D, h, m)
    got = whole[where][:, m]
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(got - want).max())
    print("PFB edges M %d D %d L %d rows %d (%s): err / scale %.3g, %d outputs x %d bins compared"
          % (M, D, L, b.size, "LDS copy" if pl["staged"] else "from memory", err / scale, m.size, uniq.size))
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(L))
    assert m[-1] == n // D - 1 and (m[-1] + 1) * D - 1 >= L      # the filter is full in what is compared


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L,n_sel", REFUSED)
def test_shapes_outside_the_limits_are_refused(gpu, M, D, L, n_sel):
    import lora_sdr_amd as Lh
    lib = Lh.load()
    assert lib.lorahip_pfb_check(M, D, L, n_sel) == -1
    assert lib.lorahip_last_error().decode().startswith("polyphase channeliser:")
    with Lh.Context(7) as ctx:
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseChannelizer(ctx, M, D, np.ones(L, np.float32), np.zeros(n_sel, np.int32))
        assert lib.lorahip_last_error().decode().startswith("polyphase channeliser:")


# ---------------------------------------------------------------------------------------------------------------------------
# item 2: noise 2^31 samples into the stream
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(16, 8, 64), (512, 640, 1000)])
def test_noise_two_billion_samples_into_the_stream(gpu, M, D, L):
    """2^31 + 12345 zero samples, then three tiles' worth of noise in ragged chunks (the first shorter than the filter), with the
    input copied to the LDS (the first shape) and read from memory (the second): every output against the definition at absolute
    sample indices, and bit for bit against one call from the same stream position"""
    import torch
    import lora_sdr_amd as Lh
    pl = plan(M, D, L)
    assert pl["staged"] == (M == 16)
    T = pl["T"]
    rng = np.random.default_rng(31 + M)
    bins = np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:8]]).astype(np.int32)
    K = bins.size
    h = _taps(rng, D, L)
    n = 3 * T * D + 5
    x = _stream(rng, n)
    xd = torch.from_numpy(x).cuda()
    x0 = (1 << 31) + 12345
    zeros = torch.zeros(1 << 24, dtype=torch.complex64, device="cuda")
    sink = torch.empty((K, (1 << 24) // D + 1), dtype=torch.complex64, device="cuda")
    runs = []
    with Lh.Context(7) as ctx:
        for sizes in ([L // 2 - 1, 1, D - 1, T * D + 3, 0, 7, n], [n]):
            pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
            for _ in range(128):
                pf.run(zeros, out=sink)
            pf.run(zeros[:12345], out=sink)
            assert pf.out_count(D) == (x0 + D) // D - x0 // D
            parts, pos = [], 0
            for s in sizes:
                s = min(s, n - pos)
                parts.append(pf.run(xd[pos:pos + s]).cpu().numpy())
                pos += s
            assert pos == n
            runs.append(np.concatenate(parts, axis=1))
            pf.close()
    ragged, whole = runs
    m = np.arange(x0 // D, (x0 + n) // D)
    assert ragged.shape == whole.shape == (K, m.size)
    assert np.array_equal(_bits(ragged), _bits(whole))
    want = definition_at(x, x0, bins / float(M), D, h, m)
    scale = float(np.abs(h).sum() * np.abs(x).max())
    err = float(np.abs(ragged - want).max())
    print("PFB deep stream M %d D %d L %d: err / scale %.3g" % (M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)


# ---------------------------------------------------------------------------------------------------------------------------
# item 3: non-finite samples
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(16, 8, 64), (16, 8, 67), (512, 640, 1000)])
def test_non_finite_samples_reach_exactly_their_filter_span(gpu, M, D, L):
    """a NaN, a +Inf and a -Inf in the stream, all taps non-zero: output m of every selected row is non-finite exactly when
    n_m - L < n_bad <= n_m for one of them -- also where L is not a multiple of M and the tap table is padded to whole rounds:
    every residue runs its own number of rounds, so no product with the padding is formed --; every other output is within TOL.
    The stream is fed in two calls with the NaN in the history of the second."""
    import torch
    import lora_sdr_amd as Lh
    pl = plan(M, D, L)
    assert pl["staged"] == (M == 16)
    T = pl["T"]
    rng = np.random.default_rng(6 + L)
    n = 3 * T * D + 3 * L + 20 * D + 11
    cut = T * D + L + 5 * D + 2                                  # the stream is fed as [0, cut) and [cut, n)
    x = _stream(rng, n)
    at_nan = cut - 3                                             # inside what becomes the second call's history
    m1 = 2 * T + L // D + 2
    at_pinf = (m1 + 1) * D - 1 - L - 3                           # L + 3 samples before an output: inside the padding where L < Lp
    at_ninf = (m1 + 1 + L // D + 9) * D - 1 - L                  # L before another: the first sample the definition excludes
    assert at_nan + L < at_pinf and at_pinf + L < at_ninf and at_ninf + L < n
    x[at_nan] = np.float32("nan")
    x[at_pinf] = complex(np.float32("inf"), 1.0)
    x[at_ninf] = complex(0.5, -np.float32("inf"))
    bins = None if M == 16 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:8]]).astype(np.int32)
    h = _taps(rng, D, L)
    assert np.all(h != 0)
    n_m = (np.arange(n // D) + 1) * D - 1
    hit = np.zeros(n // D, bool)
    padded = np.zeros(n // D, bool)
    for b in (at_nan, at_pinf, at_ninf):
        hit |= (n_m - L < b) & (b <= n_m)
        padded |= (n_m - pl["Lp"] < b) & (b <= n_m)
    freqs = (np.arange(M) if bins is None else bins) / float(M)
    want = definition_at(x, 0, freqs, D, h, np.arange(n // D))
    assert np.array_equal(~np.isfinite(want), np.broadcast_to(hit, want.shape))
    assert L % M == 0 or (padded & ~hit).any()                   # the padding would reach outputs the definition excludes
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        whole = pf.run(xd).cpu().numpy()
        pf.reset()
        two = np.concatenate([pf.run(xd[:cut]).cpu().numpy(), pf.run(xd[cut:]).cpu().numpy()], axis=1)
        pf.close()
    scale = float(np.abs(h).sum() * np.abs(x[np.isfinite(x)]).max())
    for y in (whole, two):
        assert y.shape == want.shape
        bad = ~np.isfinite(y)
        print("PFB non-finite M %d D %d L %d: %d non-finite output times, %d by the definition, %d if the padding counted"
              % (M, D, L, bad.any(axis=0).sum(), hit.sum(), padded.sum()))
        assert np.array_equal(bad, np.broadcast_to(hit, y.shape)), (np.nonzero(bad.any(axis=0) != hit)[0][:10].tolist(), int(hit.sum()))
        err = float(np.abs(y[:, ~hit] - want[:, ~hit]).max())
        assert err <= TOL * scale, (err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# item 4: extreme amplitudes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(16, 8, 64), (256, 320, 2048)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_follow_the_definition(gpu, M, D, L, amp):
    """inputs of the order of 1e-30 and of 1e30: the same tolerance relative to sum|h| max|x| at that scale"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(60 + M)
    T = plan(M, D, L)["T"]
    n = _length(M, D, L)
    x = (_stream(rng, n) * np.float32(amp)).astype(np.complex64)
    bins = None if M == 16 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:8]]).astype(np.int32)
    freqs = (np.arange(M) if bins is None else bins) / float(M)
    h = _taps(rng, D, L)
    want = definition_at(x, 0, freqs, D, h, np.arange(n // D))
    scale = float(np.abs(h).sum() * np.abs(x).max())
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    # on the host first, as tests/test_gpu_channelizer_edges.py does: normal numbers in, the definition finite with head room for
    # every partial sum, and the tolerance itself far above the smallest normal number
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(parts).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < huge / 4 and TOL * scale > 1e2 * tiny
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        y = pf.run(torch.from_numpy(x).cuda()).cpu().numpy()
        pf.close()
    assert np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max())
    print("PFB amplitude %g M %d D %d L %d: err / scale %.3g" % (amp, M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# item 5: 64-bit row addressing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_beyond_2_pow_32_bytes(gpu):
    """out= is a strided view of ONE uninitialised allocation with out_stride = 2^28 + 5 and 9 rows: row 2 lies beyond 2^32 bytes,
    row 8 beyond 2^31 samples. The outputs equal the tight run's bit for bit, and a guard band of 64 marked samples on either side
    of every row's run is unchanged. Skipped only when less than 18 GB are free."""
    import torch
    import lora_sdr_amd as Lh
    M, D, L, K, G = 16, 8, 64, 9, 64
    stride = (1 << 28) + 5
    T = plan(M, D, L)["T"]
    n = (2 * T + 37) * D + 3
    n_out = n // D
    total = (K - 1) * stride + 2 * G + n_out
    need = 8 * total + (1 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    rng = np.random.default_rng(64)
    x = torch.from_numpy(_stream(rng, n)).cuda()
    h = _taps(rng, D, L)
    bins = rng.permutation(M)[:K].astype(np.int32)
    PAT = np.uint32(0x7FC0BEEF)
    marker = torch.view_as_complex(torch.from_numpy(np.full((K, n_out + 2 * G, 2), PAT, np.uint32).view(np.float32)).cuda())
    big = torch.empty(total, dtype=torch.complex64, device="cuda")
    framed = big.as_strided((K, n_out + 2 * G), (stride, 1))
    framed.copy_(marker)
    out = big.as_strided((K, n_out), (stride, 1), G)
    assert out[2].data_ptr() - big.data_ptr() > 1 << 32 and out[8].data_ptr() - big.data_ptr() > 8 << 31
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer(ctx, M, D, h, bins)
        tight = pf.run(x).cpu().numpy()
        pf.reset()
        got = pf.run(x, out=out)
        assert got.data_ptr() == out.data_ptr() and got.shape == (K, n_out)
        after = framed.cpu().numpy()
        pf.close()
    del big, framed, out, got
    assert np.array_equal(_bits(after[:, G:G + n_out]), _bits(tight))
    assert np.all(_bits(after[:, :G]) == PAT) and np.all(_bits(after[:, G + n_out:]) == PAT)
    assert np.isfinite(tight.view(np.float32)).all() and float(np.abs(tight).max()) > 0.0
