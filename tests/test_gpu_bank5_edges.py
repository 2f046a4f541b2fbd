"""GPU: the two polyphase banks on 5 * 2^a bins at the edges their definitions cover (PolyphaseChannelizer.radix5 and
PolyphaseSynthesizer.radix5: the M = 5 .. 320 instances of pfbChannelize<M>, psbTransform / psbFold / psbHistory<M> in
lora_sdr_amd/csrc/lorahip_pfb.hip and lorahip_psb.hip) -- the places where these instances differ from the power-of-two ones that
tests/test_gpu_pfb_edges.py and tests/test_gpu_psb_edges.py hold.

The yardsticks are the float64 evaluations tests/pfb_def.py::channelize and tests/psb_def.py::synthesize / synthesize_at with their n0
argument: the phase is exp(-+2 pi i ((b mod M) (n mod M) mod M) / M) with n the absolute 64-bit index, reduced in integers before any
floating point sees it (at n = 4.3e9 the product 2 pi (b / M) n in float64 is off by 1e-6 rad, the order of the tolerance, because
b / M is inexact for these M). tests/test_pfb5_cpu.py and tests/test_psb5_cpu.py hold n0 to explicit zeros, hold these evaluations to
the direct forms, and show in integers that the two deep positions used here move every residue under a 32-bit or 31-bit position.
Tolerances: TOL = 4e-6 of sum|h| max|x| (channeliser) and of synthesizer_def.error_scale (synthesis bank), the project's front-end
tolerance.

    what                                                      test
    plan5() restates lorahip_psb_create_radix5; the segment   test_segment_shapes_sit_where_they_claim (no gpu marker)
    list below by that rule: seg mod M, seg mod T, HC
    against seg
    channeliser: noise 2^31 + 12345 and 2^32 + 54321          test_channeliser_noise_beyond_2_pow_31_and_2_pow_32: one object a
    samples into the stream, with the LDS copy (5, 8, 37)     shape, zeros in between, ragged calls (the first shorter than the
    and from memory (320, 512, 1000): for these M the          history, one empty), every output against the definition at
    position modulo M is a true remainder of 64 bits          absolute indices, out_count at both places, reset and position 0
    synthesis bank: the same in input times, (5, 3, 20) and   test_synthesis_noise_beyond_2_pow_31_and_2_pow_32
    (10, 3, 20), three rows of which two share a bin
    synthesis bank: a second workspace segment that starts    test_segments_of_the_synthesis_bank: one call, the ragged chunks
    at a non-zero phase and inside a tile (M = 20, 160);      of tests/test_gpu_psb.py and chunks cut at seg - 1, seg, seg + 1,
    history one short of, equal to and longer than a          bit for bit; the definition around every segment boundary, in
    segment (M = 320: 13107 input times); a last segment      the last HC input times and at seeded others
    shorter than the history and a call that reaches back
    through it (M = 5, U = 1)
    channeliser: NaN, +Inf, -Inf reach exactly the L          test_non_finite_samples_reach_exactly_their_filter_span
    outputs of the definition (L no multiple of M: a count
    by the padded length would differ)
    1e-30 and 1e30 on either bank                             test_extreme_amplitudes_channeliser, test_extreme_amplitudes_synthesis
    bins INT32_MIN, INT32_MAX, -1, M, -M - 1, 0 are the       test_extreme_bins_channeliser, test_extreme_bins_synthesis
    rows of their residues in [0, M), bit for bit

NOT here, on purpose: rows beyond 2^32 bytes, calls of 2^30 outputs and the largest row count. The store and launch code they reach
does not depend on M, and the power-of-two files hold it (test_rows_beyond_2_pow_32_bytes, test_row_beyond_2_pow_31_samples,
test_calls_of_2_pow_30_outputs, test_most_rows_the_check_accepts).

err / scale of every accuracy case is printed by the tests (`-s`). Measured on an MI355X (TOL is 4e-6; the other radix-5 files
measure 3.6e-9 .. 1.6e-7):

    deep stream, channeliser       3.1e-8 .. 3.8e-8 (5, 8, 37), 3.7e-9 .. 5.4e-9 (320, 512, 1000)   at 2^31 + 12345, 2^32 + 54321 and 0
    deep stream, synthesis bank    5.5e-8 .. 7.1e-8 (5, 3, 20), 4.5e-8 .. 6.0e-8 (10, 3, 20)        at the same input times
    segments                       3.1e-8 (M = 20), 3.3e-8 (M = 160), 1.7e-8, 1.7e-8, 1.4e-8 (M = 320: HC = 13106, 13107, 16383),
                                   1.9e-8 (M = 5, U = 1, two calls)
    non-finite, the other outputs  3.3e-8 (5, 8, 67), 1.0e-8 (40, 64, 323), 5.2e-9 (320, 512, 1000)
    1e-30 and 1e30, channeliser    2.4e-8 .. 2.6e-8 (10, 16, 80), 4.5e-9 (160, 256, 1283)
    1e-30 and 1e30, synthesis      2.7e-8 .. 3.2e-8 (10, 16, 80), 2.7e-8 .. 3.2e-8 (160, 256, 1283)
    extreme bins                   3.6e-8, 4.1e-9 (channeliser, M = 5, 320), 3.2e-8, 2.3e-8 (synthesis bank)

Nothing is above 1e-6; the deep positions measure what position 0 measures. Non-finite samples: 24 non-finite output times at
(5, 8, 67), 15 at (40, 64, 323) and 4 at (320, 512, 1000), the definition's counts; a count by the padded length would give 26, 17
and 7. The whole file takes 5 s on an MI355X (25 device cases, the slowest 0.4 s).

That these tests can fail was shown once with one-line changes that move a residue inside [0, M) and nothing else:
unsigned(nFirst) % M in pfbChannelize fails both channeliser deep-stream cases, unsigned(a.m0) % M in psbFold both synthesis
deep-stream cases, and the first segment's position given to every segment of a call in psbRun fails the five segment shapes with
seg mod M != 0 (the sixth, M = 5, has seg mod M == 0 and cannot see it).
"""
import numpy as np
import pytest

import pfb_def as fd
import psb_def as yd
import synthesizer_def as sd
import test_gpu_pfb5 as rx5                 # plan(), _taps, _stream of the channeliser's radix-5 file; none of its tests
import test_gpu_psb5 as tx5                 # _tile, _taps, _rows, RAGGED of the synthesis bank's
from test_gpu_psb_edges import _all_phases, _flat_taps, segments

TOL = 4e-6
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
DEEP = ((1 << 31) + 12345, (1 << 32) + 54321)      # tests/test_pfb5_cpu.py, tests/test_psb5_cpu.py: a 32-bit position shows at both
ZEROS = 1 << 24
_bits = rx5._bits


# ---------------------------------------------------------------------------------------------------------------------------
# host side: the constructor's rule for the synthesis bank, the segment list, which outputs are compared
# ---------------------------------------------------------------------------------------------------------------------------
def plan5(M, U, L):
    """what lorahip_psb_create_radix5 derives from a shape: input times per workgroup T (the largest power of two with T M <= 4096,
    8 at least and 256 at most), input times per workspace segment, taps per phase I and the history HC in input times"""
    M, U, L = int(M), int(U), int(L)
    I = -(-L // U)
    T = max(8, min(256, 1 << ((4096 // M).bit_length() - 1)))
    return dict(T=T, seg=min((1 << 22) // M, (1 << 30) // U), I=I, HC=I - 1)


#       M    U  L      n                a second call
SEGS = [(20,  3, 20,    2 * 209715 + 11, 0),           # the second segment starts at phase 15 and inside a tile
        (160, 3, 20,    2 * 26214 + 11,  0),           # the same at another M
        (320, 4, 52428, 3 * 13107 + 7,   0),           # HC = 13106: history one short of a segment
        (320, 4, 52432, 3 * 13107 + 7,   0),           # HC = 13107: equal to a segment
        (320, 4, 65536, 3 * 13107 + 7,   0),           # HC = 16383: longer than a segment (and the longest filter)
        (5,   1, 300,   838860 + 5,      400)]         # a last segment of 5 input times, HC = 299; the next call reaches back through it


def _seg_compared(rng, M, U, L, n, follow, K):
    """the outputs a SEGS shape is compared at: every phase of the first input times, of those where the filter is first full, of the
    two either side of every segment boundary of both calls, of the last three, of seeded ones among the last HC, and of seeded others
    up to a budget"""
    pl = plan5(M, U, L)
    total = n + follow
    m = set(range(3)) | set(range(total - 3, total)) | {t for t in (pl["I"] - 2, pl["I"] - 1, pl["I"]) if 0 <= t < total}
    for first, cnt in [(0, n)] + ([(n, follow)] if follow else []):
        for a, _ in segments(cnt, pl["seg"]):
            m |= {t for t in range(first + a - 2, first + a + 2) if 0 <= t < total}
    lo = max(0, total - pl["HC"])
    m |= set(int(v) for v in rng.choice(np.arange(lo, total), min(8, total - lo), replace=False))
    want = int(2e7 / (U * pl["I"] * K))
    if want > len(m):
        m |= set(int(v) for v in rng.choice(total, min(total, want), replace=False)[:want - len(m)])
    return _all_phases(sorted(m), U)


def test_segment_shapes_sit_where_they_claim():
    """the list above by the constructor's rule: a segment that is a multiple of neither M nor T (a power of two gives a multiple of
    both), HC below, equal to and above a segment, a last segment shorter than HC; and the compared outputs reach both sides of every
    segment boundary and the last HC input times"""
    assert [plan5(M, 3, 20)["T"] for M in tx5.RADIX5] == [256, 256, 128, 64, 32, 16, 8]
    assert all(plan5(M, 3, 20)["T"] == tx5._tile(M) for M in tx5.RADIX5)
    p = [plan5(M, U, L) for M, U, L, _, _ in SEGS]
    assert [q["seg"] for q in p] == [209715, 26214, 13107, 13107, 13107, 838860]
    assert [q["seg"] % M for (M, _, _, _, _), q in zip(SEGS, p)] == [15, 134, 307, 307, 307, 0]       # the phase a second segment starts at
    assert [q["seg"] % q["T"] for q in p] == [51, 6, 3, 3, 3, 204]                                    # ... and its place in a tile
    assert plan5(320, 4096, 1)["seg"] == 13107 and plan5(5, 4096, 1)["seg"] == 1 << 18                 # M decides, then 2^30 / U
    assert [q["HC"] for q in p[2:5]] == [p[2]["seg"] - 1, p[2]["seg"], 16383] and SEGS[4][2] == 65536
    assert [len(segments(n, q["seg"])) for (_, _, _, n, _), q in zip(SEGS, p)] == [3, 3, 4, 4, 4, 2]
    assert all(segments(n, q["seg"])[-1][1] < q["seg"] for (_, _, _, n, _), q in zip(SEGS, p))         # a ragged last segment
    M, U, L, n, follow = SEGS[5]
    assert segments(n, p[5]["seg"])[-1][1] == 5 < p[5]["HC"] == 299 < follow and U == 1
    lib_limits = [M in tx5.RADIX5 and 1 <= U <= 4096 and 1 <= L <= 65536 for M, U, L, _, _ in SEGS]
    assert all(lib_limits)
    rng = np.random.default_rng(0)
    for (M, U, L, n, follow), q in zip(SEGS, p):
        idx = _seg_compared(rng, M, U, L, n, follow, 3)
        got = set((idx // U).tolist())
        for a, _ in segments(n, q["seg"])[1:]:
            assert {a - 1, a} <= got
        assert n + follow - 1 in got and len([t for t in got if t >= n + follow - q["HC"]]) >= min(8, q["HC"])
        assert idx.size * q["I"] * 3 <= 4e7


def _ragged(total):
    sizes, pos = [], 0
    while pos < total:
        sizes.append(min(tx5.RAGGED[len(sizes) % len(tx5.RAGGED)], total - pos))
        pos += sizes[-1]
    return sizes


# ---------------------------------------------------------------------------------------------------------------------------
# item 1: deep stream positions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(5, 8, 37), (320, 512, 1000)])
def test_channeliser_noise_beyond_2_pow_31_and_2_pow_32(gpu, M, D, L):
    """zeros up to 2^31 + 12345, three tiles' worth of noise in ragged calls (the first shorter than the history, one empty), zeros up
    to 2^32 + 54321, the same noise again, reset, the same noise at position 0: ONE object, every output of the three stretches
    against the float64 definition at absolute indices. The first shape copies its input to the LDS, the second reads memory."""
    import torch
    import lora_sdr_amd as Lh
    pl = rx5.plan(M, D, L)
    assert pl["staged"] == (M == 5)
    T = pl["T"]
    rng = np.random.default_rng(31 + M)
    bins = None if M == 5 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:8]]).astype(np.int32)
    K = M if bins is None else bins.size
    h = rx5._taps(rng, D, L)
    n = 3 * T * D + 5
    x = rx5._stream(rng, n)
    xd = torch.from_numpy(x).cuda()
    sizes = [L // 2 - 1, 1, D - 1, T * D + 3, 0, 7, n]
    assert 0 < sizes[0] < pl["Lp"] - 1 and sum(sizes[:-1]) < n
    zeros = torch.zeros(ZEROS, dtype=torch.complex64, device="cuda")
    sink = torch.empty((K, ZEROS // D + 1), dtype=torch.complex64, device="cuda")
    got = []
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        pos = 0
        for x0 in DEEP + (0,):
            if x0 == 0:
                pf.reset()
                pos = 0
            assert x0 == 0 or x0 - pos > pl["Lp"]                # the history of the stretch is zeros, as the definition has it
            while pos < x0:
                s = min(ZEROS, x0 - pos)
                pf.run(zeros[:s], out=sink)
                pos += s
            assert pf.out_count(D) == (x0 + D) // D - x0 // D and pf.out_count(1) == (x0 + 1) // D - x0 // D
            parts, fed = [], 0
            for s in sizes:
                s = min(s, n - fed)
                assert pf.out_count(s) == (pos + s) // D - pos // D
                parts.append(pf.run(xd[fed:fed + s]).cpu().numpy())
                fed += s
                pos += s
            assert fed == n and pos == x0 + n
            got.append(np.concatenate(parts, axis=1))
        pf.close()
    scale = fd.scale(x, h)
    for x0, y in zip(DEEP + (0,), got):
        want = fd.channelize(x, M, D, h, bins, n0=x0)
        assert y.shape == want.shape == (K, (x0 + n) // D - x0 // D)
        err = float(np.abs(y - want).max())
        print("bank5 deep stream, channeliser M %d D %d L %d (%s) at %d: err / scale %.3g"
              % (M, D, L, "LDS copy" if pl["staged"] else "from memory", x0, err / scale))
        assert err <= TOL * scale, (x0, err, scale)
        assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", [(5, 3, 20), (10, 3, 20)])
def test_synthesis_noise_beyond_2_pow_31_and_2_pow_32(gpu, M, U, L):
    """the same in input times: zeros up to input time 2^31 + 12345, three tiles' worth of noise on three rows (two of them on one
    bin) in ragged calls, zeros up to 2^32 + 54321, the noise again, reset, the noise at position 0. U = 3 is no multiple of 5, so
    the residue (m U + p) mod M moves with a position cut to 32 bits (tests/test_psb5_cpu.py)."""
    import torch
    import lora_sdr_amd as Lh
    pl = plan5(M, U, L)
    T = pl["T"]
    rng = np.random.default_rng(32 + M)
    bins = np.array([2, 2 - M, M - 1], np.int32)
    K = bins.size
    assert bins[0] % M == bins[1] % M != bins[2] % M and U % 5
    h = tx5._taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    n = 3 * T + 5
    x = tx5._rows(rng, K, n)
    xd = torch.from_numpy(x).cuda()
    sizes = [pl["HC"] // 2, 1, T + 3, 0, 7, n]
    assert 0 < sizes[0] < pl["HC"] and sum(sizes[:-1]) < n
    zeros = torch.zeros((K, ZEROS), dtype=torch.complex64, device="cuda")
    sink = torch.empty(ZEROS * U, dtype=torch.complex64, device="cuda")
    got = []
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        pos = 0
        for x0 in DEEP + (0,):
            if x0 == 0:
                ps.reset()
                pos = 0
            assert x0 == 0 or x0 - pos > pl["HC"]
            while pos < x0:
                s = min(ZEROS, x0 - pos)
                ps.run(zeros[:, :s], out=sink)
                pos += s
            parts, fed = [], 0
            for s in sizes:
                s = min(s, n - fed)
                assert ps.out_count(s) == s * U
                parts.append(ps.run(xd[:, fed:fed + s]).cpu().numpy())
                fed += s
                pos += s
            assert fed == n and pos == x0 + n
            got.append(np.concatenate(parts))
        ps.close()
    scale = sd.error_scale(x, h, U, g)
    for x0, y in zip(DEEP + (0,), got):
        want = yd.synthesize(x, M, U, h, bins, g, n0=x0)
        assert y.shape == want.shape == (n * U,)
        err = float(np.abs(y - want).max()) / scale
        print("bank5 deep stream, synthesis M %d U %d L %d at input time %d: err / scale %.3g" % (M, U, L, x0, err))
        assert err <= TOL, (x0, err)
        assert float(np.abs(want).max()) / scale > 0.05 / np.sqrt(K * pl["I"])


# ---------------------------------------------------------------------------------------------------------------------------
# item 2: the workspace segments of the synthesis bank
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L,n,follow", SEGS, ids=["M%d-U%d-L%d-n%d" % s[:4] for s in SEGS])
def test_segments_of_the_synthesis_bank(gpu, M, U, L, n, follow):
    """one call (and, for the shape with a second call, that call behind it); ragged chunks and chunks cut at seg - 1, seg and
    seg + 1, bit for bit against it; the sampled float64 definition. Flat taps: every tap of the long filters, and so every row of
    a long history, weighs above TOL."""
    import torch
    import lora_sdr_amd as Lh
    pl = plan5(M, U, L)
    seg, total = pl["seg"], n + follow
    rng = np.random.default_rng(M + U + L)
    bins = np.array([1 - M, M // 2 + 1, 3 * M + 2], np.int32)
    K = bins.size
    x = tx5._rows(rng, K, total)
    h = _flat_taps(rng, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    cuts = [seg - 1, 1, 1, seg, seg + 1, total]                  # ends at seg - 1, seg, seg + 1; calls of seg and of seg + 1 input times
    ways = [_ragged(total), cuts] + ([[total]] if follow else [])
    runs = []
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        whole = torch.cat([ps.run(xd[:, :n])] + ([ps.run(xd[:, n:])] if follow else [])).cpu().numpy()
        for sizes in ways:
            ps.reset()
            parts, pos = [], 0
            for s in sizes:
                s = min(s, total - pos)
                parts.append(ps.run(xd[:, pos:pos + s]))
                pos += s
            assert pos == total
            runs.append(torch.cat(parts).cpu().numpy())
        ps.close()
    assert whole.shape == (total * U,)
    for sizes, y in zip(ways, runs):
        assert np.array_equal(_bits(y), _bits(whole)), sizes[:6]
    idx = _seg_compared(rng, M, U, L, n, follow, K)
    want = yd.synthesize_at(x, M, U, h, bins, g, n=idx)
    scale = sd.error_scale(x, h, U, g)
    err = float(np.abs(whole[idx] - want).max()) / scale
    print("bank5 segments M %d U %d L %d (HC %d, segment %d = %d mod M, %d mod T) n %d%s: err / scale %.3g, %d outputs compared"
          % (M, U, L, pl["HC"], seg, seg % M, seg % pl["T"], n, " + %d" % follow if follow else "", err, idx.size))
    assert err <= TOL, err
    assert float(np.abs(want).max()) / scale > 0.05 / np.sqrt(K * pl["I"])


# ---------------------------------------------------------------------------------------------------------------------------
# item 3: non-finite samples, extreme amplitudes, extreme bins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(5, 8, 67), (40, 64, 323), (320, 512, 1000)])
def test_non_finite_samples_reach_exactly_their_filter_span(gpu, M, D, L):
    """a NaN, a +Inf and a -Inf in the stream, all taps non-zero: output m of every selected row is non-finite exactly when
    n_m - L < n_bad <= n_m for one of them. L is no multiple of M and the tap table is padded to whole rounds: every residue runs
    unsigned(L - r + M - 1) / M rounds of its own, so no product with the padding is formed; every other output is within TOL. The
    stream is fed in two calls with the NaN in the history of the second."""
    import torch
    import lora_sdr_amd as Lh
    pl = rx5.plan(M, D, L)
    assert pl["staged"] == (M != 320) and L % M and pl["Lp"] > L
    T = pl["T"]
    rng = np.random.default_rng(6 + L)
    n = 3 * T * D + 3 * L + 20 * D + 11
    cut = T * D + L + 5 * D + 2                                  # the stream is fed as [0, cut) and [cut, n)
    x = rx5._stream(rng, n)
    at_nan = cut - 3                                             # inside what becomes the second call's history
    m1 = 2 * T + L // D + 2
    at_pinf = (m1 + 1) * D - 1 - L - 3                           # L + 3 samples before an output
    at_ninf = (m1 + 1 + L // D + 9) * D - 1 - L                  # L before another: the first sample the definition excludes, the first of the padding
    assert at_nan + L < at_pinf and at_pinf + L < at_ninf and at_ninf + L < n
    x[at_nan] = np.float32("nan")
    x[at_pinf] = complex(np.float32("inf"), 1.0)
    x[at_ninf] = complex(0.5, -np.float32("inf"))
    bins = None if M <= 40 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:8]]).astype(np.int32)
    h = rx5._taps(rng, D, L)
    assert np.all(h != 0)
    n_m = (np.arange(n // D) + 1) * D - 1
    hit = np.zeros(n // D, bool)
    padded = np.zeros(n // D, bool)
    for b in (at_nan, at_pinf, at_ninf):
        hit |= (n_m - L < b) & (b <= n_m)
        padded |= (n_m - pl["Lp"] < b) & (b <= n_m)
    with np.errstate(invalid="ignore", over="ignore"):
        want = fd.channelize(x, M, D, h, bins)
    assert np.array_equal(~np.isfinite(want), np.broadcast_to(hit, want.shape))
    assert (padded & ~hit).any()                                 # a count by the padded length would reach outputs the definition excludes
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        whole = pf.run(xd).cpu().numpy()
        pf.reset()
        two = np.concatenate([pf.run(xd[:cut]).cpu().numpy(), pf.run(xd[cut:]).cpu().numpy()], axis=1)
        pf.close()
    scale = float(np.abs(h).sum() * np.abs(x[np.isfinite(x)]).max())
    for y in (whole, two):
        assert y.shape == want.shape
        bad = ~np.isfinite(y)
        err = float(np.abs(y[:, ~hit] - want[:, ~hit]).max())
        print("bank5 non-finite M %d D %d L %d: %d non-finite output times, %d by the definition, %d if the padding counted; elsewhere err / scale %.3g"
              % (M, D, L, bad.any(axis=0).sum(), hit.sum(), padded.sum(), err / scale))
        assert np.array_equal(bad, np.broadcast_to(hit, y.shape)), (np.nonzero(bad.any(axis=0) != hit)[0][:10].tolist(), int(hit.sum()))
        assert err <= TOL * scale, (err, scale)


def _length(M, D, L):
    """two tiles and a third of one plus a ragged tail, and long enough to fill the filter and cross a tile after that"""
    T = rx5.plan(M, D, L)["T"]
    return max((2 * T + T // 3 + 1) * D + 7, L + (T + T // 3) * D + 7)


def _some_bins(rng, M, rows):
    return np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:rows - 3]]).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(10, 16, 80), (160, 256, 1283)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_channeliser(gpu, M, D, L, amp):
    """inputs of the order of 1e-30 and of 1e30: the same tolerance relative to sum|h| max|x| at that scale"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(60 + M)
    n = _length(M, D, L)
    x = (rx5._stream(rng, n) * np.float32(amp)).astype(np.complex64)
    bins = None if M == 10 else _some_bins(rng, M, 11)
    h = rx5._taps(rng, D, L)
    want = fd.channelize(x, M, D, h, bins)
    scale = fd.scale(x, h)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    # on the host first, as tests/test_gpu_pfb_edges.py does: normal numbers in, the definition finite with head room for every
    # partial sum, and the tolerance itself far above the smallest normal number
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(parts).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < huge / 4 and TOL * scale > 1e2 * tiny
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        y = pf.run(torch.from_numpy(x).cuda()).cpu().numpy()
        pf.close()
    assert y.shape == want.shape and np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max())
    print("bank5 amplitude %g, channeliser M %d D %d L %d: err / scale %.3g" % (amp, M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", [(10, 16, 80), (160, 256, 1283)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_synthesis(gpu, M, U, L, amp):
    """inputs of the order of 1e-30 and of 1e30 (all 10 bins; 19 rows on 160): the same tolerance relative to error_scale at that
    amplitude"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(61 + M)
    T = tx5._tile(M)
    n = 2 * T + T // 3 + 1
    bins = None if M == 10 else _some_bins(rng, M, 19)
    K = M if bins is None else bins.size
    x = (tx5._rows(rng, K, n) * np.float32(amp)).astype(np.complex64)
    h = tx5._taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    want = yd.synthesize(x, M, U, h, bins, g)
    scale = sd.error_scale(x, h, U, g)
    tiny = float(np.finfo(np.float32).tiny)
    # on the host first, as tests/test_gpu_psb_edges.py does: normal numbers in, the definition and everything it is made of inside
    # fp32, the tolerance far above the smallest normal number
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(parts).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < 1e36 and TOL * scale > 1e2 * tiny
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(K * (L // U))
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        y = ps.run(torch.from_numpy(x).cuda()).cpu().numpy()
        ps.close()
    assert y.shape == want.shape and np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max()) / scale
    print("bank5 amplitude %g, synthesis M %d U %d L %d: err / scale %.3g" % (amp, M, U, L, err))
    assert err <= TOL, err


EXTREME_BINS = {5: [2, 2, 4, 0, 4, 0], 320: [192, 127, 319, 0, 319, 0]}        # INT32_MIN, INT32_MAX, -1, M, -M - 1, 0 modulo M


def _extreme_bins(M):
    bins = [INT32_MIN, INT32_MAX, -1, M, -M - 1, 0]
    folded = [v % M for v in bins]                              # Python integers: 0 .. M - 1
    assert folded == EXTREME_BINS[M]
    return bins, folded


@pytest.mark.gpu
@pytest.mark.parametrize("M,D,L", [(5, 8, 43), (320, 512, 1000)])
def test_extreme_bins_channeliser(gpu, M, D, L):
    """the rows of the object built on the residues, bit for bit, and the definition within TOL"""
    import torch
    import lora_sdr_amd as Lh
    bins, folded = _extreme_bins(M)
    rng = np.random.default_rng(70 + M)
    n = _length(M, D, L)
    x = rx5._stream(rng, n)
    h = rx5._taps(rng, D, L)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, bins)
        freqs = pf.freqs.copy()
        got = pf.run(xd).cpu().numpy()
        pf.close()
        pf = Lh.PolyphaseChannelizer.radix5(ctx, M, D, h, folded)
        same = pf.run(xd).cpu().numpy()
        pf.close()
    assert np.array_equal(freqs, np.array(bins, np.float64) / M) and freqs[0] == -(2.0 ** 31) / M and freqs[1] == (2.0 ** 31 - 1) / M
    assert got.shape == (len(bins), n // D) and np.array_equal(_bits(got), _bits(same))
    want = fd.channelize(x, M, D, h, bins)
    assert np.array_equal(want, fd.channelize(x, M, D, h, folded))
    scale = fd.scale(x, h)
    err = float(np.abs(got - want).max())
    print("bank5 extreme bins, channeliser M %d D %d L %d: err / scale %.3g" % (M, D, L, err / scale))
    assert err <= TOL * scale, (err, scale)
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(L)
    assert not np.array_equal(_bits(got[0]), _bits(got[2]))      # rows of different residues differ


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", [(5, 3, 20), (320, 7, 50)])
def test_extreme_bins_synthesis(gpu, M, U, L):
    """the stream of the object built on the residues, bit for bit, and the definition within TOL"""
    import torch
    import lora_sdr_amd as Lh
    bins, folded = _extreme_bins(M)
    rng = np.random.default_rng(71 + M)
    T = tx5._tile(M)
    n = 2 * T + T // 3 + 1
    x = tx5._rows(rng, len(bins), n)
    h = tx5._taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, len(bins)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, bins, g)
        freqs = ps.freqs.copy()
        got = ps.run(xd).cpu().numpy()
        ps.close()
        ps = Lh.PolyphaseSynthesizer.radix5(ctx, M, U, h, folded, g)
        same = ps.run(xd).cpu().numpy()
        ps.close()
    assert np.array_equal(freqs, np.array(bins, np.float64) / M) and freqs[0] == -(2.0 ** 31) / M and freqs[1] == (2.0 ** 31 - 1) / M
    assert got.shape == (n * U,) and np.array_equal(_bits(got), _bits(same))
    want = yd.synthesize(x, M, U, h, bins, g)
    scale = sd.error_scale(x, h, U, g)
    err = float(np.abs(got - want).max()) / scale
    print("bank5 extreme bins, synthesis M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
    assert err <= TOL, err
    assert float(np.abs(want).max()) / scale > 0.05 / np.sqrt(len(bins) * (-(-L // U)))
