"""GPU: the polyphase synthesis filter bank at the edges its definition covers (lora_sdr_amd/csrc/lorahip_psb.hip against
tests/synthesizer_def.py).

The bank's output is BY DEFINITION the direct-form synthesiser's for freq = bins / M, so every test here compares with

    y[n] = sum_k g_k exp(+2 pi i b_k n / M) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]

through synthesizer_def.synthesize_at(x, bins / M, U, h, gains, n=idx), within TOL = 4e-6 of synthesizer_def.error_scale (the
tolerance of tests/test_gpu_psb.py and of include/lorahip.h). Where every output of a full bank is wanted, psb_def.synthesize
(held to the definition by tests/test_psb_cpu.py, and here again at sampled outputs of the same case) stands in for it.

    what                                                      test
    plan() / check() restate lorahip_psb_create / _check;     test_shape_lists_sit_where_they_claim (no gpu marker)
    the lists below by that rule
    full banks K = M = 128 .. 1024, U = 5M/4 and odd,         test_full_banks_against_float64_definition, every shape also
    L = 8U + 3, with gains and without                        in two chunks, bit for bit
    accuracy relative to EACH row, gains 0 .. -60 dB,         test_yardstick_is_an_fp32_rounding_figure (no gpu marker),
    M = 8, 64, 1024 at U = 5, L = 40                          test_accuracy_relative_to_each_row
    history one short of, equal to and longer than a          test_history_against_segments, every shape in one call, in
    segment (M = 1024: 4096 input times); a last segment      ragged chunks and in chunks cut at seg - 1, seg, seg + 1, bit
    shorter than the history and a call that reaches back     for bit; the definition around every segment boundary and in
    through it; several segments at M = 512                   the last HC input times
    a row 2^31 + 5 samples (16 GiB) into the allocation       test_row_beyond_2_pow_31_samples
    one segment of exactly 2^30 outputs (2^22 fold blocks);   test_calls_of_2_pow_30_outputs
    2^30 outputs over 256 segments; a guard behind both
    n_sel = 65535 * 8 rows with random int32 bins             test_most_rows_the_check_accepts
    one step outside each limit, n_sel + 1 among them         test_shapes_outside_the_limits_are_refused
    bins INT32_MIN, INT32_MAX, -1, M, -M - 1, 0               test_extreme_bins_are_taken_modulo_n_bins
    1e-30 and 1e30                                            test_extreme_amplitudes_follow_the_definition
    gains 0.0, -0.0, negative, 1e-20; a row of gain 0.0       test_zero_negative_and_tiny_gains
    is, bit for bit, a row that is not there
    a row of gain 0.0 that carries an Inf: NaN over the       test_non_finite_sample_under_a_zero_gain_reaches_the_definitions_span
    definition's span, as 0 * Inf is in the definition

NOT here, on purpose: a "2^31 input times deep" test like the receive bank's. The stream position enters the kernels only as
(m0 + c) & (M - 1) with M a power of two, so any truncation of m0 leaves that value unchanged and such a test cannot fail; at
M = 1024 it would also push some 35 TB through the workspace.

Accuracy relative to each row (test_accuracy_relative_to_each_row): a K = M object, one unit tone in row k and exact zeros in
the others (by linearity, and exact zeros add nothing in fp32), gains from 0 to -60 dB over the rows; the figure of a row is
max|y - definition_k| / max|definition_k|, the worst row counts. "plain fp32" is the header's evaluation for that one row in
numpy float32 / complex64 (gain, textbook radix-2 inverse DFT with twiddles computed in double and rounded to float32, fold
in ascending i), measured on the host; "walk" is the host test's random-walk ceiling for it, 2^-24 * 4 sqrt(ceil(L/U) + log2 M);
the kernel's bound is 4 x plain fp32, as in tests/test_gpu_channelizer_edges.py and tests/test_gpu_synthesizer_edges.py.
All rows at M = 8 and 64; at M = 1024 a seeded 64 rows and the bins 0, 1, 511, 512, 513, 1023.

    shape (M, U, L)     plain fp32 vs float64   walk       bound (4 x)   kernel vs float64 (MI355X)
    (8, 5, 40)          2.96e-7                 7.91e-7    1.18e-6       2.19e-7
    (64, 5, 40)         3.13e-7                 8.92e-7    1.25e-6       3.23e-7
    (1024, 5, 40)       3.64e-7                 1.01e-6    1.46e-6       3.80e-7

err / scale of every other accuracy case is printed by the tests (`-s`). Measured on an MI355X, of error_scale (TOL is 4e-6):

    full banks, 8 shapes x 2           2.7e-9 .. 9.7e-9   (largest: M = 128, U = 77 with gains)
    history against segments           1.2e-8, 1.4e-8, 1.5e-8 (HC = 4095, 4096, 8191), 1.9e-8 (U = 1, two calls), 3.5e-8 (M = 512)
    a row 2^31 + 5 samples in          6.3e-8
    2^30 outputs                       5.0e-8 (one segment), 9.6e-8 (256 segments)
    65535 * 8 rows                     1.8e-10
    extreme bins                       3.8e-8 (M = 8), 3.8e-8 (M = 1024)
    1e-30 and 1e30                     2.6e-8 .. 4.1e-8 (16, 8, 64), 2.1e-8 .. 2.6e-8 (256, 320, 2048)
    gains with 0.0, -0.0, < 0, 1e-20   2.6e-8 (all 16 bins), 3.8e-8 (9 rows that share bins)

Non-finite under a gain of 0.0: three bad samples make 183 outputs non-finite at (16, 8, 61) and 192 at (16, 8, 64), the
definition's count, the silenced row's Inf included.
"""
import numpy as np
import pytest

import psb_def as pd
import synthesizer_def as sd
from test_gpu_psb import ODD_U, RAGGED, TOL, _bits, _err, _rows, _taps, _tile

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
N_SEL_MAX = 65535 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# host side: the constructor's rule, the shape lists, which outputs are compared
# ---------------------------------------------------------------------------------------------------------------------------
def plan(M, U, L):
    """what lorahip_psb_create derives from a shape: input times per workgroup T, input times per segment, taps per phase I, the
    history HC in input times, and the transform's LDS bytes"""
    M, U, L = int(M), int(U), int(L)
    I = -(-L // U)
    T = max(8, min(256, 4096 // M))
    return dict(T=T, seg=min((1 << 22) // M, (1 << 30) // U), I=I, HC=I - 1, lds=(T * (M + 1) + M // 2) * 8)


def check(M, U, L, n_sel):
    """lorahip_psb_check restated"""
    return (8 <= M <= 1024 and M & (M - 1) == 0) and 1 <= U <= 4096 and 1 <= L <= 65536 and 1 <= n_sel <= N_SEL_MAX


def segments(n, seg):
    """(first input time, input times) of every segment of one call of n input times"""
    return [(a, min(seg, n - a)) for a in range(0, n, seg)]


#        M, U: one U that is no multiple of M and the odd one of tests/test_gpu_psb.py; L = 8 U + 3
FULL = [(M, U, 8 * U + 3) for M in (128, 256, 512, 1024) for U in (5 * M // 4, ODD_U[M])]

#        M, U, L: U odd, so the outputs of a bin walk through every residue s = n mod M
PER_ROW = [(8, 5, 40), (64, 5, 40), (1024, 5, 40)]

#        M     U  L      n             a second call    (M = 1024: 4096 input times a segment; M = 512: 8192)
HIST = [(1024, 8, 32768, 3 * 4096 + 7, 0),             # HC = 4095: history one short of a segment
        (1024, 8, 32776, 3 * 4096 + 7, 0),             # HC = 4096: equal to a segment
        (1024, 8, 65536, 3 * 4096 + 7, 0),             # HC = 8191: longer than a segment (and the longest filter)
        (1024, 1, 300,   4096 + 5,     400),           # a last segment of 5 input times, HC = 299; the next call reaches back through it
        (512,  3, 20,    2 * 8192 + 11, 0)]            # several segments at a second M

#        M     U     n_in     K  L      bins
BIG = [(8,    4096, 1 << 18, 1, 8197,  [3]),           # ONE segment of exactly 2^30 outputs: the 32-bit output index, 2^22 fold blocks
       (1024, 1024, 1 << 20, 2, 2048,  [3, -5])]       # 2^30 outputs over 256 segments: out + done * U, in + done

DISTANT = dict(M=16, U=8, L=64, stride=(1 << 31) + 5)

REFUSED = [(4, 4, 8, 4), (2048, 4, 8, 4), (24, 4, 8, 4), (16, 0, 8, 4), (16, 4097, 8, 4), (16, 4, 0, 4), (16, 4, 65537, 4),
           (16, 4, 8, 0), (16, 4, 8, N_SEL_MAX + 1)]
MOST_ROWS = (1024, 3, 20, N_SEL_MAX)


def _flat_taps(rng, L):
    """taps of one order of magnitude from the first to the last, random signs: every tap of a long filter, and so every row of a long
    history, weighs about 1 / ceil(L/U) of error_scale -- a low-pass of this length would hide its far taps below TOL"""
    return (rng.uniform(0.5, 1.5, L) * rng.choice([-1.0, 1.0], L)).astype(np.float32)


def _all_phases(m, U):
    m = np.unique(np.asarray(m, np.int64))
    return (m[:, None] * U + np.arange(U, dtype=np.int64)[None, :]).reshape(-1)


def _hist_compared(rng, M, U, L, n, follow, K):
    """the outputs a HIST shape is compared at: every phase of the first input times, of those where the filter is first full, of
    the two either side of every segment boundary of both calls, of the last three, of seeded ones among the last HC, and of seeded
    others up to a budget"""
    pl = plan(M, U, L)
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


def _big_compared(rng, M, U, n_in):
    """the outputs a BIG call is compared at without copying 8 GiB: the first and the last, the outputs either side of every segment
    boundary (eight either side of every 16th, and seeded phases of the input time behind it, which is folded from the history),
    either side of every 64th tile boundary, around the byte offsets 2^31, 2^32 and 3 * 2^31 of the output, and seeded places"""
    pl = plan(M, U, 1)
    n_out = n_in * U
    idx = [np.arange(3000), np.arange(n_out - 3000, n_out), rng.integers(0, n_out, 4000)]
    for j, (a, _) in enumerate(segments(n_in, pl["seg"])[1:], 1):
        w = 8 if j % 16 == 0 else 1
        idx.append(np.arange(a * U - w, a * U + w))
        if j % 16 == 0:
            idx.append(a * U + rng.integers(0, U, 16))
    for b in range(64 * pl["T"], n_in, 64 * pl["T"]):
        idx.append(np.arange(b * U - 2, b * U + 2))
    for at in (1 << 28, 1 << 29, 3 << 28):
        idx.append(np.arange(at - 4, at + 4))
    return np.unique(np.concatenate(idx).astype(np.int64))


def test_shape_lists_sit_where_they_claim():
    """the lists above by the constructor's rule: HC below, equal to and above a segment; a last segment shorter than HC; a
    segment of exactly 2^30 outputs and a call of 2^30 outputs over many; every limit of lorahip_psb_check reached from inside;
    every refused shape outside exactly one limit"""
    assert [plan(M, 8, 64)["T"] for M in (8, 16, 32, 64, 128, 256, 512, 1024)] == [256, 256, 128, 64, 32, 16, 8, 8]
    assert [plan(M, 8, 64)["lds"] for M in (8, 16, 512, 1024)] == [18464, 34880, 34880, 69696]     # the table of DESIGN.md section 8d
    assert plan(8, 4096, 1)["seg"] == 1 << 18 and plan(8, 1, 1)["seg"] == 1 << 19 and plan(1024, 4096, 1)["seg"] == 4096
    # full banks: above the M of tests/test_gpu_psb.py's full banks, U no multiple of M
    assert {M for M, _, _ in FULL} == {128, 256, 512, 1024}
    assert all(U % M and L == 8 * U + 3 and check(M, U, L, M) for M, U, L in FULL)
    assert all(any(U % 2 for m, U, _ in FULL if m == M) and any(U > M for m, U, _ in FULL if m == M) for M in (128, 256, 512, 1024))
    # per row: odd U, all of them in every limit
    assert all(U % 2 and check(M, U, L, M) for M, U, L in PER_ROW)
    # history against segments
    p = [plan(M, U, L) for M, U, L, _, _ in HIST]
    assert all(check(M, U, L, 4) for M, U, L, _, _ in HIST)
    assert [q["seg"] for q in p] == [4096, 4096, 4096, 4096, 8192]
    assert [q["HC"] for q in p[:3]] == [p[0]["seg"] - 1, p[0]["seg"], 2 * p[0]["seg"] - 1]
    assert [len(segments(n, q["seg"])) for (_, _, _, n, _), q in zip(HIST, p)] == [4, 4, 4, 2, 3]
    assert all(segments(n, q["seg"])[-1][1] < q["seg"] for (_, _, _, n, _), q in zip(HIST, p))         # a ragged last segment
    M, U, L, n, follow = HIST[3]
    assert segments(n, p[3]["seg"])[-1][1] == 5 < p[3]["HC"] == 299 < follow                           # the next call reaches back through it
    assert HIST[2][2] == 65536 and HIST[3][1] == 1                                                     # L and U at their limits
    # the calls of 2^30 outputs
    (M0, U0, n0, K0, L0, _), (M1, U1, n1, K1, L1, _) = BIG
    assert n0 * U0 == n1 * U1 == 1 << 30
    assert segments(n0, plan(M0, U0, L0)["seg"]) == [(0, n0)] and n0 * U0 == 1 << 30                  # cnt * U == 2^30 in one segment
    assert len(segments(n1, plan(M1, U1, L1)["seg"])) == 256
    assert check(M0, U0, L0, K0) and check(M1, U1, L1, K1) and U0 == 4096 and M0 == 8 and M1 == 1024
    assert (n0 * U0 + 255) // 256 == 1 << 22
    # the distant row
    assert DISTANT["stride"] * 8 > 1 << 34 and (DISTANT["stride"] * 8) % (1 << 32) == 5 * 8             # a 32-bit byte offset lands on sample 5 of row 0
    # limits
    assert check(*MOST_ROWS) and not check(*MOST_ROWS[:3], MOST_ROWS[3] + 1)
    assert check(8, 1, 1, 1) and check(1024, 4096, 65536, N_SEL_MAX)
    assert not any(check(*s) for s in REFUSED)
    inside = (16, 4, 8, 4)
    assert check(*inside)
    for s in REFUSED:
        assert sum(a != b for a, b in zip(s, inside)) == 1
    # which outputs: both sides of every segment boundary, and the last HC input times
    rng = np.random.default_rng(0)
    for (M, U, L, n, follow), q in zip(HIST, p):
        idx = _hist_compared(rng, M, U, L, n, follow, 3)
        got = set((idx // U).tolist())
        for a, _ in segments(n, q["seg"])[1:]:
            assert {a - 1, a} <= got
        assert n + follow - 1 in got and len([t for t in got if t >= n + follow - q["HC"]]) >= min(8, q["HC"])
        assert idx.size * q["I"] * 3 <= 4e7


# ---------------------------------------------------------------------------------------------------------------------------
# item 1: full banks above M = 64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", FULL, ids=["M%d-U%d-L%d" % s for s in FULL])
def test_full_banks_against_float64_definition(gpu, M, U, L):
    """K = M: every input of the transform and every bin list is in use. All outputs against psb_def.synthesize, which is held to
    the definition at the outputs either side of every tile boundary, the first, the last and seeded ones of this very case"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(M * 10000 + U)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    x = _rows(rng, M, n)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, M).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    idx = np.unique(np.concatenate([[0, 1, n * U - 2, n * U - 1], [T * U - 1, T * U, 2 * T * U - 1, 2 * T * U], rng.integers(0, n * U, 56)]))
    cut = n // 3
    with Lh.Context(7) as ctx:
        for gains in (g, None):
            ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, None, gains)
            got = ps.run(xd).cpu().numpy()
            ps.reset()
            two = np.concatenate([ps.run(xd[:, :cut]).cpu().numpy(), ps.run(xd[:, cut:]).cpu().numpy()])
            freqs = ps.freqs.copy()
            assert ps.n_channels == M
            ps.close()
            assert got.shape == (n * U,) and np.array_equal(freqs, np.arange(M) / M)
            assert np.array_equal(_bits(two), _bits(got))
            scale = sd.error_scale(x, h, U, gains)
            every = pd.synthesize(x, M, U, h, None, gains)
            want = sd.synthesize_at(x, freqs, U, h, gains, n=idx)
            assert float(np.abs(every[idx] - want).max()) <= 1e-12 * scale
            err = float(np.abs(got - every).max()) / scale
            err_def = float(np.abs(got[idx] - want).max()) / scale
            print("PSB full bank M %d U %d L %d %s: err / scale %.3g (all outputs), %.3g (the definition at %d outputs)"
                  % (M, U, L, "gains" if gains is not None else "no gains", err, err_def, idx.size))
            assert err <= TOL and err_def <= TOL, (err, err_def)
            assert float(np.abs(every).max()) / scale > 0.05 / np.sqrt(M * (-(-L // U)))


# ---------------------------------------------------------------------------------------------------------------------------
# item 2: accuracy relative to each row
# ---------------------------------------------------------------------------------------------------------------------------
def _idft_radix2_c64(X):
    """textbook radix-2 decimation-in-frequency transform with exp(+2 pi i k / M), complex64 throughout, twiddles computed in double
    and rounded to float32; rows of X, natural order in and out"""
    n, M = X.shape
    tw = np.exp(2j * np.pi * np.arange(M // 2) / M).astype(np.complex64)
    v = X.astype(np.complex64)
    hs = M // 2
    while hs >= 1:
        v = v.reshape(n, -1, 2, hs)
        a, b = v[:, :, 0, :], v[:, :, 1, :]
        v = np.stack([a + b, (a - b) * tw[np.arange(hs) * (M // (2 * hs))]], axis=2)
        hs //= 2
    v = v.reshape(n, M)                                          # bit-reversed
    logm = M.bit_length() - 1
    rev = np.array([int(format(s, "0%db" % logm)[::-1], 2) for s in range(M)])
    return v[:, rev]


_ROW_CASES = {}


def _row_case(M, U, L):
    """the inputs of one PER_ROW shape, the float64 definition of every row that is run and the plain-fp32 figure of each: computed
    once and shared by the host test and the GPU test"""
    if (M, U, L) in _ROW_CASES:
        return _ROW_CASES[(M, U, L)]
    import lora_sdr_amd as Lh
    pl = plan(M, U, L)
    rng = np.random.default_rng(M * 1000 + U)
    n = max(2 * pl["T"] + pl["T"] // 3 + 1, -(-M // U) + 2 * pl["I"] + 3)       # more than two tiles, and every residue s with a full filter
    gains = (10.0 ** (-60.0 * np.arange(M) / (M - 1) / 20.0)).astype(np.float32)
    h = (Lh.design_lowpass(U, L) * U).astype(np.float32)
    tone = rng.uniform(-0.3, 0.3, M)                            # cycles per INPUT sample: inside the pass band of U h
    x = np.exp(2j * np.pi * tone[:, None] * np.arange(n)[None, :]).astype(np.complex64)
    rows = np.arange(M) if M <= 64 else np.unique(np.concatenate([rng.choice(M, 64, replace=False), [0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1]]))
    nn = np.arange(n * U, dtype=np.int64)
    p, m, s = nn % U, nn // U, nn % M
    want, plain = {}, {}
    for k in rows:
        k = int(k)
        w = sd.synthesize_at(x[k:k + 1], [k / M], U, h, gains[k:k + 1], n=nn)
        # the header's evaluation of this one row in float32: gain, transform, fold in ascending i
        X = np.zeros((n, M), np.complex64)
        X[:, k] = (gains[k] * x[k].real) + 1j * (gains[k] * x[k].imag)
        u = _idft_radix2_c64(X)
        acc = np.zeros(n * U, np.complex64)
        for i in range(pl["I"]):
            ok = (p + i * U < L) & (m - i >= 0)
            acc[ok] = acc[ok] + h[(p + i * U)[ok]] * u[(m - i)[ok], s[ok]]
        assert acc.dtype == np.complex64 and u.dtype == np.complex64
        want[k] = w
        plain[k] = float(np.abs(acc - w).max() / np.abs(w).max())
    c = dict(M=M, U=U, L=L, n=n, x=x, h=h, gains=gains, rows=[int(k) for k in rows], want=want, plain=plain, I=pl["I"])
    _ROW_CASES[(M, U, L)] = c
    return c


def _walk(M, I):
    """ceiling for the plain-fp32 figure: ceil(L/U) + log2 M steps in a row (one butterfly or one fold term each: a product and a sum
    that round to half an ulp, 2^-24, per component), adding up as a random walk; 4 for the two components of a complex number and
    for the worst of some thousand outputs against the root mean square"""
    return 2.0 ** -24 * 4.0 * np.sqrt(I + np.log2(M))


def test_yardstick_is_an_fp32_rounding_figure():
    """the transform of the yardstick is the inverse DFT (against numpy's), every row carries its tone, and the plain-fp32 error of
    the worst row is an fp32 rounding figure: above a quarter ulp, below the random walk of its roundings"""
    rng = np.random.default_rng(2)
    for M in (8, 64, 1024):
        X = (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))).astype(np.complex64)
        assert np.abs(_idft_radix2_c64(X) - np.fft.ifft(X.astype(np.complex128), axis=1) * M).max() <= 1e-6 * M
    for M, U, L in PER_ROW:
        c = _row_case(M, U, L)
        assert c["n"] * U >= M + 2 * L and {0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1} <= set(c["rows"])
        assert len(c["rows"]) == M if M <= 64 else 64 <= len(c["rows"]) <= 70
        for k in c["rows"]:
            assert np.abs(c["want"][k]).max() > 0.5 * c["gains"][k]          # the row carries its tone
        worst = max(c["plain"].values())
        print("PSB per-row case M %d U %d L %d: plain fp32 vs float64, worst of %d rows %.3e (walk %.3e)" % (M, U, L, len(c["rows"]), worst, _walk(M, c["I"])))
        assert 2.0 ** -26 < worst < _walk(M, c["I"])


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", PER_ROW)
def test_accuracy_relative_to_each_row(gpu, M, U, L):
    """see the table in the module docstring: kernel vs float64 within 4 x (plain fp32 vs float64), per row relative to that row's
    largest output, every row alone in a K = M object with gains from 0 to -60 dB"""
    import torch
    import lora_sdr_amd as Lh
    c = _row_case(M, U, L)
    n = c["n"]
    kern = {}
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, c["h"], None, c["gains"])
        rows = torch.zeros((M, n), dtype=torch.complex64, device="cuda")
        for k in c["rows"]:
            rows[k] = torch.from_numpy(c["x"][k]).cuda()
            ps.reset()
            y = ps.run(rows).cpu().numpy()
            rows[k] = 0
            kern[k] = float(np.abs(y - c["want"][k]).max() / np.abs(c["want"][k]).max())
        ps.close()
    plain = max(c["plain"].values())
    worst = max(kern, key=kern.get)
    print("PSB per-row accuracy M %d U %d L %d (%d rows): plain fp32 %.3e, walk %.3e, bound %.3e, kernel %.3e (worst row %d)"
          % (M, U, L, len(kern), plain, _walk(M, c["I"]), 4.0 * plain, kern[worst], worst))
    if M > 64:
        print("  rows run: " + " ".join(str(k) for k in c["rows"]))
    assert kern[worst] <= 4.0 * plain, (worst, kern[worst], plain)


# ---------------------------------------------------------------------------------------------------------------------------
# item 3: the history against the segments of a call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L,n,follow", HIST, ids=["M%d-U%d-L%d-n%d" % s[:4] for s in HIST])
def test_history_against_segments(gpu, M, U, L, n, follow):
    """one call (and, for the shape with a second call, that call behind it); ragged chunks and chunks cut at seg - 1, seg and
    seg + 1, bit for bit against it; the sampled float64 definition"""
    import torch
    import lora_sdr_amd as Lh
    pl = plan(M, U, L)
    seg, total = pl["seg"], n + follow
    rng = np.random.default_rng(M + U + L)
    bins = np.array([1 - M, M // 2 + 1, 3 * M + 7], np.int32)
    K = bins.size
    x = _rows(rng, K, total)
    h = _flat_taps(rng, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    ragged, pos = [], 0
    while pos < total:
        ragged.append(min(RAGGED[len(ragged) % len(RAGGED)], total - pos))
        pos += ragged[-1]
    cuts = [seg - 1, 1, 1, seg, seg + 1, total]                  # ends at seg - 1, seg, seg + 1; calls of seg and of seg + 1 input times
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        whole = torch.cat([ps.run(xd[:, :n])] + ([ps.run(xd[:, n:])] if follow else [])).cpu().numpy()
        for sizes in [ragged, cuts] + ([[total]] if follow else []):
            ps.reset()
            parts, pos = [], 0
            for s in sizes:
                s = min(s, total - pos)
                parts.append(ps.run(xd[:, pos:pos + s]))
                pos += s
            assert pos == total
            assert np.array_equal(_bits(torch.cat(parts).cpu().numpy()), _bits(whole)), sizes[:6]
        ps.close()
    assert whole.shape == (total * U,)
    idx = _hist_compared(rng, M, U, L, n, follow, K)
    err, level = _err(whole, x, bins / M, U, h, g, idx)
    print("PSB history M %d U %d L %d (HC %d, segment %d) n %d%s: err / scale %.3g, %d outputs compared"
          % (M, U, L, pl["HC"], seg, n, " + %d" % follow if follow else "", err, idx.size))
    assert err <= TOL, err
    assert level > 0.05 / np.sqrt(K * pl["I"])


# ---------------------------------------------------------------------------------------------------------------------------
# item 4: 64-bit addressing
# ---------------------------------------------------------------------------------------------------------------------------
def _free_or_skip(torch, need):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (need / 1e9, free / 1e9))


@pytest.mark.gpu
def test_row_beyond_2_pow_31_samples(gpu):
    """two rows with in_stride = 2^31 + 5 samples in ONE uninitialised allocation: row 1 starts 16 GiB in. Only the two windows that
    are read are filled; row 0's window goes on behind the row with other data, so that a row offset formed in 32 bits (of bytes:
    sample 5 of row 0) reads something else. Against the definition, and bit for bit against the same rows packed tightly. Skipped
    only when less than that is free."""
    import torch
    import lora_sdr_amd as Lh
    M, U, L, stride = DISTANT["M"], DISTANT["U"], DISTANT["L"], DISTANT["stride"]
    n = 2 * _tile(M) + 37
    _free_or_skip(torch, 8 * (stride + n) + (1 << 30))
    rng = np.random.default_rng(64)
    x = _rows(rng, 2, n)
    behind = _rows(rng, 1, 64)[0]
    bins = np.array([3, -5], np.int32)
    h = _taps(rng, U, L)
    g = np.array([0.75, 1.5], np.float32)
    big = torch.empty(stride + n, dtype=torch.complex64, device="cuda")
    big[:n] = torch.from_numpy(x[0]).cuda()
    big[n:n + 64] = torch.from_numpy(behind).cuda()
    big[stride:stride + n] = torch.from_numpy(x[1]).cuda()
    rows = big.as_strided((2, n), (stride, 1))
    assert rows[1].data_ptr() - big.data_ptr() == 8 * ((1 << 31) + 5)
    assert not np.array_equal(np.concatenate([x[0], behind])[5:5 + n], x[1])
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        tight = ps.run(torch.from_numpy(x).cuda()).cpu().numpy()
        ps.reset()
        cut = 100
        loose = np.concatenate([ps.run(rows[:, :cut]).cpu().numpy(), ps.run(rows[:, cut:]).cpu().numpy()])
        ps.close()
    del big, rows
    assert np.array_equal(_bits(loose), _bits(tight))
    err, level = _err(loose, x, bins / M, U, h, g)
    print("PSB distant row: err / scale %.3g" % err)
    assert err <= TOL and level > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,n_in,K,L,bins", BIG, ids=["one-segment", "256-segments"])
def test_calls_of_2_pow_30_outputs(gpu, M, U, n_in, K, L, bins):
    """the largest call, 2^30 outputs (8 GiB), as one segment and as 256: slices of the output against the definition (nothing but
    they are copied to the host), and a guard behind the output that stays as it was. Skipped only when less than that is free."""
    import torch
    import lora_sdr_amd as Lh
    n_out, G = n_in * U, 64
    assert n_out == 1 << 30
    _free_or_skip(torch, 8 * (n_out + G) + 8 * K * n_in + (1 << 30))
    rng = np.random.default_rng(M + K)
    x = _rows(rng, K, n_in)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    bins = np.array(bins, np.int32)
    idx = _big_compared(rng, M, U, n_in)
    assert idx[0] == 0 and idx[-1] == n_out - 1
    guard = complex(3.0, -7.0)
    out = torch.empty(n_out + G, dtype=torch.complex64, device="cuda")
    out[n_out:] = guard
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        assert ps.out_count(n_in) == n_out
        y = ps.run(torch.from_numpy(x).cuda(), out=out)
        assert y.data_ptr() == out.data_ptr() and y.shape == (n_out,)
        got = y[torch.from_numpy(idx).cuda()].cpu().numpy()
        behind = out[n_out:].cpu().numpy()
        ps.close()
    del out, y
    assert np.all(behind == np.complex64(guard))
    want = sd.synthesize_at(x, bins / M, U, h, g, n=idx)
    scale = sd.error_scale(x, h, U, g)
    err = float(np.abs(got - want).max()) / scale
    print("PSB 2^30 outputs M %d U %d n_in %d (%d segments): err / scale %.3g, %d outputs compared"
          % (M, U, n_in, len(segments(n_in, plan(M, U, L)["seg"])), err, idx.size))
    assert err <= TOL, err
    assert float(np.abs(want).max()) / scale > 0.05 / np.sqrt(K * (-(-L // U)))


# ---------------------------------------------------------------------------------------------------------------------------
# item 5: the limits from inside
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_most_rows_the_check_accepts(gpu):
    """n_sel = 65535 * 8 rows with random int32 bins (the two extremes among them) on 1024 bins: every bin sums some 512 rows.
    Rows that share a bin modulo M share their frequency exactly, so the definition of the whole is the definition of the 1024
    float64 bin sums on the bins 0 .. M - 1"""
    import torch
    import lora_sdr_amd as Lh
    M, U, L, K = MOST_ROWS
    n = 20
    rng = np.random.default_rng(8)
    bins = rng.integers(INT32_MIN, INT32_MAX + 1, K).astype(np.int32)
    bins[:2] = INT32_MIN, INT32_MAX
    b = bins.astype(np.int64) % M
    assert np.bincount(b, minlength=M).min() > 400
    x = _rows(rng, K, n)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    X = np.zeros((M, n), np.complex128)
    np.add.at(X, b, g.astype(np.float64)[:, None] * x)
    want = sd.synthesize_at(X, np.arange(M) / M, U, h, None, n=np.arange(n * U))
    scale = sd.error_scale(x, h, U, g)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        assert ps.n_channels == K and np.array_equal(ps.freqs, bins / M)
        got = ps.run(xd).cpu().numpy()
        ps.reset()
        two = np.concatenate([ps.run(xd[:, :7]).cpu().numpy(), ps.run(xd[:, 7:]).cpu().numpy()])
        ps.close()
    assert np.array_equal(_bits(two), _bits(got))
    err = float(np.abs(got - want).max()) / scale
    print("PSB n_sel %d: err / scale %.3g" % (K, err))
    assert err <= TOL, err
    assert float(np.abs(want).max()) / scale > 0.05 / np.sqrt(K * (-(-L // U)))


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L,n_sel", REFUSED)
def test_shapes_outside_the_limits_are_refused(gpu, M, U, L, n_sel):
    import lora_sdr_amd as Lh
    lib = Lh.load()
    assert lib.lorahip_psb_check(M, U, L, n_sel) == -1
    assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
    with Lh.Context(7) as ctx:
        with pytest.raises(Lh.LoraHipError):
            Lh.PolyphaseSynthesizer(ctx, M, U, np.ones(L, np.float32), np.zeros(n_sel, np.int32))
        assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")


@pytest.mark.gpu
@pytest.mark.parametrize("M", [8, 1024])
def test_extreme_bins_are_taken_modulo_n_bins(gpu, M):
    import torch
    import lora_sdr_amd as Lh
    U, L = 5, 40
    bins = [INT32_MIN, INT32_MAX, -1, M, -M - 1, 0]
    rng = np.random.default_rng(M)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    x = _rows(rng, len(bins), n)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, len(bins)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        freqs = ps.freqs.copy()
        got = ps.run(xd).cpu().numpy()
        ps.close()
        folded = [v % M for v in bins]                          # Python integers: 0 .. M - 1
        assert folded == [0, M - 1, M - 1, 0, M - 1, 0]
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, folded, g)
        same = ps.run(xd).cpu().numpy()
        ps.close()
    assert np.array_equal(freqs, np.array(bins, np.float64) / M) and freqs[0] == -(2.0 ** 31) / M and freqs[1] == (2.0 ** 31 - 1) / M
    assert np.array_equal(_bits(got), _bits(same))
    err, level = _err(got, x, freqs, U, h, g)
    print("PSB extreme bins M %d: err / scale %.3g" % (M, err))
    assert err <= TOL and level > 0.05 / np.sqrt(len(bins) * (L // U))


# ---------------------------------------------------------------------------------------------------------------------------
# item 6: values
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", [(16, 8, 64), (256, 320, 2048)])
@pytest.mark.parametrize("amp", [1e-30, 1e30])
def test_extreme_amplitudes_follow_the_definition(gpu, M, U, L, amp):
    """inputs of the order of 1e-30 and of 1e30 (all 16 bins; 19 rows on 256): the same tolerance relative to error_scale at that
    amplitude"""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(60 + M)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    bins = None if M == 16 else np.concatenate([[0, M // 2, M - 1], rng.permutation(M)[:16]]).astype(np.int32)
    K = M if bins is None else bins.size
    x = (_rows(rng, K, n) * np.float32(amp)).astype(np.complex64)
    h = _taps(rng, U, L)
    g = rng.uniform(0.25, 2.0, K).astype(np.float32)
    freqs = (np.arange(M) if bins is None else bins) / M
    want = sd.synthesize_at(x, freqs, U, h, g, n=np.arange(n * U))
    scale = sd.error_scale(x, h, U, g)
    tiny = float(np.finfo(np.float32).tiny)
    # on the host first: normal numbers in, the definition and everything it is made of inside fp32, the tolerance far above the
    # smallest normal number
    parts = np.abs(x.view(np.float32))
    assert np.isfinite(parts).all() and parts[parts > 0].min() >= tiny
    assert np.isfinite(want).all() and scale < 1e36 and TOL * scale > 1e2 * tiny
    assert float(np.abs(want).max()) > 0.05 * scale / np.sqrt(K * (L // U))
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        y = ps.run(torch.from_numpy(x).cuda()).cpu().numpy()
        ps.close()
    assert np.isfinite(y.view(np.float32)).all()
    err = float(np.abs(y.astype(np.complex128) - want).max()) / scale
    print("PSB amplitude %g M %d U %d L %d: err / scale %.3g" % (amp, M, U, L, err))
    assert err <= TOL, err


@pytest.mark.gpu
def test_zero_negative_and_tiny_gains(gpu):
    """gains 0.0, -0.0, negative, 1e-20 and -1e-20 among ordinary ones, on a full bank and on rows that share bins: within TOL of
    the definition; and a row of gain 0.0 (or -0.0), first, in the middle or last in its bin's list or alone in its bin, gives bit
    for bit the stream of the object built without that row"""
    import torch
    import lora_sdr_amd as Lh
    M, U, L = 16, 8, 61
    rng = np.random.default_rng(17)
    T = _tile(M)
    n = 2 * T + T // 3 + 1
    h = _taps(rng, U, L)
    special = np.array([0.0, -0.0, -1.5, 1e-20, -1e-20, -0.25], np.float32)
    with Lh.Context(7) as ctx:
        for bins in (None, np.array([3, 9, 3 - M, 3, 12, -4, 3 + 5 * M, 9, 0], np.int32)):
            K = M if bins is None else bins.size
            x = _rows(rng, K, n)
            xd = torch.from_numpy(x).cuda()
            g = rng.uniform(0.25, 2.0, K).astype(np.float32) * rng.choice([-1.0, 1.0], K).astype(np.float32)
            g[rng.permutation(K)[:special.size]] = special
            ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
            got = ps.run(xd).cpu().numpy()
            ps.close()
            b = np.arange(M) if bins is None else bins
            err, level = _err(got, x, b / M, U, h, g)
            print("PSB gains with zeros, signs and 1e-20, K %d: err / scale %.3g" % (K, err))
            assert err <= TOL and level > 0.05 / np.sqrt(K * 8)
            # one row at a time silenced: the same bits as without it
            for k, zero in [(0, 0.0), (2, 0.0), (3, -0.0), (K - 3, 0.0), (K - 1, -0.0)]:
                gz = rng.uniform(0.25, 2.0, K).astype(np.float32)
                gz[k] = zero
                keep = np.arange(K) != k
                ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, b, gz)
                with_row = ps.run(xd).cpu().numpy()
                ps.close()
                ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, b[keep], gz[keep])
                without = ps.run(xd[torch.from_numpy(keep).cuda()].contiguous()).cpu().numpy()
                ps.close()
                assert np.isfinite(with_row.view(np.float32)).all() and float(np.abs(with_row).max()) > 0.0
                assert np.array_equal(_bits(with_row), _bits(without)), (K, k, zero)


@pytest.mark.gpu
@pytest.mark.parametrize("M,U,L", [(16, 8, 61), (16, 8, 64)])
def test_non_finite_sample_under_a_zero_gain_reaches_the_definitions_span(gpu, M, U, L):
    """three rows, the middle one with gain 0.0: a +Inf in it, a NaN in the first row and a -Inf in the third. 0 * Inf is NaN in the
    definition and in a fused multiply-add alike: the non-finite outputs are exactly those synthesize_at makes non-finite -- L a
    sample, the silenced row's included --, and every other output is, bit for bit, the stream with those input times zeroed. In
    one call, and with the silenced Inf in the history of a later call."""
    import torch
    import lora_sdr_amd as Lh
    rng = np.random.default_rng(16 + L)
    bins = np.array([0, 4, 7], np.int32)
    g = np.array([1.25, 0.0, 0.5], np.float32)
    T = _tile(M)
    n = 3 * T + 11
    cut = T + 45
    x = _rows(rng, 3, n)
    clean = x.copy()
    at_pinf, at_nan, at_ninf = cut - 3, 2 * T - 1, 2 * T + 29      # in the second call's history; the last time of a tile; elsewhere
    x[1, at_pinf] = complex(np.float32("inf"), 1.0)
    x[0, at_nan] = np.float32("nan")
    x[2, at_ninf] = complex(0.5, -np.float32("inf"))
    for m in (at_pinf, at_nan, at_ninf):
        clean[:, m] = 0
    h = (Lh.design_lowpass(U, L) * U * rng.uniform(0.5, 1.5, L)).astype(np.float32)
    assert np.all(h != 0)
    nn = np.arange(n * U, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        want = sd.synthesize_at(x, bins / M, U, h, g, n=nn)
    hit = ~np.isfinite(want)                                     # from the definition, not from the kernel
    span = np.zeros(n * U, bool)
    for m in (at_pinf, at_nan, at_ninf):
        span |= (nn >= m * U) & (nn < m * U + L)
    assert np.array_equal(hit, span) and hit.sum() == 3 * L      # what the header says of it: L outputs a sample, gain 0 or not
    assert np.all(~np.isfinite(want[at_pinf * U:at_pinf * U + L]))
    xd = torch.from_numpy(x).cuda()
    with Lh.Context(7) as ctx:
        ps = Lh.PolyphaseSynthesizer(ctx, M, U, h, bins, g)
        whole = ps.run(xd).cpu().numpy()
        ps.reset()
        two = np.concatenate([ps.run(xd[:, :cut]).cpu().numpy(), ps.run(xd[:, cut:]).cpu().numpy()])
        ps.reset()
        base = ps.run(torch.from_numpy(clean).cuda()).cpu().numpy()
        ps.close()
    assert np.isfinite(base.view(np.float32)).all()
    for y in (whole, two):
        bad = ~np.isfinite(y)
        print("PSB non-finite under gain 0, U=%d L=%d: %d non-finite outputs, %d by the definition" % (U, L, bad.sum(), hit.sum()))
        assert np.array_equal(bad, hit), (np.nonzero(bad != hit)[0][:10].tolist(), int(bad.sum()), int(hit.sum()))
        assert np.array_equal(_bits(y[~hit]), _bits(base[~hit]))
    err, _ = _err(base, clean, bins / M, U, h, g)
    assert err <= TOL
