"""The soft-decision definitions (tests/soft_def.py) against the hard ones they extend: no GPU, no library."""
import numpy as np
import pytest

import codec_def as D
import codec_hdr_def as H
import soft_def as S


@pytest.mark.parametrize("sf,ppm", [(7, 7), (7, 5), (8, 8), (10, 8), (12, 12), (12, 10)])
def test_llr_sign_is_the_gray_code_of_the_argmax(sf, ppm):
    rng = np.random.default_rng(100 * sf + ppm)
    N = 1 << sf
    bins = (rng.standard_normal((64, N)) + 1j * rng.standard_normal((64, N))).astype(np.complex64)
    llr = S.llr_def(bins, sf, ppm)
    assert llr.shape == (64, ppm) and llr.dtype == np.float32
    assert np.all(llr != 0), "a tie between the two classes' maxima: choose another seed"
    k = S.power_def(bins).argmax(axis=1)
    g = S.gray_map(sf, ppm)[k]
    want = (g[:, None] >> np.arange(ppm, dtype=np.uint32)) & 1
    assert np.array_equal((llr > 0).astype(np.uint32), want)
    # the mapping is the decoder's: the Gray-coded, rounded symbol value of bin k
    assert np.array_equal(S.gray_map(sf, ppm), H.gray_rounded(np.arange(N, dtype=np.uint16), sf, ppm) & ((1 << ppm) - 1))


def test_llr_is_the_difference_of_the_class_maxima():
    sf, ppm = 7, 5
    bins = np.zeros((1, 128), np.complex64)
    bins[0, 9] = 3 + 4j         # P = 25; (9 + 2) >> 2 = 2 -> gray 3: bits 0, 1
    bins[0, 40] = 2 + 0j        # P = 4;  (40 + 2) >> 2 = 10 -> gray 15: bits 0..3
    bins[0, 127] = 1 + 1j       # P = 2;  (127 + 2) >> 2 = 32 -> gray 48, masked to 5 bits: bit 4
    assert np.array_equal(S.llr_def(bins, sf, ppm)[0], np.array([25 - 2, 25 - 2, 4 - 25, 4 - 25, 2 - 25], np.float32))


CASES = [(sf, ppm, rdd, explicit, crc) for (sf, ppm) in ((7, 0), (7, 5), (9, 0), (9, 7)) for rdd in range(5) for explicit in (1, 0) for crc in (1, 0)]


@pytest.mark.parametrize("sf,ppm,rdd,explicit,crc", CASES)
def test_unit_llrs_of_clean_symbols_decode_like_the_hard_walk(sf, ppm, rdd, explicit, crc):
    rng = np.random.default_rng(sf * 1000 + ppm * 100 + rdd * 10 + explicit * 2 + crc)
    P = ppm or sf
    for length in (1, 6, 13):
        payload = rng.integers(0, 256, length, dtype=np.uint8)
        syms, _ = D.build(sf, payload, ppm, rdd, bool(explicit), bool(crc))
        for hdr in (1, 0):
            cfg = (sf, ppm, rdd, crc, 1, 1, explicit, hdr, length)
            want = H.walk(syms, cfg)
            got = S.decode_soft_def(S.llr_of_symbols(syms, sf, P), cfg)
            assert (got[0] is None) == (want[0] is None) and (want[0] is None or np.array_equal(got[0], want[0]))
            assert got[1] == want[1] == 0 and got[2] == want[2]
    if explicit:                                     # the rate from the header
        cfg = (sf, ppm, H.RDD_FROM_HEADER, crc, 1, 1, 1, 0, 0)
        got = S.decode_soft_def(S.llr_of_symbols(syms, sf, P), cfg)
        want = H.walk(syms, cfg)
        assert (got[0] is None) == (want[0] is None) and (want[0] is None or np.array_equal(got[0], want[0])) and got[2] == want[2]
        assert not crc or np.array_equal(got[0], payload)


def test_short_rows_and_counts_as_the_hard_walk():
    sf, ppm, rdd = 8, 0, 2
    payload = np.arange(9, dtype=np.uint8)
    syms, _ = D.build(sf, payload, ppm, rdd, True, True)
    cfg = (sf, ppm, rdd, 1, 1, 0, 1, 0, 0)
    llr = S.llr_of_symbols(syms, sf, sf)
    for n in (0, 7, 8, 9, syms.size - 1, syms.size, syms.size + 3):
        want = H.walk(syms[:min(n, syms.size)], cfg, n)
        got = S.decode_soft_def(llr[:min(n, syms.size)], cfg, n)
        assert (got[0] is None) == (want[0] is None) and got[1] == want[1] and got[2] == want[2]
        if want[0] is not None:
            assert np.array_equal(got[0], want[0])


def _metric(L, x, rate, dtype):
    code = int(D.fec_def(x, rate))
    m = dtype(0)
    for k in range(4 + rate):
        m = dtype(m + dtype(L[k] if (code >> k) & 1 else -L[k]))
    return m


def test_one_codeword_pins_the_tie_and_order_rules():
    # 4/8, x = 5 sent. Bit 0 arrives hard-wrong at |L| = 8; the other three data bits are right at |L| = 1, the parity bits right at
    # |L| = 4. Hard decision: one error, corrected back to 5. Soft: M(5) = -8 + 3 + 16 = 11, but the three codewords at distance 4 from
    # 5's that differ from it in bit 0, two weak data bits and one parity bit score 8 + 2 - 1 + 8 - 4 + ... = 15 each: x = 2, 8 and 14
    # tie for the maximum and the smallest wins.
    code5 = int(D.fec_def(5, 4))
    L = np.array([(1.0 if (code5 >> k) & 1 else -1.0) * (1.0 if k < 4 else 4.0) for k in range(8)], np.float32)
    L[0] *= -8.0
    M = [float(_metric(L, x, 4, np.float32)) for x in range(16)]
    assert M == [9, -15, 15, -9, 3, 11, 9, -15, 15, -9, -11, -3, 9, -15, 15, -9]
    assert S.soft_nibble(L, 4) == 2
    assert H.hamming84_def(sum(1 << k for k in range(8) if L[k] > 0)) == (5, True)       # where hard and soft part ways
    # ties: all-zero LLRs score 0 for every x -- the smallest wins
    assert S.soft_nibble(np.zeros(8, np.float32), 4) == 0
    assert S.soft_nibble(np.array([0, 1, 0, 0, 0, 0, 0, 0], np.float32), 0) == 2         # 4/4 reads bits 0..3: every x with bit 1 scores alike
    # order: float32, k ascending from 0. With L = (2^24, 1, -2^24, 1) at 4/4 the exact maximum is x = 11 (2^25 + 2); in float32 the
    # ones are lost against 2^24 and x = 1, 3, 9 and 11 all come to 2^25: the definition answers 1
    L4 = np.array([2.0 ** 24, 1.0, -(2.0 ** 24), 1.0, 0, 0, 0, 0], np.float32)
    exact = [float(_metric(L4.astype(np.float64), x, 0, np.float64)) for x in range(16)]
    assert exact.index(max(exact)) == 11 and exact.count(max(exact)) == 1
    f32 = [float(_metric(L4, x, 0, np.float32)) for x in range(16)]
    assert [x for x in range(16) if f32[x] == max(f32)] == [1, 3, 9, 11]
    assert S.soft_nibble(L4, 0) == 1


# ---- bins and LLRs that are not finite: the rule of include/lorahip.h, restated by class_max and by soft_nibble's loop ------------------
def _serial_llr(P, sf, ppm):
    """the rule written out as the scan it is: both maxima from 0, a bin enters only by P[k] > max"""
    g = S.gray_map(sf, ppm)
    out = np.zeros(ppm, np.float32)
    for m in range(ppm):
        hi = lo = np.float32(0)
        for k in range(1 << sf):
            if (int(g[k]) >> m) & 1:
                hi = P[k] if P[k] > hi else hi
            else:
                lo = P[k] if P[k] > lo else lo
        with np.errstate(invalid="ignore"):
            out[m] = hi - lo
    return out


def _same(a, b):
    """bit for bit, or NaN for NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_llr_of_bins_that_are_not_finite():
    sf, ppm = 6, 4                      # shift 2, half 2: bins 62, 63 round up to v = 16, whose masked Gray value 8 is not bin 0's
    N = 1 << sf
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    assert int(S.gray_map(sf, ppm)[N - 1]) == 8 and int(S.gray_map(sf, ppm)[0]) == 0
    rows = np.zeros((7, N), np.complex64)
    rows[0, 9] = 3 + 4j; rows[0, 40] = 2; rows[0, 11] = complex(np.nan, 0)               # a NaN bin beside finite ones: never enters
    rows[1, 9] = 3 + 4j; rows[1, 40] = complex(np.inf, 0)                                # +Inf enters: bits of g(40) +Inf, the others -Inf
    rows[2, 9] = complex(np.inf, 0); rows[2, 40] = complex(0, -np.inf)                   # +Inf on both sides of a bit: NaN there
    rows[3, :] = complex(np.nan, np.nan)                                                 # all NaN: nothing admitted
    # row 4: all zero
    rows[5, :] = complex(np.nan, 1); rows[5, 63] = 2                                     # every bin NaN but the last
    rows[6, 9] = complex(np.inf, np.nan); rows[6, 40] = 1e-30                            # Inf beside NaN is NaN: out; 1e-60 underflows to 0: not admitted
    got = S.llr_def(rows, sf, ppm)
    assert got.dtype == np.float32 and got.shape == (7, ppm)
    P = S.power_def(rows)
    for r in range(7):
        assert _same(got[r], _serial_llr(P[r], sf, ppm)), (r, got[r])
    g9, g40 = int(S.gray_map(sf, ppm)[9]), int(S.gray_map(sf, ppm)[40])
    assert (g9, g40) == (3, 15)
    assert got[0].tolist() == [25 - 0, 25 - 0, 4 - 25, 4 - 25]                           # as if the NaN bin were not there
    assert got[1].tolist() == [np.inf, np.inf, np.inf, np.inf]
    assert got[2, :2].tolist() == [np.inf, np.inf] and np.isnan(got[2, 2:]).all()        # bits 0, 1: both bins on side 1, Inf - 0; bits 2, 3: Inf - Inf
    for r in (3, 4, 6):
        assert np.array_equal(got[r].view(np.uint32), np.zeros(ppm, np.uint32)), (r, got[r])        # +0.0, not -0.0, not NaN
    assert got[5].tolist() == [-4, -4, -4, 4]
    # finite rows: the rule is the plain maximum
    rng = np.random.default_rng(6)
    bins = (rng.standard_normal((16, N)) + 1j * rng.standard_normal((16, N))).astype(np.complex64)
    Pf = S.power_def(bins)
    for m in range(ppm):
        one = ((S.gray_map(sf, ppm) >> np.uint32(m)) & 1).astype(bool)
        assert np.array_equal(S.llr_def(bins, sf, ppm)[:, m], Pf[:, one].max(axis=1) - Pf[:, ~one].max(axis=1))


def _nibble_loop(L, rate):
    """the rule of include/lorahip.h in scalar float32: x = 0 the incumbent, replaced only by M(x) > M(incumbent)"""
    best, best_m = 0, None
    for x in range(16):
        with np.errstate(invalid="ignore"):
            m = _metric(np.asarray(L, np.float32), x, rate, np.float32)
        if x == 0 or m > best_m:
            best, best_m = x, m
    return best


def test_soft_nibble_on_llrs_that_are_not_finite():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    code = lambda x, r: int(D.fec_def(x, r))
    # a NaN LLR that every codeword reads: every M(x) is NaN, x = 0 stays
    assert S.soft_nibble(np.array([1, nan, -1, 1, 1, -1, 1, 1], np.float32), 4) == 0
    # 4/4: bit k of enc(x) is bit k of x. L = (+Inf, 1, -1, 1): M(x) = +Inf for odd x, -Inf for even x: the first odd x
    assert [code(x, 0) & 15 for x in range(16)] == list(range(16))
    assert S.soft_nibble(np.array([inf, 1, -1, 1, 0, 0, 0, 0], np.float32), 0) == 1
    assert S.soft_nibble(np.array([-inf, 1, -1, 1, 0, 0, 0, 0], np.float32), 0) == 0
    # M(0) = -Inf and a later M(x) NaN: L = (+Inf, +Inf, ...). x = 0: -Inf - Inf = -Inf; x = 1, 2: Inf - Inf = NaN (never win); x = 3: +Inf wins
    L = np.array([inf, inf, -1, -1, 0, 0, 0, 0], np.float32)
    with np.errstate(invalid="ignore"):
        M = [float(_metric(L, x, 0, np.float32)) for x in range(4)]
    assert M[0] == -np.inf and np.isnan(M[1]) and np.isnan(M[2]) and M[3] == np.inf
    assert S.soft_nibble(L, 0) == 3
    # the same with nothing finite to follow: M(0) = -Inf, every other M(x) NaN or -Inf -> 0 stays (argmax would answer the first NaN)
    L = np.array([inf, -inf, nan, nan, 0, 0, 0, 0], np.float32)
    with np.errstate(invalid="ignore"):
        M = np.array([_metric(L, x, 0, np.float32) for x in range(16)])
    assert np.isnan(M).all()
    assert S.soft_nibble(L, 0) == 0
    L = np.array([-inf, -inf, inf, 1, 0, 0, 0, 0], np.float32)       # M(0) = Inf - Inf ... : -(-Inf) - (-Inf) - Inf = NaN at x = 0: never replaced
    with np.errstate(invalid="ignore"):
        assert np.isnan(_metric(L, 0, 0, np.float32)) and _metric(L, 4, 0, np.float32) == np.inf
    assert S.soft_nibble(L, 0) == 0
    L = np.array([-inf, 2, -3, 5, 0, 0, 0, 0], np.float32)           # M(0) = +Inf - 2 + 3 - 5: every even x is +Inf, none greater: 0
    assert S.soft_nibble(L, 0) == 0
    L = np.array([inf, 2, -3, 5, 0, 0, 0, 0], np.float32)            # M(0) = -Inf, M(1) = +Inf
    assert S.soft_nibble(L, 0) == 1
    # mixed signs, every rate, random places of NaN / +Inf / -Inf: the vector form is the scalar loop
    rng = np.random.default_rng(41)
    seen_nan0 = seen_later = 0
    for trial in range(400):
        rate = trial % 5
        L = rng.standard_normal(8).astype(np.float32) * np.float32(4)
        for k in rng.choice(8, int(rng.integers(0, 4)), replace=False):
            L[k] = (nan, inf, -inf)[int(rng.integers(0, 3))]
        want = _nibble_loop(L, rate)
        assert S.soft_nibble(L, rate) == want, (trial, L, rate)
        with np.errstate(invalid="ignore"):
            M = np.array([_metric(L, x, rate, np.float32) for x in range(16)])
        seen_nan0 += int(np.isnan(M[0]))
        seen_later += int(not np.isnan(M[0]) and int(np.argmax(M)) != want)      # a later NaN that argmax would have answered
    assert seen_nan0 > 10 and seen_later > 10, (seen_nan0, seen_later)           # the draw holds both kinds
