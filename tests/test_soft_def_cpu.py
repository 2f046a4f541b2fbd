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
