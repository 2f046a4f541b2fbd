"""CPU: the polyphase synthesis bank's 5 * 2^a bin counts without a device -- the C ABI's two new entry points (the seven bin counts and
nothing else, every limit from inside and one step outside, the old pair unchanged), the Python front, the tile rule the GPU shapes
are sized from, and the gather + inverse FFT + fold evaluation (tests/psb_def.py) against the direct-form definition
(tests/synthesizer_def.py) for these M: b / M is not exact in the 64-bit phase counter there, so the GPU tests' yardstick is held to
the exact-phase evaluation here, to 1e-9 of the scale (the margin of tests/test_pfb5_cpu.py; measured: at most 7e-13)."""
import ctypes as C

import numpy as np
import pytest

import psb_def as pd
import synthesizer_def as sd

INVALID = -1        # LORAHIP_E_INVALID
RADIX5 = (5, 10, 20, 40, 80, 160, 320)


def tile(M):
    """what lorahip_psb_create_radix5 derives from M: T = the largest power of two with T M <= 4096, 8 at least and 256 at most, and
    the input times of a workspace segment"""
    T = max(8, min(256, 1 << ((4096 // M).bit_length() - 1)))
    return T, (1 << 22) // M


def test_tiles_and_segments_by_the_constructors_rule():
    assert [tile(M)[0] for M in RADIX5] == [256, 256, 128, 64, 32, 16, 8]
    assert [tile(M)[1] for M in RADIX5] == [(1 << 22) // M for M in RADIX5] and tile(320)[1] == 13107
    for M in RADIX5:
        T = tile(M)[0]
        assert T & (T - 1) == 0 and (T * M <= 4096 or T == 8) and (2 * T * M > 4096 or T == 256)
        assert 8 * (T * (M + 1) + M // 10 + M) <= 23 << 10         # the transform's LDS: rows M + 1 apart and both tables


def test_check_radix5_accepts_the_seven_bin_counts_and_nothing_else():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lorahip_psb_check_radix5", "lorahip_psb_create_radix5"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    check = lib.lorahip_psb_check_radix5
    accepted = [M for M in range(1400) if check(M, 1, 1, 1) == 0]
    assert accepted == list(RADIX5)
    for M in (0, 1, 3, 6, 8, 15, 16, 25, 30, 64, 640, 1280):
        assert check(M, 8, 64, 1) == INVALID, M
        assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser"), M
    # each limit from inside, and passed by one
    table = [((40, 0, 8, 1), False), ((40, 1, 8, 1), True), ((40, 4096, 8, 1), True), ((40, 4097, 8, 1), False),
             ((40, 64, 0, 1), False), ((40, 64, 1, 1), True), ((40, 64, 65536, 1), True), ((40, 64, 65537, 1), False),
             ((40, 64, 8, 0), False), ((40, 64, 8, 1), True), ((40, 64, 8, 65535 * 8), True), ((40, 64, 8, 65535 * 8 + 1), False),
             ((5, 1, 1, 1), True), ((320, 4096, 65536, 65535 * 8), True)]
    for args, ok in table:
        rc = check(*args)
        assert rc == (0 if ok else INVALID), (args, rc)
        if not ok:
            assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser"), args


def test_the_old_entry_points_are_unchanged_and_nulls_are_refused():
    import lora_sdr_amd as L
    lib = L.load()
    for M in RADIX5 + (12, 24, 96, 640):
        assert lib.lorahip_psb_check(M, 1, 1, 1) == INVALID, M
        assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser"), M
    for log2m in range(3, 11):                                 # the two pairs are disjoint
        assert lib.lorahip_psb_check(1 << log2m, 1, 1, 1) == 0
        assert lib.lorahip_psb_check_radix5(1 << log2m, 1, 1, 1) == INVALID
        assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
    taps = np.ones(8, np.float32)
    h = C.c_void_p()
    assert lib.lorahip_psb_create_radix5(None, None, 40, None, 40, None, 64, taps.ctypes.data, 8) == INVALID
    assert lib.lorahip_psb_create_radix5(C.byref(h), None, 40, None, 40, None, 64, taps.ctypes.data, 8) == INVALID   # no context: no CPU path
    assert not h.value
    assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
    assert lib.lorahip_version() == 4                          # an addition: the ABI version stays


def test_python_front_without_a_device_fails_loudly():
    import lora_sdr_amd as L
    taps = np.ones(8, np.float32)
    assert callable(L.PolyphaseSynthesizer.radix5) and callable(L.PolyphaseSynthesizer.for_plan)

    class NoContext:
        _h = None
    with pytest.raises(L.LoraHipError):
        L.PolyphaseSynthesizer.radix5(NoContext(), 40, 64, taps)
    with pytest.raises(L.LoraHipError):
        L.PolyphaseSynthesizer.for_plan(NoContext(), (5, 8, np.array([-1, 0, 1])), taps)
    with pytest.raises(L.LoraHipError):                        # a power-of-two plan goes to the constructor, which needs a context too
        L.PolyphaseSynthesizer.for_plan(NoContext(), (64, 64, [0, 1]), taps, gains=[1.0, 0.5])
    with pytest.raises(L.LoraHipError):                        # 24 bins: neither constructor takes them
        L.PolyphaseSynthesizer.for_plan(NoContext(), (24, 4, [0]), taps)
    with pytest.raises(ValueError):
        L.PolyphaseSynthesizer.radix5(NoContext(), 40, 64, taps, bins=[1, 2], gains=[1.0])


@pytest.mark.parametrize("M,U,L", [(5, 8, 67), (10, 7, 80), (40, 64, 323), (160, 100, 700), (320, 512, 2563), (320, 273, 160)])
def test_gather_fft_fold_is_the_direct_form_for_these_bin_counts(M, U, L):
    """U > M and U < M, L < U and L not a multiple of U, 11 rows on random bins in [-2M, 3M) (negative, beyond M, duplicates at
    M = 5), with gains, 23 input times"""
    rng = np.random.default_rng(M * 13 + U)
    K, n = 11, 23
    x = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    h = rng.uniform(-1.0, 1.0, L)                            # asymmetric: the tap order matters
    g = rng.uniform(0.25, 2.0, K)
    bins = rng.integers(-2 * M, 3 * M, K)
    got = pd.synthesize(x, M, U, h, bins, g)
    want = sd.synthesize(x, bins / M, U, h, g)
    assert got.shape == want.shape == (n * U,)
    err = float(np.abs(got - want).max()) / sd.error_scale(x, h, U, g)
    print("M %d U %d L %d: err / scale %.3g" % (M, U, L, err))
    assert err <= 1e-9
    assert float(np.abs(want).max()) > 0.0
    if L < U:
        assert np.all(got.reshape(n, U)[:, L:] == 0)


DEEP = ((1 << 31) + 12345, (1 << 32) + 54321)      # the input times where tests/test_gpu_bank5_edges.py puts its noise


@pytest.mark.parametrize("M,U,L", [(5, 3, 20), (40, 64, 323), (320, 7, 150)])
def test_n0_is_that_many_explicit_zeros(M, U, L):
    """synthesize(rows, n0 = k) is synthesize(k zero input times + rows) without the outputs of the zeros: k a multiple of M, k not a
    multiple of M, and k with k U no multiple of M either; and synthesize_at, the direct form with the same integer phase, gives the
    same outputs at either position"""
    rng = np.random.default_rng(M * 13 + U)
    K, n = 7, 23
    x = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    h = rng.uniform(-1.0, 1.0, L)
    g = rng.uniform(0.25, 2.0, K)
    bins = rng.integers(-2 * M, 3 * M, K)
    bins[1] = bins[0] + M                                     # two rows on one bin
    starts = (3 * M, 3 * M + 1, 2 * M + 3)
    assert [k % M == 0 for k in starts] == [True, False, False] and (starts[2] * U) % M != 0
    assert np.array_equal(pd.synthesize(x, M, U, h, bins, g, n0=0), pd.synthesize(x, M, U, h, bins, g))
    scale = sd.error_scale(x, h, U, g)
    for k in (0,) + starts:
        got = pd.synthesize(x, M, U, h, bins, g, n0=k)
        want = pd.synthesize(np.concatenate([np.zeros((K, k)), x], axis=1), M, U, h, bins, g)[k * U:]
        assert got.shape == want.shape == (n * U,)
        at = pd.synthesize_at(x, M, U, h, bins, g, n=k * U + np.arange(n * U, dtype=np.int64), n0=k)
        err = float(np.abs(got - want).max()) / scale
        err_at = float(np.abs(at - want).max()) / scale
        print("M %d U %d L %d n0 %d: err / scale %.3g, the direct form %.3g" % (M, U, L, k, err, err_at))
        assert err <= 1e-12 and err_at <= 1e-12
        assert float(np.abs(want).max()) > 0.0


def test_the_deep_positions_can_show_a_32_bit_position():
    """pure integers: the residue of output n = m U + p is (m U + p) mod M; with the input time m cut to 32 bits (unsigned, from
    2^32 on; signed, from 2^31 on) or to 31 bits it moves by 2^32 U or 2^31 U, which is no multiple of 5 for the U = 3 of the GPU
    test -- at every output of the stretches compared there, for M = 5 and 10. (U = 5 would hide it, and so would a power of two.)"""
    U = 3
    for m0 in DEEP:
        m = m0 + np.arange(3 * 256 + 5, dtype=np.int64)
        cut = {"uint32": m & 0xFFFFFFFF, "int32": ((m + (1 << 31)) & 0xFFFFFFFF) - (1 << 31), "31 bits": m & 0x7FFFFFFF}
        assert np.array_equal(cut["int32"], m.astype(np.int32).astype(np.int64))
        for M in (5, 10):
            for p in range(U):
                true = pd.residues(m * U + p, M)
                assert int(true[0]) == (m0 * U + p) % M        # Python's own integers
                for name, t in cut.items():
                    if name == "uint32" and m0 < 1 << 32:
                        assert np.array_equal(pd.residues(t * U + p, M), true)     # nothing is cut yet: the second position is there for this
                    else:
                        assert np.all(pd.residues(t * U + p, M) != true), (m0, M, p, name)
            assert np.array_equal(pd.residues(cut["uint32"] * 5, M), pd.residues(m * 5, M))
        assert all(np.array_equal(pd.residues(t * U, 64), pd.residues(m * U, 64)) for t in cut.values())
