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
