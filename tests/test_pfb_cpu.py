"""CPU: the polyphase filter-bank channeliser without a device -- the fold + FFT evaluation (tests/pfb_def.py) against the direct-form
definition the object's rows have (oracle/channelizer.py), the exactness of b / M in the 64-bit phase counter that makes the two the
same thing, and the C ABI's symbols, shape check and refusals."""
import ctypes as C

import numpy as np
import pytest

import pfb_def as pd

INVALID = -1        # LORAHIP_E_INVALID

# M, D, L: D < M, D > M, D = M, L < M, L not a multiple of M, one tap set per residue and fewer
SHAPES = [(8, 8, 64), (16, 20, 128), (64, 64, 512), (32, 5, 37), (4, 1, 9), (1024, 1024, 4096), (16, 3, 7), (128, 160, 1027)]


@pytest.mark.parametrize("M,D,L", SHAPES)
def test_fold_and_fft_is_the_direct_form(M, D, L):
    from oracle import channelizer as oc
    rng = np.random.default_rng(M * 7 + D)
    n = max(6 * D + 3, 2 * L + 5) if M < 1024 else 6 * D + 3
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.uniform(-1.0, 1.0, L)                            # asymmetric: the tap order matters
    bins = np.concatenate([rng.permutation(M)[:min(M, 12)], [0, M // 2, M - 1, -1, -M // 2, -3 * M - 2, 5, 5, M + 5]]).astype(np.int64)
    got = pd.channelize(x, M, D, h, bins)
    want = oc.channelize(x, bins / M, D, h)
    assert got.shape == want.shape == (bins.size, n // D)
    err = float(np.abs(got - want).max()) / pd.scale(x, h)
    print("M %d D %d L %d: err / scale %.3g" % (M, D, L, err))
    assert err <= 1e-12
    assert float(np.abs(want).max()) > 0.0
    if M <= 64:                                              # the whole bank, in order
        full = pd.channelize(x, M, D, h)
        assert np.abs(full - oc.channelize(x, np.arange(M) / M, D, h)).max() <= 1e-12 * pd.scale(x, h)


def test_bin_frequencies_are_exact_in_the_phase_counter():
    import lora_sdr_amd as L
    from oracle import channelizer as oc
    lib = L.load()
    for log2m in range(3, 11):
        M = 1 << log2m
        for b in sorted({0, 1, 2, 3, M // 2 - 1, M // 2, M // 2 + 1, M - 1, M, M + 3, -1, -2, -M // 2, -M, -3 * M + 5, 12345, -54321}):
            want = (b % M) * 2 ** 64 // M
            assert int(lib.lorahip_channelizer_phase_inc(b / M)) == want, (M, b)
            assert oc.phase_inc(b / M) == want, (M, b)


def test_symbols_nulls_and_shape_check():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lorahip_pfb_check", "lorahip_pfb_create", "lorahip_pfb_destroy", "lorahip_pfb_reset", "lorahip_pfb_out_count", "lorahip_pfb_run"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    check = lib.lorahip_pfb_check
    assert check(64, 64, 512, 64) == 0
    # each limit, its two neighbours, and what is not a power of two
    table = [((8, 1, 1, 1), True), ((7, 1, 1, 1), False), ((9, 1, 1, 1), False), ((4, 1, 1, 1), False), ((16, 1, 1, 1), True),
             ((1024, 1, 1, 1), True), ((1023, 1, 1, 1), False), ((1025, 1, 1, 1), False), ((2048, 1, 1, 1), False), ((512, 1, 1, 1), True),
             ((0, 1, 1, 1), False), ((1, 1, 1, 1), False), ((12, 1, 1, 1), False), ((40, 1, 1, 1), False), ((640, 1, 1, 1), False), ((96, 1, 1, 1), False),
             ((64, 0, 8, 1), False), ((64, 1, 8, 1), True), ((64, 2, 8, 1), True), ((64, 4095, 8, 1), True), ((64, 4096, 8, 1), True), ((64, 4097, 8, 1), False),
             ((64, 64, 0, 1), False), ((64, 64, 1, 1), True), ((64, 64, 2, 1), True), ((64, 64, 65535, 1), True), ((64, 64, 65536, 1), True), ((64, 64, 65537, 1), False),
             ((64, 64, 8, 0), False), ((64, 64, 8, 1), True), ((64, 64, 8, 2), True), ((64, 64, 8, 65535 * 8 - 1), True), ((64, 64, 8, 65535 * 8), True),
             ((64, 64, 8, 65535 * 8 + 1), False)]
    for args, ok in table:
        rc = check(*args)
        assert rc == (0 if ok else INVALID), (args, rc)
        if not ok:
            assert lib.lorahip_last_error().decode().startswith("polyphase channeliser"), args
    # NULL arguments
    taps = np.ones(8, np.float32)
    h = C.c_void_p()
    assert lib.lorahip_pfb_create(None, None, 8, None, 8, 8, taps.ctypes.data, 8) == INVALID
    assert lib.lorahip_pfb_create(C.byref(h), None, 8, None, 8, 8, taps.ctypes.data, 8) == INVALID       # no context: no CPU path
    assert not h.value
    assert lib.lorahip_pfb_reset(None) == INVALID
    assert lib.lorahip_pfb_out_count(None, 100) == 0
    assert lib.lorahip_pfb_run(None, None, 0, None, 0, None) == INVALID
    lib.lorahip_pfb_destroy(None)
    assert lib.lorahip_version() == 4                      # an addition: the ABI version stays
    assert callable(L.PolyphaseChannelizer)


def test_create_without_a_device_fails_loudly():
    import torch
    import lora_sdr_amd as L
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert L.device_count() == 0
    with pytest.raises(L.LoraHipError):                      # the object borrows a context, and there is none to be had
        L.Context(7)

    class NoContext:
        _h = None
    with pytest.raises(L.LoraHipError):                      # ... and without one it refuses: there is no CPU path
        L.PolyphaseChannelizer(NoContext(), 16, 16, np.ones(16, np.float32))
