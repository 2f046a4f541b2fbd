"""CPU: the polyphase channeliser's 5 * 2^a bin counts without a device -- the C ABI's two new entry points (the seven bin counts and
nothing else, every limit from inside and one step outside, the old pair unchanged), uniform_plan for the 200 kHz LoRaWAN grids, and
the fold + FFT evaluation (tests/pfb_def.py) against the direct-form definition (oracle/channelizer.py) for these M: b / M is not exact
in the 64-bit phase counter there, so the GPU tests' yardstick is held to the direct definition here, to 1e-9 of the scale."""
import ctypes as C

import numpy as np
import pytest

import pfb_def as pd

INVALID = -1        # LORAHIP_E_INVALID
RADIX5 = (5, 10, 20, 40, 80, 160, 320)


def test_check_radix5_accepts_the_seven_bin_counts_and_nothing_else():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lorahip_pfb_check_radix5", "lorahip_pfb_create_radix5"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    check = lib.lorahip_pfb_check_radix5
    accepted = [M for M in range(0, 1400) if check(M, 1, 1, 1) == 0]
    assert accepted == list(RADIX5)
    for M in (0, 1, 3, 6, 8, 15, 16, 25, 30, 64, 640, 1280):
        assert check(M, 8, 64, 1) == INVALID, M
        assert lib.lorahip_last_error().decode().startswith("polyphase channeliser"), M
    # each limit from inside, and passed by one
    table = [((40, 0, 8, 1), False), ((40, 1, 8, 1), True), ((40, 4096, 8, 1), True), ((40, 4097, 8, 1), False),
             ((40, 64, 0, 1), False), ((40, 64, 1, 1), True), ((40, 64, 65536, 1), True), ((40, 64, 65537, 1), False),
             ((40, 64, 8, 0), False), ((40, 64, 8, 1), True), ((40, 64, 8, 65535 * 8), True), ((40, 64, 8, 65535 * 8 + 1), False),
             ((5, 1, 1, 1), True), ((320, 4096, 65536, 65535 * 8), True)]
    for args, ok in table:
        rc = check(*args)
        assert rc == (0 if ok else INVALID), (args, rc)
        if not ok:
            assert lib.lorahip_last_error().decode().startswith("polyphase channeliser"), args


def test_the_old_entry_points_are_unchanged_and_nulls_are_refused():
    import lora_sdr_amd as L
    lib = L.load()
    for M in RADIX5 + (12, 24, 96, 640):
        assert lib.lorahip_pfb_check(M, 1, 1, 1) == INVALID, M
        assert lib.lorahip_last_error().decode().startswith("polyphase channeliser"), M
    for log2m in range(3, 11):                                 # the two pairs are disjoint
        assert lib.lorahip_pfb_check(1 << log2m, 1, 1, 1) == 0
        assert lib.lorahip_pfb_check_radix5(1 << log2m, 1, 1, 1) == INVALID
    taps = np.ones(8, np.float32)
    h = C.c_void_p()
    assert lib.lorahip_pfb_create_radix5(None, None, 40, None, 40, 64, taps.ctypes.data, 8) == INVALID
    assert lib.lorahip_pfb_create_radix5(C.byref(h), None, 40, None, 40, 64, taps.ctypes.data, 8) == INVALID     # no context: no CPU path
    assert not h.value
    assert lib.lorahip_last_error().decode().startswith("polyphase channeliser")
    assert lib.lorahip_version() == 4                          # an addition: the ABI version stays
    assert callable(L.PolyphaseChannelizer.radix5) and callable(L.PolyphaseChannelizer.for_plan) and callable(L.uniform_plan)

    class NoContext:
        _h = None
    with pytest.raises(L.LoraHipError):
        L.PolyphaseChannelizer.radix5(NoContext(), 40, 64, taps)
    with pytest.raises(L.LoraHipError):
        L.PolyphaseChannelizer.for_plan(NoContext(), (5, 8, np.array([-1, 0, 1])), taps)


def test_uniform_plan_for_the_lorawan_grids():
    import lora_sdr_amd as L
    n_bins, decim, bins = L.uniform_plan(1e6, 868.3e6, [868.1e6, 868.3e6, 868.5e6])
    assert (n_bins, decim) == (5, 8) and bins.tolist() == [-1, 0, 1] and bins.dtype == np.int32
    us915 = 902.3e6 + 0.2e6 * np.arange(64)
    with pytest.raises(ValueError, match="off the channel grid"):         # bins -31.5 ...: the centre lies between two channels
        L.uniform_plan(16e6, 908.6e6, us915)
    n_bins, decim, bins = L.uniform_plan(16e6, 908.7e6, us915)
    assert (n_bins, decim) == (80, 128) and bins.tolist() == list(range(-32, 32))
    for fs, M, D in ((2e6, 10, 16), (4e6, 20, 32), (8e6, 40, 64), (32e6, 160, 256), (64e6, 320, 512)):
        assert L.uniform_plan(fs, 868.3e6, [868.1e6])[:2] == (M, D)
    # a power-of-two plan: spacing = bandwidth
    n_bins, decim, bins = L.uniform_plan(8e6, 915e6, 915e6 + 125e3 * np.array([-32, -1, 0, 5, 32]), spacing_hz=125e3)
    assert (n_bins, decim) == (64, 64) and bins.tolist() == [-32, -1, 0, 5, 32]
    assert L.uniform_plan(4e6, 0.0, [0.0], spacing_hz=250e3, bandwidth_hz=125e3)[:2] == (16, 32)


def test_uniform_plan_names_what_is_wrong():
    import lora_sdr_amd as L
    ch = [868.1e6, 868.3e6]
    with pytest.raises(ValueError, match="n_bins = sample rate / spacing"):
        L.uniform_plan(1.1e6, 868.3e6, ch)
    with pytest.raises(ValueError, match="decim = sample rate / bandwidth"):
        L.uniform_plan(1e6, 868.3e6, ch, bandwidth_hz=120e3)
    with pytest.raises(ValueError, match="a bin"):
        L.uniform_plan(1e6, 868.25e6, ch)
    with pytest.raises(ValueError, match="neither a power of two"):        # 3 MHz: 15 bins
        L.uniform_plan(3e6, 868.3e6, ch)
    with pytest.raises(ValueError, match="neither a power of two"):        # 128 MHz: 640 bins
        L.uniform_plan(128e6, 868.3e6, ch)
    with pytest.raises(ValueError, match="neither a power of two"):        # 4 bins: a power of two below 8
        L.uniform_plan(500e3, 868.3e6, [868.3e6], spacing_hz=125e3)
    with pytest.raises(ValueError, match="outside 1..4096"):
        L.uniform_plan(64e6, 868.3e6, ch, bandwidth_hz=7812.5)
    with pytest.raises(ValueError, match="out of band"):                   # bin 3 of 5
        L.uniform_plan(1e6, 868.3e6, [868.9e6])
    assert L.uniform_plan(2e6, 868.3e6, [869.3e6, 867.3e6])[2].tolist() == [5, -5]     # |bin| = n_bins / 2 is the band's edge: in
    with pytest.raises(ValueError, match="out of band"):
        L.uniform_plan(2e6, 868.3e6, [869.5e6])
    with pytest.raises(ValueError):
        L.uniform_plan(0.0, 868.3e6, ch)


@pytest.mark.parametrize("M,D,L", [(5, 8, 37), (5, 3, 2), (40, 64, 323), (40, 7, 19), (320, 512, 700), (320, 99, 150)])
def test_fold_and_fft_is_the_direct_form_for_these_bin_counts(M, D, L):
    """D > M and D < M (the first outputs then have n - s < 0), L < M and L not a multiple of M, negative bins and bins beyond +-M"""
    from oracle import channelizer as oc
    rng = np.random.default_rng(M * 7 + D)
    n = max(6 * D + 3, 2 * L + 5)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.uniform(-1.0, 1.0, L)                            # asymmetric: the tap order matters
    bins = np.concatenate([rng.permutation(M)[:min(M, 12)], [0, M // 2, M - 1, -1, -(M // 2), -3 * M - 2, 4, 4, M + 4]]).astype(np.int64)
    got = pd.channelize(x, M, D, h, bins)
    want = oc.channelize(x, bins / M, D, h)
    assert got.shape == want.shape == (bins.size, n // D)
    err = float(np.abs(got - want).max()) / pd.scale(x, h)
    print("M %d D %d L %d: err / scale %.3g" % (M, D, L, err))
    assert err <= 1e-9
    assert float(np.abs(want).max()) > 0.0


DEEP = ((1 << 31) + 12345, (1 << 32) + 54321)      # where tests/test_gpu_bank5_edges.py puts its noise


@pytest.mark.parametrize("M,D,L", [(5, 8, 37), (40, 64, 323), (320, 512, 700)])
def test_n0_is_that_many_explicit_zeros(M, D, L):
    """channelize(x, n0 = k) is channelize(k zeros + x) without the outputs of the zeros: k a multiple of M and of D, a multiple of D
    but not of M, and a multiple of neither; a short stream, all bins and some beyond +-M"""
    rng = np.random.default_rng(M + D)
    n = 3 * D + L + 5
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.uniform(-1.0, 1.0, L)
    bins = np.concatenate([np.arange(min(M, 12)), [M - 1, -1, -3 * M - 2, M + 4]]).astype(np.int64)
    starts = (M * D, M * D + D, 2 * M + 3)
    assert [(k % M == 0, k % D == 0) for k in starts] == [(True, True), (False, True), (False, False)]
    assert np.array_equal(pd.channelize(x, M, D, h, bins, n0=0), pd.channelize(x, M, D, h, bins))
    for k in starts:
        got = pd.channelize(x, M, D, h, bins, n0=k)
        want = pd.channelize(np.concatenate([np.zeros(k), x]), M, D, h, bins)[:, k // D:]
        assert got.shape == want.shape == (bins.size, (k + n) // D - k // D)
        assert np.array_equal(pd.out_times(n, D, k), np.arange(k // D, (k + n) // D))
        err = float(np.abs(got - want).max()) / pd.scale(x, h)
        print("M %d D %d L %d n0 %d: err / scale %.3g" % (M, D, L, k, err))
        assert err <= 1e-12
        assert float(np.abs(want).max()) > 0.0


def test_the_deep_positions_can_show_a_32_bit_position():
    """pure integers: 2^32 = 1 and 2^31 = 3 (mod 5), so a stream position cut to 32 bits (unsigned, from 2^32 on; signed, from 2^31
    on) or to 31 bits moves every residue n mod M the definition takes -- at every sample of the stretches the GPU test compares, for
    every radix-5 bin count. (For a power of two none of them moves.)"""
    for n0 in DEEP:
        n = n0 + np.arange(3 * 256 * 512 + 5, dtype=np.int64)          # beyond the longest stretch compared
        assert n.dtype == np.int64 and int(n[-1]) == n0 + 3 * 256 * 512 + 4
        cut = {"uint32": n & 0xFFFFFFFF, "int32": ((n + (1 << 31)) & 0xFFFFFFFF) - (1 << 31), "31 bits": n & 0x7FFFFFFF}
        assert np.array_equal(cut["int32"], n.astype(np.int32).astype(np.int64))
        for M in RADIX5:
            true = pd.residues(n, M)
            assert true.min() == 0 and true.max() == M - 1
            assert int(true[0]) == n0 % M                              # Python's own integers
            for name, t in cut.items():
                if name == "uint32" and n0 < 1 << 32:
                    assert np.array_equal(pd.residues(t, M), true)     # nothing is cut yet: the second position is there for this one
                else:
                    assert np.all(pd.residues(t, M) != true), (n0, M, name)
        for M in (8, 64, 1024):
            assert all(np.array_equal(pd.residues(t, M), pd.residues(n, M)) for t in cut.values())
