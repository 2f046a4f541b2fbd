"""CPU: the polyphase synthesis filter bank without a device -- the gather + inverse FFT + fold evaluation (tests/psb_def.py) against the
direct-form definition its output has (tests/synthesizer_def.py), and the C ABI's symbols, shape check and refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import psb_def as pd
import synthesizer_def as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1        # LORAHIP_E_INVALID

# M, U, L, K: U <, =, > M, U not dividing M, L < U, L not a multiple of U, one FFT size per decade of M
SHAPES = [(8, 8, 64, 8), (16, 11, 131, 5), (32, 48, 1024, 32), (64, 64, 512, 64), (8, 3, 2, 3), (16, 40, 7, 9), (1024, 1024, 8195, 19),
          (128, 1, 9, 7), (256, 200, 1603, 256)]
NAMES = ("lorahip_psb_check", "lorahip_psb_create", "lorahip_psb_destroy", "lorahip_psb_reset", "lorahip_psb_out_count", "lorahip_psb_run")


@pytest.mark.parametrize("M,U,L,K", SHAPES)
def test_gather_fft_fold_is_the_direct_form(M, U, L, K):
    rng = np.random.default_rng(M * 13 + U)
    n = 2 * (-(-L // U)) + 5                                  # the filter fills and runs full for a while
    x = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    h = rng.uniform(-1.0, 1.0, L)                            # asymmetric: the tap order matters
    g = rng.uniform(0.25, 2.0, K)
    bins = None if K == M else rng.integers(-M, 2 * M, K)    # negative, beyond M and (K > 1) most likely duplicate
    freqs = (np.arange(M) if bins is None else bins) / M
    for gains in (g, None):
        got = pd.synthesize(x, M, U, h, bins, gains)
        want = sd.synthesize(x, freqs, U, h, gains)
        assert got.shape == want.shape == (n * U,)
        err = float(np.abs(got - want).max()) / sd.error_scale(x, h, U, gains)
        print("M %d U %d L %d K %d: err / scale %.3g" % (M, U, L, K, err))
        assert err <= 1e-12
        assert float(np.abs(want).max()) > 0.0
    if L < U:
        assert np.all(got.reshape(n, U)[:, L:] == 0)


def test_symbols_nulls_and_shape_check():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    check = lib.lorahip_psb_check
    assert check(64, 64, 512, 64) == 0
    # each limit, its two neighbours, and what is not a power of two; the text a refusal must carry
    bins_, interp_, taps_, sel_ = "n_bins must be", "interp must be", "n_taps must be", "n_sel must be"
    table = [((8, 1, 1, 1), None), ((7, 1, 1, 1), bins_), ((9, 1, 1, 1), bins_), ((4, 1, 1, 1), bins_), ((16, 1, 1, 1), None),
             ((1024, 1, 1, 1), None), ((1023, 1, 1, 1), bins_), ((1025, 1, 1, 1), bins_), ((2048, 1, 1, 1), bins_), ((512, 1, 1, 1), None),
             ((0, 1, 1, 1), bins_), ((1, 1, 1, 1), bins_), ((12, 1, 1, 1), bins_), ((40, 1, 1, 1), bins_), ((96, 1, 1, 1), bins_), ((640, 1, 1, 1), bins_),
             ((64, 0, 8, 1), interp_), ((64, 1, 8, 1), None), ((64, 2, 8, 1), None), ((64, 4095, 8, 1), None), ((64, 4096, 8, 1), None), ((64, 4097, 8, 1), interp_),
             ((64, 64, 0, 1), taps_), ((64, 64, 1, 1), None), ((64, 64, 2, 1), None), ((64, 64, 65535, 1), None), ((64, 64, 65536, 1), None), ((64, 64, 65537, 1), taps_),
             ((64, 64, 8, 0), sel_), ((64, 64, 8, 1), None), ((64, 64, 8, 2), None), ((64, 64, 8, 65535 * 8 - 1), None), ((64, 64, 8, 65535 * 8), None),
             ((64, 64, 8, 65535 * 8 + 1), sel_)]
    for args, why in table:
        rc = check(*args)
        assert rc == (0 if why is None else INVALID), (args, rc)
        if why is not None:
            text = lib.lorahip_last_error().decode()
            assert text.startswith("polyphase synthesiser") and why in text, (args, text)
    # NULL arguments
    taps = np.ones(8, np.float32)
    h = C.c_void_p()
    assert lib.lorahip_psb_create(None, None, 8, None, 8, None, 8, taps.ctypes.data, 8) == INVALID
    assert lib.lorahip_psb_create(C.byref(h), None, 8, None, 8, None, 8, taps.ctypes.data, 8) == INVALID       # no context: no CPU path
    assert not h.value
    assert lib.lorahip_last_error().decode().startswith("polyphase synthesiser")
    assert lib.lorahip_psb_reset(None) == INVALID
    assert lib.lorahip_psb_out_count(None, 100) == 0
    assert lib.lorahip_psb_run(None, None, 0, 0, None, None) == INVALID
    lib.lorahip_psb_destroy(None)
    assert lib.lorahip_version() == 4                      # an addition: the ABI version stays
    assert callable(L.PolyphaseSynthesizer) and "PolyphaseSynthesizer" in L.__all__


def test_header_is_plain_c99_with_the_bank_declarations(tmp_path):
    """include/lorahip.h compiles as C99 with -pedantic -Werror, and a C caller reaches the six entry points"""
    from lora_sdr_amd import _lib
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    lorahip_psb *p = 0; float h = 1.0f; size_t n = 7; int32_t b = -3;\n"
                   "    if (lorahip_psb_check(64, 64, 512, 64) != LORAHIP_OK) return 1;\n"
                   "    if (lorahip_psb_check(40, 64, 512, 64) != LORAHIP_E_INVALID) return 2;\n"
                   "    if (lorahip_psb_create(&p, 0, 8, &b, 1, 0, 1, &h, 1) != LORAHIP_E_INVALID || p != 0) return 3;\n"
                   "    if (lorahip_psb_out_count(0, 5) != 0) return 4;\n"
                   "    if (lorahip_psb_run(0, 0, 0, 0, 0, &n) != LORAHIP_E_INVALID) return 5;\n"
                   "    if (lorahip_psb_reset(0) != LORAHIP_E_INVALID) return 6;\n"
                   "    lorahip_psb_destroy(0);\n"
                   "    return lorahip_version() == 4 ? 0 : 7;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_create_without_a_device_fails_loudly():
    import lora_sdr_amd as L

    class NoContext:
        _h = None
    with pytest.raises(L.LoraHipError):                      # the object borrows a context; without one it refuses: there is no CPU path
        L.PolyphaseSynthesizer(NoContext(), 16, 16, np.ones(16, np.float32))
    with pytest.raises(ValueError):
        L.PolyphaseSynthesizer(NoContext(), 16, 16, np.ones(16, np.float32), bins=[1, 2], gains=[1.0])
