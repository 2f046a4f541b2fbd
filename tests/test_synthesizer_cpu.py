"""CPU: the front-end synthesiser without a device -- the C ABI's symbols, refusals and header; the float64 definition
(tests/synthesizer_def.py) against an independent implementation from textbook pieces; and bytes -> bytes through one wideband stream
from the definitions alone (synthesiser definition -> channeliser definition -> restated demodulator -> restated decoder), with the
inputs of the device loopback in tests/test_gpu_synthesizer.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import synthesizer_def as sd

SYMBOLS = ["lorahip_synthesizer_create", "lorahip_synthesizer_destroy", "lorahip_synthesizer_reset", "lorahip_synthesizer_out_count",
           "lorahip_synthesizer_run"]


def test_symbols_and_entry_points(tmp_path):
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
    taps = np.ones(4, np.float32); fr = np.zeros(1)
    assert lib.lorahip_synthesizer_create(None, None, 1, fr.ctypes.data, None, 2, taps.ctypes.data, 4) == -1      # LORAHIP_E_INVALID
    h = C.c_void_p()
    assert lib.lorahip_synthesizer_create(C.byref(h), None, 1, fr.ctypes.data, None, 2, taps.ctypes.data, 4) == -1  # no context: no CPU path
    assert not h.value
    assert lib.lorahip_synthesizer_out_count(None, 100) == 0
    assert lib.lorahip_synthesizer_reset(None) == -1
    assert lib.lorahip_synthesizer_run(None, None, 0, 0, None, None) == -1
    lib.lorahip_synthesizer_destroy(None)
    assert lib.lorahip_version() == 4                      # an addition: the ABI version stays
    assert callable(L.Synthesizer)
    # include/lorahip.h with the new declarations is plain C99
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    lorahip_synthesizer *s = 0;\n"
                   "    double f = 0.0; float h = 1.0f; size_t n = 7;\n"
                   "    if (lorahip_synthesizer_create(0, 0, 1, &f, 0, 1, &h, 1) != LORAHIP_E_INVALID) return 1;\n"
                   "    if (lorahip_synthesizer_create(&s, 0, 1, &f, 0, 1, &h, 1) != LORAHIP_E_INVALID || s != 0) return 2;\n"
                   "    if (lorahip_synthesizer_out_count(0, 5) != 0) return 3;\n"
                   "    if (lorahip_synthesizer_run(0, 0, 0, 0, 0, &n) != LORAHIP_E_INVALID) return 4;\n"
                   "    if (lorahip_synthesizer_reset(0) != LORAHIP_E_INVALID) return 5;\n"
                   "    lorahip_synthesizer_destroy(0);\n"
                   "    return lorahip_version() == 4 ? 0 : 6;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.parametrize("K,U,L,n,n0", [(3, 4, 31, 1000, 0), (5, 16, 128, 600, 0), (2, 1, 9, 257, 0), (4, 10, 3, 300, 0), (3, 8, 64, 500, 4096)])
def test_definition_is_stuff_filter_mix_sum(K, U, L, n, n0):
    """zero-stuff, scipy.signal.upfirdn, multiply by a float64 carrier whose frequency has a small integer period (so that the 64-bit
    phase increment is exact and the carrier can be evaluated from n mod period), scale, sum"""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(K * 100 + U)
    x = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    h = rng.uniform(-1.0, 1.0, L)
    periods = [1, 8, 16, 4, 32][:K]
    freqs = [0.0 if p == 1 else (3 if p > 4 else 1) / p * (-1) ** i for i, p in enumerate(periods)]
    gains = rng.uniform(0.25, 2.0, K)
    got = sd.synthesize(x, freqs, U, h, gains, n0=n0)
    idx = n0 * U + np.arange(n * U)
    want = np.zeros(n * U, np.complex128)
    for k in range(K):
        up = signal.upfirdn(h, x[k], up=U)
        up = np.concatenate([up, np.zeros(max(0, n * U - up.size))])[: n * U]      # (n - 1) U + L samples come back
        num = int(round(freqs[k] * periods[k]))
        carrier = np.exp(2j * np.pi * ((num * idx) % periods[k]) / periods[k])
        want += gains[k] * up * carrier
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the library's phase increment is the definition's
    import lora_sdr_amd
    lib = lora_sdr_amd.load()
    for f in freqs + [0.1, -0.35, 1.0 / 3.0]:
        assert int(lib.lorahip_channelizer_phase_inc(float(f))) == sd.phase_inc(float(f))


def test_definition_explicit_sum_and_zero_phases():
    rng = np.random.default_rng(2)
    K, U, L, n = 2, 10, 3, 50
    x = rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))
    h = np.array([0.5, -1.25, 2.0])
    freqs, gains = [0.05, -0.3], [1.5, 0.75]
    y = sd.synthesize(x, freqs, U, h, gains)
    assert np.all(y.reshape(n, U)[:, L:] == 0)             # phases without a tap
    for nn in (0, 1, 2, 10, 12, 491):
        s = 0j
        for k in range(K):
            turns = ((sd.phase_inc(freqs[k]) * nn) % (1 << 64)) / 2.0 ** 64
            for j in range(L):
                if nn - j >= 0 and (nn - j) % U == 0:
                    s += gains[k] * np.exp(2j * np.pi * turns) * h[j] * x[k, (nn - j) // U]
        assert abs(s - y[nn]) < 1e-12


@pytest.mark.parametrize("sf,cr", [(7, "4/5"), (9, "4/8")])
def test_byte_loopback_from_the_definitions(oracle, ref, sf, cr):
    """the inputs of tests/test_gpu_synthesizer.py::test_device_loopback_bytes_to_bytes, every step a float64 / restated definition:
    all 8 channels return their bytes with crc check and error check on (the integer delay of the two 128-tap filters at U = D = 16
    is absorbed by the demodulator's sync)"""
    import lora_sdr_amd as L
    from oracle import channelizer as oc
    msgs, freqs, gains = sd.loopback_case(sf)
    K, U, Lt, N = 8, 16, 128, 1 << sf
    h = L.design_lowpass(U, Lt, cutoff=0.6 / U)
    syms = [ref.encode(sf, m, cr=cr) for m in msgs]
    longest_bytes = max(len(m) for m in msgs)
    mtu = len(ref.encode(sf, np.zeros(longest_bytes, np.uint8), cr=cr))      # the rows are walked to the longest message's length
    frames = np.stack([oracle.mod_frame(sf, s, padding=2 + mtu - len(s)) for s in syms])
    frames = np.concatenate([np.zeros((K, N // 2 + 3), np.complex64), frames, np.zeros((K, 3 * N), np.complex64)], axis=1)
    rows = sd.stagger(frames)
    wide = sd.synthesize(rows, freqs, U, U * h.astype(np.float64), gains)
    rng = np.random.default_rng(3)
    wide = wide + 0.2 * (rng.standard_normal(wide.size) + 1j * rng.standard_normal(wide.size))
    narrow = oc.channelize(wide, freqs, U, h)
    for k in range(K):
        pk = oracle.demod_run(sf, narrow[k].astype(np.complex64), mtu=mtu)["packets"]
        assert len(pk) == 1, (k, len(pk))
        out, dropped = oracle.decode(sf, pk[0][1], cr=cr, crcc=True, error_check=True)
        assert dropped == 0 and out is not None and np.array_equal(out, msgs[k]), k
