"""CPU: the rational-rate resampler without a device -- the float64 definition (tests/resampler_def.py) against an independent
construction from textbook pieces (scipy), against the synthesiser's definition at D = 1 and the channeliser's at U = 1, cut into
chunks; lorahip_resampler_check's limits; the C ABI's symbols and header; and bytes -> bytes through a stream at 6/5 of the grid rate
from the definitions alone, with the inputs of the device loopback in tests/test_gpu_resampler.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import resampler_def as rd
import synthesizer_def as sd

SYMBOLS = ["lorahip_resampler_check", "lorahip_resampler_plan", "lorahip_resampler_create", "lorahip_resampler_destroy", "lorahip_resampler_reset",
           "lorahip_resampler_reset_at", "lorahip_resampler_out_count", "lorahip_resampler_run", "lorahip_resampler_run_iq"]

SHAPES = [(5, 6, 192), (6, 5, 192), (25, 24, 800), (24, 25, 800), (25, 256, 4096), (125, 128, 4000), (1, 8, 64), (8, 1, 64), (1, 1, 1)]


def _rows(rng, K, n):
    return rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))


@pytest.mark.parametrize("U,D,L,N", [(5, 6, 120, 1000), (6, 5, 96, 777), (25, 24, 400, 500), (4, 6, 48, 601), (7, 3, 4, 300), (1, 8, 64, 1003),
                                     (8, 1, 64, 250), (1, 1, 1, 50), (25, 256, 1000, 3000)])
def test_definition_is_upfirdn_then_every_dth(U, D, L, N):
    """zero-stuff and filter with scipy.signal.upfirdn, then keep the samples D - 1, 2 D - 1, ...: floor(N U / D) of them"""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(U * 1000 + D)
    x = _rows(rng, 2, N)
    h = rng.uniform(-1.0, 1.0, L)
    got = rd.resample(x, U, D, h)
    assert got.shape == (2, N * U // D) and rd.out_count(0, N, U, D) == N * U // D
    for k in range(2):
        full = signal.upfirdn(h, x[k], U, 1)                             # (N - 1) U + L samples come back: zeros behind them where L < U
        want = np.concatenate([full, np.zeros(max(0, N * U - full.size))])[D - 1::D][:N * U // D]
        assert want.shape == got[k].shape
        assert np.abs(got[k] - want).max() <= 1e-12 * rd.error_scale(x, h, U)
    # and the selected-output form is the same definition
    m = np.unique(rng.integers(0, N * U // D, 40))
    assert np.abs(rd.resample_at(x, U, D, h, m=m) - got[:, m]).max() <= 1e-12 * rd.error_scale(x, h, U)


@pytest.mark.parametrize("U,L", [(1, 9), (4, 31), (16, 128), (10, 3)])
def test_down_1_is_the_synthesiser_at_frequency_0(U, L):
    rng = np.random.default_rng(U)
    x = _rows(rng, 1, 400)
    h = rng.uniform(-1.0, 1.0, L)
    want = sd.synthesize(x, [0.0], U, h)
    got = rd.resample(x, U, 1, h)
    assert got.shape == (1, want.size)
    assert np.abs(got[0] - want).max() <= 1e-12 * rd.error_scale(x, h, U)
    if L < U:
        assert np.all(got[0].reshape(-1, U)[:, L:] == 0)               # phases without a tap


@pytest.mark.parametrize("D,L", [(1, 5), (8, 64), (7, 30), (16, 129)])
def test_up_1_is_the_channeliser_at_frequency_0(D, L):
    from oracle import channelizer as oc
    rng = np.random.default_rng(D)
    x = _rows(rng, 1, 1000)
    h = rng.uniform(-1.0, 1.0, L)
    want = oc.channelize(x[0], [0.0], D, h)
    got = rd.resample(x, 1, D, h)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * rd.error_scale(x, h, 1)


@pytest.mark.parametrize("U,D,L", [(25, 24, 400), (3, 7, 20), (6, 5, 96)])
def test_chunks_at_their_positions_add_up_to_one_piece(U, D, L):
    """the definition is linear and rows before n0 read as zero: the stream is the sum of its chunks, each standing at its position n0
    and followed by zeros -- and out_count of the chunks adds up"""
    rng = np.random.default_rng(U + D)
    N = 900
    x = _rows(rng, 3, N)
    h = rng.uniform(-1.0, 1.0, L)
    whole = rd.resample(x, U, D, h)
    total, pos, count = np.zeros_like(whole), 0, 0
    for s in [1, 3, 0, 7, 200, 5, 111, 2, 571]:
        chunk = np.zeros((3, N - pos), np.complex128)
        chunk[:, :s] = x[:, pos:pos + s]
        part = rd.resample(chunk, U, D, h, n0=pos)
        assert part.shape[1] == rd.out_count(pos, N - pos, U, D) == whole.shape[1] - pos * U // D
        total[:, pos * U // D:] += part
        count += rd.out_count(pos, s, U, D)
        pos += s
    assert pos == N and count == whole.shape[1]
    assert np.abs(total - whole).max() <= 1e-12 * rd.error_scale(x, h, U)
    # a deep position moves nothing but the indices when it is a multiple of D: the same values
    deep = rd.resample(x, U, D, h, n0=D * (2 ** 40 + 1))
    assert np.array_equal(deep, whole)


def test_check_accepts_the_listed_shapes_and_refuses_beyond_the_limits():
    import lora_sdr_amd as L
    lib = L.load()
    for U, D, taps in SHAPES:
        for rows in (1, 64):
            assert lib.lorahip_resampler_check(U, D, taps, rows) == 0, (U, D, taps, rows, lib.lorahip_last_error())
    assert lib.lorahip_resampler_check(1024, 1024, 65536, 65535 * 8) == 0
    assert lib.lorahip_resampler_check(1, 1024, 64, 1) == 0 and lib.lorahip_resampler_check(1024, 1, 64, 1) == 0
    for bad in [(0, 6, 192, 1), (5, 0, 192, 1), (5, 6, 0, 1), (5, 6, 192, 0), (1025, 6, 192, 1), (5, 1025, 192, 1), (5, 6, 65537, 1),
                (5, 6, 192, 65535 * 8 + 1), (1, 1, 65536, 1)]:           # the last one: 65536 samples of history do not fit the LDS
        lib.lorahip_resampler_check(5, 6, 192, 1)
        assert lib.lorahip_resampler_check(*bad) == -1, bad              # LORAHIP_E_INVALID
        text = lib.lorahip_last_error()
        assert text.startswith(b"resampler: ") and len(text) > 20, (bad, text)


def test_symbols_and_entry_points(tmp_path):
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
    taps = np.ones(4, np.float32)
    assert lib.lorahip_resampler_create(None, None, 1, 2, 3, taps.ctypes.data, 4) == -1       # LORAHIP_E_INVALID
    h = C.c_void_p()
    assert lib.lorahip_resampler_create(C.byref(h), None, 1, 2, 3, taps.ctypes.data, 4) == -1   # no context: no CPU path
    assert not h.value
    assert lib.lorahip_resampler_out_count(None, 100) == 0
    assert lib.lorahip_resampler_reset(None) == -1 and lib.lorahip_resampler_reset_at(None, 5) == -1
    assert lib.lorahip_resampler_run(None, None, 0, 0, None, 0, None) == -1
    assert lib.lorahip_resampler_run_iq(None, None, 1, 1.0, 0, 0, None, 0, None) == -1
    lib.lorahip_resampler_destroy(None)
    assert lib.lorahip_version() == 4                      # additions: the ABI version stays
    assert callable(L.Resampler)
    t = L.Resampler.design(6, 5, 192)
    assert t.dtype == np.float32 and t.shape == (192,) and np.array_equal(t, (6.0 * L.design_lowpass(6, 192)).astype(np.float32))
    assert np.array_equal(L.Resampler.design(5, 6, 192), (5.0 * L.design_lowpass(6, 192)).astype(np.float32))
    # include/lorahip.h with the new declarations is plain C99
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    lorahip_resampler *r = 0;\n"
                   "    float h = 1.0f; size_t n = 7;\n"
                   "    lorahip_resampler_tiling t;\n"
                   "    if (lorahip_resampler_check(5, 6, 192, 1) != LORAHIP_OK) return 1;\n"
                   "    if (lorahip_resampler_check(5, 1025, 192, 1) != LORAHIP_E_INVALID) return 2;\n"
                   "    if (lorahip_resampler_plan(5, 6, 192, 1, &t) != LORAHIP_OK || t.up_reduced != 5 || t.down_reduced != 6 || t.t != 39) return 9;\n"
                   "    if (lorahip_resampler_plan(5, 1025, 192, 1, &t) != LORAHIP_E_INVALID || t.ns != 0) return 10;\n"
                   "    if (lorahip_resampler_plan(5, 6, 192, 1, 0) != LORAHIP_E_INVALID) return 11;\n"
                   "    if (lorahip_resampler_create(&r, 0, 1, 5, 6, &h, 1) != LORAHIP_E_INVALID || r != 0) return 3;\n"
                   "    if (lorahip_resampler_out_count(0, 5) != 0) return 4;\n"
                   "    if (lorahip_resampler_run(0, 0, 0, 0, 0, 0, &n) != LORAHIP_E_INVALID) return 5;\n"
                   "    if (lorahip_resampler_run_iq(0, 0, LORAHIP_IQ_SC16, 1.0f, 0, 0, 0, 0, &n) != LORAHIP_E_INVALID) return 6;\n"
                   "    if (lorahip_resampler_reset(0) != LORAHIP_E_INVALID || lorahip_resampler_reset_at(0, 1) != LORAHIP_E_INVALID) return 7;\n"
                   "    lorahip_resampler_destroy(0);\n"
                   "    return lorahip_version() == 4 ? 0 : 8;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_byte_loopback_at_a_rate_off_the_grid_from_the_definitions(oracle, ref):
    """the inputs of tests/test_gpu_resampler.py::test_device_loopback_at_a_rate_off_the_grid, every step a float64 / restated
    definition: synthesiser (16x) -> resampler 6/5 (the "2.4 Msps" stream) -> noise -> resampler 5/6 -> channeliser -> restated
    demodulator -> restated decoder returns every channel's bytes with crc check and error check on. The proof that the grid and the
    tap counts of resampler_def.LOOPBACK_* leave the reference chain inside its margin."""
    import lora_sdr_amd as L
    from oracle import channelizer as oc
    sf, cr = 7, "4/5"
    msgs, freqs = rd.loopback_messages(sf), rd.LOOPBACK_FREQS
    K, U, N = 8, rd.LOOPBACK_INTERP, 1 << sf
    h = L.design_lowpass(U, rd.LOOPBACK_CHANNEL_TAPS, cutoff=0.6 / U)
    syms = [ref.encode(sf, m, cr=cr) for m in msgs]
    mtu = len(ref.encode(sf, np.zeros(max(len(m) for m in msgs), np.uint8), cr=cr))
    frames = np.stack([oracle.mod_frame(sf, s, padding=2 + mtu - len(s)) for s in syms])
    frames = np.concatenate([np.zeros((K, N // 2 + 3), np.complex64), frames, np.zeros((K, 3 * N), np.complex64)], axis=1)
    rows = sd.stagger(frames)
    wide = sd.synthesize(rows, freqs, U, U * h.astype(np.float64))
    up = rd.resample(wide[None], 6, 5, L.Resampler.design(6, 5, rd.LOOPBACK_RESAMPLER_TAPS))[0]
    assert up.size == wide.size * 6 // 5
    rng = np.random.default_rng(3)
    up = up + rd.LOOPBACK_SIGMA * (rng.standard_normal(up.size) + 1j * rng.standard_normal(up.size))
    back = rd.resample(up[None], 5, 6, L.Resampler.design(5, 6, rd.LOOPBACK_RESAMPLER_TAPS))[0]
    narrow = oc.channelize(back, freqs, U, h)
    for k in range(K):
        pk = oracle.demod_run(sf, narrow[k].astype(np.complex64), mtu=mtu)["packets"]
        assert len(pk) == 1, (k, len(pk))
        out, dropped = oracle.decode(sf, pk[0][1], cr=cr, crcc=True, error_check=True)
        assert dropped == 0 and out is not None and np.array_equal(out, msgs[k]), k
