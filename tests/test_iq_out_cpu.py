"""CPU: the integer IQ output of the two synthesisers (include/lorahip.h, "Integer IQ output": lorahip_synthesizer_run_iq,
lorahip_psb_run_iq, the *_clipped pair) without a device -- the symbols, the refusal of a NULL handle, the header as plain C, the checks
Python makes before any call, and the numpy restatement of the definition (tests/iq_out_def.py) against hand-written cases."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import iq_out_def as qd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1        # LORAHIP_E_INVALID
NEW = ("lorahip_synthesizer_run_iq", "lorahip_psb_run_iq", "lorahip_synthesizer_clipped", "lorahip_psb_clipped")


def test_symbols_and_null_handles():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    lib = L.load()
    assert lib.lorahip_version() == 4                      # additions: the ABI version stays
    got, count = C.c_size_t(77), C.c_ulonglong(55)
    for fmt in (0, 1, 2):
        assert lib.lorahip_synthesizer_run_iq(None, None, 0, 0, None, fmt, 1.0, C.byref(got)) == INVALID
        assert lib.lorahip_psb_run_iq(None, None, 0, 0, None, fmt, 1.0, C.byref(got)) == INVALID
    assert lib.lorahip_synthesizer_clipped(None, C.byref(count)) == INVALID
    assert lib.lorahip_psb_clipped(None, C.byref(count)) == INVALID
    assert got.value == 77 and count.value == 55
    for cls in (L.Synthesizer, L.PolyphaseSynthesizer):
        assert callable(cls.run_int) and callable(cls.clipped)


def test_header_is_plain_c99_with_the_output_declarations(tmp_path):
    """include/lorahip.h compiles as C99 with -pedantic -Werror, and a C caller reaches the four entry points"""
    from lora_sdr_amd import _lib
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    size_t n = 7; unsigned long long c = 5; short iq16[2]; signed char iq8[2]; float row[2] = {0.0f, 0.0f};\n"
                   "    if (lorahip_synthesizer_run_iq(0, row, 1, 1, iq16, LORAHIP_IQ_SC16, 32767.0f, &n) != LORAHIP_E_INVALID) return 1;\n"
                   "    if (lorahip_psb_run_iq(0, row, 1, 1, iq8, LORAHIP_IQ_SC8, 127.0f, &n) != LORAHIP_E_INVALID) return 2;\n"
                   "    if (lorahip_synthesizer_clipped(0, &c) != LORAHIP_E_INVALID) return 3;\n"
                   "    if (lorahip_psb_clipped(0, &c) != LORAHIP_E_INVALID) return 4;\n"
                   "    return lorahip_version() == 4 && n == 7 && c == 5 ? 0 : 5;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_refuses_before_any_call_into_the_library():
    """the checks of run_int need no device: host tensors, numpy arrays, wrong dtypes, shapes and scales raise ValueError and name
    what is expected"""
    import torch
    from lora_sdr_amd import api
    host = torch.zeros((3, 8), dtype=torch.complex64)
    # the format and the scale are looked at first, the tensors after them
    for dtype in (torch.int32, torch.uint8, torch.float32, None):
        with pytest.raises(ValueError, match="torch.int16 or torch.int8"):
            api._iq_out_args(host, 3, dtype, None)
    for scale in (float("inf"), float("-inf"), float("nan"), 1e39, -1e39, "x"):
        with pytest.raises(ValueError, match="finite real number that float32 holds"):
            api._iq_out_args(host, 3, torch.int16, scale)
    # a numpy array, a host tensor, a wrong dtype and wrong shapes of the rows
    for rows in (np.zeros((3, 8), np.complex64), host, torch.zeros((3, 8), dtype=torch.float32), torch.zeros((2, 8), dtype=torch.complex64),
                 torch.zeros(24, dtype=torch.complex64)):
        for dtype, scale in ((torch.int16, None), (torch.int8, 0.5)):
            with pytest.raises(ValueError, match=r"rows must be a \(K, n\) complex64 device tensor"):
                api._iq_out_args(rows, 3, dtype, scale)
    # and of the output buffer
    for out in (np.zeros((64, 2), np.int16), torch.zeros((64, 2), dtype=torch.int16), torch.zeros((64, 2), dtype=torch.int8),
                torch.zeros((63, 2), dtype=torch.int16), torch.zeros((64, 3), dtype=torch.int16), torch.zeros(128, dtype=torch.int16)):
        with pytest.raises(ValueError, match=r"device tensor of dtype torch.int16.*strides \(2, 1\)"):
            api._iq_out_buffer(out, torch.int16, 64, None)


def _q(values, fmt, scale):
    q, n = qd.quantise(np.array(values, np.float32), fmt, scale)
    return q.tolist(), n


def test_the_numpy_definition_on_hand_written_cases():
    f32 = np.float32
    # ties to even, at scale 1
    assert _q([0.5, 1.5, 2.5, -0.5, -1.5], "sc16", 1.0) == ([0, 2, 2, 0, -2], 0)
    # the upper end: 32767.5 ties to 32768 and clips; the float32 below it (32767.498) rounds to 32767 and does not
    assert f32(32767.49) < f32(32767.5)
    assert _q([32767.5], "sc16", 1.0) == ([32767], 1)
    assert _q([32767.49], "sc16", 1.0) == ([32767], 0)
    # the lower end: -32768.5 ties to the even -32768 and does not clip, -32769 does
    assert _q([-32768.5], "sc16", 1.0) == ([-32768], 0)
    assert _q([-32769.0], "sc16", 1.0) == ([-32768], 1)
    assert _q([32767.0, -32768.0, 32768.0], "sc16", 1.0) == ([32767, -32768, 32767], 1)
    # non-finite values
    assert _q([np.nan], "sc16", 1.0) == ([0], 1)
    assert _q([np.inf, -np.inf], "sc16", 1.0) == ([32767, -32768], 2)
    assert _q([3e38, -3e38], "sc16", 2.0) == ([32767, -32768], 2)          # the product overflows to +-Inf
    assert _q([np.inf], "sc16", 0.0) == ([0], 1)                           # 0 * Inf = NaN
    # a denormal and the negative zero
    assert _q([1e-45, -1e-45, -0.0], "sc16", 1.0) == ([0, 0, 0], 0)
    assert _q([1e-45], "sc16", 3e38) == ([0], 0)
    # a negative scale mirrors, and the asymmetric range shows: -32768 is reachable only from the positive side
    assert _q([1.0, -1.0, 0.5, 1.5], "sc16", -32768.0) == ([-32768, 32767, -16384, -32768], 2)
    assert _q([0.25, 0.75, -0.25], "sc16", -2.0) == ([0, -2, 0], 0)        # -0.5 -> -0, -1.5 -> -2, 0.5 -> 0
    # one fp32 multiply: 0.1f * 32767f rounds to 3276.7 in fp32
    assert _q([0.1], "sc16", 32767.0) == ([int(np.rint(f32(0.1) * f32(32767.0)))], 0)
    # the sc8 bounds
    assert _q([127.0, 127.49, 127.5, 128.0, -128.0, -128.5, -129.0], "sc8", 1.0) == ([127, 127, 127, 127, -128, -128, -128], 3)
    assert _q([np.nan, np.inf, -np.inf, 3e38], "sc8", 2.0) == ([0, 127, -128, 127], 4)
    assert _q([1.0, -1.0, 0.5, -0.5], "sc8", 127.0) == ([127, -127, 64, -64], 0)      # 63.5 ties to the even 64
    # complex input is I, Q pairs, and the dtypes are the formats'
    q, n = qd.quantise(np.array([1 + 2j, 3e5 - 1j], np.complex64), "sc16", 1.0)
    assert q.dtype == np.int16 and q.tolist() == [[1, 2], [32767, -1]] and n == 1
    assert qd.quantise(np.zeros(3, np.float32), "sc8", 1.0)[0].dtype == np.int8


def test_the_numpy_and_torch_forms_agree():
    """the torch expression the GPU tests quantise run() with, against the numpy definition: ties, both ends, NaN, +-Inf, +-3e38, a
    denormal, -0.0, positive, negative and non-power-of-two scales"""
    import torch
    rng = np.random.default_rng(5)
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 32767.5, 32767.49, -32768.5, -32769.0,
                        127.5, -128.5, -129.0], np.float32)
    vals = np.concatenate([special, (rng.integers(-70000, 70000, 4000) + 0.5).astype(np.float32),
                           (rng.standard_normal(4000) * 20000).astype(np.float32), (rng.standard_normal(4000) * 100).astype(np.float32)])
    for fmt, tdt in (("sc16", torch.int16), ("sc8", torch.int8)):
        lo, hi = qd.BOUNDS[fmt]
        for scale in (1.0, -1.0, 0.37, 2.0, qd.DEFAULT_SCALE[fmt] / 20000.0):
            want, n = qd.quantise(vals, fmt, scale)
            r = torch.round(torch.from_numpy(vals) * float(np.float32(scale)))
            got = torch.nan_to_num(r, nan=0.0, posinf=float(hi), neginf=float(lo)).clamp(lo, hi).to(tdt)
            assert np.array_equal(got.numpy(), want), (fmt, scale)
            assert int((torch.isnan(r) | (r < lo) | (r > hi)).sum()) == n, (fmt, scale)
