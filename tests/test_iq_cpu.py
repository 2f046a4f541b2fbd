"""CPU: the integer IQ input of the receive front ends (include/lorahip.h: LORAHIP_IQ_*, the *_run_iq entry points) without a device --
the symbols, the sample sizes, the refusal of a NULL handle, the header as plain C, and the checks Python makes before any call."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1        # LORAHIP_E_INVALID
NEW = ("lorahip_iq_sample_bytes", "lorahip_channelizer_run_iq", "lorahip_channelizer_run_captures_iq", "lorahip_pfb_run_iq")


def test_symbols_sizes_and_null_handles():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert lib.lorahip_version() == 4                      # additions: the ABI version stays
    assert (_lib.IQ_CF32, _lib.IQ_SC16, _lib.IQ_SC8) == (0, 1, 2)
    assert [lib.lorahip_iq_sample_bytes(f) for f in (0, 1, 2)] == [8, 4, 2]
    assert [lib.lorahip_iq_sample_bytes(f) for f in (3, -1, 255, 2 ** 31 - 1)] == [0, 0, 0, 0]
    got = C.c_size_t(77)
    for fmt in (0, 1, 2):
        assert lib.lorahip_channelizer_run_iq(None, None, fmt, 1.0, 0, None, 0, C.byref(got)) == INVALID
        assert lib.lorahip_channelizer_run_captures_iq(None, None, fmt, 1.0, 0, 0, 0, None, 0, C.byref(got)) == INVALID
        assert lib.lorahip_pfb_run_iq(None, None, fmt, 1.0, 0, None, 0, C.byref(got)) == INVALID
    assert got.value == 77
    for cls in (L.Channelizer, L.PolyphaseChannelizer):
        assert callable(cls.run_int)
    assert callable(L.Channelizer.run_captures_int)


def test_header_is_plain_c99_with_the_iq_declarations(tmp_path):
    """include/lorahip.h compiles as C99 with -pedantic -Werror, and a C caller reaches the formats and the four entry points"""
    from lora_sdr_amd import _lib
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    size_t n = 7; short iq16[2] = {1, -1}; signed char iq8[2] = {1, -1};\n"
                   "    if (LORAHIP_IQ_CF32 != 0 || LORAHIP_IQ_SC16 != 1 || LORAHIP_IQ_SC8 != 2) return 1;\n"
                   "    if (lorahip_iq_sample_bytes(LORAHIP_IQ_CF32) != 8 || lorahip_iq_sample_bytes(LORAHIP_IQ_SC16) != sizeof iq16) return 2;\n"
                   "    if (lorahip_iq_sample_bytes(LORAHIP_IQ_SC8) != sizeof iq8 || lorahip_iq_sample_bytes(3) != 0) return 3;\n"
                   "    if (lorahip_channelizer_run_iq(0, iq16, LORAHIP_IQ_SC16, 1.0f / 32768.0f, 1, 0, 0, &n) != LORAHIP_E_INVALID) return 4;\n"
                   "    if (lorahip_channelizer_run_captures_iq(0, iq8, LORAHIP_IQ_SC8, 1.0f / 128.0f, 1, 1, 1, 0, 0, &n) != LORAHIP_E_INVALID) return 5;\n"
                   "    if (lorahip_pfb_run_iq(0, iq16, LORAHIP_IQ_SC16, 1.0f, 1, 0, 0, &n) != LORAHIP_E_INVALID) return 6;\n"
                   "    return lorahip_version() == 4 && n == 7 ? 0 : 7;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_refuses_what_is_not_an_integer_device_tensor():
    """the checks of run_int come before any call into the library: host tensors, numpy arrays, wrong dtypes, shapes and scales raise
    ValueError and name what is expected"""
    import torch
    from lora_sdr_amd import api
    for wide in (np.zeros((8, 2), np.int16), torch.zeros((8, 2), dtype=torch.int16), torch.zeros(8, dtype=torch.complex64)):
        with pytest.raises(ValueError, match="int16 or int8 device tensor"):
            api._iq_args(wide, None, 0)
