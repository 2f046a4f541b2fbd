"""CPU: the host-side half of the batched encoder's C ABI -- lorahip_encode_num_symbols against the verbatim LoRaEncoder.cpp, the
configurations the entry points refuse, and the header with the new declarations as plain C99."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import lora_sdr_amd as L
from lora_sdr_amd import _lib

RATES = ["4/4", "4/5", "4/6", "4/7", "4/8"]
LENGTHS = list(range(0, 41)) + [100, 255, 300]


def cfg(sf=10, ppm=0, rdd=4, explicit=1, crc=1, whitening=1):
    return _lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, ppm, rdd, explicit, crc, whitening)


def num_symbols(c, n):
    return int(L.load().lorahip_encode_num_symbols(C.byref(c), n))


def test_struct_and_limits():
    lib = L.load()
    assert C.sizeof(_lib.EncoderCfg) == 8 + 6 * 4
    assert lib.lorahip_encode_max_bytes() == 4096 == lib.lorahip_decode_max_data_length()
    assert lib.lorahip_version() == 4                      # the additions do not change the ABI version
    d = cfg()                                              # the block's defaults (LoRaEncoder.cpp:78-85)
    assert (d.sf, d.ppm, d.rdd, d.explicit_hdr, d.crc, d.whitening) == (10, 0, 4, 1, 1, 1)


@pytest.mark.parametrize("sf", range(7, 13))
def test_num_symbols_equals_the_verbatim_encoder(ref, sf):
    """lorahip_encode_num_symbols == len(LoRaEncoder.cpp's output) over SF x rate x header x crc x symbol size x length, wherever
    the reference is defined; -1 for the empty message without crc and header (its own expression wraps)"""
    import numpy as np
    checked = 0
    for rdd, cr in enumerate(RATES):
        for explicit in (0, 1):
            for crc in (0, 1):
                for ppm in (0, sf - 1, sf - 2):
                    c = cfg(sf, ppm, rdd, explicit, crc)
                    for n in LENGTHS:
                        got = num_symbols(c, n)
                        if n == 0 and not crc:
                            # an empty byte vector: without a header the reference's own count wraps (-1 here); with one its
                            # encodeFec reads pad nibbles through a null pointer and the block crashes -- here the pad is 0
                            # and the count is the closed form (test_num_symbols_closed_form)
                            assert got == (8 if explicit else -1)
                            continue
                        want = len(ref.encode(sf, np.zeros(n, np.uint8), ppm=ppm, cr=cr, explicit=bool(explicit), crc=bool(crc)))
                        assert got == want, (sf, ppm, cr, explicit, crc, n, got, want)
                        checked += 1
    assert checked == 5 * 3 * (2 * len(LENGTHS) + 2 * (len(LENGTHS) - 1))


def test_num_symbols_closed_form():
    """without the reference build: LoRaEncoder.cpp:171-176 written out"""
    for sf in range(7, 13):
        for rdd in range(5):
            for explicit in (0, 1):
                for crc in (0, 1):
                    for ppm in (0, sf - 1, sf - 2):
                        P = ppm or sf
                        for n in LENGTHS:
                            ncw = -(-(2 * (n + 2 * crc) + 5 * explicit) // P) * P
                            want = -1 if ncw == 0 else 8 + (ncw // P - 1) * (4 + rdd)
                            assert num_symbols(cfg(sf, ppm, rdd, explicit, crc), n) == want
    c = cfg(12, 0, 0, 0, 0)
    counts = [num_symbols(c, n) for n in range(1, 200)]
    assert counts == sorted(counts)                        # never decreases: the count of the longest row bounds a launch


def test_refused_configurations():
    """LORAHIP_E_INVALID of section 'Batched encoder' in include/lorahip.h, through the host-only entry (no device needed): a valid
    configuration answers with a count, a refused one with -1"""
    lib = L.load()
    assert num_symbols(cfg(), 10) > 0
    bad = cfg(); bad.struct_size = 8
    assert num_symbols(bad, 10) == -1
    assert lib.lorahip_encode_num_symbols(None, 10) == -1
    for sf in (0, -1, 13):
        assert num_symbols(cfg(sf=sf), 10) == -1
    assert num_symbols(cfg(sf=7, ppm=8), 10) == -1         # PPM > SF: the reference throws
    assert num_symbols(cfg(sf=7, ppm=-1), 10) == -1
    for rdd in (-1, 5):
        assert num_symbols(cfg(rdd=rdd), 10) == -1
    assert num_symbols(cfg(sf=7, ppm=4, explicit=1), 10) == -1      # explicit header needs PPM >= 5
    assert num_symbols(cfg(sf=7, ppm=4, explicit=0), 10) > 0
    assert num_symbols(cfg(sf=7, ppm=5, explicit=1), 10) > 0
    assert num_symbols(cfg(), 4096) > 0 and num_symbols(cfg(), 4097) == -1
    # the device entries without a context: an error code, never a crash
    c = cfg()
    assert lib.lorahip_encode_packets(None, C.byref(c), None, 16, None, 0, None, 64, None) == -1
    assert lib.lorahip_encode_packets_host(None, C.byref(c), None, 16, None, 0, None, 64, None) == -1
    assert lib.lorahip_mod_frames_var(None, None, 0, None, 0, None, 0, 1, 0x12, 1.0, 1) == -1


def test_python_encoder_mirrors_the_block():
    import torch
    if torch.cuda.is_available():
        e = L.LoRaEncoder()
        with pytest.raises(ValueError):
            e.setCodingRate("4/9")
        e.setCodingRate("4/5")
        assert e._cfg.rdd == 1
    else:
        with pytest.raises(L.LoraHipError):                # no CPU path behind it
            L.LoRaEncoder()
    assert callable(L.transmit)


def test_header_is_plain_c99_with_the_encoder_declarations(tmp_path):
    """include/lorahip.h compiles as C99 with -pedantic -Werror, and a C caller can fill the encoder configuration"""
    cc = shutil.which("gcc")
    if cc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "lorahip.h"\n'
                   "int main(void) {\n"
                   "    lorahip_encoder_cfg c;\n"
                   "    c.struct_size = sizeof c; c.sf = 10; c.ppm = 0; c.rdd = 4; c.explicit_hdr = 1; c.crc = 1; c.whitening = 1;\n"
                   "    if (lorahip_encode_num_symbols(&c, 16) != 8 + (5 - 1) * 8) return 1;      /* 36 + 5 codewords -> 5 blocks of 10 */\n"
                   "    if (lorahip_encode_max_bytes() != 4096) return 2;\n"
                   "    if (lorahip_encode_packets(0, &c, 0, 0, 0, 0, 0, 8, 0) != LORAHIP_E_INVALID) return 3;\n"
                   "    if (lorahip_encode_packets_host(0, &c, 0, 0, 0, 0, 0, 8, 0) != LORAHIP_E_INVALID) return 4;\n"
                   "    if (lorahip_mod_frames_var(0, 0, 0, 0, 0, 0, 0, 1, 0x12, 1.0f, 1) != LORAHIP_E_INVALID) return 5;\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "use"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
