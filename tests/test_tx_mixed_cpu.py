"""CPU: the entry points of the mixed-SF transmit side (lorahip_encode_packets_cfgs[_host], lorahip_mod_frames_sched,
lorahip_mod_body_len) exist, refuse NULL and out-of-range arguments with LORAHIP_E_INVALID before anything touches a device, and the
body length is the definition's frame less its padding."""
import ctypes as C

import numpy as np
import pytest

import lora_sdr_amd as L
from lora_sdr_amd import _lib
from modulator_def import mod_frame_len_def

INVALID = -1


def cfg(sf=7, ppm=0, rdd=4, explicit=1, crc=1, whitening=1):
    return _lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, ppm, rdd, explicit, crc, whitening)


def table(*cfgs):
    t = (_lib.EncoderCfg * len(cfgs))()
    for i, c in enumerate(cfgs):
        t[i] = c
    return t


@pytest.fixture(scope="module")
def handle():
    """Something to pass as the context where the arguments behind it are what is refused: every check of these entry points comes before
    the first use of the context, so a refusal never reads it (a zeroed block, in case one ever did)."""
    block = (C.c_char * 65536)()
    return C.cast(block, C.c_void_p)


@pytest.mark.parametrize("sf", range(4, 15))
def test_body_len_is_the_frame_without_its_padding(sf):
    lib = L.load()
    N = 1 << sf
    for n in (0, 1, 2, 17, 64, 16384):
        want = mod_frame_len_def(sf, n, 1) - N if 6 <= sf <= 12 else 0
        assert lib.lorahip_mod_body_len(sf, n) == want, (sf, n)
        if want:
            assert want == 14 * N + N // 4 + n * N and want == lib.lorahip_mod_frame_len(sf, n, 1) - N


def test_python_names_exist():
    assert callable(L.transmit_mixed) and callable(L.LoRaEncoderSet) and callable(L.Context.mod_frames_sched)
    for name in ("lorahip_encode_packets_cfgs", "lorahip_encode_packets_cfgs_host", "lorahip_mod_body_len", "lorahip_mod_frames_sched"):
        assert name in _lib.SIGNATURES


@pytest.mark.parametrize("entry", ["lorahip_encode_packets_cfgs", "lorahip_encode_packets_cfgs_host"])
def test_encoder_table_refusals(handle, entry):
    fn = getattr(L.load(), entry)
    good = table(cfg(7), cfg(12, rdd=1))
    p = C.c_void_p(256)                                            # never read: every call below is refused or has no packets
    assert fn(None, good, 2, None, None, 0, None, 16, None, 0, None, 64, None) == INVALID                # no context
    assert fn(handle, None, 2, None, None, 0, None, 16, None, 0, None, 64, None) == INVALID              # no table of settings
    assert fn(handle, good, 0, None, None, 0, None, 16, None, 0, None, 64, None) == INVALID
    assert fn(handle, (_lib.EncoderCfg * 65)(*([cfg()] * 65)), 65, None, None, 0, None, 16, None, 0, None, 64, None) == INVALID
    assert fn(handle, (_lib.EncoderCfg * 64)(*([cfg()] * 64)), 64, None, None, 0, None, 16, None, 0, None, 64, None) == 0    # no packets: no work
    for bad in (cfg(sf=13), cfg(sf=0), cfg(ppm=8), cfg(rdd=5), cfg(rdd=-1), cfg(ppm=4, explicit=1), _lib.EncoderCfg(8, 7, 0, 4, 1, 1, 1)):
        assert fn(handle, table(cfg(7), bad), 2, None, None, 0, None, 16, None, 0, None, 64, None) == INVALID    # an entry no packet uses
    assert fn(handle, good, 2, None, p, 0, None, 16, None, 0, None, 64, None) == INVALID                 # a table of no entries
    assert fn(handle, good, 2, None, p, 0x80000000, None, 16, None, 0, None, 64, None) == INVALID
    lib = L.load()
    assert fn(handle, good, 2, None, None, 0, None, lib.lorahip_encode_max_bytes() + 1, None, 0, None, 64, None) == INVALID
    assert fn(handle, good, 2, None, None, 0, None, 16, None, 0, None, 0, None) == INVALID
    assert fn(handle, good, 2, None, None, 0, None, 16, None, 0, None, lib.lorahip_decode_max_symbols() + 1, None) == INVALID
    # packets, and a pointer missing
    assert fn(handle, good, 2, None, None, 0, p, 16, p, 3, p, 64, p) == INVALID                          # no index
    assert fn(handle, good, 2, p, None, 0, None, 16, p, 3, p, 64, p) == INVALID
    assert fn(handle, good, 2, p, None, 0, p, 16, None, 3, p, 64, p) == INVALID
    assert fn(handle, good, 2, p, None, 0, p, 16, p, 3, None, 64, p) == INVALID
    assert fn(handle, good, 2, p, None, 0, p, 16, p, 3, p, 64, None) == INVALID
    assert fn(handle, good, 2, p, None, 0, p, 16, p, 0x80000000, p, 64, p) == INVALID
    assert fn(handle, good, 2, None, None, 0, None, 16, None, 0, None, 64, None) == 0


def test_scheduled_modulator_refusals(handle):
    lib = L.load()
    fn = lib.lorahip_mod_frames_sched
    p = C.c_void_p(256)
    big = lib.lorahip_decode_max_symbols()

    def call(ctx=handle, iq=p, n_rows=4, stride=1000, row_len=1000, syms=p, sym_stride=8, nsyms=p, sf=p, row=p, start=p, ampl_of=None, n=3,
             lanes=0, status=None):
        return fn(ctx, iq, n_rows, stride, row_len, syms, sym_stride, nsyms, sf, row, start, ampl_of, n, 0x12, 1.0, lanes, status)
    assert call(ctx=None) == INVALID and call(ctx=None, n=0) == INVALID
    assert call(n=0) == 0 and call(n=0, iq=None, syms=None, nsyms=None, sf=None, row=None, start=None) == 0      # no frames: no work
    for missing in ("iq", "syms", "nsyms", "sf", "row", "start"):
        assert call(**{missing: None}) == INVALID, missing
    assert call(row_len=1001) == INVALID and call(n=0, row_len=1001) == INVALID
    assert call(sym_stride=0) == INVALID and call(sym_stride=big + 1) == INVALID and call(n=0, sym_stride=big) == 0
    for lanes in (-1, 1, 2, 8, 32, 63, 65, 128):
        assert call(lanes=lanes) == INVALID and call(n=0, lanes=lanes) == INVALID, lanes
    for lanes in (0, 4, 16, 64):
        assert call(n=0, lanes=lanes) == 0
    assert call(n=0x80000000) == INVALID and call(n_rows=0x80000000) == INVALID
