"""CPU: the coding rate from the explicit header (rdd = LORAHIP_RDD_FROM_HEADER) and the header report (lorahip_packet_info), as far as
they need no device: tests/codec_hdr_def.py -- the definition the GPU tests compare the kernels with -- pinned to the reference through
the oracle; the inputs proven sound by the reference alone; lorahip_decode_plan for a header-rate entry; the refusals of every entry
point; the header as C. Every comparison is integer and exact.

A configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr, data_length)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as S
import codec_hdr_def as H
from test_decode_plan_cpu import KIB160, cfg_array, plan

PAIRS = ((7, 0), (9, 7))                                             # (sf, ppm) of the pinned sets: symbol size = sf, and two bits less
WALKED = 13                                                          # every 13th header of the grid also goes through the whole walk


@pytest.fixture(scope="module")
def lib():
    import lora_sdr_amd as L
    return L.load()


@functools.lru_cache(maxsize=None)
def grid_decodes(oracle, sf, ppm, r, hdr, crcc, ec):
    """the oracle over the 4096 headers of set H on a body coded at rate r, decoder set to rate r"""
    return S.oracle_table(oracle, (sf, ppm, r, crcc, 1, ec, 1, hdr, 8), S.set_h(sf, ppm, r))


@pytest.mark.parametrize("sf,ppm", PAIRS)
@pytest.mark.parametrize("r", range(5))
def test_header_fields_are_the_bytes_the_reference_posts(oracle, sf, ppm, r):
    """with enableHdr the reference posts bytes 0..2 = length, flags, residue (LoRaDecoder.cpp:283-291, :375): every posted header of the
    grid equals the restatement's, the grid's own three arrays are what it reads back, and a header from the encoder has residue 0"""
    packets = S.set_h(sf, ppm, r)
    ln, crc, rate = S.header_grid(range(256))
    length, flags, residue, err = H.header_fields(packets, sf, ppm)
    assert np.array_equal(length, ln) and np.array_equal(flags, crc | rate << 1) and not residue.any() and not err.any()
    assert np.array_equal(H.header_rate(packets, sf, ppm), rate)
    posted = 0
    for p, (o, dropped) in enumerate(grid_decodes(oracle, sf, ppm, r, 1, 0, 0)):
        assert (o is None) == bool(dropped) and (rate[p] <= 4 or dropped), p
        if o is not None:
            assert (int(o[0]), int(o[1]), int(o[2])) == (int(length[p]), int(flags[p]), int(residue[p])), p
            posted += 1
    assert posted >= 2048
    # a header whose checksum nibbles are wrong: the residue is the difference, in the restatement and in the posted byte
    s = D.flip(D.flip(packets[300], sf, ppm, r, 3, 1), sf, ppm, r, 3, 2)             # two bits of the codeword of ck >> 4: not correctable
    o, dropped = oracle.decode(sf, s, ppm=ppm, cr=S.RDD_TO_CR[r], hdr=True)
    f = H.header_fields(s, sf, ppm)
    assert f[3] and f[2] != 0 and (o is None or int(o[2]) == int(f[2]))
    assert (int(f[0]), int(f[1])) == (int(length[300]), int(flags[300]))


@pytest.mark.parametrize("sf,ppm", PAIRS)
@pytest.mark.parametrize("r", range(5))
def test_the_report_is_what_the_reference_shows_through_its_drops(oracle, sf, ppm, r):
    """crc from the reference's drop with crcc on and off, fec_error from its drop with error_check on and off, need_syms from
    codec_def.decoded_end / num_symbols_def, the outcome of the whole walk under all four flag settings -- on every 13th header of the grid,
    clean and with one header bit damaged"""
    P = ppm or sf
    grid = S.set_h(sf, ppm, r)
    ln, crc_flag, rate = S.header_grid(range(256))
    sel = list(range(0, grid.shape[0], WALKED))
    tables = {(crcc, ec): grid_decodes(oracle, sf, ppm, r, 0, crcc, ec) for crcc in (0, 1) for ec in (0, 1)}
    seen = set()
    for p in sel:
        rep = {}
        for (crcc, ec), table in tables.items():
            o, dropped, rep[crcc, ec] = H.walk(grid[p], (sf, ppm, r, crcc, 1, ec, 1, 0, 8))
            want_o, want_d = table[p]
            assert dropped == want_d and (o is None) == (want_o is None) and (o is None or np.array_equal(o, want_o)), (p, crcc, ec)
        length, rdd, crc, res, err, need = rep[0, 0]
        assert (length, rdd, res) == (ln[p], rate[p], 0)
        ended_in_header = bool(tables[0, 0][p][1])                   # dropped with both checks off: the rate field (:297) or the length (:313)
        assert ended_in_header == (rate[p] > 4 or need < 0)
        if ended_in_header:
            assert (crc, err) == (0, 0) and rep[1, 1][2:] == (0, 0, 0, need)
            seen.add("header")
            continue
        # the walk passed :313: need_syms, then the two flags from the drops
        c_end, _ = D.decoded_end(P, True, int(ln[p]) + (5 if crc_flag[p] else 3))
        assert need == D.num_symbols_def(-(-c_end // P) * P, P, r) <= grid.shape[1]
        assert err == tables[0, 1][p][1]                             # error_check on drops exactly the packets whose flag is up at the end
        want_crc = 0 if not crc_flag[p] else -1 if tables[1, 0][p][1] else 1
        assert crc == want_crc, p
        assert rep[1, 0][2] == crc and rep[0, 1][2] == (0 if err else crc)        # (a decode that error_check ended before: none evaluated)
        seen.add(("crc", crc)); seen.add(("err", err))
    assert seen >= {"header", ("crc", 0), ("crc", -1), ("err", 0)} and (r == 0 or ("err", 1) in seen)
    # one bit of a header codeword: corrected, flagged, and dropped by the error check in the header (:293) -- the fields stay reported
    for p in sel[:40]:
        for c in range(5):
            s = D.flip(grid[p], sf, ppm, r, c, (p + c) % 8)
            f = H.header_fields(s, sf, ppm)
            assert f[3] and (int(f[0]), int(f[1]), int(f[2])) == (ln[p], crc_flag[p] | rate[p] << 1, 0)
            o, dropped, rep = H.walk(s, (sf, ppm, r, 1, 1, 1, 1, 0, 8))
            assert (o, dropped) == (None, 1) == oracle.decode(sf, s, ppm=ppm, cr=S.RDD_TO_CR[r], crcc=True, error_check=True)
            assert rep == (ln[p], rate[p], 0, 0, 1, -1)


def test_the_own_pair_of_the_encoder_is_crc_1(oracle):
    """a packet from the definition's encoder with its own header: crc 1, no error, residue 0 -- and -1 once a payload bit is flipped"""
    for sf, ppm in PAIRS:
        for r in range(5):
            s, _ = D.build(sf, np.arange(11, dtype=np.uint8), ppm, r, True, True)
            cfg = (sf, ppm, r, 1, 1, 1, 1, 0, 8)
            o, dropped, rep = H.walk(s, cfg)
            assert dropped == 0 and o.tolist() == list(range(11)) and rep == (11, r, 1, 0, 0, s.size)
            assert H.walk(s, (sf, ppm, -1, 1, 1, 1, 1, 0, 8))[2] == rep
            bad = D.flip(D.flip(s, sf, ppm, r, (ppm or sf) + 2, 0), sf, ppm, r, (ppm or sf) + 2, 1)
            want = oracle.decode(sf, bad, ppm=ppm, cr=S.RDD_TO_CR[r], crcc=True)
            o, dropped, rep = H.walk(bad, (sf, ppm, r, 1, 1, 0, 1, 0, 8))
            assert (o, dropped) == (None, 1) == want and rep[2] == -1
    # not reached
    assert H.walk(np.zeros(7, np.uint16), (7, 0, -1, 0, 1, 0, 1, 0, 8)) == (None, 0, H.NOT_REACHED)
    assert H.walk(np.zeros(9, np.uint16), (7, 0, 2, 0, 0, 0, 1, 0, 8))[1:] == (0, H.NOT_REACHED)
    # without a header: the setter's length and rate, no residue
    s, _ = D.build(8, np.arange(6, dtype=np.uint8), 0, 3, False, True)
    assert H.walk(s, (8, 0, 3, 1, 1, 0, 0, 0, 6))[2] == (6, 3, 1, -1, 0, s.size)
    assert H.walk(s, (8, 0, 3, 0, 1, 0, 0, 0, 6))[2][:3] == (6, 3, 0)


def test_inputs_are_sound_by_the_reference_alone(ref):
    """the reference encodes at all 30 (SF, rate) settings, and the reference decodes each message at the rate its header names (crc check
    and error check on): the payload. The rate the header names is the one it was sent at."""
    rng = np.random.default_rng(30)
    for sf in range(7, 13):
        for r in range(5):
            payload = rng.integers(0, 256, int(rng.integers(1, 41))).astype(np.uint8)
            s = ref.encode(sf, payload, cr=S.RDD_TO_CR[r])
            named = int(H.header_rate(s, sf, 0))
            assert named == r
            o, dropped = ref.decode(sf, s, cr=S.RDD_TO_CR[named], crcc=True, error_check=True)
            assert dropped == 0 and np.array_equal(o, payload), (sf, r)


# ---- lorahip_decode_plan ------------------------------------------------------------------------------------------------------------------
STRIDES = S.G_STRIDES + (16384,)


def hdr_cfg(sf, ppm=0, crcc=1, ec=0, hdr=0):
    return (sf, ppm, H.RDD_FROM_HEADER, crcc, 1, ec, 1, hdr, 8)


def test_plan_of_a_header_rate_entry_is_the_largest_of_the_five_rates(lib):
    for sf in range(7, 13):
        for stride in STRIDES:
            rc, t = plan(lib, [hdr_cfg(sf)], stride)
            assert rc == 0, (sf, stride)
            five = []
            for r in range(5):
                rc, m = plan(lib, [(sf, 0, r, 1, 1, 0, 1, 0, 8)], stride)
                assert rc == 0
                five.append(m)
            assert t.sym_cap == max(m.sym_cap for m in five) and t.cw_cap == max(m.cw_cap for m in five), (sf, stride)
            assert t.lds_slice_bytes == max(m.lds_slice_bytes for m in five), (sf, stride)
            lanes = 8 if t.sym_cap <= 48 else 16 if t.sym_cap <= 96 else 32 if t.sym_cap <= 200 else 64
            assert t.lanes_per_packet == lanes == max(m.lanes_per_packet for m in five)
            assert t.packets_per_workgroup == min(256 // lanes, KIB160 // t.lds_slice_bytes) >= 1
            # the slice holds every rate's layout and the Gray-code load of up to sym_cap symbols
            assert t.lds_slice_bytes >= 2 * t.sym_cap
    assert [plan(lib, [hdr_cfg(7)], s)[1].lanes_per_packet for s in S.G_STRIDES] == [8, 16, 32, 64]


def test_plan_of_a_mixed_table_with_header_rate_entries(lib):
    others = [(7, 0, 1, 1, 1, 0, 1, 0, 8), (12, 0, 4, 1, 1, 0, 0, 0, 70), (9, 7, 2, 0, 0, 0, 1, 0, 8), (7, 5, 4, 1, 1, 0, 0, 0, 300)]
    for stride in STRIDES:
        for cfgs in ([hdr_cfg(sf) for sf in range(7, 13)], others + [hdr_cfg(8, 6), hdr_cfg(12)], [hdr_cfg(10)] + others):
            rc, t = plan(lib, cfgs, stride)
            assert rc == 0
            members = [plan(lib, [c], stride)[1] for c in cfgs]
            assert t.sym_cap == max(m.sym_cap for m in members) and t.cw_cap == max(m.cw_cap for m in members)
            assert t.lds_slice_bytes == max(m.lds_slice_bytes for m in members)
            assert t.lanes_per_packet == max(m.lanes_per_packet for m in members)
            assert t.packets_per_workgroup == min(256 // t.lanes_per_packet, KIB160 // t.lds_slice_bytes)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def refused_tables():
    ok = (7, 0, 1, 1, 1, 0, 1, 0, 8)
    return {"header rate without a header": [ok, (7, 0, -1, 1, 1, 0, 0, 0, 8)], "header rate without interleaving": [(7, 0, -1, 1, 0, 0, 1, 0, 8)],
            "rdd -2": [(7, 0, -2, 1, 1, 0, 1, 0, 8), ok]}


def test_every_entry_point_refuses_the_same_without_a_device(lib):
    """the plan refuses each table by its configuration check. The decode entry points are called here with a NULL context, which they refuse
    by itself before they read a configuration (the last lines show it): that every one of them reaches the same check with a real
    context is tests/test_gpu_header_rate.py::test_refusals_with_a_context_leave_the_outputs_untouched."""
    from lora_sdr_amd import _lib
    p = C.c_void_p(16)                                               # (never dereferenced: nothing is launched)
    ok = hdr_cfg(7)
    t = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
    assert plan(lib, [ok], 64)[0] == 0
    for name, cfgs in refused_tables().items():
        rc, t = plan(lib, cfgs, 64)
        assert rc == -1 and t.lanes_per_packet == 0, name
        arr = cfg_array(cfgs)
        for fn in (lib.lorahip_decode_packets_cfgs, lib.lorahip_decode_packets_cfgs_host):
            assert fn(None, arr, len(cfgs), p, None, 0, p, 64, p, 1, p, 144, p, p) == -1, name
        for fn in (lib.lorahip_decode_packets_info, lib.lorahip_decode_packets_info_host):
            assert fn(None, arr, len(cfgs), p, None, 0, p, 64, p, 1, p, 144, p, p, p) == -1, name
            assert fn(None, arr, len(cfgs), p, None, 0, p, 64, p, 1, p, 144, p, p, None) == -1, name
        bad = cfg_array([c for c in cfgs if c[2] < 0 and (c[2] < -1 or not (c[4] and c[6]))][:1])
        for fn in (lib.lorahip_decode_packets, lib.lorahip_decode_packets_host):
            assert fn(None, bad, p, 64, p, 1, p, 144, p, p) == -1, name
    for fn in (lib.lorahip_decode_packets_info, lib.lorahip_decode_packets_info_host):
        assert fn(None, cfg_array([ok, ok]), 2, None, None, 0, p, 64, p, 1, p, 144, p, p, p) == -1      # index NULL with two entries
        assert fn(None, cfg_array([ok]), 1, None, None, 0, p, 64, p, 1, p, 144, p, p, p) == -1           # (and a NULL context by itself)


def test_the_refusal_says_why(lib):
    """rdd = -1 without a header: refused by the configuration check every entry point shares, with the reason in lorahip_last_error"""
    rc, _ = plan(lib, [(7, 0, -1, 1, 1, 0, 0, 0, 8)], 64)
    assert rc == -1 and b"LORAHIP_RDD_FROM_HEADER" in lib.lorahip_last_error()


def test_python_surface_without_a_device():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    assert _lib.RDD_FROM_HEADER == -1 and C.sizeof(_lib.PacketInfo) == 32
    assert [n for n, _ in _lib.PacketInfo._fields_][:6] == list(H.FIELDS)
    d = L.LoRaDecoder.__new__(L.LoRaDecoder)
    d._cfg = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), 10, 0, 4, 0, 1, 0, 1, 0, 8)
    d.setCodingRate("header")
    assert d._cfg.rdd == -1
    for cr in ("4/4", "4/5", "4/6", "4/7", "4/8"):
        d.setCodingRate(cr)
        assert d._cfg.rdd == int(cr[2]) - 4
    for cr in ("4/9", "Header", "", "hdr"):
        with pytest.raises(ValueError):
            d.setCodingRate(cr)
    with pytest.raises(ValueError):                                  # the encoder's strings are the block's five: a frame is SENT at a rate
        L.LoRaEncoder.__new__(L.LoRaEncoder).setCodingRate("header")
    assert "header" not in L.LoRaEncoder._CR and sorted(L.LoRaEncoder._CR) == ["4/4", "4/5", "4/6", "4/7", "4/8"]
    d.setCodingRate("header")
    five = []
    for cr in ("4/4", "4/5", "4/6", "4/7", "4/8"):
        e = L.LoRaDecoder.__new__(L.LoRaDecoder)
        e._cfg = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), 10, 0, 4, 0, 1, 0, 1, 0, 8)
        e.setCodingRate(cr)
        five.append(L.LoRaDecoderSet.plan([e], 160))
    mine = L.LoRaDecoderSet.plan([d], 160)
    assert all(mine[k] == max(f[k] for f in five) for k in ("sym_cap", "cw_cap", "lds_slice_bytes", "lanes_per_packet"))
    d.enableExplicit(False)
    with pytest.raises(L.LoraHipError):
        L.LoRaDecoderSet.plan([d], 160)


def test_version_and_the_header_as_c(lib, tmp_path):
    """the ABI version stays 4 (additions only), and include/lorahip.h still compiles as C99 with the new struct at 32 bytes"""
    import shutil
    import subprocess
    from conftest import ROOT
    assert lib.lorahip_version() == 4
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "hdr.c"
    src.write_text(r'''
#include "lorahip.h"
typedef char info_is_32_bytes[sizeof(lorahip_packet_info) == 32 ? 1 : -1];
typedef char cfg_is_unchanged[sizeof(lorahip_decoder_cfg) == sizeof(size_t) + 9 * 4 + (sizeof(size_t) == 8 ? 4 : 0) ? 1 : -1];
int main(void)
{
    lorahip_decoder_cfg cfg = { sizeof(lorahip_decoder_cfg), 7, 0, LORAHIP_RDD_FROM_HEADER, 1, 1, 0, 1, 0, 8 };
    lorahip_packet_info info[1];
    int (*dev)(lorahip_ctx *, const lorahip_decoder_cfg *, size_t, const int32_t *, const int32_t *, size_t, const uint16_t *, size_t, const int32_t *,
               size_t, uint8_t *, size_t, int32_t *, int32_t *, lorahip_packet_info *) = lorahip_decode_packets_info;
    int (*host)(lorahip_ctx *, const lorahip_decoder_cfg *, size_t, const int32_t *, const int32_t *, size_t, const uint16_t *, size_t, const int32_t *,
                size_t, uint8_t *, size_t, int32_t *, int32_t *, lorahip_packet_info *) = lorahip_decode_packets_info_host;
    if (cfg.rdd != -1 || lorahip_version() != 4) return 10;
    if (dev(NULL, &cfg, 1, NULL, NULL, 0, NULL, 16, NULL, 0, NULL, 48, NULL, NULL, info) != LORAHIP_E_INVALID) return 11;
    if (host(NULL, &cfg, 1, NULL, NULL, 0, NULL, 16, NULL, 0, NULL, 48, NULL, NULL, info) != LORAHIP_E_INVALID) return 12;
    return 0;
}
''')
    exe = tmp_path / "hdr"
    from lora_sdr_amd import _lib
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-llorahip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
