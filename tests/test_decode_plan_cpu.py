"""CPU: what a decoder launch runs on (lorahip_decode_plan, host only -- the function the launches themselves call) held to the rules
include/lorahip.h states: lanes per packet by the largest sym_cap, the LDS slice from the caps, packets per workgroup from the slice; a
table's plan is the largest of its members'; and the argument errors of the plan and of lorahip_decode_packets_cfgs that need no device.

A configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr, data_length)."""
import ctypes as C
import itertools

import pytest

import codec_edge_inputs as S

KIB160 = 160 << 10
ROWS = S.G_STRIDES                                                   # 16, 64, 160, 512: the rows that select 8 / 16 / 32 / 64 lanes
HEADERS = [(1, 8), (0, 6), (0, 70), (0, 300), (0, 4096)]            # (explicit, data_length)
SINGLES = [(sf, 0, rdd, 1, 1, 0, explicit, 0, dlen) for sf in range(7, 13) for rdd in range(5) for explicit, dlen in HEADERS]


def cfg_array(cfgs):
    from lora_sdr_amd import _lib
    arr = (_lib.DecoderCfg * max(1, len(cfgs)))()
    for i, c in enumerate(cfgs):
        arr[i] = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), *c)
    return arr


def plan(lib, cfgs, stride):
    from lora_sdr_amd import _lib
    t = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
    rc = lib.lorahip_decode_plan(cfg_array(cfgs), len(cfgs), stride, C.byref(t))
    return rc, t


@pytest.fixture(scope="module")
def lib():
    import lora_sdr_amd as L
    return L.load()


@pytest.fixture(scope="module")
def single_plans(lib):
    """the plan of every single configuration at every row length, computed once: {(cfg, stride): DecodeTiling}"""
    out = {}
    for cfg, stride in itertools.product(SINGLES, ROWS):
        rc, t = plan(lib, [cfg], stride)
        assert rc == 0, (cfg, stride)
        out[cfg, stride] = t
    return out


def test_single_configuration_plans_keep_the_stated_rules(single_plans):
    seen = set()
    for (cfg, stride), t in single_plans.items():
        lanes = 8 if t.sym_cap <= 48 else 16 if t.sym_cap <= 96 else 32 if t.sym_cap <= 200 else 64
        assert t.lanes_per_packet == lanes, (cfg, stride, t.sym_cap)
        assert t.lds_slice_bytes == (t.sym_cap * 2 + 2 * t.cw_cap + 15) & ~15, (cfg, stride)
        assert t.packets_per_workgroup == min(256 // lanes, KIB160 // t.lds_slice_bytes) >= 1, (cfg, stride)
        assert t.reserved == 0 and t.struct_size == C.sizeof(type(t))
        # the restatement the decoder's edge tests select their inputs with says the same
        assert (t.lanes_per_packet, t.lds_slice_bytes, t.packets_per_workgroup) == S.launch_shape(cfg[0], cfg[1], cfg[2], cfg[6], cfg[8], stride), (cfg, stride)
        seen.add(lanes)
    assert seen == {8, 16, 32, 64}
    # the four rows are the ones that select the four lane counts with an explicit header (SF7 4/8)
    assert [single_plans[(7, 0, 4, 1, 1, 0, 1, 0, 8), r].lanes_per_packet for r in ROWS] == [8, 16, 32, 64]


def test_a_table_plan_is_the_largest_of_its_members(lib, single_plans):
    tables = [SINGLES[:30], SINGLES[::7], [SINGLES[3], SINGLES[3]], SINGLES[-64:], [c for c in SINGLES if c[8] != 4096][:64]]
    for cfgs in tables:
        assert 1 <= len(cfgs) <= 64
        for stride in ROWS:
            rc, t = plan(lib, cfgs, stride)
            assert rc == 0
            members = [single_plans[c, stride] for c in cfgs]
            assert t.sym_cap == max(m.sym_cap for m in members) and t.cw_cap == max(m.cw_cap for m in members)
            assert t.lds_slice_bytes == max(m.lds_slice_bytes for m in members)
            assert t.lanes_per_packet == max(m.lanes_per_packet for m in members)
            assert t.packets_per_workgroup == min(256 // t.lanes_per_packet, KIB160 // t.lds_slice_bytes)


def test_one_long_entry_costs_every_packet_of_the_table(lib):
    """an implicit-header entry with data_length 4096 in rows of 16384 symbols: fewer packets per workgroup than lane groups"""
    short = (7, 0, 1, 1, 1, 0, 1, 0, 8)
    long_ = (7, 5, 4, 1, 1, 0, 0, 0, 4096)
    rc, alone = plan(lib, [short], 16384)
    assert rc == 0 and alone.packets_per_workgroup == 256 // alone.lanes_per_packet
    rc, both = plan(lib, [short, long_, (12, 0, 4, 1, 1, 0, 0, 0, 6)], 16384)
    assert rc == 0 and both.lanes_per_packet == 64 and both.packets_per_workgroup == 3 < 256 // both.lanes_per_packet
    assert both.lds_slice_bytes == S.launch_shape(7, 5, 4, 0, 4096, 16384)[1]


def bad_tables():
    ok = (7, 0, 1, 1, 1, 0, 1, 0, 8)
    return {"sf 13": [ok, (13, 0, 1, 1, 1, 0, 1, 0, 8)], "data_length 4097": [(7, 0, 1, 1, 1, 0, 0, 0, 4097), ok],
            "rdd 5": [(7, 0, 5, 1, 1, 0, 1, 0, 8)], "ppm above sf": [ok, ok, (7, 8, 1, 1, 1, 0, 1, 0, 8)],
            "explicit header below 5 bits": [(7, 4, 1, 1, 1, 0, 1, 0, 8)], "negative data_length": [(7, 0, 1, 1, 1, 0, 0, 0, -1)]}


def test_plan_argument_errors(lib):
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    ok = (7, 0, 1, 1, 1, 0, 1, 0, 8)
    t = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 64, C.byref(t)) == 0 and t.lanes_per_packet == 16
    assert lib.lorahip_decode_plan(cfg_array([ok]), 0, 64, C.byref(t)) == -1 and t.lanes_per_packet == 0      # (a refusal zeroes the plan)
    assert lib.lorahip_decode_plan(cfg_array([ok] * 65), 65, 64, C.byref(t)) == -1
    assert lib.lorahip_decode_plan(cfg_array([ok] * 64), 64, 64, C.byref(t)) == 0
    assert lib.lorahip_decode_plan(None, 1, 64, C.byref(t)) == -1
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 64, None) == -1
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 0, C.byref(t)) == -1
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 16385, C.byref(t)) == -1
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 16384, C.byref(t)) == 0
    wrong = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling) - 4)
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 64, C.byref(wrong)) == -1
    stale = cfg_array([ok, ok])
    stale[1].struct_size -= 4
    assert lib.lorahip_decode_plan(stale, 2, 64, C.byref(t)) == -1 and lib.lorahip_decode_plan(stale, 1, 64, C.byref(t)) == 0
    for name, cfgs in bad_tables().items():
        assert plan(lib, cfgs, 64)[0] == -1, name
    # interleaving off reads no length: the same data_length is no error there, as in lorahip_decode_packets
    assert plan(lib, [(7, 0, 1, 1, 0, 0, 0, 0, 4097)], 64)[0] == 0
    # the Python surface: a dict of the tiling, LoraHipError where the library refuses
    d = L.LoRaDecoder.__new__(L.LoRaDecoder)
    d._cfg = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), *ok)
    p = L.LoRaDecoderSet.plan([d], 64)
    assert lib.lorahip_decode_plan(cfg_array([ok]), 1, 64, C.byref(t)) == 0
    assert p == dict(lanes_per_packet=16, sym_cap=t.sym_cap, cw_cap=t.cw_cap, lds_slice_bytes=t.lds_slice_bytes, packets_per_workgroup=16)
    with pytest.raises(L.LoraHipError):
        L.LoRaDecoderSet.plan([], 64)
    with pytest.raises(L.LoraHipError):
        L.LoRaDecoderSet.plan([d] * 65, 64)


def test_table_launch_refuses_the_same_before_a_device_is_touched(lib):
    """lorahip_decode_packets_cfgs with a NULL context: every refusal of the plan, and the launch's own, without a device"""
    ok = (7, 0, 1, 1, 1, 0, 1, 0, 8)
    p = C.c_void_p(16)                                               # (never dereferenced: nothing is launched)

    def call(fn, cfgs, n_cfgs, index=p, table=None, n_table=0, stride=64, n_packets=1, out_stride=144):
        return fn(None, cfgs, n_cfgs, index, table, n_table, p, stride, p, n_packets, p, out_stride, p, p)

    for fn in (lib.lorahip_decode_packets_cfgs, lib.lorahip_decode_packets_cfgs_host):
        assert call(fn, cfg_array([ok]), 0) == -1
        assert call(fn, cfg_array([ok] * 65), 65) == -1
        assert call(fn, None, 1) == -1
        for name, cfgs in bad_tables().items():
            assert call(fn, cfg_array(cfgs), len(cfgs)) == -1, name
        assert call(fn, cfg_array([ok]), 1, index=None) == -1
        assert call(fn, cfg_array([ok]), 1, table=p, n_table=0) == -1
        assert call(fn, cfg_array([ok]), 1, stride=16385, out_stride=2 * (16385 + 8)) == -1
        assert call(fn, cfg_array([ok]), 1, out_stride=2 * 64) == -1
        assert call(fn, cfg_array([ok]), 1, out_stride=145) == -1
        assert call(fn, cfg_array([ok]), 1) == -1                    # (and a NULL context by itself)
