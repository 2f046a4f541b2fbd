"""GPU: the batched decoder (lorahip_decode_packets: decodeGroup, the default, and the one-lane checker decodePackets) on crafted packets
-- tests/codec_def.py builds them, tests/codec_edge_inputs.py holds the sets, the CPU oracle's restated LoRaDecoder block says what comes out.
Everything is integer and exact: per packet the bytes, out_len (-1 nothing posted, -2 rows too short) and the dropped flag.

    set H  one body under all 4096 headers (256 lengths x crc flag x rate field 0..7): a header that contradicts the decoder's settings
    set E  one flipped bit in the codewords around the end of the range the reference decodes, and around the first block's end
    set G  E and the 16-symbol packets of H at rows that select 8 / 16 / 32 / 64 lanes per packet
    set R  rows shorter than their packet: decoded when the announced length fits the row, -2 when it does not
    set P  slices so long that three packets share a workgroup of four lane groups
    set B  packets per launch around a workgroup's 32, sentinel-filled outputs: every packet writes its own out_len bytes and nothing else

tests/test_codec_def_cpu.py checks without a GPU that every set holds the cases it is named for."""
import ctypes as C

import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as S

pytestmark = pytest.mark.gpu


def configure(dec, cfg):
    sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = cfg
    dec.setSpreadFactor(sf); dec.setSymbolSize(ppm); dec.setCodingRate(S.RDD_TO_CR[rdd]); dec.enableCrcc(crcc)
    dec.enableInterleaving(inter); dec.enableErrorCheck(ec); dec.enableExplicit(explicit); dec.enableHdr(hdr); dec.setDataLength(dlen)


@pytest.fixture(scope="module")
def dec(gpu):
    import lora_sdr_amd as L
    d = L.LoRaDecoder()
    yield d
    d._ctx.set_variant(0)


def launch(torch, dec, cfg, rows, nsyms, variant=0):
    """one lorahip_decode_packets launch through decode_batch -> host (out, out_len, dropped)"""
    dec._ctx.set_variant(variant)
    configure(dec, cfg)
    rows = np.array(rows, np.uint16)                                   # a copy: the sets are shared and read-only
    out, n, d = dec.decode_batch(torch.from_numpy(rows.view(np.int16)).cuda(), torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda())
    return out.cpu().numpy(), n.cpu().numpy(), d.cpu().numpy()


def assert_equals_table(got, table, tag):
    out, n, d = got
    want_n, want_d, want_b = S.table_arrays(table)
    bad = np.flatnonzero((n != want_n) | (d != want_d))
    assert bad.size == 0, (tag, "packet", int(bad[0]), "out_len", int(n[bad[0]]), int(want_n[bad[0]]), "dropped", int(d[bad[0]]), int(want_d[bad[0]]))
    width = want_b.shape[1]
    differs = (out[:, :width] != want_b) & (np.arange(width)[None, :] < want_n[:, None])
    bad = np.flatnonzero(differs.any(axis=1))
    assert bad.size == 0, (tag, "packet", int(bad[0]), "bytes", out[bad[0], :max(0, want_n[bad[0]])].tolist(), want_b[bad[0], :max(0, want_n[bad[0]])].tolist())


def same_results(a, b):
    """two launches gave the same out_len, dropped and bytes in [0, out_len)"""
    if not (np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])):
        return False
    w = min(a[0].shape[1], b[0].shape[1])
    assert int(a[1].max()) <= w
    live = np.arange(w)[None, :] < a[1][:, None]
    return bool(((a[0][:, :w] == b[0][:, :w]) | ~live).all())


# ---- set H ----------------------------------------------------------------------------------------------------------------------
FLAGS = [(hdr, crcc, ec) for hdr in (0, 1) for crcc in (0, 1) for ec in (0, 1)]


@pytest.mark.parametrize("sf,ppm,rdd", S.H_CONFIGS)
def test_set_h_every_header_vs_oracle(gpu, oracle, dec, sf, ppm, rdd):
    """4096 headers over one body per launch, the group kernel against the oracle: the rate taken from the header (fields 5..7 drop, the
    others decode the body's codewords as THAT code), the crc check cleared by the flag, lengths the packet cannot hold, the
    `dataLength -= 5` that goes below zero (nothing posted, no drop). hdr, crcc and error_check each off and on."""
    packets = S.set_h(sf, ppm, rdd)
    nsyms = np.full(packets.shape[0], packets.shape[1], np.int32)
    tables = {f: S.set_h_table(oracle, (sf, ppm, rdd, f[1], 1, f[2], 1, f[0], 8)) for f in FLAGS}
    S.check_set_h(tables)
    for (hdr, crcc, ec), table in tables.items():
        cfg = (sf, ppm, rdd, crcc, 1, ec, 1, hdr, 8)
        assert_equals_table(launch(gpu, dec, cfg, packets, nsyms), table, cfg)


@pytest.mark.parametrize("sf,ppm,rdd", S.H_CONFIGS)
def test_set_h_short_both_kernels_vs_oracle(gpu, oracle, dec, sf, ppm, rdd):
    """the same sweep over the lengths 0..16 on a body the one-lane checker can hold (at most 520 symbols): it and the group kernel
    against the oracle and against each other"""
    packets = S.set_h(sf, ppm, rdd, 16, 8)
    assert packets.shape[1] <= 520
    nsyms = np.full(packets.shape[0], packets.shape[1], np.int32)
    tables = {f: S.set_h_table(oracle, (sf, ppm, rdd, f[1], 1, f[2], 1, f[0], 8), 16, 8) for f in FLAGS}
    S.check_set_h(tables)
    for (hdr, crcc, ec), table in tables.items():
        cfg = (sf, ppm, rdd, crcc, 1, ec, 1, hdr, 8)
        got = [launch(gpu, dec, cfg, packets, nsyms, variant) for variant in (0, 1)]
        for variant in (0, 1):
            assert_equals_table(got[variant], table, (cfg, "variant", variant))
        assert same_results(got[0], got[1]), cfg


# ---- set E ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,ppm", S.E_SYMBOL_SIZES)
def test_set_e_damage_at_the_decode_boundary(gpu, oracle, dec, sf, ppm):
    """rates 4/5 .. 4/8, header on / off, crc on, a length whose decoded range ends with the first block (where that block is long
    enough) and one whose range ends behind it: every single bit of the codewords around both ends, of the header codewords and of
    the packet's last codeword, and two bits in one codeword. error_check off and on, both kernels == the oracle. The end of the
    decoded range is walked from the reference's loops (codec_def.decoded_end), and before anything is compared the oracle's own
    results must show the boundary: damage in the last decoded codeword is dropped, damage in the next one is not seen."""
    for group in S.e_groups():
        if group[:2] != (sf, ppm):
            continue
        packets, labels, c_end, _ = S.set_e(*group)
        nsyms = np.full(packets.shape[0], packets.shape[1], np.int32)
        S.check_set_e(labels, c_end, S.set_e_table(oracle, *group, 0), S.set_e_table(oracle, *group, 1))
        for ec in (0, 1):
            for variant in (0, 1):
                assert_equals_table(launch(gpu, dec, S.e_cfg(*group, ec), packets, nsyms, variant), S.set_e_table(oracle, *group, ec),
                                    (group, "error_check", ec, "variant", variant))


# ---- set G ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,ppm", S.E_SYMBOL_SIZES)
def test_set_g_every_lane_group_size_explicit(gpu, oracle, dec, sf, ppm):
    """The lanes per packet follow the slice a launch can need (lorahip_codec.hip: decodeCaps, launchDecode): with an explicit header
    that is min(what 260 bytes need, the row rounded up to blocks + 8), and the kernel takes 8 / 16 / 32 / 64 lanes up to 48 / 96 /
    200 / more symbols. A row of 16 symbols gives 40..44 at the five rates, 64 gives 88..92, 160 gives 184..190, 512 is past what 260
    bytes need (233 symbols or more; only SF12 at 4/4 stops at 188 and stays at 32 lanes) -- codec_edge_inputs.launch_shape restates
    this and test_codec_def_cpu.py asserts the four sizes from it. The group size cannot be observed; asserted is that the same
    packets, zero-padded to each row length, give the oracle's result at every one. Set E runs at the three rows that hold its
    packets (up to 64 symbols), the 16-symbol packets of set H at all four."""
    for group in S.e_groups():
        if group[:2] != (sf, ppm) or not group[3]:
            continue
        packets, _, _, _ = S.set_e(*group)
        results = []
        for stride in S.G_STRIDES[1:]:
            rows, nsyms = S.as_rows(packets, stride)
            results.append(launch(gpu, dec, S.e_cfg(*group, 1), rows, nsyms))
            assert_equals_table(results[-1], S.set_e_table(oracle, *group, 1), (group, "stride", stride))
        assert all(same_results(results[0], r) for r in results[1:]), group
    for rdd in range(5):
        packets = S.set_h(sf, ppm, rdd, 4, 2, 16)
        for hdr, crcc in ((0, 1), (1, 0)):
            cfg = (sf, ppm, rdd, crcc, 1, 1, 1, hdr, 8)
            table = S.set_h_table(oracle, cfg, 4, 2, 16)
            results = []
            for stride in S.G_STRIDES:
                rows, nsyms = S.as_rows(packets, stride)
                results.append(launch(gpu, dec, cfg, rows, nsyms))
                assert_equals_table(results[-1], table, (cfg, "stride", stride))
            assert all(same_results(results[0], r) for r in results[1:]), cfg


@pytest.mark.parametrize("sf,ppm,rdd", [(12, 0, 4), (7, 0, 1)])
def test_set_g_every_lane_group_size_implicit(gpu, oracle, dec, sf, ppm, rdd):
    """without a header the slice follows data_length: 6, 30, 70 and 300 bytes at rows of 512 symbols need 32 / 64 / 112 / 424 symbols at
    SF12 4/8 and 28 / 63 / 118 / 448 at SF7 4/5 -- 8, 16, 32 and 64 lanes. Set E's damage at each length, both error_check settings."""
    for length in (6, 30, 70, 300):
        packets, labels, c_end, _ = S.set_e(sf, ppm, rdd, 0, length)
        assert packets.shape[1] <= 512
        rows, nsyms = S.as_rows(packets, 512)
        S.check_set_e(labels, c_end, S.set_e_table(oracle, sf, ppm, rdd, 0, length, 0), S.set_e_table(oracle, sf, ppm, rdd, 0, length, 1))
        for ec in (0, 1):
            assert_equals_table(launch(gpu, dec, S.e_cfg(sf, ppm, rdd, 0, length, ec), rows, nsyms), S.set_e_table(oracle, sf, ppm, rdd, 0, length, ec),
                                (sf, ppm, rdd, length, ec))


# ---- set R ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,ppm", [(7, 0), (9, 7)])
def test_set_r_rows_shorter_than_the_packet(gpu, oracle, dec, sf, ppm):
    """explicit-header packets of 2, 9 and 40 bytes at 4/4, 4/6 and 4/8, two zero-nibble blocks longer than they need, in rows cut to
    exactly the whole interleaver blocks their announced bytes need (nsyms stays the packet's): the result is the oracle's on the
    FULL packet -- clean, and with one bit flipped in the last decoded codeword (dropped) and in the one behind it (decoded).
    One block fewer: out_len -2, not dropped. With interleaving off every symbol is output, so any nsyms > stride is -2; the one-lane
    checker refuses every nsyms > stride."""
    P = ppm or sf
    for rdd in (0, 2, 4):
        for length in (2, 9, 40):
            clean, cw = D.build(sf, np.random.default_rng(length).integers(0, 256, length).astype(np.uint8), ppm, rdd, True, True, n_blocks=2)
            c_end, _ = D.decoded_end(P, True, length + 5)
            need = D.num_symbols_def(-(-c_end // P) * P, P, rdd)
            assert 8 < need < clean.size
            packets = np.stack([clean, D.flip(clean, sf, ppm, rdd, c_end - 1, 0), D.flip(clean, sf, ppm, rdd, c_end, 0)])
            nsyms = np.full(3, clean.size, np.int32)
            cfg = (sf, ppm, rdd, 1, 1, 1, 1, 0, 8)
            table = S.oracle_table(oracle, cfg, packets)
            if rdd:
                assert [S.outcome(r) for r in table] == ["bytes", "dropped", "bytes"]
            assert_equals_table(launch(gpu, dec, cfg, packets[:, :need], nsyms), table, (cfg, length, "stride", need))
            _, n, d = launch(gpu, dec, cfg, packets[:, :need - (4 + rdd)], nsyms)
            assert n.tolist() == [-2] * 3 and d.tolist() == [0] * 3, (cfg, length)
            _, n, d = launch(gpu, dec, cfg, packets[:, :need], nsyms, variant=1)
            assert n.tolist() == [-2] * 3 and d.tolist() == [0] * 3, (cfg, length)
            _, n, d = launch(gpu, dec, (sf, ppm, rdd, 1, 0, 1, 1, 0, 8), packets[:, :need], nsyms)
            assert n.tolist() == [-2] * 3 and d.tolist() == [0] * 3, (cfg, length)


# ---- set P ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ppm", [5, 4, 2])
def test_set_p_fewer_packets_per_workgroup_than_lane_groups(gpu, oracle, dec, ppm):
    """SF7, no header, data_length 4096, crc, 4/8, rows of 16384 symbols: a packet's slice of LDS is 42752 / 49280 / 41072 bytes at PPM
    5 / 4 / 2, three fit the 160 KiB of a workgroup that has four groups of 64 lanes (launchDecodeGroup: perBlock = ldsMax / slice) --
    codec_edge_inputs.launch_shape. Seven rows (not a multiple of three), then one and four: each packet must come out of its own row
    into its own row. At PPM 5: five packets with different payloads, one with a payload byte changed behind the crc, one cut to 4000
    symbols. At PPM 4 and 2 a 4096-byte packet is longer than the longest row, the rows hold its first 16384 symbols and the reference
    drops every one -- and with the packet's true count in nsyms the rows are too short for the announced length: -2."""
    assert S.launch_shape(7, ppm, 4, 0, S.P_LENGTH, S.P_ROW)[2] == 3
    rows, nsyms = S.set_p(ppm)
    for ec in (0, 1):
        table = S.set_p_table(oracle, ppm, ec)
        for count in (7, 1, 4):
            assert_equals_table(launch(gpu, dec, S.p_cfg(ppm, ec), rows[:count], nsyms[:count]), table[:count], (ppm, ec, count))
    if ppm != 5:
        true_count = D.num_symbols_def(-(-2 * (S.P_LENGTH + 2) // ppm) * ppm, ppm, 4)
        assert true_count > S.P_ROW
        _, n, d = launch(gpu, dec, S.p_cfg(ppm, 0), rows[:5], np.full(5, true_count, np.int32))
        assert n.tolist() == [-2] * 5 and d.tolist() == [0] * 5


# ---- set B ----------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def sentinel_launch(torch, dec, cfg, rows, nsyms, out_stride, spare=3):
    """lorahip_decode_packets itself on outputs filled with 0xA5, `spare` more entries than packets in all three
    -> host (out (P + spare, out_stride) uint8, out_len, dropped)"""
    import lora_sdr_amd as L
    lib = L.load()
    configure(dec, cfg)
    P, stride = rows.shape
    syms = torch.from_numpy(np.array(rows, np.uint16).view(np.int16)).cuda()
    n_dev = torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda()
    out = torch.full((P + spare, out_stride), SENTINEL, dtype=torch.uint8, device="cuda")
    out_len = torch.full(((P + spare) * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    dropped = torch.full(((P + spare) * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    dec._ctx.use_torch_stream()
    rc = lib.lorahip_decode_packets(dec._ctx._h, C.byref(dec._cfg), C.c_void_p(syms.data_ptr()), stride, C.c_void_p(n_dev.data_ptr()), P,
                                    C.c_void_p(out.data_ptr()), out_stride, C.c_void_p(out_len.data_ptr()), C.c_void_p(dropped.data_ptr()))
    assert rc == 0, lib.lorahip_last_error()
    return out.cpu().numpy(), out_len.cpu().numpy().view(np.int32), dropped.cpu().numpy().view(np.int32)


def b_packets(count, seed):
    """`count` packets in rows of 16 symbols at SF7 4/8 (8 lanes per packet, 32 packets per workgroup), every one with bytes of its own,
    the outcomes in turn: bytes; dropped for its rate field; nothing posted (no crc flag, length 0); the first 16 symbols of a
    40-symbol packet whose 10 bytes need all 40 (-2); dropped for its crc; zero bytes posted (no crc flag, length 2); five symbols only (nothing posted whatever the
    settings).
    -> (rows, nsyms, packets as the oracle gets them, which are the -2 ones)"""
    rng = np.random.default_rng(seed)
    headers = [dict(), dict(hdr_rdd=6), dict(hdr_len=0, hdr_crc=0), None, dict(hdr_len=1), dict(hdr_crc=0), "cut"]
    rows, nsyms, packets, short = np.zeros((count, 16), np.uint16), np.zeros(count, np.int32), [], []
    for i in range(count):
        h = headers[i % len(headers)]
        if h is None:
            s, _ = D.build(7, rng.integers(0, 256, 10).astype(np.uint8), 0, 4, True, True)
            assert s.size == 40
            short.append(i)
        elif h == "cut":
            s = D.build(7, rng.integers(0, 256, 2).astype(np.uint8), 0, 4, True, True)[0][:5]
        else:
            s, _ = D.build(7, rng.integers(0, 256, 2).astype(np.uint8), 0, 4, True, True, **h)
            assert s.size == 16
        rows[i, :min(16, s.size)], nsyms[i] = s[:16], s.size
        packets.append(s)
    return rows, nsyms, packets, short


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("count", [1, 31, 32, 33, 65])
def test_set_b_placement_and_containment(gpu, oracle, dec, count, variant):
    """outputs pre-filled with 0xA5, out_stride (96) larger than needed (48): row p holds packet p's oracle bytes in [0, out_len) and the
    sentinel behind them -- in every byte where nothing is posted --, and the entries behind n_packets are untouched in out, out_len
    and dropped. hdr off and on (the header bytes in front make every posted length differ)."""
    dec._ctx.set_variant(variant)
    rows, nsyms, packets, short = b_packets(count, 7 * count)
    for hdr in (0, 1):
        cfg = (7, 0, 4, 1, 1, 1, 1, hdr, 8)
        table = S.oracle_table(oracle, cfg, packets)
        for i in short:
            assert table[i][0] is not None                          # the whole packet decodes; its row is too short
            table[i] = (None, 0)
        if count >= 7:
            assert {S.outcome(r) for r in table} == {"bytes", "dropped", "nothing"}
        out, n, d = sentinel_launch(gpu, dec, cfg, rows, nsyms, 96)
        want_n, want_d, _ = S.table_arrays(table)
        want_n[short] = -2
        assert np.array_equal(n[:count], want_n) and np.array_equal(d[:count], want_d), (count, hdr, n[:count].tolist(), want_n.tolist())
        for i in range(count):
            k = max(0, int(want_n[i]))
            assert k == 0 or np.array_equal(out[i, :k], table[i][0]), (count, hdr, i)
            assert (out[i, k:] == SENTINEL).all(), (count, hdr, i, "written behind out_len")
        assert (out[count:] == SENTINEL).all() and (n[count:].view(np.uint8) == SENTINEL).all() and (d[count:].view(np.uint8) == SENTINEL).all()


@pytest.mark.parametrize("variant", [0, 1])
def test_set_b_containment_with_interleaving_off(gpu, oracle, dec, variant):
    """interleaving off posts the Gray-coded symbols, out_len counts uint16: row p is written in [0, 2 * out_len) bytes only. Symbol
    counts below 8 (nothing), 8, 13 and 16 (rounded up to blocks of 8), 17 in a row of 16 (-2); 33 packets."""
    dec._ctx.set_variant(variant)
    rng = np.random.default_rng(9)
    counts = [(5, 8, 13, 16, 17, 0, 12)[i % 7] for i in range(33)]
    rows = rng.integers(0, 128, (33, 16)).astype(np.uint16)
    cfg = (7, 5, 4, 0, 0, 0, 1, 0, 8)
    out, n, d = sentinel_launch(gpu, dec, cfg, rows, np.array(counts, np.int32), 64)
    for i, c in enumerate(counts):
        if c > 16:
            assert n[i] == -2 and d[i] == 0 and (out[i] == SENTINEL).all(), i
            continue
        o, dr = oracle.decode(7, rows[i, :c], ppm=5, cr="4/8", interleaving=False)
        assert d[i] == dr == 0 and n[i] == (-1 if o is None else o.size), (i, c)
        k = 0 if o is None else 2 * o.size
        assert np.array_equal(out[i, :k].view(np.uint16), o if o is not None else np.zeros(0, np.uint16)), (i, c)
        assert (out[i, k:] == SENTINEL).all(), (i, c, "written behind 2 * out_len")
    assert (out[33:] == SENTINEL).all() and (n[33:].view(np.uint8) == SENTINEL).all() and (d[33:].view(np.uint8) == SENTINEL).all()
