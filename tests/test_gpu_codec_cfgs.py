"""GPU: the decoder launch whose packets each pick their configuration from a table (lorahip_decode_packets_cfgs: decodeGroupCfgs, and the
one-lane checker decodePacketsCfgs as context variant 1). Per packet it is the reference's LoRaDecoder::work() under that packet's
settings: every row is compared with the CPU oracle under its own configuration, and -- every byte of the output row, the 0xA5 the
outputs are pre-filled with included -- with what lorahip_decode_packets gives that configuration's packets in a uniform launch.
Everything is integer and exact.

    set 1  600 packets with random configurations out of a table of 30 (SF 7..12 x rate 4/4..4/8) and out of one that varies the symbol
           size, hdr, crcc, error_check and implicit lengths; half of them damaged
    set 2  neighbours that differ as much as they can (SF7 4/4 8 symbols | SF12 4/8 as long as the row holds), the boundary at every
           group position of a wavefront, packet counts round a workgroup's share, the four rows that select 8 / 16 / 32 / 64 lanes
    set 3  an entry whose LDS slice is 42 KiB beside two small ones: three packets per workgroup, each laid out by its own entry
    set 4  interleaving on and off in one launch
    set 5  indices without an entry (-3), the table_dev form
    set 6  a table of one entry == the uniform entry point on the golden vectors
    set 7  the _host form == the device form

A decoder configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr,
data_length). Rows are 16, 64, 160 or 512 symbols (set G of test_gpu_decoder_edges.py) except set 3's 16384."""
import ctypes as C

import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def cfg_array(cfgs):
    from lora_sdr_amd import _lib
    arr = (_lib.DecoderCfg * len(cfgs))()
    for i, c in enumerate(cfgs):
        arr[i] = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), *c)
    return arr


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as L
    c = L.Context(7)                                                 # device and stream only
    yield c
    c.set_variant(0)


def _outputs(torch, P, out_stride):
    return (torch.full((P, out_stride), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((P,), -77, dtype=torch.int32, device="cuda"),
            torch.full((P,), -77, dtype=torch.int32, device="cuda"))


def _host(out, n, d):
    return out.cpu().numpy(), n.cpu().numpy(), d.cpu().numpy()


def table_launch(torch, ctx, cfgs, rows, nsyms, index, table=None, variant=0, out_stride=None):
    """lorahip_decode_packets_cfgs on outputs filled with 0xA5 -> host (out (P, out_stride), out_len, dropped)"""
    rows = np.array(rows, np.uint16)
    P, stride = rows.shape
    out_stride = out_stride or 2 * (stride + 8)
    syms = torch.from_numpy(rows.view(np.int16)).cuda()
    n_dev = torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda()
    i_dev = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    t_dev = None if table is None else torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda()
    out, n, d = _outputs(torch, P, out_stride)
    ctx.set_variant(variant); ctx.use_torch_stream()
    rc = ctx._lib.lorahip_decode_packets_cfgs(ctx._h, cfg_array(cfgs), len(cfgs), C.c_void_p(i_dev.data_ptr()),
                                              None if t_dev is None else C.c_void_p(t_dev.data_ptr()), 0 if t_dev is None else t_dev.numel(),
                                              C.c_void_p(syms.data_ptr()), stride, C.c_void_p(n_dev.data_ptr()), P, C.c_void_p(out.data_ptr()), out_stride,
                                              C.c_void_p(n.data_ptr()), C.c_void_p(d.data_ptr()))
    assert rc == 0, ctx._lib.lorahip_last_error()
    return _host(out, n, d)


def uniform_launch(torch, ctx, cfg, rows, nsyms, variant=0, out_stride=None):
    """lorahip_decode_packets on the same kind of outputs"""
    rows = np.array(rows, np.uint16)
    P, stride = rows.shape
    out_stride = out_stride or 2 * (stride + 8)
    syms = torch.from_numpy(rows.view(np.int16)).cuda()
    n_dev = torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda()
    out, n, d = _outputs(torch, P, out_stride)
    ctx.set_variant(variant); ctx.use_torch_stream()
    rc = ctx._lib.lorahip_decode_packets(ctx._h, cfg_array([cfg]), C.c_void_p(syms.data_ptr()), stride, C.c_void_p(n_dev.data_ptr()), P,
                                         C.c_void_p(out.data_ptr()), out_stride, C.c_void_p(n.data_ptr()), C.c_void_p(d.data_ptr()))
    assert rc == 0, ctx._lib.lorahip_last_error()
    return _host(out, n, d)


def uniform_by_configuration(torch, ctx, cfgs, rows, nsyms, index, variant=0, out_stride=None):
    """the rows bucketed by configuration, one lorahip_decode_packets launch per bucket, scattered back to the rows' order"""
    rows, nsyms, index = np.asarray(rows), np.asarray(nsyms), np.asarray(index)
    out_stride = out_stride or 2 * (rows.shape[1] + 8)
    out = np.full((rows.shape[0], out_stride), SENTINEL, np.uint8)
    n, d = np.full(rows.shape[0], -77, np.int32), np.full(rows.shape[0], -77, np.int32)
    for i in np.unique(index).tolist():
        sel = np.flatnonzero(index == i)
        out[sel], n[sel], d[sel] = uniform_launch(torch, ctx, cfgs[i], rows[sel], nsyms[sel], variant, out_stride)
    return out, n, d


def assert_rows_equal_oracle(got, cfgs, index, table, tag, short=()):
    """out_len, dropped and the bytes in front of out_len are the oracle's under each row's configuration (rows in `short`: -2), and
    nothing is written behind out_len -- behind 2 * out_len where the row's configuration has interleaving off"""
    out, n, d = got
    want_n, want_d, _ = S.table_arrays(table)
    want_n[list(short)] = -2
    bad = np.flatnonzero((n != want_n) | (d != want_d))
    assert bad.size == 0, (tag, "packet", int(bad[0]), cfgs[index[bad[0]]], "out_len", int(n[bad[0]]), int(want_n[bad[0]]), "dropped", int(d[bad[0]]), int(want_d[bad[0]]))
    for i, (o, _) in enumerate(table):
        k = max(0, int(want_n[i])) * (1 if cfgs[index[i]][4] else 2)
        if k:
            assert np.array_equal(out[i, :k], np.ascontiguousarray(o).view(np.uint8)), (tag, "packet", i, cfgs[index[i]])
        assert (out[i, k:] == SENTINEL).all(), (tag, "packet", i, cfgs[index[i]], "written behind out_len")


def assert_same_launch(a, b, tag):
    """two launches left the same bytes in every output row, and the same out_len and dropped"""
    for x, y, what in zip(a, b, ("out", "out_len", "dropped")):
        bad = np.flatnonzero((x != y).reshape(x.shape[0], -1).any(axis=1))
        assert bad.size == 0, (tag, what, "packet", int(bad[0]))


def oracle_rows(oracle, cfgs, packets, index):
    return [S.oracle_table(oracle, cfgs[i], [s])[0] for s, i in zip(packets, index)]


# ---- set 1 ----------------------------------------------------------------------------------------------------------------------
TABLE_A = [(sf, 0, rdd, 1, 1, 0, 1, 0, 8) for sf in range(7, 13) for rdd in range(5)]
# symbol size sf and sf - 2; header in the output or not, no header with 6 and with 30 bytes; crcc with error_check off and the reverse
TABLE_B = [(sf, ppm, (sf + k + m) % 5, crcc, 1, ec, explicit, hdr, dlen)
           for sf in (7, 10, 12) for k, ppm in enumerate((0, sf - 2))
           for m, (explicit, hdr, dlen) in enumerate(((1, 0, 8), (1, 1, 8), (0, 0, 6), (0, 0, 30))) for crcc, ec in ((1, 0), (0, 1))]
SET1_ROW = 160


def encode(L, cfg, payloads):
    sf, ppm, rdd, crcc, _, _, explicit, _, _ = cfg
    enc = L.LoRaEncoder()
    enc.setSpreadFactor(sf); enc.setSymbolSize(ppm); enc.setCodingRate(S.RDD_TO_CR[rdd]); enc.enableExplicit(bool(explicit))
    enc.enableCrc(bool(explicit or crcc))                           # (without a header the decoder's crcc says whether two crc bytes follow)
    return enc.work(payloads)


def build_set1(cfgs, seed):
    """600 packets: random entries of `cfgs`, payloads of 1..40 bytes (the entry's data_length without a header) from the encoder under the
    entry's settings, every second one with one or two flipped symbol bits -> (rows (600, 160), nsyms, index, packets)"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(seed)
    index = rng.integers(0, len(cfgs), 600)
    packets = [None] * 600
    for i in np.unique(index).tolist():
        sel = np.flatnonzero(index == i)
        lengths = rng.integers(1, 41, sel.size) if cfgs[i][6] else np.full(sel.size, cfgs[i][8])
        for p, s in zip(sel.tolist(), encode(L, cfgs[i], [rng.integers(0, 256, int(n)).astype(np.uint8) for n in lengths])):
            packets[p] = np.array(s, np.uint16)
    for p in range(0, 600, 2):
        for _ in range(int(rng.integers(1, 3))):
            packets[p][int(rng.integers(0, packets[p].size))] ^= np.uint16(1 << int(rng.integers(0, cfgs[index[p]][0])))
    assert max(s.size for s in packets) <= SET1_ROW
    rows, nsyms = S.as_rows(packets, SET1_ROW)
    return rows, nsyms, index.astype(np.int32), packets


@pytest.fixture(scope="module")
def set1(gpu, oracle):
    """both tables' packets and what the oracle says about each, computed once"""
    out = {}
    for name, cfgs, seed in (("A", TABLE_A, 11), ("B", TABLE_B, 12)):
        rows, nsyms, index, packets = build_set1(cfgs, seed)
        table = oracle_rows(oracle, cfgs, packets, index)
        kinds = [S.outcome(r) for r in table]
        assert kinds.count("bytes") > 300 and kinds.count("dropped") > 20, (name, kinds.count("bytes"), kinds.count("dropped"))
        assert np.unique(index).size == len(cfgs)
        out[name] = (cfgs, rows, nsyms, index, table)
    return out


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_set1_every_packet_under_its_own_settings(gpu, ctx, set1, name, variant):
    assert len(TABLE_A) == 30 and len(TABLE_B) == 48 and len(set(TABLE_B)) == 48
    cfgs, rows, nsyms, index, table = set1[name]
    got = table_launch(gpu, ctx, cfgs, rows, nsyms, index, variant=variant)
    assert_rows_equal_oracle(got, cfgs, index, table, (name, variant))
    assert_same_launch(got, uniform_by_configuration(gpu, ctx, cfgs, rows, nsyms, index, variant), (name, variant))


def test_set1_both_kernels_agree(gpu, ctx, set1):
    for name in ("A", "B"):
        cfgs, rows, nsyms, index, _ = set1[name]
        assert_same_launch(table_launch(gpu, ctx, cfgs, rows, nsyms, index, variant=0), table_launch(gpu, ctx, cfgs, rows, nsyms, index, variant=1), name)


# ---- set 2 ----------------------------------------------------------------------------------------------------------------------
SMALL, LARGE = (7, 0, 0, 1, 1, 1, 1, 1, 8), (12, 0, 4, 1, 1, 1, 1, 0, 8)      # (SMALL with the header bytes in the output: one payload byte without a crc posts nothing otherwise)
COUNTS = (1, 31, 32, 33, 65)


def neighbours(stride, run, seed):
    """65 packets in runs of `run`: SF7 4/4 with a one-byte payload and no crc (8 symbols), then SF12 4/8 with the longest payload whose
    packet the row holds (at most 255 bytes); every fifth packet has one bit flipped in its last payload codeword"""
    rng = np.random.default_rng(seed)
    blocks = (stride - 8) // 8 + 1
    long_len = min(255, (12 * blocks - 5) // 2 - 2)
    packets, index = [], []
    for p in range(65):
        large = (p // run) & 1
        if large:
            s, cw = D.build(12, rng.integers(0, 256, long_len).astype(np.uint8), 0, 4, True, True)
            last = 5 + 2 * (long_len + 2) - 1
        else:
            s, cw = D.build(7, rng.integers(0, 256, 1).astype(np.uint8), 0, 0, True, False)
            last = 6
            assert s.size == 8
        if p % 5 == 4:
            s = D.flip(s, LARGE[0] if large else SMALL[0], 0, 4 if large else 0, last, 1)
        assert s.size <= stride and (not large or s.size + 8 > stride or long_len == 255)
        packets.append(s); index.append(large)
    return packets, np.array(index, np.int32)


@pytest.mark.parametrize("stride", S.G_STRIDES)
def test_set2_neighbours_that_differ_as_much_as_they_can(gpu, oracle, ctx, stride):
    """the lanes of one wavefront hold 8 / 4 / 2 / 1 packets whose symbol size, block size, codeword count and every trip count differ;
    256 / G packets share a workgroup and its barriers. Counts round that share, the boundary between the two kinds at every run length."""
    from test_decode_plan_cpu import plan
    import lora_sdr_amd as L
    rc, t = plan(L.load(), [SMALL, LARGE], stride)
    assert rc == 0 and t.lanes_per_packet == {16: 8, 64: 16, 160: 32, 512: 64}[stride] and t.packets_per_workgroup == 256 // t.lanes_per_packet
    for run in (1, 2, 4, 8):
        packets, index = neighbours(stride, run, 100 * stride + run)
        table = oracle_rows(oracle, [SMALL, LARGE], packets, index)
        assert {(int(i), S.outcome(r)) for i, r in zip(index, table)} == {(0, "bytes"), (0, "dropped"), (1, "bytes"), (1, "dropped")}
        rows, nsyms = S.as_rows(packets, stride)
        for count in COUNTS:
            for variant in (0, 1):
                got = table_launch(gpu, ctx, [SMALL, LARGE], rows[:count], nsyms[:count], index[:count], variant=variant)
                assert_rows_equal_oracle(got, [SMALL, LARGE], index[:count], table[:count], (stride, run, count, variant))


# ---- set 3 ----------------------------------------------------------------------------------------------------------------------
def test_set3_every_group_lays_out_its_slice_by_its_own_entry(gpu, oracle, ctx):
    """{explicit SF7 4/5, no header SF7 PPM 5 4/8 data_length 4096, no header SF12 4/8 data_length 6} in rows of 16384 symbols: the slice is
    the long entry's 42752 bytes, three packets per workgroup of four lane groups; seven packets that mix all three."""
    from test_decode_plan_cpu import plan
    import lora_sdr_amd as L
    cfgs = [(7, 0, 1, 1, 1, 1, 1, 0, 8), S.p_cfg(5, 1), (12, 0, 4, 1, 1, 1, 0, 0, 6)]
    rc, t = plan(L.load(), cfgs, S.P_ROW)
    assert rc == 0 and t.packets_per_workgroup == 3 and t.lanes_per_packet == 64 and t.lds_slice_bytes == 42752
    rng = np.random.default_rng(3)
    long_rows, long_n = S.set_p(5)
    index = np.array([0, 1, 2, 1, 0, 2, 1], np.int32)
    rows, nsyms = np.zeros((7, S.P_ROW), np.uint16), np.zeros(7, np.int32)
    for p, i in enumerate(index.tolist()):
        if i == 1:
            rows[p], nsyms[p] = long_rows[p], long_n[p]             # (row 5: a wrong crc, row 6: cut to 4000 symbols -- p = 1, 3, 6: two good ones and the cut one)
        else:
            s, _ = D.build(cfgs[i][0], rng.integers(0, 256, 17 if i == 0 else 6).astype(np.uint8), 0, cfgs[i][2], bool(cfgs[i][6]), True)
            if p == 4:
                s = D.flip(s, 7, 0, 1, 20, 0)                        # a parity error behind the first block: dropped with error_check
            rows[p, :s.size], nsyms[p] = s, s.size
    table = oracle_rows(oracle, cfgs, [rows[p, :nsyms[p]] for p in range(7)], index)
    assert [S.outcome(r) for r in table] == ["bytes", "bytes", "bytes", "bytes", "dropped", "bytes", "dropped"]
    got = table_launch(gpu, ctx, cfgs, rows, nsyms, index)
    assert_rows_equal_oracle(got, cfgs, index, table, "set 3")
    assert_same_launch(got, uniform_by_configuration(gpu, ctx, cfgs, rows, nsyms, index), "set 3")


# ---- set 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set4_interleaving_on_and_off_in_one_launch(gpu, oracle, ctx, variant):
    """rows of 16 symbols: the rows of the entry without interleaving post their Gray-coded symbols as uint16 (5, 8, 13, 16 and 12 of them, and
    17 in a row of 16: -2), the others their bytes; 33 packets, the two kinds in turn"""
    cfgs = [(7, 5, 4, 0, 0, 0, 1, 0, 8), (7, 0, 4, 1, 1, 1, 1, 0, 8)]
    rng = np.random.default_rng(4)
    counts = (5, 8, 13, 16, 17, 12)
    rows, nsyms, index, packets, short = np.zeros((33, 16), np.uint16), np.zeros(33, np.int32), np.zeros(33, np.int32), [], []
    for p in range(33):
        index[p] = p & 1
        if index[p]:
            s, _ = D.build(7, rng.integers(0, 256, 2).astype(np.uint8), 0, 4, True, True)
            assert s.size == 16
            rows[p], nsyms[p] = s, 16
            packets.append(s)
        else:
            c = counts[(p // 2) % len(counts)]
            rows[p] = rng.integers(0, 128, 16)
            nsyms[p] = c
            packets.append(rows[p, :min(c, 16)].copy())
            if c > 16:
                short.append(p)
    table = oracle_rows(oracle, cfgs, packets, index)
    assert len(short) == 3
    got = table_launch(gpu, ctx, cfgs, rows, nsyms, index, variant=variant)
    assert_rows_equal_oracle(got, cfgs, index, table, ("set 4", variant), short=short)
    assert np.flatnonzero(got[1] == -2).tolist() == short
    assert_same_launch(got, uniform_by_configuration(gpu, ctx, cfgs, rows, nsyms, index, variant), ("set 4", variant))


# ---- set 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set5_indices_without_an_entry(gpu, oracle, ctx, variant):
    """-1, n_cfgs and 2^31 - 1 give -3, dropped 0 and an untouched row; the table_dev form gives what the direct form gives, an index outside
    the table -3"""
    cfgs = [SMALL, LARGE, (9, 7, 2, 1, 1, 0, 1, 1, 8)]
    packets, index = neighbours(64, 1, 5)
    packets, index = packets[:40], index[:40].copy()
    rows, nsyms = S.as_rows(packets, 64)
    table = oracle_rows(oracle, cfgs, packets, index)
    bad = {3: -1, 8: len(cfgs), 9: 2 ** 31 - 1, 17: -2 ** 31, 33: 64, 39: 3}
    direct = index.copy()
    for p, v in bad.items():
        direct[p] = v
    out, n, d = table_launch(gpu, ctx, cfgs, rows, nsyms, direct, variant=variant)
    good = np.array([p for p in range(40) if p not in bad])
    for p in bad:
        assert n[p] == -3 and d[p] == 0 and (out[p] == SENTINEL).all(), (p, bad[p])
    assert_rows_equal_oracle((out[good], n[good], d[good]), cfgs, index[good], [table[p] for p in good], ("direct", variant))
    # channels 0..119 with configuration c % 3 -- and channel 7 with one the table does not have; packet p comes from channel 3 p + its entry
    cfg_of_channel = (np.arange(120) % 3).astype(np.int32)
    cfg_of_channel[7] = 5
    channel = (3 * np.arange(40) + index).astype(np.int32)
    assert channel.max() < 120 and 7 not in channel
    outside = {2: 120, 11: -1, 20: 2 ** 31 - 1, 30: 7}
    for p, v in outside.items():
        channel[p] = v
    got = table_launch(gpu, ctx, cfgs, rows, nsyms, channel, table=cfg_of_channel, variant=variant)
    want = index.copy()
    want[list(outside)] = -1
    assert_same_launch(got, table_launch(gpu, ctx, cfgs, rows, nsyms, want, variant=variant), ("table", variant))
    assert all(got[1][p] == -3 and (got[0][p] == SENTINEL).all() for p in outside)
    good = np.array([p for p in range(40) if p not in outside])
    assert_rows_equal_oracle(tuple(x[good] for x in got), cfgs, index[good], [table[p] for p in good], ("table", variant))


# ---- set 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set6_one_entry_equals_the_uniform_entry_point_on_the_golden_vectors(gpu, golden, ctx, variant):
    g = golden("codec_kat.npz")
    groups = {}
    for i in range(int(g["count"])):
        groups.setdefault(tuple(int(v) for v in g["cfg_%d" % i]), []).append(i)
    checked = 0
    for cfg, idx in groups.items():
        packets = [np.asarray(g["syms_%d" % i]).astype(np.uint16) for i in idx]
        rows, nsyms = S.as_rows(packets, max(8, max(s.size for s in packets)))
        got = table_launch(gpu, ctx, [cfg], rows, nsyms, np.zeros(len(idx), np.int32), variant=variant)
        assert_same_launch(got, uniform_launch(gpu, ctx, cfg, rows, nsyms, variant), (cfg, variant))
        for p, i in enumerate(idx):
            n, drp, _ = (int(v) for v in g["res_%d" % i])
            assert got[1][p] == n and got[2][p] == drp, (cfg, i)
            if n > 0:
                assert np.array_equal(got[0][p, :n * (1 if cfg[4] else 2)], np.ascontiguousarray(g["out_%d" % i]).view(np.uint8)), (cfg, i)
            checked += 1
    assert checked == int(g["count"])


# ---- set 7 ----------------------------------------------------------------------------------------------------------------------
def test_set7_the_host_form_equals_the_device_form(gpu, ctx, set1):
    for name in ("A", "B"):
        cfgs, rows, nsyms, index, _ = set1[name]
        index = index.copy()
        index[5] = len(cfgs)                                         # (a row without an entry stays as the caller had it)
        dev = table_launch(gpu, ctx, cfgs, rows, nsyms, index)
        P, stride = rows.shape
        out_stride = 2 * (stride + 8)
        for table in (None, np.arange(len(cfgs) + 1, dtype=np.int32)):
            out, n, d = np.full((P, out_stride), SENTINEL, np.uint8), np.full(P, -77, np.int32), np.full(P, -77, np.int32)
            syms = np.array(rows, np.uint16)
            ctx.set_variant(0); ctx.use_torch_stream()
            rc = ctx._lib.lorahip_decode_packets_cfgs_host(ctx._h, cfg_array(cfgs), len(cfgs), index.ctypes.data, None if table is None else table.ctypes.data,
                                                           0 if table is None else table.size, syms.ctypes.data, stride, nsyms.ctypes.data, P, out.ctypes.data,
                                                           out_stride, n.ctypes.data, d.ctypes.data)
            assert rc == 0, ctx._lib.lorahip_last_error()
            assert_same_launch((out, n, d), dev, (name, "host", table is not None))
        assert dev[1][5] == -3


def test_decoder_set_python_surface(gpu, oracle, set1):
    """LoRaDecoderSet: decode_batch == the raw launch, work() the host-list form (None where nothing is posted, the dropped count), and the
    errors for a packet without a decoder and one that does not fit its row"""
    import lora_sdr_amd as L
    from test_gpu_decoder_edges import configure
    cfgs, rows, nsyms, index, table = set1["B"]
    decs = []
    for c in cfgs:
        d = L.LoRaDecoder(); configure(d, c); decs.append(d)
    ds = L.LoRaDecoderSet(decs)
    decs[0].setSpreadFactor(9)                                       # (copied at construction: not seen by the set)
    packets = [rows[p, :nsyms[p]] for p in range(100)]
    res = ds.work(packets, index[:100])
    for p, (o, dr) in enumerate(table[:100]):
        assert (o is None) == (res[p] is None) and (o is None or np.array_equal(o, res[p])), p
    assert ds.getDropped() == sum(dr for _, dr in table[:100]) > 0
    ds.activate()
    assert ds.getDropped() == 0 and ds.work([], []) == []
    with pytest.raises(ValueError):
        ds.work(packets[:3], [0, len(cfgs), 1])
    with pytest.raises(ValueError):
        ds.work(packets[:3], [0, 1])
    out, n, d = ds.decode_batch(gpu.from_numpy(np.array(rows, np.uint16).view(np.int16)).cuda(), gpu.from_numpy(nsyms).cuda(), gpu.from_numpy(index).cuda())
    want_n, want_d, _ = S.table_arrays(table)
    assert np.array_equal(n.cpu().numpy(), want_n) and np.array_equal(d.cpu().numpy(), want_d)
    with pytest.raises(ValueError):
        L.LoRaDecoderSet([])
    with pytest.raises(ValueError):
        L.LoRaDecoderSet(decs + decs)
