"""GPU: the decoder that takes each packet's coding rate from its explicit header (rdd = LORAHIP_RDD_FROM_HEADER) and reports what the
header and the checksum say (lorahip_decode_packets_info), in both kernels: decodeGroup / decodeGroupCfgs at 8, 16, 32 and 64 lanes per
packet, and the one-lane checker (context variant 1). The definition under test: a packet under an entry with rdd = -1 gives exactly --
every byte of the output row, the 0xA5 the outputs are pre-filled with included -- what lorahip_decode_packets gives it under the same
entry with the rate its header names; and that is what the CPU oracle gives under that rate. The report equals tests/codec_hdr_def.py,
which tests/test_header_rate_cpu.py pins to the reference. Everything is integer and exact.

    set 1  600 encoder-made packets over SF 7..12 x rate 4/4..4/8, half of them damaged, through six entries (sf, rdd = -1)
    set 2  every rate field, both crc flags, lengths 0 / 1 / 2 / 20 / 255 as headers on bodies coded at ANOTHER rate; crcc and error_check
    set 3  rows that hold exactly the blocks a length needs, one block fewer (-2), and a packet longer than its row
    set 4  header-rate, fixed-rate, implicit-header and interleaving-off entries in one launch; indices without an entry; table_dev
    set 5  1 / 31 / 32 / 33 / 65 packets, neighbours under different entries across the workgroup boundary
    set 6  the report; info_dev = NULL; nothing written behind n_packets
    set 7  lorahip_decode_packets with rdd = -1 == a table of one entry; the _host form == the device form

A configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr, data_length)."""
import ctypes as C

import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as S
import codec_hdr_def as H
import test_gpu_codec_cfgs as T
from test_decode_plan_cpu import plan

pytestmark = pytest.mark.gpu

SENTINEL = T.SENTINEL
INFO_FILL = -1234567


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as L
    c = L.Context(7)                                                 # device and stream only
    yield c
    c.set_variant(0)


def info_launch(torch, ctx, cfgs, rows, nsyms, index, table=None, variant=0, info=True, slack=3):
    """lorahip_decode_packets_info on outputs filled with 0xA5 and a report array of P + slack rows filled with INFO_FILL
    -> host (out, out_len, dropped), report (P + slack, 8) or None. index None: the one-entry form without an index."""
    rows = np.array(rows, np.uint16)
    P, stride = rows.shape
    out_stride = 2 * (stride + 8)
    syms = torch.from_numpy(rows.view(np.int16)).cuda()
    n_dev = torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda()
    i_dev = None if index is None else torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    t_dev = None if table is None else torch.from_numpy(np.ascontiguousarray(table, np.int32)).cuda()
    out, n, d = T._outputs(torch, P, out_stride)
    rep = torch.full((P + slack, 8), INFO_FILL, dtype=torch.int32, device="cuda") if info else None
    ctx.set_variant(variant); ctx.use_torch_stream()
    rc = ctx._lib.lorahip_decode_packets_info(ctx._h, T.cfg_array(cfgs), len(cfgs), None if i_dev is None else C.c_void_p(i_dev.data_ptr()),
                                              None if t_dev is None else C.c_void_p(t_dev.data_ptr()), 0 if t_dev is None else t_dev.numel(),
                                              C.c_void_p(syms.data_ptr()), stride, C.c_void_p(n_dev.data_ptr()), P, C.c_void_p(out.data_ptr()), out_stride,
                                              C.c_void_p(n.data_ptr()), C.c_void_p(d.data_ptr()), None if rep is None else C.c_void_p(rep.data_ptr()))
    assert rc == 0, ctx._lib.lorahip_last_error()
    return T._host(out, n, d), None if rep is None else rep.cpu().numpy()


def at_rate(cfg, r):
    return cfg[:2] + (int(r),) + cfg[3:]


def expand(cfgs, rows, index):
    """a table with header-rate entries and its rows -> (table of fixed-rate entries, index into it): every header-rate entry becomes five
    entries, and a row under it picks the one its header names (a field of 5..7: 4/8 -- every rate drops such a header)"""
    fixed, first = [], []
    for c in cfgs:
        first.append(len(fixed))
        fixed.extend([at_rate(c, r) for r in range(5)] if c[2] < 0 else [c])
    index = np.asarray(index)
    out = np.full(index.shape, -1, np.int32)
    for p, i in enumerate(index.tolist()):
        if 0 <= i < len(cfgs):
            c = cfgs[i]
            out[p] = first[i] + (min(int(H.header_rate(rows[p], c[0], c[1])), 4) if c[2] < 0 else 0)
    return fixed, out


def check_against_uniform_and_oracle(torch, ctx, oracle, cfgs, rows, nsyms, index, variant, tag, packets=None, short=()):
    """the launch under `cfgs` (header-rate entries among them) == the uniform launches bucketed by (entry, rate named by the header) == the
    oracle under that rate; -> ((out, out_len, dropped), report)"""
    fixed, eff = expand(cfgs, rows, index)
    got, rep = info_launch(torch, ctx, cfgs, rows, nsyms, index, variant=variant)
    known = np.flatnonzero(eff >= 0)
    want = T.uniform_by_configuration(torch, ctx, fixed, np.asarray(rows)[known], np.asarray(nsyms)[known], eff[known], variant)
    T.assert_same_launch(tuple(x[known] for x in got), want, (tag, variant, "uniform"))
    packets = packets if packets is not None else [np.asarray(rows)[p, :nsyms[p]] for p in range(len(rows))]
    table = T.oracle_rows(oracle, fixed, [packets[p] for p in known], eff[known])
    where = {int(p): k for k, p in enumerate(known)}
    T.assert_rows_equal_oracle(tuple(x[known] for x in got), fixed, eff[known], table, (tag, variant, "oracle"), short=[where[p] for p in short])
    return got, rep, eff, fixed


def assert_report(rep, want, P, tag, skip=()):
    keep = np.array([p for p in range(P) if p not in set(skip)], np.int64)
    bad = np.flatnonzero((rep[keep] != want[keep]).any(axis=1))
    assert bad.size == 0, (tag, "packet", int(keep[bad[0]]), dict(zip(H.FIELDS, rep[keep[bad[0]]].tolist())), dict(zip(H.FIELDS, want[keep[bad[0]]].tolist())))
    assert (rep[P:] == INFO_FILL).all(), (tag, "written behind n_packets")


# ---- set 1 ----------------------------------------------------------------------------------------------------------------------
HDR6 = [(sf, 0, H.RDD_FROM_HEADER, 1, 1, 0, 1, 0, 8) for sf in range(7, 13)]


@pytest.fixture(scope="module")
def set1(gpu):
    rows, nsyms, index, packets = T.build_set1(T.TABLE_A, 21)
    sent = index % 5                                                 # TABLE_A: SF major, rate minor
    named = np.array([H.header_rate(rows[p], 7 + index[p] // 5, 0) for p in range(rows.shape[0])])
    assert np.unique(index).size == 30 and (named == sent).sum() > 500
    return rows, nsyms, (index // 5).astype(np.int32), packets, sent


@pytest.mark.parametrize("variant", [0, 1])
def test_set1_encoder_made_packets_through_one_entry_per_sf(gpu, oracle, ctx, set1, variant):
    import lora_sdr_amd as L
    rc, t = plan(L.load(), HDR6, T.SET1_ROW)
    assert rc == 0 and t.lanes_per_packet == 32
    rows, nsyms, index, packets, sent = set1
    got, rep, eff, fixed = check_against_uniform_and_oracle(gpu, ctx, oracle, HDR6, rows, nsyms, index, variant, "set 1", packets)
    assert fixed == T.TABLE_A
    # the undamaged half decodes to payloads, and the 30-entry launch with the SENT rate says the same wherever the header still names it
    clean = np.arange(1, 600, 2)
    assert (got[1][clean] >= 1).all() and not got[2][clean].any()
    same = np.flatnonzero(eff == index * 5 + sent)
    T.assert_same_launch(tuple(x[same] for x in got), tuple(x[same] for x in T.table_launch(gpu, ctx, T.TABLE_A, rows, nsyms, index * 5 + sent, variant=variant)),
                         ("set 1", variant, "30 entries"))
    assert_report(rep, H.report_rows(rows, nsyms, HDR6, index), 600, ("set 1", variant))
    assert (rep[clean, 1] == sent[clean]).all() and (rep[clean, 2] == 1).all() and not rep[clean, 3].any()


# ---- set 2 ----------------------------------------------------------------------------------------------------------------------
SET2 = (((7, 0, 1), 512, None), ((10, 0, 3), 160, 160))              # (body (sf, ppm, rate), row, symbols the body is cut to)
SET2_LENGTHS = (0, 1, 2, 20, 255)
FLAGS = [(crcc, ec) for crcc in (0, 1) for ec in (0, 1)]


@pytest.fixture(scope="module")
def set2(gpu):
    out = []
    for (sf, ppm, body_rate), stride, cut in SET2:
        grid = S.set_h(sf, ppm, body_rate, n_symbols=cut) if cut else S.set_h(sf, ppm, body_rate)
        pick = np.array([ln * 16 + k for ln in SET2_LENGTHS for k in range(16)])
        packets = [grid[p] for p in pick for _ in FLAGS]
        index = np.array([f for _ in pick for f in range(len(FLAGS))], np.int32)
        cfgs = [(sf, ppm, H.RDD_FROM_HEADER, crcc, 1, ec, 1, 0, 8) for crcc, ec in FLAGS]
        rows, nsyms = S.as_rows(packets, stride)
        assert int(nsyms.max()) <= stride
        ln, crc, rate = S.header_grid(range(256))
        out.append((cfgs, rows, nsyms, index, np.repeat(rate[pick], len(FLAGS)), np.repeat(ln[pick], len(FLAGS)), np.repeat(crc[pick], len(FLAGS)),
                    body_rate, stride))
    return out


@pytest.mark.parametrize("variant", [0, 1])
def test_set2_crafted_headers_on_bodies_of_another_rate(gpu, oracle, ctx, set2, variant):
    import lora_sdr_amd as L
    for cfgs, rows, nsyms, index, rate, length, crc_flag, body_rate, stride in set2:
        rc, t = plan(L.load(), cfgs, stride)
        assert rc == 0 and t.lanes_per_packet == {512: 64, 160: 32}[stride]
        got, rep, eff, fixed = check_against_uniform_and_oracle(gpu, ctx, oracle, cfgs, rows, nsyms, index, variant, ("set 2", stride))
        out, n, d = got
        high = np.flatnonzero(rate > 4)
        assert high.size == 3 * 2 * len(SET2_LENGTHS) * len(FLAGS)
        assert (n[high] == -1).all() and (d[high] == 1).all() and (out[high] == SENTINEL).all()
        # the body decodes where the header names its rate and its length, and only there the checksum agrees
        own = np.flatnonzero((rate == body_rate) & (length == 20) & (crc_flag == 1))
        assert own.size == len(FLAGS) and (n[own] == 20).all() and not d[own].any() and (rep[own, 2] == 1).all()
        assert set(np.unique(n).tolist()) >= {-1, 0, 1, 2, 20} and {0, 1} == set(np.unique(d).tolist())
        want = H.report_rows(rows, nsyms, cfgs, index)
        assert_report(rep, want, rows.shape[0], ("set 2", stride, variant))
        assert (rep[:rows.shape[0], 1] == rate).all() and (rep[:rows.shape[0], 0] == length).all() and not rep[:rows.shape[0], 3].any()
        assert {-1, 0, 1} == set(np.unique(want[:, 2]).tolist()) and {0, 1} == set(np.unique(want[:, 4]).tolist())


# ---- set 3 ----------------------------------------------------------------------------------------------------------------------
def limits_packet(r, extra_blocks, seed):
    """SF7, 20 bytes + crc at rate r: 49 codewords are read, 7 blocks, 8 + 6 * (4 + r) symbols; extra_blocks of zero nibbles behind them"""
    s, _ = D.build(7, np.random.default_rng(seed).integers(0, 256, 20).astype(np.uint8), 0, r, True, True, n_blocks=extra_blocks)
    need = 8 + 6 * (4 + r)
    assert s.size == need + extra_blocks * (4 + r)
    return s, need


@pytest.mark.parametrize("r", range(5))
def test_set3_row_limits_are_those_of_the_rate_the_header_names(gpu, oracle, ctx, r):
    """per rate: the row is exactly what the length needs (the packet as long, and four blocks longer than its row): decodes; one block
    fewer: -2 with the need reported. The uniform launch at rate r says the same, byte for byte."""
    cfg = (7, 0, H.RDD_FROM_HEADER, 1, 1, 1, 1, 0, 8)
    exact, need = limits_packet(r, 0, 50 + r)
    longer, _ = limits_packet(r, 4, 60 + r)
    payload = oracle.decode(7, exact, cr=S.RDD_TO_CR[r], crcc=True, error_check=True)[0]
    assert payload is not None and payload.size == 20
    for stride, fits in ((need, True), (need - (4 + r), False)):
        rows, nsyms = S.as_rows([exact, longer, exact[:stride]], stride)
        (out, n, d), rep = info_launch(gpu, ctx, [cfg], rows, nsyms, np.zeros(3, np.int32))
        T.assert_same_launch((out, n, d), T.uniform_launch(gpu, ctx, at_rate(cfg, r), rows, nsyms), ("set 3", r, stride))
        if fits:
            assert n.tolist() == [20, 20, 20] and not d.any() and all(np.array_equal(out[p, :20], payload) for p in (0, 2))
            assert np.array_equal(oracle.decode(7, longer, cr=S.RDD_TO_CR[r], crcc=True, error_check=True)[0], out[1, :20])
        else:
            # the first two announce more than the row holds (-2); the third IS as short as its row: the reference drops it (by count, :313,
            # at 4/8; behind the zeros it reads instead of the missing block at the other rates, whose count takes the first block for a short one)
            assert n.tolist() == [-2, -2, -1] and d.tolist() == [0, 0, 1] and (out == SENTINEL).all()
            assert oracle.decode(7, exact[:stride], cr=S.RDD_TO_CR[r], crcc=True, error_check=True) == (None, 1)
        assert rep[:2, 5].tolist() == [need, need] and rep[:3, 1].tolist() == [r] * 3 and rep[:3, 0].tolist() == [20] * 3
        want = H.report_rows(rows, nsyms, [cfg], np.zeros(3, np.int32))
        want[n == -2, 2] = want[n == -2, 4] = 0                     # (-2 is the kernels' own outcome: their decode ends there; the header is clean)
        assert_report(rep, want, 3, ("set 3", r, stride))


def test_set3_five_rates_in_one_row_length(gpu, oracle, ctx):
    """rows of 44 symbols: 20 bytes need 32 / 38 / 44 / 50 / 56 symbols at 4/4 .. 4/8 -- three rates decode, two are -2, in one launch, each
    four blocks longer than needed. The entry's plan is that of the largest rate; each packet's decision that of its own."""
    cfg = (7, 0, H.RDD_FROM_HEADER, 1, 1, 1, 1, 0, 8)
    packets = [limits_packet(p % 5, 4, 70 + p)[0] for p in range(40)]
    rows, nsyms = S.as_rows(packets, 44)
    assert (nsyms >= 44).all()
    (out, n, d), rep = info_launch(gpu, ctx, [cfg], rows, nsyms, np.zeros(40, np.int32))
    fixed, eff = expand([cfg], rows, np.zeros(40, np.int32))
    assert eff.tolist() == [p % 5 for p in range(40)]
    T.assert_same_launch((out, n, d), T.uniform_by_configuration(gpu, ctx, fixed, rows, nsyms, eff), "set 3, one row length")
    assert n.tolist() == [20 if p % 5 <= 2 else -2 for p in range(40)] and not d.any()
    for p in range(40):
        if p % 5 <= 2:
            assert np.array_equal(out[p, :20], oracle.decode(7, packets[p], cr=S.RDD_TO_CR[p % 5], crcc=True, error_check=True)[0])
    assert rep[:40, 5].tolist() == [8 + 6 * (4 + p % 5) for p in range(40)]


# ---- set 4 ----------------------------------------------------------------------------------------------------------------------
SET4 = [(7, 0, H.RDD_FROM_HEADER, 1, 1, 1, 1, 0, 8), (7, 0, 2, 1, 1, 0, 1, 1, 8), (12, 0, 4, 1, 1, 1, 0, 0, 6), (7, 5, 4, 0, 0, 0, 1, 0, 8),
        (12, 0, H.RDD_FROM_HEADER, 0, 1, 0, 1, 1, 8)]
SET4_ROW = 64


@pytest.fixture(scope="module")
def set4(gpu):
    rng = np.random.default_rng(44)
    packets, index = [], []
    for p in range(70):
        i = p % len(SET4)
        sf, ppm, rdd, _, inter, _, explicit, _, dlen = SET4[i]
        if not inter:
            s = rng.integers(0, 128, (5, 8, 13, 16, 12)[(p // 5) % 5]).astype(np.uint16)
        else:
            r = int(rng.integers(0, 5)) if rdd < 0 else rdd
            s, _ = D.build(sf, rng.integers(0, 256, int(rng.integers(4, 12)) if explicit else dlen).astype(np.uint8), ppm, r, bool(explicit), True)
            if p % 7 == 3:
                s = D.flip(s, sf, ppm, r, (ppm or sf) + 1, 1)
        packets.append(s); index.append(i)
    rows, nsyms = S.as_rows(packets, SET4_ROW)
    assert int(nsyms.max()) <= SET4_ROW
    return rows, nsyms, np.array(index, np.int32), packets


@pytest.mark.parametrize("variant", [0, 1])
def test_set4_every_kind_of_entry_in_one_launch(gpu, oracle, ctx, set4, variant):
    import lora_sdr_amd as L
    rows, nsyms, index, packets = set4
    rc, t = plan(L.load(), SET4, SET4_ROW)
    assert rc == 0 and t.lanes_per_packet == 16
    got, rep, eff, fixed = check_against_uniform_and_oracle(gpu, ctx, oracle, SET4, rows, nsyms, index, variant, "set 4", packets)
    assert len(fixed) == 13 and {S.outcome(r) for r in T.oracle_rows(oracle, fixed, packets, eff)} >= {"bytes", "dropped"}
    assert_report(rep, H.report_rows(rows, nsyms, SET4, index), 70, ("set 4", variant))
    off = np.flatnonzero(index == 3)
    assert (rep[off, :6] == np.array(H.NOT_REACHED)).all() and set(got[1][off].tolist()) == {-1, 8, 16}
    implicit = np.flatnonzero(index == 2)
    assert (rep[implicit, 3] == -1).all() and (rep[implicit, 0] == 6).all() and (rep[implicit, 1] == 4).all()
    # indices without an entry: -3, the row untouched, the report "not reached"; the table_dev form gives the direct form's result
    bad = {4: -1, 9: len(SET4), 31: 2 ** 31 - 1, 32: -2 ** 31}
    direct = index.copy()
    for p, v in bad.items():
        direct[p] = v
    (out, n, d), rep_bad = info_launch(gpu, ctx, SET4, rows, nsyms, direct, variant=variant)
    for p in bad:
        assert n[p] == -3 and d[p] == 0 and (out[p] == SENTINEL).all() and rep_bad[p].tolist() == list(H.NOT_REACHED) + [0, 0]
    good = np.array([p for p in range(70) if p not in bad])
    T.assert_same_launch(tuple(x[good] for x in (out, n, d)), tuple(x[good] for x in got), ("set 4", variant, "direct"))
    assert np.array_equal(rep_bad[good], rep[good])
    entry_of_channel = (np.arange(100) % len(SET4)).astype(np.int32)
    entry_of_channel[13] = 9
    channel = (5 * (np.arange(70) % 20) + index).astype(np.int32)
    assert channel.max() < 100 and 13 not in channel
    outside = {2: 100, 11: -1, 30: 13}
    for p, v in outside.items():
        channel[p] = v
    want = index.copy()
    want[list(outside)] = -1
    via, rep_via = info_launch(gpu, ctx, SET4, rows, nsyms, channel, table=entry_of_channel, variant=variant)
    ref_, rep_ref = info_launch(gpu, ctx, SET4, rows, nsyms, want, variant=variant)
    T.assert_same_launch(via, ref_, ("set 4", variant, "table"))
    assert np.array_equal(rep_via, rep_ref) and all(via[1][p] == -3 for p in outside)


# ---- set 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set5_launch_sizes_round_a_workgroup(gpu, oracle, ctx, variant):
    """rows of 16 symbols, 8 lanes and 32 packets per workgroup: packet 31 runs under the SF8 entry, packet 32 under the SF7 entry; rates in
    turn, every fifth packet damaged"""
    import lora_sdr_amd as L
    cfgs = [(7, 0, H.RDD_FROM_HEADER, 1, 1, 0, 1, 0, 8), (8, 0, H.RDD_FROM_HEADER, 1, 1, 1, 1, 1, 8)]
    rc, t = plan(L.load(), cfgs, 16)
    assert rc == 0 and t.lanes_per_packet == 8 and t.packets_per_workgroup == 32
    rng = np.random.default_rng(5)
    packets, index = [], []
    for p in range(65):
        i, r = p & 1, (p // 2) % 5
        s, _ = D.build(7 + i, rng.integers(0, 256, 1 + (p // 10) % 2 + i).astype(np.uint8), 0, r, True, True)
        if p % 5 == 4:
            s = D.flip(s, 7 + i, 0, r, 7 + i + 1, 0)
        assert s.size <= 16
        packets.append(s); index.append(i)
    index = np.array(index, np.int32)
    rows, nsyms = S.as_rows(packets, 16)
    for count in T.COUNTS:
        got, rep, eff, _ = check_against_uniform_and_oracle(gpu, ctx, oracle, cfgs, rows[:count], nsyms[:count], index[:count], variant, ("set 5", count),
                                                            packets[:count])
        assert_report(rep, H.report_rows(rows[:count], nsyms[:count], cfgs, index[:count]), count, ("set 5", count, variant))
    assert set(eff.tolist()) == set(range(10)) and {0, 1} == set(got[2].tolist())


# ---- set 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set6_without_a_report_it_is_the_table_launch(gpu, ctx, set1, set4, variant):
    rows, nsyms, index, _, _ = set1
    for cfgs, (r_, n_, i_) in ((HDR6, (rows, nsyms, index)), (SET4, set4[:3])):
        with_rep, rep = info_launch(gpu, ctx, cfgs, r_, n_, i_, variant=variant)
        without, none = info_launch(gpu, ctx, cfgs, r_, n_, i_, variant=variant, info=False)
        assert none is None and (rep[:len(r_)] != INFO_FILL).all()
        T.assert_same_launch(without, T.table_launch(gpu, ctx, cfgs, r_, n_, i_, variant=variant), ("set 6", variant))
        T.assert_same_launch(with_rep, without, ("set 6", variant, "the report changes nothing"))


def test_set6_the_report_of_fixed_rate_entries(gpu, ctx):
    """the report does not need a header-rate entry: TABLE_A's packets under TABLE_A, both kernels"""
    rows, nsyms, index, _ = T.build_set1(T.TABLE_A, 23)
    want = H.report_rows(rows[:200], nsyms[:200], T.TABLE_A, index[:200])
    for variant in (0, 1):
        got, rep = info_launch(gpu, ctx, T.TABLE_A, rows[:200], nsyms[:200], index[:200], variant=variant)
        T.assert_same_launch(got, T.table_launch(gpu, ctx, T.TABLE_A, rows[:200], nsyms[:200], index[:200], variant=variant), ("fixed", variant))
        assert_report(rep, want, 200, ("fixed", variant))


# ---- set 7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_set7_uniform_entry_point_and_the_form_without_an_index(gpu, ctx, set2, variant):
    cfgs, rows, nsyms, index, *_ = set2[1]
    sel = np.flatnonzero(index == 2)
    one = [cfgs[2]]
    table, rep_t = info_launch(gpu, ctx, one, rows[sel], nsyms[sel], np.zeros(sel.size, np.int32), variant=variant)
    T.assert_same_launch(T.uniform_launch(gpu, ctx, one[0], rows[sel], nsyms[sel], variant), table, ("set 7", variant, "uniform"))
    bare, rep_b = info_launch(gpu, ctx, one, rows[sel], nsyms[sel], None, variant=variant)
    T.assert_same_launch(bare, table, ("set 7", variant, "no index"))
    assert np.array_equal(rep_b, rep_t)


def test_set7_the_host_form_equals_the_device_form(gpu, ctx, set4):
    from lora_sdr_amd import _lib
    rows, nsyms, index, _ = set4
    index = index.copy()
    index[5] = len(SET4)                                             # (a row without an entry stays as the caller had it)
    dev, rep_dev = info_launch(gpu, ctx, SET4, rows, nsyms, index)
    P, stride = rows.shape
    out_stride = 2 * (stride + 8)
    for table, with_info in ((None, True), (np.arange(len(SET4) + 1, dtype=np.int32), True), (None, False)):
        out, n, d = np.full((P, out_stride), SENTINEL, np.uint8), np.full(P, -77, np.int32), np.full(P, -77, np.int32)
        rep = np.full((P + 3, 8), INFO_FILL, np.int32)
        syms = np.array(rows, np.uint16)
        ctx.set_variant(0); ctx.use_torch_stream()
        rc = ctx._lib.lorahip_decode_packets_info_host(ctx._h, T.cfg_array(SET4), len(SET4), index.ctypes.data, None if table is None else table.ctypes.data,
                                                       0 if table is None else table.size, syms.ctypes.data, stride, nsyms.ctypes.data, P, out.ctypes.data,
                                                       out_stride, n.ctypes.data, d.ctypes.data, rep.ctypes.data if with_info else None)
        assert rc == 0, ctx._lib.lorahip_last_error()
        T.assert_same_launch((out, n, d), dev, ("host", table is not None, with_info))
        assert np.array_equal(rep, rep_dev) if with_info else (rep == INFO_FILL).all()
    assert dev[1][5] == -3 and C.sizeof(_lib.PacketInfo) == 32
    # the one-entry form without an index, in host memory
    sel = np.flatnonzero(index == 0)
    one, rep_one = info_launch(gpu, ctx, SET4[:1], rows[sel], nsyms[sel], None)
    out, n, d = np.full((sel.size, out_stride), SENTINEL, np.uint8), np.full(sel.size, -77, np.int32), np.full(sel.size, -77, np.int32)
    rep = np.full((sel.size + 3, 8), INFO_FILL, np.int32)
    syms, ns = np.array(rows[sel], np.uint16), np.ascontiguousarray(nsyms[sel])
    rc = ctx._lib.lorahip_decode_packets_info_host(ctx._h, T.cfg_array(SET4[:1]), 1, None, None, 0, syms.ctypes.data, stride, ns.ctypes.data, sel.size,
                                                   out.ctypes.data, out_stride, n.ctypes.data, d.ctypes.data, rep.ctypes.data)
    assert rc == 0, ctx._lib.lorahip_last_error()
    T.assert_same_launch((out, n, d), one, "host, no index")
    assert np.array_equal(rep, rep_one)


def test_python_surface(gpu, ctx, set1):
    """LoRaDecoder.setCodingRate("header"), decode_batch(info=True) of a decoder and of a set; work() as before"""
    import lora_sdr_amd as L
    rows, nsyms, index, packets, sent = set1
    decs = []
    for sf in range(7, 13):
        d = L.LoRaDecoder(); d.setSpreadFactor(sf); d.setCodingRate("header"); d.enableCrcc(True)
        decs.append(d)
    ds = L.LoRaDecoderSet(decs)
    syms_dev = gpu.from_numpy(np.array(rows, np.uint16).view(np.int16)).cuda()
    res = ds.decode_batch(syms_dev, gpu.from_numpy(nsyms).cuda(), gpu.from_numpy(index).cuda(), info=True)
    assert len(res) == 4 and res[3].shape == (600, 8) and res[3].dtype == gpu.int32
    (_, n, d), rep = info_launch(gpu, ctx, HDR6, rows, nsyms, index)
    assert np.array_equal(res[1].cpu().numpy(), n) and np.array_equal(res[2].cpu().numpy(), d) and np.array_equal(res[3].cpu().numpy(), rep[:600])
    assert len(ds.decode_batch(syms_dev, gpu.from_numpy(nsyms).cuda(), gpu.from_numpy(index).cuda())) == 3
    sel = np.flatnonzero(index == 2)
    one = decs[2].decode_batch(syms_dev[sel], gpu.from_numpy(nsyms[sel]).cuda(), info=True)
    assert len(one) == 4 and np.array_equal(one[1].cpu().numpy(), n[sel]) and np.array_equal(one[3].cpu().numpy(), rep[sel])
    assert len(decs[2].decode_batch(syms_dev[sel], gpu.from_numpy(nsyms[sel]).cuda())) == 3
    back = ds.work([packets[p] for p in range(1, 60, 2)], index[1:60:2])
    assert all(b is not None and 1 <= b.size <= 40 for b in back) and ds.getDropped() == 0


# ---- refusals with a real context ------------------------------------------------------------------------------------------------
def test_refusals_with_a_context_leave_the_outputs_untouched(gpu, ctx):
    """rdd = -1 without a header or without interleaving, rdd = -2, and a NULL index with two entries: LORAHIP_E_INVALID from every decode
    entry point, device and host form, with a context that would launch -- and not a byte of the 0xA5-filled outputs or of the report
    written. The same calls with a table that is in order return 0 and write."""
    from test_header_rate_cpu import refused_tables
    lib = ctx._lib
    ok = (7, 0, H.RDD_FROM_HEADER, 1, 1, 0, 1, 0, 8)
    s, _ = D.build(7, np.arange(2, dtype=np.uint8), 0, 2, True, True)
    P, stride, out_stride = 4, 16, 48
    rows, nsyms = S.as_rows([s] * P, stride)
    rows = np.array(rows, np.uint16)
    index = np.zeros(P, np.int32)
    ctx.set_variant(0); ctx.use_torch_stream()

    def device_call(fn, cfgs, with_index=True, info=True, uniform=False):
        syms_d, n_d = gpu.from_numpy(rows.view(np.int16)).cuda(), gpu.from_numpy(nsyms).cuda()
        i_d = gpu.from_numpy(index).cuda()
        out, n, d = T._outputs(gpu, P, out_stride)
        rep = gpu.full((P, 8), INFO_FILL, dtype=gpu.int32, device="cuda")
        tail = (C.c_void_p(syms_d.data_ptr()), stride, C.c_void_p(n_d.data_ptr()), P, C.c_void_p(out.data_ptr()), out_stride, C.c_void_p(n.data_ptr()),
                C.c_void_p(d.data_ptr()))
        if uniform:
            rc = fn(ctx._h, T.cfg_array(cfgs), *tail)
        else:
            head = (ctx._h, T.cfg_array(cfgs), len(cfgs), C.c_void_p(i_d.data_ptr()) if with_index else None, None, 0)
            rc = fn(*head, *tail, C.c_void_p(rep.data_ptr())) if info else fn(*head, *tail)
        gpu.cuda.synchronize()
        return rc, out.cpu().numpy(), n.cpu().numpy(), d.cpu().numpy(), rep.cpu().numpy()

    def host_call(fn, cfgs, with_index=True, info=True, uniform=False):
        out, n, d = np.full((P, out_stride), SENTINEL, np.uint8), np.full(P, -77, np.int32), np.full(P, -77, np.int32)
        rep = np.full((P, 8), INFO_FILL, np.int32)
        tail = (rows.ctypes.data, stride, nsyms.ctypes.data, P, out.ctypes.data, out_stride, n.ctypes.data, d.ctypes.data)
        if uniform:
            rc = fn(ctx._h, T.cfg_array(cfgs), *tail)
        else:
            head = (ctx._h, T.cfg_array(cfgs), len(cfgs), index.ctypes.data if with_index else None, None, 0)
            rc = fn(*head, *tail, rep.ctypes.data) if info else fn(*head, *tail)
        return rc, out, n, d, rep

    def untouched(res):
        rc, out, n, d, rep = res
        return rc == -1 and (out == SENTINEL).all() and (n == -77).all() and (d == -77).all() and (rep == INFO_FILL).all()

    def written(res):
        rc, out, n, d, rep = res
        return rc == 0 and (n == 2).all() and not d.any() and (out[:, :2] == [0, 1]).all()

    tables = refused_tables()
    assert len(tables) == 3
    for name, cfgs in tables.items():
        bad = [c for c in cfgs if c[2] < 0 and (c[2] < -1 or not (c[4] and c[6]))][:1]
        assert len(bad) == 1
        assert untouched(device_call(lib.lorahip_decode_packets_info, cfgs)), name
        assert untouched(host_call(lib.lorahip_decode_packets_info_host, cfgs)), name
        assert untouched(device_call(lib.lorahip_decode_packets_cfgs, cfgs, info=False)), name
        assert untouched(host_call(lib.lorahip_decode_packets_cfgs_host, cfgs, info=False)), name
        assert untouched(device_call(lib.lorahip_decode_packets, bad, uniform=True)), name
        assert untouched(host_call(lib.lorahip_decode_packets_host, bad, uniform=True)), name
        assert untouched(device_call(lib.lorahip_decode_packets_info, bad, with_index=False)), name
    # a NULL index: the uniform launch of ONE entry, refused with two
    assert untouched(device_call(lib.lorahip_decode_packets_info, [ok, ok], with_index=False))
    assert untouched(host_call(lib.lorahip_decode_packets_info_host, [ok, ok], with_index=False))
    # the same calls with a table that is in order launch and write
    assert written(device_call(lib.lorahip_decode_packets_info, [ok, ok]))
    assert written(host_call(lib.lorahip_decode_packets_info_host, [ok, ok]))
    assert written(device_call(lib.lorahip_decode_packets_info, [ok], with_index=False))
    assert written(host_call(lib.lorahip_decode_packets_info_host, [ok], with_index=False))
    assert written(device_call(lib.lorahip_decode_packets_cfgs, [ok, ok], info=False))
    assert written(host_call(lib.lorahip_decode_packets_cfgs_host, [ok, ok], info=False))
    assert written(device_call(lib.lorahip_decode_packets, [ok], uniform=True))
    assert written(host_call(lib.lorahip_decode_packets_host, [ok], uniform=True))


def test_the_checker_keeps_its_row_rule_in_front_of_a_rate_field_above_4(gpu, ctx):
    """variant 1 only: a packet longer than its row is -2 under every fixed rate, so it is -2 under a header-rate entry too, whatever its
    rate field says; as long as its row, a field of 5..7 is (-1, dropped 1). The group kernel (variant 0) drops both in the header."""
    cfg = (7, 0, H.RDD_FROM_HEADER, 1, 1, 0, 1, 0, 8)
    body, _ = D.build(7, np.arange(2, dtype=np.uint8), 0, 4, True, True)
    assert body.size == 16
    packets = D.set_header(body, 7, 0, np.full(8, 2), np.ones(8, np.int64), np.arange(8))
    rows, _ = S.as_rows(list(packets), 16)
    for nsyms, want_high in ((16, (-1, 1)), (17, (-2, 0))):
        n_arr = np.full(8, nsyms, np.int32)
        (out, n, d), _ = info_launch(gpu, ctx, [cfg], rows, n_arr, np.zeros(8, np.int32), variant=1)
        for r in range(8):
            uni = T.uniform_launch(gpu, ctx, at_rate(cfg, min(r, 4)), rows[r:r + 1], n_arr[r:r + 1], variant=1)
            assert (int(n[r]), int(d[r])) == (int(uni[1][0]), int(uni[2][0])), (nsyms, r)
            assert np.array_equal(out[r], uni[0][0]), (nsyms, r)
            if r > 4:
                assert (int(n[r]), int(d[r])) == want_high and (out[r] == SENTINEL).all(), (nsyms, r)
        (out0, n0, d0), _ = info_launch(gpu, ctx, [cfg], rows, n_arr, np.zeros(8, np.int32), variant=0)
        assert n0[5:].tolist() == [-1] * 3 and d0[5:].tolist() == [1] * 3
