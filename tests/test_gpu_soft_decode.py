"""GPU: the soft-decision decoder (lorahip_decode_packets_soft / _soft_host; LoRaDecoder.decode_soft, LoRaDecoderSet.decode_soft) against its
definition, tests/soft_def.py::decode_soft_def -- codec_hdr_def.walk with LLRs for symbols and a maximum-likelihood nibble for every FEC
call. Everything compared is integer and exact: out rows with the 0xA5 they are pre-filled with, out_len, dropped, the header report.

One table launch carries every rate 4/4..4/8 with explicit and implicit headers, crcc / error_check / hdr on and off, ppm < sf, and two
header-rate entries; its packets are half noise (normal LLRs) and half encoder-made packets under noise, a third of all rows quantised
to multiples of 1/2 (equal metrics: the tie rule) and sprinkled with exact zeros; rows of 60 symbols, counts from 0 to beyond the row,
indices without an entry. The reference has no rows: a packet longer than its row whose length needs symbols behind the row is -2, with
the report the walk had behind the length check.

A configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr, data_length)."""
import ctypes as C

import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as E
import codec_hdr_def as H
import soft_def as S
import test_gpu_codec_cfgs as T

pytestmark = pytest.mark.gpu

SENTINEL = T.SENTINEL
INFO_FILL = -1234567
STRIDE, WIDTH = 60, 10

CFGS = []
for _r in range(5):
    CFGS += [(7, 0, _r, 1, 1, 0, 1, 0, 0), (9, 7, _r, 0, 1, 1, 1, 1, 0), (8, 0, _r, 1, 1, 0, 0, 0, 6), (8, 6, _r, 0, 1, 1, 0, 1, 9)]
CFGS += [(7, 0, H.RDD_FROM_HEADER, 1, 1, 0, 1, 0, 0), (10, 8, H.RDD_FROM_HEADER, 0, 1, 1, 1, 1, 0)]


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as L
    c = L.Context(7)                                                 # device and stream only
    yield c
    c.close()


def _ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def soft_launch(torch, ctx, cfgs, rows, nsyms, index, table=None, host=False, info=True, stride=STRIDE):
    """lorahip_decode_packets_soft (or its host form) on outputs filled with 0xA5 and a report filled with INFO_FILL; rows (P, llr_stride) float32"""
    rows = np.ascontiguousarray(rows, np.float32)
    P, llr_stride = rows.shape
    out_stride = 2 * (stride + 8)
    n = np.ascontiguousarray(nsyms, np.int32)
    i = None if index is None else np.ascontiguousarray(index, np.int32)
    t = None if table is None else np.ascontiguousarray(table, np.int32)
    if host:
        out, ol, dr = np.full((P, out_stride), SENTINEL, np.uint8), np.full(P, -77, np.int32), np.full(P, -77, np.int32)
        rep = np.full((P, 8), INFO_FILL, np.int32) if info else None
        rc = ctx._lib.lorahip_decode_packets_soft_host(ctx._h, T.cfg_array(cfgs), len(cfgs), _ptr(i), _ptr(t), 0 if t is None else t.size, _ptr(rows), llr_stride, stride,
                                                       _ptr(n), P, _ptr(out), out_stride, _ptr(ol), _ptr(dr), _ptr(rep))
        assert rc == 0, ctx._lib.lorahip_last_error()
        return (out, ol, dr), rep
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (rows, n, i, t)]
    out, ol, dr = T._outputs(torch, P, out_stride)
    rep = torch.full((P, 8), INFO_FILL, dtype=torch.int32, device="cuda") if info else None
    ctx.use_torch_stream()
    rc = ctx._lib.lorahip_decode_packets_soft(ctx._h, T.cfg_array(cfgs), len(cfgs), _ptr(dev[2]), _ptr(dev[3]), 0 if t is None else t.size, _ptr(dev[0]), llr_stride, stride,
                                              _ptr(dev[1]), P, _ptr(out), out_stride, _ptr(ol), _ptr(dr), _ptr(rep))
    assert rc == 0, ctx._lib.lorahip_last_error()
    return T._host(out, ol, dr), None if rep is None else rep.cpu().numpy()


def make_rows(seed, per_cfg=20):
    """-> rows (P, STRIDE * WIDTH) float32 (7.0 where a packet's entry reads nothing), nsyms, index"""
    rng = np.random.default_rng(seed)
    rows, nsyms, index = [], [], []
    for i, cfg in enumerate(CFGS):
        sf, ppm, rdd, crcc, _, _, explicit, _, dlen = cfg
        P = ppm or sf
        for j in range(per_cfg):
            if j % 2:                                                # noise
                n = int(rng.choice([0, 5, 7, 8, 9, 16, 23, 40, 59, 60, 61, 75, 300]))
                llr = rng.standard_normal((STRIDE, P)).astype(np.float32)
            else:                                                    # an encoder-made packet under noise
                rate = int(rng.integers(0, 5)) if rdd < 0 else rdd
                # (every sixth: a message much longer than the row -- its header decodes, its length needs symbols behind the row)
                payload = rng.integers(0, 256, (40 if j % 12 == 10 else int(rng.integers(1, 9))) if explicit else dlen, dtype=np.uint8)
                syms, _ = D.build(sf, payload, ppm, rate, bool(explicit), bool(crcc) if not explicit else bool(j % 4 == 0))
                n = int(syms.size) + (int(rng.integers(1, 20)) if j % 6 == 4 else 0)        # now and then a count that runs on behind the packet
                llr = np.zeros((max(STRIDE, syms.size), P), np.float32)
                llr[:syms.size] = S.llr_of_symbols(syms, sf, P) * rng.uniform(0.5, 2.0, (syms.size, P)).astype(np.float32)
                llr += ((0.1, 0.35, 0.6)[(j // 2) % 3] * rng.standard_normal(llr.shape)).astype(np.float32)
                llr = llr[:STRIDE]
            if j % 3 == 0:                                           # equal metrics: few distinct magnitudes
                llr = (np.round(llr * 2) / 2).astype(np.float32)
            llr[rng.random(llr.shape) < 0.04] = 0.0                  # exact zeros
            row = np.full(STRIDE * WIDTH, 7.0, np.float32)
            row[:STRIDE * P] = llr.reshape(-1)
            rows.append(row); nsyms.append(n); index.append(i)
    for bad in (-1, len(CFGS), 1000):                                # no such entry
        rows.append(rng.standard_normal(STRIDE * WIDTH).astype(np.float32)); nsyms.append(30); index.append(bad)
    order = rng.permutation(len(rows))                               # neighbours under different entries
    return np.stack(rows)[order], np.array(nsyms, np.int32)[order], np.array(index, np.int32)[order]


def expected(cfgs, rows, nsyms, index, stride=STRIDE):
    P = len(rows)
    out = np.full((P, 2 * (stride + 8)), SENTINEL, np.uint8)
    out_len, dropped = np.full(P, -1, np.int32), np.zeros(P, np.int32)
    rep = np.zeros((P, 8), np.int32)
    short = []
    for p in range(P):
        i = int(index[p])
        if not 0 <= i < len(cfgs):
            out_len[p] = -3
            rep[p, :6] = H.NOT_REACHED
            continue
        cfg = cfgs[i]
        W = cfg[1] or cfg[0]
        n = int(nsyms[p])
        by, dr, r = S.decode_soft_def(rows[p, :stride * W].reshape(stride, W)[:max(0, min(n, stride))], cfg, n)
        rep[p, :6] = r
        if n > stride and r[5] > stride:                             # the row rule: reported, never guessed
            out_len[p] = -2
            rep[p, 2] = 0
            short.append(p)
            continue
        dropped[p] = dr
        if by is not None:
            out_len[p] = by.size
            out[p, :by.size] = by
    return (out, out_len, dropped), rep, short


def assert_equal(got, rep, want, wrep, short, tag):
    for name, a, b in zip(("out", "out_len", "dropped"), got, want):
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, (tag, name, "packet", int(bad[0]), a[bad[0]], b[bad[0]])
    if rep is not None:
        cols = np.ones(8, bool)
        for p in range(len(rep)):
            cols[4] = p not in short                                 # fec_error of a -2 packet: the header's, the walk went on
            assert np.array_equal(rep[p][cols], wrep[p][cols]), (tag, "report of packet", p, rep[p], wrep[p])


@pytest.fixture(scope="module")
def table_set(gpu):
    rows, nsyms, index = make_rows(2024)
    want = expected(CFGS, rows, nsyms, index)
    o, n, d = want[0]
    # the set reaches every outcome and both ends of the decode
    assert (n > 0).sum() > 60 and (d == 1).sum() > 40 and (n == -2).sum() >= 1 and (n == -3).sum() == 3 and ((n == -1) & (d == 0)).sum() >= 5
    assert (want[1][:, 2] == 1).sum() > 20 and (want[1][:, 2] == -1).sum() > 5 and (want[1][:, 4] == 1).sum() > 40
    return rows, nsyms, index, want


def test_table_launch_equals_the_definition(gpu, ctx, table_set):
    rows, nsyms, index, (want, wrep, short) = table_set
    got, rep = soft_launch(gpu, ctx, CFGS, rows, nsyms, index)
    assert_equal(got, rep, want, wrep, short, "device")
    # a table between the index and the entries; no report: the same outputs
    perm = np.random.default_rng(5).permutation(len(CFGS)).astype(np.int32)
    inv = np.argsort(perm).astype(np.int32)
    idx2 = np.where((index >= 0) & (index < len(CFGS)), inv[np.clip(index, 0, len(CFGS) - 1)], np.where(index < 0, -1, 999)).astype(np.int32)
    got2, none = soft_launch(gpu, ctx, CFGS, rows, nsyms, idx2, table=perm, info=False)
    assert none is None
    assert_equal(got2, None, want, wrep, short, "table")


def test_host_form_equals_the_device_form(gpu, ctx, table_set):
    rows, nsyms, index, (want, wrep, short) = table_set
    got, rep = soft_launch(gpu, ctx, CFGS, rows, nsyms, index, host=True)
    assert_equal(got, rep, want, wrep, short, "host")


def decoder_of(L, cfg):
    """a LoRaDecoder set up through the block's setters to the configuration tuple"""
    sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = cfg
    d = L.LoRaDecoder()
    d.setSpreadFactor(sf); d.setSymbolSize(ppm); d.setCodingRate("header" if rdd < 0 else "4/%d" % (4 + rdd))
    d.enableCrcc(bool(crcc)); d.enableInterleaving(bool(inter)); d.enableErrorCheck(bool(ec)); d.enableExplicit(bool(explicit)); d.enableHdr(bool(hdr))
    d.setDataLength(dlen)
    return d


def test_decoder_set_decode_soft(gpu, table_set):
    """LoRaDecoderSet.decode_soft over fixed-rate and header-rate decoders, indices without a decoder among them: the definition again,
    through the public object -- without and with a table, with and without the report. Its output rows start as zeros."""
    import lora_sdr_amd as L
    torch = gpu
    rows, nsyms, index, (want, wrep, short) = table_set
    decoders = [decoder_of(L, c) for c in CFGS]
    dset = L.LoRaDecoderSet(decoders)
    zeroed = want[0].copy()
    for p, n in enumerate(want[1]):
        zeroed[p, max(int(n), 0):] = 0
    llr = torch.from_numpy(rows.reshape(len(rows), STRIDE, WIDTH)).cuda()
    n_dev, i_dev = torch.from_numpy(nsyms).cuda(), torch.from_numpy(index).cuda()
    out, out_len, dropped, rep = (t.cpu().numpy() for t in dset.decode_soft(llr, n_dev, i_dev, info=True))
    assert_equal((out, out_len, dropped), rep, (zeroed, want[1], want[2]), wrep, short, "set")
    perm = np.random.default_rng(6).permutation(len(CFGS)).astype(np.int32)
    inv = np.argsort(perm).astype(np.int32)
    idx2 = np.where((index >= 0) & (index < len(CFGS)), inv[np.clip(index, 0, len(CFGS) - 1)], np.where(index < 0, -1, 999)).astype(np.int32)
    got = tuple(t.cpu().numpy() for t in dset.decode_soft(llr, n_dev, torch.from_numpy(idx2).cuda(), table=torch.from_numpy(perm).cuda()))
    assert len(got) == 3
    assert_equal(got, None, (zeroed, want[1], want[2]), wrep, short, "set with a table")
    # one decoder of the set by itself: its packets' rows repacked to its own symbol size
    i = 1                                                            # (9, 7, 0, ...): 7 of the 10 values per symbol
    mine = np.flatnonzero(index == i)
    own = np.ascontiguousarray(rows[mine, :STRIDE * 7].reshape(len(mine), STRIDE, 7))
    one = tuple(t.cpu().numpy() for t in decoders[i].decode_soft(torch.from_numpy(own).cuda(), torch.from_numpy(nsyms[mine]).cuda(), info=True))
    assert_equal(one[:3], one[3], tuple(x[mine] for x in (zeroed, want[1], want[2])), wrep[mine], [k for k, p in enumerate(mine) if p in short], "one decoder")
    with pytest.raises(ValueError):                                  # a tensor of another width is refused, not read as packed rows
        decoders[i].decode_soft(llr[mine.tolist()], torch.from_numpy(nsyms[mine]).cuda())
    with pytest.raises(ValueError):
        dset.decode_soft(llr, n_dev, i_dev[:-1])
    for d in decoders:
        d._ctx.close()
    dset._ctx.close()


@pytest.mark.parametrize("cfg", [CFGS[16], CFGS[3], CFGS[20]])
def test_uniform_launch_and_every_lane_count(gpu, ctx, cfg):
    """one entry without an index (the uniform launch) over rows of 12, 60, 120 and 260 symbols: 8, 16, 32 and 64 lanes per packet"""
    sf, ppm, rdd, crcc, _, _, explicit, _, dlen = cfg
    W = ppm or sf
    rng = np.random.default_rng(sf * 10 + W)
    for stride in (12, 60, 120, 260):
        rows, nsyms = [], []
        for j in range(9):
            payload = rng.integers(0, 256, int(rng.integers(1, 3 if stride == 12 else 12)) if explicit else dlen, dtype=np.uint8)
            syms, _ = D.build(sf, payload, ppm, int(rng.integers(0, 5)) if rdd < 0 else rdd, bool(explicit), bool(crcc))
            llr = np.zeros((max(stride, syms.size), W), np.float32)
            llr[:syms.size] = S.llr_of_symbols(syms, sf, W)
            llr = (llr + 0.5 * rng.standard_normal(llr.shape).astype(np.float32))[:stride]
            rows.append(llr.reshape(-1)); nsyms.append(min(int(syms.size), stride + 3 * (j % 2)))
        rows = np.stack(rows)
        want, wrep, short = expected([cfg], rows, nsyms, np.zeros(len(rows), np.int32), stride=stride)
        got, rep = soft_launch(gpu, ctx, [cfg], rows, nsyms, None, stride=stride)
        assert_equal(got, rep, want, wrep, short, ("uniform", stride))
    assert (want[1] > 0).any()


# ---- the hard decoder's crafted edge packets through the soft decoder ------------------------------------------------------------------
EDGE_STRIDES = (60, 260)                                             # rows that plan 16 and 64 lanes per packet
EDGE_OUTCOMES = ("header error check", "rdd > 4", ":313", "-2", "crc mismatch", "delivered")


def edge_set(stride):
    """-> cfgs, rows (P, stride * 7) float32, nsyms, index: packets of tests/codec_edge_inputs.py as LLRs that spell their symbols, each of
    a random magnitude in [0.5, 2] (7.0 behind what the row holds of a packet: never read). Set H at (7, 0, 4) and (9, 7, 1), every header
    of the lengths 0..6 over a body of 6 bytes, whole and cut to two interleaver blocks (lengths the packet cannot hold), even lengths under
    crcc + error_check without the header bytes, odd ones under neither with them; set R at (7, 0), 4/4, 4/6 and 4/8, with a length of 200
    beside its 2, 9 and 40 so that rows of 260 symbols are too short for some as rows of 60 are; the one-bit flips in the five header
    codewords of set E's (7, 0) 4/8 packet, which neither H nor R holds: the only packets the header's error check drops."""
    rng = np.random.default_rng(stride)
    cfgs, packets, index = [], [], []
    for sf, ppm, rdd in E.H_CONFIGS[:2]:
        cfgs += [(sf, ppm, rdd, 1, 1, 1, 1, 0, 8), (sf, ppm, rdd, 0, 1, 0, 1, 1, 8)]
        for n_symbols in (None, 2 * (4 + rdd)):
            for j, s in enumerate(E.set_h(sf, ppm, rdd, 6, 6, n_symbols)):
                packets.append((sf, ppm, s)); index.append(len(cfgs) - 2 + (j // 16) % 2)   # (16 headers per length)
    for rdd in (0, 2, 4):
        if rdd != 4:
            cfgs.append((7, 0, rdd, 1, 1, 1, 1, 0, 8))
        for length in (2, 9, 40, 200):
            for s in E.set_r(7, 0, rdd, length)[0]:
                packets.append((7, 0, s)); index.append(0 if rdd == 4 else len(cfgs) - 1)
    flips, labels, _, _ = E.set_e(7, 0, 4, 1, 1)
    for s, (kind, c, _) in zip(flips, labels):
        if kind == "flip" and c < D.N_HDR_CODEWORDS:
            packets.append((7, 0, s)); index.append(0)
    rows = np.full((len(packets), stride * 7), 7.0, np.float32)
    for row, (sf, ppm, s) in zip(rows, packets):
        llr = S.llr_of_symbols(s[:stride], sf, ppm)
        row[:llr.size] = (llr * rng.uniform(0.5, 2.0, llr.shape).astype(np.float32)).reshape(-1)
    return cfgs, rows, np.array([s.size for _, _, s in packets], np.int32), np.array(index, np.int32)


def edge_outcomes(cfgs, index, want, wrep):
    """which packets reach which of EDGE_OUTCOMES, from the definition's results alone"""
    _, n, d = want
    ec = np.array([c[5] for c in cfgs])[index]
    at_header = (d == 1) & (wrep[:, 5] == -1) & (wrep[:, 1] <= 4)       # dropped before the needs were worked out, under a valid rate field
    by_check = at_header & (wrep[:, 4] == 1) & (ec == 1)
    return dict(zip(EDGE_OUTCOMES, (by_check, (d == 1) & (wrep[:, 1] > 4), at_header & ~by_check, n == -2, (d == 1) & (wrep[:, 2] == -1), n > 0)))


@pytest.mark.parametrize("stride", EDGE_STRIDES)
def test_crafted_edge_packets_of_the_hard_decoder(gpu, ctx, stride):
    """Both group decoders run the same header, length, row and checksum stages (lorahip_codec.hip: packetOf .. writePacket), so the packets
    crafted to reach every branch of them in the hard decoder go through the soft one, as one table launch per row length."""
    cfgs, rows, nsyms, index = edge_set(stride)
    assert len(rows) <= 620
    assert E.launch_shape(7, 0, 4, 1, 8, stride)[0] == {60: 16, 260: 64}[stride]
    want, wrep, short = expected(cfgs, rows, nsyms, index, stride=stride)
    for name, hit in edge_outcomes(cfgs, index, want, wrep).items():
        assert hit.any(), (stride, name)
    got, rep = soft_launch(gpu, ctx, cfgs, rows, nsyms, index, stride=stride)
    assert_equal(got, rep, want, wrep, short, ("edges", stride))


@pytest.mark.parametrize("explicit", [1, 0])
def test_unit_llrs_of_clean_symbols_give_the_hard_decoders_result(gpu, explicit):
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(77 + explicit)
    for sf, ppm in ((7, 0), (9, 7)):
        W = ppm or sf
        for cr, rdd in (("4/4", 0), ("4/5", 1), ("4/6", 2), ("4/7", 3), ("4/8", 4)):
            packets = [D.build(sf, rng.integers(0, 256, 7, dtype=np.uint8), ppm, rdd, bool(explicit), True)[0] for _ in range(6)]
            stride = max(p.size for p in packets) + 2
            host = np.zeros((len(packets), stride), np.uint16)
            for i, p in enumerate(packets):
                host[i, :p.size] = p
            nsyms = torch.from_numpy(np.array([p.size for p in packets], np.int32)).cuda()
            dec = L.LoRaDecoder()
            dec.setSpreadFactor(sf); dec.setSymbolSize(ppm); dec.setCodingRate(cr); dec.enableExplicit(bool(explicit)); dec.enableCrcc(True)
            dec.enableErrorCheck(True); dec.setDataLength(7)
            hard = dec.decode_batch(torch.from_numpy(host.view(np.int16)).cuda(), nsyms, info=True)
            llr = S.llr_of_symbols(host, sf, W)
            for i, p in enumerate(packets):
                llr[i, p.size:] = 0                                  # nothing is read behind a packet's symbols
            soft = dec.decode_soft(torch.from_numpy(llr).cuda(), nsyms, info=True)
            for a, b in zip(hard, soft):
                assert torch.equal(a, b), (sf, ppm, cr, explicit)
            assert (hard[1].cpu().numpy() == (7 if explicit else 9)).all()       # (without a header the two crc bytes are posted too)
            dec._ctx.close()


def test_refusals(gpu, ctx):
    import lora_sdr_amd as L
    torch = gpu
    dec = L.LoRaDecoder()
    dec.enableInterleaving(False)
    llr = torch.zeros((2, 16, 10), dtype=torch.float32, device="cuda")
    n = torch.full((2,), 16, dtype=torch.int32, device="cuda")
    with pytest.raises(L.LoraHipError):
        dec.decode_soft(llr, n)
    dec.enableInterleaving(True)
    assert dec.decode_soft(llr, n)[1].cpu().numpy().tolist() == dec.decode_batch(torch.zeros((2, 16), dtype=torch.int16, device="cuda"), n)[1].cpu().numpy().tolist()
    # a row too short for sym_stride symbols of the entry's size; no packets is no work
    lib, h = ctx._lib, ctx._h
    cfg = T.cfg_array([CFGS[0]])
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.zeros((2, 48), dtype=torch.uint8, device="cuda")
    ol = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, p(llr), 16 * 7 - 1, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == -1
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, None, 16 * 7, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == -1
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, p(llr), 0, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == -1
    wide = torch.zeros(2 * 16 * 12 * 8, dtype=torch.float32, device="cuda")       # the widest row stride taken
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, p(wide), 16 * 12 * 8, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == 0
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, p(llr), 16 * 12 * 8 + 1, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == -1
    assert lib.lorahip_decode_packets_soft_host(h, cfg, 1, None, None, 0, None, 1 << 62, 16, None, 1 << 30, None, 48, None, None, None) == -1
    assert lib.lorahip_decode_packets_soft(h, cfg, 1, None, None, 0, None, 16 * 7, 16, None, 0, None, 48, None, None, None) == 0
    off = T.cfg_array([CFGS[0][:4] + (0,) + CFGS[0][5:]])
    assert lib.lorahip_decode_packets_soft(h, off, 1, None, None, 0, p(llr), 16 * 7, 16, p(n), 2, p(out), 48, p(ol), p(ol), None) == -1
    dec._ctx.close()


# ---- LLRs that are not finite -----------------------------------------------------------------------------------------------------------
NF_STRIDE = 40
NF_CFGS = [(7, 0, 1, 1, 1, 0, 1, 0, 0), (7, 0, 4, 1, 1, 1, 1, 0, 0)]            # 4/5 and 4/8, explicit header, crcc on; error_check off / on
NF_PLACES = (("header codeword", 2, 3), ("payload codeword", 9, 2), ("header symbol", 3, None), ("payload symbol", 10, None))
NF_VALUES = ("nan", "+inf", "-inf", "inf of the sent sign")


def non_finite_set():
    """-> rows (P, NF_STRIDE * 7) float32, nsyms, index, payloads, labels: per rate one valid packet as LLRs of magnitude 0.5..2 that spell
    its symbols, then the same packet with one LLR (symbol s, bit m) -- which lands in one codeword of the header block / of a payload
    block -- or one whole symbol (a bit of every codeword of its block) overwritten by NaN, +Inf, -Inf, or the infinity of the sign it had"""
    rng = np.random.default_rng(99)
    rows, nsyms, index, payloads, labels = [], [], [], [], []
    for i, cfg in enumerate(NF_CFGS):
        sf, ppm, rdd = cfg[:3]
        payload = rng.integers(0, 256, 6, dtype=np.uint8)
        syms, _ = D.build(sf, payload, ppm, rdd, True, True)
        assert 10 < syms.size <= NF_STRIDE
        base = np.zeros((NF_STRIDE, sf), np.float32)
        base[:syms.size] = S.llr_of_symbols(syms, sf, sf) * rng.uniform(0.5, 2.0, (syms.size, sf)).astype(np.float32)
        variants = [("untouched", base)]
        for place, s, m in NF_PLACES:
            for value in NF_VALUES:
                llr = base.copy()
                at = (s, slice(None) if m is None else m)
                llr[at] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}.get(value, np.float32(np.inf) * np.sign(llr[at]))
                variants.append((place + ": " + value, llr))
        for label, llr in variants:
            rows.append(llr.reshape(-1)); nsyms.append(syms.size); index.append(i); payloads.append(payload); labels.append((cfg[2], label))
    return np.stack(rows), np.array(nsyms, np.int32), np.array(index, np.int32), payloads, labels


def test_llrs_that_are_not_finite_decode_as_the_definition(gpu, ctx):
    """NaN and infinite LLRs (lorahip_soft_symbols gives them for windows with infinite bins): the nibble rule of include/lorahip.h --
    x = 0 the incumbent, replaced only by a greater metric, so a NaN metric never wins and a NaN M(0) stays; the hard bit llr > 0"""
    rows, nsyms, index, payloads, labels = non_finite_set()
    assert not np.isfinite(rows).all()
    want, wrep, short = expected(NF_CFGS, rows, nsyms, index, stride=NF_STRIDE)
    out, n, d = want
    # the set, judged by the definition alone: the untouched packets decode to their payload; at either rate a touched packet is dropped,
    # and a touched packet still decodes. (An infinite LLR of the sign that was sent does not help: every x whose codeword agrees in
    # that bit scores +Inf, they tie, and the smallest wins.)
    assert not short
    touched = np.array([label != "untouched" for _, label in labels])
    for p in np.flatnonzero(~touched):
        assert n[p] == 6 and d[p] == 0 and np.array_equal(out[p, :6], payloads[p]), labels[p]
    for rdd in (1, 4):
        assert (d[touched & np.array([r == rdd for r, _ in labels])] == 1).any(), rdd
    assert any(n[p] == 6 and np.array_equal(out[p, :6], payloads[p]) for p in np.flatnonzero(touched))
    got, rep = soft_launch(gpu, ctx, NF_CFGS, rows, nsyms, index, stride=NF_STRIDE)
    assert_equal(got, rep, want, wrep, short, "not finite, device")
    got, rep = soft_launch(gpu, ctx, NF_CFGS, rows, nsyms, index, host=True, stride=NF_STRIDE)
    assert_equal(got, rep, want, wrep, short, "not finite, host")
