"""GPU: the encoder with the configuration per packet (lorahip_encode_packets_cfgs, LoRaEncoderSet) against the uniform launch of each
entry (lorahip_encode_packets, itself pinned to the verbatim LoRaEncoder.cpp by tests/test_gpu_encoder.py) and, where a message leaves
no pad nibbles, against the verbatim encoder directly. Everything compared is integer and exact: whole symbol rows and counts."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_encoder import encoder, pad_nibbles, rows

pytestmark = pytest.mark.gpu

FILL = 0xA5A5


def entries(L):
    """SF7..12 x 4/5 and 4/8 (explicit header, crc), one entry without a header and one with ppm = sf - 2:
    [(sf, ppm, cr, explicit, crc)], the encoders in the same order"""
    spec = [(sf, 0, cr, True, True) for sf in range(7, 13) for cr in ("4/5", "4/8")]
    spec += [(9, 0, "4/7", False, True), (10, 8, "4/6", True, True)]
    return spec, [encoder(L, *s) for s in spec]


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def uniform_rows(encs, data, nb, sym_stride):
    """[(syms, nsyms) of encs[i].encode_batch over ALL the rows]: what every row must equal under entry i"""
    return [(u16(s), n.cpu().numpy()) for s, n in (e.encode_batch(data, nb, sym_stride=sym_stride) for e in encs)]


def dev_i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


@pytest.fixture(scope="module")
def set1(gpu):
    """about 200 packets of 0..40 bytes in shuffled order over the 14 entries, every entry used; the table launch and the uniform launches"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(20)
    spec, encs = entries(L)
    lens = rng.permutation(np.tile(np.arange(41), 5))[:200]
    msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in lens]
    index = rng.permutation(np.arange(200) % len(encs)).astype(np.int32)
    data, nb = rows(gpu, msgs, stride=40)
    es = L.LoRaEncoderSet(encs)
    S = es.max_symbols(40)
    syms, nsyms = es.encode_batch(data, nb, dev_i32(gpu, index))
    assert tuple(syms.shape) == (200, S)
    return dict(spec=spec, encs=encs, msgs=msgs, index=index, data=data, nb=nb, S=S, syms=u16(syms), nsyms=nsyms.cpu().numpy(),
                uni=uniform_rows(encs, data, nb, S))


def test_every_row_equals_the_uniform_launch_of_its_entry(set1):
    s = set1
    assert set(s["index"].tolist()) == set(range(len(s["encs"])))
    for p, i in enumerate(s["index"]):
        us, un = s["uni"][i]
        assert s["nsyms"][p] == un[p], (p, s["spec"][i], len(s["msgs"][p]))
        assert np.array_equal(s["syms"][p], us[p]), (p, s["spec"][i], len(s["msgs"][p]))         # the whole row, zeros behind the packet included
    assert (s["nsyms"] >= 8).all()                                                               # header or crc everywhere: nothing undefined


def test_rows_without_pad_nibbles_equal_the_verbatim_encoder(set1, ref):
    s = set1
    compared = 0
    for p, i in enumerate(s["index"]):
        sf, ppm, cr, explicit, crc = s["spec"][i]
        m = s["msgs"][p]
        if pad_nibbles(len(m), sf, ppm, explicit, crc):
            continue
        want = ref.encode(sf, m, ppm=ppm, cr=cr, explicit=explicit, crc=crc)
        assert s["nsyms"][p] == len(want) and np.array_equal(s["syms"][p, :len(want)], want), (p, s["spec"][i], len(m))
        compared += 1
    assert compared >= 10, compared


@pytest.mark.parametrize("sym_stride", [16, 64, 160, 512])
def test_unlike_neighbours_at_every_lane_count(gpu, sym_stride):
    """SF7 4/5 next to SF12 4/8, alternating, in rows of 16 / 64 / 160 / 512 symbols: the launches run 8 / 16 / 32 / 64 lanes per packet
    (the rows bound what a packet can be, the byte stride of 255 does not), more than one workgroup each; messages that do not fit the
    rows are the uniform launch's -2 and zero row"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(sym_stride)
    encs = [encoder(L, 7, 0, "4/5", True, True), encoder(L, 12, 0, "4/8", True, True)]
    most = {16: 8, 64: 48, 160: 130, 512: 255}[sym_stride]
    P = 70
    msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in rng.integers(0, most + 1, P)]
    index = (np.arange(P) % 2).astype(np.int32)
    index[40:] = 1 - index[40:]                                     # both parities of the group number see both entries
    data, nb = rows(gpu, msgs, stride=255)
    syms, nsyms = L.LoRaEncoderSet(encs).encode_batch(data, nb, dev_i32(gpu, index), sym_stride=sym_stride)
    syms, nsyms = u16(syms), nsyms.cpu().numpy()
    uni = uniform_rows(encs, data, nb, sym_stride)
    for p, i in enumerate(index):
        assert nsyms[p] == uni[i][1][p] and np.array_equal(syms[p], uni[i][0][p]), (p, i, len(msgs[p]))
    assert (nsyms > 0).sum() >= P // 3 and ((nsyms == -2).any() or sym_stride == 512)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 65])
def test_missing_entries_and_nothing_behind_the_rows(gpu, P):
    """index -1 and n_cfgs, and a table entry out of range: -3 and a zero row, the neighbours the uniform launch's rows; symbol rows and
    counts pre-filled with 0xA5A5: nothing is written behind the P rows of sym_stride symbols or behind the P counts"""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(300 + P)
    encs = [encoder(L, 8, 0, "4/6", True, True), encoder(L, 11, 9, "4/8", True, False), encoder(L, 7, 0, "4/5", False, True)]
    es = L.LoRaEncoderSet(encs)
    msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in rng.integers(0, 25, P)]
    data, nb = rows(torch, msgs, stride=24)
    S = es.max_symbols(24)
    index = rng.integers(0, 3, P).astype(np.int32)
    for p, bad in ((0, -1), (P // 2, 3), (P - 1, -2 ** 31), (P // 3, 2 ** 31 - 1)):
        index[p] = bad
    uni = uniform_rows(encs, data, nb, S)
    lib = L.load()

    def launch(idx, table):
        buf = torch.full(((P + 3) * S + 5,), FILL - 0x10000, dtype=torch.int16, device="cuda")
        cnt = torch.full((P + 7,), FILL, dtype=torch.int32, device="cuda")
        di = dev_i32(torch, idx)
        dt = None if table is None else dev_i32(torch, table)
        es._ctx.use_torch_stream()
        rc = lib.lorahip_encode_packets_cfgs(es._ctx._h, es._cfgs, 3, C.c_void_p(di.data_ptr()), None if dt is None else C.c_void_p(dt.data_ptr()),
                                             0 if dt is None else dt.numel(), C.c_void_p(data.data_ptr()), 24, C.c_void_p(nb.data_ptr()), P,
                                             C.c_void_p(buf.data_ptr()), S, C.c_void_p(cnt.data_ptr()))
        assert rc == 0
        torch.cuda.synchronize()
        got, n = u16(buf), cnt.cpu().numpy()
        assert (got[P * S:] == FILL).all() and (n[P:] == FILL).all()
        return got[:P * S].reshape(P, S), n[:P]

    def compare(got, n, entry_of):
        for p in range(P):
            i = entry_of[p]
            if i is None:
                assert n[p] == -3 and not got[p].any(), p
            else:
                assert n[p] == uni[i][1][p] and np.array_equal(got[p], uni[i][0][p]), (p, i)

    got, n = launch(index, None)
    compare(got, n, [int(i) if 0 <= i < 3 else None for i in index])
    # the same through a table: index -> table -> entry; a table index out of range, and a table ENTRY out of range
    table = np.array([2, 0, 7, 1, -1, 0], np.int32)
    tindex = rng.integers(0, 6, P).astype(np.int32)
    tindex[0], tindex[P - 1] = 6, -1
    got, n = launch(tindex, table)
    compare(got, n, [(int(table[j]) if 0 <= table[j] < 3 else None) if 0 <= j < 6 else None for j in tindex])
    if P >= 31:
        assert (n == -3).sum() >= 3 and (n >= 8).sum() >= 3


def test_one_entry_table_equals_the_uniform_entry_point(gpu):
    import lora_sdr_amd as L
    rng = np.random.default_rng(4)
    for spec in ((7, 0, "4/5", True, True), (12, 10, "4/8", True, True), (9, 0, "4/4", False, False)):
        e = encoder(L, *spec)
        msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in list(range(0, 41)) + [100, 255]]
        data, nb = rows(gpu, msgs)
        us, un = e.encode_batch(data, nb)
        zeros = gpu.zeros(len(msgs), dtype=gpu.int32, device="cuda")
        ts, tn = L.LoRaEncoderSet([e]).encode_batch(data, nb, zeros)
        assert ts.shape == us.shape and np.array_equal(u16(ts), u16(us)) and np.array_equal(tn.cpu().numpy(), un.cpu().numpy()), spec
        ts, tn = L.LoRaEncoderSet([e]).encode_batch(data, nb, zeros + 5, table=dev_i32(gpu, [9, 9, 9, 9, 9, 0]))
        assert np.array_equal(u16(ts), u16(us)) and np.array_equal(tn.cpu().numpy(), un.cpu().numpy()), spec


def test_host_form_equals_device_form(gpu):
    import lora_sdr_amd as L
    lib = L.load()
    rng = np.random.default_rng(5)
    spec, encs = entries(L)
    es = L.LoRaEncoderSet(encs)
    P = 45
    msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in rng.integers(0, 65, P)]
    hb = np.zeros((P, 64), np.uint8)
    for i, m in enumerate(msgs):
        hb[i, :len(m)] = m
    hn = np.array([len(m) for m in msgs], np.int32)
    for table in (None, rng.integers(-1, len(encs) + 1, 20).astype(np.int32)):
        idx = rng.integers(-1, (len(encs) if table is None else 20) + 1, P).astype(np.int32)
        d_s, d_n = es.encode_batch(gpu.from_numpy(hb).cuda(), gpu.from_numpy(hn).cuda(), dev_i32(gpu, idx),
                                   table=None if table is None else dev_i32(gpu, table), sym_stride=200)
        hs, hl = np.full((P + 1, 200), FILL, np.uint16), np.full(P + 1, FILL, np.int32)
        rc = lib.lorahip_encode_packets_cfgs_host(es._ctx._h, es._cfgs, len(encs), idx.ctypes.data, None if table is None else table.ctypes.data,
                                                  0 if table is None else table.size, hb.ctypes.data, 64, hn.ctypes.data, P, hs.ctypes.data, 200,
                                                  hl.ctypes.data)
        assert rc == 0
        assert np.array_equal(hs[:P], u16(d_s)) and np.array_equal(hl[:P], d_n.cpu().numpy())
        assert (hs[P] == FILL).all() and hl[P] == FILL and (hl[:P] == -3).any() and (hl[:P] >= 8).any()


def test_host_refusals(gpu):
    """a bad entry that no packet uses, n_cfgs 0 and 65, a table of no entries: LORAHIP_E_INVALID and nothing written"""
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    torch = gpu
    e = encoder(L, 8, 0, "4/6", True, True)
    data, nb = rows(torch, [np.arange(5, dtype=np.uint8)] * 4, stride=8)
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    syms = torch.full((4, 40), FILL - 0x10000, dtype=torch.int16, device="cuda")
    cnt = torch.full((4,), FILL, dtype=torch.int32, device="cuda")

    def call(cfgs, n_cfgs, table=None, n_table=0, byte_stride=8, sym_stride=40):
        e._ctx.use_torch_stream()
        return lib.lorahip_encode_packets_cfgs(e._ctx._h, cfgs, n_cfgs, C.c_void_p(idx.data_ptr()), table, n_table, C.c_void_p(data.data_ptr()),
                                               byte_stride, C.c_void_p(nb.data_ptr()), 4, C.c_void_p(syms.data_ptr()), sym_stride, C.c_void_p(cnt.data_ptr()))
    many = (_lib.EncoderCfg * 65)(*([e._cfg] * 65))
    assert call(many, 0) == -1 and call(many, 65) == -1 and call(None, 1) == -1
    for field, value in (("struct_size", 8), ("sf", 13), ("sf", 0), ("ppm", 9), ("rdd", 5), ("rdd", -1)):
        two = (_lib.EncoderCfg * 2)(e._cfg, e._cfg)
        setattr(two[1], field, value)                               # entry 1: no packet names it
        assert call(two, 2) == -1, field
    assert call(many, 2, table=C.c_void_p(idx.data_ptr()), n_table=0) == -1
    assert call(many, 2, byte_stride=lib.lorahip_encode_max_bytes() + 1) == -1 and call(many, 2, sym_stride=0) == -1
    torch.cuda.synchronize()
    assert (u16(syms) == FILL).all() and (cnt.cpu().numpy() == FILL).all()
    assert call(many, 64) == 0                                      # 64 entries travel in the kernel's arguments
    torch.cuda.synchronize()
    want_s, want_n = e.encode_batch(data, nb, sym_stride=40)
    assert np.array_equal(u16(syms), u16(want_s)) and np.array_equal(cnt.cpu().numpy(), want_n.cpu().numpy())


def test_encoder_set_surface(gpu):
    import lora_sdr_amd as L
    rng = np.random.default_rng(7)
    spec, encs = entries(L)
    es = L.LoRaEncoderSet(encs)
    assert len(es) == len(encs) and es.spread_factors == [s[0] for s in spec]
    for i, e in enumerate(encs):
        for n in (0, 1, 20, 255):
            assert es.num_symbols(i, n) == e.num_symbols(n)
    assert es.max_symbols(20) == max(e.num_symbols(20) for e in encs)
    msgs = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in rng.integers(1, 30, 30)]
    index = rng.integers(0, len(encs), 30)
    out = es.work([bytes(m) for m in msgs], index)
    for m, i, o in zip(msgs, index, out):
        assert np.array_equal(o, encs[i].work([m])[0])
    assert es.work([], []) == []
    # the configurations were copied: a later setter call on a member does not reach the set
    encs[0].setSpreadFactor(12)
    assert es.spread_factors[0] == 7 and np.array_equal(es.work([msgs[0]], [0])[0], L.LoRaEncoderSet([encoder(L, *spec[0])]).work([msgs[0]], [0])[0])
    with pytest.raises(ValueError):
        es.work([b"abc"], [len(encs)])
    with pytest.raises(ValueError):
        es.work([b"abc"], [-1])
    with pytest.raises(ValueError):
        es.work([b"abc", b"d"], [0])
    with pytest.raises(ValueError):
        L.LoRaEncoderSet([])
    with pytest.raises(ValueError):
        L.LoRaEncoderSet([encs[1]] * 65)
    nohdr = L.LoRaEncoderSet([encoder(L, 8, 0, "4/6", False, False), encs[1]])
    assert nohdr.work([b"", b"abc"], [0, 1])[0] is None             # the reference's undefined case stays -1
