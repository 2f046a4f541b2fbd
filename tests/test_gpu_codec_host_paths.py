"""The host-pointer forms of the batched decoder and encoder share ONE trip through the context's staging pair (lorahip_codec_api.cpp:
Staged). What that makes common and no other test pins, on SF7 packets of 4..20 bytes in rows of 64 symbols:

    the uniform host form, lorahip_decode_packets_host, against lorahip_decode_packets, packet for packet (out[:out_len], out_len, dropped;
        the bytes of a row behind out_len are unspecified in the host form)
    stage reuse: four host calls of different shapes on one context, each against the same call on a fresh context
    absent pieces: no table and no report, both, no index (the uniform form of lorahip_decode_packets_info_host), no payload bytes
        (lorahip_encode_packets_host with byte_stride 0) -- each against its device form
    a configuration that is refused (rdd = 7) by every host form on a live context, and a good call behind it"""
import ctypes as C

import numpy as np
import pytest

import codec_edge_inputs as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ROW = 64
# (sf, ppm, rdd, crcc, interleaving, error_check, explicit_hdr, hdr, data_length): 4/8, 4/5, and the rate each packet's header names
DEC = [(7, 0, 4, 1, 1, 0, 1, 0, 8), (7, 0, 1, 1, 1, 0, 1, 0, 8), (7, 0, -1, 1, 1, 0, 1, 0, 8)]
RATE_OF = (4, 1, 2)                                                 # what the packets of each entry are encoded at
# (sf, ppm, rdd, explicit_hdr, crc, whitening)
ENC = [(7, 0, 4, 1, 1, 1), (7, 0, 1, 1, 1, 1)]


def dec_cfgs(cfgs):
    from lora_sdr_amd import _lib
    arr = (_lib.DecoderCfg * len(cfgs))()
    for i, c in enumerate(cfgs):
        arr[i] = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), *c)
    return arr


def enc_cfgs(cfgs):
    from lora_sdr_amd import _lib
    arr = (_lib.EncoderCfg * len(cfgs))()
    for i, c in enumerate(cfgs):
        arr[i] = _lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), *c)
    return arr


class Bufs:
    """numpy arrays where an entry point wants them: as they are (a host form), or as device copies that back() copies home"""

    def __init__(self, torch, on_device):
        self.torch, self.on_device, self.pairs = torch, on_device, []

    def ptr(self, a):
        if a is None:
            return None
        assert a.flags["C_CONTIGUOUS"]
        if not self.on_device:
            return a.ctypes.data
        t = self.torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
        self.pairs.append((a, t))
        return t.data_ptr()

    def back(self):
        for a, t in self.pairs:
            a.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()


def decode(torch, ctx, name, cfgs, rows, nsyms, index=None, table=None, info=False):
    """entry point `name` (a device or a _host form) on outputs filled with 0xA5 / -77 -> (rc, (out, out_len, dropped, report or None))"""
    P, stride = rows.shape
    out_stride = 2 * (stride + 8)
    out, n, d = np.full((P, out_stride), SENTINEL, np.uint8), np.full(P, -77, np.int32), np.full(P, -77, np.int32)
    rep = np.full((P, 8), -77, np.int32) if info else None
    b = Bufs(torch, not name.endswith("_host"))
    args = [b.ptr(rows), stride, b.ptr(nsyms), P, b.ptr(out), out_stride, b.ptr(n), b.ptr(d)]
    if name.startswith("lorahip_decode_packets_cfgs") or name.startswith("lorahip_decode_packets_info"):
        args = [len(cfgs), b.ptr(index), b.ptr(table), 0 if table is None else table.size] + args
        if name.startswith("lorahip_decode_packets_info"):
            args.append(b.ptr(rep))
    ctx.set_variant(0); ctx.use_torch_stream()
    rc = getattr(ctx._lib, name)(ctx._h, dec_cfgs(cfgs), *args)
    b.back()
    return rc, (out, n, d, rep)


def encode(torch, ctx, name, cfgs, data, nbytes, index=None, table=None, sym_stride=ROW):
    """entry point `name` (a device or a _host form) on outputs filled with 0xA5A5 / -77 -> (rc, (syms, nsyms)); data None: byte_stride 0"""
    P = nbytes.size
    syms, n = np.full((P, sym_stride), 0xA5A5, np.uint16), np.full(P, -77, np.int32)
    b = Bufs(torch, not name.endswith("_host"))
    args = [b.ptr(data), 0 if data is None else data.shape[1], b.ptr(nbytes), P, b.ptr(syms), sym_stride, b.ptr(n)]
    if name.startswith("lorahip_encode_packets_cfgs"):
        args = [len(cfgs), b.ptr(index), b.ptr(table), 0 if table is None else table.size] + args
    ctx.use_torch_stream()
    rc = getattr(ctx._lib, name)(ctx._h, enc_cfgs(cfgs), *args)
    b.back()
    return rc, (syms, n)


def assert_same(a, b, tag):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (tag, i)
        if x is not None:
            bad = np.flatnonzero((x != y).reshape(x.shape[0], -1).any(axis=1))
            assert bad.size == 0, (tag, "array", i, "packet", int(bad[0]), x[bad[0]], y[bad[0]])


def posted(res):
    """a uniform decode with what the host form leaves unspecified taken out: the bytes of every row behind out_len"""
    out, n, d = res[0].copy(), res[1], res[2]
    for p in range(n.size):
        out[p, max(0, int(n[p])):] = 0
    return out, n, d


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as L
    return L.Context(7)                                              # device, stream and staging pair only


@pytest.fixture(scope="module")
def packets(gpu):
    """per coding rate of RATE_OF: rows of 8 packets of 4..20 bytes from the encoder; packet 1 with one flipped symbol bit, packet 4 with
    bit 3 of every payload symbol flipped (one wrong bit in most codewords: beyond 4/5 and 4/6, so the crc drops it there)"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(20)
    sets = {}
    for rdd in RATE_OF:
        enc = L.LoRaEncoder()
        enc.setSpreadFactor(7); enc.setCodingRate(S.RDD_TO_CR[rdd])
        syms = [np.array(s, np.uint16) for s in enc.work([rng.integers(0, 256, int(k)).astype(np.uint8) for k in rng.integers(4, 21, 8)])]
        syms[1][int(rng.integers(8, syms[1].size))] ^= np.uint16(1 << int(rng.integers(0, 7)))
        syms[4][8:] ^= np.uint16(1 << 3)
        assert max(s.size for s in syms) <= ROW
        sets[rdd] = S.as_rows(syms, ROW)
    return sets


@pytest.fixture(scope="module")
def mixed(packets):
    """8 rows for the table DEC: packet p under entry index[p] (through a table: entry table[index[p]]), packet 5 without an entry"""
    index = np.array([0, 1, 2, 0, 1, 3, 2, 1], np.int32)
    pick = [RATE_OF[i % 3] for i in index]
    rows = np.stack([packets[r][0][p] for p, r in enumerate(pick)])
    nsyms = np.array([packets[r][1][p] for p, r in enumerate(pick)], np.int32)
    table = np.array([2, 0, 1, 7], np.int32)                        # entry of index value: a permutation, and one entry out of range
    via_table = np.array([1, 2, 0, 1, 2, 3, 0, 2], np.int32)        # table[via_table[p]] == index[p] where that is an entry
    assert all(table[v] == i for v, i in zip(via_table, index) if i < 3)
    return rows, nsyms, index, table, via_table


def test_uniform_host_form_equals_the_device_form(gpu, ctx, packets):
    decoded = dropped = 0
    for cfg, rdd in zip(DEC, RATE_OF):
        rows, nsyms = packets[rdd]
        rc_d, dev = decode(gpu, ctx, "lorahip_decode_packets", [cfg], rows, nsyms)
        rc_h, host = decode(gpu, ctx, "lorahip_decode_packets_host", [cfg], rows, nsyms)
        assert (rc_d, rc_h) == (0, 0), ctx._lib.lorahip_last_error()
        assert_same(posted(host), posted(dev), ("uniform", cfg))
        assert (dev[1] != -77).all() and (dev[2] != -77).all()
        decoded, dropped = decoded + int((dev[1] > 0).sum()), dropped + int(dev[2].sum())
    assert decoded >= 12 and dropped >= 1                            # (both outcomes were compared)


def _sequence(packets, mixed):
    """the four host calls of the stage-reuse test: (tag, call(torch, ctx) -> comparable arrays)"""
    rows, nsyms, index, table, via_table = mixed
    rng = np.random.default_rng(21)
    data, nbytes = np.zeros((3, 64), np.uint8), np.array([4, 20, 11], np.int32)
    for p in range(3):
        data[p, :nbytes[p]] = rng.integers(0, 256, nbytes[p])

    def table_decode(torch, c):
        rc, res = decode(torch, c, "lorahip_decode_packets_info_host", DEC, rows, nsyms, via_table, table, info=True)
        assert rc == 0, c._lib.lorahip_last_error()
        return res

    def uniform_decode(torch, c):
        rc, res = decode(torch, c, "lorahip_decode_packets_host", [DEC[0]], packets[4][0][:1], packets[4][1][:1])
        assert rc == 0, c._lib.lorahip_last_error()
        return posted(res)

    def encode3(torch, c):
        rc, res = encode(torch, c, "lorahip_encode_packets_host", [ENC[0]], data, nbytes)
        assert rc == 0, c._lib.lorahip_last_error()
        return res

    return [("table decode", table_decode), ("uniform decode", uniform_decode), ("encode", encode3), ("table decode again", table_decode)]


def test_stage_reuse_across_calls_of_different_shapes(gpu, packets, mixed):
    import lora_sdr_amd as L
    shared = L.Context(7)
    for tag, call in _sequence(packets, mixed):
        got = call(gpu, shared)
        fresh = L.Context(7)
        assert_same(got, call(gpu, fresh), tag)
        fresh.close()
    shared.close()


def test_absent_pieces_equal_the_device_forms(gpu, ctx, packets, mixed):
    rows, nsyms, index, table, via_table = mixed
    for tag, idx, tab, info in (("no table, no report", index, None, False), ("table and report", via_table, table, True)):
        rc_d, dev = decode(gpu, ctx, "lorahip_decode_packets_info", DEC, rows, nsyms, idx, tab, info)
        rc_h, host = decode(gpu, ctx, "lorahip_decode_packets_info_host", DEC, rows, nsyms, idx, tab, info)
        assert (rc_d, rc_h) == (0, 0), ctx._lib.lorahip_last_error()
        assert_same(host, dev, tag)                                  # (whole rows: they travel both ways, the row without an entry included)
        assert dev[1][5] == -3 and (dev[0][5] == SENTINEL).all() and (dev[1][[0, 3, 6]] > 0).all()
    u_rows, u_n = packets[4]
    rc_d, dev = decode(gpu, ctx, "lorahip_decode_packets_info", [DEC[0]], u_rows, u_n, None, None, True)
    rc_h, host = decode(gpu, ctx, "lorahip_decode_packets_info_host", [DEC[0]], u_rows, u_n, None, None, True)
    assert (rc_d, rc_h) == (0, 0), ctx._lib.lorahip_last_error()
    assert_same(host, dev, "no index: the uniform launch")
    assert (dev[1] > 0).sum() >= 6 and (dev[3][:, 0] >= 4).sum() >= 6   # (lengths announced in the report)
    # messages of no bytes, crc on: nothing to upload but the lengths
    nbytes = np.zeros(5, np.int32)
    rc_d, dev = encode(gpu, ctx, "lorahip_encode_packets", [ENC[0]], None, nbytes)
    rc_h, host = encode(gpu, ctx, "lorahip_encode_packets_host", [ENC[0]], None, nbytes)
    assert (rc_d, rc_h) == (0, 0), ctx._lib.lorahip_last_error()
    assert_same(host, dev, "no payload bytes")
    assert (dev[1] == 16).all()                                     # 2 crc bytes and 5 header codewords: two blocks of SF7


def test_refused_configuration_then_a_good_call(gpu, ctx, packets, mixed):
    rows, nsyms, index, table, via_table = mixed
    bad_dec = [DEC[0], DEC[1][:2] + (7,) + DEC[1][3:]]
    bad_enc = [ENC[0], ENC[1][:2] + (7,) + ENC[1][3:]]
    rng = np.random.default_rng(22)
    data, nbytes = rng.integers(0, 256, (4, 20)).astype(np.uint8), np.array([20, 4, 9, 15], np.int32)
    e_index = np.array([0, 1, 1, 0], np.int32)
    u_rows, u_n = packets[4]
    cases = [
        ("lorahip_decode_packets_host", lambda name, bad: decode(gpu, ctx, name, bad_dec[1:] if bad else [DEC[0]], u_rows, u_n)),
        ("lorahip_decode_packets_cfgs_host", lambda name, bad: decode(gpu, ctx, name, bad_dec if bad else DEC, rows, nsyms, index)),
        ("lorahip_decode_packets_info_host", lambda name, bad: decode(gpu, ctx, name, bad_dec if bad else DEC, rows, nsyms, via_table, table, True)),
        ("lorahip_encode_packets_host", lambda name, bad: encode(gpu, ctx, name, bad_enc[1:] if bad else [ENC[0]], data, nbytes)),
        ("lorahip_encode_packets_cfgs_host", lambda name, bad: encode(gpu, ctx, name, bad_enc if bad else ENC, data, nbytes, e_index)),
    ]
    for name, call in cases:
        want = call(name[:-len("_host")], False)                     # the device form under the good configuration
        assert want[0] == 0, ctx._lib.lorahip_last_error()
        rc, res = call(name, True)
        assert rc == -1, name
        for a in res:                                                # (refused: the caller's arrays are as they were)
            assert a is None or (a == (-77 if a.dtype == np.int32 else 0xA5A5 if a.dtype == np.uint16 else SENTINEL)).all(), name
        rc, res = call(name, False)
        assert rc == 0, ctx._lib.lorahip_last_error()
        if name == "lorahip_decode_packets_host":
            assert_same(posted(res), posted(want[1]), name)
        else:
            assert_same(res, want[1], name)
