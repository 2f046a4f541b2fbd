"""GPU: lorahip_rx_info (end_pos, data_pos, sync_pos, freq_error per packet) and the signals' positions through every path that
delivers packets or signals -- the host queue, the device hand-off, the receiver steps, the segment runs, a mixed handle, the scheduled
transmitter's frames -- with integer equality against the definition (tests/rx_info_def.py) evaluated on the CPU oracle's call trace
(the restated block, pinned to the verbatim LoRaDemod.cpp)."""
import ctypes as C

import numpy as np
import pytest

import rx_info_def as D
from test_gpu_demod import MODES
from test_gpu_receiver import _streams

pytestmark = pytest.mark.gpu

AHEAD = 16
MTU = 8


def _want(oracle, sf, host, mtu=MTU, thresh=-30.0):
    """per channel: (info (P, 4), signal positions (S,), the oracle's run)"""
    out = []
    for c in range(host.shape[0]):
        r = oracle.demod_run(sf, host[c], mtu=mtu, thresh=thresh, keep=False)
        info, pos = D.from_oracle(r)
        out.append((info, pos, r))
    return out


def _by_channel(chan, rows, B):
    chan = np.asarray(chan)
    return [np.asarray(rows)[chan == c] for c in range(B)]


def _check_one_shot(gpu, L, d, iq, want, B, sf):
    """a one-shot work() of `d` with signals kept: queue info == hand-off info == the definition, signal positions, the join"""
    d.set_signals(True)
    d.work(iq)
    consumed = d.consumed_all()
    # first of all, while a streaming run's records are still on the device: the hand-off packs them there
    dsy, dns, dch, dinfo = d.packets_device(stride=MTU, clear=False, info=True)
    sch, srd, ser, spw, ssn, sps = d.signals(pos=True)
    ch, rd, ln, sy, info = d.packets_arrays(clear=False, info=True)
    assert info.dtype == np.int64 and info.shape == (ch.size, 4) and sps.dtype == np.int64
    assert dinfo.dtype == gpu.int64 and tuple(dinfo.shape) == (ch.size, 4)
    # ... and now that the queue is on the host, the hand-off uploads from it, in the queue's order
    usy, uns, uch, uinfo = d.packets_device(stride=MTU, clear=False, info=True)
    assert np.array_equal(uch.cpu().numpy(), ch) and np.array_equal(uinfo.cpu().numpy(), info)
    dch_h, dinfo_h = dch.cpu().numpy(), dinfo.cpu().numpy()
    pair = L.match_signals(info, ch, sch, sps)
    pair_dev = L.match_signals(dinfo, dch, gpu.from_numpy(sch).cuda(), gpu.from_numpy(sps).cuda())
    assert pair_dev.is_cuda and pair_dev.dtype == gpu.int64
    pair_dev = pair_dev.cpu().numpy()
    for c in range(B):
        winfo, wpos, r = want[c]
        assert winfo.shape[0] >= 3
        assert np.array_equal(_by_channel(ch, info, B)[c], winfo), ("queue", c)
        assert np.array_equal(_by_channel(dch_h, dinfo_h, B)[c], winfo), ("hand-off", c)
        assert np.array_equal(sps[sch == c], wpos), ("signal positions", c)
        assert D.identities(winfo, ln[ch == c], 1 << sf)
        # every packet pairs with the reference's signal: the one emitted by its frame's DOWNCHIRP1 call, which carries its error
        mine = np.nonzero(ch == c)[0]
        assert (pair[mine] >= 0).all() and np.array_equal(sch[pair[mine]], np.full(mine.size, c)) and np.array_equal(sps[pair[mine]], winfo[:, D.SYNC_POS])
        assert np.array_equal(ser[pair[mine]], winfo[:, D.FREQ_ERROR])
        dmine = np.nonzero(dch_h == c)[0]
        assert np.array_equal(sps[pair_dev[dmine]], winfo[:, D.SYNC_POS])
        assert consumed[c] == sum(k["consumed"] for k in r["calls"])
    return (ch, rd, ln, sy), (sch, srd, ser, spw, ssn), consumed


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sf", [7, 9, 10, 11, 12])
def test_one_shot_work(gpu, oracle, sf, mode):
    import lora_sdr_amd as L
    B = 9
    host = _streams(oracle, np.random.default_rng(1900 + sf), sf, B)
    iq = gpu.from_numpy(host).cuda()
    want = _want(oracle, sf, host)
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(mode); d.setMTU(MTU)
    pk, sg, consumed = _check_one_shot(gpu, L, d, iq, want, B, sf)
    d.close()
    # a run that asks for nothing: the same packets, signals and consumption
    p = L.LoRaDemod(sf, n_channels=B); p.set_mode(mode); p.setMTU(MTU); p.set_signals(True)
    p.work(iq)
    assert np.array_equal(p.consumed_all(), consumed)
    assert all(np.array_equal(a, b) for a, b in zip(p.signals(), sg))
    assert all(np.array_equal(a, b) for a, b in zip(p.packets_arrays(clear=False), pk))
    plain = p.packets_device(stride=MTU)
    assert len(plain) == 3
    p.close()


LANES = [(7, 4), (7, 5), (8, 5), (8, 6), (9, 6), (7, AHEAD | 3), (7, AHEAD | 4), (7, AHEAD | 5), (8, AHEAD | 4), (8, AHEAD | 5), (9, AHEAD | 5)]


@pytest.mark.parametrize("sf,lanes", LANES)
def test_lane_instances(gpu, oracle, sf, lanes):
    """the wider-lane instances and the pair (AHEAD) instances, whose DATASYMBOLS-only arm posts packets on its own (lorahip_streamkernel.h);
    an MTU of 8 behind frames of 8..12 symbols: packets posted in the middle of a run of DATASYMBOLS calls"""
    import lora_sdr_amd as L
    B = 5
    host = _streams(oracle, np.random.default_rng(2900 + sf), sf, B)
    iq = gpu.from_numpy(host).cuda()
    want = _want(oracle, sf, host)
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.set_stream_lanes(lanes)
    assert d.stream_lanes() == lanes                          # the build holds the instance
    _check_one_shot(gpu, L, d, iq, want, B, sf)
    d.close()


def _steps(gpu, L, oracle, sf):
    rng = np.random.default_rng(3900 + sf)
    N, B = 1 << sf, 7
    host = _streams(oracle, rng, sf, B)
    cap = host.shape[1]
    want = _want(oracle, sf, host)
    iq = gpu.from_numpy(host).cuda()
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.set_signals(True)
    return rng, N, B, cap, want, iq, d


@pytest.mark.parametrize("async_", [False, True, 2])
@pytest.mark.parametrize("sf", [7, 10, 12])
def test_receiver_steps(gpu, oracle, sf, async_):
    """chunks of N/2 .. 7N samples: the info rows and the signals' pos of every step are absolute positions in the channel's row"""
    import lora_sdr_amd as L
    rng, N, B, cap, want, iq, d = _steps(gpu, L, oracle, sf)
    rows = d.receiver_rows(cap_packets=4 * B, stride=MTU, info=True)
    sig = d.receiver_signal_rows(4 * B + B, pos=True)
    assert len(rows) == 4 and len(sig) == 5
    got, gsig = [[] for _ in range(B)], [[] for _ in range(B)]

    def take(n):
        gpu.cuda.synchronize()
        chn, inf = rows[2][:n].cpu().numpy(), rows[3][:n].cpu().numpy()
        for i in range(n):
            got[int(chn[i])].append(inf[i])
        ns = d.last_signals()
        sc, sp = sig[0][:ns].cpu().numpy(), sig[4][:ns].cpu().numpy()
        for i in range(ns):
            gsig[int(sc[i])].append(int(sp[i]))

    w = 0
    while w < cap:
        w = min(cap, w + int(rng.integers(N // 2, 7 * N)))
        n, _ = d.receive(iq, w, rows, async_=async_)
        take(n)
    n, _ = d.receive_flush(rows)
    take(n)
    for c in range(B):
        assert np.array_equal(np.array(got[c], np.int64).reshape(-1, 4), want[c][0]), c
        assert gsig[c] == want[c][1].tolist(), c
    d.close()



def _due(want, N, w):
    """packets posted once the rows hold w samples: a call runs while 2N samples are left (LoRaDemod.cpp:148), and the posting call
    starts at end_pos - N"""
    return sum(int((info[:, D.END_POS] + N <= w).sum()) for info, _, _ in want)


@pytest.mark.parametrize("async_", [True, 2])
def test_rows_one_too_small_lose_nothing(gpu, oracle, async_):
    """a step whose rows are one short returns the error; the next call, with rows that hold them, delivers everything with its info"""
    import lora_sdr_amd as L
    sf = 7
    rng, N, B, cap, want, iq, d = _steps(gpu, L, oracle, sf)
    rows = d.receiver_rows(cap_packets=4 * B, stride=MTU, info=True)
    got, refused = [[] for _ in range(B)], 0

    def take(n):
        gpu.cuda.synchronize()
        chn, inf = rows[2][:n].cpu().numpy(), rows[3][:n].cpu().numpy()
        for i in range(n):
            got[int(chn[i])].append(inf[i])

    levels = [0]
    while levels[-1] < cap:
        levels.append(min(cap, levels[-1] + int(rng.integers(2 * N, 7 * N))))
    for k in range(1, len(levels)):
        w = levels[k]
        # what this call delivers: an ordinary step its own packets; a pipelined one those of the step before (the first call of a
        # pipeline is an ordinary step, so the second has nothing left to deliver)
        if async_ == 2:
            need = _due(want, N, w) if k == 1 else (0 if k == 2 else _due(want, N, levels[k - 1]) - _due(want, N, levels[k - 2]))
        else:
            need = _due(want, N, w) - _due(want, N, levels[k - 1])
        if need >= 2 and k > 2 and not refused:
            short = tuple(t[:need - 1] for t in rows)
            with pytest.raises(L.LoraHipError):
                d.receive(iq, w, short, async_=async_)
            refused += 1
        n, _ = d.receive(iq, w, rows, async_=async_)
        assert n == need
        take(n)
    n, _ = d.receive_flush(rows)
    take(n)
    assert refused == 1
    for c in range(B):
        assert np.array_equal(np.array(got[c], np.int64).reshape(-1, 4), want[c][0]), c
    d.close()


class _RowsV4(C.Structure):           # lorahip_packet_rows as it was before info_dev: the previous struct_size
    _fields_ = [("struct_size", C.c_size_t), ("syms_dev", C.c_void_p), ("sym_stride", C.c_size_t), ("nsyms_dev", C.c_void_p),
                ("channel_dev", C.c_void_p), ("cap_packets", C.c_size_t), ("async_", C.c_int32), ("reserved", C.c_int32)]


class _RowsV4Guard(C.Structure):      # ... followed by a word the library must not take for info_dev
    _fields_ = [("rows", _RowsV4), ("behind", C.c_void_p)]


class _SigV4(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("channel", C.c_void_p), ("error", C.c_void_p), ("power", C.c_void_p), ("snr", C.c_void_p), ("cap", C.c_size_t)]


class _SigV4Guard(C.Structure):
    _fields_ = [("rows", _SigV4), ("behind", C.c_void_p)]


def test_the_previous_struct_size_still_works_and_writes_no_info(gpu, oracle):
    import lora_sdr_amd as L
    sf = 7
    rng, N, B, cap, want, iq, d = _steps(gpu, L, oracle, sf)
    lib = L.load()
    syms, nsyms, chan, info = d.receiver_rows(cap_packets=8 * B, stride=MTU, info=True)
    info.fill_(-7)
    spos = gpu.full((8 * B,), -7, dtype=gpu.int64, device="cuda")
    sch = gpu.empty(8 * B, dtype=gpu.int32, device="cuda")
    g = _RowsV4Guard()
    g.rows.struct_size = C.sizeof(_RowsV4)
    assert C.sizeof(_RowsV4) == 56 and C.sizeof(L._lib.PacketRowsInfo) == 64
    g.rows.syms_dev, g.rows.sym_stride, g.rows.nsyms_dev, g.rows.channel_dev = syms.data_ptr(), MTU, nsyms.data_ptr(), chan.data_ptr()
    g.rows.cap_packets, g.rows.async_ = 8 * B, 0
    g.behind = info.data_ptr()                                  # where info_dev would be: beyond struct_size, must not be read
    s = _SigV4Guard()
    s.rows.struct_size = C.sizeof(_SigV4)
    s.rows.channel, s.rows.cap = sch.data_ptr(), 8 * B
    s.behind = spos.data_ptr()
    assert lib.lorahip_demod_receive_signal_rows(d._h, C.cast(C.byref(s), C.POINTER(L._lib.SignalRows))) == 0
    n, calls = C.c_size_t(), C.c_int64()
    rc = lib.lorahip_demod_receive(d._h, C.c_void_p(iq.data_ptr()), iq.shape[1], cap, C.cast(C.byref(g), C.POINTER(L._lib.PacketRows)), C.byref(n), C.byref(calls))
    gpu.cuda.synchronize()
    assert rc == 0 and n.value == sum(w[0].shape[0] for w in want) and d.last_signals() == sum(w[1].size for w in want)
    assert bool((info == -7).all()) and bool((spos == -7).all())
    # any other size is refused as before
    g.rows.struct_size = 48
    assert lib.lorahip_demod_receive(d._h, C.c_void_p(iq.data_ptr()), iq.shape[1], cap, C.cast(C.byref(g), C.POINTER(L._lib.PacketRows)), C.byref(n), C.byref(calls)) == -1
    d.close()


def test_resident_steps_refuse_info_and_pos(gpu, oracle):
    """async = 3 with info_dev, or with signal rows that carry pos: LORAHIP_E_INVALID and the documented text before anything is rung;
    an ordinary step on the same object then delivers"""
    import lora_sdr_amd as L
    sf = 7
    rng, N, B, cap, want, iq, d = _steps(gpu, L, oracle, sf)
    lib = L.load()
    rows = d.receiver_rows(cap_packets=8 * B, stride=MTU, info=True)
    with pytest.raises(L.LoraHipError) as e:
        d.receive(iq, cap, rows, async_=3)
    assert e.value.code == -1 and "info_dev / signal positions are not delivered by resident steps" in lib.lorahip_last_error().decode()
    assert not d.resident_active()
    d.receiver_signal_rows(8 * B, pos=True)
    with pytest.raises(L.LoraHipError):
        d.receive(iq, cap, rows[:3], async_=3)
    assert "info_dev / signal positions are not delivered by resident steps" in lib.lorahip_last_error().decode()
    assert not d.resident_active()
    n, _ = d.receive(iq, cap, rows, async_=False)
    chn, inf = rows[2][:n].cpu().numpy(), rows[3][:n].cpu().numpy()
    for c in range(B):
        assert np.array_equal(inf[chn == c], want[c][0])
    d.close()


def test_segment_runs_in_two_pieces(gpu, oracle):
    """the cut falls inside the second frame's data symbols: the second run's packet began in the first, so its relative data_pos and
    sync_pos are below 0, and info + first_sample is the one-shot position"""
    import lora_sdr_amd as L
    sf, B = 9, 4
    N = 1 << sf
    host = _streams(oracle, np.random.default_rng(4900), sf, B)
    want = _want(oracle, sf, host)
    row = host.shape[1]
    buf = gpu.from_numpy(host).cuda().reshape(-1)
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.set_signals(True)
    # piece 1 ends one and a half symbols into the second frame's data (from the reference's trace): the run stops with fewer than 2N
    # samples left, inside that packet
    cut = np.array([int(w[0][1, D.DATA_POS]) + 3 * N + N // 2 for w in want], np.int64)
    base = np.arange(B, dtype=np.int64) * row
    d.work_segments(buf, base, cut.astype(np.uint64))
    used = d.consumed_all()
    ch1, _, _, _, info1 = d.packets_arrays(info=True)
    d.work_segments(buf, base + used, (row - used).astype(np.uint64))
    dinfo2 = d.packets_device(stride=MTU, clear=False, info=True)           # (packed on the device: the records are still there)
    sps2 = d.signals(pos=True)
    ch2, _, _, _, info2 = d.packets_arrays(info=True)
    assert np.array_equal(dinfo2[3].cpu().numpy()[np.argsort(dinfo2[2].cpu().numpy(), kind="stable")], info2[np.argsort(ch2, kind="stable")])
    assert (info2[:, D.DATA_POS] < 0).any() and (info2[:, D.SYNC_POS] < 0).any()
    for c in range(B):
        a, b = info1[ch1 == c].copy(), info2[ch2 == c].copy()
        b[:, :3] += used[c]
        assert np.array_equal(np.concatenate([a, b]), want[c][0]), c
        assert a.shape[0] == 1 and b[0, D.DATA_POS] < used[c]
        assert np.array_equal(sps2[5][sps2[0] == c] + used[c], want[c][1][2:]), c
    d.close()


def test_mixed_handle_on_one_device(gpu, oracle):
    """SF 7, 9, 12, two channels each: the rows of packets_device(info=True), with global channels, against single-SF objects"""
    import lora_sdr_amd as L
    sfs = np.array([7, 9, 12, 12, 9, 7], np.int32)
    rng = np.random.default_rng(5900)
    streams = [_streams(oracle, rng, int(sf), 1)[0] for sf in sfs]
    cnt = np.array([s.size for s in streams], np.uint64)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    buf = gpu.from_numpy(np.concatenate(streams)).cuda()
    m = L.LoRaDemod(channel_sf=sfs, devices=[0]); m.setMTU(MTU); m.set_signals(True)
    m.work_segments(buf, first, cnt)
    syms, nsyms, chan, info = m.packets_device(stride=MTU, clear=False, info=True)      # every part packed on the device
    sig = m.signals(pos=True)
    qch, _, qln, _, qinfo = m.packets_arrays(clear=False, info=True)
    usyms, unsyms, uchan, uinfo = m.packets_device(stride=MTU, info=True)               # ... and uploaded from the parts' host queues
    assert np.array_equal(uchan.cpu().numpy(), qch) and np.array_equal(uinfo.cpu().numpy(), qinfo)   # in the queue's order
    chan, info, nsyms = chan.cpu().numpy(), info.cpu().numpy(), nsyms.cpu().numpy()
    part_of = [int(np.nonzero(np.unique(sfs) == sf)[0][0]) for sf in sfs]
    assert (np.diff([part_of[c] for c in chan]) >= 0).all() and chan.size == qch.size   # parts one after the other, SF ascending
    for c, sf in enumerate(sfs):
        one = L.LoRaDemod(int(sf), n_channels=1); one.set_mode(1); one.setMTU(MTU); one.set_signals(True)
        one.work(gpu.from_numpy(streams[c][None, :]).cuda())
        osig = one.signals(pos=True)
        _, _, oln, _, oinfo = one.packets_arrays(info=True)
        one.close()
        winfo, wpos, _ = _want(oracle, int(sf), streams[c][None, :])[0]
        assert np.array_equal(oinfo, winfo) and oinfo.shape[0] >= 3
        assert np.array_equal(info[chan == c], oinfo) and np.array_equal(nsyms[chan == c], oln) and np.array_equal(qinfo[qch == c], oinfo)
        assert np.array_equal(sig[5][sig[0] == c], osig[5]) and np.array_equal(osig[5], wpos)
    m.close()


def test_pack_scan_across_workgroups(gpu, oracle):
    """2500 SF7 channels (three workgroups of the describing kernel) cycled over five reference streams, one run"""
    import lora_sdr_amd as L
    sf, B, K = 7, 2500, 5
    host = _streams(oracle, np.random.default_rng(6900), sf, K)
    want = _want(oracle, sf, host)
    iq = gpu.from_numpy(host).cuda()[gpu.arange(B, device="cuda") % K].contiguous()
    d = L.LoRaDemod(sf, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.set_signals(True)
    d.work(iq)
    syms, nsyms, chan, info = d.packets_device(stride=MTU, info=True, clear=False)      # the describing kernel, three workgroups
    sch, _, _, _, _, sps = d.signals(pos=True)
    pair = L.match_signals(info, chan, gpu.from_numpy(sch).cuda(), gpu.from_numpy(sps).cuda()).cpu().numpy()
    chan, info = chan.cpu().numpy(), info.cpu().numpy()
    per = [w[0].shape[0] for w in want]
    assert chan.size == sum(per[c % K] for c in range(B)) and (np.diff(chan) >= 0).all()
    expect = np.concatenate([want[c % K][0] for c in range(B)])
    assert np.array_equal(info, expect)
    assert np.array_equal(sps, np.concatenate([want[c % K][1] for c in range(B)]))
    assert (pair >= 0).all() and np.array_equal(sch[pair], chan) and np.array_equal(sps[pair], info[:, D.SYNC_POS])
    _, _, _, _, qinfo = d.packets_arrays(info=True)
    assert np.array_equal(np.sort(qinfo[:, 0]), np.sort(expect[:, 0]))
    d.close()


def test_end_to_end_from_the_scheduled_transmitter(gpu, oracle, capsys):
    """transmit_mixed places frames of SF 7, 9, 12 at known start samples; a mixed receiver reports where they arrived: the reference
    block's positions on the same rows. data_pos - start against the nominal 14.25 N (preamble 10 + sync 2 + down 2.25) is printed, not
    asserted: it is a property of the block"""
    import lora_sdr_amd as L
    from test_gpu_tx_mixed_chain import encoder, MTU as TX_MTU, SQUELCH_DB
    configs = [(7, "4/5"), (9, "4/8"), (12, "4/5")]
    encs = [encoder(L, sf, 0, cr, True, True) for sf, cr in configs]
    rng = np.random.default_rng(7900)
    flat, index, row, start, row_len = [], [], [], [], 0
    for r, (sf, _) in enumerate(configs):
        N, at = 1 << sf, (1 << sf) // 2 + 3 + 11 * r
        for _ in range(2):
            msg = rng.integers(0, 256, int(rng.integers(5, 12))).astype(np.uint8)
            n = encs[r].num_symbols(len(msg))
            flat.append(msg); index.append(r); row.append(r); start.append(at)
            at += 14 * N + N // 4 + n * N + (TX_MTU + 4) * N
        row_len = max(row_len, at)
    start = np.array(start, np.int64)
    iq, nsyms, status = L.transmit_mixed(flat, encs, np.array(index, np.int32), np.array(row, np.int32), start, len(configs), row_len, sigma=0.05, seed=3)
    assert not status.cpu().numpy().any()
    host = iq.cpu().numpy()
    m = L.LoRaDemod(channel_sf=np.array([sf for sf, _ in configs], np.int32), devices=[0]); m.setMTU(TX_MTU); m.setThreshold(SQUELCH_DB)
    m.work_segments(iq.reshape(-1), np.arange(len(configs), dtype=np.int64) * row_len, np.full(len(configs), row_len, np.uint64))
    syms, ns, chan, info = m.packets_device(stride=TX_MTU, info=True)
    chan, info = chan.cpu().numpy(), info.cpu().numpy()
    m.close()
    for c, (sf, _) in enumerate(configs):
        winfo, _, _ = _want(oracle, sf, host[c:c + 1], mtu=TX_MTU, thresh=SQUELCH_DB)[0]
        assert winfo.shape[0] == 2 and np.array_equal(info[chan == c], winfo), c
        lag = (winfo[:, D.DATA_POS] - start[2 * c:2 * c + 2]) / float(1 << sf)
        with capsys.disabled():
            print("\nSF%d: data_pos - start = %s N (nominal 14.25 N); freq_error %s" % (sf, lag.tolist(), winfo[:, D.FREQ_ERROR].tolist()))
