"""GPU: the mixed-SF transmit path at the head of the mixed-SF receive path -- test_mixed_gateway_bytes_in_bytes_out (tests/
test_gpu_mixed_chain.py) with its load made by ONE transmit_mixed call instead of twelve transmit() calls: bytes -> one encoder launch with
the configuration per packet -> one scheduled modulator launch into (12, row_len) channel rows -> noise -> one mixed LoRaDemod ->
packets_device -> one LoRaDecoderSet launch -> the bytes. Everything compared is integer and exact."""
import numpy as np
import pytest

from test_gpu_encoder import encoder

pytestmark = pytest.mark.gpu

MTU = 64
# The squelch of the demodulator, on the reference and on the receiver alike. The block's default of -30 dB is "off": snr = peak bin over all
# the other bins, which noise alone brings to about 10 log10((ln N + 0.6) / N) -- -14 dB at SF7, -27 dB at SF12 -- so every noise window passes,
# and a window passes the frame sync when three bins in a row fall into their 8-bin ranges: (8 / N)^3, 1 in 4096 at SF7. transmit() per
# configuration makes an SF7 stream of some 300 windows. Here every row has the length the SF12 rows need, about a million samples: 8000
# windows of noise at SF7, and the reference alone finds seven packets in them that nobody sent (measured on the first run of this test; no
# seed and no spacing cures a rate). At sigma 0.3 an aligned chirp of amplitude 1 stands at 10 log10(1 / (2 sigma^2)) = +7.4 dB at every SF,
# and noise reaches 0 dB only when one bin holds half the window's energy (e^-64 at SF7): 0 dB lies 7 dB from either.
SQUELCH_DB = 0.0


def gateway_schedule(L, rng, configs):
    """two payloads of 5..20 bytes per row (one row per configuration (sf, cr)), placed as gateway_traffic() of test_gpu_mixed_chain.py
    places them: the first frame starts at N / 2 + 3, the second (MTU + 4) N behind the first's end, (MTU + 4) N of silence behind the second
    -> (encoders, payloads per row, flat payload list, index, row, start, row_len)"""
    encs = [encoder(L, sf, 0, cr, True, True) for sf, cr in configs]
    payloads, flat, index, row, start, row_len = [], [], [], [], [], 0
    for r, (sf, cr) in enumerate(configs):
        N = 1 << sf
        sent = [rng.integers(0, 256, int(rng.integers(5, 21))).astype(np.uint8) for _ in range(2)]
        at = N // 2 + 3
        for m in sent:
            n = encs[r].num_symbols(len(m))
            assert 8 <= n <= MTU
            flat.append(m); index.append(r); row.append(r); start.append(at)
            at += 14 * N + N // 4 + n * N + (MTU + 4) * N
        payloads.append(sent)
        row_len = max(row_len, at)
    return encs, payloads, flat, np.array(index, np.int32), np.array(row, np.int32), np.array(start, np.int64), row_len


def receive(L, gpu, iq, configs, thresh=None):
    """one mixed handle over the rows of iq, the packet hand-off, one decoder launch whose table says "decoder of channel" -> per channel the
    payloads that arrived, in order"""
    B, row_len = iq.shape
    sfs = np.array([sf for sf, _ in configs])
    m = L.LoRaDemod(channel_sf=sfs, devices=[0])
    m.setMTU(MTU)
    if thresh is not None:
        m.setThreshold(thresh)
    m.work_segments(iq.reshape(-1), np.arange(B, dtype=np.int64) * row_len, np.full(B, row_len, np.uint64))
    syms, nsyms, chan = m.packets_device(stride=MTU)
    decoders = []
    for sf, cr in configs:
        d = L.LoRaDecoder(); d.setSpreadFactor(sf); d.setCodingRate(cr); d.enableCrcc(True); d.enableErrorCheck(True)
        decoders.append(d)
    got = [[] for _ in range(B)]
    if syms.shape[0]:
        out, out_len, dropped = L.LoRaDecoderSet(decoders).decode_batch(syms, nsyms, index=chan, table=gpu.arange(B, dtype=gpu.int32, device="cuda"))
        out, out_len, dropped, chan = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy(), chan.cpu().numpy()
        assert int(dropped.sum()) == 0 and (out_len >= 5).all()
        for r in range(chan.size):
            got[int(chan[r])].append(out[r, :out_len[r]].tolist())
    m.close()
    return got


def test_mixed_gateway_bytes_in_bytes_out_from_one_transmit_call(gpu, oracle):
    """12 rows, SF 7..12 x coding rate 4/5 and 4/8, two payloads each, sigma 0.3: every payload of every row, in order. Before that the
    reference alone (the oracle's demodulator and decoder on the CPU) must recover every payload from the same samples. Both run with the
    squelch at SQUELCH_DB (above): the rows are long, and mostly noise at the low SFs."""
    import lora_sdr_amd as L
    configs = [(sf, cr) for sf in range(7, 13) for cr in ("4/5", "4/8")]
    encs, payloads, flat, index, row, start, row_len = gateway_schedule(L, np.random.default_rng(2025), configs)
    iq, nsyms, status = L.transmit_mixed(flat, encs, index, row, start, len(configs), row_len, sigma=0.3, seed=5)
    assert iq.shape == (len(configs), row_len) and iq.dtype == gpu.complex64
    assert not status.cpu().numpy().any()
    assert nsyms.cpu().tolist() == [encs[i].num_symbols(len(m)) for i, m in zip(index, flat)]
    host = iq.cpu().numpy()
    for c, (sf, cr) in enumerate(configs):
        pk = oracle.demod_run(sf, host[c], thresh=SQUELCH_DB, mtu=MTU)["packets"]
        dec = [oracle.decode(sf, np.asarray(q).astype(np.uint16), cr=cr, crcc=True, error_check=True) for _, q in pk]
        assert [None if o is None else o.tolist() for o, _ in dec] == [p.tolist() for p in payloads[c]], ("the reference at this noise", c)
    got = receive(L, gpu, iq, configs, thresh=SQUELCH_DB)
    for c, (sf, cr) in enumerate(configs):
        assert got[c] == [p.tolist() for p in payloads[c]], ("channel", c, "SF%d" % sf, cr)


def test_a_payload_without_an_encoder_leaves_its_slot_silent(gpu):
    """one payload's index names no entry: nsyms -3, status -1, not a sample of its slot written (no noise here, so silence is zeros) --
    and the row's other packet, like every other row's packets, still arrives. Through a table, into a caller's buffer."""
    import lora_sdr_amd as L
    configs = [(7, "4/5"), (8, "4/8"), (9, "4/5"), (7, "4/8")]
    encs, payloads, flat, index, row, start, row_len = gateway_schedule(L, np.random.default_rng(2026), configs)
    table = np.array([3, 2, 1, 0, 9], np.int32)                     # index -> entry, and one index whose entry does not exist
    tindex = np.array([3 - i for i in index], np.int32)
    lost = 2                                                        # the first payload of row 1
    tindex[lost] = 4
    out = gpu.full((len(configs), row_len), 7.0, dtype=gpu.complex64, device="cuda")
    iq, nsyms, status = L.transmit_mixed(flat, L.LoRaEncoderSet(encs), tindex, row, start, len(configs), row_len, table=table, out=out)
    assert iq.data_ptr() == out.data_ptr()
    want_n = [encs[i].num_symbols(len(m)) for i, m in zip(index, flat)]
    want_n[lost] = -3
    assert nsyms.cpu().tolist() == want_n and status.cpu().tolist() == [-1 if p == lost else 0 for p in range(len(flat))]
    host = iq.cpu().numpy()
    assert not host[1, :start[lost + 1]].any() and host[1, start[lost + 1]:start[lost + 1] + 1000].all()
    for p in range(len(flat)):                                      # the buffer was zeroed, and nothing lies outside the bodies
        end = start[p + 1] if p + 1 < len(flat) and row[p + 1] == row[p] else row_len
        body = 0 if p == lost else (14 << configs[row[p]][0]) + (1 << (configs[row[p]][0] - 2)) + (want_n[p] << configs[row[p]][0])
        assert (p and row[p - 1] == row[p]) or not host[row[p], :start[p]].any(), p
        assert not host[row[p], start[p] + body:end].any() and (body == 0 or host[row[p], start[p]:start[p] + body].all()), p
    got = receive(L, gpu, iq, configs)
    for c in range(len(configs)):
        want = [p.tolist() for p in payloads[c]]
        assert got[c] == (want[1:] if c == 1 else want), ("channel", c)
