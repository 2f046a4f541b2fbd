"""GPU: a gateway that is told no coding rate. Payload bytes -> transmit_mixed with a LoRaEncoderSet of 30 encoders (SF 7..12 x 4/4..4/8),
one short frame each, placed on six channel rows by SF -> noise -> ONE mixed LoRaDemod -> packets_device -> ONE LoRaDecoderSet of six
"header" decoders whose table says "SF index of channel" -> the payload bytes, with the header report beside them. Before that the
reference alone (the oracle's demodulator and decoder on the CPU) must recover every payload from the same samples; and the output must
equal, byte for byte, the 30-entry fixed-rate table launch on the same rows. The pattern and the squelch are those of
tests/test_gpu_tx_mixed_chain.py. Everything compared is integer and exact."""
import numpy as np
import pytest

from test_gpu_encoder import encoder
from test_gpu_tx_mixed_chain import SQUELCH_DB

pytestmark = pytest.mark.gpu

MTU = 24
RATES = ("4/4", "4/5", "4/6", "4/7", "4/8")
N_BYTES = 4                                                          # 17 nibbles with header and crc: 3 blocks at SF7 (24 symbols at 4/8), 2 at SF12


def schedule(L, rng):
    """row sf - 7 carries that SF's five frames, rate 4/4 first: each starts (MTU + 4) symbols behind the end of the one before
    -> (encoders, payloads [row][k], flat payloads, index, row, start, row_len)"""
    encs = [encoder(L, sf, 0, cr, True, True) for sf in range(7, 13) for cr in RATES]
    payloads, flat, index, row, start, row_len = [], [], [], [], [], 0
    for r, sf in enumerate(range(7, 13)):
        N = 1 << sf
        at = N // 2 + 3
        sent = []
        for k in range(len(RATES)):
            m = rng.integers(0, 256, N_BYTES).astype(np.uint8)
            n = encs[5 * r + k].num_symbols(N_BYTES)
            assert 8 <= n <= MTU
            sent.append(m); flat.append(m); index.append(5 * r + k); row.append(r); start.append(at)
            at += 14 * N + N // 4 + n * N + (MTU + 4) * N
        payloads.append(sent)
        row_len = max(row_len, at)
    return encs, payloads, flat, np.array(index, np.int32), np.array(row, np.int32), np.array(start, np.int64), row_len


def test_gateway_with_one_decoder_per_sf(gpu, oracle):
    import lora_sdr_amd as L
    encs, payloads, flat, index, row, start, row_len = schedule(L, np.random.default_rng(2027))
    assert len(encs) == 30
    iq, nsyms, status = L.transmit_mixed(flat, L.LoRaEncoderSet(encs), index, row, start, 6, row_len, sigma=0.3, seed=7)
    assert not status.cpu().numpy().any()
    host = iq.cpu().numpy()
    for c, sf in enumerate(range(7, 13)):
        pk = oracle.demod_run(sf, host[c], thresh=SQUELCH_DB, mtu=MTU)["packets"]
        assert len(pk) == len(RATES), ("the reference at this noise", c, len(pk))
        dec = [oracle.decode(sf, np.asarray(q).astype(np.uint16), cr=cr, crcc=True, error_check=True) for (_, q), cr in zip(pk, RATES)]
        assert [None if o is None else o.tolist() for o, _ in dec] == [p.tolist() for p in payloads[c]], ("the reference at this noise", c)

    m = L.LoRaDemod(channel_sf=np.arange(7, 13), devices=[0])
    m.setMTU(MTU)
    m.setThreshold(SQUELCH_DB)
    m.work_segments(iq.reshape(-1), np.arange(6, dtype=np.int64) * row_len, np.full(6, row_len, np.uint64))
    syms, nsyms_rx, chan = m.packets_device(stride=MTU)
    assert syms.shape == (30, MTU)
    by_header = []
    for sf in range(7, 13):
        d = L.LoRaDecoder(); d.setSpreadFactor(sf); d.setCodingRate("header"); d.enableCrcc(True); d.enableErrorCheck(True)
        by_header.append(d)
    sf_index_of_channel = gpu.arange(6, dtype=gpu.int32, device="cuda")
    out, out_len, dropped, info = L.LoRaDecoderSet(by_header).decode_batch(syms, nsyms_rx, index=chan, table=sf_index_of_channel, info=True)
    ch = chan.cpu().numpy()
    o, n, d, rep = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy(), info.cpu().numpy()
    assert not d.any() and (n == N_BYTES).all()
    order = np.zeros(30, np.int64)                                   # the k-th packet of its channel was sent at rate k
    for c in range(6):
        rows_c = np.flatnonzero(ch == c)
        assert rows_c.size == len(RATES), ("channel", c)
        order[rows_c] = np.arange(len(RATES))
        assert [o[r, :N_BYTES].tolist() for r in rows_c] == [p.tolist() for p in payloads[c]], ("channel", c)
    assert np.array_equal(rep[:, 1], order), "the report's rdd is the rate each frame was sent at"
    assert (rep[:, 0] == N_BYTES).all() and (rep[:, 2] == 1).all() and not rep[:, 3].any() and not rep[:, 6:].any()
    # the existing way: 30 entries and somebody who knows each packet's rate
    fixed = []
    for sf in range(7, 13):
        for cr in RATES:
            dd = L.LoRaDecoder(); dd.setSpreadFactor(sf); dd.setCodingRate(cr); dd.enableCrcc(True); dd.enableErrorCheck(True)
            fixed.append(dd)
    index30 = gpu.from_numpy((5 * ch + order).astype(np.int32)).cuda()
    out30, len30, drop30 = L.LoRaDecoderSet(fixed).decode_batch(syms, nsyms_rx, index=index30)
    assert gpu.equal(out30, out) and gpu.equal(len30, out_len) and gpu.equal(drop30, dropped)
    m.close()
