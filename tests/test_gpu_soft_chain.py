"""GPU: the soft-decision receive path end to end.

Known positions: 256 frames of 12 random bytes at SF7, 4/8, CRC on -- LoRaEncoder -> mod_frames -> add_awgn(SIGMA) -> soft_symbols at the
known start of the data symbols -> decode_soft, and decode_batch on the same call's hard symbols. The data symbols start 14.25 N behind
the frame's first sample (10 preamble + 2 sync + 2.25 down-chirps); the windows are taken ONE SAMPLE EARLIER, where the demodulator's own
FRAMESYNC alignment lands on a clean frame: a chirp of symbol s peaks in bin s + 1 of the window that starts with it, and
in bin s of the window one sample early -- the value the decoder reads. SIGMA was chosen beforehand (tools/bench_soft.py) so
that the hard path loses between 20 % and 60 % of the frames; the counts are printed, and asserted only as far as they show that the
soft decoder recovers no fewer frames than the hard one from the same windows.

Through the receiver: four SF8 channels, transmit -> LoRaDemod with a trace -> packets_device(info=True). A packet's soft symbols are
taken at its data_pos with the fine-tune state of the call that starts there (fine_idx_before / fine_err_before); their hard symbols
must be the demodulator's packet symbols, and decode_soft must recover every payload."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMA = 2.4            # per component, amplitude 1 (-10.6 dB): the hard path loses about a third of the frames there
FRAMES, NBYTES, LEAD = 256, 12, 19
DATASYMBOLS = 4        # lorahip_work_result::state_before of a call that reads a data symbol


def known_position_counts(torch, L, sigma, seed=5, early=1, frames=FRAMES):
    """-> (frames the hard path recovers, frames the soft path recovers, hard symbols wrong) of `frames` frames under noise `sigma`"""
    sf, N = 7, 128
    rng = np.random.default_rng(404)
    payload = rng.integers(0, 256, (frames, NBYTES), dtype=np.uint8)
    with L.Context(sf) as ctx:
        enc = L.LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setCodingRate("4/8"); enc.enableExplicit(True); enc.enableCrc(True); enc.enableWhitening(True)
        syms, nsyms = enc.encode_batch(torch.from_numpy(payload).cuda(), torch.full((frames,), NBYTES, dtype=torch.int32, device="cuda"))
        S = int(syms.shape[1])
        iq = ctx.mod_frames(syms, lead=LEAD, nsyms=nsyms)
        if sigma:
            ctx.add_awgn(iq, sigma, seed)
        first = torch.arange(frames, dtype=torch.int64, device="cuda") * int(iq.shape[1]) + (LEAD + 14 * N + N // 4 - early)
        llr, hard = ctx.soft_symbols(iq, first, nsyms, sym_stride=S, hard=True)
        dec = L.LoRaDecoder()
        dec.setSpreadFactor(sf); dec.setCodingRate("4/8"); dec.enableCrcc(True)
        want = torch.from_numpy(payload).cuda()
        counts = []
        for out, out_len, _ in (dec.decode_batch(hard, nsyms), dec.decode_soft(llr, nsyms)):
            counts.append(int(((out_len == NBYTES) & (out[:, :NBYTES] == want).all(dim=1)).sum()))
        wrong = int((hard != syms).sum())
        dec._ctx.close()
    return counts[0], counts[1], wrong


def test_known_positions_soft_recovers_no_fewer_frames(gpu, capsys):
    import lora_sdr_amd as L
    clean = known_position_counts(gpu, L, 0.0, frames=16)
    assert clean == (16, 16, 0), clean                   # the windows are the data symbols
    hard_ok, soft_ok, wrong = known_position_counts(gpu, L, SIGMA)
    with capsys.disabled():
        print("\nSF7 4/8, sigma %.2f: hard %d / %d frames, soft %d / %d (%d hard symbols wrong)" % (SIGMA, hard_ok, FRAMES, soft_ok, FRAMES, wrong))
    assert soft_ok >= hard_ok and hard_ok < FRAMES
    # the setting the comparison was chosen for: the hard path loses between 20 % and 60 % of the frames (the generator is counter-based:
    # the same noise on every run)
    assert 0.4 * FRAMES <= hard_ok <= 0.8 * FRAMES, hard_ok


def test_through_the_receiver(gpu):
    import lora_sdr_amd as L
    torch = gpu
    sf, N, B, MTU = 8, 256, 4, 48
    rng = np.random.default_rng(808)
    msgs = [rng.integers(0, 256, int(n), dtype=np.uint8) for n in (12, 5, 9, 12)]
    with L.Context(sf) as ctx:
        iq, _ = L.transmit([m.tobytes() for m in msgs], sf=sf, cr="4/8", lead=3 * N + 17, tail=(MTU + 4) * N, sigma=0.05, seed=9, ctx=ctx)
        d = L.LoRaDemod(sf, n_channels=B)
        d.setMTU(MTU); d.set_trace(True)
        d.work(iq)
        syms, nsyms, chan, info = d.packets_device(stride=MTU, info=True)
        chan_h, info_h, n_h = chan.cpu().numpy(), info.cpu().numpy(), nsyms.cpu().numpy()
        assert sorted(chan_h.tolist()) == list(range(B)), chan_h
        idx0, err = np.zeros(len(chan_h), np.int32), np.zeros(len(chan_h), np.float32)
        for p, c in enumerate(chan_h):
            tr = d.trace_array(int(c))
            starts = np.concatenate([[0], np.cumsum(tr["consumed"])[:-1]])
            at = np.flatnonzero((starts == info_h[p, L.RxInfo.DATA_POS]) & (tr["state_before"] == DATASYMBOLS))
            assert at.size >= 1, (p, c)
            idx0[p], err[p] = tr["fine_idx_before"][at[0]], tr["fine_err_before"][at[0]]
        d.close()
        row = int(iq.shape[1])
        first = torch.from_numpy(chan_h.astype(np.int64) * row + info_h[:, L.RxInfo.DATA_POS]).cuda()
        llr, hard = ctx.soft_symbols(iq, first, nsyms, fine_idx0=torch.from_numpy(idx0).cuda(), fine_err=torch.from_numpy(err).cuda(),
                                     sym_stride=MTU, hard=True)
        got, dem = hard.cpu().numpy(), syms.cpu().numpy()
        for p in range(len(chan_h)):
            assert np.array_equal(got[p, :n_h[p]], dem[p, :n_h[p]]), (p, got[p, :n_h[p]], dem[p, :n_h[p]])
        dec = L.LoRaDecoder()
        dec.setSpreadFactor(sf); dec.setCodingRate("4/8"); dec.enableCrcc(True)
        out, out_len, dropped = (t.cpu().numpy() for t in dec.decode_soft(llr, nsyms))
        for p, c in enumerate(chan_h):
            assert out_len[p] == len(msgs[c]) and np.array_equal(out[p, :out_len[p]], msgs[c]) and dropped[p] == 0, (p, c)
        dec._ctx.close()
