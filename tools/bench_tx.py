"""The transmit side on one GPU: does the encoder matter in the chain? For SF7 / SF10 / SF12, P packets of 8..64 random bytes (mixed
lengths in one launch), device-event times of the encode launch alone, of lorahip_mod_frames_var alone and of transmit() (encode ->
modulate -> AWGN), warm-up first, median of --reps. The reference encoder has no batch form to time against: the comparison is encode
time against modulate time PER PACKET on the same build.

The modulator writes a whole frame per packet (SF12: 3.6 MB), so it runs on the first F packets that fit --iq-bytes (it is linear in
the frames); the encoder runs on all P. Both are reported per packet.   python tools/bench_tx.py [--packets 65536] [--cr 4/8]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=65536); ap.add_argument("--cr", default="4/8"); ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--sfs", default="7,10,12")
ap.add_argument("--iq-bytes", type=float, default=2 * 2.0 ** 30, help="device memory for the modulator's output rows")
a = ap.parse_args()
assert a.reps >= 10, "median of at least 10"
P = a.packets


def event_ms(fn):
    """median device time of fn() between two events on the current stream"""
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


for sf in [int(s) for s in a.sfs.split(",")]:
    rng = np.random.default_rng(sf)
    n = rng.integers(8, 65, P).astype(np.int32)
    host = rng.integers(0, 256, (P, 64)).astype(np.uint8)
    data, nb = torch.from_numpy(host).cuda(), torch.from_numpy(n).cuda()
    ctx = L.Context(sf)
    enc = L.LoRaEncoder(ctx=ctx)
    enc.setSpreadFactor(sf); enc.setCodingRate(a.cr)
    S = enc.num_symbols(64)
    syms, nsyms = enc.encode_batch(data, nb)
    assert int(nsyms.min()) >= 8 and int(nsyms.max()) <= S
    t_enc = event_ms(lambda: enc.encode_batch(data, nb))
    enc_bytes = int(n.sum()) + 4 * P + 2 * P * S + 4 * P           # payload + lengths read; symbol rows + counts written
    flen = ctx.mod_frame_len(S, 1)
    F = int(max(256, min(P, (a.iq_bytes // (8 * flen)) // 256 * 256)))
    fs, fn_, fd, fb = syms[:F].contiguous(), nsyms[:F].contiguous(), data[:F].contiguous(), nb[:F].contiguous()
    t_mod = event_ms(lambda: ctx.mod_frames(fs, nsyms=fn_))          # includes the zero fill of the rows it allocates
    t_tx = event_ms(lambda: L.transmit(fd, sf=sf, cr=a.cr, sigma=0.3, seed=1, nbytes=fb, ctx=ctx))
    rec = {"sf": sf, "cr": a.cr, "packets": P, "sym_stride": S, "encode_ms": round(t_enc, 4), "encode_packets_per_s": round(P / t_enc * 1e3),
           "encode_bytes_moved": enc_bytes, "encode_GB_per_s": round(enc_bytes / t_enc / 1e6, 2),
           "mod_frames": F, "mod_var_ms": round(t_mod, 3), "mod_packets_per_s": round(F / t_mod * 1e3),
           "transmit_ms": round(t_tx, 3), "transmit_packets_per_s": round(F / t_tx * 1e3),
           "encode_us_per_packet": round(t_enc / P * 1e3, 5), "mod_us_per_packet": round(t_mod / F * 1e3, 3),
           "encode_share_of_encode_plus_mod": round((t_enc / P) / (t_enc / P + t_mod / F), 6)}
    print(json.dumps(rec), flush=True)
    del syms, nsyms, fs, fn_, fd, fb
    ctx.close()
    torch.cuda.empty_cache()
