"""The soft-decision receive path on one GPU. Device-event times over --calls calls back to back, warm-up first, median of
--reps, as tools/bench_codec_var.py takes them:

    symbols    lorahip_soft_symbols over 4096 runs of 64 windows at SF7 and 512 runs of 64 at SF12 (ppm = sf, hard symbols too), against
               lorahip_detect_batch over the same windows (launch-uniform: the hard receiver's steady state)
    decode     lorahip_decode_packets_soft over --packets packets of 8..64 bytes through one configuration (SF7, 4/8) and through the
               30-entry table SF7..12 x 4/4..4/8, against the hard launches on the same packets' symbols; the LLRs are +1 / -1 made from
               those symbols, and both decoders must give the same bytes before either is timed
    recovery   frames recovered by the hard and the soft path of tests/test_gpu_soft_chain.py at its sigma and 1 dB either side
               (--sweep: at every sigma given, to choose one)

    python tools/bench_soft.py [--packets 65536] [--sweep 1.6,1.8,2.0,...]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import lora_sdr_amd as L
from lora_sdr_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=65536); ap.add_argument("--reps", type=int, default=11); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=20, help="calls between two events"); ap.add_argument("--sweep", default="")
ap.add_argument("--only", default="", help="symbols, decode or recovery")
a = ap.parse_args()
assert a.reps >= 10, "median of at least 10"
RATE = {0: "4/4", 1: "4/5", 2: "4/6", 3: "4/7", 4: "4/8"}


def event_ms(fn):
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) / a.calls)
    return float(np.median(ts))


def bench_symbols():
    for sf, runs in ((7, 4096), (12, 512)):
        N, S = 1 << sf, 64
        with L.Context(sf) as ctx:
            ctx.use_torch_stream()
            sym = torch.from_numpy(np.random.default_rng(sf).integers(0, N, runs * S).astype(np.int16)).cuda()
            iq = ctx.synth_symbols(sym, noise_sigma=1.0, seed=sf)
            first = torch.arange(runs, dtype=torch.int64, device="cuda") * (S * N)
            n = torch.full((runs,), S, dtype=torch.int32, device="cuda")
            llr = torch.zeros((runs, S, sf), dtype=torch.float32, device="cuda")
            hard = torch.zeros((runs, S), dtype=torch.int16, device="cuda")
            out = [torch.empty(runs * S, dtype=t, device="cuda") for t in (torch.int16, torch.float32, torch.float32, torch.float32)]
            batch = ctx.make_batch(iq, runs * S, *out)
            ctx.detect_batch_raw(batch)
            ctx.soft_symbols(iq, first, n, sym_stride=S, hard=True, out=(llr, hard))
            assert torch.equal(hard.reshape(-1), out[0])
            t_hard = event_ms(lambda: ctx.detect_batch_raw(batch))
            t_soft = event_ms(lambda: ctx.soft_symbols(iq, first, n, sym_stride=S, hard=True, out=(llr, hard)))
            print(json.dumps({"what": "soft symbols against the hard batch", "sf": sf, "runs": runs, "windows": runs * S, "detect_batch_ms": round(t_hard, 4),
                              "soft_symbols_ms": round(t_soft, 4), "soft_over_hard": round(t_soft / t_hard, 3),
                              "soft_windows_per_s": round(runs * S / t_soft * 1e3)}), flush=True)


def cfg_array(cfgs):
    arr = (_lib.DecoderCfg * len(cfgs))()
    for i, (sf, rdd) in enumerate(cfgs):
        arr[i] = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), sf, 0, rdd, 1, 1, 0, 1, 0, 8)
    return arr


def bench_decode():
    ctx = L.Context(7)
    lib = ctx._lib
    ctx.use_torch_stream()
    for cfgs in ([(7, 4)], [(sf, rdd) for sf in range(7, 13) for rdd in range(5)]):
        stride = max(int(lib.lorahip_encode_num_symbols(C.byref(_lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, 0, rdd, 1, 1, 1)), 64)) for sf, rdd in cfgs)
        width = max(sf for sf, _ in cfgs)
        per = a.packets // len(cfgs)
        syms, nsyms, llrs = [], [], []
        for sf, rdd in cfgs:
            rng = np.random.default_rng(100 * sf + rdd)
            enc = L.LoRaEncoder()
            enc.setSpreadFactor(sf); enc.setCodingRate(RATE[rdd])
            s, n = enc.encode_batch(torch.from_numpy(rng.integers(0, 256, (per, 64)).astype(np.uint8)).cuda(),
                                    torch.from_numpy(rng.integers(8, 65, per).astype(np.int32)).cuda(), sym_stride=stride)
            g = s.to(torch.int32) & 0xffff
            g = g ^ (g >> 1)
            bits = (g[:, :, None] >> torch.arange(sf, device="cuda", dtype=torch.int32)) & 1
            row = torch.zeros((per, stride * width), dtype=torch.float32, device="cuda")
            row[:, :stride * sf] = (bits.to(torch.float32) * 2 - 1).reshape(per, -1)       # symbol s of an SF's packet at s * sf of its row
            syms.append(s); nsyms.append(n); llrs.append(row)
        P = per * len(cfgs)
        perm = torch.from_numpy(np.random.default_rng(1).permutation(P)).cuda()            # the order a receiver delivers
        syms, nsyms, llr = torch.cat(syms)[perm].contiguous(), torch.cat(nsyms)[perm].contiguous(), torch.cat(llrs)[perm].contiguous()
        index = torch.arange(len(cfgs), dtype=torch.int32, device="cuda").repeat_interleave(per)[perm].contiguous()
        tab = cfg_array(cfgs)
        outs = [(torch.zeros((P, 2 * (stride + 8)), dtype=torch.uint8, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda"),
                 torch.zeros(P, dtype=torch.int32, device="cuda")) for _ in range(2)]

        def hard(o=outs[0]):
            rc = lib.lorahip_decode_packets_info(ctx._h, tab, len(cfgs), index.data_ptr(), None, 0, syms.data_ptr(), stride, nsyms.data_ptr(), P, o[0].data_ptr(),
                                                 2 * (stride + 8), o[1].data_ptr(), o[2].data_ptr(), None)
            assert rc == 0, lib.lorahip_last_error()

        def soft(o=outs[1]):
            rc = lib.lorahip_decode_packets_soft(ctx._h, tab, len(cfgs), index.data_ptr(), None, 0, llr.data_ptr(), stride * width, stride, nsyms.data_ptr(), P,
                                                 o[0].data_ptr(), 2 * (stride + 8), o[1].data_ptr(), o[2].data_ptr(), None)
            assert rc == 0, lib.lorahip_last_error()

        hard(); soft()
        assert all(torch.equal(x, y) for x, y in zip(*outs)) and int((outs[0][1] > 0).sum()) == P
        t_hard, t_soft = event_ms(hard), event_ms(soft)
        print(json.dumps({"what": "soft decoder against the hard table launch", "configurations": len(cfgs), "packets": P, "sym_stride": stride,
                          "llr_row_floats": stride * width, "hard_ms": round(t_hard, 4), "soft_ms": round(t_soft, 4), "soft_over_hard": round(t_soft / t_hard, 3),
                          "soft_packets_per_s": round(P / t_soft * 1e3)}), flush=True)
        del syms, nsyms, llr, llrs, outs
        torch.cuda.empty_cache()
    ctx.close()


def bench_recovery():
    import test_gpu_soft_chain as T
    sigmas = [float(s) for s in a.sweep.split(",")] if a.sweep else [T.SIGMA * 10 ** (-1 / 20), T.SIGMA, T.SIGMA * 10 ** (1 / 20)]
    for sigma in sigmas:
        hard_ok, soft_ok, wrong = T.known_position_counts(torch, L, sigma)
        print(json.dumps({"what": "frames recovered, SF7 4/8, 12 bytes + crc", "sigma": round(sigma, 4), "snr_db": round(-10 * np.log10(2 * sigma * sigma), 2),
                          "frames": T.FRAMES, "hard_ok": hard_ok, "soft_ok": soft_ok, "hard_symbols_wrong": wrong}), flush=True)


for name, fn in (("symbols", bench_symbols), ("decode", bench_decode), ("recovery", bench_recovery)):
    if not a.only or a.only == name:
        fn()
