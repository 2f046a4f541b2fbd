"""The host-staged decoder on one GPU: what does one lorahip_decode_packets_info_host call cost, copies and wait included? P packets of
8..64 random bytes split evenly over SF7..12 at 4/8, rows of the longest packet's symbols in HOST memory, a table of six entries, index,
channel table and header report all present (every piece the staging carries). Host clock round the synchronous call, warm-up first,
median of --reps; --rounds times over, so that the spread between rounds is known before two builds are compared (LORAHIP_LIB).

    python tools/bench_codec_host.py [--packets 4096]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L
from lora_sdr_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=4096); ap.add_argument("--reps", type=int, default=51); ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
ctx = L.Context(7)                                                   # device, stream and staging pair only
lib = ctx._lib
sfs = list(range(7, 13))
stride = max(int(lib.lorahip_encode_num_symbols(C.byref(_lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, 0, 4, 1, 1, 1)), 64)) for sf in sfs)
per = a.packets // len(sfs)
P = per * len(sfs)
rows, counts = [], []
for sf in sfs:
    rng = np.random.default_rng(sf)
    enc = L.LoRaEncoder()
    enc.setSpreadFactor(sf)
    s, n = enc.encode_batch(torch.from_numpy(rng.integers(0, 256, (per, 64)).astype(np.uint8)).cuda(),
                            torch.from_numpy(rng.integers(8, 65, per).astype(np.int32)).cuda(), sym_stride=stride)
    rows.append(s.cpu().numpy().view(np.uint16)); counts.append(n.cpu().numpy())
perm = np.random.default_rng(1).permutation(P)
syms, nsyms = np.ascontiguousarray(np.concatenate(rows)[perm]), np.ascontiguousarray(np.concatenate(counts)[perm])
index = np.ascontiguousarray(np.repeat(np.arange(6, dtype=np.int32), per)[perm])
table = np.arange(6, dtype=np.int32)
cfgs = (_lib.DecoderCfg * 6)(*[_lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), sf, 0, 4, 1, 1, 0, 1, 0, 8) for sf in sfs])
out_stride = 2 * (stride + 8)
out, out_len, dropped = np.zeros((P, out_stride), np.uint8), np.zeros(P, np.int32), np.zeros(P, np.int32)
info = np.zeros((P, 8), np.int32)


def call():
    rc = lib.lorahip_decode_packets_info_host(ctx._h, cfgs, 6, index.ctypes.data, table.ctypes.data, 6, syms.ctypes.data, stride, nsyms.ctypes.data, P,
                                              out.ctypes.data, out_stride, out_len.ctypes.data, dropped.ctypes.data, info.ctypes.data)
    assert rc == 0, lib.lorahip_last_error()


call()
assert int((out_len > 0).sum()) == P and int(dropped.sum()) == 0 and bool((info[:, 0] >= 8).all())
rounds = []
for _ in range(a.rounds):
    for _ in range(a.warmup):
        call()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e6)
    rounds.append(float(np.median(ts)))
print(json.dumps({"what": "lorahip_decode_packets_info_host, six entries, index + table + report", "packets": P, "sym_stride": stride,
                  "staged_bytes_in": int(syms.nbytes + nsyms.nbytes + index.nbytes + table.nbytes + out.nbytes),
                  "staged_bytes_out": int(out.nbytes + out_len.nbytes + dropped.nbytes + info.nbytes),
                  "call_us": [round(t, 1) for t in rounds], "median_us": round(float(np.median(rounds)), 1)}), flush=True)
