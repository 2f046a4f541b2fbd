"""The test-signal kernels on one GPU: synth_symbols without and with noise and add_awgn over the same number of samples, device events,
the three alternating inside each repetition; one JSON line per SF with the median and (min .. max) of --reps.

    python tools/bench_testsignal.py [--sfs 7,12] [--samples 67108864] [--reps 9]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--sfs", default="7,12"); ap.add_argument("--samples", type=int, default=1 << 26)
ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda", 0)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


for sf in [int(s) for s in a.sfs.split(",")]:
    ctx = L.Context(sf)
    W = a.samples >> sf
    sym = torch.from_numpy(np.random.default_rng(sf).integers(0, 1 << sf, W).astype(np.uint16).view(np.int16)).to(dev)
    iq = ctx.synth_symbols(sym)
    fns = {"synth_clean": lambda: ctx.synth_symbols(sym), "synth_noisy": lambda: ctx.synth_symbols(sym, noise_sigma=0.3, seed=5),
           "add_awgn": lambda: ctx.add_awgn(iq, 0.3, seed=5)}
    ts = dict((k, []) for k in fns)
    for rep in range(a.warmup + a.reps):
        for k, fn in fns.items():
            t = event_ms(fn)
            if rep >= a.warmup:
                ts[k].append(t)
    rec = {"sf": sf, "windows": W, "samples": W << sf}
    for k, v in ts.items():
        rec[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    print(json.dumps(rec), flush=True)
    ctx.close()
    del sym, iq
    torch.cuda.empty_cache()
