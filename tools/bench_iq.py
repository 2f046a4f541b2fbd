"""Integer IQ input of the receive front ends beside cf32: the same object, the same samples, one process. Per shape
four variants: (a) cf32 run(), (b) sc16 run_int(), (c) sc8 run_int(), (d) what a caller did before run_int existed -- the sc16 tensor
converted on the device with ints.float().mul_(scale), then run(), timed together. HIP events on the context (lorahip_timer_*), 0.4 s of
warm-up per shape, then alternating windows of all four; the median window is reported with its spread. One JSON line per shape, then a
table for DESIGN.md. M = 0 is the direct-form channeliser with K channels; M a power of two or 5 * 2^a the polyphase bank.
    python tools/bench_iq.py [--windows 7] [--reps 10] [--shapes "M,K,D,L,W;..."]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

# M (0: direct form), K, D, L, wideband samples per call
SHAPES = [(16, 16, 16, 128, 1 << 24), (64, 64, 64, 512, 1 << 24), (1024, 1024, 1024, 8192, 1 << 24), (80, 80, 128, 640, 1 << 24),
          (0, 16, 16, 128, 1 << 24)]
VARIANTS = ["cf32", "sc16", "sc8", "convert"]

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="", help="M,K,D,L,W;... instead of the standard shapes")
a = ap.parse_args()
if a.shapes:
    SHAPES = [tuple(int(v) for v in part.split(",")) for part in a.shapes.split(";")]
ctx = L.Context(7)
g = torch.Generator(device="cuda"); g.manual_seed(1)


def window(fn):
    ctx.use_torch_stream()
    ctx.timer_start()
    for _ in range(a.reps):
        fn()
    return ctx.timer_stop() * 1e-3 / a.reps


recs = []
for M, K, D, Lt, W in SHAPES:
    i16 = torch.randint(-32768, 32768, (W, 2), generator=g, device="cuda", dtype=torch.int16)
    i8 = torch.randint(-128, 128, (W, 2), generator=g, device="cuda", dtype=torch.int8)
    s16 = 2.0 ** -15
    wide = torch.view_as_complex(i16.float().mul_(s16))
    h = L.design_lowpass(D, Lt)
    if M:
        obj = L.PolyphaseChannelizer.for_plan(ctx, (M, D, np.arange(K) - K // 2), h)
    else:
        obj = L.Channelizer(ctx, (np.arange(K) - K // 2) / float(K), D, h)
    narrow = torch.empty((K, W // D + 1), dtype=torch.complex64, device="cuda")
    run = {"cf32": lambda: obj.run(wide, out=narrow),
           "sc16": lambda: obj.run_int(i16, out=narrow),
           "sc8": lambda: obj.run_int(i8, out=narrow),
           "convert": lambda: obj.run(torch.view_as_complex(i16.float().mul_(s16)), out=narrow)}
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        for v in VARIANTS:
            run[v]()
        torch.cuda.synchronize()
    t = {v: [] for v in VARIANTS}
    for _ in range(a.windows):                         # alternating: all four see the same machine
        for v in VARIANTS:
            t[v].append(window(run[v]))
    out_bytes = 8.0 * K * (W // D) / W
    # per wideband sample: the kernel reads the sample once and writes K / D outputs; the conversion reads 4 and writes 8 (float()), then
    # reads 8 and writes 8 (mul_) before the kernel reads the 8
    bytes_per_sample = {"cf32": 8 + out_bytes, "sc16": 4 + out_bytes, "sc8": 2 + out_bytes, "convert": 4 + 8 + 8 + 8 + 8 + out_bytes}
    rec = dict(M=M, K=K, D=D, L=Lt, wide_samples=W, reps=a.reps, windows=a.windows)
    for v in VARIANTS:
        med = float(np.median(t[v]))
        rec[v] = dict(ms=med * 1e3, ms_min=min(t[v]) * 1e3, ms_max=max(t[v]) * 1e3, gsps=W / med / 1e9, bytes_per_sample=bytes_per_sample[v])
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    obj.close()
    del wide, narrow, i16, i8

print("| front end | M | K | D | L | " + " | ".join("%s Gsamples/s (min .. max), B/sample" % v for v in VARIANTS) + " |")
print("|---|---|---|---|---|" + "---|" * len(VARIANTS))
for r in recs:
    W = r["wide_samples"]
    cells = ["%.1f (%.1f .. %.1f), %.1f" % (r[v]["gsps"], W / r[v]["ms_max"] / 1e6, W / r[v]["ms_min"] / 1e6, r[v]["bytes_per_sample"]) for v in VARIANTS]
    print("| %s | %s | %d | %d | %d | %s |" % ("polyphase" if r["M"] else "direct", r["M"] or "-", r["K"], r["D"], r["L"], " | ".join(cells)))
