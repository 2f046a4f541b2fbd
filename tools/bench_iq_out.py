"""Integer IQ output of the two synthesisers beside cf32: the same object, the same rows, one process. Per shape
four variants: (a) cf32 run(), (b) sc16 run_int(), (c) sc8 run_int(), (d) what a caller did before run_int existed -- run(), then the
torch expression of the definition over the wideband buffer (multiply, round, nan_to_num, clamp, cast to int16), timed together. HIP
events on the context (lorahip_timer_*), 0.4 s of warm-up per shape, then alternating windows of all four; the median window is
reported with its spread. One JSON line per shape, then a table for DESIGN.md. M = 0 is the direct-form synthesiser with K channels
(the shapes of tools/bench_synth.py); M a power of two or 5 * 2^a the polyphase bank (the shapes of tools/bench_psb.py).
    python tools/bench_iq_out.py [--windows 7] [--reps 10] [--shapes "M,K,U,L,W;..."]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

# M (0: direct form), K, U, L, wideband samples per call
SHAPES = [(0, 8, 16, 128, 1 << 24), (0, 64, 16, 128, 1 << 24), (0, 512, 16, 128, 1 << 22), (0, 64, 64, 512, 1 << 24),
          (16, 16, 16, 128, 1 << 24), (64, 64, 64, 512, 1 << 24), (256, 256, 256, 2048, 1 << 24), (1024, 1024, 1024, 8192, 1 << 24),
          (64, 64, 80, 512, 1 << 24), (512, 512, 256, 2048, 1 << 24), (64, 16, 64, 512, 1 << 24),
          (5, 3, 8, 128, 1 << 24), (40, 8, 64, 1024, 1 << 24), (40, 40, 64, 1024, 1 << 24), (80, 64, 128, 2048, 1 << 24),
          (160, 128, 256, 4096, 1 << 24), (320, 256, 512, 8192, 1 << 24)]
VARIANTS = ["cf32", "sc16", "sc8", "convert"]

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="", help="M,K,U,L,W;... instead of the standard shapes")
a = ap.parse_args()
if a.shapes:
    SHAPES = [tuple(int(v) for v in part.split(",")) for part in a.shapes.split(";")]
ctx = L.Context(7)
g = torch.Generator(device="cuda"); g.manual_seed(1)


def window(fn, reps):
    ctx.use_torch_stream()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() * 1e-3 / reps


recs = []
for M, K, U, Lt, W in SHAPES:
    n_in = W // U
    W = n_in * U
    rows = torch.view_as_complex(torch.randn((K, n_in, 2), generator=g, device="cuda"))
    h = (L.design_lowpass(U, Lt) * U).astype(np.float32)
    if M:
        obj = L.PolyphaseSynthesizer.for_plan(ctx, (M, U, np.arange(K) - K // 2), h)
    else:
        obj = L.Synthesizer(ctx, (np.arange(K) - 0.5 * (K - 1)) * (0.8 / K), U, h)
    wide = torch.empty(W, dtype=torch.complex64, device="cuda")
    o16 = torch.empty((W, 2), dtype=torch.int16, device="cuda")
    o8 = torch.empty((W, 2), dtype=torch.int8, device="cuda")
    # the rows are unit Gaussians, K of them summed: a scale that keeps most components inside the range, as a caller would choose
    s16 = 32767.0 / (4.0 * np.sqrt(K))
    s8 = 127.0 / (4.0 * np.sqrt(K))

    def convert():
        y = torch.view_as_real(obj.run(rows, out=wide))
        return torch.nan_to_num(torch.round(y * s16), nan=0.0, posinf=32767.0, neginf=-32768.0).clamp(-32768, 32767).to(torch.int16)

    run = {"cf32": lambda: obj.run(rows, out=wide),
           "sc16": lambda: obj.run_int(rows, torch.int16, s16, out=o16),
           "sc8": lambda: obj.run_int(rows, torch.int8, s8, out=o8),
           "convert": convert}
    run["cf32"](); torch.cuda.synchronize()
    t1 = time.time(); run["convert"](); torch.cuda.synchronize()
    reps = max(1, min(a.reps, int(0.5 / max(time.time() - t1, 1e-6))))      # the direct form at large K: fewer calls a window
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        for v in VARIANTS:
            run[v]()
        torch.cuda.synchronize()
    t = {v: [] for v in VARIANTS}
    for _ in range(a.windows):                         # alternating: all four see the same machine
        for v in VARIANTS:
            t[v].append(window(run[v], reps))
    in_bytes = 8.0 * K * n_in / W
    # per wideband sample, beyond reading the rows: the kernel writes the sample once; the conversion reads 8 and writes 8 four times
    # (multiply, round, nan_to_num, clamp), then reads 8 and writes 4 (the cast)
    bytes_per_sample = {"cf32": in_bytes + 8, "sc16": in_bytes + 4, "sc8": in_bytes + 2, "convert": in_bytes + 8 + 4 * 16 + 12}
    rec = dict(M=M, K=K, U=U, L=Lt, wide_samples=W, reps=reps, windows=a.windows, clipped_sc16=obj.clipped())
    for v in VARIANTS:
        med = float(np.median(t[v]))
        rec[v] = dict(ms=med * 1e3, ms_min=min(t[v]) * 1e3, ms_max=max(t[v]) * 1e3, gsps=W / med / 1e9, bytes_per_sample=bytes_per_sample[v])
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    obj.close()
    del rows, wide, o16, o8

print("| synthesiser | M | K | U | L | " + " | ".join("%s Gsamples/s (min .. max), B/sample" % v for v in VARIANTS) + " | sc16 / cf32 | sc16 / convert |")
print("|---|---|---|---|---|" + "---|" * (len(VARIANTS) + 2))
for r in recs:
    W = r["wide_samples"]
    cells = ["%.2f (%.2f .. %.2f), %.1f" % (r[v]["gsps"], W / r[v]["ms_max"] / 1e6, W / r[v]["ms_min"] / 1e6, r[v]["bytes_per_sample"]) for v in VARIANTS]
    print("| %s | %s | %d | %d | %d | %s | %.2f | %.2f |" % ("polyphase" if r["M"] else "direct", r["M"] or "-", r["K"], r["U"], r["L"], " | ".join(cells),
                                                        r["cf32"]["ms"] / r["sc16"]["ms"], r["convert"]["ms"] / r["sc16"]["ms"]))
