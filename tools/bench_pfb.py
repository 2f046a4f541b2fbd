"""Polyphase filter-bank channeliser beside the direct-form channeliser: the same shape, the same input, one process. HIP events on the
context (lorahip_timer_*), 0.4 s of warm-up per shape, then alternating windows of both; the median window is reported with its
spread. A shape the direct form refuses is printed as refused, never skipped. One JSON line per shape, then a table for DESIGN.md.
M may be a power of two or 5 * 2^a (the radix-5 bank: PolyphaseChannelizer.for_plan picks the constructor).
    python tools/bench_pfb.py [--windows 7] [--reps 10] [--shapes "M,K,D,L,W;..."]
the 200 kHz LoRaWAN grid at 16 MHz beside its power-of-two neighbours:
    python tools/bench_pfb.py --shapes "80,80,128,640,16777216;80,64,128,640,16777216;64,64,128,640,16777216;128,128,128,640,16777216"
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

COPY_TBPS = 6.29            # the achievable copy rate the project measures against
# M, K (rows: the first K bins), D, L, wideband samples per call
SHAPES = [(16, 16, 16, 128, 1 << 24), (64, 64, 64, 512, 1 << 24), (256, 256, 256, 2048, 1 << 24), (1024, 1024, 1024, 8192, 1 << 24),
          (64, 64, 80, 512, 1 << 24), (1024, 16, 1024, 8192, 1 << 24)]

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
    wide = torch.view_as_complex(torch.randn((W, 2), generator=g, device="cuda"))
    h = L.design_lowpass(D, Lt)
    bins = np.arange(K) - K // 2
    pf = L.PolyphaseChannelizer.for_plan(ctx, (M, D, bins), h)
    narrow = torch.empty((K, W // D + 1), dtype=torch.complex64, device="cuda")
    run_p = lambda: pf.run(wide, out=narrow)
    try:
        ch = L.Channelizer(ctx, pf.freqs, D, h)
        narrow_d = torch.empty((K, W // D + 1), dtype=torch.complex64, device="cuda")
        run_d = lambda: ch.run(wide, out=narrow_d)
        refused = ""
    except L.LoraHipError as e:
        ch, run_d, refused = None, None, str(e)
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        run_p()
        if run_d:
            run_d()
        torch.cuda.synchronize()
    tp, td = [], []
    for _ in range(a.windows):                         # alternating: both see the same machine
        tp.append(window(run_p))
        if run_d:
            td.append(window(run_d))
    tp_med = float(np.median(tp))
    nbytes = 8.0 * W + 8.0 * K * (W // D)
    rec = dict(M=M, K=K, D=D, L=Lt, wide_samples=W, reps=a.reps, windows=a.windows, pfb_ms=tp_med * 1e3, pfb_ms_min=min(tp) * 1e3,
               pfb_ms_max=max(tp) * 1e3, pfb_gsps=W / tp_med / 1e9, bytes_moved=nbytes, pfb_copy_fraction=nbytes / tp_med / (COPY_TBPS * 1e12))
    if run_d:
        td_med = float(np.median(td))
        rec.update(direct_ms=td_med * 1e3, direct_ms_min=min(td) * 1e3, direct_ms_max=max(td) * 1e3, direct_gsps=W / td_med / 1e9,
                   pfb_over_direct=td_med / tp_med)
        ch.close()
    else:
        rec.update(direct_refused=refused)
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    pf.close()
    del wide, narrow

print("| M | K | D | L | PFB Gsamples/s (min .. max) | of the copy rate | direct form Gsamples/s (min .. max) | PFB / direct |")
print("|---|---|---|---|---|---|---|---|")
for r in recs:
    W = r["wide_samples"]
    p = "%.1f (%.1f .. %.1f)" % (r["pfb_gsps"], W / r["pfb_ms_max"] / 1e6, W / r["pfb_ms_min"] / 1e6)
    if "direct_gsps" in r:
        d = "%.2f (%.2f .. %.2f)" % (r["direct_gsps"], W / r["direct_ms_max"] / 1e6, W / r["direct_ms_min"] / 1e6)
        ratio = "%.1f" % r["pfb_over_direct"]
    else:
        d, ratio = "refused", "-"
    print("| %d | %d | %d | %d | %s | %.1f %% | %s | %s |" % (r["M"], r["K"], r["D"], r["L"], p, 100.0 * r["pfb_copy_fraction"], d, ratio))
