"""Polyphase synthesis filter bank beside the direct-form synthesiser: the same plan, the same rows, one process. HIP events on the
context (lorahip_timer_*), 0.4 s of warm-up per shape, then alternating windows of both; the median window is reported with its
spread. M is a power of two 8..1024 or 5 * 2^a (5 .. 320). A shape the direct form refuses is printed as refused, never skipped. One
JSON line per shape, then a table for DESIGN.md.
    python tools/bench_psb.py [--windows 7] [--reps 10] [--shapes "M,K,U,L,W;..."]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

COPY_TBPS = 6.29            # the achievable copy rate the project measures against
# M, K (rows: the first K bins around 0), U, L, wideband samples per call; the last two: 16 rows against all 64 (independence of K)
SHAPES = [(16, 16, 16, 128, 1 << 24), (64, 64, 64, 512, 1 << 24), (256, 256, 256, 2048, 1 << 24), (1024, 1024, 1024, 8192, 1 << 24),
          (64, 64, 80, 512, 1 << 24), (512, 512, 256, 2048, 1 << 24), (64, 16, 64, 512, 1 << 24),
          # the 200 kHz LoRaWAN grids (M = 5 * 2^a, U = 8 M / 5, L = 16 U): 1, 8, 16, 32 and 64 MHz
          (5, 3, 8, 128, 1 << 24), (40, 8, 64, 1024, 1 << 24), (40, 40, 64, 1024, 1 << 24), (80, 64, 128, 2048, 1 << 24),
          (160, 128, 256, 4096, 1 << 24), (320, 256, 512, 8192, 1 << 24)]

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
    bins = np.arange(K) - K // 2
    ps = L.PolyphaseSynthesizer.for_plan(ctx, (M, U, bins), h)     # the constructor or radix5, by M
    wide = torch.empty(W, dtype=torch.complex64, device="cuda")
    run_p = lambda: ps.run(rows, out=wide)
    try:
        sy = L.Synthesizer(ctx, ps.freqs, U, h)
        wide_d = torch.empty(W, dtype=torch.complex64, device="cuda")
        run_d = lambda: sy.run(rows, out=wide_d)
        refused = ""
    except L.LoraHipError as e:
        sy, run_d, refused = None, None, str(e)
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        run_p()
        torch.cuda.synchronize()
    reps_d = a.reps
    if run_d:                                          # the direct form may take a second per call at large K: fewer of them a window
        run_d(); torch.cuda.synchronize()
        t1 = time.time(); run_d(); torch.cuda.synchronize()
        reps_d = max(1, min(a.reps, int(0.5 / max(time.time() - t1, 1e-6))))
    tp, td = [], []
    for _ in range(a.windows):                         # alternating: both see the same machine
        tp.append(window(run_p, a.reps))
        if run_d:
            td.append(window(run_d, reps_d))
    tp_med = float(np.median(tp))
    nbytes = 8.0 * K * n_in + 8.0 * W
    rec = dict(M=M, K=K, U=U, L=Lt, wide_samples=W, reps=a.reps, windows=a.windows, psb_ms=tp_med * 1e3, psb_ms_min=min(tp) * 1e3,
               psb_ms_max=max(tp) * 1e3, psb_gsps=W / tp_med / 1e9, bytes_moved=nbytes, psb_copy_fraction=nbytes / tp_med / (COPY_TBPS * 1e12))
    if run_d:
        td_med = float(np.median(td))
        rec.update(direct_reps=reps_d, direct_ms=td_med * 1e3, direct_ms_min=min(td) * 1e3, direct_ms_max=max(td) * 1e3, direct_gsps=W / td_med / 1e9,
                   psb_over_direct=td_med / tp_med)
        sy.close()
    else:
        rec.update(direct_refused=refused)
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    ps.close()
    del rows, wide

print("| M | K | U | L | PSB ms a call | PSB Gsamples/s (min .. max) | of the copy rate | direct form Gsamples/s (min .. max) | PSB / direct |")
print("|---|---|---|---|---|---|---|---|---|")
for r in recs:
    W = r["wide_samples"]
    p = "%.1f (%.1f .. %.1f)" % (r["psb_gsps"], W / r["psb_ms_max"] / 1e6, W / r["psb_ms_min"] / 1e6)
    if "direct_gsps" in r:
        d = "%.2f (%.2f .. %.2f)" % (r["direct_gsps"], W / r["direct_ms_max"] / 1e6, W / r["direct_ms_min"] / 1e6)
        ratio = "%.1f" % r["psb_over_direct"]
    else:
        d, ratio = "refused", "-"
    print("| %d | %d | %d | %d | %.3f | %s | %.1f %% | %s | %s |" % (r["M"], r["K"], r["U"], r["L"], r["psb_ms"], p, 100.0 * r["psb_copy_fraction"], d, ratio))
