"""Synthesiser throughput beside the channeliser's on the mirrored shape (same K, D = U, L: the same number of complex multiply-adds per
wideband sample). HIP events on the context (lorahip_timer_*), warm-up until the clocks have left idle, then alternating windows of
both kernels; the median window is reported. One JSON line per shape, then a table for DESIGN.md.
    python tools/bench_synth.py [--windows 7] [--reps 10] [--shapes "512,16,128,16777216"]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

SHAPES = [(8, 16, 128, 1 << 24), (64, 16, 128, 1 << 24), (512, 16, 128, 1 << 22), (64, 64, 512, 1 << 24)]     # K, U, L, wideband samples per call

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="", help="K,U,L,W;K,U,L,W;... instead of the four standard shapes")
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


rows_out = []
for K, U, Lt, W in SHAPES:
    n = W // U
    rows = torch.view_as_complex(torch.randn((K, n, 2), generator=g, device="cuda"))
    wide_in = torch.view_as_complex(torch.randn((W, 2), generator=g, device="cuda"))
    freqs = (np.arange(K) - 0.5 * (K - 1)) * (0.8 / K)
    h = L.design_lowpass(U, Lt)
    sy = L.Synthesizer(ctx, freqs, U, U * h)
    ch = L.Channelizer(ctx, freqs, U, h)
    wide_out = torch.empty(W, dtype=torch.complex64, device="cuda")
    narrow = torch.empty((K, n + 1), dtype=torch.complex64, device="cuda")
    run_s = lambda: sy.run(rows, out=wide_out)
    run_c = lambda: ch.run(wide_in, out=narrow)
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        run_s(); run_c()
        torch.cuda.synchronize()
    ts, tc = [], []
    for _ in range(a.windows):                         # alternating: both see the same machine
        ts.append(window(run_s)); tc.append(window(run_c))
    ts_med, tc_med = float(np.median(ts)), float(np.median(tc))
    flop = 8.0 * K * (-(-Lt // U)) * W                 # 8 per complex multiply-add, K * ceil(L/U) of them per wideband sample
    rec = dict(K=K, U=U, L=Lt, wide_samples=W, reps=a.reps, windows=a.windows,
               synth_ms=ts_med * 1e3, synth_ms_min=min(ts) * 1e3, synth_ms_max=max(ts) * 1e3, synth_gsps=W / ts_med / 1e9, synth_tflops=flop / ts_med / 1e12,
               chan_ms=tc_med * 1e3, chan_ms_min=min(tc) * 1e3, chan_ms_max=max(tc) * 1e3, chan_gsps=W / tc_med / 1e9, chan_tflops=flop / tc_med / 1e12,
               synth_over_chan_rate=tc_med / ts_med)
    rows_out.append(rec)
    print(json.dumps(rec), flush=True)
    sy.close(); ch.close()
    del rows, wide_in, wide_out, narrow

print("| K | U = D | L | synthesiser Gsamples/s (wideband out) | TFLOP/s | channeliser Gsamples/s (wideband in) | TFLOP/s | synth / chan |")
print("|---|---|---|---|---|---|---|---|")
for r in rows_out:
    print("| %d | %d | %d | %.2f | %.1f | %.2f | %.1f | %.2f |" % (r["K"], r["U"], r["L"], r["synth_gsps"], r["synth_tflops"], r["chan_gsps"],
                                                               r["chan_tflops"], r["synth_over_chan_rate"]))
