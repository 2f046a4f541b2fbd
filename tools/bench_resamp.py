"""Rational-rate resampler: time per call and algorithmic traffic beside the streaming rate lorahip_membw_probe reaches in the same
process. HIP events on the context (lorahip_timer_*), 0.4 s of warm-up per shape, then windows of --reps calls; the median window is
reported with its spread. Traffic = what the algorithm has to move: every input sample once in its format (8 bytes cf32, 4 bytes sc16)
and every output once (8 bytes). One JSON line per shape, then a table for DESIGN.md section 8h.
    python tools/bench_resamp.py [--windows 7] [--reps 10] [--shapes "U,D,L,K,N,fmt;..."]      (fmt: cf32 | sc16 | sc8)
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

# up, down, taps, rows, samples per row and call, input format
SHAPES = [(5, 6, 192, 1, 1 << 26, "cf32"), (5, 6, 192, 1, 1 << 26, "sc16"), (25, 24, 800, 1, 1 << 26, "cf32"), (25, 24, 800, 1, 1 << 26, "sc16"),
          (25, 256, 4096, 512, 1 << 17, "cf32")]
IN_BYTES = {"cf32": 8, "sc16": 4, "sc8": 2}

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="", help="U,D,L,K,N,fmt;... instead of the standard shapes")
a = ap.parse_args()
if a.shapes:
    SHAPES = [tuple(v if i == 5 else int(v) for i, v in enumerate(part.split(","))) for part in a.shapes.split(";")]
ctx = L.Context(7)
lib = L.load()
g = torch.Generator(device="cuda"); g.manual_seed(1)


def window(fn):
    ctx.use_torch_stream()
    ctx.timer_start()
    for _ in range(a.reps):
        fn()
    return ctx.timer_stop() * 1e-3 / a.reps


def probe_rate():
    """the best streaming read rate of lorahip_membw_probe over 1 GiB, bytes per second"""
    n = 1 << 30
    buf = torch.zeros(n // 4, dtype=torch.float32, device="cuda")
    best = 0.0
    for bpc in (4, 8, 16):
        run = lambda: lib.lorahip_membw_probe(ctx._h, C.c_void_p(buf.data_ptr()), n, 0, bpc)
        window(run)
        best = max(best, n / min(window(run) for _ in range(3)))
    return best


recs = []
for U, D, Lt, K, N, fmt in SHAPES:
    h = L.Resampler.design(U, D, Lt)
    rs = L.Resampler(ctx, U, D, h, n_rows=K)
    if fmt == "cf32":
        rows = torch.view_as_complex(torch.randn((K, N, 2), generator=g, device="cuda"))
        run = lambda: rs.run(rows, out=out)
    else:
        dt = torch.int16 if fmt == "sc16" else torch.int8
        rows = torch.randint(-100, 100, (K, N, 2), generator=g, device="cuda", dtype=dt)
        run = lambda: rs.run_int(rows, out=out)
    out = torch.empty((K, N * U // D + 1), dtype=torch.complex64, device="cuda")
    t0 = time.time()
    while time.time() - t0 < 0.4:                      # the clocks need ~40 ms of load to leave idle
        run()
        torch.cuda.synchronize()
    rate = probe_rate()                                # beside every shape: the same machine state
    ts = [window(run) for _ in range(a.windows)]
    med = float(np.median(ts))
    nbytes = float(IN_BYTES[fmt]) * K * N + 8.0 * K * (N * U // D)
    rec = dict(up=U, down=D, taps=Lt, taps_per_output=-(-Lt // U), rows=K, samples_per_row=N, format=fmt, reps=a.reps, windows=a.windows,
               ms=med * 1e3, ms_min=min(ts) * 1e3, ms_max=max(ts) * 1e3, in_gsps=K * N / med / 1e9, bytes_moved=nbytes,
               traffic_gbps=nbytes / med / 1e9, probe_gbps=rate / 1e9, of_probe=nbytes / med / rate)
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    rs.close()
    del rows, out

print("| up/down | taps (per output) | rows | format | input Gsamples/s (min .. max) | traffic GB/s | streaming probe GB/s | of the probe |")
print("|---|---|---|---|---|---|---|---|")
for r in recs:
    n = r["rows"] * r["samples_per_row"]
    print("| %d/%d | %d (%d) | %d | %s | %.2f (%.2f .. %.2f) | %.0f | %.0f | %.1f %% |"
          % (r["up"], r["down"], r["taps"], r["taps_per_output"], r["rows"], r["format"], r["in_gsps"], n / r["ms_max"] / 1e6, n / r["ms_min"] / 1e6,
             r["traffic_gbps"], r["probe_gbps"], 100.0 * r["of_probe"]))
