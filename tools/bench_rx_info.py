"""What lorahip_rx_info costs where it is asked for, on one GPU: a receiver step with and without info rows (and signal positions),
and the device hand-off packets_device() with and without info.

The load: --channels SF--sf channels, every channel a stream of --frames frames of 16 symbols (MTU 16) at a small carrier offset and
noise 0.05, given to the receiver in chunks of --windows symbol windows.
  * step:     lorahip_demod_receive (async_=True and 2) over the whole stream, host clock around all its steps and a device synchronise,
              with plain rows and with info rows + signal positions, ALTERNATING inside each repetition;
  * hand-off: one work() over the whole stream, then packets_device(clear=False) with and without info (host clock around the call and a
              device synchronise; every call packs on the device from the kernel's records, which stay there).
Median and (min .. max) of --reps; one JSON line per figure.

    python tools/bench_rx_info.py [--sf 7] [--channels 4096] [--frames 4] [--windows 8] [--reps 9]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=7); ap.add_argument("--channels", type=int, default=4096); ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--windows", type=int, default=8); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
SF, N, B, MTU = a.sf, 1 << a.sf, a.channels, 16
dev = torch.device("cuda", 0)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4), "max_ms": round(float(max(ts)), 4)}


def load():
    """(B, row) complex64 on the device: 8 distinct streams made by the library's own modulator, cycled over the channels"""
    ctx = L.Context(SF)
    rng = np.random.default_rng(19)
    K = 8
    frame = int(ctx._lib.lorahip_mod_body_len(SF, MTU))
    gap = (MTU + 4) * N
    row = N + a.frames * (frame + gap)
    F = K * a.frames
    syms = torch.from_numpy(rng.integers(0, N, (F, MTU)).astype(np.uint16).view(np.int16)).to(dev)
    nsyms = torch.full((F,), MTU, dtype=torch.int32, device=dev)
    sfs = torch.full((F,), SF, dtype=torch.int32, device=dev)
    rows = torch.arange(F, dtype=torch.int32, device=dev) // a.frames
    start = (N // 2 + 3 + 5 * rows.long() + (torch.arange(F, device=dev) % a.frames) * (frame + gap)).contiguous()
    iq = torch.zeros((K, row), dtype=torch.complex64, device=dev)
    ctx.mod_frames_sched(syms, nsyms, sfs, rows.contiguous(), start, iq)
    ctx.add_awgn(iq, 0.05, 7)
    ctx.synchronize()
    ctx.close()
    return iq[torch.arange(B, device=dev) % K].contiguous()


def steps(d, iq, rows, async_):
    row = iq.shape[1]
    w, total = 0, 0
    while w < row:
        w = min(row, w + a.windows * N)
        n, _ = d.receive(iq, w, rows, async_=async_)
        total += n
    n, _ = d.receive_flush(rows)
    torch.cuda.synchronize()
    return total + n


def bench_steps(iq, async_):
    out = {}
    objs = {}
    for name, info in (("plain", False), ("info", True)):
        d = L.LoRaDemod(SF, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.setThreshold(0.0); d.set_signals(True)
        objs[name] = (d, d.receiver_rows(2 * B, stride=MTU, info=info), d.receiver_signal_rows(3 * B, pos=info))
        out[name] = []
    packets = None
    for rep in range(a.warmup + a.reps):
        for name, (d, rows, sig) in objs.items():
            d.rewind(); d.activate(); d.register_signal_rows(sig)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = steps(d, iq, rows, async_)
            ms = (time.perf_counter() - t0) * 1e3
            assert packets is None or n == packets, (n, packets)
            packets = n
            if rep >= a.warmup:
                out[name].append(ms)
    n_steps = -(-iq.shape[1] // (a.windows * N))
    rec = {"figure": "receiver steps", "async": int(async_), "sf": SF, "channels": B, "windows_per_step": a.windows, "steps": n_steps, "packets": packets}
    for name, ts in out.items():
        rec[name] = stats(ts)
        rec[name]["us_per_step"] = round(float(np.median(ts)) / n_steps * 1e3, 2)
    rec["info_over_plain"] = round(float(np.median(out["info"]) / np.median(out["plain"])), 4)
    print(json.dumps(rec), flush=True)
    for d, _, _ in objs.values():
        d.close()


def bench_handoff(iq):
    d = L.LoRaDemod(SF, n_channels=B); d.set_mode(1); d.setMTU(MTU); d.setThreshold(0.0)
    d.work(iq)
    out = {"plain": [], "info": []}
    for rep in range(a.warmup + a.reps):
        for name in out:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = d.packets_device(stride=MTU, clear=False, info=(name == "info"))
            torch.cuda.synchronize()
            if rep >= a.warmup:
                out[name].append((time.perf_counter() - t0) * 1e3)
    rec = {"figure": "packets_device (packed on the device)", "sf": SF, "channels": B, "packets": int(r[0].shape[0])}
    for name, ts in out.items():
        rec[name] = stats(ts)
    rec["info_over_plain"] = round(float(np.median(out["info"]) / np.median(out["plain"])), 4)
    print(json.dumps(rec), flush=True)
    d.close()


iq = load()
for async_ in (True, 2):
    bench_steps(iq, async_)
bench_handoff(iq)
