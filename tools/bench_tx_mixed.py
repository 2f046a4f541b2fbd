"""The mixed-SF transmit path on one GPU against the per-configuration loop it replaces, and the lane instances of the scheduled modulator.

Default: the traffic of gateway_traffic() (tests/test_gpu_mixed_chain.py) -- SF 7..12 x coding rate 4/5 and 4/8, payloads of 5..20 bytes,
sigma 0.3, every frame followed by (MTU + 4) silent symbols -- scaled to --scales frames per configuration, sent
  * through ONE transmit_mixed() call (encode with the configuration per packet -> scheduled modulator -> AWGN). The frames of SF s stand
    2^(12-s) to a row, back to back with their silence, so that every row is one SF12 slot long;
  * through the loop of twelve transmit() calls, a fresh Context per call as gateway_traffic() makes them, and with the twelve contexts
    reused. Unchanged code: the path before transmit_mixed existed. Every frame is a row of its own there.
Both start from payload rows that are on the device already and end in a device synchronise; host clock, warm-up first, the two paths
ALTERNATING inside each repetition; median and (min .. max) of --reps. Then the modulator launch alone at lanes = 4 / 16 / 64 and 0
(automatic) on the same schedule, device events.

--table: the measurement behind the automatic lane rule: lanes = 4 / 16 / 64 at 16 .. 65536 frames of 32 symbols,
SF7 and SF12, device events, the instances alternating inside each repetition. The frames go to min(F, 4096) rows, the later ones over the
earlier ones (an overlap leaves the value of one of the frames in each sample: fine for a timing, and it bounds the memory).

    python tools/bench_tx_mixed.py [--scales 1,16,1024] [--reps 7]      python tools/bench_tx_mixed.py --table"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="1,16,1024"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--table", action="store_true"); ap.add_argument("--counts", default="16,256,4096,65536"); ap.add_argument("--sfs", default="7,12")
a = ap.parse_args()
MTU, STRIDE = 64, 20
CONFIGS = [(sf, cr) for sf in range(7, 13) for cr in ("4/5", "4/8")]
dev = torch.device("cuda", 0)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(min(ts)), 3), "max_ms": round(float(max(ts)), 3)}


def alternating(fns, clock):
    """{name: [ms]}: warm-up of every fn, then --reps rounds that run every fn once, in turn"""
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = dict((k, []) for k in fns)
    for _ in range(a.reps):
        for k, fn in fns.items():
            out[k].append(clock(fn))
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def encoder(sf, cr, ctx=None):
    e = L.LoRaEncoder(ctx=ctx) if ctx is not None else L.LoRaEncoder()
    e.setSpreadFactor(sf); e.setCodingRate(cr)
    return e


def lane_table():
    ctx = L.Context(7)
    S = 32
    for sf in [int(s) for s in a.sfs.split(",")]:
        body = int(ctx._lib.lorahip_mod_body_len(sf, S))
        for F in [int(c) for c in a.counts.split(",")]:
            rng = np.random.default_rng(F + sf)
            rows = min(F, 4096)
            syms = torch.from_numpy(rng.integers(0, 1 << sf, (F, S)).astype(np.uint16).view(np.int16)).to(dev)
            nsyms = torch.full((F,), S, dtype=torch.int32, device=dev)
            sfs = torch.full((F,), sf, dtype=torch.int32, device=dev)
            row = (torch.arange(F, dtype=torch.int32, device=dev) % rows).contiguous()
            start = torch.zeros(F, dtype=torch.int64, device=dev)
            out = torch.zeros((rows, body), dtype=torch.complex64, device=dev)
            fns = dict((lanes, (lambda lanes=lanes: ctx.mod_frames_sched(syms, nsyms, sfs, row, start, out, lanes=lanes))) for lanes in (4, 16, 64))
            ts = alternating(fns, event_ms)
            med = dict((k, float(np.median(v))) for k, v in ts.items())
            best = min(med, key=med.get)
            rec = {"table": True, "sf": sf, "frames": F, "nsyms": S, "samples": F * body, "best": best}
            for k, v in ts.items():
                rec["lanes%d" % k] = stats(v)
                rec["lanes%d" % k]["Msamples_per_s"] = round(F * body / med[k] / 1e3, 1)
            print(json.dumps(rec), flush=True)
            del syms, out
            torch.cuda.empty_cache()
    ctx.close()


def gateway(K):
    rng = np.random.default_rng(2024 + K)
    ctx = L.Context(7)
    encs = [encoder(sf, cr) for sf, cr in CONFIGS]
    es = L.LoRaEncoderSet(encs, ctx=ctx)
    slot12 = (1 << 11) + 3 + int(ctx._lib.lorahip_mod_body_len(12, es.max_symbols(STRIDE))) + ((MTU + 4) << 12)
    data, nb, index, row, start = [], [], [], [], []
    per_cfg, n_rows = [], 0
    for i, (sf, cr) in enumerate(CONFIGS):
        n = rng.integers(5, STRIDE + 1, K).astype(np.int32)
        d = rng.integers(0, 256, (K, STRIDE)).astype(np.uint8)
        per_cfg.append((torch.from_numpy(d).to(dev), torch.from_numpy(n).to(dev)))
        per_row = 1 << (12 - sf)
        slot = slot12 >> (12 - sf)
        f = np.arange(K)
        data.append(d); nb.append(n); index.append(np.full(K, i, np.int32))
        row.append((n_rows + f // per_row).astype(np.int32))
        start.append(((f % per_row) * slot + (1 << (sf - 1)) + 3).astype(np.int64))
        n_rows += -(-K // per_row)
    data, nb = torch.from_numpy(np.concatenate(data)).to(dev), torch.from_numpy(np.concatenate(nb)).to(dev)
    index, row, start = [torch.from_numpy(np.concatenate(v)).to(dev) for v in (index, row, start)]
    F = 12 * K
    ctxs = [L.Context(sf) for sf, _ in CONFIGS]

    def mixed():
        return L.transmit_mixed(data, es, index, row, start, n_rows, slot12, sigma=0.3, seed=5, nbytes=nb, ctx=ctx)

    def loop(reuse):
        keep = []
        for i, (sf, cr) in enumerate(CONFIGS):
            N = 1 << sf
            keep.append(L.transmit(per_cfg[i][0], sf=sf, cr=cr, padding=2, sigma=0.3, seed=5 + i, nbytes=per_cfg[i][1], lead=N // 2 + 3,
                                   tail=(MTU + 4) * N, ctx=ctxs[i] if reuse else None))
        return keep
    iq, nsyms, status = mixed()
    assert not status.cpu().numpy().any() and int(nsyms.min()) >= 8 and int(nsyms.max()) <= MTU
    ts = alternating({"transmit_mixed": mixed, "loop_fresh_contexts": lambda: loop(False), "loop_reused_contexts": lambda: loop(True)}, host_ms)
    rec = {"frames_per_config": K, "frames": F, "mixed_rows": n_rows, "mixed_row_len": slot12,
           "mixed_GB": round(n_rows * slot12 * 8 / 1e9, 3), "loop_GB": round(sum(k[0].numel() for k in loop(True)) * 8 / 1e9, 3)}
    for k, v in ts.items():
        rec[k] = stats(v)
        rec[k]["frames_per_s"] = round(F / np.median(v) * 1e3)
    rec["mixed_over_loop_fresh"] = round(float(np.median(ts["loop_fresh_contexts"]) / np.median(ts["transmit_mixed"])), 2)
    rec["mixed_over_loop_reused"] = round(float(np.median(ts["loop_reused_contexts"]) / np.median(ts["transmit_mixed"])), 2)
    # the modulator launch alone, per lane instance, on the schedule of the mixed call
    syms, nsyms = es.encode_batch(data, nb, index, sym_stride=es.max_symbols(STRIDE))
    sf = torch.tensor([c[0] for c in CONFIGS], dtype=torch.int32, device=dev)[index.long()].contiguous()
    fns = dict((lanes, (lambda lanes=lanes: ctx.mod_frames_sched(syms, nsyms, sf, row, start, iq, lanes=lanes))) for lanes in (0, 4, 16, 64))
    for k, v in alternating(fns, event_ms).items():
        rec["mod_sched_lanes%d" % k] = stats(v)
    print(json.dumps(rec), flush=True)
    for c in ctxs:
        c.close()
    ctx.close()
    torch.cuda.empty_cache()


if a.table:
    lane_table()
else:
    for K in [int(s) for s in a.scales.split(",")]:
        gateway(K)
