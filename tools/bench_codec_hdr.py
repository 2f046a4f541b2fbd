"""The decoder that reads each packet's coding rate from its header, on one GPU: what does a table of six entries (sf, rdd =
LORAHIP_RDD_FROM_HEADER) cost against the table of thirty (sf, rate) entries it replaces -- which needs somebody who knows every packet's
rate? P packets of 8..64 random bytes, split evenly over SF7..12 x 4/4..4/8, encoded by the batched encoder, rows of the longest packet's
symbols, in mixed order (any configuration beside any other). Three launches on the SAME rows, in turn, --rounds times over, so that the
spread between the rounds of one launch is known before two launches are compared:

    fixed30    lorahip_decode_packets_cfgs, 30 entries, index = 5 * sf index + rate (runs identically before this feature)
    header6    lorahip_decode_packets_info, 6 entries with the rate from the header, index = sf index, no report
    header6+i  the same with the header report (32 bytes per packet written)

Each figure: device-event time of one launch out of --calls back to back, warm-up first, median of --reps. Before anything is timed the
three give the same bytes, and the report's rate is the rate sent.

    python tools/bench_codec_hdr.py [--packets 65536]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L
from lora_sdr_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=65536); ap.add_argument("--reps", type=int, default=11); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--calls", type=int, default=200, help="calls between two events (200 x 0.1 ms: a window of 20 ms)")
a = ap.parse_args()
assert a.reps >= 10, "median of at least 10"
RATE = {0: "4/4", 1: "4/5", 2: "4/6", 3: "4/7", 4: "4/8"}
ctx = L.Context(7)                                                   # device and stream only
lib = ctx._lib


def event_ms(fn):
    """median device time of one fn() out of --calls between two events on the current stream"""
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) / a.calls)
    return float(np.median(ts))


def cfg_array(cfgs):
    arr = (_lib.DecoderCfg * len(cfgs))()
    for i, (sf, rdd) in enumerate(cfgs):
        arr[i] = _lib.DecoderCfg(C.sizeof(_lib.DecoderCfg), sf, 0, rdd, 1, 1, 0, 1, 0, 8)
    return arr


def encode(sf, rdd, count, stride, seed):
    """count packets of 8..64 random bytes under (sf, rdd) -> (rows (count, stride) int16, nsyms) on the device"""
    rng = np.random.default_rng(seed)
    enc = L.LoRaEncoder()
    enc.setSpreadFactor(sf); enc.setCodingRate(RATE[rdd])
    data = torch.from_numpy(rng.integers(0, 256, (count, 64)).astype(np.uint8)).cuda()
    nb = torch.from_numpy(rng.integers(8, 65, count).astype(np.int32)).cuda()
    syms, nsyms = enc.encode_batch(data, nb, sym_stride=stride)
    assert int(nsyms.min()) >= 8 and int(nsyms.max()) <= stride
    return syms, nsyms


def plan_of(cfgs, n, stride):
    t = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
    assert lib.lorahip_decode_plan(cfgs, n, stride, C.byref(t)) == 0
    return {f: int(getattr(t, f)) for f in ("lanes_per_packet", "sym_cap", "cw_cap", "lds_slice_bytes", "packets_per_workgroup")}


ctx.use_torch_stream()
pairs = [(sf, rdd) for sf in range(7, 13) for rdd in range(5)]
stride = max(int(lib.lorahip_encode_num_symbols(C.byref(_lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, 0, rdd, 1, 1, 1)), 64)) for sf, rdd in pairs)
per = a.packets // len(pairs)
P = per * len(pairs)
parts = [encode(sf, rdd, per, stride, 100 * sf + rdd) for sf, rdd in pairs]
perm = torch.from_numpy(np.random.default_rng(1).permutation(P)).cuda()
syms = torch.cat([s for s, _ in parts])[perm].contiguous()
nsyms = torch.cat([n for _, n in parts])[perm].contiguous()
index30 = torch.arange(30, dtype=torch.int32, device="cuda").repeat_interleave(per)[perm].contiguous()
index6 = (index30 // 5).to(torch.int32).contiguous()
out_stride = 2 * (stride + 8)
out = torch.zeros((P, out_stride), dtype=torch.uint8, device="cuda")
n_out, d_out = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
info = torch.zeros((P, 8), dtype=torch.int32, device="cuda")
tab30, tab6 = cfg_array(pairs), cfg_array([(sf, _lib.RDD_FROM_HEADER) for sf in range(7, 13)])


def fixed30():
    rc = lib.lorahip_decode_packets_cfgs(ctx._h, tab30, 30, index30.data_ptr(), None, 0, syms.data_ptr(), stride, nsyms.data_ptr(), P, out.data_ptr(), out_stride,
                                         n_out.data_ptr(), d_out.data_ptr())
    assert rc == 0, lib.lorahip_last_error()


def header6(report):
    rc = lib.lorahip_decode_packets_info(ctx._h, tab6, 6, index6.data_ptr(), None, 0, syms.data_ptr(), stride, nsyms.data_ptr(), P, out.data_ptr(), out_stride,
                                         n_out.data_ptr(), d_out.data_ptr(), info.data_ptr() if report else None)
    assert rc == 0, lib.lorahip_last_error()


def result():
    return out.clone(), n_out.clone(), d_out.clone()


# the launches give the same bytes before any of them is timed
fixed30(); want = result()
out.zero_(); header6(False); got = result()
out.zero_(); header6(True); got_i = result()
assert all(torch.equal(x, y) for x, y in zip(want, got)) and all(torch.equal(x, y) for x, y in zip(want, got_i))
assert int((want[1] > 0).sum()) == P and int(want[2].sum()) == 0
assert torch.equal(info[:, 1], index30 % 5) and bool((info[:, 2] == 1).all()) and not bool(info[:, 3].any())

times = {"fixed30": [], "header6": [], "header6_info": []}
for _ in range(a.rounds):                                            # in turn: the spread between rounds is what a difference has to exceed
    times["fixed30"].append(event_ms(fixed30))
    times["header6"].append(event_ms(lambda: header6(False)))
    times["header6_info"].append(event_ms(lambda: header6(True)))
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({"what": "header-rate table of 6 against the fixed-rate table of 30, same rows, mixed order", "packets": P, "sym_stride": stride,
                  "plan_fixed30": plan_of(tab30, 30, stride), "plan_header6": plan_of(tab6, 6, stride),
                  "fixed30_ms": [round(t, 4) for t in times["fixed30"]], "header6_ms": [round(t, 4) for t in times["header6"]],
                  "header6_info_ms": [round(t, 4) for t in times["header6_info"]],
                  "median_ms": {k: round(v, 4) for k, v in med.items()},
                  "spread_ms": {k: round(max(v) - min(v), 4) for k, v in times.items()},
                  "fixed30_packets_per_s": round(P / med["fixed30"] * 1e3), "header6_packets_per_s": round(P / med["header6"] * 1e3),
                  "header6_over_fixed30": round(med["header6"] / med["fixed30"], 4),
                  "header6_info_over_fixed30": round(med["header6_info"] / med["fixed30"], 4)}), flush=True)
ctx.close()
