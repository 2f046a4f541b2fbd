"""The decoder with the configuration per packet on one GPU: what does one table launch (lorahip_decode_packets_cfgs) cost against the
launches it replaces? P packets of 8..64 random bytes, split evenly over SF7..12, first at one coding rate (6 configurations), then at all
five (30), encoded by the batched encoder, in rows of the longest packet's symbols. Device-event times over --calls calls back to back, warm-up first, median of --reps:

    table      one table launch over the rows in mixed order (the order a receiver delivers: any configuration beside any other), and over
               the same rows sorted by configuration
    uniform    the 6 (30) lorahip_decode_packets launches of the same rows ALREADY bucketed by configuration, back to back on one stream --
               the bucketing itself (read back, sort, upload -- or a gather kernel) is not counted, which favours the old way
    one entry  a table of one entry against lorahip_decode_packets on the same P rows of one configuration (SF7 and SF12): what the table
               form itself costs

    python tools/bench_codec_var.py [--packets 65536] [--cr 4/8]"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lora_sdr_amd as L
from lora_sdr_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=65536); ap.add_argument("--cr", default="4/8"); ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--calls", type=int, default=20, help="calls between two events")
a = ap.parse_args()
assert a.reps >= 10, "median of at least 10"
P = a.packets
CR = {"4/4": 0, "4/5": 1, "4/6": 2, "4/7": 3, "4/8": 4}
RATE = {v: k for k, v in CR.items()}
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


class Rows:
    """decoder inputs and outputs that stay allocated: the timed calls launch and nothing else"""
    def __init__(self, syms, nsyms):
        self.syms, self.nsyms, self.P, self.stride = syms.contiguous(), nsyms.contiguous(), int(syms.shape[0]), int(syms.shape[1])
        self.out_stride = 2 * (self.stride + 8)
        self.out = torch.zeros((self.P, self.out_stride), dtype=torch.uint8, device="cuda")
        self.n = torch.zeros(self.P, dtype=torch.int32, device="cuda")
        self.d = torch.zeros(self.P, dtype=torch.int32, device="cuda")

    def table(self, cfgs, n_cfgs, index):
        rc = lib.lorahip_decode_packets_cfgs(ctx._h, cfgs, n_cfgs, index.data_ptr(), None, 0, self.syms.data_ptr(), self.stride, self.nsyms.data_ptr(), self.P,
                                             self.out.data_ptr(), self.out_stride, self.n.data_ptr(), self.d.data_ptr())
        assert rc == 0, lib.lorahip_last_error()

    def uniform(self, cfg, lo=0, hi=None):
        hi = self.P if hi is None else hi
        rc = lib.lorahip_decode_packets(ctx._h, cfg, self.syms.data_ptr() + 2 * lo * self.stride, self.stride, self.nsyms.data_ptr() + 4 * lo, hi - lo,
                                        self.out.data_ptr() + lo * self.out_stride, self.out_stride, self.n.data_ptr() + 4 * lo, self.d.data_ptr() + 4 * lo)
        assert rc == 0, lib.lorahip_last_error()

    def result(self):
        return self.out.clone(), self.n.clone(), self.d.clone()


ctx.use_torch_stream()
for rates in ([CR[a.cr]], [0, 1, 2, 3, 4]):
    cfgs = [(sf, rdd) for sf in range(7, 13) for rdd in rates]
    stride = max(int(L.load().lorahip_encode_num_symbols(C.byref(_lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, 0, rdd, 1, 1, 1)), 64)) for sf, rdd in cfgs)
    per = P // len(cfgs)
    parts = [encode(sf, rdd, per, stride, 100 * sf + rdd) for sf, rdd in cfgs]
    bucketed = Rows(torch.cat([s for s, _ in parts]), torch.cat([n for _, n in parts]))
    sorted_index = torch.arange(len(cfgs), dtype=torch.int32, device="cuda").repeat_interleave(per).contiguous()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(per * len(cfgs))).cuda()
    mixed = Rows(bucketed.syms[perm], bucketed.nsyms[perm])
    mixed_index = sorted_index[perm].contiguous()
    tab, one = cfg_array(cfgs), [cfg_array([c]) for c in cfgs]

    def uniform_all():
        for i in range(len(cfgs)):
            bucketed.uniform(one[i], i * per, (i + 1) * per)

    # the three ways give the same bytes before any of them is timed
    uniform_all(); want = bucketed.result()
    bucketed.table(tab, len(cfgs), sorted_index); got = bucketed.result()
    mixed.table(tab, len(cfgs), mixed_index); got_mixed = mixed.result()
    assert all(torch.equal(x, y) for x, y in zip(want, got)) and all(torch.equal(x[perm], y) for x, y in zip(want, got_mixed))
    assert int((want[1] > 0).sum()) == per * len(cfgs) and int(want[2].sum()) == 0
    t_uni = event_ms(uniform_all)
    t_tab_sorted = event_ms(lambda: bucketed.table(tab, len(cfgs), sorted_index))
    t_tab_mixed = event_ms(lambda: mixed.table(tab, len(cfgs), mixed_index))
    tiling = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
    assert lib.lorahip_decode_plan(tab, len(cfgs), stride, C.byref(tiling)) == 0
    plan = {f: int(getattr(tiling, f)) for f in ("lanes_per_packet", "sym_cap", "cw_cap", "lds_slice_bytes", "packets_per_workgroup")}
    n = per * len(cfgs)
    print(json.dumps({"what": "table against bucketed uniform launches", "configurations": len(cfgs), "rates": [RATE[r] for r in rates], "packets": n,
                      "sym_stride": stride, "plan": plan, "uniform_launches": len(cfgs), "uniform_ms": round(t_uni, 4),
                      "table_mixed_order_ms": round(t_tab_mixed, 4), "table_sorted_order_ms": round(t_tab_sorted, 4),
                      "uniform_packets_per_s": round(n / t_uni * 1e3), "table_mixed_packets_per_s": round(n / t_tab_mixed * 1e3),
                      "table_mixed_over_uniform": round(t_tab_mixed / t_uni, 4), "table_sorted_over_uniform": round(t_tab_sorted / t_uni, 4)}), flush=True)
    del bucketed, mixed, parts
    torch.cuda.empty_cache()

for sf in (7, 12):
    rdd = CR[a.cr]
    stride = int(L.load().lorahip_encode_num_symbols(C.byref(_lib.EncoderCfg(C.sizeof(_lib.EncoderCfg), sf, 0, rdd, 1, 1, 1)), 64))
    rows = Rows(*encode(sf, rdd, P, stride, sf))
    cfg = cfg_array([(sf, rdd)])
    zeros = torch.zeros(P, dtype=torch.int32, device="cuda")
    rows.uniform(cfg); want = rows.result()
    rows.table(cfg, 1, zeros)
    assert all(torch.equal(x, y) for x, y in zip(want, rows.result()))
    # in turn, four times: the spread between the rounds is what a difference between the two has to exceed
    tu, tt = [], []
    for _ in range(4):
        tu.append(event_ms(lambda: rows.uniform(cfg))); tt.append(event_ms(lambda: rows.table(cfg, 1, zeros)))
    print(json.dumps({"what": "one-entry table against the uniform entry", "sf": sf, "cr": a.cr, "packets": P, "sym_stride": stride,
                      "uniform_ms": [round(t, 4) for t in tu], "table_ms": [round(t, 4) for t in tt],
                      "table_over_uniform": round(float(np.median(tt) / np.median(tu)), 4)}), flush=True)
    del rows
    torch.cuda.empty_cache()
ctx.close()
