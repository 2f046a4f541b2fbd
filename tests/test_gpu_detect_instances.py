"""GPU: edge windows through every shipped instance of lorahip_detect_batch.

The batch entry runs a different kernel instance per SF, variant and shape of the call (launchByShape in lorahip_fast.hip,
launchWideByShape in lorahip_wide.hip): launch-uniform (no chirp_sel array, no fine_err), per-window settings (either of them,
no debug port), debug ports (want_fft / want_dec) -- each under variant 0 and variant 10, 42 tuned instances beside the generic
kernel (variant 1). The inputs of detect_edge_inputs.py -- exact ties, near-ties decided by rounding, NaN / Inf samples, subnormal
and overflowing squares, all-zero windows, a peak in every bin once -- go through all of them:

  shape UNI    the launch-uniform instances
  shape SEL    the per-window-settings instances by a chirp_sel array
  shape FINE   the per-window-settings instances by fine_idx0 / fine_err, moving and still windows in one wavefront
  shape PORTS  the debug-port instances, with UNI's and with FINE's arguments

Against the oracle: test_gpu_scan_keys.compare (sym equal; power / powerAvg / fIndex of the same class and within TOL_DB /
TOL_FIDX or two float ulps), fineIdxOut equal where a fine_idx0 goes in, and for PORTS dec and fft bit for bit -- except the bins
of a window that holds an infinite sample, handled as test_gpu_parity.test_inputs_at_the_edges_of_fp32 handles them (DESIGN.md
section 2: Inf * 0 of a skipped unit twiddle; every |X|^2 of such a window is NaN on both sides). Across instances: variants 0
and 10 against variant 1, sym bit for bit and the three floats bit for bit wherever the oracle's value is finite. That rests on
exact fp64 totals, i.e. on the inputs holding no window of more than CLEAN_SNR_DB between peak and floor: check_inputs asserts
that, and the rest of what the inputs are meant to be, on the oracle's output.

What it found when written (profiles/r13/README.md): under PORTS with FINE's arguments the fft port of variants 0 and 10 had the
sign of a zero wrong in 2 to 10 floats of the all-zero case at every SF -- the skipped multiplication by twiddle(0) of phase 0,
which the debug-port instances now carry out. Every other instance, shape and input agreed with the oracle and the generic kernel."""
import numpy as np
import pytest

from detect_edge_inputs import SFS, check_inputs, expected, has_infinite_sample, inputs, shape_args
from test_gpu_parity import _bits_differ, sym_np, to_np
from test_gpu_scan_keys import compare

pytestmark = pytest.mark.gpu

FLOATS = ("power", "powerAvg", "fIndex")


def device_args(torch, args):
    kw = {}
    for k, v in args.items():
        if isinstance(v, np.ndarray):
            kw[k] = torch.from_numpy(v).cuda()
        else:
            kw["chirp_sel_all"] = v
    return kw


def compare_ports(g, o, iq, where):
    """dec and fft bit for bit; the bins of windows with an infinite sample: every |X|^2 NaN on both sides"""
    assert _bits_differ(to_np(g["dec"]), o["dec"]) == 0, "dec " + where
    gf, of = to_np(g["fft"]), o["fft"]
    hit = has_infinite_sample(iq)
    assert _bits_differ(gf[~hit], of[~hit]) == 0, "fft " + where
    for f in (gf[hit], of[hit]):
        with np.errstate(all="ignore"):
            m = f.real.astype(np.float32) ** 2 + f.imag.astype(np.float32) ** 2
        assert np.isnan(m).all(), "fft of the windows with an infinite sample " + where
    assert np.all(o["sym"][hit] == 0), where


@pytest.mark.parametrize("shape", ["UNI", "SEL", "FINE", "PORTS"])
@pytest.mark.parametrize("sf", SFS)
def test_edge_windows_through_every_instance(gpu, oracle, sf, shape):
    import lora_sdr_amd as L
    ports = shape == "PORTS"
    ctx = L.Context(sf)
    try:
        for sub in (("UNI", "FINE") if ports else (shape,)):
            outs = expected(oracle, sf, sub)
            check_inputs(oracle, sf, sub, outs)
            for i, o in zip(inputs(sf), outs):
                args = shape_args(sf, i.kind, len(i.iq), sub)
                if ports:                                               # the oracle's ports are not kept: the sweep's are 2 x 134 MB at SF12
                    with np.errstate(all="ignore"):
                        o = oracle.detect_batch(sf, i.iq, want_fft=True, want_dec=True, nthreads=8, **args)
                d = gpu.from_numpy(i.iq).cuda()
                kw = device_args(gpu, args)
                got = {}
                for v in (1, 0, 10):
                    where = "sf%d %s%s variant %d: %s" % (sf, sub, " with ports" if ports else "", v, i.name)
                    ctx.set_variant(v)
                    g = ctx.detect_batch(d, want_fft=ports, want_dec=ports, want_fine_idx=True, **kw)
                    gpu.cuda.synchronize()
                    compare(g, o, where)
                    if "fine_idx0" in args:
                        assert np.array_equal(to_np(g["fineIdxOut"]), o["fineIdxOut"]), "fineIdxOut " + where
                    if ports:
                        compare_ports(g, o, i.iq, where)
                    got[v] = dict({k: to_np(g[k]).copy() for k in FLOATS}, sym=sym_np(g["sym"]).copy())
                for v in (0, 10):
                    where = "sf%d %s%s variant %d against the generic kernel: %s" % (sf, sub, " with ports" if ports else "", v, i.name)
                    assert np.array_equal(got[v]["sym"], got[1]["sym"]), "sym " + where
                    for k in FLOATS:
                        f = np.isfinite(o[k])
                        assert _bits_differ(got[v][k][f], got[1][k][f]) == 0, k + " " + where
    finally:
        ctx.close()
