"""GPU: the launch-uniform batch kernels' bin scan -- the arg-max through 64-bit max keys (lorahip_device.h: laneScanKeys,
groupMaxKeySumF64; FastCore::scan) -- against the CPU oracle.

The edge tests of test_gpu_parity.py ask for the fft / dec outputs and therefore run the debug-port instances, which scan with
compare-and-select. Every call here is ctx.detect_batch with NO want_fft / want_dec / fine_err / chirp_sel: the launch-uniform
instance runs. W = 67 windows per case: not a multiple of the windows per wavefront (16 / 8 / 4 / 4 / 1 at SF6..10) nor of 64, so
partial wavefronts and the flush of the deferred tails are covered; every eighth window stays an ordinary chirp + AWGN window, so a
wavefront mixes cases (the NaN branch is taken by whole wavefronts: clean windows go through it beside the NaN ones).

Tolerances are test_gpu_parity.py's: sym equal; power / powerAvg / fIndex of the same class (finite, +Inf, -Inf, NaN) and within
TOL_DB / TOL_FIDX or two float ulps, whichever is larger (the absolute bounds are below one ulp beyond 256 dB, where the
overflow amplitudes live); powerAvg of windows whose floor lies more than CLEAN_SNR_DB under the peak within TOL_DB_CLEAN."""
import functools

import numpy as np
import pytest

from test_gpu_parity import CLEAN_SNR_DB, TOL_DB, TOL_DB_CLEAN, TOL_FIDX, _bits_differ, make_iq, sym_np, to_np

pytestmark = pytest.mark.gpu

W = 67
SFS = [6, 7, 8, 9, 10]


@functools.lru_cache(maxsize=None)
def cases(sf):
    """[(name, iq[W, N] complex64)]: built once per SF and shared (read-only) by both tests"""
    N = 1 << sf
    rng = np.random.default_rng(700 + sf)
    base, _ = make_iq(rng, sf, W, snr_db=5.0)
    keep = np.arange(W) % 8 == 0                      # ordinary windows inside every case

    def mixed(x):
        x = np.array(x, np.complex64)
        x[keep] = base[keep]
        x.setflags(write=False)
        return x

    out = [("all-zero", mixed(np.zeros((W, N))))]
    for n in (0, N // 2, 1, 3, N - 1):
        x = np.zeros((W, N), np.complex64)
        x[:, n] = 1.0
        out.append(("lone sample at %d" % n, mixed(x)))
    out.append(("halfbin", mixed(make_iq(rng, sf, W, snr_db=None, kind="halfbin")[0])))
    out.append(("noise", mixed(make_iq(rng, sf, W, kind="noise")[0])))
    wide = base.astype(np.complex128)
    with np.errstate(over="ignore"):
        for scale in (1e-19, 1e-21, 3e-39, 1e18, 3e37):
            out.append(("amplitude %g" % scale, mixed((wide * scale).astype(np.complex64))))
    x = base.copy(); x[1::3, 5] = np.nan
    out.append(("NaN sample", mixed(x)))
    x = base.copy(); x[1::3, N // 2] = np.inf
    out.append(("infinite sample", mixed(x)))
    return out


_EXPECTED = {}


def expected(oracle, sf):
    """the oracle's outputs for cases(sf): computed once, shared by both tests"""
    if sf not in _EXPECTED:
        with np.errstate(all="ignore"):
            _EXPECTED[sf] = [oracle.detect_batch(sf, iq, want_fft=False) for _, iq in cases(sf)]
    return _EXPECTED[sf]


def compare(g, o, where):
    assert np.array_equal(sym_np(g["sym"]), o["sym"]), "sym " + where
    clean = np.isfinite(o["powerAvg"]) & ((o["power"].astype(np.float64) - o["powerAvg"]) > CLEAN_SNR_DB)
    for k in ("power", "powerAvg", "fIndex"):
        a, b = to_np(g[k]), o[k]
        for cls in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(cls(a), cls(b)), "%s class %s" % (k, where)
        f = np.isfinite(b)
        if f.any():
            tol = np.maximum(2 * np.spacing(np.abs(b[f]).astype(np.float32)), np.float32(TOL_FIDX if k == "fIndex" else TOL_DB))
            if k == "powerAvg":
                tol = np.where(clean[f], TOL_DB_CLEAN, tol)
            err = np.abs(a[f].astype(np.float64) - b[f])
            assert np.all(err <= tol), "%s differs by %g %s" % (k, err.max(), where)


@pytest.mark.parametrize("sf", SFS)
def test_key_scan_against_the_oracle(gpu, oracle, sf):
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    for (name, iq), o in zip(cases(sf), expected(oracle, sf)):
        g = ctx.detect_batch(gpu.from_numpy(iq).cuda())
        gpu.cuda.synchronize()
        compare(g, o, "sf%d %s" % (sf, name))
        # the sanity of the test itself: these cases are the ties they are meant to be (every bin the same |X|^2, or none taken)
        if name in ("all-zero", "lone sample at 0", "lone sample at %d" % (1 << (sf - 1))):
            assert np.all(o["sym"][np.arange(W) % 8 != 0] == 0), name
        if name == "infinite sample":
            hit = ~np.isfinite(iq).all(axis=1)
            assert hit.any() and not hit.all() and np.all(o["sym"][hit] == 0), name
    ctx.close()


@pytest.mark.parametrize("sf", SFS)
def test_key_scan_against_the_generic_kernel(gpu, oracle, sf):
    """variant 1 (detectGeneric: the compare-and-select scan) and the default: all four outputs bit for bit wherever the oracle's
    are finite"""
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    for (name, iq), o in zip(cases(sf), expected(oracle, sf)):
        d = gpu.from_numpy(iq).cuda()
        got = []
        for v in (1, 0):
            ctx.set_variant(v)
            g = ctx.detect_batch(d)
            gpu.cuda.synchronize()
            got.append({k: to_np(g[k]).copy() for k in ("sym", "power", "powerAvg", "fIndex")})
        where = "sf%d %s" % (sf, name)
        assert np.array_equal(got[0]["sym"].view(np.uint16), got[1]["sym"].view(np.uint16)), where
        for k in ("power", "powerAvg", "fIndex"):
            f = np.isfinite(o[k])
            assert _bits_differ(got[0][k][f], got[1][k][f]) == 0, where + " " + k
    ctx.close()
