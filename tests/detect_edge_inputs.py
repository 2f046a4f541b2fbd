"""The edge windows of lorahip_detect_batch and the call shapes that select its kernel instances: shared by
test_gpu_detect_instances.py (every shipped instance against the CPU oracle) and test_detect_compare_cpu.py (the comparison itself).

Three sets of inputs per SF, built once and read-only:
  1. the 15 cases of test_gpu_scan_keys.cases(sf), unchanged (W = 67, every eighth window an ordinary chirp + AWGN window);
  2. "twin tones": windows exp(2 pi i a t / N) + exp(2 pi i b t / N), no chirp: an exact two-bin tie inside one lane, across
     lanes and -- at SF11 / SF12 -- across wavefronts; the lowest bin wins. Padded to W = 67 with ordinary windows;
  3. "sweep": W = N windows, window k a tone at bin k + f_k, f_k = (0, +0.3, -0.3)[k mod 3], AWGN of sigma 0.05 per component, no
     dechirp: every lane, register slot and wavefront owns the peak once and hands over both neighbours once, the wrap at bins 0
     and N - 1 included. The off-bin thirds have |fIndex| ~ 0.07: swapped neighbours cannot hide inside TOL_FIDX.

Call shapes (shape_args): UNI -- no per-window argument; SEL -- a chirp_sel array; FINE -- fine_idx0 and a fine_err that is 0 on
even windows, so that moving and still windows share a wavefront. Sets 2 and 3 run without a chirp under UNI and SEL
(CHIRP_NONE); under FINE they are dechirped like any window (the fine-tune index only moves in dechirped windows), and are then
no ties and no sweep any more: plain windows compared with the oracle."""
import collections
import functools

import numpy as np

from test_gpu_parity import CLEAN_SNR_DB, make_iq
from test_gpu_scan_keys import W, cases

CHIRP_NONE = 2                    # lora_sdr_amd.CHIRP_NONE, the oracle's chirp_sel value too
SFS = [6, 7, 8, 9, 10, 11, 12]
SWEEP_OFFSETS = (0.0, 0.3, -0.3)
SWEEP_SIGMA = 0.05
TWIN_AT = (1, 10, 23, 40, 66)     # the windows of the twin-tone input that hold the pairs; 66 is alone in the last, partial set

Input = collections.namedtuple("Input", "kind name iq")      # kind: "scan" / "twins" / "sweep"


def twin_pairs(sf):
    """(a, b), a < b: bins of equal |X|^2"""
    N = 1 << sf
    pairs = [(5, 5 + N // 2), (0, N - 1), (63, 64), (127, 128), (N // 4 - 1, 3 * N // 4)]
    return [(a, b) for a, b in pairs if b < N]


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def inputs(sf):
    """[Input]: the 15 scan-key cases, the twin tones, the sweep"""
    N = 1 << sf
    t = np.arange(N)
    out = [Input("scan", name, iq) for name, iq in cases(sf)]

    rng = np.random.default_rng(800 + sf)
    x, _ = make_iq(rng, sf, W, snr_db=5.0)
    for w, (a, b) in zip(TWIN_AT, twin_pairs(sf)):
        x[w] = (np.exp(2j * np.pi * a * t / N) + np.exp(2j * np.pi * b * t / N)).astype(np.complex64)
    out.append(Input("twins", "twin tones", _frozen(x)))

    rng = np.random.default_rng(850 + sf)
    x = np.empty((N, N), np.complex64)
    step = max(1, (1 << 20) // N)                                        # rows per block: bounds the complex128 temporaries
    for k0 in range(0, N, step):
        k = np.arange(k0, min(N, k0 + step))
        f = k + np.asarray(SWEEP_OFFSETS)[k % 3]
        tone = np.exp(2j * np.pi * f[:, None] * t[None, :] / N)
        noise = rng.standard_normal((k.size, N, 2), np.float32).view(np.complex64)[..., 0]
        x[k] = tone.astype(np.complex64) + np.float32(SWEEP_SIGMA) * noise
    out.append(Input("sweep", "sweep", _frozen(x)))
    return out


def shape_args(sf, kind, n, shape):
    """the per-window arguments of one call shape for an input of n windows, as the oracle takes them (numpy; chirp_sel an int for
    a launch-uniform selection, absent for the default up-chirp)"""
    N = 1 << sf
    if shape == "UNI":
        return {} if kind == "scan" else {"chirp_sel": CHIRP_NONE}
    if shape == "SEL":
        sel = np.arange(n) % 3 if kind == "scan" else np.full(n, CHIRP_NONE)
        return {"chirp_sel": sel.astype(np.int32)}
    assert shape == "FINE"
    rng = np.random.default_rng(900 + sf)
    idx0 = rng.integers(0, 128 * N, n).astype(np.int32)
    err = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(-2.5, 2.5, n)).astype(np.float32)
    return {"fine_idx0": idx0, "fine_err": err}


_EXPECTED = {}


def expected(oracle, sf, shape):
    """the oracle's sym / power / powerAvg / fIndex / fineIdxOut for every input of inputs(sf) under one call shape: computed once"""
    if (sf, shape) not in _EXPECTED:
        with np.errstate(all="ignore"):
            _EXPECTED[sf, shape] = [oracle.detect_batch(sf, i.iq, nthreads=8, **shape_args(sf, i.kind, len(i.iq), shape)) for i in inputs(sf)]
    return _EXPECTED[sf, shape]


def clean_windows(o):
    """windows whose powerAvg the comparison checks to TOL_DB_CLEAN only: their fp64 total is not exact in every summation order"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(o["powerAvg"]) & ((o["power"].astype(np.float64) - o["powerAvg"]) > CLEAN_SNR_DB)


def has_infinite_sample(iq):
    return (np.isinf(iq.real) | np.isinf(iq.imag)).any(axis=1)


def check_inputs(oracle, sf, shape, outs):
    """the sanity of the inputs, on the ORACLE's values (outs: its results for inputs(sf) under `shape`): no clean window (so
    every fp64 total is exact and the instances can be compared bit for bit), the all-bin ties resolve to bin 0, windows with an
    infinite sample exist but are not all, and -- where nothing dechirps sets 2 and 3 -- the twins are exact ties won by the lower
    bin and every bin wins the sweep once"""
    N = 1 << sf
    for i, o in zip(inputs(sf), outs):
        assert clean_windows(o).sum() == 0, "sf%d %s %s: clean windows" % (sf, shape, i.name)
        if i.name in ("all-zero", "lone sample at 0", "lone sample at %d" % (N // 2)):
            assert np.all(o["sym"][np.arange(W) % 8 != 0] == 0), i.name
        if i.name == "infinite sample":
            hit = has_infinite_sample(i.iq)
            assert hit.any() and not hit.all() and np.all(o["sym"][hit] == 0), i.name
        if shape == "FINE":
            continue
        if i.kind == "twins":
            at = list(TWIN_AT[:len(twin_pairs(sf))])
            fft = oracle.detect_batch(sf, i.iq[at], chirp_sel=CHIRP_NONE, want_fft=True)["fft"]
            for w, row, (a, b) in zip(at, fft, twin_pairs(sf)):
                m = row.real * row.real + row.imag * row.imag            # fp32, as the scan of LoRaDetector.hpp:36-48 takes it
                assert m.dtype == np.float32 and m[a].tobytes() == m[b].tobytes(), "sf%d bins %d, %d are no tie: %r %r" % (sf, a, b, m[a], m[b])
                assert m[a] == m.max() and o["sym"][w] == a, "sf%d twin (%d, %d)" % (sf, a, b)
        if i.kind == "sweep":
            assert np.array_equal(o["sym"], np.arange(N)), "sf%d sweep" % sf
            off = np.arange(N) % 3 != 0
            # a tone 0.3 bins off the grid: fIndex ~ +-0.07 (the reference's estimator is biased low); 0.01 is 5000 TOL_FIDX
            assert np.all(np.sign(o["fIndex"][off]) == np.sign(np.asarray(SWEEP_OFFSETS)[np.arange(N) % 3][off]))
            assert np.all(np.abs(o["fIndex"][off]) > 0.01)
