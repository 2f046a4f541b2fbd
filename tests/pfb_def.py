"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the polyphase filter-bank channeliser's evaluation (include/lorahip.h):

    n_m    = (m + 1) D - 1
    v_s[m] = sum_{j<L, (n_m - j) mod M == s} h[j] x[n_m - j],   x[n<0] = 0
    y_b[m] = sum_{s<M} v_s[m] exp(-2 pi i b s / M)

The DEFINITION of the object's rows is the direct form's, oracle/channelizer.py::channelize(x, [b / M ...], D, h);
tests/test_pfb_cpu.py holds this file to it, and the GPU tests hold the fp32 kernel to that definition."""
import numpy as np


def fold(x, n_bins, decim, taps):
    """the M folded sums of every output time: (n_out, M) complex128"""
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    M, D, L = int(n_bins), int(decim), h.size
    n_out = x.size // D
    v = np.zeros((n_out, M), np.complex128)
    n_m = (np.arange(n_out, dtype=np.int64) + 1) * D - 1
    for j in range(L):
        n = n_m - j
        ok = n >= 0
        np.add.at(v, (np.nonzero(ok)[0], n[ok] % M), h[j] * x[n[ok]])
    return v


def channelize(x, n_bins, decim, taps, bins=None):
    """rows bins[i] (any integers, taken modulo M; None: 0 .. M - 1) of the bank: (K, len(x) // decim) complex128"""
    M = int(n_bins)
    b = np.arange(M) if bins is None else np.asarray(bins, np.int64) % M
    y = np.fft.fft(fold(x, M, decim, taps), axis=1)          # forward: exp(-2 pi i b s / M)
    return np.ascontiguousarray(y[:, b].T)


def scale(x, taps):
    """what no output can exceed: sum|h| * max|x|"""
    return float(np.abs(np.asarray(taps, np.float64)).sum() * np.abs(x).max())
