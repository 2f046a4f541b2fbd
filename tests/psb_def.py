"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the polyphase synthesis filter bank's evaluation (include/lorahip.h):

    X_b[m] = sum_{k : b_k mod M == b} g_k x_k[m]
    u_s[m] = sum_{b<M} X_b[m] exp(+2 pi i b s / M)
    y[n]   = sum_{i : p + iU < L, n/U - i >= 0} h[p + iU] u_{n mod M}[n/U - i],   p = n mod U

The DEFINITION of the object's output is the direct form's, tests/synthesizer_def.py::synthesize(rows, bins / M, U, h, gains);
tests/test_psb_cpu.py holds this file to it, and the GPU tests hold the fp32 kernel to that definition."""
import numpy as np


def gather(rows, n_bins, bins=None, gains=None):
    """the M bin sums of every input time: (n, M) complex128"""
    x = np.asarray(rows, np.complex128)
    K, n = x.shape
    M = int(n_bins)
    b = np.arange(K) % M if bins is None else np.asarray(bins, np.int64) % M
    g = np.ones(K) if gains is None else np.asarray(gains, np.float64)
    X = np.zeros((n, M), np.complex128)
    for k in range(K):
        X[:, b[k]] += g[k] * x[k]
    return X


def synthesize(rows, n_bins, interp, taps, bins=None, gains=None):
    """the n * interp outputs of a stream that starts with rows[:, 0]: complex128"""
    h = np.asarray(taps, np.float64)
    M, U, L = int(n_bins), int(interp), h.size
    X = gather(rows, M, bins, gains)
    n = X.shape[0]
    u = np.fft.ifft(X, axis=1) * M                           # unnormalised inverse: exp(+2 pi i b s / M)
    nn = np.arange(n * U, dtype=np.int64)
    p, m, s = nn % U, nn // U, nn % M
    y = np.zeros(n * U, np.complex128)
    for i in range(-(-L // U)):
        ok = (p + i * U < L) & (m - i >= 0)
        y[ok] += h[(p + i * U)[ok]] * u[(m - i)[ok], s[ok]]
    return y
