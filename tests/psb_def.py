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


def residues(n, n_bins):
    """n mod M of absolute output indices as the definition takes it: Python integers or int64, never a float"""
    return np.asarray(n, np.int64) % int(n_bins)


def synthesize(rows, n_bins, interp, taps, bins=None, gains=None, n0=0):
    """the n * interp outputs of a stream that starts with rows[:, 0]: complex128. With n0 > 0 (a Python integer; n0 * interp below
    2^62): rows holds the input times n0 .. n0 + n - 1 behind n0 zeros, and the outputs are n0 * interp .. (n0 + n) * interp - 1.
    The residue s is taken of the absolute output index in 64-bit integers, so the phase of every term is
    exp(+2 pi i ((b mod M) (n mod M) mod M) / M): the transform below sees integers in [0, M) alone."""
    h = np.asarray(taps, np.float64)
    M, U, L = int(n_bins), int(interp), h.size
    n0 = int(n0)
    X = gather(rows, M, bins, gains)
    n = X.shape[0]
    u = np.fft.ifft(X, axis=1) * M                           # unnormalised inverse: exp(+2 pi i b s / M)
    nn = n0 * U + np.arange(n * U, dtype=np.int64)           # absolute
    p, m, s = nn % U, nn // U - n0, residues(nn, M)          # m: the input time in rows
    y = np.zeros(n * U, np.complex128)
    for i in range(-(-L // U)):
        ok = (p + i * U < L) & (m - i >= 0)
        y[ok] += h[(p + i * U)[ok]] * u[(m - i)[ok], s[ok]]
    return y


def synthesize_at(rows, n_bins, interp, taps, bins=None, gains=None, n=(), n0=0):
    """the same for SELECTED outputs, in the direct form: n holds absolute output indices (int64), rows (K, cnt) the input times
    n0 .. n0 + cnt - 1; every input time outside them reads as 0. Returns len(n) complex128:

        y[n] = sum_k g_k exp(+2 pi i ((b_k mod M) (n mod M) mod M) / M) sum_{i : p + iU < L} h[p + iU] x_k[n/U - i],   p = n mod U

    Only the products the definition names are formed, so a non-finite sample reaches exactly those outputs."""
    x = np.asarray(rows, np.complex128)
    h = np.asarray(taps, np.float64)
    M, U, L = int(n_bins), int(interp), h.size
    K, cnt = x.shape
    b = np.arange(K) % M if bins is None else np.asarray(bins, np.int64) % M
    g = np.ones(K) if gains is None else np.asarray(gains, np.float64)
    n = np.asarray(n, np.int64)
    i = np.arange(-(-L // U), dtype=np.int64)
    j = (n % U)[:, None] + i[None, :] * U                    # the taps of output n
    c = (n // U)[:, None] - i[None, :] - int(n0)             # and where their samples stand in rows
    ok = (j < L) & (c >= 0) & (c < cnt)
    hj = np.where(ok, h[np.minimum(j, L - 1)], 0.0)
    cc = np.clip(c, 0, max(cnt - 1, 0))
    turns = (b[:, None] * residues(n, M)[None, :]) % M       # integers in [0, M)
    y = np.zeros(n.size, np.complex128)
    step = max(1, (1 << 21) // max(1, n.size * i.size))
    for a in range(0, K, step):
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.sum(np.where(ok[None], hj[None] * x[a:a + step][:, cc], 0.0), axis=2)
            y += np.sum(g[a:a + step, None] * f * np.exp(2j * np.pi * turns[a:a + step] / M), axis=0)
    return y
