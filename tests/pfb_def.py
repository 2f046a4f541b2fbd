"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the polyphase filter-bank channeliser's evaluation (include/lorahip.h):

    n_m    = (m + 1) D - 1
    v_s[m] = sum_{j<L, (n_m - j) mod M == s} h[j] x[n_m - j],   x[n<0] = 0
    y_b[m] = sum_{s<M} v_s[m] exp(-2 pi i b s / M)

The DEFINITION of the object's rows is the direct form's, oracle/channelizer.py::channelize(x, [b / M ...], D, h);
tests/test_pfb_cpu.py holds this file to it, and the GPU tests hold the fp32 kernel to that definition."""
import numpy as np


def residues(n, n_bins):
    """n mod M of absolute sample indices as the definition takes it: Python integers or int64, never a float"""
    return np.asarray(n, np.int64) % int(n_bins)


def scale(x, taps):
    """what no output can exceed: sum|h| * max|x|"""
    return float(np.abs(np.asarray(taps, np.float64)).sum() * np.abs(x).max())


def out_times(n_in, decim, n0=0):
    """the output times m whose newest sample n_m lies in [n0, n0 + n_in): int64, (n0 + n_in) // D - n0 // D of them"""
    n0, D = int(n0), int(decim)
    return np.arange(n0 // D, (n0 + int(n_in)) // D, dtype=np.int64)


def fold(x, n_bins, decim, taps, n0=0):
    """the M folded sums of every output time: (n_out, M) complex128. x[i] is the sample of absolute index n0 + i (a Python integer
    of any size below 2^62) of a stream whose samples before n0 are all zero; the output times are out_times(len(x), decim, n0). The
    residue s is taken of the absolute index in 64-bit integers: nothing of the phase is left to floating point."""
    x = np.asarray(x, np.complex128)
    h = np.asarray(taps, np.float64)
    M, D, L = int(n_bins), int(decim), h.size
    n0 = int(n0)
    m = out_times(x.size, D, n0)
    v = np.zeros((m.size, M), np.complex128)
    n_m = (m + 1) * D - 1                                    # absolute, int64
    for j in range(L):
        n = n_m - j
        ok = n >= n0                                         # before n0 (and before the start of the stream): zeros
        np.add.at(v, (np.nonzero(ok)[0], residues(n[ok], M)), h[j] * x[n[ok] - n0])
    return v


def channelize(x, n_bins, decim, taps, bins=None, n0=0):
    """rows bins[i] (any integers, taken modulo M; None: 0 .. M - 1) of the bank: (K, len(x) // decim) complex128. With n0 > 0: x
    holds the samples n0 .. n0 + len(x) - 1 behind n0 zeros, and the outputs are those of out_times(len(x), decim, n0). The phase of
    every term is exp(-2 pi i ((b mod M) (n mod M) mod M) / M) with n the absolute 64-bit index: the transform below sees integers
    in [0, M) alone."""
    M = int(n_bins)
    b = np.arange(M) if bins is None else np.asarray(bins, np.int64) % M
    y = np.fft.fft(fold(x, M, decim, taps, n0), axis=1)      # forward: exp(-2 pi i b s / M)
    return np.ascontiguousarray(y[:, b].T)
