"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the synthesiser's definition (include/lorahip.h). Like the channeliser, the
synthesiser is not a reference component: this file DEFINES what the kernel must compute, tests/test_synthesizer_cpu.py holds it to an
independent implementation from textbook pieces (scipy), and the GPU tests hold the fp32 kernel to it within a derived bound.

    y[n] = sum_k gain[k] exp(+2 pi i frac(w_k n / 2^64)) sum_{j<L, (n-j) mod U == 0, n-j >= 0} h[j] x_k[(n-j)/U]
    x_k[m<0] = 0,  w_k = floor(frac(f_k) 2^64),  f_k in cycles per OUTPUT sample
"""
import math

import numpy as np


def phase_inc(freq):
    """64-bit phase increment of a frequency (same arithmetic as lorahip_channelizer_phase_inc)"""
    frac = freq - math.floor(freq)
    return 0 if frac >= 1.0 else int(math.ldexp(frac, 64))


def synthesize(rows, freqs, interp, taps, gains=None, n0=0):
    """rows: (K, n) complex, the samples n0 .. n0 + n - 1 of every channel of a stream whose samples before n0 are all zero;
    returns the outputs n0 * interp .. (n0 + n) * interp - 1 as complex128"""
    x = np.asarray(rows, np.complex128)
    h = np.asarray(taps, np.float64)
    U = int(interp)
    K, n = x.shape
    g = np.ones(K) if gains is None else np.asarray(gains, np.float64)
    idx = np.uint64(int(n0) * U) + np.arange(n * U, dtype=np.uint64)         # absolute output indices (< 2^64)
    y = np.zeros(n * U, np.complex128)
    for k in range(K):
        z = np.zeros(n * U, np.complex128)
        z[::U] = x[k]                                                         # zero-stuffed: the non-zero inputs sit at multiples of U
        f = np.convolve(z, h)[: n * U]                                        # f[n] = sum_j h[j] z[n - j]
        with np.errstate(over="ignore"):
            ph = (np.uint64(phase_inc(freqs[k])) * idx).astype(np.int64)      # wraps mod 2^64, read as signed: turns * 2^64 in [-0.5, 0.5)
        y += g[k] * f * np.exp(2j * np.pi * (ph.astype(np.float64) * 2.0 ** -64))
    return y


def synthesize_at(rows, freqs, interp, taps, gains=None, n=(), n0=0):
    """the definition for SELECTED outputs: n holds absolute output indices (int array), rows (K, cnt) the samples n0 .. n0 + cnt - 1
    of every channel; every sample outside them (and before the start of the stream) reads as 0. Returns len(n) complex128. Only the
    products the definition names are formed (j < L, (n - j) mod U == 0), so a non-finite sample reaches exactly those outputs."""
    x = np.asarray(rows, np.complex128)
    h = np.asarray(taps, np.float64)
    U, L = int(interp), h.size
    K, cnt = x.shape
    g = np.ones(K) if gains is None else np.asarray(gains, np.float64)
    n = np.asarray(n, np.int64)
    i = np.arange(-(-L // U), dtype=np.int64)
    j = (n % U)[:, None] + i[None, :] * U                                     # the taps of output n: j = n mod U + i U
    c = (n // U)[:, None] - i[None, :] - int(n0)                              # and where their samples stand in rows
    ok = (j < L) & (c >= -int(n0)) & (c >= 0) & (c < cnt)
    hj = np.where(ok, h[np.minimum(j, L - 1)], 0.0)
    cc = np.clip(c, 0, max(cnt - 1, 0))
    w = np.array([phase_inc(f) for f in freqs], np.uint64)
    nu = n.astype(np.uint64)
    y = np.zeros(n.size, np.complex128)
    step = max(1, (1 << 21) // max(1, n.size * i.size))
    for a in range(0, K, step):
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.sum(np.where(ok[None], hj[None] * x[a:a + step][:, cc], 0.0), axis=2) if cnt else np.zeros((min(step, K - a), n.size))
            ph = (w[a:a + step, None] * nu[None, :]).astype(np.int64)         # wraps mod 2^64, read as signed
            y += np.sum(g[a:a + step, None] * f * np.exp(2j * np.pi * (ph.astype(np.float64) * 2.0 ** -64)), axis=0)
    return y


def error_scale(rows, taps, interp, gains=None):
    """max|x| * sum_k |gain_k| * max_p sum_i |h[p + i U]|: what no output can exceed"""
    h = np.abs(np.asarray(taps, np.float64))
    U = int(interp)
    K = np.asarray(rows).shape[0]
    g = float(K) if gains is None else float(np.abs(np.asarray(gains, np.float64)).sum())
    per_phase = max(float(h[p::U].sum()) for p in range(min(U, h.size)))
    return float(np.abs(rows).max()) * g * per_phase


def loopback_case(sf):
    """the inputs of the bytes-to-bytes loopback through one wideband stream (CPU from the definitions, GPU on the device): 8 channels
    on a 0.1-cycle grid at 16x the channel rate, one message of 4..24 random bytes each, 0 .. -14 dB of near/far"""
    rng = np.random.default_rng(sf)
    msgs = [rng.integers(0, 256, int(rng.integers(4, 25))).astype(np.uint8) for _ in range(8)]
    freqs = (np.arange(8) - 3.5) * 0.1
    gains = 10.0 ** (-2.0 * np.arange(8) / 20.0)
    return msgs, freqs, gains


def stagger(frames, step=37):
    """row k delayed by step * k samples (numpy or torch rows of equal length): the frames start at different times"""
    K, T = frames.shape
    if isinstance(frames, np.ndarray):
        rows = np.zeros((K, T + step * K), frames.dtype)
    else:
        import torch
        rows = torch.zeros((K, T + step * K), dtype=frames.dtype, device=frames.device)
    for k in range(K):
        rows[k, step * k:step * k + T] = frames[k]
    return rows
