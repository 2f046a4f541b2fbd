"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the rational-rate resampler's definition (include/lorahip.h). The resampler is
not a reference component: this file DEFINES what the kernel must compute, tests/test_resampler_cpu.py holds it to an independent
construction from textbook pieces (scipy) and to the synthesiser's and the channeliser's definitions at D = 1 and U = 1, and the GPU
tests hold the fp32 kernel to it within a derived bound.

    t_m    = (m + 1) D - 1
    y_k[m] = sum_{j<L, (t_m - j) mod U == 0, t_m - j >= 0} h[j] x_k[(t_m - j) / U]
    x_k[n<0] = 0;  after N samples per row floor(N U / D) outputs per row exist
"""
import numpy as np


def out_count(n0, n, up, down):
    """outputs per row that the n samples following the first n0 give"""
    return (int(n0) + int(n)) * int(up) // int(down) - int(n0) * int(up) // int(down)


def resample(rows, up, down, taps, n0=0):
    """rows: (K, n) complex, the samples n0 .. n0 + n - 1 of every row of a stream whose samples before n0 are all zero; returns the
    (K, out_count(n0, n, up, down)) outputs floor(n0 U / D) .. floor((n0 + n) U / D) - 1 as complex128"""
    x = np.asarray(rows, np.complex128)
    h = np.asarray(taps, np.float64)
    U, D, n0 = int(up), int(down), int(n0)
    K, n = x.shape
    # Python integers: no limit on the stream position; t_m counted from the first zero-stuffed sample of rows
    t = np.array([(mm + 1) * D - 1 - n0 * U for mm in range(n0 * U // D, (n0 + n) * U // D)], np.int64)
    y = np.zeros((K, t.size), np.complex128)
    for k in range(K):
        z = np.zeros(max(n * U, 1), np.complex128)
        z[:n * U:U] = x[k]                                                 # zero-stuffed: the samples sit at multiples of U
        y[k] = np.convolve(z, h)[t]                                        # f[t] = sum_j h[j] z[t - j]
    return y


def resample_at(rows, up, down, taps, m=(), n0=0):
    """the definition for SELECTED outputs: m holds absolute output indices (integers), rows (K, cnt) the samples n0 .. n0 + cnt - 1 of
    every row; every sample outside them (and before the start of the stream) reads as 0. Returns (K, len(m)) complex128. Only the
    products the definition names are formed (j < L, (t_m - j) mod U == 0), so a non-finite sample reaches exactly those outputs."""
    x = np.asarray(rows, np.complex128)
    h = np.asarray(taps, np.float64)
    U, D, L, n0 = int(up), int(down), h.size, int(n0)
    K, cnt = x.shape
    t = [(int(mm) + 1) * D - 1 for mm in m]
    p = np.array([tt % U for tt in t], np.int64)
    c = np.array([tt // U - n0 for tt in t], np.int64)                     # the newest sample of every output, as a column of rows
    i = np.arange(-(-L // U), dtype=np.int64)
    j = p[:, None] + i[None, :] * U
    col = c[:, None] - i[None, :]
    ok = (j < L) & (col >= 0) & (col < cnt) & (col + n0 >= 0)
    hj = np.where(ok, h[np.minimum(j, L - 1)], 0.0)
    cc = np.clip(col, 0, max(cnt - 1, 0))
    if cnt == 0:
        return np.zeros((K, len(t)), np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sum(np.where(ok[None], hj[None] * x[:, cc], 0.0), axis=2)


def error_scale(rows, taps, up):
    """max|x| * max_p sum_i |h[p + i U]|: what no output can exceed"""
    h = np.abs(np.asarray(taps, np.float64))
    U = int(up)
    return float(np.abs(rows).max()) * max(float(h[p::U].sum()) for p in range(min(U, h.size)))


def nonfinite_outputs(c, up, down, n_taps, n0, n):
    """the absolute outputs m, among those of the samples n0 .. n0 + n - 1, that a non-finite sample at absolute index c reaches by
    the rule of the padded taps: floor(t_m / U) - T < c <= floor(t_m / U), T = ceil(L / U)"""
    U, D, T = int(up), int(down), -(-int(n_taps) // int(up))
    lo, hi = int(n0) * U // D, (int(n0) + int(n)) * U // D
    return [m for m in range(lo, hi) if ((m + 1) * D - 1) // U - T < c <= ((m + 1) * D - 1) // U]


# the bytes-to-bytes loopback at a rate off the grid (CPU from the definitions, GPU on the device): 8 channels 1/16 wide on a grid of
# 0.075 cycles per sample of the 16x stream, so that the outermost channel edge, 3.5 * 0.075 + 1/32 = 0.294, stays inside the flat
# band of design(6, 5, 192) and design(5, 6, 192) (both cut off at 0.5 cycles per sample of the 16x stream and are flat to about 0.3)
LOOPBACK_FREQS = (np.arange(8) - 3.5) * 0.075
LOOPBACK_INTERP, LOOPBACK_CHANNEL_TAPS, LOOPBACK_RESAMPLER_TAPS, LOOPBACK_SIGMA = 16, 128, 192, 0.2


def loopback_messages(sf):
    """one message of 4..24 random bytes for each of the 8 channels"""
    rng = np.random.default_rng(1000 + sf)
    return [rng.integers(0, 256, int(rng.integers(4, 25))).astype(np.uint8) for _ in range(8)]
