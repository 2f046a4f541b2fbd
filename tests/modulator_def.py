"""TEST INFRASTRUCTURE ONLY -- the DEFINITION of the transmit waveform kernels' output (include/lorahip.h: lorahip_mod_frames,
lorahip_mod_frames_var, lorahip_synth_symbols), restated in numpy.

The modulator is a sequential float32 recurrence. With N = 2^sf and ALL state in float32

    fMin = f32(-pi), fMax = f32(pi), fStep = f32(2 pi / N), phase = 0 at the start of a frame

a chirp of n samples with start frequency f0 (computed in double, rounded once) is

    f = f32(fMin + f32(f0))
    n times:  f += fStep;  if f > fMax: f -= f32(fMax - fMin);  phase += f  (a down-chirp: phase -= f)
              sample = (f32(ampl) * f32(cos(double(phase))), f32(ampl) * f32(sin(double(phase))))
    phase = f32(p - floor(p / (2 pi)) * 2 pi),  p = double(phase)

and a frame is: 10 up-chirps of N; two sync chirps with f0 = 2 pi 8 (sync >> 4) / N and 2 pi 8 (sync & 15) / N; two down-chirps
of N and one of N / 4; one up-chirp per symbol with f0 = 2 pi sym / N, the symbol AS GIVEN (a symbol >= N is not masked: f then
stays above fMax, one wrap a sample does not bring it back, and the recurrence is followed all the same); max(1, padding) symbols
of zeros, which touch neither f nor the phase. ONE phase accumulator runs through the whole frame.

cos and sin are "the double value, rounded once to float32": that is what the kernels compute, and it is the correctly rounded
float32 value except where the double result lies within ~2^-28 ulp of a float32 rounding boundary (tests/test_modulator_cpu.py
counts those against a 60-digit evaluation). A float libm -- glibc's cosf / sinf, which the reference modulator calls -- is NOT
this: it misses the correctly rounded value in one to two per cent of the samples, by one ulp.

synth_symbols_def is lorahip_synth_symbols' closed form of ONE such up-chirp per window from phase 0, in double, with the symbol
masked to sf bits; the same double expressions in the same order as the kernel (the library is built without contraction, so the
phase is reproduced exactly). Its noise term is not part of this file (tests/test_gpu_noise.py)."""
import numpy as np

F32 = np.float32
TWO_PI = 2 * np.pi                                          # the double nearest 2 pi; 2 * pi_double is exact


def mod_frame_len_def(sf, nsyms, padding):
    """samples of a frame of nsyms symbols: 10 + 2 sync + 2.25 down + symbols + max(1, padding) zero symbols"""
    N = 1 << int(sf)
    return N * (10 + 2 + 2 + int(nsyms) + max(1, int(padding))) + N // 4


def mod_phases_def(sf, syms, sync, nsyms=None):
    """the float32 phase of every sample of the frames' body (everything before the zero padding) and which samples are chirp
    samples at all: ((F, 14.25 N + S N) float32, (F, same) bool). sync is one byte, or one per frame (the kernels take one per
    launch). With nsyms, frame f is walked over its first nsyms[f] symbols only and the rest of its body is not a chirp; a count
    below 0 or above S makes the whole row silent."""
    N = 1 << int(sf)
    syms = np.asarray(syms)
    assert syms.ndim == 2
    F, S = syms.shape
    syms = syms.astype(np.int64) & 0xffff                    # uint16 as given, NOT masked to sf bits
    sync = np.broadcast_to(np.asarray(sync, np.int64) & 0xff, (F,))
    if nsyms is None:
        count, silent = np.full(F, S, np.int64), np.zeros(F, bool)
    else:
        count = np.asarray(nsyms, np.int64).reshape(F)
        silent = (count < 0) | (count > S)
    fMin, fMax, fStep = F32(-np.pi), F32(np.pi), F32(TWO_PI / N)
    span = F32(fMax - fMin)
    zero = np.zeros(F, np.float64)
    # (f0 in double, down, samples, rows for which this is a chirp)
    chirps = [(zero, False, N, ~silent)] * 10
    chirps.append(((TWO_PI * ((sync >> 4) * 8)) / N, False, N, ~silent))
    chirps.append(((TWO_PI * ((sync & 15) * 8)) / N, False, N, ~silent))
    chirps += [(zero, True, N, ~silent), (zero, True, N, ~silent), (zero, True, N // 4, ~silent)]
    for k in range(S):
        chirps.append(((TWO_PI * syms[:, k]) / N, False, N, ~silent & (k < count)))
    L = sum(c[2] for c in chirps)
    phases, live = np.zeros((F, L), F32), np.zeros((F, L), bool)
    phase = np.zeros(F, F32)
    pos = 0
    for f0, down, n, on in chirps:
        f = (fMin + np.asarray(f0, np.float64).astype(F32)).astype(F32)
        acc = phase.copy()
        for i in range(n):
            f = f + fStep
            f = np.where(f > fMax, f - span, f)
            acc = acc - f if down else acc + f
            phases[:, pos + i] = acc
        assert f.dtype == F32 and acc.dtype == F32
        p = acc.astype(np.float64)
        with np.errstate(invalid="ignore"):
            red = (p - np.floor(p / TWO_PI) * TWO_PI).astype(F32)
        phase = np.where(on, red, phase)                     # a zero chirp leaves the accumulator alone
        live[on, pos:pos + n] = True
        pos += n
    return phases, live


def polar_def(ampl, phases, live=None):
    """(f32(ampl) * f32(cos(double(phase))), f32(ampl) * f32(sin(double(phase)))) as complex64; +0 where live is False"""
    a = F32(ampl)
    p = np.asarray(phases, F32).astype(np.float64)
    out = np.empty(p.shape + (2,), F32)
    with np.errstate(all="ignore"):
        out[..., 0] = a * np.cos(p).astype(F32)
        out[..., 1] = a * np.sin(p).astype(F32)
    if live is not None:
        out[~live] = 0.0
    return out.view(np.complex64)[..., 0]


def mod_frames_def(sf, syms, sync, ampl, padding, nsyms=None):
    """(F, mod_frame_len_def(sf, S, padding)) complex64: the frames of lorahip_mod_frames for the (F, S) symbols, or with nsyms the
    rows of lorahip_mod_frames_var"""
    phases, live = mod_phases_def(sf, syms, sync, nsyms)
    body = polar_def(ampl, phases, live)
    F, S = np.asarray(syms).shape
    out = np.zeros((F, mod_frame_len_def(sf, S, padding)), np.complex64)
    out[:, :body.shape[1]] = body
    return out


def synth_symbols_def(sf, sym, ampl):
    """(len(sym), N) complex64: lorahip_synth_symbols without noise. Window w is the up-chirp of symbol sym[w] & (N - 1) from phase
    0 in closed form: phi_i = sum_{j <= i} f_j, f_j = -pi + 2 pi s / N + (j + 1) 2 pi / N less 2 pi once it has passed +pi."""
    N = 1 << int(sf)
    s = (np.asarray(sym).astype(np.int64) & 0xffff & (N - 1))[:, None]
    i = np.arange(N, dtype=np.int64)[None, :]
    twoPiN = TWO_PI / N
    n1 = (i + 1).astype(np.float64)
    phi = n1 * (-np.pi + twoPiN * s.astype(np.float64)) + twoPiN * 0.5 * n1 * (n1 + 1.0)
    wrapped = i - (N - s) + 1
    phi = np.where(wrapped > 0, phi - TWO_PI * wrapped.astype(np.float64), phi)
    phi = phi - TWO_PI * np.floor(phi / TWO_PI)
    a = F32(ampl)
    out = np.empty((s.shape[0], N, 2), F32)
    out[..., 0] = a * np.cos(phi).astype(F32)
    out[..., 1] = a * np.sin(phi).astype(F32)
    return out.view(np.complex64)[..., 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the two criteria
# ---------------------------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """distance in float32 steps between two float32 arrays (ordered-integer map, so it counts through zero and the subnormals)"""
    ia = np.ascontiguousarray(a).view(np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b).view(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def is_power_of_two(ampl):
    a = abs(float(F32(ampl)))
    return a > 0 and np.isfinite(a) and np.frexp(a)[0] == 0.5


def ulp_bound(ampl):
    """a last-place difference in cos / sin is one ulp of the product when |ampl| is a power of two (the product is exact) and
    up to two when it is not: ampl * (c + ulp(c)) moves by ampl * ulp(c), which is between one and two ulps of a product that sits
    just above a power of two while c sits just below the next, and the product's own rounding can fall either way"""
    return 1 if is_power_of_two(ampl) else 2
