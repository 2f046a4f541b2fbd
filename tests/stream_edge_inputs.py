"""The edge streams of the streaming demodulator (mode 1: the frame machine on the device): shared by test_gpu_stream_instances.py
(every shipped streaming instance against the CPU oracle) and test_stream_edge_inputs_cpu.py (the inputs are what they claim to
be, on the oracle's own output).

Every stream is zeros(N + k), one frame of oracle.mod_frame(sf, syms, padding=1), zeros(2 N). The frame -- not the zeros -- carries
a carrier offset of (0, +0.3, -0.3)[channel mod 3] bins and AWGN of sigma 0.05 per component. The lead stays exact zeros: a zero
window is the all-bin tie (value 0, consumes N), so the window alignment at the frame's start is the chosen k and not a draw
of the noise. Three sets per SF, built once, read-only, fixed seeds:

  A  "data sweep": N / S channels of S data symbols, channel c sends (j B + c) mod N: every bin wins a data symbol once -- every
     lane, register slot and wavefront owns the peak of a DATASYMBOLS window once. Three ordinary channels of random symbols behind
     them make the channel count no multiple of the channels per wavefront or workgroup.
  B  "sync sweep": one channel per target bin b with the lead k = (1 - b) mod N: the first signal-bearing FRAMESYNC window
     peaks in b -- the window whose fIndex (both neighbours of the peak, the wrap at bins 0 and N - 1 included) goes into
     the fine-tune state. Every bin at SF6 to SF10; 256 strided bins and the 8 bins around 0, N / 2 and N - 1 at SF11 and SF12.
  C  "non-finite and extreme": NaN, +-Inf, overflowing and subnormal squares, all of them in DOWNCHIRP0, DOWNCHIRP1 or
     DATASYMBOLS windows: in FRAMESYNC the reference has no defined behaviour for them
     (test_gpu_demod.py::test_streams_with_non_finite_and_extreme_samples)."""
import collections
import functools

import numpy as np

SFS = [6, 7, 8, 9, 10, 11, 12]
SETS = ("A", "B", "C")
OFFSETS = (0.0, 0.3, -0.3)
SIGMA = 0.05
EXTRA_A = 3                        # the ordinary channels behind set A's sweep channels
# the seed of (sf, set) is 1500 + 16 sf + the set's position unless listed here. Set B's low targets have a lead near N: their first
# window holds a few dozen samples of the frame at -20 dB, and its fIndex is the noise's draw. At SF11 the default seed draws
# |fIndex| = 0.0036 for bin 31, which could hide a wrong neighbour less badly than the 0.01 asked of every off-bin channel
# (test_stream_edge_inputs_cpu.py, on the ORACLE's values); this one does not.
SEEDS = {(11, "B"): 3176}
PREAMBLE = 10                     # up-chirps in front of the two sync words (LoRaMod.cpp)

StreamSet = collections.namedtuple("StreamSet", "name mtu streams syms leads targets")
# streams: [complex64 (len,)] read-only; syms: [uint16 (S,)] what each channel sent; leads: [k]; targets: set B's bins (else None)


def symbols_per_frame(sf):
    return 64 if sf == 12 else 32


def sync_targets(sf):
    """set B's target bins, one channel each"""
    N = 1 << sf
    if sf <= 10:
        return list(range(N))
    # bin 2 first: its lead is N - 1, its first window holds ONE sample of the frame and is squelched at these SFs (snr -33 / -36 dB):
    # no fIndex to speak of, so it takes a slot without a carrier offset (channel 0)
    t = [2, 0, 1, N - 2, N - 1, N // 2 - 1, N // 2, N // 2 + 1]
    for j in range(256):
        b = j * (N // 256 + 1) % N
        if b not in t:
            t.append(b)
    return t


def _stream(oracle, rng, sf, syms, k, i):
    """zeros(N + k), the frame with channel i's carrier offset and the noise, zeros(2 N)"""
    N = 1 << sf
    fr = oracle.mod_frame(sf, syms, padding=1)
    off = OFFSETS[i % 3]
    if off:
        fr = (fr * np.exp(2j * np.pi * off * np.arange(fr.size) / N)).astype(np.complex64)
    fr = fr + np.float32(SIGMA) * rng.standard_normal((fr.size, 2), np.float32).view(np.complex64)[:, 0]
    st = np.zeros(N + k + fr.size + 2 * N, np.complex64)
    st[N + k:N + k + fr.size] = fr
    return st


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _build(sf, name):
    from oracle.oracle import Oracle
    oracle = Oracle()                                                  # the modulator only (bit-exact with the reference's)
    N = 1 << sf
    rng = np.random.default_rng(SEEDS.get((sf, name), 1500 + 16 * sf + SETS.index(name)))
    syms, leads, targets = [], [], None
    if name == "A":
        S = symbols_per_frame(sf)
        B = N // S
        for c in range(B):
            syms.append(((np.arange(S) * B + c) % N).astype(np.uint16))
            leads.append((c * S + 5) % N)
        for _ in range(EXTRA_A):
            syms.append(rng.integers(0, N, S).astype(np.uint16))
            leads.append(int(rng.integers(0, N)))
    elif name == "B":
        S = 2
        targets = sync_targets(sf)
        for b in targets:
            syms.append(rng.integers(0, N, S).astype(np.uint16))
            leads.append((1 - b) % N)
    else:
        S = 8
        for _ in range(7):
            syms.append(rng.integers(0, N, S).astype(np.uint16))
            leads.append(int(rng.integers(0, N)))
    streams = [_stream(oracle, rng, sf, s, k, i) for i, (s, k) in enumerate(zip(syms, leads))]
    if name == "C":
        nan, inf = np.float32(np.nan), np.float32(np.inf)
        f0 = [N + k for k in leads]
        d0 = [f + (PREAMBLE + 2) * N for f in f0]                       # DOWNCHIRP0's window
        d1 = [f + (PREAMBLE + 3) * N for f in f0]                       # DOWNCHIRP1's
        da = [f + (PREAMBLE + 4) * N + N // 4 for f in f0]              # the first data symbol
        streams[0][d0[0] + N // 3] = complex(nan, nan)
        streams[1][d1[1] + 5] = complex(inf, 0.0)
        streams[2][da[2] + 2 * N + 7] = complex(0.0, nan)
        streams[2][da[2] + 5 * N + N // 2] = complex(-inf, inf)
        streams[3][da[3] + 3 * N:da[3] + 4 * N] *= np.float32(3e19)     # |X|^2 overflows
        streams[4][da[4] + 7 * N + N // 2] = complex(3e38, -3e38)
        streams[5][:] *= np.float32(1e-21)                              # subnormal squares throughout
    return StreamSet(name, S, [_frozen(s) for s in streams], [_frozen(s) for s in syms], leads, targets)


def inputs(sf, name):
    """the StreamSet of one SF and set ("A" / "B" / "C")"""
    return _build(int(sf), name)


@functools.lru_cache(maxsize=None)
def rows(sf, name):
    """the set's streams as one read-only (channels, samples) array for the receivers that take a device buffer: zero padded at the
    end to a common length of whole 128-byte lines (16 samples)"""
    st = inputs(sf, name).streams
    cap = max(s.size for s in st)
    cap += -cap % 16
    out = np.zeros((len(st), cap), np.complex64)
    for c, s in enumerate(st):
        out[c, :s.size] = s
    return _frozen(out)


_EXPECTED = {}


def expected(oracle, sf, name, padded=False):
    """the oracle's restated LoRaDemod block over every stream of the set (padded: over the rows of rows(sf, name)), one
    demod_run dict per channel: computed once"""
    key = (int(sf), name, bool(padded))
    if key not in _EXPECTED:
        s = inputs(sf, name)
        with np.errstate(all="ignore"):
            _EXPECTED[key] = [oracle.demod_run(sf, st, mtu=s.mtu, keep=False) for st in (rows(sf, name) if padded else s.streams)]
    return _EXPECTED[key]
