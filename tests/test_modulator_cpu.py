"""CPU: the modulator's definition (tests/modulator_def.py) pinned to the reference modulator -- the plain-C restatement
(oracle.mod_frame) always, the verbatim LoRaMod.cpp (ref.mod_frame) where it is built.

The criterion between DEFINITION and REFERENCE is the loose one, because the two evaluate cos / sin differently: the definition
rounds the double value once, the reference calls the platform's cosf / sinf (glibc: up to 0.56 ulp). A last-place difference there
is one ulp of ampl * cos when |ampl| is a power of two and up to two when it is not (modulator_def.ulp_bound), so

    same length; padding exactly zero; every non-zero sample within 1 ulp (|ampl| a power of two) or 2 ulps (any other);
    at most 5 % of them different at all (the cap of test_batched_modulator_matches_loramod).

The float32 frequency / phase recurrence itself must be IDENTICAL: an error in it does not stay in the last place, it grows along
the frame, which the long frames (600 symbols at SF7: a 255-byte packet) would show as a rising share.

Measured with glibc 2.3x on x86-64, over the cases below: worst 1 ulp at ampl 1, 0.5, 1e-40 (subnormal products), 2 ulps at 3.0,
-1.5 and 3e38; 0.96 % .. 1.18 % of the samples of a spreading factor differ, 1.26 % .. 1.29 % of a long frame's, whose first and last
tenth hold 201 and 192, 208 and 182, 227 and 203 differing components of some 16000 each.

The kernels are held to the definition, not to the reference, by tests/test_gpu_modulator_edges.py."""
import numpy as np
import pytest

import modulator_def as md

SFS = [6, 7, 9, 12]
SYNCS = [0x00, 0xff, 0x0f, 0xf0, 0x12]
PADDINGS = [0, 1, 2]
AMPLS = [1.0, 0.5, 3.0, -1.5, 0.0, 1e-40, 3e38]
LONG = [(7, 600), (6, 1200), (8, 300)]
SHARE = 5e-2


def symbol_rows(sf):
    """one symbol; the corners of the alphabet; symbols at and above N, which the modulator takes as given"""
    N = 1 << sf
    return [[0], [N - 1, 0, 1, N // 2, N - 1], [N, N + 1, 2 * N - 1, 65535, 3 * N + 5]]


_PHASES = {}


def phases(sf, row, sync):
    """the definition's phases of one frame, walked once per (sf, symbols) for all sync words together and shared by every case"""
    key = (sf, tuple(row))
    if key not in _PHASES:
        ph, live = md.mod_phases_def(sf, np.tile(np.asarray(row, np.uint16), (len(SYNCS), 1)), SYNCS)
        assert live.all()
        ph.setflags(write=False)
        _PHASES[key] = ph
    return _PHASES[key][SYNCS.index(sync)]


def definition_frame(sf, row, sync, ampl, padding):
    body = md.polar_def(ampl, phases(sf, row, sync))
    out = np.zeros(md.mod_frame_len_def(sf, len(row), padding), np.complex64)
    out[:body.size] = body
    return out


def compare(want, have, ampl, body):
    """-> (worst ulp, differing, compared) over the non-zero samples of the body; asserts length and zero padding"""
    assert have.shape == want.shape
    a, b = have.view(np.float32), want.view(np.float32)
    assert not a[2 * body:].any() and not b[2 * body:].any()
    a, b = a[:2 * body], b[:2 * body]
    if np.float32(ampl) == 0:
        assert not a.any() and not b.any()
        return 0, 0, 0
    d = md.ulp_distance(a, b)                              # counts through zero: a product of a subnormal amplitude can round to it
    return int(d.max()), int((d > 0).sum()), d.size


@pytest.fixture(scope="module")
def modulators(oracle):
    from oracle.oracle import Ref
    mods = [("oracle", oracle.mod_frame)]
    if Ref.available():
        mods.append(("ref", Ref().mod_frame))
    return mods


@pytest.mark.parametrize("sf", SFS)
def test_definition_against_the_reference_modulator(modulators, sf):
    """every symbol row x sync word x amplitude at padding 1; padding 0 and 2, which change the zero tail only, at ampl 1 and 3"""
    N = 1 << sf
    for name, mod_frame in modulators:
        worst_of, differ, total = {}, 0, 0
        for row in symbol_rows(sf):
            body = 14 * N + N // 4 + len(row) * N
            for sync in SYNCS:
                for padding in PADDINGS:
                    for ampl in (AMPLS if padding == 1 else (1.0, 3.0)):
                        want = mod_frame(sf, np.asarray(row, np.uint16), sync=sync, ampl=ampl, padding=padding)
                        have = definition_frame(sf, row, sync, ampl, padding)
                        w, d, t = compare(want, have, ampl, body)
                        assert w <= md.ulp_bound(ampl), (name, row, hex(sync), padding, ampl, w)
                        assert d <= SHARE * t, (name, row, hex(sync), padding, ampl, d, t)
                        worst_of[ampl] = max(worst_of.get(ampl, 0), w)
                        differ, total = differ + d, total + t
        print("SF%d %s: worst ulp by amplitude %s, %.2f %% of %d samples differ" % (sf, name, worst_of, 100.0 * differ / total, total))


@pytest.mark.parametrize("sf,nsyms", LONG)
def test_long_frames_do_not_drift(modulators, sf, nsyms):
    """frames of hundreds of symbols: the criterion holds over the whole frame, and the share of differing samples in the last tenth
    is that of the first tenth (both are samples of the same 1 .. 2 % population; a recurrence that drifted would push the last
    tenth towards 100 %, so 'at most twice the first tenth plus 1 %' separates the two without depending on the draw)"""
    N = 1 << sf
    syms = np.random.default_rng(100 + sf).integers(0, N, nsyms).astype(np.uint16)
    have = md.mod_frames_def(sf, syms[None, :], 0x12, 1.0, 1)[0]
    body = 14 * N + N // 4 + nsyms * N
    for name, mod_frame in modulators:
        want = mod_frame(sf, syms, sync=0x12, ampl=1.0, padding=1)
        w, d, t = compare(want, have, 1.0, body)
        assert w <= 1 and d <= SHARE * t, (name, w, d, t)
        dd = md.ulp_distance(have.view(np.float32)[:2 * body], want.view(np.float32)[:2 * body]) > 0
        tenth = dd.size // 10
        first, last = int(dd[:tenth].sum()), int(dd[-tenth:].sum())
        print("SF%d x %d %s: %.2f %% differ; first tenth %d, last tenth %d of %d" % (sf, nsyms, name, 100.0 * d / t, first, last, tenth))
        assert last <= 2 * first + tenth // 100, (name, first, last, tenth)


def test_frame_length(oracle):
    for sf in range(6, 13):
        for padding in (0, 1, 2, 5):
            for nsyms in (1, 2, 17):
                assert md.mod_frame_len_def(sf, nsyms, padding) == oracle.L.lo_mod_frame_len(sf, padding, nsyms), (sf, padding, nsyms)


def test_per_frame_counts_are_frames_with_more_padding():
    """with nsyms, row f is the frame of its first nsyms[f] symbols padded to the common length; silent rows are zero; what lies
    behind a row's count has no effect"""
    sf, S = 6, 4
    rng = np.random.default_rng(3)
    syms = rng.integers(0, 1 << sf, (6, S)).astype(np.uint16)
    n = np.array([S, 1, 0, -1, S + 1, 2], np.int32)
    rows = md.mod_frames_def(sf, syms, 0x12, 0.5, 2, nsyms=n)
    junk = syms.copy()
    for f, k in enumerate(n):
        junk[f, max(0, min(int(k), S)):] = 0xffff
    assert np.array_equal(rows.view(np.uint32), md.mod_frames_def(sf, junk, 0x12, 0.5, 2, nsyms=n).view(np.uint32))
    for f, k in enumerate(n):
        if k < 0 or k > S:
            assert not rows[f].any()
        elif k == 0:
            full = md.mod_frames_def(sf, syms[f:f + 1, :1], 0x12, 0.5, 2 + S - 1)[0]
            body = 14 * 64 + 16
            assert np.array_equal(rows[f, :body].view(np.uint32), full[:body].view(np.uint32)) and not rows[f, body:].any()
        else:
            full = md.mod_frames_def(sf, syms[f:f + 1, :k], 0x12, 0.5, 2 + S - k)[0]
            assert np.array_equal(rows[f].view(np.uint32), full.view(np.uint32))


def test_closed_form_is_the_recurrence_in_exact_arithmetic():
    """synth_symbols_def against the chirp it states, summed term by term in double: the two differ by double rounding only (1e-9 of
    a radian at SF12), symbols >= N give their masked value's window bit for bit"""
    for sf in (6, 9, 12):
        N = 1 << sf
        sym = np.array([0, 1, N // 2, N - 1, N, N + 5, 65535], np.uint16)
        got = md.synth_symbols_def(sf, sym, 0.75)
        assert np.array_equal(got[4:].view(np.uint32), md.synth_symbols_def(sf, sym[4:] & (N - 1), 0.75).view(np.uint32))
        n1 = np.arange(N) + 1.0
        for k, s in enumerate((sym & (N - 1)).tolist()):
            f = -np.pi + 2 * np.pi * s / N + n1 * (2 * np.pi / N)
            f = np.where(f > np.pi, f - 2 * np.pi, f)
            exact = 0.75 * np.exp(1j * np.cumsum(f))
            assert np.abs(got[k] - exact).max() <= 0.75 * (2.0 ** -24 + 1e-9 * N), (sf, s)


def test_double_cos_sin_rounded_once_is_the_correctly_rounded_float():
    """the definition's 'double value rounded once' against a 60-digit evaluation rounded once, on the phases of a frame: the two can
    differ only where the double result lies within its own error (< 1 ulp of double, 2^-29 ulp of float32) of a float32 rounding
    boundary, so on 2048 phases none is expected. (20480 phases of SF7 frames: 0.)"""
    mpmath = pytest.importorskip("mpmath")
    ph, _ = md.mod_phases_def(7, np.array([[5, 100]], np.uint16), 0x12)
    p = ph[0, 13 * 128:13 * 128 + 2048].astype(np.float64)
    c, s = np.cos(p).astype(np.float32), np.sin(p).astype(np.float32)
    off = 0
    with mpmath.workprec(200):
        for k, x in enumerate(p.tolist()):
            for exact, mine in ((mpmath.cos(x), c[k]), (mpmath.sin(x), s[k])):
                near = [abs(exact - mpmath.mpf(float(v))) for v in (mine, np.nextafter(mine, np.float32(-2)), np.nextafter(mine, np.float32(2)))]
                off += not (near[0] <= near[1] and near[0] <= near[2])       # mine is the float32 nearest the exact value
    assert off == 0
