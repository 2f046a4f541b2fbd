"""GPU: the transmit waveform kernels at the edges of their definition -- modFrames through both its entry points
(lorahip_mod_frames, lorahip_mod_frames_var) and synthSymbols, all in lorahip_tx.hip -- against tests/modulator_def.py.

The comparison is with what the kernels COMPUTE, the reference's float32 recurrence with cos / sin taken in double and rounded once
(the definition), not with the reference modulator's own cosf / sinf: tests/test_modulator_cpu.py holds the definition to the
reference within the loose criterion (1 or 2 ulps, a percent or two of the samples), and here a kernel has to be DEFINITION-EQUAL:

    every component is of the definition's class (NaN, +Inf, -Inf, zero, finite non-zero);
    every finite non-zero component is within 1 ulp of it when |ampl| is a power of two, within 2 ulps otherwise;
    at most 1e-4 of the components differ at all.

1e-4 is a condition, not a measurement: any evaluation of cos / sin in float differs from the double value rounded once in about
1 % of the components, a hundred times the bound, so the share tells "double, rounded once" from everything else; the expected count
is zero, since the device's and the host's double sincos can round to different floats only within ~2^-28 ulp of a rounding boundary.
Every frame and every window of every launch is compared. The counts are printed (`-s`); measured on an MI355X they are in DESIGN.md
(section "Modulator and symbol generator: the definition").

    what                                                         test
    SF 6 .. 12, 70 frames (SF6: the quarter down-chirp is        test_every_spreading_factor
    exactly one 16-sample staging block)
    symbols 0, 1, N/2, N-1 and N, N+1, 2N-1, 65535, 3N+5          test_symbol_and_sync_edges
    (taken unmasked); sync 0x00, 0xff, 0x0f, 0xf0, 0x12
    F = 1, 63, 64, 65, 255, 256, 257; rows of an odd stride at    test_frame_counts_at_the_lane_and_block_boundaries
    an odd offset; a sentinel around every frame
    600 symbols at SF7, 1200 at SF6: no growth along the frame    test_long_frames
    ampl 3, -1.5, 0, 1e-40, 3e38, +Inf, NaN                       test_amplitudes
    padding 0 == padding 1; padding 5; two launches               test_padding_and_determinism
    nsyms 0 and 2^23, padding 2^23, a short stride, null          test_refusals_leave_the_output_alone
    pointers; n_frames 0; frame length of SF 5 and 13
    per-frame counts 0, 1, max, max + 1, -1, -2 at lanes 0, 63,   test_per_frame_counts
    64, F - 1; a loose symbol stride; 0xffff behind the count
    synthSymbols SF 6 .. 12, ampl 0.75 and 3; symbols >= N        test_synth_symbols
    8193 windows at SF6: the grid-stride loop's second pass       test_synth_symbols_second_pass_of_the_grid_stride_loop

synth_symbols(noise_sigma, seed) == add_awgn(synth_symbols(0), sigma, seed) bit for bit is tests/test_gpu_noise.py's
(test_synth_noise_is_add_awgn) and not repeated here."""
import ctypes as C

import numpy as np
import pytest

from conftest import same_values

import modulator_def as md

pytestmark = pytest.mark.gpu

SHARE = 1e-4
E_INVALID = -1
SYNCS = [0x00, 0xff, 0x0f, 0xf0, 0x12]
SENTINEL = 9.0 + 7.0j


def f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(f32(a).view(np.uint32), f32(b).view(np.uint32))


def differing(got, want):
    """which components differ at all (NaN against NaN and +0 against -0 do not)"""
    a, b = f32(got), f32(want)
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def definition_equal(got, want, ampl, what):
    """the criterion of this file; -> the number of components that differ"""
    assert got.shape == want.shape, what
    a, b = f32(got).ravel(), f32(want).ravel()
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN where the definition has none, or the reverse"
    inf = np.isinf(a) | np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), what + ": infinities"
    assert np.array_equal(a == 0, b == 0), what + ": zeros"
    fin = np.isfinite(b) & (b != 0)
    d = md.ulp_distance(a[fin], b[fin])
    worst, differ = int(d.max(initial=0)), int((d > 0).sum())
    print("%s: %d of %d components differ, worst %d ulp" % (what, differ, a.size, worst))
    assert worst <= md.ulp_bound(ampl), "%s: %d ulps from the definition" % (what, worst)
    assert differ <= SHARE * a.size, "%s: %d of %d components differ from the definition" % (what, differ, a.size)
    return differ


def dev_syms(torch, syms):
    return torch.from_numpy(np.ascontiguousarray(syms, np.uint16).view(np.int16)).cuda()


def frames(torch, ctx, syms, sync=0x12, ampl=1.0, padding=1, **kw):
    iq = ctx.mod_frames(dev_syms(torch, syms), sync=sync, ampl=ampl, padding=padding, **kw)
    torch.cuda.synchronize()
    return iq.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the uniform modulator
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf", [6, 7, 8, 9, 10, 11, 12])
def test_every_spreading_factor(gpu, sf):
    import lora_sdr_amd as L
    syms = np.random.default_rng(sf).integers(0, 1 << sf, (70, 3)).astype(np.uint16)
    ctx = L.Context(sf)
    got = frames(gpu, ctx, syms, lead=5, tail=3)
    assert got.shape == (70, 5 + md.mod_frame_len_def(sf, 3, 1) + 3) == (70, 5 + ctx.mod_frame_len(3, 1) + 3)
    assert not got[:, :5].any() and not got[:, -3:].any()
    definition_equal(got[:, 5:-3], md.mod_frames_def(sf, syms, 0x12, 1.0, 1), 1.0, "SF%d" % sf)
    ctx.close()


@pytest.mark.parametrize("sf", [6, 7, 12])
def test_symbol_and_sync_edges(gpu, sf):
    """the symbol rows and sync words of tests/test_modulator_cpu.py. Symbols >= N are used as given, as the reference uses them:
    their frames differ from the masked symbols' in far more than the criterion's share of components (asserted on the definition,
    so that the comparison cannot pass on a masking definition and a masking kernel)"""
    import lora_sdr_amd as L
    N = 1 << sf
    one = np.array([[0]], np.uint16)
    five = np.array([[N - 1, 0, 1, N // 2, N - 1], [N, N + 1, 2 * N - 1, 65535, 3 * N + 5]], np.uint16)
    # the definition, walked once for all sync words: rows (sync, symbol row)
    want1 = md.mod_frames_def(sf, np.repeat(one, len(SYNCS), 0), SYNCS, 1.0, 1)
    want5 = md.mod_frames_def(sf, np.tile(five, (len(SYNCS), 1)), np.repeat(SYNCS, 2), 1.0, 1).reshape(len(SYNCS), 2, -1)
    masked = md.mod_frames_def(sf, five[1:] & (N - 1), 0x12, 1.0, 1)[0]
    assert differing(want5[4, 1], masked).mean() > 100 * SHARE
    ctx = L.Context(sf)
    F = 66
    differ = 0
    for k, sync in enumerate(SYNCS):
        # every frame of a launch: all frames of one symbol row carry the bits of the first, and that one is compared
        got = frames(gpu, ctx, np.repeat(one, F, 0), sync=sync)
        assert (f32(got).view(np.uint32) == f32(got[0]).view(np.uint32)).all()
        differ += definition_equal(got[:1], want1[k:k + 1], 1.0, "SF%d sync %#04x one symbol" % (sf, sync))
        got = frames(gpu, ctx, np.tile(five, (F // 2, 1)), sync=sync)
        u = f32(got).view(np.uint32).reshape(F // 2, 2, -1)
        assert (u == u[0]).all()
        differ += definition_equal(got[:2], want5[k], 1.0, "SF%d sync %#04x five symbols" % (sf, sync))
    print("SF%d: %d components differ over all sync words" % (sf, differ))
    ctx.close()


_BOUNDARY = {}


def boundary_case():
    """257 frames of 2 symbols at SF6 and their definition, computed once; a launch of F frames is its first F rows"""
    if not _BOUNDARY:
        syms = np.random.default_rng(6).integers(0, 64, (257, 2)).astype(np.uint16)
        want = md.mod_frames_def(6, syms, 0x12, 1.0, 1)
        want.setflags(write=False)
        _BOUNDARY["case"] = (syms, want)
    return _BOUNDARY["case"]


def raw_mod_frames(torch, L, ctx, syms, sync, ampl, padding, stride, lead=5, tail=3, nsyms=None, sym_stride=None, max_nsyms=None):
    """lorahip_mod_frames / _var into a buffer filled with a sentinel: rows of `stride` samples from `lead` samples into the
    allocation, `tail` samples behind the last row. -> (rc, the whole buffer on the host)"""
    lib = L.load()
    F = syms.shape[0]
    buf = torch.full((lead + F * stride + tail,), SENTINEL, dtype=torch.complex64, device="cuda")
    d = dev_syms(torch, syms)
    ctx.use_torch_stream()
    base = C.c_void_p(buf.data_ptr() + 8 * lead)
    if nsyms is None:
        rc = lib.lorahip_mod_frames(ctx._h, base, stride, C.c_void_p(d.data_ptr()), F, syms.shape[1], sync, ampl, padding)
    else:
        dn = torch.from_numpy(np.ascontiguousarray(nsyms, np.int32)).cuda()
        rc = lib.lorahip_mod_frames_var(ctx._h, base, stride, C.c_void_p(d.data_ptr()), sym_stride, C.c_void_p(dn.data_ptr()), F, max_nsyms,
                                        sync, ampl, padding)
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()


def split_rows(buf, F, stride, flen, lead=5):
    """-> (the F frames, everything else) of a raw_mod_frames buffer"""
    body = buf[lead:lead + F * stride].reshape(F, stride)
    rest = np.concatenate([buf[:lead], body[:, flen:].ravel(), buf[lead + F * stride:]])
    return body[:, :flen], rest


@pytest.mark.parametrize("F", [1, 63, 64, 65, 255, 256, 257])
def test_frame_counts_at_the_lane_and_block_boundaries(gpu, F):
    """a wavefront holds 64 frames and a workgroup 256: one frame, one lane short of, exactly and one lane past each. Rows of
    frame length + 3 samples from 5 samples into the allocation, so that no row is 16-byte aligned and the staged 128-byte stores
    straddle; the samples before, between and behind the frames keep their sentinel"""
    import lora_sdr_amd as L
    syms, want = boundary_case()
    ctx = L.Context(6)
    flen = md.mod_frame_len_def(6, 2, 1)
    rc, buf = raw_mod_frames(gpu, L, ctx, syms[:F], 0x12, 1.0, 1, flen + 3)
    assert rc == 0
    got, rest = split_rows(buf, F, flen + 3, flen)
    assert rest.size == 5 + 3 * F + 3 and (rest == np.complex64(SENTINEL)).all(), "samples outside the frames were written"
    definition_equal(got, want[:F], 1.0, "SF6 F = %d" % F)
    ctx.close()


@pytest.mark.parametrize("sf,nsyms", [(7, 600), (6, 1200)])
def test_long_frames(gpu, sf, nsyms):
    """a 255-byte packet is about 600 symbols at SF7: 77000 steps of the float32 recurrence through one accumulator. An error in the
    recurrence (a contracted multiply-add, a missing reduction, a different wrap) would GROW along the frame, so beside the
    criterion over the whole frame the last tenth of the frame must not differ in more components than the first tenth"""
    import lora_sdr_amd as L
    F = 66
    syms = np.random.default_rng(1000 + sf).integers(0, 1 << sf, (F, nsyms)).astype(np.uint16)
    ctx = L.Context(sf)
    got = frames(gpu, ctx, syms)
    want = md.mod_frames_def(sf, syms, 0x12, 1.0, 1)
    definition_equal(got, want, 1.0, "SF%d x %d symbols" % (sf, nsyms))
    body = got.shape[1] - (1 << sf)
    tenth = body // 10
    first, last = int(differing(got[:, :tenth], want[:, :tenth]).sum()), int(differing(got[:, body - tenth:body], want[:, body - tenth:body]).sum())
    print("SF%d x %d symbols: %d components differ in the first tenth, %d in the last" % (sf, nsyms, first, last))
    assert last <= first
    ctx.close()


_AMPL = {}


def ampl_case():
    if not _AMPL:
        syms = np.random.default_rng(77).integers(0, 128, (65, 4)).astype(np.uint16)
        ph, live = md.mod_phases_def(7, syms, 0x12)
        ph.setflags(write=False)
        _AMPL["case"] = (syms, ph, live)
    return _AMPL["case"]


@pytest.mark.parametrize("ampl", [3.0, -1.5, 0.0, 1e-40, 3e38, float("inf"), float("nan")])
def test_amplitudes(gpu, ampl):
    """amplitudes that are no power of two (2 ulps: see modulator_def.ulp_bound), negative, subnormal in float32 (1e-40: the
    products are subnormal or zero, and kept), next to the largest float (3e38: no product overflows, |cos| <= 1), and 0, +Inf, NaN,
    for which the definition's value is a class and a sign: (+-0, +-0), (+-Inf, +-Inf), NaN"""
    import lora_sdr_amd as L
    syms, ph, live = ampl_case()
    ctx = L.Context(7)
    got = frames(gpu, ctx, syms, ampl=ampl)
    N = 128
    assert got.shape == (65, md.mod_frame_len_def(7, 4, 1)) and not got[:, -N:].any()
    got = got[:, :-N]
    want = md.polar_def(ampl, ph, live)
    if ampl == 0 or not np.isfinite(ampl):
        a, b = f32(got), f32(want)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a == 0, b == 0)
        assert same_values(got, want)
        assert np.isnan(a).all() if np.isnan(ampl) else np.isinf(a).all() if np.isinf(ampl) else not a.any()
    else:
        definition_equal(got, want, ampl, "SF7 ampl %g" % ampl)
        if ampl == 1e-40:
            a = np.abs(f32(got))
            assert a.max() < 2.0 ** -126 and np.count_nonzero(a) > 0.99 * a.size, "subnormal products were flushed"
    ctx.close()


def test_padding_and_determinism(gpu):
    """padding 0 is padding 1 (the reference emits one zero symbol before it tests its counter); padding 5 is the same frame with
    four more zero symbols; a second launch gives the same bits"""
    import lora_sdr_amd as L
    sf, N = 8, 256
    syms = np.random.default_rng(8).integers(0, N, (65, 3)).astype(np.uint16)
    ctx = L.Context(sf)
    p0, p1, p5 = (frames(gpu, ctx, syms, sync=0x34, ampl=0.5, padding=p) for p in (0, 1, 5))
    assert bits_equal(p0, p1)
    assert p5.shape[1] == p1.shape[1] + 4 * N == md.mod_frame_len_def(sf, 3, 5)
    assert bits_equal(p5[:, :p1.shape[1]], p1) and not p5[:, -5 * N:].any() and p5[:, -5 * N - 1].all()
    assert bits_equal(frames(gpu, ctx, syms, sync=0x34, ampl=0.5, padding=1), p1)
    definition_equal(p5, md.mod_frames_def(sf, syms, 0x34, 0.5, 5), 0.5, "SF8 padding 5")
    ctx.close()


def test_refusals_leave_the_output_alone(gpu):
    import lora_sdr_amd as L
    torch = gpu
    lib = L.load()
    ctx = L.Context(7)
    F, S = 3, 2
    flen = md.mod_frame_len_def(7, S, 1)
    syms = np.zeros((F, S), np.uint16)
    buf = torch.full((F * flen,), SENTINEL, dtype=torch.complex64, device="cuda")
    d = dev_syms(torch, syms)
    ctx.use_torch_stream()
    out, sy = C.c_void_p(buf.data_ptr()), C.c_void_p(d.data_ptr())
    assert lib.lorahip_mod_frames(ctx._h, out, flen, sy, F, S, 0x12, 1.0, 1) == 0            # the call the refused ones are one step from
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    assert lib.lorahip_mod_frames(ctx._h, out, flen - 1, sy, F, S, 0x12, 1.0, 1) == E_INVALID
    assert lib.lorahip_mod_frames(ctx._h, out, 1 << 40, sy, F, S, 0x12, 1.0, 0x800000) == E_INVALID
    assert lib.lorahip_mod_frames(ctx._h, out, flen, sy, F, 0, 0x12, 1.0, 1) == E_INVALID
    # a count the symbol rows do not hold: refused on the count alone, before anything is read
    assert lib.lorahip_mod_frames(ctx._h, out, 1 << 40, sy, F, 0x800000, 0x12, 1.0, 1) == E_INVALID
    assert lib.lorahip_mod_frames(ctx._h, None, flen, sy, F, S, 0x12, 1.0, 1) == E_INVALID
    assert lib.lorahip_mod_frames(ctx._h, out, flen, None, F, S, 0x12, 1.0, 1) == E_INVALID
    assert lib.lorahip_mod_frames(None, out, flen, sy, F, S, 0x12, 1.0, 1) == E_INVALID
    assert lib.lorahip_mod_frames(ctx._h, None, flen, None, 0, S, 0x12, 1.0, 1) == 0          # nothing to do is not an error
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == np.complex64(SENTINEL)).all()
    assert lib.lorahip_mod_frame_len(5, 3, 1) == 0 and lib.lorahip_mod_frame_len(13, 3, 1) == 0
    for sf in range(6, 13):
        for nsyms, padding in [(1, 0), (2, 1), (17, 5)]:
            assert lib.lorahip_mod_frame_len(sf, nsyms, padding) == md.mod_frame_len_def(sf, nsyms, padding)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# per-frame counts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("sf", [6, 8, 12])
def test_per_frame_counts(gpu, sf, placement):
    """130 frames (two full wavefronts and two lanes of a third) of up to 9 symbols; the counts 0, 1, max, max + 1, -1 and -2 sit
    at the first lane, at both sides of the wavefront boundary and at the last frame, in two placements; symbol rows of a loose stride
    whose entries behind the row's count are 0xffff -- the definition is given the ORIGINAL symbols there, so a kernel that read
    them would differ; the output rows lie in a sentinel"""
    import lora_sdr_amd as L
    F, S, N = 130, 9, 1 << sf
    rng = np.random.default_rng(10 * sf + placement)
    syms = rng.integers(0, N, (F, S + 3)).astype(np.uint16)
    n = rng.integers(1, S + 1, F).astype(np.int32)
    n[[0, 63, 64, F - 1]] = [(0, 1, S + 1, -1), (S, -2, 0, S + 1)][placement]
    n[[1, 62, 65, F - 2]] = [(S, -2, S, 0), (-1, 1, S, 1)][placement]
    junk = syms.copy()
    for f in range(F):
        junk[f, max(0, min(int(n[f]), S)):] = 0xffff
    ctx = L.Context(sf)
    flen = md.mod_frame_len_def(sf, S, 2)
    rc, buf = raw_mod_frames(gpu, L, ctx, junk, 0x12, 1.0, 2, flen + 3, nsyms=n, sym_stride=S + 3, max_nsyms=S)
    assert rc == 0
    got, rest = split_rows(buf, F, flen + 3, flen)
    assert (rest == np.complex64(SENTINEL)).all(), "samples outside the rows were written"
    silent = (n < 0) | (n > S)
    assert silent.sum() >= 3 and not got[silent].any()
    want = md.mod_frames_def(sf, syms[:, :S], 0x12, 1.0, 2, nsyms=n)
    definition_equal(got, want, 1.0, "SF%d per-frame counts, placement %d" % (sf, placement))
    for f in np.flatnonzero(~silent):                       # behind a row's own symbols: zero chirps to the common length
        assert not got[f, 14 * N + N // 4 + int(n[f]) * N:].any() and got[f, 14 * N + N // 4 + int(n[f]) * N - 1] != 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the symbol generator
# ---------------------------------------------------------------------------------------------------------------------------
def synth(torch, ctx, sym, ampl):
    iq = ctx.synth_symbols(dev_syms(torch, sym), ampl=ampl)
    torch.cuda.synchronize()
    return iq.cpu().numpy().reshape(len(sym), ctx.N)


@pytest.mark.parametrize("ampl", [0.75, 3.0])
@pytest.mark.parametrize("sf", [6, 7, 8, 9, 10, 11, 12])
def test_synth_symbols(gpu, sf, ampl):
    """the generator of every benchmark's input against its closed form; a symbol >= N gives the window of its low sf bits, bit for
    bit (the generator MASKS, the modulator does not); no windows is no work"""
    import lora_sdr_amd as L
    torch = gpu
    N = 1 << sf
    rng = np.random.default_rng(sf)
    sym = np.concatenate([[0, 1, N // 2, N - 1], rng.integers(0, N, 60), [N, N + 5, 65535]]).astype(np.uint16)
    ctx = L.Context(sf)
    got = synth(torch, ctx, sym, ampl)
    definition_equal(got, md.synth_symbols_def(sf, sym, ampl), ampl, "synth SF%d ampl %g" % (sf, ampl))
    assert bits_equal(got[-3:], synth(torch, ctx, sym[-3:] & (N - 1), ampl))
    assert bits_equal(got[-3], got[0])                      # N -> symbol 0's window
    assert L.load().lorahip_synth_symbols(ctx._h, None, None, 0, ampl, 0.0, 0) == 0
    assert ctx.synth_symbols(dev_syms(torch, sym[:0]), ampl=ampl).numel() == 0
    ctx.close()


def test_synth_symbols_second_pass_of_the_grid_stride_loop(gpu):
    """2048 workgroups of 256 threads cover 524288 elements a pass: 8193 windows of 64 samples reach 64 elements into the second.
    Every window is compared; the first, the last and the two at element 524288 are named"""
    import lora_sdr_amd as L
    sf, W = 6, 8193
    assert (W - 1) * 64 == 2048 * 256
    sym = np.random.default_rng(61).integers(0, 64, W).astype(np.uint16)
    ctx = L.Context(sf)
    got = synth(gpu, ctx, sym, 0.75)
    want = md.synth_symbols_def(sf, sym, 0.75)
    definition_equal(got, want, 0.75, "synth SF6 x %d windows" % W)
    for w in (0, W - 2, W - 1):
        assert md.ulp_distance(f32(got[w]), f32(want[w])).max() <= 2 and got[w].all(), w
    assert not bits_equal(got[W - 1], got[W - 2])
    ctx.close()
