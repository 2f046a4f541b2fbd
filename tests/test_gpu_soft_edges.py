"""GPU: lorahip_soft_symbols at the inputs and launch shapes tests/test_gpu_soft_symbols.py leaves out -- every kernel instance (SF6 to
SF12), the exact index chain beside the closed form in one wavefront, edge windows (all-zero, NaN, infinite, denormal and overflowing
|X|^2), a maximum owned by every lane, register slot and wavefront, and the four-wavefront workgroup with a partly filled tail.

The reference is the definition's own construction (include/lorahip.h): window s of run p IS the lorahip_detect_batch window at
first_sample[p] + s*N with the up-chirp table, the run's fine_err and the fine-tune index window s - 1 left. So for step s there is one
ctx.detect_batch call over the runs that have a window s, the index carried forward from its fineIdxOut; the expected LLRs are
soft_def.llr_def of that call's fft, the expected hard symbols that call's sym (tests/test_gpu_detect_instances.py ties those windows
to the CPU oracle). Every comparison is bit for bit; where the expected LLR is NaN (Inf - Inf) the result must be NaN, of any bit
pattern. Outputs are pre-filled, sym_stride is one above the longest run: whatever lies behind a run's windows, and every row of an empty
run, must still hold the fill. The sanity of the inputs is asserted on the reference or on host-only calls, before a result is looked at.

A1, fine-state classes: eight runs, one per class (CLASSES), so that chain windows, closed-form windows, still and finished lane groups
    share a wavefront at SF6 / SF7. The issue's lengths 3, 1, 4, 2, 5, 0, 4, 3 leave the `irr+` run empty, and so without a window to
    take the chain in; the test therefore sends a second arrangement as well, the same lengths in reverse order (there `reg-` is the
    empty run and `irr+` has four windows). The reference is five windows deep for every class and serves both.
A2, edge windows: the 15 "scan" inputs of detect_edge_inputs.inputs(sf), each one run of 67 windows, plus a 16th run. With the 3e-39
    input every |X|^2 underflows to exactly zero (its LLRs are all +0.0, which is asserted), and no amplitude of the existing list
    leaves a non-zero LLR below 2^-126 at SF8 and above: an LLR is at least the peak less the runner-up, and the peak of the 1e-21
    input is N^2 * 1e-42, normal from SF8 on. The 16th run is the same chirp + AWGN windows at amplitude 2^-64 / N, whose peak |X|^2 is
    about 2^-128 at every SF; the denormal-LLR condition is asserted on it (and, where it holds, noted for the 1e-21 run).
A3, owners of the maximum: clean chirps with AWGN of sigma 0.05 per component; every bin (SF6 to SF10), or every wavefront and register
    slot (SF11 / SF12), owns the peak of a window.
A4, launch shapes (SF6 to SF10): the smallest run count the tiling query (lorahip_soft_plan) reports four wavefronts per workgroup for,
    plus runs_per_wavefront + 1 runs -- a last workgroup of one full wavefront, one wavefront with a single run and two with none --
    and 3 * runs_per_wavefront + 1 runs, which are four one-wavefront workgroups, the last with one run."""
import ctypes as C

import numpy as np
import pytest

import soft_def as S

pytestmark = pytest.mark.gpu

SFS = [6, 7, 8, 9, 10, 11, 12]
FAST_SFS = [6, 7, 8, 9, 10]
LLR_FILL, SYM_FILL = 12345.0, 0x5A5A
LEAD = 37                                                # odd, and no multiple of N

CLASSES = ("still", "reg+", "reg-", "int+", "sat", "irr+", "irr-", "hitM")
CHAIN = ("irr+", "irr-", "hitM")                          # must reach the exact index chain (path 0) in a window
CLOSED = ("reg+", "reg-", "int+", "sat")                  # the closed form (path 1) in every window
A1_LENS = (3, 1, 4, 2, 5, 0, 4, 3)
A1_DEPTH = 5


def class_state(sf):
    """-> fine_idx0 (8,) int32, fine_err (8,) float32 in the order of CLASSES. d = fine_err * 128:
    still 0; reg+ 39.68 (closed form mod M + 1); reg- -34.56 (mod M); int+ 40 exactly (mod M with d > 0); sat 0.51 (the index walks
    down from N + 5, reaches 0 inside the second window and stays); irr+ 40 + 2^-12 and irr- -(40 - 2^-12) (the fraction is within
    M 2^-25 of an integer: no closed form at any SF); hitM 39.68 from 239, which lands on ceil(d) - 1 = 39 after five steps."""
    N = 1 << sf
    err = np.array([0.0, 0.31, -0.27, 0.3125, 0.51 / 128, (40 + 2.0 ** -12) / 128, -(40 - 2.0 ** -12) / 128, 0.31], np.float32)
    idx0 = np.array([77, 77, 128 * N - 1, 5, N + 5, 1000, 1000, 239], np.int32)
    return idx0, err


# ---- the reference and the comparison -----------------------------------------------------------------------------------------------
def reference(detect, N, first, lens, idx0, err):
    """-> [(runs, fft (R, N) complex64, sym (R,) uint16, idx_before (R,) int32 or None, idx_after (R,) int32)] per step s: the windows s
    of the runs that have one. detect(offsets, fine_idx0 or None, fine_err or None) -> (fft, sym, fineIdxOut), numpy."""
    first, lens = np.asarray(first, np.int64), np.asarray(lens, np.int64)
    cur = None if idx0 is None else np.array(idx0, np.int32)
    steps = []
    for s in range(int(lens.max())):
        runs = np.flatnonzero(lens > s)
        fft, sym, nxt = detect(first[runs] + s * N, None if cur is None else cur[runs], None if err is None else np.asarray(err, np.float32)[runs])
        steps.append((runs, fft, sym, None if cur is None else cur[runs].copy(), nxt))
        if cur is not None:
            cur[runs] = nxt
    return steps


def gpu_detect(torch, ctx, iq):
    import lora_sdr_amd as L

    def detect(offsets, idx, err):
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        o = ctx.detect_batch(iq, offsets=dev(offsets), chirp_sel_all=L.CHIRP_UP, fine_idx0=dev(idx), fine_err=dev(err), want_fft=True, want_fine_idx=True)
        return o["fft"].cpu().numpy(), o["sym"].cpu().numpy().view(np.uint16), o["fineIdxOut"].cpu().numpy()
    return detect


def expected(steps, lens, stride, sf, ppm):
    """-> llr (P, stride, ppm) float32, sym (P, stride) uint16: the definition's values in the windows s < lens[p], the fill elsewhere.
    `steps` may be deeper than lens."""
    lens = np.asarray(lens, np.int64)
    assert lens.max() < stride
    llr = np.full((len(lens), stride, ppm), LLR_FILL, np.float32)
    sym = np.full((len(lens), stride), SYM_FILL, np.uint16)
    for s, (runs, fft, hard, _, _) in enumerate(steps):
        keep = lens[runs] > s
        if keep.any():
            llr[runs[keep], s] = S.llr_def(fft[keep], sf, ppm)
            sym[runs[keep], s] = hard[keep]
    return llr, sym


def run(torch, ctx, iq, first, lens, idx0, err, ppm, stride, hard=True):
    """lorahip_soft_symbols into pre-filled rows -> llr (P, stride, ppm), sym (P, stride) uint16 or None"""
    P = len(lens)
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    llr = torch.full((P, stride, ppm), LLR_FILL, dtype=torch.float32, device="cuda")
    sym = torch.full((P, stride), SYM_FILL, dtype=torch.int16, device="cuda") if hard else None
    ctx.soft_symbols(iq, dev(first, np.int64), dev(lens, np.int32), fine_idx0=dev(idx0, np.int32), fine_err=dev(err, np.float32),
                     ppm=ppm, sym_stride=stride, hard=hard, out=(llr, sym) if hard else llr)
    return llr.cpu().numpy(), sym.cpu().numpy().view(np.uint16) if hard else None


def compare(got, want, tag):
    """LLRs bit for bit where the expected value is not NaN, NaN where it is; sym equal; the fill behind the runs is part of `want`"""
    (llr, sym), (wllr, wsym) = got, want
    assert llr.shape == wllr.shape and llr.dtype == np.float32
    nan = np.isnan(wllr)
    bad = np.where(nan, ~np.isnan(llr), llr.view(np.uint32) != wllr.view(np.uint32))
    if bad.any():
        p, s, m = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((tag, "llr of run %d window %d bit %d" % (p, s, m), llr[p, s], wllr[p, s], "%d entries differ" % bad.sum()))
    if sym is not None:
        bad = sym != wsym
        if bad.any():
            p, s = (int(v) for v in np.argwhere(bad)[0])
            raise AssertionError((tag, "sym of run %d window %d" % (p, s), int(sym[p, s]), int(wsym[p, s]), "%d entries differ" % bad.sum()))


def noisy_chirps(torch, ctx, syms, sigma, seed, lead=LEAD):
    """LEAD zeros, the up-chirps of `syms` back to back, a window of zeros; AWGN of `sigma` per component over all of it"""
    clean = ctx.synth_symbols(torch.from_numpy(np.asarray(syms, np.uint16).view(np.int16)).cuda(), ampl=1.0)
    iq = torch.zeros(lead + clean.numel() + ctx.N, dtype=torch.complex64, device="cuda")
    iq[lead:lead + clean.numel()] = clean
    ctx.add_awgn(iq, sigma, seed=seed)
    return iq


_CASES = {}


def cached(torch, key, build):
    """one context, one stream and one reference per (part, sf), shared by that part's ppm cases and left unchanged"""
    if key not in _CASES:
        _CASES[key] = build(torch, key[1])
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for case in _CASES.values():
        case["ctx"].close()
    _CASES.clear()


# ---- A1: the fine-state classes in one wavefront -------------------------------------------------------------------------------------
def a1_paths(lib, sf, steps):
    """path[p][s] of lorahip_fine_indices_host (host only) on the carried index: 1 the closed form, 0 the exact chain; its end index
    must be the one the reference window left"""
    N = 1 << sf
    _, err = class_state(sf)
    paths = np.full((len(CLASSES), len(steps)), -1, np.int64)
    scratch = np.empty(N, np.int32)
    for s, (runs, _, _, before, after) in enumerate(steps):
        for j, p in enumerate(runs):
            end, path = C.c_int32(), C.c_int32()
            assert lib.lorahip_fine_indices_host(sf, int(before[j]), float(err[p]), scratch.ctypes.data, C.byref(end), C.byref(path)) == 0
            assert end.value == int(after[j]), (sf, CLASSES[p], s, end.value, int(after[j]))
            paths[p, s] = path.value
    return paths


def check_a1_paths(paths, lens):
    """what an arrangement of lengths sends: a chain window in every chain class it has a window of, the closed form everywhere else"""
    for p, name in enumerate(CLASSES):
        mine = paths[p, :lens[p]]
        assert np.all(mine >= 0)
        if name in CHAIN and lens[p]:
            assert (mine == 0).any(), (name, "never takes the exact chain", mine)
        if name in CLOSED or name == "still":
            assert np.all(mine == 1), (name, "leaves the closed form", mine)


A1_ARRANGEMENTS = (A1_LENS, A1_LENS[::-1])


def build_a1(torch, sf):
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    N = 1 << sf
    rng = np.random.default_rng(100 + sf)
    iq = noisy_chirps(torch, ctx, rng.integers(0, N, len(CLASSES) * A1_DEPTH), 0.3, 2000 + sf)
    first = LEAD + N * A1_DEPTH * np.arange(len(CLASSES), dtype=np.int64)
    idx0, err = class_state(sf)
    steps = reference(gpu_detect(torch, ctx, iq), N, first, [A1_DEPTH] * len(CLASSES), idx0, err)
    assert first[0] % 2 == 1 and first[0] % N != 0
    paths = a1_paths(ctx._lib, sf, steps)
    for lens in A1_ARRANGEMENTS:
        check_a1_paths(paths, lens)
    for name in CLASSES:                                  # every class has a window in one arrangement at least
        assert any(lens[CLASSES.index(name)] for lens in A1_ARRANGEMENTS), name
    sat = CLASSES.index("sat")
    assert steps[0][4][sat] == 5 and steps[1][4][sat] == 0 and steps[2][4][sat] == 0       # down to 0 inside the second window, and held
    return dict(ctx=ctx, iq=iq, first=first, idx0=idx0, err=err, steps=steps)


def a1_ppms(sf):
    return list(range(1, 8)) if sf == 7 else sorted({sf, sf - 2, 1})


@pytest.mark.parametrize("sf,ppm", [(sf, ppm) for sf in SFS for ppm in a1_ppms(sf)])
def test_fine_state_classes_share_a_wavefront(gpu, sf, ppm):
    c = cached(gpu, ("a1", sf), build_a1)
    for lens in A1_ARRANGEMENTS:
        want = expected(c["steps"], lens, A1_DEPTH + 1, sf, ppm)
        got = run(gpu, c["ctx"], c["iq"], c["first"], lens, c["idx0"], c["err"], ppm, A1_DEPTH + 1)
        compare(got, want, ("a1", sf, ppm, lens))


@pytest.mark.parametrize("sf", SFS)
def test_without_hard_symbols_the_llrs_are_the_same(gpu, sf):
    c = cached(gpu, ("a1", sf), build_a1)
    for lens in A1_ARRANGEMENTS:
        with_sym, _ = run(gpu, c["ctx"], c["iq"], c["first"], lens, c["idx0"], c["err"], sf, A1_DEPTH + 1)
        without, none = run(gpu, c["ctx"], c["iq"], c["first"], lens, c["idx0"], c["err"], sf, A1_DEPTH + 1, hard=False)
        assert none is None
        assert np.array_equal(without.view(np.uint32), with_sym.view(np.uint32)), (sf, lens)
        compare((without, None), expected(c["steps"], lens, A1_DEPTH + 1, sf, sf), ("a1 no sym", sf, lens))


# ---- A2: edge windows ----------------------------------------------------------------------------------------------------------------
A2_W = 67
TINY = "amplitude 2^-64 / N"


def a2_inputs(sf):
    """[(name, iq (67, N) complex64)]: the 15 scan inputs and the tiny-amplitude run (the chirp + AWGN windows of the amplitude inputs,
    recovered from the 1e18 one, whose scaling is exact enough: only the size matters)"""
    import detect_edge_inputs as E
    ins = [(i.name, i.iq) for i in E.inputs(sf) if i.kind == "scan"]
    assert len(ins) == 15 and all(iq.shape == (A2_W, 1 << sf) for _, iq in ins)
    base = dict(ins)["amplitude 1e+18"].astype(np.complex128) * 1e-18
    tiny = (base * (2.0 ** -64 / (1 << sf))).astype(np.complex64)
    keep = np.arange(A2_W) % 8 == 0
    tiny[keep] = dict(ins)["all-zero"][keep]                                             # the ordinary windows, as every input has them
    return ins + [(TINY, tiny)]


def check_a2_reference(sf, names, steps):
    """the inputs are the edges they are meant to be, judged on the reference's bins alone"""
    fft = np.stack([f for _, f, _, _, _ in steps], axis=1)                               # (runs, W, N): every run has all 67 windows
    sym = np.stack([h for _, _, h, _, _ in steps], axis=1)
    at = dict((n, i) for i, n in enumerate(names))
    llr = lambda name: S.llr_def(fft[at[name]], sf, sf)
    odd = np.arange(A2_W) % 8 != 0
    z = at["all-zero"]
    assert np.all(llr("all-zero")[odd].view(np.uint32) == 0) and np.all(sym[z, odd] == 0)
    for name in ("NaN sample", "infinite sample"):
        finite = np.isfinite(fft[at[name]].view(np.float32)).all(axis=1)
        assert (~finite).any() and finite.any(), name
    big = llr("amplitude 3e+37")
    assert (np.isposinf(big) | np.isnan(big)).any()
    small = llr("amplitude 3e-39")                                                       # bins of about N * 3e-39: every |X|^2 underflows to zero
    assert np.all(np.any(fft[at["amplitude 3e-39"]][odd] != 0, axis=1)) and np.all(small[odd].view(np.uint32) == 0)
    tiny = np.abs(llr(TINY)[odd])
    assert ((tiny > 0) & (tiny < 2.0 ** -126)).any(), "no denormal LLR"
    P = S.power_def(fft[at[TINY]][odd])
    assert ((P > 0) & (P < 2.0 ** -126)).mean() > 0.9                                    # |X|^2 in the denormal range, not zero


def build_a2(torch, sf):
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    N = 1 << sf
    ins = a2_inputs(sf)
    P = len(ins)
    host = np.concatenate([iq.reshape(-1) for _, iq in ins] + [np.zeros(N, np.complex64)])
    iq = torch.from_numpy(host).cuda()
    first = A2_W * N * np.arange(P, dtype=np.int64)
    err = np.where(np.arange(P) % 2 == 0, 0.0, 0.31).astype(np.float32)
    idx0 = np.random.default_rng(300 + sf).integers(0, 128 * N, P).astype(np.int32)
    steps = reference(gpu_detect(torch, ctx, iq), N, first, [A2_W] * P, idx0, err)
    check_a2_reference(sf, [n for n, _ in ins], steps)
    return dict(ctx=ctx, iq=iq, first=first, idx0=idx0, err=err, steps=steps, lens=[A2_W] * P)


@pytest.mark.parametrize("sf,less", [(sf, less) for sf in SFS for less in (0, 2)])
def test_edge_windows(gpu, sf, less):
    c = cached(gpu, ("a2", sf), build_a2)
    ppm = sf - less
    want = expected(c["steps"], c["lens"], A2_W + 1, sf, ppm)
    got = run(gpu, c["ctx"], c["iq"], c["first"], c["lens"], c["idx0"], c["err"], ppm, A2_W + 1)
    compare(got, want, ("a2", sf, ppm))


# ---- A3: every lane, register slot and wavefront owns a maximum ----------------------------------------------------------------------
A3_SIGMA = 0.05


def a3_bins(sf):
    """the bins the peaks are sent to, in sending order: all N (SF6 to SF10), or the 32 lowest, the 32 highest and 192 drawn"""
    N = 1 << sf
    rng = np.random.default_rng(400 + sf)
    if sf <= 10:
        return rng.permutation(N)
    bins = np.concatenate([np.arange(32), np.arange(N - 32, N), 32 + rng.choice(N - 64, 192, replace=False)])
    return rng.permutation(bins)


def build_a3(torch, sf):
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    N = 1 << sf
    bins = a3_bins(sf)
    per = len(bins) // 8
    iq = noisy_chirps(torch, ctx, (bins - 1) % N, A3_SIGMA, 4000 + sf)                   # (the generator's symbol s peaks in bin s + 1)
    first = LEAD + N * per * np.arange(8, dtype=np.int64)
    steps = reference(gpu_detect(torch, ctx, iq), N, first, [per] * 8, None, None)
    sym = np.stack([h for _, _, h, _, _ in steps], axis=1).reshape(-1).astype(np.int64)  # run-major: the sending order
    assert np.array_equal(sym, bins), (sf, "a peak is not where it was sent")
    if sf <= 10:
        assert np.array_equal(np.sort(sym), np.arange(N))                                # every bin owns the peak once
    else:
        T, log2t = N // 16, sf - 4
        assert set((sym % T) >> 6) == set(range(T // 64)) and set(sym >> log2t) == set(range(16))
    half = 2                                                                             # ppm = sf - 2: (1 << 2) / 2
    assert (sym >= N - half).any() and (sym % 4 == 1).any() and (sym % 4 == 2).any()
    return dict(ctx=ctx, iq=iq, first=first, steps=steps, lens=[per] * 8)


@pytest.mark.parametrize("sf,less", [(sf, less) for sf in SFS for less in (0, 2)])
def test_every_lane_slot_and_wavefront_owns_a_maximum(gpu, sf, less):
    c = cached(gpu, ("a3", sf), build_a3)
    ppm = sf - less
    stride = c["lens"][0] + 1
    want = expected(c["steps"], c["lens"], stride, sf, ppm)
    got = run(gpu, c["ctx"], c["iq"], c["first"], c["lens"], None, None, ppm, stride)
    compare(got, want, ("a3", sf, ppm))
    # clean peaks: the signs of the LLRs spell the Gray code of the bin
    g = S.gray_map(sf, ppm)[want[1][:, :stride - 1].astype(np.int64)]
    assert np.array_equal(got[0][:, :stride - 1] > 0, ((g[..., None] >> np.arange(ppm, dtype=np.uint32)) & 1).astype(bool))


# ---- A4: launch shapes ---------------------------------------------------------------------------------------------------------------
def a4_runs(sf, n):
    N = 1 << sf
    p = np.arange(n)
    idx0, err = class_state(sf)
    return LEAD + (p % 61) * 3, np.array([1, 2, 0])[p % 3], idx0[p % 8], err[p % 8]


def build_a4(torch, sf):
    import lora_sdr_amd as L
    ctx = L.Context(sf)
    N = 1 << sf
    wpw = ctx.soft_plan(1)["runs_per_wavefront"]
    assert wpw == 64 >> (sf - 4)
    n4 = 4 * wpw
    while n4 <= 2 ** 17 and ctx.soft_plan(n4)["waves_per_workgroup"] != 4:
        n4 *= 2
    assert n4 <= 2 ** 17, "the launch rule changed: resize this test"
    n = -(-n4 // (4 * wpw)) * 4 * wpw + wpw + 1
    iq = torch.zeros(LEAD + 60 * 3 + 3 * N, dtype=torch.complex64, device="cuda")
    ctx.add_awgn(iq, 1.0, seed=5000 + sf)
    first, lens, idx0, err = a4_runs(sf, n)
    assert int(first.max()) + 2 * N <= iq.numel()
    steps = reference(gpu_detect(torch, ctx, iq), N, first, lens, idx0, err)
    assert len(steps) == 2
    return dict(ctx=ctx, iq=iq, n=n, n4=n4, wpw=wpw, steps=steps)


@pytest.mark.parametrize("sf", FAST_SFS)
def test_four_wavefront_workgroups_with_a_partly_filled_tail(gpu, sf):
    c = cached(gpu, ("a4", sf), build_a4)
    ctx, n, wpw = c["ctx"], c["n"], c["wpw"]
    plan = ctx.soft_plan(n)
    assert plan == dict(runs_per_wavefront=wpw, waves_per_workgroup=4, workgroups=(n - wpw - 1) // (4 * wpw) + 1), plan
    first, lens, idx0, err = a4_runs(sf, n)
    want = expected(c["steps"], lens, 3, sf, sf)
    got = run(gpu, ctx, c["iq"], first, lens, idx0, err, sf, 3)
    compare(got, want, ("a4", sf, n))


@pytest.mark.parametrize("sf", FAST_SFS)
def test_one_wavefront_workgroups_with_a_partly_filled_tail(gpu, sf):
    c = cached(gpu, ("a4", sf), build_a4)
    ctx, wpw = c["ctx"], c["wpw"]
    n = 3 * wpw + 1
    assert ctx.soft_plan(n) == dict(runs_per_wavefront=wpw, waves_per_workgroup=1, workgroups=4)
    first, lens, idx0, err = a4_runs(sf, n)
    want = expected([(r[r < n], f[r < n], h[r < n], None, None) for r, f, h, _, _ in c["steps"]], lens, 3, sf, sf)
    got = run(gpu, ctx, c["iq"], first, lens, idx0, err, sf, 3)
    compare(got, want, ("a4 small", sf, n))


def test_soft_plan_wide_and_refusals(gpu):
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    for sf, waves in ((11, 2), (12, 4)):
        with L.Context(sf) as ctx:
            for n in (0, 1, 5, 100000, 0x7fffffff):
                assert ctx.soft_plan(n) == dict(runs_per_wavefront=0, waves_per_workgroup=waves, workgroups=n)
    with L.Context(7) as ctx:
        assert ctx.soft_plan(0) == dict(runs_per_wavefront=8, waves_per_workgroup=1, workgroups=0)
        assert ctx.soft_plan(9) == dict(runs_per_wavefront=8, waves_per_workgroup=1, workgroups=2)
        assert ctx.soft_plan(0x7fffffff) == dict(runs_per_wavefront=8, waves_per_workgroup=4, workgroups=2 ** 26)
        lib, h = ctx._lib, ctx._h
        t = _lib.SoftTiling(C.sizeof(_lib.SoftTiling))
        assert lib.lorahip_soft_plan(h, 0x80000000, C.byref(t)) == -1 and t.waves_per_workgroup == 0 and t.struct_size == C.sizeof(_lib.SoftTiling)
        assert lib.lorahip_soft_plan(None, 1, C.byref(t)) == -1
        assert lib.lorahip_soft_plan(h, 1, None) == -1
        t = _lib.SoftTiling(C.sizeof(_lib.SoftTiling) - 8)
        assert lib.lorahip_soft_plan(h, 1, C.byref(t)) == -1
