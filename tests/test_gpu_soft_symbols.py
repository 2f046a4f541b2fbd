"""GPU: lorahip_soft_symbols against its definition (include/lorahip.h; tests/soft_def.py). Window s of run p is the window
lorahip_detect_batch evaluates at first_sample[p] + s*N with the up-chirp table, the run's fine_err and the fine-tune index the previous
window left; its bins are that call's fft_out, its hard symbol that call's sym, and the LLRs are llr_def of those bins -- bit for bit.

One small case per kernel family member: SF7, 8, 10 (a run per lane group of a wavefront: 8, 4 and 1 runs per wavefront) and SF11, 12
(a run per workgroup). Five runs of 1, 2, 3, 9 and 0 windows at starts that are no multiple of N (nor of two samples), in noise that
leaves some windows wrong; fine_err 0 / +0.31 / -0.27 and fine_idx0 0 / 77 / 128 N - 1; ppm = sf and sf - 2."""
import ctypes as C
import math

import numpy as np
import pytest

import soft_def as S

pytestmark = pytest.mark.gpu

LENS = [1, 2, 3, 9, 0]
ERRS = [0.0, 0.31, -0.27, 0.31, -0.27]
STRIDE = 10                                              # one entry more than the longest run: it must stay as it was
LLR_FILL, SYM_FILL = 12345.0, 0x5A5A
LEAD = 37


def _case(torch, sf):
    """-> (ctx, iq, first (5,), nsyms, idx0, err, sent symbols per run, reference bins / syms per (run, window))"""
    import lora_sdr_amd as L
    N = 1 << sf
    ctx = L.Context(sf)
    rng = np.random.default_rng(sf)
    total = sum(LENS)
    sent = rng.integers(0, N, total).astype(np.uint16)
    clean = ctx.synth_symbols(torch.from_numpy(sent.view(np.int16)).cuda(), ampl=1.0)
    iq = torch.zeros(LEAD + clean.numel() + N, dtype=torch.complex64, device="cuda")
    iq[LEAD:LEAD + clean.numel()] = clean
    # a bin of pure noise is Rayleigh with scale sigma sqrt(N) (sigma per component); the largest of N of them reaches the peak N at
    # about sigma = sqrt(N / (2 ln N)), and the peak itself moves by sigma sqrt(N): a little below that sigma a good part of the windows
    # decide wrong and a good part right
    ctx.add_awgn(iq, 0.9 * math.sqrt(N / (2 * math.log(N))), seed=1000 + sf)
    first = LEAD + N * np.concatenate([[0], np.cumsum(LENS)[:-1]]).astype(np.int64)
    idx0 = np.array([77, 128 * N - 1, 0, 77, 0], np.int32)
    err = np.array(ERRS, np.float32)
    # the reference: call s covers window s of every run that has one
    cur = idx0.copy()
    bins, syms = {}, {}
    for s in range(max(LENS)):
        runs = [p for p in range(len(LENS)) if LENS[p] > s]
        o = ctx.detect_batch(iq, offsets=torch.from_numpy(first[runs] + s * N).cuda(), chirp_sel_all=L.CHIRP_UP,
                             fine_idx0=torch.from_numpy(cur[runs]).cuda(), fine_err=torch.from_numpy(err[runs]).cuda(),
                             want_fft=True, want_fine_idx=True)
        fft, sym, nxt = o["fft"].cpu().numpy(), o["sym"].cpu().numpy().view(np.uint16), o["fineIdxOut"].cpu().numpy()
        for j, p in enumerate(runs):
            bins[p, s], syms[p, s] = fft[j], sym[j]
            cur[p] = nxt[j]
    return ctx, iq, first, idx0, err, sent, bins, syms


@pytest.fixture(scope="module", params=[7, 8, 10, 11, 12])
def case(request, gpu):
    c = _case(gpu, request.param)
    yield (request.param,) + c
    c[0].close()


def _run(torch, ctx, iq, first, nsyms, idx0, err, ppm, stride=STRIDE):
    W = ppm or ctx.sf
    P = len(nsyms)
    llr = torch.full((P, stride, W), LLR_FILL, dtype=torch.float32, device="cuda")
    sym = torch.full((P, stride), SYM_FILL, dtype=torch.int16, device="cuda")
    ctx.soft_symbols(iq, torch.from_numpy(np.asarray(first, np.int64)).cuda(), torch.from_numpy(np.asarray(nsyms, np.int32)).cuda(),
                     fine_idx0=None if idx0 is None else torch.from_numpy(idx0).cuda(), fine_err=None if err is None else torch.from_numpy(err).cuda(),
                     ppm=ppm, sym_stride=stride, hard=True, out=(llr, sym))
    return llr.cpu().numpy(), sym.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("less", [0, 2])
def test_llrs_and_hard_symbols_equal_the_definition(case, gpu, less):
    sf, ctx, iq, first, idx0, err, sent, bins, syms = case
    ppm = sf - less
    llr, sym = _run(gpu, ctx, iq, first, LENS, idx0, err, ppm if less else 0)
    checked = 0
    at = np.concatenate([[0], np.cumsum(LENS)])
    for p, n in enumerate(LENS):
        for s in range(n):
            want = S.llr_def(bins[p, s][None, :], sf, ppm)[0]
            assert np.array_equal(llr[p, s].view(np.uint32), want.view(np.uint32)), (sf, ppm, p, s, llr[p, s], want)
            assert sym[p, s] == syms[p, s], (sf, p, s)
            # the invariant: the signs spell the Gray code of the hard symbol (a tie between the two maxima of a bit would excuse a window)
            assert np.all(llr[p, s] != 0), (sf, ppm, p, s, "an exact tie: choose another seed")
            g = int(S.gray_map(sf, ppm)[sym[p, s]])
            assert [int(v > 0) for v in llr[p, s]] == [(g >> m) & 1 for m in range(ppm)], (sf, ppm, p, s)
            checked += 1
        assert np.all(llr[p, n:] == np.float32(LLR_FILL)) and np.all(sym[p, n:] == SYM_FILL), (sf, p, "written behind the run")
    assert checked == sum(LENS)
    # the noise does its work: some windows are decided wrong, not all
    # (the generator's symbol s peaks in bin s + 1)
    all_wrong = sum(int((int(syms[p, s]) - int(sent[at[p] + s])) % (1 << sf) != 1) for p, n in enumerate(LENS) for s in range(n))
    assert 0 < all_wrong < checked, (sf, all_wrong)


def test_rows_shorter_than_the_run_and_no_fine_state(case, gpu):
    sf, ctx, iq, first, idx0, err, sent, bins, syms = case
    # windows s >= sym_stride are not evaluated
    llr, sym = _run(gpu, ctx, iq, first, LENS, idx0, err, 0, stride=4)
    for p, n in enumerate(LENS):
        for s in range(min(n, 4)):
            assert np.array_equal(llr[p, s].view(np.uint32), S.llr_def(bins[p, s][None, :], sf, sf)[0].view(np.uint32)) and sym[p, s] == syms[p, s]
        assert np.all(llr[p, min(n, 4):] == np.float32(LLR_FILL))
    # null fine_idx0 / fine_err are zeros; negative counts are empty runs
    import lora_sdr_amd as L
    N = 1 << sf
    a, b = _run(gpu, ctx, iq, first, [2, -3, 1, 0, 0], None, None, 0)
    o = ctx.detect_batch(iq, offsets=gpu.from_numpy(np.array([first[0], first[0] + N, first[2]], np.int64)).cuda(), chirp_sel_all=L.CHIRP_UP, want_fft=True)
    want = S.llr_def(o["fft"].cpu().numpy(), sf, sf)
    assert np.array_equal(np.stack([a[0, 0], a[0, 1], a[2, 0]]).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.array([b[0, 0], b[0, 1], b[2, 0]]), o["sym"].cpu().numpy().view(np.uint16))
    assert np.all(a[1] == np.float32(LLR_FILL)) and np.all(a[3:] == np.float32(LLR_FILL)) and np.all(b[1] == SYM_FILL)


def test_a_fine_index_outside_the_table_is_no_fault(case, gpu):
    sf, ctx, iq, first, idx0, err, sent, bins, syms = case
    bad = np.array([-5, 128 * (1 << sf), 2 ** 31 - 1, -2 ** 31, 77], np.int32)
    llr, sym = _run(gpu, ctx, iq, first, LENS, bad, err, 0)
    assert np.all(np.isfinite(llr[3, :9])) and np.all(llr[4] == np.float32(LLR_FILL))


def test_arguments(gpu):
    import lora_sdr_amd as L
    torch = gpu
    with L.Context(7) as ctx:
        lib, h = ctx._lib, ctx._h
        E = -1                                           # LORAHIP_E_INVALID
        iq = torch.zeros(4 * 128, dtype=torch.complex64, device="cuda")
        first = torch.zeros(2, dtype=torch.int64, device="cuda")
        n = torch.ones(2, dtype=torch.int32, device="cuda")
        llr = torch.zeros((2, 3, 7), dtype=torch.float32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        ctx.use_torch_stream()
        call = lib.lorahip_soft_symbols
        assert call(h, None, None, None, None, None, 0, 0, None, 3, None) == 0                      # no packets: no work
        assert call(h, p(iq), p(first), p(n), None, None, 2, 0, p(llr), 3, None) == 0
        for args in ((None, p(first), p(n), p(llr)), (p(iq), None, p(n), p(llr)), (p(iq), p(first), None, p(llr)), (p(iq), p(first), p(n), None)):
            assert call(h, args[0], args[1], args[2], None, None, 2, 0, args[3], 3, None) == E
        for ppm in (-1, 8):
            assert call(h, p(iq), p(first), p(n), None, None, 2, ppm, p(llr), 3, None) == E
            assert call(h, None, None, None, None, None, 0, ppm, None, 3, None) == E
        for stride in (0, lib.lorahip_decode_max_symbols() + 1):
            assert call(h, p(iq), p(first), p(n), None, None, 2, 0, p(llr), stride, None) == E
        assert call(h, p(iq), p(first), p(n), None, None, 0x80000000, 0, p(llr), 3, None) == E
        assert call(None, p(iq), p(first), p(n), None, None, 2, 0, p(llr), 3, None) == E
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            ctx.soft_symbols(iq, first, n)               # sym_stride is the caller's to give
