"""CPU: the resampler's tiling (lorahip_resampler_plan, host only) held to what include/lorahip.h and the comment above resampPlan in
lorahip_resamp.hip state about it, over every down 1..1024 against a few dozen up and the reverse, filters of T = ceil(n_taps / up) =
1, 64 and the longest the tap limit allows up to 16384, and 1, 2, 3, 5 and 9 rows; and the refusal edge of the longest filter, found
by bisection on lorahip_resampler_check and compared with the formula, not with a number."""
import ctypes as C
import math

import numpy as np
import pytest

KIB64, KIB160 = 64 << 10, 160 << 10
SOME = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 25, 31, 32, 33, 48, 63, 64, 65, 100, 125, 128, 255, 256, 257, 500, 512, 513, 1000, 1023, 1024]
ROWS = [1, 2, 3, 5, 9]
FIELDS = ("ns", "rg", "pb", "n_phase_blocks", "ti", "qp", "waves", "lds_bytes", "t", "up_reduced", "down_reduced")


def _ceil(a, b):
    return -(-a // b)


def _span(NS, T, PB, U, D, Dp):
    """TI of the header: (NS - 1) D' + T + ceil((PB - 1) D / U) + 1"""
    return (NS - 1) * Dp + T + _ceil((PB - 1) * D, U) + 1


def _lds(NS, RG, T, PB, U, D, Dp):
    """bytes of LDS the header's formula gives a tiling: the span rounded up to D' * QP with QP odd, next to NS * PB outputs"""
    QP = _ceil(_span(NS, T, PB, U, D, Dp), Dp) | 1
    return RG * (Dp * QP + NS * PB) * 8


def test_plan_fields_and_refusal_match_check():
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    assert [n for n, _ in _lib.ResamplerTiling._fields_] == list(FIELDS)
    p = L.Resampler.plan(5, 6, 120, 9)
    assert sorted(p) == sorted(FIELDS) and p["t"] == 24 and p["up_reduced"] == 5 and p["down_reduced"] == 6 and p["rg"] == 8
    assert L.Resampler.plan(4, 6, 48) == L.Resampler.plan(4, 6, 48, n_rows=1) and L.Resampler.plan(4, 6, 48)["up_reduced"] == 2
    t = _lib.ResamplerTiling()
    for bad in [(0, 6, 192, 1), (5, 0, 192, 1), (5, 6, 0, 1), (5, 6, 192, 0), (1025, 6, 192, 1), (5, 1025, 192, 1), (5, 6, 65537, 1),
                (5, 6, 192, 65535 * 8 + 1), (1, 1, 65536, 1)]:
        assert lib.lorahip_resampler_plan(5, 6, 192, 1, C.byref(t)) == 0 and t.ns != 0
        assert lib.lorahip_resampler_check(*bad) == -1
        text = lib.lorahip_last_error()
        lib.lorahip_resampler_check(5, 6, 192, 1)
        assert lib.lorahip_resampler_plan(*bad, C.byref(t)) == -1, bad
        assert lib.lorahip_last_error() == text and text.startswith(b"resampler: ")       # the refusal of _check, word for word
        assert all(getattr(t, n) == 0 for n in FIELDS)
        with pytest.raises(L.LoraHipError):
            L.Resampler.plan(*bad)
    assert lib.lorahip_resampler_plan(5, 6, 192, 1, None) == -1


def test_every_plan_of_the_sweep_keeps_the_stated_rules():
    import time
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    lib = L.load()
    t_start = time.time()
    pairs = sorted(set([(U, D) for U in SOME for D in range(1, 1025)] + [(U, D) for D in SOME for U in range(1, 1025)]))
    assert {1, 31, 32, 33, 1023, 1024} <= {U // math.gcd(U, D) for U, D in pairs}
    cases = []
    for U, D in pairs:
        for T in sorted({1, 64, min(16384, 65536 // U)}):      # n_taps <= 65536: T = 16384 exists for up <= 4, the longest T elsewhere
            for K in ROWS:
                cases.append((U, D, T * U - (U // 2 if T > 1 else 0), K, T))
    n = len(cases)
    buf = (_lib.ResamplerTiling * n)()
    size = C.sizeof(_lib.ResamplerTiling)
    plan = lib.lorahip_resampler_plan
    refused = [i for i, (U, D, Lt, K, T) in enumerate(cases) if plan(U, D, Lt, K, C.byref(buf, i * size)) != 0]
    assert not refused, ("T <= 16384 is never refused", cases[refused[0]])
    got = np.frombuffer(buf, dtype=np.uint64).reshape(n, len(FIELDS)).astype(np.int64)
    NS, RG, PB, NPB, TI, QP, W, LDS, T, Up, Dp = got.T
    U, D, Lt, K, Tw = np.array(cases, np.int64).T
    g = np.gcd(U, D)

    def holds(ok, what):
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (what, cases[bad[0]], dict(zip(FIELDS, got[bad[0]])))
    holds((T == Tw) & (T == -(-Lt // U)) & (Up == U // g) & (Dp == D // g), "T, U', D'")
    assert {1, 64, 16384} <= set(T.tolist())
    holds((NS >= 1) & (NS <= 512) & ((NS & (NS - 1)) == 0), "NS is a power of two in 1..512")
    holds(np.isin(RG, [1, 2, 4, 8]) & (RG < 2 * K), "RG in {1, 2, 4, 8} and RG < 2 K")
    holds(PB == np.minimum(Up, 32), "PB = min(U', 32)")
    holds(NPB == -(-Up // PB), "phase blocks = ceil(U' / PB)")
    holds(TI == (NS - 1) * Dp + T + -(-((PB - 1) * D) // U) + 1, "TI")
    holds((QP % 2 == 1) & (Dp * QP >= TI), "QP odd and D' QP >= TI")
    holds(LDS == RG * (Dp * QP + NS * PB) * 8, "LDS bytes")
    holds(LDS <= np.where((RG > 1) | (NS > 64), KIB64, KIB160), "64 KiB where RG > 1 or NS > 64, 160 KiB always")
    holds((W >= 1) & (W <= 8), "wavefronts per workgroup in 1..8")
    # fewer than 64 steps only where 64 steps of one row do not fit the 160 KiB
    QP64 = -(-((63 * Dp + T + -(-((PB - 1) * D) // U) + 1)) // Dp) | 1
    holds((NS >= 64) | ((Dp * QP64 + 64 * PB) * 8 > KIB160), "NS < 64 only where NS = 64 at RG = 1 exceeds 160 KiB")
    # every branch exists in the sweep (but NS = 1: it takes T > 16384, test_refusal_edge_is_where_the_formula_puts_it stands on it)
    assert set(NS.tolist()) == {2, 4, 8, 16, 32, 64, 128, 256, 512} and set(RG.tolist()) == {1, 2, 4, 8}
    assert np.any((NS == 64) & (LDS > KIB64)) and np.any((RG == 1) & (K > 1) & (LDS <= KIB64))
    print("resampler plan sweep: %d plans in %.1f s" % (n, time.time() - t_start))


@pytest.mark.parametrize("U,D", [(1, 1024), (1, 1)])
def test_refusal_edge_is_where_the_formula_puts_it(U, D):
    """the longest filter of one row: accepted while ONE step (NS = 1, RG = 1) fits 160 KiB by the header's formula"""
    import lora_sdr_amd as L
    lib = L.load()
    accepted = lambda Lt: lib.lorahip_resampler_check(U, D, Lt, 1) == 0
    lo, hi = 1, 65536
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    by_formula = [Lt for Lt in range(1, 65537) if _lds(1, 1, _ceil(Lt, U), 1, U, D, D) <= KIB160]
    assert by_formula == list(range(1, by_formula[-1] + 1))                # monotone: bisection finds THE edge
    assert lo == by_formula[-1] > 16384 * U, (lo, by_formula[-1])
    p = L.Resampler.plan(U, D, lo, 1)
    assert p["ns"] == 1 and p["rg"] == 1 and p["lds_bytes"] == _lds(1, 1, lo, 1, U, D, D) <= KIB160
    assert b"LDS" in (lib.lorahip_resampler_check(U, D, lo + 1, 1), lib.lorahip_last_error())[1]
    # and more rows change nothing about the edge
    assert lib.lorahip_resampler_check(U, D, lo, 9) == 0 and lib.lorahip_resampler_check(U, D, lo + 1, 9) == -1
    print("resampler %d/%d: the longest filter is %d taps (%d bytes of LDS)" % (U, D, lo, p["lds_bytes"]))
