"""GPU: the rational-rate resampler on every branch of its tiling and through every kernel instance. tests/test_gpu_resampler.py runs
NS = 64 .. 512 steps with filters of T <= 64; here are the plans with fewer than 64 steps (idle lanes), the filters of thousands of
taps a lane, every remainder of the tap loop's last round, a last phase block of one phase and phase blocks without a tap, row grids
beyond 65535 groups, the twelve instances {RG 1, 2, 4, 8} x {cf32, sc16, sc8}, and stream positions up to the 2^52 limit.

Every case first asks Resampler.plan (lorahip_resampler_plan) for the tiling and asserts the branch it is named for: a retuned
resampPlan that moves a shape fails the case instead of silently leaving the branch uncovered.

The instrument for a wrong tap: taps that are integers in [-3, 3] and samples with integer components in [-7, 7]. Every partial sum of
the T fused multiply-adds is an integer of magnitude <= 21 T < 2^24, so the fp32 chain is exact and the kernel must EQUAL the float64
definition (tests/resampler_def.py), value for value. The (T + 2) 2^-24 scale bound of the random-data checks is right as a worst
case but spans +-48 around outputs of about 300 at T = 18500: one dropped, doubled or misplaced tap passes it, and fails the equality.

What stays untested: the refusal of a call whose tiles x phase blocks exceed the launch grid (DESIGN.md section 8h says why)."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

import resampler_def as rd

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
KIB64, KIB160 = 64 << 10, 160 << 10


def _ceil(a, b):
    return -(-a // b)


def _rows(rng, K, n):
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def _int_rows(rng, K, n):
    """components that are integers in [-7, 7]"""
    return (rng.integers(-7, 8, (K, n)) + 1j * rng.integers(-7, 8, (K, n))).astype(np.complex64)


def _int_taps(rng, L):
    """integers in [-3, 3], none of them 0: every tap shows in the sum"""
    return (rng.integers(1, 4, L) * rng.choice([-1, 1], L)).astype(np.float32)


def _taps(Lh, rng, U, D, L):
    """a low-pass made asymmetric by random factors: the tap order matters"""
    h = Lh.Resampler.design(U, D, L) if L > 1 else np.ones(1, np.float32)
    return (h * rng.uniform(0.5, 1.5, L)).astype(np.float32)


def bound(T, scale):
    """T fused multiply-adds per component, each ONE rounding of a partial sum that error_scale bounds: (T + 2) * 2^-24 * scale"""
    return (T + 2) * U24 * scale


def _def_at(x, U, D, h, ms, n0=0):
    """rd.resample_at in slices of ms, so that the (K, outputs, T) products it forms stay within about 2^21 elements"""
    ms = [int(m) for m in ms]
    step = max(1, (1 << 21) // (x.shape[0] * _ceil(len(h), U)))
    return np.concatenate([rd.resample_at(x, U, D, h, m=ms[i:i + step], n0=n0) for i in range(0, len(ms), step)], axis=1)


def _oldest(p, U, D, tile, block):
    """absolute index of the oldest sample that workgroup (tile, phase block) stages: T - 1 before the newest sample of its first output"""
    m = tile * p["ns"] * p["up_reduced"] + block * p["pb"]
    return ((m + 1) * D - 1) // U - (p["t"] - 1)


# (K, up, down, n_taps): the branch it was chosen for, as a predicate on the plan
TILINGS = [
    ((1, 1, 1024, 18500), "one step a tile", lambda p: p["ns"] == 1 and p["lds_bytes"] > KIB160 - 16384),
    ((2, 3, 1024, 49152), "T = 16384 at D' = 1024: two steps, one row a group of two rows", lambda p: p["t"] == 16384 and p["ns"] == 2 and p["rg"] == 1),
    ((1, 1, 700, 12000), "8 steps", lambda p: p["ns"] == 8),
    ((1, 1, 256, 8000), "32 steps", lambda p: p["ns"] == 32),
    ((2, 1023, 1024, 4096), "16 steps, phase blocks of 32 and 31", lambda p: p["ns"] == 16 and p["n_phase_blocks"] == 32 and p["up_reduced"] % 32 == 31),
    ((1, 1024, 1023, 4096), "16 steps, 32 full phase blocks", lambda p: p["ns"] == 16 and p["n_phase_blocks"] == 32 and p["up_reduced"] == 1024),
    ((1, 1, 1, 16385), "64 steps in 160 KiB, D' = 1, a last round of one tap", lambda p: p["ns"] == 64 and p["lds_bytes"] > KIB64 and p["qp"] > 16384 and p["t"] % 16 == 1),
    ((5, 1, 1, 8000), "one row a group by the 64 KiB budget although K > 1", lambda p: p["rg"] == 1 and p["ns"] == 64 and KIB64 - 1024 < p["lds_bytes"] <= KIB64),
    ((9, 33, 32, 330), "a last phase block of one phase", lambda p: p["n_phase_blocks"] == 2 and p["up_reduced"] - p["pb"] == 1),
    ((3, 1024, 1, 4096), "two rows a group, the last group half filled, 32 phase blocks, D' = 1",
     lambda p: p["rg"] == 2 and p["n_phase_blocks"] == 32 and p["down_reduced"] == 1),
    ((3, 100, 3, 40), "n_taps < up, U' > 32: phases without a tap", lambda p: p["t"] == 1 and p["n_phase_blocks"] == 4),
    ((2, 1000, 7, 64), "n_taps < up, U' > 32: phase blocks without a tap", lambda p: p["t"] == 1 and p["n_phase_blocks"] == 32),
]


@pytest.mark.parametrize("shape,branch,on_branch", TILINGS, ids=["K%d-%d/%d-L%d" % s for s, _, _ in TILINGS])
def test_tiling_branch(gpu, shape, branch, on_branch):
    """(a) integer data: equal to the definition; (b) random data: within the bound, and cut into calls at the places the plan makes
    critical -- the first call ends exactly with the span of a workgroup (the last sample with which it still takes the staging path
    of a tile wholly inside the call), one sample earlier, one later, in the middle of a tile, and with a piece shorter than T - 1 --
    bit-identical to one call."""
    import torch
    import lora_sdr_amd as Lh
    K, U, D, L = shape
    p = Lh.Resampler.plan(U, D, L, K)
    assert on_branch(p), (branch, p)
    NS, Up, Dp, T, TI = p["ns"], p["up_reduced"], p["down_reduced"], p["t"], p["ti"]
    assert T == _ceil(L, U) and T * 21 < 2 ** 24
    per_tile = NS * Up
    # the first tile whose workgroups find their whole span behind the start of the stream, and from there six tiles or about 150 outputs
    first_full = _ceil(T - 1, NS * Dp) + 1
    assert _oldest(p, U, D, first_full, 0) >= 0
    tiles = first_full + max(6, min(120, 150 // per_tile))
    n = _ceil(tiles * per_tile * D, U) + 5
    n_out = n * U // D
    assert tiles <= 300 and (tiles - 1) * per_tile < n_out
    cut_tile = first_full + 2
    n1 = _oldest(p, U, D, cut_tile, p["n_phase_blocks"] - 1) + TI       # rel + TI == n_in for the last workgroup of that tile
    mid = _ceil(((cut_tile + 1) * per_tile + per_tile // 2) * D, U) + D // (2 * U)
    short = max(1, min((T - 1) // 2, (n - mid) // 2))
    assert 0 < n1 - 1 and n1 + 1 < mid < mid + short < n
    cuts = [[n1], [n1 - 1], [n1 + 1], [mid, mid + short]]
    rng = np.random.default_rng(K * 1000 + U * 7 + D)
    # the outputs the definition is evaluated at: all of them, or where that is too much the edges of every call, both sides of
    # (up to 32 of) the tile boundaries, and random ones, half of them among the outputs whose oldest tap no longer reads the zeros
    # before the stream
    if K * n_out * T <= 2 ** 24:
        sel = np.arange(n_out)
    else:
        edges = {0, n_out - 1}
        for c in sum(cuts, []):
            edges |= {c * U // D - 1, c * U // D}
        inner = np.arange(1, _ceil(n_out, per_tile)) * per_tile
        if inner.size > 32:
            inner = rng.choice(inner, 32, replace=False)
        for b in inner.tolist():
            edges |= {b - 1, b}
        edges = {m for m in edges if 0 <= m < n_out}
        m_full = _ceil((T - 1) * U + 1, D)                                 # from here on every tap of an output meets a sample of the stream
        more = max(0, 256 - len(edges))
        edges |= set(rng.integers(0, n_out, more // 2).tolist()) | set(rng.integers(m_full, n_out, more - more // 2).tolist())
        sel = np.array(sorted(edges))
        assert sel.size <= 512 and np.count_nonzero(sel >= m_full) >= 64

    with Lh.Context(7) as ctx:
        # (a)
        xi, hi = _int_rows(rng, K, n), _int_taps(rng, L)
        rs = Lh.Resampler(ctx, U, D, hi, n_rows=K)
        assert rs.out_count(n) == n_out
        got = rs.run(torch.from_numpy(xi).cuda()).cpu().numpy()
        rs.close()
        assert got.shape == (K, n_out)
        want = _def_at(xi, U, D, hi, sel)
        assert np.abs(want).max() > 21                                     # sums of many taps, not single products
        wrong = np.argwhere(got[:, sel].astype(np.complex128) != want)
        assert wrong.size == 0, ("integer data: not the definition's value", len(wrong), [(k, sel[i], got[k, sel[i]], want[k, i]) for k, i in wrong[:5]])

        # (b)
        x, h = _rows(rng, K, n), _taps(Lh, rng, U, D, L)
        xd = torch.from_numpy(x).cuda()
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        whole = rs.run(xd).cpu().numpy()
        for cut in cuts:
            rs.reset()
            parts = []
            for a, b in zip([0] + cut, cut + [n]):
                assert rs.out_count(b - a) == rd.out_count(a, b - a, U, D)
                parts.append(rs.run(xd[:, a:b]))
            glued = torch.cat(parts, dim=1).cpu().numpy()
            assert glued.shape == whole.shape == (K, n_out)
            assert np.array_equal(bits(glued), bits(whole)), ("cut at", cut)
        want = _def_at(x, U, D, h, sel)
        scale = rd.error_scale(x, h, U)
        err = float(np.abs(whole[:, sel] - want).max())
        print("resampler edges K=%d %d/%d L=%d (NS=%d RG=%d T=%d, %d B): err/scale = %.3g (bound %.3g), %d of %d outputs"
              % (K, U, D, L, NS, p["rg"], T, p["lds_bytes"], err / scale, bound(T, 1.0), sel.size, n_out))
        assert err <= bound(T, scale), (err, scale)
        assert float(np.abs(want).max()) > 0.05 * scale / max(1.0, np.sqrt(T))      # the outputs carry signal
        if L < U:
            ph = ((np.arange(n_out) + 1) * D - 1) % U
            assert np.any(ph >= L) and np.all(whole[:, ph >= L] == 0)                # phases without a tap: exact zeros
            assert np.all(whole[:, ph < L] != 0)
            dirty = x.copy()
            dirty[K - 1, n // 2] = np.nan
            dirty[0, n // 3] = np.inf
            rs.reset()
            bad = rs.run(torch.from_numpy(dirty).cuda()).cpu().numpy()
            assert not np.isfinite(bad).all() and np.all(bad[:, ph >= L] == 0)
        rs.close()


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_every_remainder_of_the_last_tap_round(gpu, K):
    """3/2 with 3 T - 1 taps and RG = K rows a workgroup (2500 samples: the second tile of 512 steps lies wholly inside the call), a round of R = 16 / RG taps: T = 1 .. 2 R + 1 cuts the last round at every
    length, after none, one and two whole rounds. Integer data: equal to the definition. A NaN in the last row: the oldest tap of every
    output stands in the cut round, so a round that read or multiplied one sample too many (or too few) moves the set of non-finite
    outputs, which must be exactly the rule's."""
    import torch
    import lora_sdr_amd as Lh
    U, D, n, c_nan = 3, 2, 2500, 1300
    R = 16 // K
    rng = np.random.default_rng(40 + K)
    x = _int_rows(rng, K, n)
    dirty = x.copy()
    dirty[K - 1, c_nan] = np.nan
    n_out = n * U // D
    ph = ((np.arange(n_out) + 1) * D - 1) % U
    with Lh.Context(7) as ctx:
        xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dirty).cuda()
        for T in range(1, 2 * R + 2):
            L = 3 * T - 1
            p = Lh.Resampler.plan(U, D, L, K)
            assert p["rg"] == K and p["t"] == T and p["ns"] >= 64, p
            h = _int_taps(rng, L)
            rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
            got = rs.run(xd).cpu().numpy()
            rs.reset()
            one = rs.run(dd).cpu().numpy()                                 # the NaN staged from the rows (a tile wholly inside the call) ...
            rs.reset()
            cut = torch.cat([rs.run(dd[:, :c_nan + 1]), rs.run(dd[:, c_nan + 1:])], dim=1).cpu().numpy()     # ... and from the carried history
            rs.close()
            want = _def_at(x, U, D, h, range(n_out))
            assert got.shape == want.shape == (K, n_out)
            assert np.array_equal(got.astype(np.complex128), want), (T, np.argwhere(got != want)[:5])
            hit = np.array(rd.nonfinite_outputs(c_nan, U, D, L, 0, n))
            assert hit.size >= T
            for bad in (one, cut):
                nonfinite = ~np.isfinite(bad)
                assert not nonfinite[:K - 1].any()
                assert sorted(np.flatnonzero(nonfinite[K - 1])) == sorted(hit[ph[hit] < L]), T      # a phase without a tap stays exactly 0
                assert np.all(bad[K - 1, hit[ph[hit] >= L]] == 0)
                assert np.array_equal(bad[~nonfinite].astype(np.complex128), want[~nonfinite]), T


def _numbered_rows(rng, K, n):
    """integer rows, every one distinct: the real parts of the first five samples spell the row number in base 15"""
    x = _int_rows(rng, K, n)
    k = np.arange(K)
    for d in range(5):
        x[:, d].real = (k // 15 ** d) % 15 - 7
    return x


@pytest.mark.parametrize("K,U,D,L,sizes,rg", [(65539, 33, 32, 330, (17, 23), 1), (65535 * 8, 3, 2, 8, (2, 4), 8)])
def test_row_grids_beyond_65535(gpu, K, U, D, L, sizes, rg):
    """one row a workgroup and 65539 rows: the row group is blockIdx.y + 65535 blockIdx.z with z = 1 for the last four; and the
    documented limit of 65535 * 8 rows, where the history kernel's grid (a row a block in y, z) has z = 0 .. 7. Two calls, so that the
    carried rows are read back through that decomposition. Every row is distinct and compared exactly; a pattern stands behind n_out
    of every row, between the rows and behind the last row."""
    import torch
    import lora_sdr_amd as Lh
    p = Lh.Resampler.plan(U, D, L, K)
    assert p["rg"] == rg and p["t"] > 1, p
    assert (_ceil(K, rg) > 65535) if rg == 1 else (K == 65535 * 8 and K > 65535)
    rng = np.random.default_rng(K % 1000)
    n = sum(sizes)
    x = _numbered_rows(rng, K, n)
    assert len(np.unique(x[:, :5].real, axis=0)) == K
    h = _int_taps(rng, L)
    n_out = n * U // D
    # the definition is linear: its outputs for the n unit rows are the matrix every row is multiplied with (exact: integers in float64)
    want = x.astype(np.complex128) @ rd.resample_at(np.eye(n), U, D, h, m=range(n_out))
    stride = n_out + 7
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        xd = torch.from_numpy(x).cuda()
        flat = torch.full((K * stride + 100,), 7.0, dtype=torch.complex64, device="cuda")
        buf = flat[:K * stride].view(K, stride)
        c1 = rs.out_count(sizes[0])
        assert c1 == rd.out_count(0, sizes[0], U, D)
        a = rs.run(xd[:, :sizes[0]], out=buf[:, 3:3 + c1])
        c2 = rs.out_count(sizes[1])
        assert c1 + c2 == n_out
        b = rs.run(xd[:, sizes[0]:], out=buf[:, 3 + c1:3 + c1 + c2 + 2])
        assert a.shape == (K, c1) and b.shape == (K, c2)
        got = buf[:, 3:3 + n_out].cpu().numpy()
        guards = bool((buf[:, :3] == 7.0).all()) and bool((buf[:, 3 + n_out:] == 7.0).all()) and bool((flat[K * stride:] == 7.0).all())
        rs.close()
    wrong = np.flatnonzero((got.astype(np.complex128) != want).any(axis=1))
    assert wrong.size == 0, ("rows that are not the definition's", wrong.size, wrong[:8])
    assert guards


@pytest.mark.parametrize("dtype", ["int16", "int8"])
@pytest.mark.parametrize("K,U,D,L", [(1, 5, 6, 120), (2, 5, 6, 120), (4, 5, 6, 120), (8, 5, 6, 120), (1, 1, 1024, 64)])
def test_integer_rows_through_every_instance(gpu, dtype, K, U, D, L):
    """{RG 1, 2, 4, 8} x {sc16, sc8}, and a plan of 16 steps in 160 KiB in both formats: bit-identical to run() on the fp32 conversion,
    in pieces and alternating with run(); and with scale 1 on integer data equal to the definition"""
    import torch
    import lora_sdr_amd as Lh
    p = Lh.Resampler.plan(U, D, L, K)
    if D == 1024:
        assert p["ns"] == 16 and p["rg"] == 1 and p["lds_bytes"] > KIB64, p
    else:
        assert p["rg"] == K, p
    per_tile_in = _ceil(p["ns"] * p["up_reduced"] * D, U)
    n = max(3000, 3 * per_tile_in + 7)
    rng = np.random.default_rng(11 + K)
    info = np.iinfo(dtype)
    ints = rng.integers(info.min, info.max + 1, (K, n + 9, 2)).astype(dtype)
    h = _taps(Lh, rng, U, D, L)
    pieces = [5, 1, 0, 700, 33, per_tile_in + 1, n]
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        di = torch.from_numpy(ints).cuda()
        for scale in (None, 3.0e-3):
            s32 = np.float32(scale if scale is not None else (2.0 ** -15 if dtype == "int16" else 2.0 ** -7))
            conv = (s32 * ints.astype(np.float32)).astype(np.float32)      # one fp32 multiply per component
            x = torch.from_numpy(np.ascontiguousarray(conv).view(np.complex64)[..., 0]).cuda()
            rs.reset()
            want = rs.run(x[:, 4:4 + n])
            rs.reset()
            parts, pos = [], 0
            for s in pieces:
                s = min(s, n - pos)
                parts.append(rs.run_int(di[:, 4 + pos:4 + pos + s], scale=scale))   # rows a slice: stride n + 9 samples
                pos += s
            assert pos == n
            got = torch.cat(parts, dim=1)
            rs.reset()
            cut = n // 3 + 1
            mixed = torch.cat([rs.run_int(di[:, 4:4 + cut], scale=scale), rs.run(x[:, 4 + cut:4 + n])], dim=1)
            assert got.shape == want.shape == (K, n * U // D)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
            assert np.array_equal(bits(mixed.cpu().numpy()), bits(want.cpu().numpy()))
        rs.close()
        # scale 1 and small integers: the conversion and the whole chain are exact
        xi, hi = _int_rows(rng, K, n), _int_taps(rng, L)
        small = np.stack([xi.real, xi.imag], axis=-1).astype(dtype)
        rs = Lh.Resampler(ctx, U, D, hi, n_rows=K)
        got = rs.run_int(torch.from_numpy(small).cuda(), scale=1.0).cpu().numpy()
        rs.close()
    assert p["t"] * 21 < 2 ** 24
    assert np.array_equal(got.astype(np.complex128), _def_at(xi, U, D, hi, range(n * U // D)))


@pytest.mark.parametrize("K,U,D,L,n", [(2, 1024, 1, 2500, 40), (2, 1023, 1024, 4000, 3000), (1, 1, 1024, 64, 5000)])
def test_the_last_samples_before_the_position_limit(gpu, K, U, D, L, n):
    """reset(2^52 - n) and n samples in two calls: counts and values are the definition's at that position (t_m reaches 2^62 at
    up = 1024), on integer data and exactly. Then nothing more fits: out_count(1) is 0, a run of one sample is refused with the limit
    in its text and consumes nothing (its buffers are real and large enough, so a missing refusal would do no harm), and after reset()
    the first outputs come again."""
    import torch
    import lora_sdr_amd as Lh
    lib = Lh.load()
    rng = np.random.default_rng(52 + U)
    n0 = 2 ** 52 - n
    x, h = _int_rows(rng, K, n), _int_taps(rng, L)
    want = _def_at(x, U, D, h, range(n0 * U // D, 2 ** 52 * U // D), n0=n0)
    first = _def_at(x, U, D, h, range(n * U // D))
    assert want.shape[1] == rd.out_count(n0, n, U, D) and np.abs(want).max() > 0
    cut = n // 3 + 1
    with Lh.Context(7) as ctx:
        rs = Lh.Resampler(ctx, U, D, h, n_rows=K)
        xd = torch.from_numpy(x).cuda()
        rs.run(xd)                                                         # something to forget
        rs.reset(position=n0)
        assert rs.out_count(n) == want.shape[1] and rs.out_count(n + 1) == 0
        assert rs.out_count(cut) == rd.out_count(n0, cut, U, D)
        a = rs.run(xd[:, :cut])
        assert rs.out_count(n - cut) == rd.out_count(n0 + cut, n - cut, U, D)
        b = rs.run(xd[:, cut:])
        got = torch.cat([a, b], dim=1).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got.astype(np.complex128), want), np.argwhere(got != want)[:5]
        # the stream stands at 2^52
        assert rs.out_count(0) == 0 and rs.out_count(1) == 0
        room = torch.full((K, 2 * U + 8), 7.0, dtype=torch.complex64, device="cuda")
        count = C.c_size_t(123)
        assert lib.lorahip_resampler_run(rs._h, C.c_void_p(xd.data_ptr()), n, 1, C.c_void_p(room.data_ptr()), 2 * U + 8, C.byref(count)) == -1
        text = lib.lorahip_last_error()
        assert count.value == 0 and text.startswith(b"resampler: ") and b"2^52" in text, text
        with pytest.raises(Lh.LoraHipError):
            rs.run(xd[:, :1])
        assert bool((room == 7.0).all())
        assert rs.out_count(1) == 0
        rs.reset()
        again = rs.run(xd).cpu().numpy()
        rs.close()
    assert np.array_equal(again.astype(np.complex128), first)
