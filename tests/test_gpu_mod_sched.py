"""GPU: the scheduled modulator (lorahip_mod_frames_sched, Context.mod_frames_sched) -- SF, channel row and start sample per frame --
against the uniform modulator (lorahip_mod_frames) and the numpy definition (tests/modulator_def.py). Every comparison is of float32 bit
patterns, at every lane count the launch can run (lanes = 0 / 4 / 16 / 64)."""
import ctypes as C

import numpy as np
import pytest

from modulator_def import mod_frames_def

pytestmark = pytest.mark.gpu

LANES = [0, 4, 16, 64]
NAN_BITS = 0x7fc12345                                               # a quiet NaN no kernel produces: "not written"


def body_len(sf, n):
    return (14 << sf) + (1 << (sf - 2)) + (n << sf)


_uniform = {}


def uniform_body(torch, sf, syms, sync=0x12, ampl=1.0):
    """the body of the frame Context(sf).mod_frames makes for these symbols, as uint32 bit patterns of (re, im); computed once per frame"""
    import lora_sdr_amd as L
    key = (sf, tuple(int(s) for s in syms), sync, float(np.float32(ampl)))
    if key not in _uniform:
        ctx = L.Context(sf)
        iq = ctx.mod_frames(torch.from_numpy(np.asarray(syms, np.uint16).reshape(1, -1).view(np.int16)).cuda(), sync=sync, ampl=ampl, padding=1)
        _uniform[key] = iq[0, :body_len(sf, len(syms))].cpu().numpy().view(np.uint32).reshape(-1, 2).copy()
        ctx.close()
    return _uniform[key]


class Sched:
    """frames (sf, symbols, row, start[, ampl]) -> the device tensors of one launch and the rows it writes into"""

    def __init__(self, torch, frames, n_rows, row_len, sym_stride=None, slack=0, nsyms=None):
        self.torch, self.frames, self.n_rows, self.row_len = torch, frames, n_rows, row_len
        F = len(frames)
        S = sym_stride or max(len(f[1]) for f in frames)
        host = np.zeros((F, S), np.uint16)
        for i, f in enumerate(frames):
            host[i, :len(f[1])] = f[1]
        self.syms = torch.from_numpy(host.view(np.int16)).cuda()
        self.nsyms = torch.from_numpy(np.array([len(f[1]) for f in frames] if nsyms is None else nsyms, np.int32)).cuda()
        self.sf = torch.from_numpy(np.array([f[0] for f in frames], np.int32)).cuda()
        self.row = torch.from_numpy(np.array([f[2] for f in frames], np.int32)).cuda()
        self.start = torch.from_numpy(np.array([f[3] for f in frames], np.int64)).cuda()
        self.ampl_of = torch.from_numpy(np.array([f[4] if len(f) > 4 else 1.0 for f in frames], np.float32)).cuda()
        self.slack = slack

    def run(self, ctx, lanes, ampl=1.0, per_frame=False, sync=0x12):
        """-> (rows as uint32 (n_rows, row_len + slack, 2), status)"""
        torch = self.torch
        fill = torch.full((self.n_rows, self.row_len + self.slack, 2), NAN_BITS, dtype=torch.int32, device="cuda")
        out = fill.view(torch.float32).view(torch.complex64)[:, :, 0][:, :self.row_len]
        status = ctx.mod_frames_sched(self.syms, self.nsyms, self.sf, self.row, self.start, out, ampl=ampl,
                                      ampl_of=self.ampl_of if per_frame else None, sync=sync, lanes=lanes)
        return fill.cpu().numpy().view(np.uint32), status.cpu().numpy()


def check_rows(got, expect):
    """expect: [(row, start, body bits)]; everything else of `got` keeps the fill"""
    want = np.full(got.shape, NAN_BITS, np.uint32)
    for row, start, body in expect:
        want[row, start:start + body.shape[0]] = body
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (row, sample, re/im): %s of %d" % (bad[0].tolist(), bad.shape[0])


@pytest.fixture(scope="module")
def ctx(gpu):
    import lora_sdr_amd as L
    c = L.Context(9)                                                # device and stream only: no frame below is SF9's because of it
    yield c
    c.close()


def set1_frames():
    rng = np.random.default_rng(61)
    frames = []
    for sf in range(6, 13):
        frames.append((sf, rng.integers(0, 1 << sf, 1 + (sf % 3)).tolist()))
    frames += [frames[0], frames[6], frames[3]]                     # duplicates: the same frame twice in one launch
    return frames


@pytest.mark.parametrize("lanes", LANES)
def test_bodies_equal_the_uniform_modulator(gpu, ctx, lanes):
    """one frame per SF 6..12 of 1..3 symbols, and three of them twice, a row each: every body is mod_frames' for the same symbols, bit for
    bit -- at amplitude 1.0 and 0.7, given per launch and per frame (ampl_dev), and with another sync word"""
    frames = set1_frames()
    row_len = body_len(12, 3) + 7
    for ampl, per_frame, sync in ((1.0, False, 0x12), (0.7, False, 0x12), (0.7, True, 0x12), (1.0, False, 0x8e)):
        a_of = [0.7 if i % 2 else 1.0 for i in range(len(frames))] if per_frame else [ampl] * len(frames)
        sched = Sched(gpu, [(sf, s, r, 5 if r % 2 else 0, a_of[r]) for r, (sf, s) in enumerate(frames)], len(frames), row_len)
        got, status = sched.run(ctx, lanes, ampl=ampl if not per_frame else 123.0, per_frame=per_frame, sync=sync)
        assert not status.any()
        check_rows(got, [(r, 5 if r % 2 else 0, uniform_body(gpu, sf, s, sync=sync, ampl=a_of[r])) for r, (sf, s) in enumerate(frames)])


@pytest.fixture(scope="module")
def def_frames():
    """SF6..8 frames, symbols >= N among them, and their bodies by the numpy definition (computed once)"""
    frames = [(6, [5, 63, 64]), (6, [0xffff]), (7, [127, 128, 300]), (8, [0, 255]), (8, [256, 40000, 7]), (7, [1])]
    bodies = []
    for sf, s in frames:
        d = mod_frames_def(sf, np.array([s], np.uint16), 0x12, 0.7, 1)[0, :body_len(sf, len(s))]
        bodies.append(np.ascontiguousarray(d).view(np.float32).view(np.uint32).reshape(-1, 2))
    return frames, bodies


@pytest.mark.parametrize("lanes", LANES)
def test_bodies_equal_the_definition(gpu, ctx, def_frames, lanes):
    """against tests/modulator_def.py directly, symbols >= N included (not masked). At SF6 the quarter down-chirp is 16 samples: it ends
    inside a tile of the walker, which then goes on into the first data chirp"""
    frames, bodies = def_frames
    row_len = max(b.shape[0] for b in bodies) + 3
    sched = Sched(gpu, [(sf, s, r, 3 * (r % 2)) for r, (sf, s) in enumerate(frames)], len(frames), row_len)
    got, status = sched.run(ctx, lanes, ampl=0.7)
    assert not status.any()
    check_rows(got, [(r, 3 * (r % 2), bodies[r]) for r in range(len(frames))])


@pytest.mark.parametrize("lanes", LANES)
def test_placement_and_untouched_samples(gpu, ctx, lanes):
    """starts 0, 1, 3 and row_len - body_len; two and three frames of different SF back to back in one row (the next start is the previous
    end); a row stride above row_len. Every sample outside the bodies, the slack behind the rows included, keeps its NaN fill"""
    rng = np.random.default_rng(62)
    sy = lambda sf, n: rng.integers(0, 1 << sf, n).tolist()
    a, b, c = (7, sy(7, 2)), (6, sy(6, 3)), (8, sy(8, 1))
    la, lb, lc = body_len(7, 2), body_len(6, 3), body_len(8, 1)
    row_len = la + lb + lc + 11
    frames = [(a[0], a[1], 0, 0), (b[0], b[1], 1, 1), (c[0], c[1], 2, 3), (a[0], a[1], 3, row_len - la),
              (b[0], b[1], 4, 2), (c[0], c[1], 4, 2 + lb),                                        # two back to back
              (c[0], c[1], 5, 0), (a[0], a[1], 5, lc), (b[0], b[1], 5, lc + la),                  # three, ending 11 short of the row
              (b[0], b[1], 6, row_len - lb), (a[0], a[1], 6, row_len - lb - la)]                  # given in the other order, ending with the row
    order = rng.permutation(len(frames))
    frames = [frames[i] for i in order]
    sched = Sched(gpu, frames, 8, row_len, slack=37)                                              # (row 7: no frame at all)
    got, status = sched.run(ctx, lanes)
    assert not status.any()
    check_rows(got, [(r, st, uniform_body(gpu, sf, s)) for sf, s, r, st in frames])


@pytest.mark.parametrize("lanes", LANES)
def test_status_and_refused_frames_write_nothing(gpu, ctx, lanes):
    """-1 for a symbol count of -3, -2, -1, 0 and sym_stride + 1; -2 for a start of -1 and a body one sample past the row; -3 for SF 5 and
    13 and for rows -1 and n_rows -- mixed among good frames, which are exact; nothing else is written. status_dev may be NULL"""
    import lora_sdr_amd as L
    rng = np.random.default_rng(63)
    S, n_rows = 4, 24
    good = lambda sf, n: (sf, rng.integers(0, 1 << sf, n).tolist())
    row_len = body_len(8, 4) + 9
    cases = []                                                      # (sf, symbols, row, start, nsyms, status)

    def add(f, row, start, nsyms, status, sf=None):
        cases.append((f[0] if sf is None else sf, f[1], row, start, len(f[1]) if nsyms is None else nsyms, status))
    for i, n in enumerate((-3, -2, -1, 0, S + 1)):
        add(good(6, 2), 2 * i, 0, None, 0)
        add(good(7, 2), 2 * i + 1, 4, n, -1)
    add(good(8, 4), 10, 9, None, 0)                                 # ends with the row
    add(good(8, 4), 11, 10, None, -2)                               # one sample past it
    add(good(6, 1), 12, -1, None, -2)
    add(good(6, 1), 13, 0, None, 0)
    add(good(7, 3), 14, row_len, None, -2)
    add(good(7, 3), 15, 2 ** 62, None, -2)
    add(good(7, 1), 16, 0, None, -3, sf=5)
    add(good(7, 1), 17, 0, None, -3, sf=13)
    add(good(7, 1), 18, 0, None, -3, sf=-7)
    add(good(7, 1), -1, 0, None, -3)
    add(good(7, 1), n_rows, 0, None, -3)
    add(good(7, 1), 2 ** 31 - 1, 0, None, -3)
    add(good(7, 1), 19, 0, None, 0)
    add(good(7, 1), 20, 5, -1, -1, sf=99)                           # the symbol count is looked at first
    order = rng.permutation(len(cases))
    cases = [cases[i] for i in order]
    sched = Sched(gpu, [(sf, s, r, st) for sf, s, r, st, _, _ in cases], n_rows, row_len, sym_stride=S, nsyms=[c[4] for c in cases])
    got, status = sched.run(ctx, lanes)
    assert status.tolist() == [c[5] for c in cases]
    check_rows(got, [(r, st, uniform_body(gpu, sf, s)) for sf, s, r, st, _, stt in cases if stt == 0])
    # without a status array: the same samples
    torch = gpu
    fill = torch.full((n_rows, row_len, 2), NAN_BITS, dtype=torch.int32, device="cuda")
    ctx.use_torch_stream()
    rc = L.load().lorahip_mod_frames_sched(ctx._h, C.c_void_p(fill.data_ptr()), n_rows, row_len, row_len, C.c_void_p(sched.syms.data_ptr()), S,
                                           C.c_void_p(sched.nsyms.data_ptr()), C.c_void_p(sched.sf.data_ptr()), C.c_void_p(sched.row.data_ptr()),
                                           C.c_void_p(sched.start.data_ptr()), None, len(cases), 0x12, 1.0, lanes, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(fill.cpu().numpy().view(np.uint32), got)


@pytest.fixture(scope="module")
def sf6_bodies(gpu):
    """257 SF6 frames of one symbol each, by the uniform modulator in one launch"""
    import lora_sdr_amd as L
    syms = ((np.arange(257) * 37 + 11) % 64).astype(np.uint16)
    c6 = L.Context(6)
    iq = c6.mod_frames(gpu.from_numpy(syms.reshape(-1, 1).view(np.int16)).cuda(), padding=1)
    bodies = iq[:, :body_len(6, 1)].cpu().numpy().view(np.uint32).reshape(257, -1, 2)
    c6.close()
    return syms, bodies


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("count", [1, 15, 16, 17, 63, 64, 65, 257])
def test_frame_counts_at_group_wave_and_workgroup_edges(gpu, ctx, sf6_bodies, lanes, count):
    """1 .. 257 SF6 frames of one symbol: the last group of a wavefront, of a workgroup and of the grid at 4, 16 and 64 lanes per frame"""
    syms, bodies = sf6_bodies
    L6 = body_len(6, 1)
    # two frames a row, 3 samples apart, so that rows and starts are not the frame number
    frames = [(6, [int(syms[f])], f // 2, (f % 2) * (L6 + 3) + 1) for f in range(count)]
    sched = Sched(gpu, frames, (count + 1) // 2, 2 * L6 + 5)
    got, status = sched.run(ctx, lanes)
    assert status.shape == (count,) and not status.any()
    check_rows(got, [(f // 2, (f % 2) * (L6 + 3) + 1, bodies[f]) for f in range(count)])


@pytest.mark.parametrize("lanes", LANES)
def test_sf6_and_sf12_frames_share_a_wavefront(gpu, ctx, lanes):
    """SF6 and SF12 frames alternating, 20 of them: at 4 lanes per frame 16 frames of either kind share a wavefront, which runs as long as
    its SF12 frames while the groups of the SF6 frames have long finished"""
    rng = np.random.default_rng(64)
    kinds = [(6, rng.integers(0, 64, 2).tolist()), (12, rng.integers(0, 4096, 1).tolist()), (6, rng.integers(0, 64, 1).tolist())]
    frames = [kinds[f % 2 if f < 16 else 2] + (f, f % 5) for f in range(20)]
    sched = Sched(gpu, frames, 20, body_len(12, 1) + 4)
    got, status = sched.run(ctx, lanes)
    assert not status.any()
    check_rows(got, [(r, st, uniform_body(gpu, sf, s)) for sf, s, r, st in frames])


def test_python_surface_refusals(gpu, ctx):
    import lora_sdr_amd as L
    torch = gpu
    sched = Sched(torch, [(7, [1, 2], 0, 0)], 1, body_len(7, 2))
    out = torch.zeros((1, body_len(7, 2)), dtype=torch.complex64, device="cuda")
    args = lambda **kw: dict(dict(syms=sched.syms, nsyms=sched.nsyms, sf=sched.sf, row=sched.row, start=sched.start, out=out), **kw)
    assert ctx.mod_frames_sched(**args()).tolist() == [0]
    for lanes in (1, 8, 32, 65, -4):
        with pytest.raises(L.LoraHipError):
            ctx.mod_frames_sched(**args(lanes=lanes))
    with pytest.raises(ValueError):
        ctx.mod_frames_sched(**args(start=sched.start.to(torch.int32)))
    with pytest.raises(ValueError):
        ctx.mod_frames_sched(**args(sf=torch.cat([sched.sf, sched.sf])))
    with pytest.raises(ValueError):
        ctx.mod_frames_sched(**args(out=out.to(torch.complex128)))
    with pytest.raises(ValueError):
        ctx.mod_frames_sched(**args(out=torch.zeros((2, 4000), dtype=torch.complex64, device="cuda")[:, ::2]))
    with pytest.raises(ValueError):
        ctx.mod_frames_sched(**args(ampl_of=torch.ones(2, device="cuda")))
    # the C entry: a row longer than its stride, symbol strides outside 1 .. lorahip_decode_max_symbols(), null pointers
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    big = lib.lorahip_decode_max_symbols()

    def call(iq=p(out), stride=out.shape[1], row_len=out.shape[1], syms=p(sched.syms), S=2, nsyms=p(sched.nsyms), sf=p(sched.sf), row=p(sched.row),
             start=p(sched.start), n=1, lanes=0):
        return lib.lorahip_mod_frames_sched(ctx._h, iq, 1, stride, row_len, syms, S, nsyms, sf, row, start, None, n, 0x12, 1.0, lanes, None)
    assert call() == 0
    assert call(row_len=out.shape[1] + 1) == -1 and call(S=0) == -1 and call(S=big + 1) == -1
    for missing in ("iq", "syms", "nsyms", "sf", "row", "start"):
        assert call(**{missing: None}) == -1 and call(n=0, **{missing: None}) == 0, missing
    torch.cuda.synchronize()
