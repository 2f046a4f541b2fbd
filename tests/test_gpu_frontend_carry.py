"""GPU: the stream carry the four front ends share (csrc/lorahip_frontend.h: StreamCarry, carriedSample, carryHistory) -- a stream cut
into calls gives, bit for bit, what one call gives, also where a call is shorter than the history (the new history is then read partly
from the old one), where a call is empty, where nothing is carried at all (a synthesiser with n_taps <= interp), and after reset().

The shapes are the smallest at which the carry can go wrong; `history` is what the object keeps between calls.

    front end                      shape                                  history     input          cuts, then the rest
    Channelizer                    K 3, decim 3, 9 taps (padded to 10)    12          200            5, 0, 4, 30
    PolyphaseChannelizer           n_bins 8, decim 3, 20 taps             23          400            7, 0, 9, 60
    PolyphaseChannelizer.radix5    n_bins 5, decim 8, 7 taps              9           400            3, 0, 4, 60
    Synthesizer                    K 3, interp 3, 10 taps                 3 a row     300 a row      1, 0, 2, 40
    Synthesizer                    K 3, interp 4, 3 taps                  0           300 a row      1, 0, 2, 40
    PolyphaseSynthesizer           n_bins 8, interp 3, 10 taps, 3 rows    3 times     300 a row      1, 0, 2, 40
    PolyphaseSynthesizer.radix5    n_bins 5, interp 3, 10 taps            3 times     300 a row      1, 0, 2, 40
    PolyphaseSynthesizer           n_bins 8, interp 4, 3 taps             0           300 a row      1, 0, 2, 40
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREQS = [-0.25, 0.1, 0.3]
SYNTH_CUTS = (1, 0, 2, 40)

# (id, make(Lh, ctx, taps) -> object, n_taps, rows of the input (0: one wideband stream), samples (a row), cuts)
CASES = [
    ("chan", lambda Lh, ctx, h: Lh.Channelizer(ctx, FREQS, 3, h), 9, 0, 200, (5, 0, 4, 30)),
    ("pfb-8", lambda Lh, ctx, h: Lh.PolyphaseChannelizer(ctx, 8, 3, h), 20, 0, 400, (7, 0, 9, 60)),
    ("pfb-5", lambda Lh, ctx, h: Lh.PolyphaseChannelizer.radix5(ctx, 5, 8, h), 7, 0, 400, (3, 0, 4, 60)),
    ("synth", lambda Lh, ctx, h: Lh.Synthesizer(ctx, FREQS, 3, h), 10, 3, 300, SYNTH_CUTS),
    ("synth-no-history", lambda Lh, ctx, h: Lh.Synthesizer(ctx, FREQS, 4, h), 3, 3, 300, SYNTH_CUTS),
    ("psb-8", lambda Lh, ctx, h: Lh.PolyphaseSynthesizer(ctx, 8, 3, h, [1, -1, 1]), 10, 3, 300, SYNTH_CUTS),
    ("psb-5", lambda Lh, ctx, h: Lh.PolyphaseSynthesizer.radix5(ctx, 5, 3, h), 10, 5, 300, SYNTH_CUTS),
    ("psb-8-no-history", lambda Lh, ctx, h: Lh.PolyphaseSynthesizer(ctx, 8, 4, h), 3, 8, 300, SYNTH_CUTS),
]


@pytest.mark.parametrize("make,n_taps,rows,n,cuts", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_cut_stream_equals_one_call_bit_for_bit(gpu, make, n_taps, rows, n, cuts):
    import lora_sdr_amd as Lh
    torch = gpu
    rng = np.random.default_rng(2024)
    h = rng.uniform(-1.0, 1.0, n_taps).astype(np.float32)
    shape = (rows, n) if rows else (n,)
    x = torch.from_numpy((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)).cuda()
    assert sum(cuts) < n
    sizes = list(cuts) + [n - sum(cuts)]
    with Lh.Context(7) as ctx:
        a, b = make(Lh, ctx, h), make(Lh, ctx, h)
        n_out = a.out_count(n)
        whole = torch.view_as_real(a.run(x))
        assert whole.shape[-2] == n_out > 0 and bool(whole.abs().sum() > 0)
        for again in range(2):                                  # the cuts, reset(), the same cuts
            if again:
                b.reset()
            parts, pos = [], 0
            for s in sizes:
                want = b.out_count(s)
                parts.append(b.run(x[..., pos:pos + s]))
                assert parts[-1].shape[-1] == want
                if s == 0:                                      # an empty call: an empty result, and (below) nothing changed
                    assert parts[-1].numel() == 0
                pos += s
            assert pos == n
            glued = torch.view_as_real(torch.cat(parts, dim=-1))
            assert glued.shape == whole.shape and torch.equal(glued, whole), "pass %d" % again
        a.close(); b.close()
