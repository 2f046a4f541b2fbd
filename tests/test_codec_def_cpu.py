"""CPU: tests/codec_def.py pinned -- through the oracle's decoder, against the golden encoder output and, where oracle/_ref is built,
against the verbatim LoRaEncoder.cpp -- and the crafted sets of tests/codec_edge_inputs.py checked on the oracle's results alone: every set
must hold what tests/test_gpu_decoder_edges.py needs it for."""
import numpy as np
import pytest

import codec_def as D
import codec_edge_inputs as S
from test_gpu_encoder import comparable

RATES = ["4/4", "4/5", "4/6", "4/7", "4/8"]
LENGTHS = list(range(0, 41)) + [100, 255, 300]               # the list of test_encoder_cpu.py


def symbol_sizes(sf):
    return sorted({0, sf - 2, 5})


@pytest.mark.parametrize("sf", [7, 9, 12])
def test_build_decodes_to_its_payload(oracle, sf):
    """build -> oracle.decode with error_check and crcc on: never dropped, and the bytes are the reference's for that packet -- the
    payload with header and crc; the payload minus its last two bytes with a header whose crc flag is off (the block cuts five
    bytes either way, LoRaDecoder.cpp:379); without a header the announced bytes, the two crc bytes cancelled to zero (:386-387)"""
    rng = np.random.default_rng(sf)
    n = 0
    for ppm in symbol_sizes(sf):
        for rdd in range(5):
            for explicit in (True, False):
                for crc in (True, False):
                    for length in range(2, 41):
                        data = rng.integers(0, 256, length).astype(np.uint8)
                        syms, cw = D.build(sf, data, ppm, rdd, explicit, crc)
                        assert syms.size == D.num_symbols_def(cw.size, ppm or sf, rdd)
                        out, dropped = oracle.decode(sf, syms, ppm=ppm, cr=RATES[rdd], crcc=crc or explicit, error_check=True, explicit=explicit,
                                                     data_length=length)
                        if explicit:
                            want = data if crc else data[:-2]
                        else:
                            want = np.concatenate([data, np.zeros(2, np.uint8)]) if crc else data
                        assert dropped == 0 and out is not None and np.array_equal(out, want), (sf, ppm, rdd, explicit, crc, length)
                        n += 1
    assert n == len(symbol_sizes(sf)) * 5 * 2 * 2 * 39


def test_build_equals_the_golden_encoder_output(golden):
    """the undamaged recorded packets of codec_kat.npz (verbatim LoRaEncoder.cpp) under the masking of `comparable`: the pad codewords'
    bits of the last block are undefined in the reference, everything else is equal bit by bit"""
    g = golden("codec_kat.npz")
    n = 0
    for i in range(int(g["count"])):
        sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = (int(v) for v in g["cfg_%d" % i])
        if int(g["res_%d" % i][2]) != 0:
            continue
        data = g["data_%d" % i]
        syms, _ = D.build(sf, data, ppm, rdd, bool(explicit), bool(crcc))
        want = g["syms_%d" % i]
        assert syms.size == want.size, i
        a, b = comparable(syms, data.size, sf, ppm, rdd, bool(explicit), bool(crcc)), comparable(want, data.size, sf, ppm, rdd, bool(explicit), bool(crcc))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
        n += 1
    assert n >= 100


@pytest.mark.parametrize("sf", [7, 9, 12])
def test_build_equals_the_verbatim_encoder(ref, sf):
    rng = np.random.default_rng(50 + sf)
    n = 0
    for ppm in symbol_sizes(sf):
        for rdd in range(5):
            for explicit in (False, True):
                for crc in (False, True):
                    for length in LENGTHS:
                        if length == 0 and not crc:
                            continue                                   # the reference cannot encode it (test_encoder_cpu.py)
                        data = rng.integers(0, 256, length).astype(np.uint8)
                        syms, _ = D.build(sf, data, ppm, rdd, explicit, crc)
                        want = ref.encode(sf, data, ppm=ppm, cr=RATES[rdd], explicit=explicit, crc=crc)
                        assert syms.size == want.size, (sf, ppm, rdd, explicit, crc, length)
                        a, b = comparable(syms, length, sf, ppm, rdd, explicit, crc), comparable(want, length, sf, ppm, rdd, explicit, crc)
                        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (sf, ppm, rdd, explicit, crc, length)
                        n += 1
    assert n == len(symbol_sizes(sf)) * 5 * (2 * len(LENGTHS) + 2 * (len(LENGTHS) - 1))


def test_flip_changes_one_bit_of_one_codeword():
    """every bit of every codeword of a packet, at a symbol size below and at the spreading factor: de-interleaved by the definition
    the damaged packet differs from the clean one in that bit of that codeword only"""
    rng = np.random.default_rng(4)
    for sf, ppm, rdd in ((7, 0, 4), (9, 7, 1), (12, 0, 0), (8, 5, 3), (10, 0, 2)):
        P = ppm or sf
        syms, cw = D.build(sf, rng.integers(0, 256, 11).astype(np.uint8), ppm, rdd, True, True, n_blocks=1)
        clean = D.codewords_of(syms, sf, ppm, rdd)
        assert np.array_equal(clean, cw)
        for c in range(cw.size):
            for b in range(8 if c < P else 4 + rdd):
                diff = D.codewords_of(D.flip(syms, sf, ppm, rdd, c, b), sf, ppm, rdd) ^ clean
                assert np.count_nonzero(diff) == 1 and diff[c] == 1 << b, (sf, ppm, rdd, c, b)
        with pytest.raises(AssertionError):
            D.flip(syms, sf, ppm, rdd, P, 4 + rdd)                     # a bit the codeword does not have


def test_set_header_equals_build_and_touches_only_the_first_block():
    rng = np.random.default_rng(6)
    for sf, ppm, rdd in ((7, 0, 4), (9, 7, 1), (8, 5, 3)):
        data = rng.integers(0, 256, 9).astype(np.uint8)
        body, _ = D.build(sf, data, ppm, rdd, True, True, n_blocks=2)
        ln, crc, rate = S.header_grid((0, 1, 9, 200, 255))
        got = D.set_header(body, sf, ppm, ln, crc, rate)
        assert got.shape == (80, body.size) and np.array_equal(got[:, 8:], np.tile(body[8:], (80, 1)))
        for i in range(80):
            want, _ = D.build(sf, data, ppm, rdd, True, True, hdr_len=int(ln[i]), hdr_crc=int(crc[i]), hdr_rdd=int(rate[i]), n_blocks=2)
            assert np.array_equal(got[i], want), (sf, ppm, rdd, i)


def test_decoded_end_is_the_closed_form_where_one_exists():
    """the walked loops against plain counting: 2 * bytes nibbles, one less behind a header's five codewords and six nibbles, never less
    than the first block and its odd nibble"""
    for P in range(5, 13):
        for explicit in (False, True):
            for nbytes in range(0, 300):
                c_end, odd = D.decoded_end(P, explicit, nbytes)
                shift = 1 if explicit else 0
                assert odd == bool((P + shift) & 1)
                assert c_end == max(2 * nbytes - shift, P + (1 if odd else 0))


@pytest.mark.parametrize("sf,ppm,rdd", S.H_CONFIGS)
def test_set_h_holds_every_outcome(oracle, sf, ppm, rdd):
    """set H on the oracle alone (the tables test_gpu_decoder_edges.py compares the kernels with): 4096 headers over one body"""
    assert S.set_h(sf, ppm, rdd).shape[0] == 4096
    S.check_set_h({(hdr, crcc, ec): S.set_h_table(oracle, (sf, ppm, rdd, crcc, 1, ec, 1, hdr, 8))
                   for hdr in (0, 1) for crcc in (0, 1) for ec in (0, 1)})
    # the one-lane checker's share: lengths 0..16 on a body of at most 520 symbols
    short = S.set_h(sf, ppm, rdd, 16, 8)
    assert short.shape[0] == 17 * 16 and short.shape[1] <= 520
    S.check_set_h({(hdr, crcc, ec): S.set_h_table(oracle, (sf, ppm, rdd, crcc, 1, ec, 1, hdr, 8), 16, 8)
                   for hdr in (0, 1) for crcc in (0, 1) for ec in (0, 1)})
    # the 16-symbol packets of sets G and B
    tiny = S.set_h(sf, ppm, rdd, 4, 2, 16)
    assert tiny.shape == (80, 16)
    kinds = {S.outcome(r) for hdr in (0, 1) for r in S.set_h_table(oracle, (sf, ppm, rdd, 1, 1, 1, 1, hdr, 8), 4, 2, 16)}
    assert kinds == {"bytes", "dropped", "nothing"}


@pytest.mark.parametrize("sf,ppm", S.E_SYMBOL_SIZES)
def test_set_e_straddles_the_decode_boundary(oracle, sf, ppm):
    P = ppm or sf
    parities, by_fill = set(), set()
    for group in S.e_groups():
        if group[:2] != (sf, ppm):
            continue
        packets, labels, c_end, odd = S.set_e(*group)
        assert packets.shape[1] <= 64 and len(labels) == packets.shape[0]
        S.check_set_e(labels, c_end, S.set_e_table(oracle, *group, 0), S.set_e_table(oracle, *group, 1))
        parities.add((group[3], odd))
        by_fill.add(c_end == P + (1 if odd else 0))
        # two flipped bits: one result at least differs from the clean packet's with error_check off (uncorrectable or miscorrected or
        # caught by the crc), so the damage is real
        off = S.set_e_table(oracle, *group, 0)
        two = [i for i, (k, _, _) in enumerate(labels) if k == "two"]
        assert len(two) == 4 and any(off[i][0] is None or not np.array_equal(off[i][0], off[0][0]) for i in two)
    # whether the nibble count is odd after the first block follows from the symbol size and the header, not from the payload: with and
    # without a header every symbol size gives one of each
    assert parities == {(1, bool((P + 1) & 1)), (0, bool(P & 1))}
    assert by_fill == {True, False}                  # the end of the range set by the first block, and by the bytes


def test_sets_select_every_group_size_and_the_reduced_launch():
    """from the launch code restated in codec_edge_inputs.launch_shape: the strides of set G select 8 / 16 / 32 / 64 lanes per packet
    with an explicit header (one exception: SF12 at 4/4 never needs more than 188 symbols, its largest group is 32), the implicit
    lengths do at one stride, set P fits three packets a workgroup where four lane groups run, set B runs at 8 lanes"""
    for sf, ppm in S.E_SYMBOL_SIZES:
        for rdd in (1, 2, 3, 4):
            assert [S.launch_shape(sf, ppm, rdd, 1, 8, st)[0] for st in S.G_STRIDES] == [8, 16, 32, 64]
    for sf, ppm, rdd in S.H_CONFIGS:
        want = [8, 16, 32, 32] if (sf, rdd) == (12, 0) else [8, 16, 32, 64]
        assert [S.launch_shape(sf, ppm, rdd, 1, 8, st)[0] for st in S.G_STRIDES] == want
    for sf, ppm, rdd, stride in ((12, 0, 4, 512), (7, 0, 1, 512)):
        assert [S.launch_shape(sf, ppm, rdd, 0, n, stride)[0] for n in (6, 30, 70, 300)] == [8, 16, 32, 64]
    assert [S.launch_shape(7, ppm, 4, 0, 4096, 16384) for ppm in (5, 4, 2)] == [(64, 42752, 3), (64, 49280, 3), (64, 41072, 3)]
    assert S.launch_shape(7, 0, 4, 1, 8, 16)[::2] == (8, 32)


@pytest.mark.parametrize("ppm", [5, 4, 2])
def test_set_p_outcomes(oracle, ppm):
    """PPM 5: five packets decode to 4098 bytes, the damaged byte and the cut packet are dropped; PPM 4 and 2: a row cannot hold the
    packet and the reference drops all seven"""
    table = S.set_p_table(oracle, ppm, 0)
    assert [S.outcome(r) for r in table] == (["bytes"] * 5 + ["dropped"] * 2 if ppm == 5 else ["dropped"] * 7)
    if ppm == 5:
        assert all(r[0].size == 4098 and not r[0][4096:].any() for r in table[:5])
        assert len({r[0].tobytes() for r in table[:5]}) == 5
