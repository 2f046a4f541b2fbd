"""GPU: the batched encoder (lorahip_encode_packets) against the verbatim LoRaEncoder.cpp, through the batched decoder, and at the
head of the whole chain bytes -> symbols -> IQ -> noise -> streaming demodulator -> decoder -> bytes; the modulator with per-frame symbol
counts (lorahip_mod_frames_var) against the verbatim LoRaMod.cpp and against the uniform kernel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = ["4/4", "4/5", "4/6", "4/7", "4/8"]
LENGTHS = list(range(0, 41)) + [100, 255, 300]


def ulp_diff(a, b):
    """distance in float32 ulps between two float arrays"""
    ia = np.ascontiguousarray(a).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def gray_to_binary(g):
    g = np.asarray(g).astype(np.uint16).copy()
    for s in (8, 4, 2, 1):
        g ^= g >> s
    return g


def pad_nibbles(n, sf, ppm, explicit, crc):
    """codewords of the message that hold no byte: numCodewords - (2 * bytes + header codewords), LoRaEncoder.cpp:175"""
    P = ppm or sf
    used = 2 * (n + (2 if crc else 0)) + (5 if explicit else 0)
    return -(-used // P) * P - used


def comparable(syms, n, sf, ppm, rdd, explicit, crc):
    """what of a packet's symbols the reference DEFINES: the Gray-domain symbols with the pad codewords' bits of the last interleaver
    block cleared (the reference reads those nibbles past the end of its byte vector), and the low sf - PPM bits beside them"""
    P = ppm or sf
    syms = np.asarray(syms).astype(np.uint16)
    low = syms & ((1 << (sf - P)) - 1)
    g = syms >> (sf - P)
    g = g ^ (g >> 1)
    pad = pad_nibbles(n, sf, ppm, explicit, crc)
    if pad:
        last = 8 if len(syms) == 8 else 4 + rdd
        for k in range(last):
            for m in range(P):
                if (m + k) % P >= P - pad:
                    g[len(syms) - last + k] &= ~np.uint16(1 << m)
    return g, low


def encoder(L, sf, ppm, cr, explicit, crc, whitening=True, reuse=None):
    e = reuse or L.LoRaEncoder()
    e.setSpreadFactor(sf); e.setSymbolSize(ppm); e.setCodingRate(cr); e.enableExplicit(explicit); e.enableCrc(crc); e.enableWhitening(whitening)
    return e


def rows(torch, msgs, stride=None):
    stride = stride or max(1, max(len(m) for m in msgs))
    host = np.zeros((len(msgs), stride), np.uint8)
    for i, m in enumerate(msgs):
        host[i, :len(m)] = m
    return torch.from_numpy(host).cuda(), torch.from_numpy(np.array([len(m) for m in msgs], np.int32)).cuda()


@pytest.mark.parametrize("sf", range(7, 13))
def test_bit_identity_with_the_verbatim_encoder(gpu, ref, sf):
    """SF x rate x header x crc x symbol size {sf, sf-1, sf-2} x lengths 0..40, 100, 255, 300 of random bytes, one launch per
    configuration with all the lengths mixed: symbol counts and symbols equal LoRaEncoder.cpp's -- all 16 bits where the message fills
    its codewords (pad == 0), and everything but the pad codewords' bits of the last block where it does not (there the reference
    reads its byte vector past the end: `comparable`). Left out: the empty byte vector (length 0 without crc), which the reference
    cannot encode at all (the count wraps without a header; with one it reads pad nibbles through a null pointer)."""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(100 + sf)
    full = {cr: 0 for cr in RATES}
    compared = 0
    e = L.LoRaEncoder()
    for rdd, cr in enumerate(RATES):
        for explicit in (False, True):
            for crc in (False, True):
                for ppm in (0, sf - 1, sf - 2):
                    msgs = [rng.integers(0, 256, n).astype(np.uint8) for n in LENGTHS]
                    encoder(L, sf, ppm, cr, explicit, crc, reuse=e)
                    syms, nsyms = e.encode_batch(*rows(torch, msgs))
                    syms, nsyms = syms.cpu().numpy().view(np.uint16), nsyms.cpu().numpy()
                    for i, m in enumerate(msgs):
                        tag = (sf, ppm, cr, explicit, crc, len(m))
                        if len(m) == 0 and not crc:
                            assert nsyms[i] == (8 if explicit else -1), tag
                            continue
                        want = ref.encode(sf, m, ppm=ppm, cr=cr, explicit=explicit, crc=crc)
                        assert nsyms[i] == len(want), tag
                        got = syms[i, :nsyms[i]]
                        assert not syms[i, nsyms[i]:].any(), tag
                        if pad_nibbles(len(m), sf, ppm, explicit, crc) == 0:
                            assert np.array_equal(got, want), tag                      # full 16-bit identity, no mask
                            full[cr] += 1
                        else:
                            g0, l0 = comparable(got, len(m), sf, ppm, rdd, explicit, crc)
                            g1, l1 = comparable(want, len(m), sf, ppm, rdd, explicit, crc)
                            assert np.array_equal(g0, g1) and np.array_equal(l0, l1), tag
                        compared += 1
    print("SF%d: %d packets compared, unmasked per rate %s" % (sf, compared, full))
    assert all(v >= 4 for v in full.values()), full                # the grid must not lose its unmasked cases
    assert compared == 5 * 3 * (2 * len(LENGTHS) + 2 * (len(LENGTHS) - 1))


def test_pad_nibbles_are_zero(gpu, ref):
    """the definition that replaces the reference's over-read: without header and crc, a message whose pad is an even number of
    nibbles encodes to the symbols of the reference given the message extended by pad / 2 zero bytes (there the reference reads
    nothing out of bounds) -- all 16 bits"""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(7)
    cases = 0
    e = L.LoRaEncoder()
    for sf in range(7, 13):
        for rdd, cr in enumerate(RATES):
            for ppm in (0, sf - 1, sf - 2):
                lens = [n for n in range(1, 41) if pad_nibbles(n, sf, ppm, False, False) > 0 and pad_nibbles(n, sf, ppm, False, False) % 2 == 0]
                msgs = [rng.integers(0, 256, n).astype(np.uint8) for n in lens]
                syms, nsyms = encoder(L, sf, ppm, cr, False, False, reuse=e).encode_batch(*rows(torch, msgs))
                syms, nsyms = syms.cpu().numpy().view(np.uint16), nsyms.cpu().numpy()
                for i, m in enumerate(msgs):
                    ext = np.concatenate([m, np.zeros(pad_nibbles(len(m), sf, ppm, False, False) // 2, np.uint8)])
                    want = ref.encode(sf, ext, ppm=ppm, cr=cr, explicit=False, crc=False)
                    assert nsyms[i] == len(want) and np.array_equal(syms[i, :nsyms[i]], want), (sf, ppm, cr, len(m))
                    cases += 1
    assert cases > 1000


@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("sf", range(7, 13))
def test_codec_round_trip_on_the_device(gpu, sf, explicit):
    """encode_batch -> LoRaDecoder.decode_batch (crc check and error check on) returns the payload with dropped == 0 at every rate;
    and at 4/7 and 4/8 one Gray-domain bit flipped in one symbol of every interleaver block -- one bit error in one codeword of every
    block, the first (always 4/8) included -- is corrected: the payload comes back and the crc check passes.

    The flipped packets are decoded with the error check OFF: LoRaDecoder.cpp drops a message on any non-zero syndrome when the error
    check is on (:293, :342, :363), corrected or not, so 'error check on' and 'still decodes' exclude each other in the reference.
    Both halves are asserted: corrected with the check off (the crc check, which stays on, proves the correction), dropped with it on."""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(sf)
    e, dec = L.LoRaEncoder(), L.LoRaDecoder()
    for rdd, cr in enumerate(RATES):
        lens = list(range(1, 34)) + [64, 200, 255] if explicit else [17] * 24
        msgs = [rng.integers(0, 256, n).astype(np.uint8) for n in lens]
        encoder(L, sf, 0, cr, explicit, True, reuse=e)
        syms, nsyms = e.encode_batch(*rows(torch, msgs))
        dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True); dec.enableExplicit(explicit)
        dec.setDataLength(17)

        def check(syms_dev, tag):
            out, out_len, dropped = dec.decode_batch(syms_dev, nsyms)
            out, out_len, dropped = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy()
            assert int(dropped.sum()) == 0, (sf, cr, tag)
            for i, m in enumerate(msgs):
                # without a header the block posts the two checksum bytes behind the payload
                assert out_len[i] == len(m) + (0 if explicit else 2) and np.array_equal(out[i, :len(m)], m), (sf, cr, tag, len(m))
        check(syms, "clean")
        if rdd < 3:
            continue
        host, n = syms.cpu().numpy().view(np.uint16).copy(), nsyms.cpu().numpy()
        for i in range(len(msgs)):
            starts = [0] + list(range(8, n[i], 4 + rdd))
            for b, s0 in enumerate(starts):
                k = int(rng.integers(0, 8 if b == 0 else 4 + rdd))
                g = host[i, s0 + k] ^ (host[i, s0 + k] >> 1)                      # sf == PPM: no shift
                g ^= np.uint16(1 << int(rng.integers(0, sf)))
                host[i, s0 + k] = gray_to_binary(g)
        damaged = torch.from_numpy(host.view(np.int16)).cuda()
        _, _, dropped = dec.decode_batch(damaged, nsyms)
        assert bool((dropped == 1).all()), (sf, cr)                               # the errors are seen ...
        dec.enableErrorCheck(False)
        check(damaged, "one bit per block")                                       # ... and corrected


def test_outcomes_and_row_limits(gpu, ref):
    """-1 / -2, sentinels behind short rows, zero fill, n_packets = 0, loose strides, > 255 bytes, the host entry"""
    import lora_sdr_amd as L
    from lora_sdr_amd import _lib
    torch = gpu
    lib = L.load()
    rng = np.random.default_rng(3)
    sf, cr = 8, "4/6"
    e = encoder(L, sf, 0, cr, False, False)
    msgs = [rng.integers(0, 256, n).astype(np.uint8) for n in (0, 5, 12, 30, 31)]
    data, nb = rows(torch, msgs, stride=40)                                       # loose byte stride
    # one buffer with a sentinel behind the symbol rows; sym_stride 40 holds 8 + 5 * 6 = 38 symbols = 24 bytes
    P, stride = len(msgs), 40
    buf = torch.full((P * stride + 64,), 0x5a5a, dtype=torch.int16, device="cuda")
    nsyms = torch.full((P + 4,), 77, dtype=torch.int32, device="cuda")
    e._ctx.use_torch_stream()
    rc = lib.lorahip_encode_packets(e._ctx._h, C.byref(e._cfg), C.c_void_p(data.data_ptr()), 40, C.c_void_p(nb.data_ptr()), P,
                                    C.c_void_p(buf.data_ptr()), stride, C.c_void_p(nsyms.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    got, n = buf.cpu().numpy().view(np.uint16), nsyms.cpu().numpy()
    assert list(n[:P]) == [-1, len(ref.encode(sf, msgs[1], cr=cr, explicit=False, crc=False)),
                           len(ref.encode(sf, msgs[2], cr=cr, explicit=False, crc=False)), -2, -2] and list(n[P:]) == [77] * 4
    assert (got[P * stride:] == 0x5a5a).all()                                     # nothing behind the rows
    for i in range(P):
        row = got[i * stride:(i + 1) * stride]
        if n[i] < 0:
            assert not row.any()                                                  # a refused packet leaves a defined (zero) row
        else:
            assert not row[n[i]:].any()
    assert np.array_equal(got[2 * stride:2 * stride + n[2]], ref.encode(sf, msgs[2], cr=cr, explicit=False, crc=False))   # 12 bytes = 24 nibbles = 3 blocks: pad 0
    # a byte row shorter than the announced length: -2, and the bytes behind the row are not read as payload
    nb_long = torch.from_numpy(np.array([5, 41], np.int32)).cuda()
    s2, n2 = e.encode_batch(data[:2].contiguous(), nb_long)
    assert n2.cpu().tolist()[1] == -2 and not s2[1].cpu().numpy().any()
    # n_packets = 0: fine with a valid configuration, refused with the ones include/lorahip.h lists
    assert lib.lorahip_encode_packets(e._ctx._h, C.byref(e._cfg), None, 16, None, 0, None, 64, None) == 0
    assert lib.lorahip_encode_packets_host(e._ctx._h, C.byref(e._cfg), None, 16, None, 0, None, 64, None) == 0
    for field, value in (("struct_size", 8), ("sf", 13), ("sf", 0), ("ppm", 9), ("rdd", 5), ("rdd", -1)):
        bad = _lib.EncoderCfg.from_buffer_copy(e._cfg)
        setattr(bad, field, value)
        assert lib.lorahip_encode_packets(e._ctx._h, C.byref(bad), None, 16, None, 0, None, 64, None) == -1, field
        assert lib.lorahip_encode_packets_host(e._ctx._h, C.byref(bad), None, 16, None, 0, None, 64, None) == -1, field
    bad = _lib.EncoderCfg.from_buffer_copy(e._cfg); bad.ppm = 4; bad.explicit_hdr = 1
    assert lib.lorahip_encode_packets(e._ctx._h, C.byref(bad), None, 16, None, 0, None, 64, None) == -1
    assert lib.lorahip_encode_packets(e._ctx._h, C.byref(e._cfg), None, lib.lorahip_encode_max_bytes() + 1, None, 0, None, 64, None) == -1
    assert lib.lorahip_encode_packets(e._ctx._h, C.byref(e._cfg), None, 16, None, 0, None, lib.lorahip_decode_max_symbols() + 1, None) == -1
    assert lib.lorahip_encode_packets(e._ctx._h, C.byref(e._cfg), None, 16, None, 0, None, 0, None) == -1
    # more than 255 bytes behind an explicit header: all the bytes, length field & 0xff -- as the reference does it (pad 0: 2 * 302 + 5 = 609 = 87 * 7)
    big = rng.integers(0, 256, 300).astype(np.uint8)
    e7 = encoder(L, 7, 0, "4/8", True, True)
    assert pad_nibbles(300, 7, 0, True, True) == 0
    out = e7.work([big, bytes(big[:20])])
    assert np.array_equal(out[0], ref.encode(7, big)) and len(out[1]) == len(ref.encode(7, big[:20]))
    # the longest payload this build takes, and one byte more
    longest = rng.integers(0, 256, 4096).astype(np.uint8)
    e12 = encoder(L, 12, 0, "4/4", False, False)
    assert pad_nibbles(4096, 12, 0, False, False) == 4
    so, no = e12.encode_batch(*rows(torch, [longest]))
    want = ref.encode(12, np.concatenate([longest, np.zeros(2, np.uint8)]), cr="4/4", explicit=False, crc=False)
    assert int(no[0]) == len(want) and np.array_equal(so[0].cpu().numpy().view(np.uint16), want)
    # the host entry equals the device entry
    msgs = [rng.integers(0, 256, n).astype(np.uint8) for n in (1, 9, 33, 64)]
    e = encoder(L, 9, 8, "4/7", True, True)
    d_s, d_n = e.encode_batch(*rows(torch, msgs), sym_stride=200)
    hb = np.zeros((4, 64), np.uint8)
    for i, m in enumerate(msgs):
        hb[i, :len(m)] = m
    hn = np.array([len(m) for m in msgs], np.int32)
    hs, hl = np.full((4, 200), 0xffff, np.uint16), np.zeros(4, np.int32)
    assert lib.lorahip_encode_packets_host(e._ctx._h, C.byref(e._cfg), hb.ctypes.data, 64, hn.ctypes.data, 4, hs.ctypes.data, 200, hl.ctypes.data) == 0
    assert np.array_equal(hs, d_s.cpu().numpy().view(np.uint16)) and np.array_equal(hl, d_n.cpu().numpy())
    assert e.work([]) == []
    assert encoder(L, 8, 0, "4/6", False, False).work([b"", b"abc"])[0] is None


@pytest.mark.parametrize("sf,sync,ampl,padding", [(7, 0x12, 1.0, 1), (11, 0x34, 0.5, 3), (9, 0x8e, 2.0, 2)])
def test_mod_frames_var_matches_loramod_and_the_uniform_kernel(gpu, ref, sf, sync, ampl, padding):
    """lorahip_mod_frames_var: row f within the batched modulator's criterion (test_batched_modulator_matches_loramod: at most 1 float
    ulp, at most 5 % of the samples differing) of the verbatim LoRaMod.cpp frame for the frame's own symbols with padding + max_nsyms
    - nsyms[f]; all-zero rows for negative and oversize counts; bit-identical to lorahip_mod_frames when all counts are equal"""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(sf)
    F, S = 70, 12                                          # more than one wavefront, ragged
    syms = rng.integers(0, 1 << sf, (F, S + 3)).astype(np.uint16)             # loose symbol stride: the kernel reads S of S + 3
    n = rng.integers(1, S + 1, F).astype(np.int32)
    n[0], n[1], n[63], n[64], n[F - 1] = S, 1, 5, -1, S + 1
    n[5], n[6] = -2, 0
    ctx = L.Context(sf)
    dsyms, dn = torch.from_numpy(syms.view(np.int16)).cuda(), torch.from_numpy(n).cuda()
    lib = L.load()
    flen = ctx.mod_frame_len(S, padding)
    iq = torch.full((F, flen + 8), 9.0, dtype=torch.complex64, device="cuda")
    ctx.use_torch_stream()
    assert lib.lorahip_mod_frames_var(ctx._h, C.c_void_p(iq.data_ptr() + 8 * 5), flen + 8, C.c_void_p(dsyms.data_ptr()), S + 3,
                                      C.c_void_p(dn.data_ptr()), F, S, sync, ampl, padding) == 0
    torch.cuda.synchronize()
    got = iq.cpu().numpy()
    assert (got[:, :5] == 9.0).all() and (got[:, -3:] == 9.0).all()           # nothing outside the frames
    got = got[:, 5:-3]
    for f in (64, F - 1, 5):
        assert not got[f].any()                                              # refused / oversize: silence
    worst, differ, total = 0, 0, 0
    for f in (0, 1, 2, 6, 62, 63, 65, F - 2):
        want = ref.mod_frame(sf, syms[f, :n[f]], sync=sync, ampl=ampl, padding=padding + S - n[f]) if n[f] > 0 else None
        if want is None:                                                     # no symbols: preamble, sync, down-chirps, then zeros
            want = ref.mod_frame(sf, syms[f, :1], sync=sync, ampl=ampl, padding=padding + S - 1)
            N = 1 << sf
            body = 14 * N + N // 4
            assert not got[f, body:].any()
            want, mine = want[:body], got[f, :body]
        else:
            mine = got[f]
        assert mine.size == want.size
        a, b = mine.view(np.float32), want.view(np.float32)
        d = ulp_diff(a, b)
        small = np.abs(b) < 1e-6 * ampl
        assert np.abs(a - b)[small].max(initial=0) < 1e-7 * ampl
        worst = max(worst, int(d[~small].max()))
        differ += int((d[~small] > 0).sum())
        total += int((~small).sum())
    print("SF%d: worst %d ulp, %d of %d samples differ" % (sf, worst, differ, total))
    assert worst <= 1, "more than one ulp from the reference modulator: %d" % worst
    assert differ <= 5e-2 * total, "%d of %d samples differ in the last ulp" % (differ, total)
    # equal counts: the uniform kernel's frames, bit for bit (this keeps the two copies of the frame walk in step)
    tight = torch.from_numpy(np.ascontiguousarray(syms[:, :S]).view(np.int16)).cuda()
    uni = ctx.mod_frames(tight, sync=sync, ampl=ampl, padding=padding, lead=3, tail=2)
    var = ctx.mod_frames(tight, sync=sync, ampl=ampl, padding=padding, lead=3, tail=2, nsyms=torch.full((F,), S, dtype=torch.int32, device="cuda"))
    assert uni.shape == var.shape and np.array_equal(uni.cpu().numpy().view(np.uint32), var.cpu().numpy().view(np.uint32))
    # a frame of fewer symbols is the uniform kernel's frame with that much more padding, bit for bit
    k = 4
    short = ctx.mod_frames(torch.from_numpy(np.ascontiguousarray(syms[:, :k]).view(np.int16)).cuda(), sync=sync, ampl=ampl, padding=padding + S - k)
    var = ctx.mod_frames(tight, sync=sync, ampl=ampl, padding=padding, nsyms=torch.full((F,), k, dtype=torch.int32, device="cuda"))
    assert short.shape == var.shape and np.array_equal(short.cpu().numpy().view(np.uint32), var.cpu().numpy().view(np.uint32))
    with pytest.raises(L.LoraHipError):                                       # max_nsyms beyond the symbol rows
        lib_rc = lib.lorahip_mod_frames_var(ctx._h, C.c_void_p(iq.data_ptr()), flen + 8, C.c_void_p(dsyms.data_ptr()), S - 1,
                                            C.c_void_p(dn.data_ptr()), F, S, sync, ampl, padding)
        L._lib.check(lib_rc, "lorahip_mod_frames_var")
    ctx.close()


@pytest.mark.parametrize("sf,cr", [(7, "4/5"), (7, "4/8"), (10, "4/5"), (10, "4/8")])
def test_loopback_from_bytes_with_mixed_lengths(gpu, sf, cr):
    """The whole chain on the device, starting from bytes (the reference's test_loopback, for many channels and lengths at once): 256
    channels, one message of 4..48 random bytes each -> transmit (encoder -> modulator with per-frame counts -> AWGN) -> streaming
    demodulator -> batched decoder (crc check and error check on) == the messages.

    Noise: per-component sigma 0.3 on a unit signal, the level of tests/test_gpu_codec.py's bytes-in-bytes-out chain
    (test_receive_chain_bytes_in_bytes_out), which runs SF7 and 4/5 as this test does. (That file's other loopback runs the
    reference's 'amplitude 4.0' at SF10 with 4/7 and 4/8 only: -15 dB is below what an SF7 symbol of 128 samples can be
    demodulated at, and 4/5 corrects nothing.) Every frame is walked to the longest message's length, so each channel's packet
    ends at the MTU; the explicit header tells the decoder where the message ends."""
    import lora_sdr_amd as L
    torch = gpu
    rng = np.random.default_rng(1000 * sf + int(cr[-1]))
    N, B = 1 << sf, 256
    msgs = [rng.integers(0, 256, int(rng.integers(4, 49))).astype(np.uint8) for _ in range(B)]
    msgs[0], msgs[1] = msgs[0][:4], rng.integers(0, 256, 48).astype(np.uint8)
    ctx = L.Context(sf)
    data, nb = rows(torch, msgs)
    iq, nsyms = L.transmit(data, sf=sf, cr=cr, padding=2, sigma=0.3, seed=11, nbytes=nb, lead=N // 2 + 3, tail=3 * N, ctx=ctx)
    enc = encoder(L, sf, 0, cr, True, True)
    mtu = enc.num_symbols(48)
    assert iq.shape == (B, N // 2 + 3 + ctx.mod_frame_len(mtu, 2) + 3 * N)
    assert nsyms.cpu().tolist() == [enc.num_symbols(len(m)) for m in msgs]
    d = L.LoRaDemod(sf, n_channels=B)
    d.setMTU(mtu)
    d.work(iq)
    pk = sorted(d.packets(), key=lambda p: p[0])
    assert [p[0] for p in pk] == list(range(B))
    dec = L.LoRaDecoder()
    dec.setSpreadFactor(sf); dec.setCodingRate(cr); dec.enableCrcc(True); dec.enableErrorCheck(True)
    out = dec.work([p[2] for p in pk])
    bad = [i for i, (o, m) in enumerate(zip(out, msgs)) if o is None or not np.array_equal(o, m)]
    assert not bad, "channels whose bytes did not come back: %s" % bad[:10]
    assert dec.getDropped() == 0
    # a list of bytes goes the same way, and without noise the symbols come back exactly
    iq2, n2 = L.transmit([bytes(m) for m in msgs[:8]], sf=sf, cr=cr, padding=2, lead=N // 2, tail=3 * N)
    d2 = L.LoRaDemod(sf, n_channels=8)
    d2.setMTU(int(n2.max()))
    d2.work(iq2)
    out2 = dec.work([p[2] for p in sorted(d2.packets(), key=lambda p: p[0])])
    assert len(out2) == 8 and all(o is not None and np.array_equal(o, m) for o, m in zip(out2, msgs[:8]))
    d.close(); d2.close(); ctx.close()
