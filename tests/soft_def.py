"""TEST INFRASTRUCTURE ONLY -- the DEFINITIONS of the soft-decision receive path (include/lorahip.h: lorahip_soft_symbols,
lorahip_decode_packets_soft), restated in numpy on the primitives of tests/codec_def.py and tests/codec_hdr_def.py. No GPU, no library import.

`llr_def`: per window, P[k] = re*re + im*im in float32; g(k) = gray(uint16((k + half) >> (sf - ppm))) & (2^ppm - 1), the decoder's own
mapping of a bin to the bits it reads (LoRaDecoder.cpp:218-222); llr[m] = max{P[k]: bit m of g(k) = 1} - max{P[k]: bit m of g(k) = 0},
each maximum starting at 0 and admitting a bin only by P[k] > max (class_max): a NaN P[k] never enters, +Inf does, no admitted bin is +0.0.

`decode_soft_def`: codec_hdr_def.walk, statement for statement, with a symbol replaced by its PPM LLRs (hard bit: llr > 0):
    - symbols behind the row or behind nsyms are all-zero LLRs (walk: zero symbols); bits a block does not carry are 0;
    - the hard codeword is the hard bits de-interleaved, XOR the whitening bits -- walk's own `cw` -- and feeds the `error` flag only;
    - the LLRs of a codeword are de-interleaved alike, a whitening bit of 1 negates;
    - every nibble is soft_nibble(L, rate): the x in 0..15 maximising M(x) = sum over k = 0..3+rate ascending of (bit k of fec_def(x, rate) ?
      +L[k] : -L[k]), accumulated in float32 from 0 in that order, the smallest x among equals -- as a loop: x = 0 is the incumbent and
      x > 0 replaces it only by M(x) > M(incumbent), so a NaN M(x) never wins and a NaN M(0) is never replaced;
    - rdd = -1 reads the rate field from the soft nibble of codeword 2.
Like walk it knows no out_len = -2."""
import numpy as np

import codec_def as D
import codec_hdr_def as H

_CODE = dict((r, np.array([int(D.fec_def(x, r)) for x in range(16)], np.uint32)) for r in range(5))


def gray_map(sf, ppm):
    """(N,) g(k): the ppm bits the de-interleaver reads from a symbol whose peak is bin k"""
    k = np.arange(1 << sf, dtype=np.uint32)
    v = ((k + np.uint32((1 << (sf - ppm)) // 2)) >> np.uint32(sf - ppm)) & np.uint32(0xffff)
    return (v ^ (v >> np.uint32(1))) & np.uint32((1 << ppm) - 1)


def power_def(bins):
    b = np.asarray(bins, np.complex64)
    re, im = b.real.astype(np.float32), b.imag.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (re * re + im * im).astype(np.float32)


def class_max(P):
    """(W, n) -> (W,): the maximum that starts at 0 and admits a value only by `value > max` -- NaN never enters, +Inf does, and a row
    (or a class: n = 0) without an admitted value is +0.0. fmax returns the operand that is not NaN, so from 0 it is that maximum."""
    return np.fmax.reduce(np.asarray(P, np.float32), axis=1, initial=np.float32(0)).astype(np.float32)


def llr_def(bins, sf, ppm):
    """(W, N) complex64 bins -> (W, ppm) float32"""
    ppm = ppm or sf
    P = power_def(bins).reshape(-1, 1 << sf)
    g = gray_map(sf, ppm)
    out = np.zeros((P.shape[0], ppm), np.float32)
    with np.errstate(invalid="ignore"):                                                  # (Inf - Inf is a result here, not an accident)
        for m in range(ppm):
            one = ((g >> np.uint32(m)) & np.uint32(1)).astype(bool)
            out[:, m] = class_max(P[:, one]) - class_max(P[:, ~one])
    return out


def llr_of_symbols(symbols, sf, ppm, mag=1.0):
    """rows of +mag / -mag LLRs that spell the Gray-coded, rounded value of each symbol: (..., n) -> (..., n, ppm) float32"""
    ppm = ppm or sf
    g = H.gray_rounded(symbols, sf, ppm).astype(np.uint32)
    bits = (g[..., None] >> np.arange(ppm, dtype=np.uint32)) & np.uint32(1)
    return np.where(bits != 0, np.float32(mag), np.float32(-mag)).astype(np.float32)


def soft_nibble(L, rate):
    """the maximum-likelihood nibble of a codeword's LLRs L[0..7] at coding rate `rate` (n = 4 + rate bits)"""
    L = np.asarray(L, np.float32)
    M = np.zeros(16, np.float32)
    code = _CODE[rate]
    with np.errstate(invalid="ignore"):
        for k in range(4 + rate):
            M = (M + np.where((code >> np.uint32(k)) & np.uint32(1), L[k], -L[k]).astype(np.float32)).astype(np.float32)
    best = 0                                                                             # x = 0 is the incumbent ...
    for x in range(1, 16):
        if M[x] > M[best]:                                                               # ... replaced only by a greater metric: the smallest x
            best = x                                                                     # among equals; a NaN never wins, a NaN M(0) stays
    return best


def decode_soft_def(llr, cfg, nsyms=None):
    """-> (out uint8 bytes / None, dropped, report tuple in the order of codec_hdr_def.FIELDS). `llr` is what the row holds of a packet of
    nsyms symbols: (rows, PPM) float32."""
    sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = cfg
    P = ppm or sf
    llr = np.asarray(llr, np.float32).reshape(-1, P)
    n = llr.shape[0] if nsyms is None else int(nsyms)
    if P > sf or n < D.N_HDR_SYMBOLS:                                                    # :202, :208
        return None, 0, H.NOT_REACHED
    assert inter, "the soft decoder has no symbol output"
    row = min(n, llr.shape[0])

    def gather(sym_off, width, i):
        L = np.zeros(8, np.float32)
        for k in range(width):
            if sym_off + k < row:
                L[k] = llr[sym_off + k, (i - k) % P]
        return L

    if rdd == H.RDD_FROM_HEADER:
        assert explicit
        rdd = (soft_nibble(gather(0, 8, 2), D.HDR_RDD) >> 1) & 7
        rdd = rdd if rdd <= 4 else D.HDR_RDD
    bs = 4 + rdd
    num_sym = -(-n // bs) * bs                                                           # :210
    num_cw = num_sym // bs * P
    Lcw = np.zeros((num_cw + 4, 8), np.float32)
    n_hdr = D.N_HDR_CODEWORDS if explicit else 0
    if rdd != D.HDR_RDD:                                                                 # :228-246
        for i in range(P):
            Lcw[i] = gather(0, 8, i)
        for x in range((num_sym - 8) // bs):
            for i in range(P):
                Lcw[P + x * P + i] = gather(8 + x * bs, bs, i)
        white_rest = num_sym - 8 > 0
    else:                                                                                # :248-254
        for x in range(num_sym // 8):
            for i in range(P):
                Lcw[x * P + i] = gather(8 * x, 8, i)
        white_rest = True
    pos = np.arange(num_cw) - n_hdr
    first = np.arange(num_cw) < P
    w4, wr = D.whitening_def(False, num_cw // 2 + 1), D.whitening_def(rdd == 1, num_cw // 2 + 1)
    mask = np.where(first, w4[pos & 1, np.maximum(pos, 0) >> 1], wr[pos & 1, np.maximum(pos, 0) >> 1] & (0xff >> (4 - rdd))).astype(np.uint8)
    mask[pos < 0] = 0
    if not white_rest:
        mask[~first] = 0
    mask = np.concatenate([mask, np.zeros(4, np.uint8)])
    hard = ((Lcw > 0).astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(axis=1).astype(np.uint8) ^ mask
    mbits = ((mask[:, None] >> np.arange(8, dtype=np.uint8)) & 1).astype(bool)
    Lw = np.where(mbits, -Lcw, Lcw).astype(np.float32)

    def dec84(c):
        return soft_nibble(Lw[c], D.HDR_RDD), H.hamming84_def(hard[c])[1]

    def dec(c, rate):
        return soft_nibble(Lw[c], rate), H.nibble_def(hard[c], rate)[1]

    error = False
    nbytes = (num_cw + 1) // 2
    by = [0] * (nbytes + 8)
    length = rate = res = need = -1
    crc_state = 0
    check_crc = bool(crcc)
    c_ofs = d_ofs = 0

    def report():
        return (length, rate, crc_state, res, int(error), need)

    if explicit:                                                                         # :283-303
        (n1, e1), (n0, e0), (n2, e2), (n4, e4), (n3, e3) = dec84(1), dec84(0), dec84(2), dec84(4), dec84(3)
        error = e0 or e1 or e2 or e3 or e4
        by[0], by[1], by[2] = n1 | n0 << 4, n2, n4 | n3 << 4
        by[2] ^= int(D.header_checksum_def(by[0], by[1]))
        length, rate, res = by[0], (by[1] >> 1) & 7, by[2]
        if error and ec:
            return None, 1, report()
        if not by[1] & 1:
            check_crc = False
        if rate > 4:
            return None, 1, report()
        rdd_body = rate
        packet_length = by[0]
        data_length = packet_length + (5 if by[1] & 1 else 3)
        c_ofs, d_ofs = D.N_HDR_CODEWORDS, 6
    else:                                                                                # :304-311
        packet_length = dlen
        data_length = packet_length + 2 if crcc else packet_length
        length, rate, rdd_body = dlen, rdd, rdd
    if data_length > nbytes:                                                             # :313
        return None, 1, report()
    c_end, _ = D.decoded_end(P, bool(explicit), data_length)
    need = D.num_symbols_def(-(-c_end // P) * P, P, rdd)
    while c_ofs < P:                                                                     # :315-320
        nib, e = dec84(c_ofs); error = error or e
        by[d_ofs >> 1] = by[d_ofs >> 1] | nib << 4 if d_ofs & 1 else nib
        c_ofs += 1; d_ofs += 1
    if d_ofs & 1:                                                                        # :322-339
        nib, e = dec(c_ofs, rdd_body); error = error or e
        by[d_ofs >> 1] |= nib << 4
        c_ofs += 1; d_ofs += 1
    d_ofs >>= 1
    if error and ec:                                                                     # :342
        return None, 1, report()
    for i in range(d_ofs, data_length):                                                  # :346-361
        lo, e = dec(c_ofs, rdd_body); error = error or e
        hi, e = dec(c_ofs + 1, rdd_body); error = error or e
        by[i] = (lo & 0xf) | (hi << 4) & 0xff
        c_ofs += 2
    if error and ec:                                                                     # :363
        return None, 1, report()
    d_ofs = 0
    if explicit:                                                                         # :367-379
        if by[1] & 1:
            crc = D.data_checksum_def(np.array(by[3:3 + packet_length], np.uint8))
            crc_state = 1 if crc == (by[3 + packet_length] | by[4 + packet_length] << 8) else -1
            if crc_state < 0 and check_crc:
                return None, 1, report()
            by[3 + packet_length] ^= crc & 0xff
            by[4 + packet_length] ^= crc >> 8
        if not hdr:
            d_ofs = 3
            data_length -= 5
    elif check_crc:                                                                      # :380-388
        crc = D.data_checksum_def(np.array(by[:dlen], np.uint8))
        crc_state = 1 if crc == (by[dlen] | by[dlen + 1] << 8) else -1
        if crc_state < 0:
            return None, 1, report()
        by[dlen] ^= crc & 0xff
        by[dlen + 1] ^= crc >> 8
    if data_length < 0:                                                                  # (a size_t that wrapped: the reference posts nothing)
        return None, 0, report()
    return np.array(by[d_ofs:d_ofs + data_length], np.uint8), 0, report()
