"""TEST INFRASTRUCTURE ONLY -- the DEFINITION of what a decoder learns from a packet's explicit header and checksum (include/lorahip.h:
struct lorahip_packet_info, rdd = LORAHIP_RDD_FROM_HEADER), restated in numpy / plain Python on the primitives of tests/codec_def.py from
LoRaDecoder.cpp:196-397. No GPU, no library import. tests/test_header_rate_cpu.py pins it to the reference through the oracle.

The header fields of a symbol row: the first 8 symbols, rounded to the symbol size and Gray-coded (:218-222), de-interleaved at 4/8 (the
first block is always that: :228-229, :248), give PPM codewords of which the first five are never whitened (:231, :250 start behind them).
Hamming(8,4)-decoded (LoRaCodes.hpp:222-253) they are  len >> 4, len & 15, flags, ck >> 4, ck & 15  with flags = crc | rate << 1; the
residue is ck ^ headerChecksum(len, flags) (:291). None of this reads the rate the decoder was set to.

`walk` is the whole of work() for one packet, statement by statement, and returns the report beside the outcome:

    length, rdd, hdr_residue   the header's as soon as it is read (:283-291) -- also where the packet is then dropped (:293, :297, :313);
                               without a header data_length, the configured rate and -1
    need_syms                  once :313 is passed: the whole interleaver blocks that hold the codewords :315-361 read (codec_def.decoded_end,
                               codec_def.num_symbols_def), else -1
    crc                        where :367-388 compute the checksum: 1 equal, -1 different; else 0
    fec_error                  the `error` flag at the statement where work() returned
    "not reached" (fewer than 8 symbols, PPM > sf, interleaving off): -1, -1, 0, -1, 0, -1

The reference has no rows, so `walk` knows no out_len = -2: a kernel's decode of such a packet ends behind :313 with need_syms set -- crc 0 and
fec_error the header's, everything else as here.

A configuration is the tuple of tests/codec_edge_inputs.py: (sf, ppm, rdd, crcc, interleaving, error_check, explicit, hdr, data_length);
rdd = -1 reads the packet at the rate its header names (a field of 5..7: any rate -- every one drops it in the header, :293 or :297)."""
import numpy as np

import codec_def as D

RDD_FROM_HEADER = -1
FIELDS = ("length", "rdd", "crc", "hdr_residue", "fec_error", "need_syms")
NOT_REACHED = (-1, -1, 0, -1, 0, -1)


def _bit(v, k):
    return (v >> k) & 1


def hamming84_def(b):
    """LoRaCodes.hpp:222-253 -> (nibble, error)"""
    b = int(b)
    p = ((_bit(b, 0) ^ _bit(b, 1) ^ _bit(b, 2) ^ _bit(b, 4)) | (_bit(b, 1) ^ _bit(b, 2) ^ _bit(b, 3) ^ _bit(b, 5)) << 1 |
         (_bit(b, 0) ^ _bit(b, 1) ^ _bit(b, 3) ^ _bit(b, 6)) << 2 | (_bit(b, 0) ^ _bit(b, 2) ^ _bit(b, 3) ^ _bit(b, 7)) << 3)
    return (b ^ {0xD: 1, 0x7: 2, 0xB: 4, 0xE: 8}.get(p, 0)) & 0xf, p != 0


def hamming74_def(b):
    """LoRaCodes.hpp:278-306"""
    b = int(b)
    p = ((_bit(b, 0) ^ _bit(b, 1) ^ _bit(b, 2) ^ _bit(b, 4)) | (_bit(b, 1) ^ _bit(b, 2) ^ _bit(b, 3) ^ _bit(b, 5)) << 1 |
         (_bit(b, 0) ^ _bit(b, 1) ^ _bit(b, 3) ^ _bit(b, 6)) << 2)
    return (b ^ {0x5: 1, 0x7: 2, 0x3: 4, 0x6: 8}.get(p, 0)) & 0xf, p != 0


def nibble_def(b, rdd):
    """one payload codeword at rate rdd (LoRaDecoder.cpp:322-361) -> (nibble, error)"""
    b = int(b)
    if rdd == 0:
        return b, False                                                                  # (:324, :347: the codeword itself)
    if rdd == 1:                                                                         # LoRaCodes.hpp:312-317
        x = b ^ (b >> 2)
        x = x ^ (x >> 1) ^ (b >> 4)
        return b & 0xf, bool(x & 1)
    if rdd == 2:                                                                         # :329-337
        x = b ^ (b >> 1) ^ (b >> 2)
        y = x ^ b ^ (b >> 3)
        return b & 0xf, bool(((x ^ (b >> 4)) | (y ^ (b >> 5))) & 1)
    return hamming74_def(b) if rdd == 3 else hamming84_def(b)


def gray_rounded(symbols, sf, ppm):
    """LoRaDecoder.cpp:218-222 in uint16 arithmetic: + half a step, shift to PPM bits, binary -> Gray"""
    s = np.asarray(symbols).astype(np.uint16)
    s = ((s + np.uint16((1 << (sf - ppm)) // 2)).astype(np.uint16) >> (sf - ppm)).astype(np.uint16)
    return s ^ (s >> 1)


def header_fields(rows, sf, ppm):
    """(..., n >= 8) symbol rows -> arrays (length, flags, residue, error): the decoded header of each row and whether any of its five
    codewords had a non-zero syndrome"""
    P = ppm or sf
    rows = np.asarray(rows)
    cw = D.deinterleave_def(gray_rounded(rows[..., :D.N_HDR_SYMBOLS], sf, P), P, 4 + D.HDR_RDD)[..., :D.N_HDR_CODEWORDS]
    table = np.array([hamming84_def(b) for b in range(256)])
    nib, err = table[cw, 0].astype(np.uint8), table[cw, 1].astype(bool)
    length = (nib[..., 0] << 4) | nib[..., 1]
    flags = nib[..., 2]
    ck = (nib[..., 3] << 4) | nib[..., 4]
    return length, flags, ck ^ D.header_checksum_def(length, flags), err.any(axis=-1)


def header_rate(rows, sf, ppm):
    """the rate field 0..7 of each row: r of include/lorahip.h"""
    return (header_fields(rows, sf, ppm)[1] >> 1) & 7


def walk(symbols, cfg, nsyms=None):
    """-> (out: uint8 bytes / uint16 symbols / None, dropped, report tuple in the order of FIELDS). `symbols` is what the row holds of a
    packet of nsyms symbols (zeros behind it, as the kernels read a packet longer than its row)."""
    sf, ppm, rdd, crcc, inter, ec, explicit, hdr, dlen = cfg
    P = ppm or sf
    symbols = np.asarray(symbols, np.uint16).reshape(-1)
    n = symbols.size if nsyms is None else int(nsyms)
    if P > sf or n < D.N_HDR_SYMBOLS:                                                    # :202, :208
        return None, 0, NOT_REACHED
    if rdd == RDD_FROM_HEADER:
        assert explicit and inter
        rdd = int(header_rate(symbols, sf, P))
        rdd = rdd if rdd <= 4 else D.HDR_RDD
    bs = 4 + rdd
    num_sym = -(-n // bs) * bs                                                           # :210
    num_cw = num_sym // bs * P
    g = gray_rounded(np.concatenate([symbols[:n], np.zeros(num_sym - min(n, symbols.size), np.uint16)]), sf, P)
    if not inter:                                                                        # :264-270
        return g, 0, NOT_REACHED
    cw = np.zeros(num_cw, np.uint8)
    n_hdr = D.N_HDR_CODEWORDS if explicit else 0
    if rdd != D.HDR_RDD:                                                                 # :228-246
        cw[:P] = D.deinterleave_def(g[:8], P, 8)
        whole = (num_sym - 8) // bs
        if whole:
            cw[P:P + whole * P] = D.deinterleave_def(g[8:8 + whole * bs], P, bs)
        white_rest = num_sym - 8 > 0
    else:                                                                                # :248-254
        cw[:] = D.deinterleave_def(g, P, 8)
        white_rest = True
    pos = np.arange(num_cw) - n_hdr                                                      # position in the whitening sequence
    first = np.arange(num_cw) < P
    w4, wr = D.whitening_def(False, num_cw // 2 + 1), D.whitening_def(rdd == 1, num_cw // 2 + 1)
    mask = np.where(first, w4[pos & 1, np.maximum(pos, 0) >> 1], wr[pos & 1, np.maximum(pos, 0) >> 1] & (0xff >> (4 - rdd))).astype(np.uint8)
    mask[pos < 0] = 0
    if not white_rest:
        mask[~first] = 0
    cw = np.concatenate([cw ^ mask, np.zeros(4, np.uint8)])                              # (the odd nibble of a one-block packet is read past the end: 0 here)

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
        n1, e1 = hamming84_def(cw[1]); n0, e0 = hamming84_def(cw[0]); n2, e2 = hamming84_def(cw[2])
        n4, e4 = hamming84_def(cw[4]); n3, e3 = hamming84_def(cw[3])
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
        nib, e = hamming84_def(cw[c_ofs]); error = error or e
        by[d_ofs >> 1] = by[d_ofs >> 1] | nib << 4 if d_ofs & 1 else nib
        c_ofs += 1; d_ofs += 1
    if d_ofs & 1:                                                                        # :322-339
        nib, e = nibble_def(cw[c_ofs], rdd_body); error = error or e
        by[d_ofs >> 1] |= nib << 4
        c_ofs += 1; d_ofs += 1
    d_ofs >>= 1
    if error and ec:                                                                     # :342
        return None, 1, report()
    for i in range(d_ofs, data_length):                                                  # :346-361
        lo, e = nibble_def(cw[c_ofs], rdd_body); error = error or e
        hi, e = nibble_def(cw[c_ofs + 1], rdd_body); error = error or e
        by[i] = (lo & 0xf) | (hi << 4) & 0xff
        c_ofs += 2
    assert c_ofs == c_end or data_length <= d_ofs
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


def report_rows(rows, nsyms, cfgs, index):
    """(P, 8) int32: struct lorahip_packet_info of every row under cfgs[index[p]] (an index without an entry: not reached)"""
    out = np.zeros((len(rows), 8), np.int32)
    for p, (row, n, i) in enumerate(zip(rows, nsyms, index)):
        out[p, :6] = walk(row[:min(int(n), len(row))], cfgs[i], n)[2] if 0 <= i < len(cfgs) else NOT_REACHED
    return out
